"""Timing and peak device memory of a forecast verification against station reports: 256 stations x 25 hourly leads = 6 400 points, the products T,
speed, u, p with three thresholds, pooled per station, per lead hour and over everything, over 8 and over 61 forecast dates (the lead times of one
epoch of SyntheticSamples stand in for the dates; the reports are the forecast plus noise, a tenth of them missing).

  fused     InterfacePhysics.verify_at: per date the encoder, the heads, the packing, the fields-only forward and dpn_verify_accumulate into a state
            that stays on the device, then dpn_verify_pool per grouping and dpn_verify_finish.
  composed  what the product replaces: M predict_points calls (and dpn_fields_out on the sampler's coord_data for the baseline), torch.stack over the
            dates, a NaN mask, masked torch reductions in fp64 per point, and index_add_ of the sufficient statistics per grouping.

Both routes are timed alternately in one process, `--reps` times after one warm-up each; peak memory is torch's max_memory_allocated during one run of a
route, above what was allocated before it.  The composed route's index_add_ is an atomic sum: its pooled bits may change from run to run, which the
tool reports (`composed_pooled_runs_differ`).  Writes the numbers as JSON (default profiles/verify_time.json).

usage: python tools/verify_time.py [--reps 5] [--out FILE]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ensemble_time import _peak, _timed

PRODUCTS = ['T', 'speed', 'u', 'p']
COLUMNS = [3, None, 0, 2]                                       # of predict_points' rows; None: speed
STATIONS, HOURS = 256, 25


def _values(rows):
    cols = [torch.sqrt(rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1]) if c is None else rows[:, c] for c in COLUMNS]
    return torch.stack(cols, dim=1)


def table_digests(result):
    """'<table>.<score> <sha256 of the bytes>' of every tensor of every table of a verify_at / verify_ensemble_at result, in the result's order: two
    commits compute the same when these lines are the same."""
    return ['%s.%s %s' % (table, k, hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest())
            for table, rows in result.items() if isinstance(rows, dict) for k, v in rows.items() if v is not None]


def _baseline(m, sampler, xi, yi, hr):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    cd = sampler.at_positions(xi, yi, hr)[3].contiguous()
    rows = torch.empty_like(cd)
    ph = m.point_config().physics()
    L.check(L.load().dpn_fields_out(_ptr(cd), cd.shape[0], ctypes.byref(ph), 0, _ptr(rows), None, None, 0, _stream()), 'dpn_fields_out')
    return rows


def composed(m, cases, xi, yi, hr, thresholds, by):
    """The scores from M single-date results: stack, mask, masked fp64 reductions, index_add_ pooling."""
    X = torch.stack([_values(m.predict_points(c['field_data'], c['sampler'], xi, yi, hr, c['forecast_h'])) for c in cases]).double()
    B = torch.stack([_values(_baseline(m, c['sampler'], xi, yi, hr)) for c in cases]).double()
    O = torch.stack([c['obs'] for c in cases]).double()
    ok = torch.isfinite(X) & torch.isfinite(B) & torch.isfinite(O)
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    X, B, O = (torch.where(ok, v, zero) for v in (X, B, O))
    d, e = X - O, B - O
    stats = dict(n=ok.double().sum(0), sum_d=d.sum(0), sum_ad=d.abs().sum(0), sum_d2=(d * d).sum(0), sum_e=e.sum(0), sum_ae=e.abs().sum(0),
                 sum_e2=(e * e).sum(0), sx=X.sum(0), so=O.sum(0), sxx=(X * X).sum(0), soo=(O * O).sum(0), sxo=(X * O).sum(0),
                 max_ad=d.abs().amax(0))
    for k, (name, side, value) in enumerate(thresholds):
        j = PRODUCTS.index(name)
        ev = (lambda z: z > value) if side == 'above' else (lambda z: z < value)
        for pre, F in (('', X), ('base_', B)):
            f, o = ev(F[:, :, j]) & ok[:, :, j], ev(O[:, :, j]) & ok[:, :, j]
            stats['%shits%d' % (pre, k)], stats['%sfalse%d' % (pre, k)], stats['%smiss%d' % (pre, k)] = \
                (f & o).double().sum(0), (f & ~o & ok[:, :, j]).double().sum(0), (~f & o).double().sum(0)

    def scores(s):
        n = s['n']
        cov, vx, vo = s['sxo'] - s['sx'] * s['so'] / n, s['sxx'] - s['sx'] ** 2 / n, s['soo'] - s['so'] ** 2 / n
        return dict(count=n, bias=s['sum_d'] / n, mae=s['sum_ad'] / n, rmse=(s['sum_d2'] / n).sqrt(), corr=cov / (vx * vo).sqrt(),
                    base_bias=s['sum_e'] / n, base_mae=s['sum_ae'] / n, base_rmse=(s['sum_e2'] / n).sqrt(), skill=1.0 - s['sum_d2'] / s['sum_e2'],
                    pod=[s['hits%d' % k] / (s['hits%d' % k] + s['miss%d' % k]) for k in range(len(thresholds))],
                    base_pod=[s['base_hits%d' % k] / (s['base_hits%d' % k] + s['base_miss%d' % k]) for k in range(len(thresholds))])
    out = {'point': scores(stats)}
    for name, ids in by.items():
        G = int(ids.max()) + 1
        pooled = {}
        for key, v in stats.items():
            if key == 'max_ad':
                continue
            pooled[key] = torch.zeros((G,) + tuple(v.shape[1:]), dtype=torch.float64, device=v.device).index_add_(0, ids, v)
        out[name] = scores(pooled)
    return out


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'verify_time.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('verify_time: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    scaled_init_(m.physics_net, seed=1)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=61)
    s = syn.sampler
    g = np.random.default_rng(256)
    sx, sy = g.random(STATIONS) * 256.0, g.random(STATIONS) * 144.0
    xi, yi, hr = np.tile(sx, HOURS), np.tile(sy, HOURS), np.repeat(np.arange(HOURS, dtype=np.float64) * 24.0 / (HOURS - 1), STATIONS)
    N = xi.size
    by_host = {'station': np.tile(np.arange(STATIONS), HOURS), 'hour': np.repeat(np.arange(HOURS), STATIONS), 'all': np.zeros(N, dtype=np.int64)}
    by_dev = {k: torch.from_numpy(v).to(dev) for k, v in by_host.items()}
    everyone = []
    for i in range(61):
        b = syn[i]
        c = dict(field_data=b['field_data'], forecast_h=b['forecast_h'], sampler=s)
        x = _values(m.predict_points(c['field_data'], s, xi, yi, hr, c['forecast_h']))
        noise = torch.randn(x.shape, device=dev) * x.std(dim=0, keepdim=True) * 0.5
        c['obs'] = torch.where(torch.rand(x.shape, device=dev) < 0.1, torch.full_like(x, float('nan')), x + noise).contiguous()
        everyone.append(c)
    first = torch.stack([c['obs'] for c in everyone[:8]])
    thr_in = {'T': [('below', float(first[..., 0].nanmedian())), float(first[..., 0].nanquantile(0.75))], 'speed': float(first[..., 1].nanmedian())}
    result = {'products': PRODUCTS, 'points': N, 'stations': STATIONS, 'hours': HOURS, 'groupings': list(by_host), 'reps': args.reps,
              'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for M in (8, 61):
        cases = everyone[:M]
        fused = lambda: m.verify_at(cases, xi, yi, hr, PRODUCTS, thresholds=thr_in, by=by_host)
        a = fused()
        print('\n'.join('sha256 dates_%d %s' % (M, line) for line in table_digests(a)))
        comp = lambda: composed(m, cases, xi, yi, hr, a['thresholds'], by_dev)
        b = comp()
        differ = {}
        for key in ('point', 'station', 'hour', 'all'):
            for score in ('bias', 'rmse', 'corr', 'skill'):
                x, y = a[key][score].double(), b[key][score]
                both = torch.isfinite(x) & torch.isfinite(y)
                differ['%s_%s' % (key, score)] = float(((x - y)[both].abs() / y[both].abs().clamp_min(1e-300)).max())
        again, runs_differ = fused(), False
        same_bits = all(torch.equal(a[key][k].view(torch.int32), again[key][k].view(torch.int32)) for key in ('point', 'station', 'hour', 'all')
                        for k in a[key] if a[key][k] is not None)
        for _ in range(3):
            c2 = comp()
            runs_differ |= any(not torch.equal(b[key][k].view(torch.int64), c2[key][k].view(torch.int64)) for key in ('station', 'hour', 'all')
                               for k in ('bias', 'rmse', 'corr'))
        del b, again, c2
        routes = [('fused', fused), ('composed', comp)]
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):                              # alternated: every route sees the same state of the box
            for name, fn in routes:
                times[name].append(_timed(fn)[0])
        row = {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for name, v in times.items()}
        for name, fn in routes:
            row[name]['peak_mib'] = _peak(fn) / 2.0 ** 20
        row.update(dates=M, worst_relative_difference=differ, fused_two_runs_same_bits=bool(same_bits), composed_pooled_runs_differ=bool(runs_differ),
                   composed_over_fused=row['composed']['median_ms'] / row['fused']['median_ms'])
        result['sizes']['dates_%d' % M] = row
        print('%d points, %d dates (largest relative difference of a score: %.3e; fused runs same bits: %s; composed pooled runs differ: %s):'
              % (N, M, max(differ.values()), same_bits, runs_differ))
        for name in times:
            print('  %-9s %9.2f ms (min %.2f .. max %.2f, n = %d)   peak %.1f MiB' % (name, row[name]['median_ms'], row[name]['min_ms'],
                                                                                     row[name]['max_ms'], args.reps, row[name]['peak_mib']))
        print('  composed / fused = %.2f' % row['composed_over_fused'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fobj:
        json.dump(result, fobj, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
