"""Timing and peak device memory of a probabilistic verification of ensembles against station reports: 256 stations x 25 hourly leads = 6 400
points, the products T, speed, u, p with three thresholds, pooled per station, per lead hour and over everything, at (cases, members) = (8, 8) and
(8, 61) (the lead times of one epoch of SyntheticSamples stand in for the members, dealt out over the cases; the reports are the first member plus
noise, a tenth of them missing).

  fused     InterfacePhysics.verify_ensemble_at: per member the encoder, the heads, the packing, the fields-only forward and dpn_pverify_stage into
            planes that stay on the device, per case dpn_pverify_case into the resident state, then dpn_pverify_pool per grouping and
            dpn_pverify_finish.
  composed  what the product replaces: C x M predict_points calls (and dpn_fields_out on the sampler's coord_data for the baseline), torch.stack
            over members and cases, torch.sort over the members, a NaN mask, masked torch reductions in fp64 per point (CRPS from the sorted
            closed form, mean error, spread, the rank, the number of event members), and index_add_ of the sufficient statistics, histograms and
            reliability tables per grouping.

Both routes are timed alternately in one process, `--reps` times after one warm-up each; peak memory is torch's max_memory_allocated during one run of a
route, above what was allocated before it.  The composed route's index_add_ is an atomic sum: its pooled bits may change from run to run, which the
tool reports (`composed_pooled_runs_differ`) next to whether two fused runs give the same bits.  Writes the numbers as JSON (default
profiles/prob_verify_time.json).

usage: python tools/prob_verify_time.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ensemble_time import _peak, _timed
from tools.verify_time import HOURS, PRODUCTS, STATIONS, _baseline, _values, table_digests

SIZES = ((8, 8), (8, 61))                                       # (cases, members)


def composed(m, cases, xi, yi, hr, thresholds, by):
    """The scores from C x M single-member results: stack, sort, mask, masked fp64 reductions, index_add_ pooling."""
    M = len(cases[0]['members'])
    sides = []
    for rows_of in (lambda c: _values(m.predict_points(c['field_data'], c['sampler'], xi, yi, hr, c['forecast_h'])),
                    lambda c: _values(_baseline(m, c['sampler'], xi, yi, hr))):
        sides.append(torch.stack([torch.stack([rows_of(mem) for mem in case['members']]) for case in cases]).double())      # [C, M, N, P]
    O = torch.stack([case['obs'] for case in cases]).double()                                                                # [C, N, P]
    ok = torch.isfinite(O) & torch.isfinite(sides[0]).all(dim=1) & torch.isfinite(sides[1]).all(dim=1)
    zero = torch.zeros((), dtype=torch.float64, device=O.device)
    O = torch.where(ok, O, zero)
    w = (2.0 * torch.arange(M, dtype=torch.float64, device=O.device) - M + 1.0).view(1, M, 1, 1)
    levels = torch.arange(M + 1, device=O.device)
    stats = {'n': ok.double().sum(0)}
    for pre, X in zip(('', 'base_'), sides):
        X = torch.where(ok[:, None], X, zero)
        srt = torch.sort(X, dim=1).values
        a, g = (X - O[:, None]).abs().mean(1), (srt * w).sum(1)
        mean = X.mean(1)
        d = mean - O
        var = X.var(1, unbiased=True) if M > 1 else torch.zeros_like(d)
        per_pair = dict(sum_crps=a - g / (M * M), sum_fair=a - g / (M * (M - 1)) if M > 1 else a, sum_d=d, sum_d2=d * d, sum_var=var)
        for key, v in per_pair.items():
            stats[pre + key] = torch.where(ok, v, zero).sum(0)
        rank = (X < O[:, None]).sum(1) + (X == O[:, None]).sum(1) // 2
        stats[pre + 'rank'] = ((rank[..., None] == levels) & ok[..., None]).double().sum(0)                                 # [N, P, M + 1]
        for k, (name, side, value) in enumerate(thresholds):
            j = PRODUCTS.index(name)
            ev = (lambda z: z > value) if side == 'above' else (lambda z: z < value)
            cnt, eo, sel = ev(X[:, :, :, j]).sum(1), ev(O[:, :, j]), ok[:, :, j]
            at = (cnt[..., None] == levels) & sel[..., None]
            stats['%srel_n%d' % (pre, k)], stats['%srel_o%d' % (pre, k)] = at.double().sum(0), (at & eo[..., None]).double().sum(0)         # [N, M + 1]

    def scores(s):
        n = s['n']
        out = dict(count=n)
        p = (levels.double() / M)
        for pre in ('', 'base_'):
            out.update({pre + 'crps': s[pre + 'sum_crps'] / n, pre + 'fair_crps': s[pre + 'sum_fair'] / n, pre + 'bias': s[pre + 'sum_d'] / n,
                        pre + 'rmse': (s[pre + 'sum_d2'] / n).sqrt(), pre + 'spread': (s[pre + 'sum_var'] / n).sqrt(), pre + 'rank_hist': s[pre + 'rank']})
            for k, (name, _, _) in enumerate(thresholds):
                nk, okk = s['%srel_n%d' % (pre, k)], s['%srel_o%d' % (pre, k)]
                out['%sbrier%d' % (pre, k)] = (okk * (1.0 - p) ** 2 + (nk - okk) * p ** 2).sum(-1) / n[:, PRODUCTS.index(name)]
        out['crpss'] = 1.0 - s['sum_crps'] / s['base_sum_crps']
        return out
    out = {'point': scores(stats)}
    for name, ids in by.items():
        G = int(ids.max()) + 1
        pooled = {key: torch.zeros((G,) + tuple(v.shape[1:]), dtype=torch.float64, device=v.device).index_add_(0, ids, v) for key, v in stats.items()}
        out[name] = scores(pooled)
    return out


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prob_verify_time.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('prob_verify_time: no GPU; nothing is measured without one')
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
    everyone = [dict(field_data=syn[i]['field_data'], forecast_h=syn[i]['forecast_h'], sampler=s) for i in range(61)]
    result = {'products': PRODUCTS, 'points': N, 'stations': STATIONS, 'hours': HOURS, 'groupings': list(by_host), 'reps': args.reps,
              'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for C, M in SIZES:
        cases = []
        for c in range(C):
            members = [everyone[(7 * c + k) % 61] for k in range(M)]
            x = _values(m.predict_points(members[0]['field_data'], s, xi, yi, hr, members[0]['forecast_h']))
            noise = torch.randn(x.shape, device=dev) * x.std(dim=0, keepdim=True) * 0.5
            cases.append(dict(members=members, obs=torch.where(torch.rand(x.shape, device=dev) < 0.1, torch.full_like(x, float('nan')), x + noise).contiguous()))
        first = torch.stack([c['obs'] for c in cases])
        thr_in = {'T': [('below', float(first[..., 0].nanmedian())), float(first[..., 0].nanquantile(0.75))], 'speed': float(first[..., 1].nanmedian())}
        fused = lambda: m.verify_ensemble_at(cases, xi, yi, hr, PRODUCTS, thresholds=thr_in, by=by_host)
        a = fused()
        print('\n'.join('sha256 cases_%d_members_%d %s' % (C, M, line) for line in table_digests(a)))
        comp = lambda: composed(m, cases, xi, yi, hr, a['thresholds'], by_dev)
        b = comp()
        differ, ranks_equal = {}, True
        for key in ('point', 'station', 'hour', 'all'):
            for score in ('crps', 'fair_crps', 'bias', 'rmse', 'spread', 'base_crps', 'crpss'):
                x, y = a[key][score].double(), b[key][score]
                both = torch.isfinite(x) & torch.isfinite(y)
                differ['%s_%s' % (key, score)] = float(((x - y)[both].abs() / y[both].abs().clamp_min(1e-300)).max())
            differ['%s_brier' % key] = float(max(((a[key]['brier'][:, k].double() - b[key]['brier%d' % k]).abs() / b[key]['brier%d' % k].abs().clamp_min(1e-300))
                                                 [torch.isfinite(b[key]['brier%d' % k])].max() for k in range(3)))
            ranks_equal &= torch.equal(a[key]['rank_hist'].double(), b[key]['rank_hist'])
        again, runs_differ = fused(), False
        same_bits = all(torch.equal(a[key][k].view(torch.int32), again[key][k].view(torch.int32)) for key in ('point', 'station', 'hour', 'all')
                        for k in a[key] if a[key][k] is not None)
        for _ in range(3):
            c2 = comp()
            runs_differ |= any(not torch.equal(b[key][k].view(torch.int64), c2[key][k].view(torch.int64)) for key in ('station', 'hour', 'all')
                               for k in ('crps', 'bias', 'rmse', 'spread'))
        del b, again, c2
        routes = [('fused', fused), ('composed', comp)]
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):                              # alternated: every route sees the same state of the box
            for name, fn in routes:
                times[name].append(_timed(fn)[0])
        row = {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for name, v in times.items()}
        for name, fn in routes:
            row[name]['peak_mib'] = _peak(fn) / 2.0 ** 20
        row.update(cases=C, members=M, worst_relative_difference=differ, rank_histograms_equal=bool(ranks_equal), fused_two_runs_same_bits=bool(same_bits),
                   composed_pooled_runs_differ=bool(runs_differ), composed_over_fused=row['composed']['median_ms'] / row['fused']['median_ms'])
        result['sizes']['cases_%d_members_%d' % (C, M)] = row
        print('%d points, %d cases of %d members (largest relative difference of a score: %.3e; fused runs same bits: %s; composed pooled runs differ: %s):'
              % (N, C, M, max(differ.values()), same_bits, runs_differ))
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
