"""Timing and peak device memory of a neighbourhood verification on the full fine grid (257 x 145 nodes) against gridded analyses: the products T,
speed, u, p with three thresholds and the window widths 1, 3, 5, 9, 17, 33, at 25 hourly leads and at one, over 8 and over 61 cases (the lead times
of one epoch of SyntheticSamples stand in for the cases; the analysis is the forecast plus noise, a twentieth of its nodes missing).

  fused     InterfacePhysics.verify_lattice: per case the encoder, the heads, the packing, per chunk dpn_sample_at, the fields-only forward and
            dpn_nbhd_stage into event masks that stay on the device, per case dpn_nbhd_fold (integer summed-area tables, the window pass of all
            scales, the two-level fp64 fold into the resident state), then dpn_nbhd_finish.
  composed  what the product replaces: per case predict_lattice and diagnostic_lattice (and dpn_fields_out on the sampler's coord_data for the
            baseline), comparisons into float planes, and per scale torch.nn.functional.avg_pool2d with divisor_override = 1 over the three event
            planes and the validity plane, the fractions and their squares summed in fp64 by torch.sum.

Both routes are timed alternately in one process, `--reps` times after one warm-up each; peak memory is torch's max_memory_allocated during one run of
a route, above what was allocated before it.  The tool reports whether two runs of each route give the same bits.  Writes the numbers as JSON
(default profiles/neighbourhood_time.json).

usage: python tools/neighbourhood_time.py [--reps 3] [--out FILE] [--sizes 25x8,25x61,1x8,1x61]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ensemble_time import _peak, _timed

PRODUCTS = ['T', 'speed', 'u', 'p']
SCALES = (1, 3, 5, 9, 17, 33)
SUMS = ('sum_fo2', 'sum_f2', 'sum_o2', 'sum_bo2', 'sum_b2')


def _values(maps, speed):
    """[nt, 4, ny, nx] in PRODUCTS' order from maps [nt, 6, ny, nx] and speed [nt, 1, ny, nx]."""
    return torch.cat([maps[:, 3:4], speed, maps[:, 0:1], maps[:, 2:3]], dim=1)


def _baseline(m, sampler, lat):
    """The interpolated coarse forecast on the lattice, de-normalised by dpn_fields_out: [nt, 4, ny, nx] in PRODUCTS' order."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    cd = sampler.sample_at(lat.n_points, lattice=lat)[4].contiguous()
    maps = torch.empty((lat.nt, 6, lat.ny, lat.nx), dtype=torch.float32, device=cd.device)
    ph, c_lat = m.point_config().physics(), lat.c_struct()
    L.check(L.load().dpn_fields_out(_ptr(cd), cd.shape[0], ctypes.byref(ph), 0, None, _ptr(maps), ctypes.byref(c_lat), 0, _stream()), 'dpn_fields_out')
    return _values(maps, (maps[:, 0:1] * maps[:, 0:1] + maps[:, 1:2] * maps[:, 1:2]).sqrt())


def composed(m, cases, lat, thresholds, radius):
    """The five sums [nt, E, K], the windows and the plane totals from per-case maps, comparisons and torch pooling."""
    dev = cases[0]['analysis'].device
    nt, E, K = lat.nt, len(thresholds), len(radius)
    out = {k: torch.zeros((nt, E, K), dtype=torch.float64, device=dev) for k in SUMS}
    out['windows'] = torch.zeros((nt, E, K), dtype=torch.int64, device=dev)
    out.update({k: torch.zeros((nt, E), dtype=torch.int64, device=dev) for k in ('n_valid', 'n_f', 'n_b', 'n_o')})
    for case in cases:
        x = _values(m.predict_lattice(case['field_data'], case['sampler'], lat, case['forecast_h']),
                    m.diagnostic_lattice(case['field_data'], case['sampler'], lat, case['forecast_h'], ['speed']))
        b, o = _baseline(m, case['sampler'], lat), case['analysis']
        ok = torch.isfinite(x) & torch.isfinite(b) & torch.isfinite(o)
        planes = []
        for name, side, value in thresholds:
            j = PRODUCTS.index(name)
            ev = (lambda z: z > value) if side == 'above' else (lambda z: z < value)
            planes.append(torch.stack([(ev(z[:, j]) & ok[:, j]).float() for z in (x, b, o)] + [ok[:, j].float()], dim=1))        # [nt, 4, ny, nx]
        planes = torch.stack(planes, dim=1)                                                                                     # [nt, E, 4, ny, nx]
        for key, q in (('n_f', 0), ('n_b', 1), ('n_o', 2), ('n_valid', 3)):
            out[key] += planes[:, :, q].sum(dim=(2, 3)).long()
        flat = planes.view(nt * E, 4, lat.ny, lat.nx)
        for k, r in enumerate(radius):
            c = F.avg_pool2d(flat, 2 * r + 1, stride=1, padding=r, divisor_override=1).double().view(nt, E, 4, lat.ny, lat.nx)
            on = c[:, :, 3] > 0
            V = torch.where(on, c[:, :, 3], torch.ones_like(c[:, :, 3]))
            Pf, Pb, Po = (torch.where(on, c[:, :, q] / V, torch.zeros_like(V)) for q in (0, 1, 2))
            for key, term in zip(SUMS, ((Pf - Po) ** 2, Pf ** 2, Po ** 2, (Pb - Po) ** 2, Pb ** 2)):
                out[key][:, :, k] += term.sum(dim=(2, 3))
            out['windows'][:, :, k] += on.sum(dim=(2, 3))
    out['fss'] = 1.0 - out['sum_fo2'] / (out['sum_f2'] + out['sum_o2'])
    out['base_fss'] = 1.0 - out['sum_bo2'] / (out['sum_b2'] + out['sum_o2'])
    return out


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.neighbourhood import check_scales
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbourhood_time.json'))
    ap.add_argument('--sizes', default='25x8,25x61,1x8,1x61', help='HOURSxCASES[,...]')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('neighbourhood_time: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    scaled_init_(m.physics_net, seed=1)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=61)
    s = syn.sampler
    everyone = [dict(field_data=syn[i]['field_data'], forecast_h=syn[i]['forecast_h'], sampler=s) for i in range(61)]
    radius = check_scales(SCALES)
    result = {'products': PRODUCTS, 'scales': list(SCALES), 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for size in args.sizes.split(','):
        H, C = (int(v) for v in size.split('x'))
        lat = s.lattice(refine=1, hours=(0.0, 1.0, H) if H > 1 else 12.0)
        cases = []
        for c in range(C):
            mem = everyone[(7 * c) % 61]
            x = _values(m.predict_lattice(mem['field_data'], s, lat, mem['forecast_h']), m.diagnostic_lattice(mem['field_data'], s, lat, mem['forecast_h'], ['speed']))
            noise = torch.randn(x.shape, device=dev) * x.std(dim=(0, 2, 3), keepdim=True) * 0.5
            cases.append(dict(mem, analysis=torch.where(torch.rand(x.shape, device=dev) < 0.05, torch.full_like(x, float('nan')), x + noise).contiguous()))
        first = cases[0]['analysis']
        thr_in = {'T': [('below', float(first[:, 0].nanmedian())), float(first[:, 0].nanquantile(0.75))], 'speed': float(first[:, 1].nanmedian())}
        fused = lambda: m.verify_lattice(cases, lat, PRODUCTS, thr_in, SCALES)
        a = fused()
        comp = lambda: composed(m, cases, lat, a['thresholds'], radius)
        b = comp()
        ints_equal = all(torch.equal(a['hour'][k], b[kk]) for k, kk in (('count', 'n_valid'), ('windows', 'windows')))
        differ = {k: float((a['hour'][k].double() - b[k]).abs()[torch.isfinite(b[k])].max()) for k in ('fss', 'base_fss')}
        again, b2 = fused(), comp()
        same_bits = all(torch.equal(a[g][k].view(torch.int32) if a[g][k].dtype == torch.float32 else a[g][k], again[g][k].view(torch.int32)
                                    if a[g][k].dtype == torch.float32 else again[g][k]) for g in ('hour', 'all') for k in a[g])
        comp_same = all(torch.equal(b[k].view(torch.int64), b2[k].view(torch.int64)) for k in SUMS)
        del b, b2, again
        routes = [('fused', fused), ('composed', comp)]
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):                              # alternated: every route sees the same state of the box
            for name, fn in routes:
                times[name].append(_timed(fn)[0])
        row = {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for name, v in times.items()}
        for name, fn in routes:
            row[name]['peak_mib'] = _peak(fn) / 2.0 ** 20
        row.update(hours=H, cases=C, nodes=lat.n_points, worst_absolute_difference=differ, counts_and_windows_equal=bool(ints_equal),
                   fused_two_runs_same_bits=bool(same_bits), composed_two_runs_same_bits=bool(comp_same),
                   composed_over_fused=row['composed']['median_ms'] / row['fused']['median_ms'])
        result['sizes']['hours_%d_cases_%d' % (H, C)] = row
        print('%d x %d nodes, %d hours, %d cases (largest difference of a score: %.3e; counts and windows equal: %s; fused runs same bits: %s; '
              'composed runs same bits: %s):' % (lat.nx, lat.ny, H, C, max(differ.values()), ints_equal, same_bits, comp_same))
        for name in times:
            print('  %-9s %9.2f ms (min %.2f .. max %.2f, n = %d)   peak %.1f MiB' % (name, row[name]['median_ms'], row[name]['min_ms'],
                                                                                     row[name]['max_ms'], args.reps, row[name]['peak_mib']))
        print('  composed / fused = %.2f' % row['composed_over_fused'], flush=True)
        del cases
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fobj:
        json.dump(result, fobj, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
