"""Timing and peak device memory of regional statistics: 100 regions that cover about 60 % of the full fine grid (257 x 145) at one hour and at all
25 hours of a sample (931 625 lattice points, 559 000 of them inside a region), and 256 stations in 8 groups at 25 hours; hi+lo mode, eager launches,
two routes alternated in the same process, a host clock around work that ends in a device synchronise, median and spread of the timed repetitions:

  regional  InterfacePhysics.regional_lattice / regional_at: the plan on the host, encoder, heads and packing once, then per chunk dpn_sample_at ->
            forward -> dpn_region_accumulate over the points inside a region only, and one dpn_region_finish.
  composed  what a user could write before: diagnostic_lattice (vorticity, speed) and predict_lattice (T) build the maps [nt, P, ny, nx] of every
            point, then torch reduces them: index_add_ for the weighted sums, the weights and the weights above the thresholds (float atomics: two
            runs need not agree), scatter_reduce_ amin / amax for the extremes.  It finds no positions of the extremes; the regional route does.

Products: vorticity, speed, T; area weights; thresholds: speed above 0.5, T above 280.  Both routes run once for warm-up and their means are compared
(reported, not assumed).  Peak memory is torch.cuda.max_memory_allocated over one run of a route, above what was allocated before it.  Writes the
numbers as JSON (default profiles/regions_time.json).

usage: python tools/regions_time.py [--reps 5] [--out FILE]"""
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

PRODUCTS = ['vorticity', 'speed', 'T']
THRESHOLDS = {'speed': [0.5], 'T': [280.0]}


def labels(ny, nx):
    """100 regions (a 10 x 10 board) over three fifths of the plane; the rest, two diagonals out of five, is in no region."""
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    lab = (iy * 10 // ny) * 10 + ix * 10 // nx
    lab[(ix + iy) % 5 < 2] = -1
    return lab.astype(np.int64)


def composed(values, lab, w, R):
    """values [nt, P, n] (P in PRODUCTS' order), lab [n] int64 (-1: none), w [n] -> mean, min, max [nt, R, P] and frac [nt, R, 2] by torch reductions."""
    nt, P, _ = values.shape
    inside = lab >= 0
    idx, wi, v = lab[inside], w[inside].double(), values[:, :, inside]
    ok = torch.isfinite(v)
    wv = torch.where(ok, wi, torch.zeros_like(wi))                            # [nt, P, n_sel]: a point that is not finite does not count
    W = torch.zeros((nt, P, R), dtype=torch.float64, device=v.device).index_add_(2, idx, wv)
    WX = torch.zeros_like(W).index_add_(2, idx, wv * torch.where(ok, v, torch.zeros_like(v)).double())
    big = torch.full((nt, P, R), float('inf'), device=v.device)
    where = idx.expand(nt, P, -1)
    lo = big.clone().scatter_reduce_(2, where, torch.where(ok, v, big[..., :1].expand_as(v)), 'amin')
    hi = (-big).scatter_reduce_(2, where, torch.where(ok, v, -big[..., :1].expand_as(v)), 'amax')
    frac = []
    for name, (t,) in THRESHOLDS.items():
        p = PRODUCTS.index(name)
        above = torch.zeros((nt, R), dtype=torch.float64, device=v.device).index_add_(1, idx, wv[:, p] * (v[:, p] > t))
        frac.append(above / W[:, p])
    return dict(mean=(WX / W).float().permute(0, 2, 1), min=lo.permute(0, 2, 1), max=hi.permute(0, 2, 1), frac=torch.stack(frac, dim=-1).float())


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.regions import area_weights, row_latitudes
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regions_time.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('regions_time: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    scaled_init_(m.physics_net, seed=1)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=1)
    s, smp = syn.sampler, syn[0]
    field, fh = smp['field_data'], smp['forecast_h']
    lab = labels(145, 257)
    lab_dev = torch.from_numpy(lab.reshape(-1)).to(dev)
    w_dev = torch.from_numpy(np.repeat(area_weights(row_latitudes(s.cfg, np.arange(145)))[:, None], 257, axis=1).reshape(-1)).to(dev)
    g = np.random.default_rng(256)
    xi, yi, groups = g.random(256) * 256.0, g.random(256) * 144.0, g.integers(0, 8, size=256)
    hours = np.arange(25.0)
    gw_dev = torch.from_numpy(area_weights(row_latitudes(s.cfg, yi))).to(dev)
    groups_dev = torch.from_numpy(groups).to(dev)
    result = {'products': PRODUCTS, 'thresholds': THRESHOLDS, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
              'regions': 100, 'share_of_the_plane_inside_a_region': float((lab >= 0).mean()), 'sizes': {}}

    def lattice_maps(lat):
        diag = m.diagnostic_lattice(field, s, lat, fh, PRODUCTS[:2])
        var = m.predict_lattice(field, s, lat, fh)
        return torch.cat([diag, var[:, 3:4]], dim=1).reshape(lat.nt, 3, -1)

    def station_rows():
        x, y, t = np.tile(xi, 25), np.tile(yi, 25), np.repeat(hours, 256)
        diag = m.diagnostics_at(field, s, x, y, t, fh, PRODUCTS[:2])
        var = m.predict_points(field, s, x, y, t, fh)
        return torch.cat([diag, var[:, 3:4]], dim=1).view(25, 256, 3).permute(0, 2, 1)

    shapes = [('lattice_1h', s.lattice(refine=1, hours=12.0)), ('lattice_25h', s.lattice(refine=1, hours=(0.0, 1.0, 25))), ('stations_25h', None)]
    for where, lat in shapes:
        if lat is not None:
            routes = [('regional', lambda: m.regional_lattice(field, s, lat, fh, lab, PRODUCTS, weights='area', thresholds=THRESHOLDS)),
                      ('composed', lambda: composed(lattice_maps(lat), lab_dev, w_dev, 100))]
            points, evaluated = lat.n_points, lat.nt * int((lab >= 0).sum())
        else:
            routes = [('regional', lambda: m.regional_at(field, s, xi, yi, hours, fh, groups, PRODUCTS, weights='area', thresholds=THRESHOLDS)),
                      ('composed', lambda: composed(station_rows(), groups_dev, gw_dev, 8))]
            points = evaluated = 25 * 256
        a, b = routes[0][1](), routes[1][1]()
        both = torch.isfinite(a['mean']) & torch.isfinite(b['mean'])
        diff = ((a['mean'] - b['mean'])[both].abs() / b['mean'][both].abs().clamp_min(1e-30)).amax().item()
        same_extremes = bool(torch.equal(a['min'][both], b['min'][both]) and torch.equal(a['max'][both], b['max'][both]))
        del a, b, both
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):                            # alternated: every route sees the same state of the box
            for name, fn in routes:
                times[name].append(_timed(fn)[0])
        row = {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for name, v in times.items()}
        for name, fn in routes:
            row[name]['peak_mib'] = _peak(fn) / 2.0 ** 20
        row.update(points=points, points_evaluated_by_regional=evaluated, max_relative_mean_difference=diff, min_and_max_equal=same_extremes,
                   composed_over_regional=row['composed']['median_ms'] / row['regional']['median_ms'])
        result['sizes'][where] = row
        print('%s, %d points, %d inside a region (means differ by at most %.3e relative; min and max equal: %s):' % (where, points, evaluated, diff,
                                                                                                                   same_extremes))
        for name in times:
            print('  %-9s %9.2f ms (min %.2f .. max %.2f, n = %d)   peak %.1f MiB' % (name, row[name]['median_ms'], row[name]['min_ms'],
                                                                                     row[name]['max_ms'], args.reps, row[name]['peak_mib']))
        print('  composed / regional = %.2f' % row['composed_over_regional'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fobj:
        json.dump(result, fobj, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
