"""Timing of a 24 h back-trajectory at 15-minute RK4 steps (96 steps, 384 stages) for 256 and for 16 384 parcels, hi+lo mode, eager launches, through
two routes alternated in the same process, a host clock around work that ends in a device synchronise, median and spread of the timed repetitions:

  fused     InterfacePhysics.trajectories: per stage the fields-only forward and dpn_traj_stage (2 launches), no host synchronisation in the loop.
  composed  what a user could write before, from entry points that predate dpn_traj_stage, kept on the device to its advantage (no host check of the
            positions): per stage CollocationSampler.sample_at (1 launch), PackedField.fields (forward + dpn_fields_out, 2 launches) and the RK4
            update in torch fp64 (the elementwise launches counted below), positions clamped to the domain in place of the parcel status.

Both routes run once for warm-up; the parcels start well inside so that none leaves, and the two end positions are compared (same operations in the
same order: the difference is reported, not assumed).  Writes the numbers as JSON (default profiles/trajectory_time.json).

usage: python tools/trajectory_time.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, STEP_H, START_H = 96, 0.25, 24.0
RK4 = ((1.0, 0.5), (2.0, 0.5), (2.0, 1.0), (1.0, None))                  # (weight, a_next = c_next)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def composed(m, field_data, sampler, xs, ys, forecast_h, tally=None):
    """The same integration from sample_at, PackedField.fields and torch; tally (a list) receives the launches of one stage."""
    dev, n, h = field_data.device, xs.numel(), -STEP_H
    c = sampler.cfg
    pf = m._inference_weights(field_data, forecast_h, n)
    rows = torch.empty((n, 6), dtype=torch.float32, device=dev)
    bufs = tuple(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)) + (torch.empty((n, 6), dtype=torch.float32, device=dev),)
    x0, y0 = xs.clone(), ys.clone()
    xe, ye = x0, y0
    te = torch.full((n,), START_H, dtype=torch.float64, device=dev)
    t0 = START_H
    for _ in range(STEPS):
        accx, accy = torch.zeros_like(x0), torch.zeros_like(y0)
        for w, a in RK4:
            count = 0
            x, y, t, _, cd = sampler.sample_at(n, xe, ye, te, out=bufs)
            pf.fields(x, y, t, cd, False, rows=rows)
            count += 3                                                   # dpn_sample_at, the forward, dpn_fields_out
            kx, ky = rows[:, 0].double() * 3600.0 / c.dx, rows[:, 1].double() * 3600.0 / c.dy
            accx, accy = accx + w * kx, accy + w * ky
            count += 10                                                  # 2 x (cast, mul, div), 2 x (mul, add)
            if a is not None:
                xe, ye = (x0 + (a * h) * kx).clamp_(0.0, c.lon_size - 1.0), (y0 + (a * h) * ky).clamp_(0.0, c.lat_size - 1.0)
                te.fill_(t0 + a * h)
                count += 7                                               # 2 x (mul, add, clamp), fill
            else:
                x0, y0 = (x0 + (h / 6.0) * accx).clamp_(0.0, c.lon_size - 1.0), (y0 + (h / 6.0) * accy).clamp_(0.0, c.lat_size - 1.0)
                xe, ye, t0 = x0, y0, t0 + h
                te.fill_(t0)
                count += 9                                               # 2 x (mul, add, clamp), fill, and the 2 zeros of the next step
            if tally is not None and len(tally) < 4:
                tally.append(count)
    return torch.stack([x0, y0], dim=1)


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'trajectory_time.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('trajectory_time: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    from deepphysinet_amd.utils.init import scaled_init_
    scaled_init_(m.physics_net, seed=1)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    field, fh, s = b['field_data'], b['forecast_h'], syn.sampler
    result = {'steps': STEPS, 'step_hours': -STEP_H, 'stages': 4 * STEPS, 'method': 'rk4', 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
              'launches_per_stage': {'fused': 2}, 'parcels': {}}
    for n in (256, 16384):
        g = np.random.default_rng(n)
        xs, ys = 64.0 + g.random(n) * 128.0, 36.0 + g.random(n) * 72.0
        xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
        tally = []
        routes = [('fused', lambda: m.trajectories(field, s, xs, ys, START_H, fh, -STEPS * STEP_H, STEP_H, 'rk4')),
                  ('composed', lambda: composed(m, field, s, xd, yd, fh))]
        fused = routes[0][1]()
        comp = composed(m, field, s, xd, yd, fh, tally)
        alive = fused['status'] == 0
        diff = (fused['positions'][-1][alive] - comp[alive]).abs().max().item() if bool(alive.any()) else float('nan')
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):                            # alternated: every route sees the same state of the box
            for name, fn in routes:
                times[name].append(_timed(fn)[0])
        result['launches_per_stage']['composed'] = tally
        row = {name: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'us_per_stage': statistics.median(v) * 1e3 / (4 * STEPS)}
               for name, v in times.items()}
        row.update(alive=int(alive.sum()), max_abs_position_difference=diff, speedup=row['composed']['median_ms'] / row['fused']['median_ms'])
        result['parcels'][str(n)] = row
        print('%6d parcels (%d alive at the end, end positions differ by at most %.3e cells):' % (n, row['alive'], diff))
        for name in times:
            print('  %-9s %8.2f ms (min %.2f .. max %.2f, n = %d)   %.1f us per stage' % (name, row[name]['median_ms'], row[name]['min_ms'],
                                                                                         row[name]['max_ms'], args.reps, row[name]['us_per_stage']))
        print('  composed / fused = %.2f' % row['speedup'])
    print('launches per stage: fused 2; composed %s (the four RK4 stages)' % tally)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fobj:
        json.dump(result, fobj, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
