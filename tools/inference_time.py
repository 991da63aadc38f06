"""Timing of lattice inference (InterfacePhysics.predict_lattice) on two shapes, hi+lo mode, eager launches, a host clock around work that ends in a
device synchronise, median and spread (min .. max) of the timed repetitions.

  refine 1, 25 hours (931 625 points): the only route there was before -- 25 x (CollocationSampler.full_grid + predict_grid) -- and ONE
      predict_lattice call, alternated in the same process (the same maps, bitwise: checked here);
  refine 4, 25 hours (14 785 625 points): predict_lattice alone -- time, points per second, peak device memory.

usage: python tools/inference_time.py [reps]        (default 7 repetitions per route)"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(v):
    return '%.2f ms (min %.2f .. max %.2f, n = %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    field, fh, s = b['field_data'], b['forecast_h'], syn.sampler
    hours = range(25)

    def old_route():
        return torch.stack([m.predict_grid(field, *s.full_grid(h)[:4], fh, with_clip=True) for h in hours])

    lat1 = s.lattice(refine=1, hours=hours)

    def new_route():
        return m.predict_lattice(field, s, lat1, fh, with_clip=True)

    for _ in range(2):                                    # warm-up of both routes
        a, c = old_route(), new_route()
    print('refine 1, 25 hours, %d points: the two routes give %s maps' % (lat1.n_points, 'bitwise equal' if torch.equal(a, c) else 'DIFFERENT'))
    t_old, t_new = [], []
    for _ in range(reps):                                 # alternated: both routes see the same state of the box
        t_old.append(_timed(old_route)[0])
        t_new.append(_timed(new_route)[0])
    print('  25 x (full_grid + predict_grid): %s' % _stats(t_old))
    print('  1 x predict_lattice:             %s   -> %.1f M points/s' % (_stats(t_new), lat1.n_points / statistics.median(t_new) / 1e3))
    del a, c
    lat4 = s.lattice(refine=4, hours=hours)
    chunk = m.chunk_size(lat4.n_points)
    new4 = lambda: m.predict_lattice(field, s, lat4, fh, with_clip=True)
    new4()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t4 = []
    for _ in range(max(3, reps // 2)):
        ms, out = _timed(new4)
        t4.append(ms)
    finite = bool(torch.isfinite(out).all())
    del out
    print('refine 4, 25 hours, %d points (maps %.0f MB) in chunks of %d: %s -> %.1f M points/s, peak device memory %.0f MB, finite %s'
          % (lat4.n_points, lat4.n_points * 24 / 1e6, chunk, _stats(t4), lat4.n_points / statistics.median(t4) / 1e3,
             torch.cuda.max_memory_allocated() / 1e6, finite))


if __name__ == '__main__':
    main()
