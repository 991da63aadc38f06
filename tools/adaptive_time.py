"""Cost of residual-weighted interior points, hi+lo mode, eager launches, a host clock around work that ends in a device synchronise, median and spread
(min .. max) of the timed repetitions after warm-up; the routes alternate in one process, so all see the same state of the box.

  (a) training_step on the shipped batch (4 096 interior + 20 480 margin points) as it runs without the option;
  (b) the same preceded by adaptive_interior at pool factors 4, 8 and 16 (one encoder forward + one fields-and-Jacobian pass over the pool + selection);
  (c) the selection launches alone on a pool that is already scored: dpn_adaptive_scores (2 launches) + dpn_adaptive_select (4 launches).

usage: python tools/adaptive_time.py [reps]        (default 9 repetitions)"""
import ctypes
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


def _stats(v, unit='ms', scale=1.0):
    v = [x * scale for x in v]
    return '%.3f %s (min %.3f .. max %.3f, n = %d)' % (statistics.median(v), unit, min(v), max(v), len(v))


def main():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.point_path import LOSS_ORDER, _ptr, _stream
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    src = SyntheticSamples(dev, leads=4, seed=1)
    batch = src[0]
    opt = m.build_optimizer()
    factors = (4, 8, 16)
    routes = {'plain': lambda: m.training_step(batch, opt, with_pde=True)}
    for pf in factors:
        routes['pool x%d' % pf] = lambda pf=pf: m.training_step(m.adaptive_interior(batch, src.sampler, pool_factor=pf), opt, with_pde=True)
        routes['refresh x%d alone' % pf] = lambda pf=pf: m.adaptive_interior(batch, src.sampler, pool_factor=pf)
    for fn in routes.values():
        fn(), fn()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(_timed(fn)[0])
    n = batch['inter_x'].shape[0]
    print('training_step, %d interior + %d margin points:' % (n, batch['margin_x'].shape[0]))
    for k in routes:
        print('  %-20s %s' % (k, _stats(times[k])))
    # (c) the selection alone, on a scored pool
    lib = L.load()
    lf = m.train_cfg['losses']['loss_factor']
    fac = (ctypes.c_double * 6)(*[float(lf[k]) for k in LOSS_ORDER])
    for pf in factors:
        pool = pf * n
        with torch.no_grad():
            field = m._inference_weights(batch['field_data'], batch['forecast_h'], pool)
            x, y, t, cd, f = src.sampler.get_inter_data(pool)
            score, stats, res, scratch = field.residual_scores(x, y, t, f.reshape(-1), cd, [float(lf[k]) for k in LOSS_ORDER])
        rows = (x, y, t, f.reshape(-1), cd)

        def select():
            L.check(lib.dpn_adaptive_scores(_ptr(res), pool, fac, 1.0, _ptr(score), _ptr(stats), _ptr(scratch), _stream()), 'dpn_adaptive_scores')
            return src.sampler.select_weighted(score, rows, n, 1.0, 1.0, scratch=scratch)
        select(), select()
        ts = [_timed(select)[0] for _ in range(reps)]
        many = lambda: [select() for _ in range(20)]
        tm = [_timed(many)[0] / 20 for _ in range(reps)]
        print('selection alone, pool %6d -> %d: one call + synchronise %s; per call in a queue of 20 %s' % (pool, n, _stats(ts, 'us', 1e3), _stats(tm, 'us', 1e3)))


if __name__ == '__main__':
    main()
