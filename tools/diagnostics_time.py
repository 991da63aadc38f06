"""Timing of the derived diagnostics on a lattice (InterfacePhysics.diagnostic_lattice), hi+lo mode, eager launches, a host clock around work that ends
in a device synchronise, median and spread (min .. max) of the timed repetitions.

  refine 1, 25 hours (931 625 points): diagnostic_lattice with all 28 products and with 2 (vorticity, dT_dt), alternated in the same process with
      residual_lattice on the same lattice -- the yardstick: the same forward with Jacobian, another output kernel.

usage: python tools/diagnostics_time.py [reps]        (default 7 repetitions per route)"""
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
    from deepphysinet_amd.diagnostics import PRODUCTS
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    field, fh, s = b['field_data'], b['forecast_h'], syn.sampler
    lat = s.lattice(refine=1, hours=range(25))
    routes = [('residual_lattice (6 residuals)', lambda: m.residual_lattice(field, s, lat, fh)),
              ('diagnostic_lattice, 28 products', lambda: m.diagnostic_lattice(field, s, lat, fh, PRODUCTS)),
              ('diagnostic_lattice, 2 products', lambda: m.diagnostic_lattice(field, s, lat, fh, ['vorticity', 'dT_dt']))]
    for _ in range(2):                                    # warm-up of every route
        outs = [fn() for _, fn in routes]
    print('refine 1, 25 hours, %d points; maps %s, %s, %s; finite %s' % (lat.n_points, *(tuple(o.shape) for o in outs),
                                                                         [bool(torch.isfinite(o).all()) for o in outs]))
    print('  the 2-product maps are columns of the 28-product maps: %s' % bool(torch.equal(outs[2], outs[1][:, [18, 11]])))
    del outs
    times = [[] for _ in routes]
    for _ in range(reps):                                 # alternated: every route sees the same state of the box
        for v, (_, fn) in zip(times, routes):
            v.append(_timed(fn)[0])
    for v, (name, _) in zip(times, routes):
        print('  %-34s %s   -> %.1f M points/s' % (name + ':', _stats(v), lat.n_points / statistics.median(v) / 1e3))


if __name__ == '__main__':
    main()
