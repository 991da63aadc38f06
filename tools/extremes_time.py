"""Window extremes on the network's own d/dt (InterfacePhysics.extremes_at / extreme_lattice) against the dense route that existed before: predict_points
/ predict_lattice on a one-minute time lattice plus a torch max.  One MI355X, hi+lo mode, a synthetic field sample, a 24 h window, the columns
T:max, T:min, speed:max; 256 stations, and the full fine grid (257 x 145 = 37 265 positions).

Per route and problem: wall time of the whole call between two device synchronisations (median and spread of the rounds after one warm-up call), peak
device memory of the call above what was allocated before it (torch.cuda.max_memory_allocated), the time resolution it reaches, and the largest amount
by which the dense maximum (minimum) exceeds (falls below) the refined one.  The arithmetic to hold the times against: K + 1 = 25 fields-only forwards
and Cr * (R + 1) = 3 * 11 = 33 forwards with the Jacobian per position, against 1441 fields-only forwards.

The slope the refinement reads is the network's d/dt at fixed interpolated input; a station's series also moves with its coarse-cube input, which the
slope does not see, and a random-weight network on random fields varies inside an hour.  The excess of the dense route printed here is therefore a
property of this synthetic sample, not of the kernels.

usage: python tools/extremes_time.py [rounds] [--scan HOURS] [--refine R]          (default 3 rounds, hourly scan, R = 10)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLUMNS = ['T:max', 'T:min', 'speed:max']
WINDOW = (0.0, 24.0)
MINUTES = 1441


def _opt(name, default, kind):
    argv = sys.argv[1:]
    return kind(argv[argv.index(name) + 1]) if name in argv else default


def _measure(fn, rounds):
    """(result of the last call, [ms per call], peak bytes above the level before the call)."""
    fn()                                                       # warm-up: allocator, packing, first launches
    times, peak, out = [], 0, None
    for _ in range(rounds):
        out = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return out, times, peak


def _line(what, times, peak, resolution):
    return '%-34s %9.1f ms (min %.1f .. max %.1f, n = %d)   peak %8.1f MiB   resolves %s' % (
        what, statistics.median(times), min(times), max(times), len(times), peak / 2.0 ** 20, resolution)


def _dense_extremes(fields, axis_of_variables):
    """(T max, T min, speed max) over the leading time axis of de-normalised fields."""
    take = lambda k: fields.select(axis_of_variables, k)
    speed = torch.sqrt(take(0) * take(0) + take(1) * take(1))
    return torch.stack([take(3).max(dim=0).values, take(3).min(dim=0).values, speed.max(dim=0).values])


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    rounds = int(next((a for a in sys.argv[1:] if a.isdigit()), 3))
    scan, refine = _opt('--scan', 1.0, float), _opt('--refine', 10, int)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    m.physics_net.eval()
    syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    field, fh, s = b['field_data'].to(dev), b['forecast_h'].to(dev), syn.sampler
    g = np.random.default_rng(0)
    xs, ys = 1.0 + g.random(256) * 254.0, 1.0 + g.random(256) * 142.0
    minutes = np.arange(MINUTES) / 60.0
    sign = torch.tensor([1.0, -1.0, 1.0], device=dev)
    K = int(round((WINDOW[1] - WINDOW[0]) / scan))
    fine = '%.3g s (scan %g h / 2**%d)' % (scan * 3600.0 / 2 ** refine, scan, refine)
    print('%s, %s, torch %s; columns %s, window %s h, scan %g h (K = %d), R = %d: %d + %d forwards per position against %d'
          % (torch.cuda.get_device_name(0), 'hi+lo', torch.__version__, ','.join(COLUMNS), WINDOW, scan, K, refine, K + 1, 3 * (refine + 1), MINUTES))

    # ---- 256 stations
    def refined_rows():
        return m.extremes_at(field, s, xs, ys, WINDOW, fh, COLUMNS, scan, refine)

    def dense_rows():
        rows = m.predict_points(field, s, np.tile(xs, MINUTES), np.tile(ys, MINUTES), np.repeat(minutes, xs.size), fh)
        return _dense_extremes(rows.view(MINUTES, xs.size, 6), 2)
    r, t_r, p_r = _measure(refined_rows, rounds)
    d, t_d, p_d = _measure(dense_rows, rounds)
    print(_line('256 stations, extremes_at', t_r, p_r, fine))
    print(_line('256 stations, predict_points + max', t_d, p_d, '60 s'))
    excess = ((d.t() - r['value']) * sign).max(dim=0).values
    print('256 stations: dense exceeds refined by at most %s (T:max K, T:min K, speed:max m/s); refined at least as good at %d of %d (station, column); '
          'statuses %s' % (['%.4g' % v for v in excess.tolist()], int(((d.t() - r['value']) * sign <= 0).sum()), 3 * xs.size,
                           dict(zip(*[v.tolist() for v in torch.unique(r['status'], return_counts=True)]))))
    del r, d

    # ---- the full fine grid
    def refined_maps():
        return m.extreme_lattice(field, s, s.lattice(refine=1, hours=0.0), WINDOW, fh, COLUMNS, scan, refine)

    def dense_maps():
        maps = m.predict_lattice(field, s, s.lattice(refine=1, hours=(0.0, 1.0 / 60.0, MINUTES)), fh)
        return _dense_extremes(maps, 1)
    r, t_r, p_r = _measure(refined_maps, rounds)
    d, t_d, p_d = _measure(dense_maps, rounds)
    print(_line('37 265 positions, extreme_lattice', t_r, p_r, fine))
    print(_line('37 265 positions, predict_lattice + max', t_d, p_d, '60 s'))
    short = (d - r['value']) * sign.view(3, 1, 1)
    print('37 265 positions: dense exceeds refined by at most %s (T:max K, T:min K, speed:max m/s); refined at least as good at %d of %d (position, '
          'column)' % (['%.4g' % v for v in short.amax(dim=(1, 2)).tolist()], int((short <= 0).sum()), short.numel()))


if __name__ == '__main__':
    main()
