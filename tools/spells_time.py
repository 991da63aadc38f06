"""Threshold spells by scan and bisection (InterfacePhysics.spells_at / spell_lattice) against the dense route that existed before: predict_points /
predict_lattice on a one-minute time lattice plus counting in torch.  One MI355X, hi+lo mode, a synthetic field sample, a 24 h window, the columns
T:below, speed:above and q:above at the medians of the 256 stations' one-minute series (found before anything is timed, so that most positions have
crossings); 256 stations, and the full fine grid (257 x 145 = 37 265 positions).

Per route and problem: wall time of the whole call between two device synchronisations (median and spread of the rounds after one warm-up call), peak
device memory of the call above what was allocated before it (torch.cuda.max_memory_allocated), the time resolution it reaches, and how the two
routes' hours agree where they count the same crossings.  The arithmetic to hold the times against: K + 1 = 25 fields-only forwards and 2 * C * R =
2 * 3 * 10 = 60 more per position, against 1441 fields-only forwards.

A random-weight network on random fields crosses a threshold many times a day, often twice inside an hour; such a spell hidden inside a scan step is
not seen by the scan, and the crossings between the first entry and the last exit keep the scan's linear interpolation -- both ends of a gap between
two spells that reach the window's ends among them.  How many positions count other crossings on the two routes, and how many are such gaps, is
printed; it is a property of this synthetic sample, not of the kernels.

usage: python tools/spells_time.py [rounds] [--scan HOURS] [--refine R]          (default 3 rounds, hourly scan, R = 10)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRODUCTS = (('T', 'below'), ('speed', 'above'), ('q', 'above'))
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
    return '%-36s %9.1f ms (min %.1f .. max %.1f, n = %d)   peak %8.1f MiB   resolves %s' % (
        what, statistics.median(times), min(times), max(times), len(times), peak / 2.0 ** 20, resolution)


def _series(fields, axis_of_variables):
    """(T, speed, q) over the leading one-minute axis of de-normalised fields."""
    take = lambda k: fields.select(axis_of_variables, k)
    return take(3), torch.sqrt(take(0) * take(0) + take(1) * take(1)), take(4)


def _dense_spells(fields, axis_of_variables, thr):
    """(hours [3, ...] fp64, crossings [3, ...], gap [3, ...] bool) of the three columns over the leading one-minute axis of de-normalised fields:
    every minute step counts the share of its two ends that is in; gap: in at both ends of the window with two crossings."""
    T, speed, q = _series(fields, axis_of_variables)
    inn = torch.stack([T < thr[0], speed > thr[1], q > thr[2]], dim=1)                     # [minutes, 3, ...]
    hours = (inn[1:].sum(dim=0, dtype=torch.float64) + inn[:-1].sum(dim=0, dtype=torch.float64)) * (0.5 / 60.0)
    crossings = (inn[1:] != inn[:-1]).sum(dim=0)
    return hours, crossings, inn[0] & inn[-1] & (crossings == 2)


def _agreement(what, r_hours, r_cross, d, unit):
    d_hours, d_cross, gap = d
    same = r_cross == d_cross
    few = same & (d_cross <= 2) & (d_cross > 0) & ~gap
    diff = (r_hours - d_hours).abs()
    print('%s: of %d (%s, column) %d have a crossing on the one-minute series and %d count the same crossings on both routes; %d of these have one or '
          'two crossings and are no gap: there |hours - dense hours| is at most %.4f h, median %.4f h; at the %d gaps at most %.3f h, median %.4f h'
          % (what, same.numel(), unit, int((d_cross > 0).sum()), int(same.sum()), int(few.sum()), float(diff[few].max()), float(diff[few].median()),
             int((same & gap).sum()), float(diff[same & gap].max()), float(diff[same & gap].median())))


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
    K = int(round((WINDOW[1] - WINDOW[0]) / scan))
    rows = m.predict_points(field, s, np.tile(xs, MINUTES), np.tile(ys, MINUTES), np.repeat(minutes, xs.size), fh)
    thr = [float('%.6g' % float(v.double().median())) for v in _series(rows.view(MINUTES, xs.size, 6), 2)]
    thr = [float(np.float32(v)) for v in thr]                  # as the request holds them
    COLUMNS = ['%s:%s:%.6g' % (name, side, v) for (name, side), v in zip(PRODUCTS, thr)]
    del rows
    fine = '%.3g s (scan %g h / 2**%d)' % (scan * 3600.0 / 2 ** refine, scan, refine)
    print('%s, %s, torch %s; columns %s, window %s h, scan %g h (K = %d), R = %d: %d + %d forwards per position against %d'
          % (torch.cuda.get_device_name(0), 'hi+lo', torch.__version__, ','.join(COLUMNS), WINDOW, scan, K, refine, K + 1, 2 * len(COLUMNS) * refine, MINUTES))

    # ---- 256 stations
    def refined_rows():
        return m.spells_at(field, s, xs, ys, WINDOW, fh, COLUMNS, scan, refine)

    def dense_rows():
        rows = m.predict_points(field, s, np.tile(xs, MINUTES), np.tile(ys, MINUTES), np.repeat(minutes, xs.size), fh)
        return _dense_spells(rows.view(MINUTES, xs.size, 6), 2, thr)
    r, t_r, p_r = _measure(refined_rows, rounds)
    d, t_d, p_d = _measure(dense_rows, rounds)
    print(_line('256 stations, spells_at', t_r, p_r, fine))
    print(_line('256 stations, predict_points + count', t_d, p_d, '60 s'))
    _agreement('256 stations', r['hours'].t(), r['crossings'].t(), d, 'station')
    print('256 stations: statuses %s' % dict(zip(*[v.tolist() for v in torch.unique(r['status'], return_counts=True)])))
    del r, d

    # ---- the full fine grid
    def refined_maps():
        return m.spell_lattice(field, s, s.lattice(refine=1, hours=0.0), WINDOW, fh, COLUMNS, scan, refine)

    def dense_maps():
        maps = m.predict_lattice(field, s, s.lattice(refine=1, hours=(0.0, 1.0 / 60.0, MINUTES)), fh)
        return _dense_spells(maps, 1, thr)
    r, t_r, p_r = _measure(refined_maps, rounds)
    d, t_d, p_d = _measure(dense_maps, rounds)
    print(_line('37 265 positions, spell_lattice', t_r, p_r, fine))
    print(_line('37 265 positions, predict_lattice + count', t_d, p_d, '60 s'))
    _agreement('37 265 positions', r['hours'], r['crossings'], d, 'position')


if __name__ == '__main__':
    main()
