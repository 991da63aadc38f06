"""Cases of the threshold spells (deepphysinet_amd/spells.py), shared by tests/test_spells_cpu.py and tests/test_gpu_spells.py: analytic series with known
crossings, the checks that drive any implementation of the driver over them (the seeded mistakes go through the same checks), and the stations,
columns and counting of the dense-route comparison (the world itself, its sampler and the fp64 oracle are tests/extremes_cases.py's).

Bars.  R rounds halve a scan step R times: a refined hour lies within W = dt / 2**R of the crossing, where the series crosses once inside the step.
In fp64 the rest is rounding of the hours (EPS64, a few hundred fp64 steps of 24 h).  In float32 a value within one float32 step of the threshold may
fall on either side of it: that moves a crossing by at most that step over the slope of the series there (each float32 check states its own)."""
import functools

import numpy as np

from deepphysinet_amd import spells as S
from tests.extremes_cases import PEAKS, Q, RHO, T, U, V, P, evaluator      # noqa: F401 (the field indices are part of the cases' vocabulary)

EPS64 = 1e-12
START, END = S.HOLDS_AT_START, S.HOLDS_AT_END


def fields(fn):
    """An evaluator from fn(hours, points) -> {column of out_n: value}."""
    return evaluator(lambda h, p: {k: (v, np.zeros_like(h)) for k, v in fn(h, p).items()})


def clipped_trapezoid(nodes, thr, side, dt):
    """The integral of max(margin, 0) of the piecewise-linear series through nodes [K + 1, n] (fp64), in closed form per step: a step with both ends
    in is a trapezoid, a step that crosses is the triangle on the in side, whose base is the in end's share of the step."""
    d = nodes.astype(np.float64) - np.float64(thr)
    d = -d if side == 'below' else d
    a, b = d[:-1], d[1:]
    with np.errstate(invalid='ignore', divide='ignore'):
        tri = lambda inside, outside: 0.5 * inside * inside / (inside - outside) * dt
        area = np.where((a > 0) & (b > 0), 0.5 * (a + b) * dt, np.where((a <= 0) & (b > 0), tri(b, a), np.where((a > 0) & (b <= 0), tri(a, b), 0.0)))
    return area.sum(axis=0)


# ------------------------------------------------------------------------------------------------ the checks (each takes the driver)
SINE_PEAKS = PEAKS[:4]                                        # extremes_cases.PEAKS whose spell lies inside (0, 24)
# (peaks, window): the spells inside the window; a spell that is still on at t1 (the day before's ended at 0.96 h, before this window begins); a
# spell that is already on at t0 (the next day's begins at 22.5 h, behind this window)
SINE_WINDOWS = ((SINE_PEAKS, (0.0, 24.0)), (np.array([20.96]), (4.0, 24.0)), (np.array([2.5]), (0.0, 20.0)))


def check_sine(run):
    """T = 280 + 5 cos((h - a) pi / 12) against 282.5: in for |h - a| < 4, the crossings at a -+ 4, 8 hours in; the peaks lie right of, left of,
    between and next to scan nodes, and two more spells are cut by their windows (in at t1, in at t0).  For R = 0, 1, 4, 10: first and last within
    W of the truth, on the in side of it, the other bracket end on the out side, the brackets W wide; hours within 2 W; in float32 plus 4e-5 h per
    crossing (one float32 step of 282.5, 3.1e-5 K, over the slope there, 5 pi / 12 sin(pi / 3) = 1.13 K/h)."""
    w = np.pi / 12.0
    for a, (t0, t1) in SINE_WINDOWS:
        ev = fields(lambda h, p: {T: 280.0 + 5.0 * np.cos((h - a[p]) * w)})
        t_in, t_out = a - 4.0, a + 4.0
        at_start, at_end = t_in < t0, t_out > t1
        first_true, last_true = np.where(at_start, t0, t_in), np.where(at_end, t1, t_out)
        for dtype, flat in ((np.float64, EPS64), (np.float32, 4e-5)):
            for R in (0, 1, 4, 10):
                r = run(ev, a.size, ['T:above:282.5'], (t0, t1), 1.0, R, dtype=dtype)
                W = 1.0 / 2 ** R
                first, last, lo, hi = (r[k][:, 0] for k in ('first', 'last', 'first_lo', 'last_hi'))
                assert r['status'][:, 0].tolist() == (START * at_start + END * at_end).tolist(), (dtype, R, r['status'])
                assert r['crossings'][:, 0].tolist() == (2 - at_start - at_end).tolist()
                assert np.all(first >= first_true - flat) and np.all(first - first_true <= W + flat), (dtype, R, first)
                assert np.all(last <= last_true + flat) and np.all(last_true - last <= W + flat), (dtype, R, last)
                assert np.all(lo <= first_true + flat) and np.all(hi >= last_true - flat), (dtype, R)
                assert np.all((first - lo)[~at_start] == W) and np.all((hi - last)[~at_end] == W)
                assert np.all((first == lo)[at_start]) and np.all((hi == last)[at_end])
                assert np.all(np.abs(r['hours'][:, 0] - (last_true - first_true)) <= 2 * W + 2 * flat), (dtype, R, r['hours'][:, 0])
    assert [(s.any(), e.any()) for s, e in [(a - 4.0 < w0, a + 4.0 > w1) for a, (w0, w1) in SINE_WINDOWS]] == [(False, False), (False, True), (True, False)]


def check_ramp(run):
    """u = 0.5 h + p over (2, 20) against 6.125 (a float32): out at the start, one entry at 12.25 - 2 p, in at the window's end."""
    ev = fields(lambda h, p: {U: 0.5 * h + p})
    truth = np.array([12.25, 10.25])
    for R in (0, 3, 10):
        r = run(ev, 2, ['u:above:6.125'], (2.0, 20.0), 1.5, R, dtype=np.float64)
        W = 1.5 / 2 ** R
        assert r['status'][:, 0].tolist() == [END, END] and r['crossings'][:, 0].tolist() == [1, 1] and r['last'][:, 0].tolist() == [20.0, 20.0]
        assert np.all(r['first'][:, 0] >= truth - EPS64) and np.all(r['first'][:, 0] - truth <= W + EPS64), (R, r['first'])
        assert np.all(np.abs(r['hours'][:, 0] - (20.0 - truth)) <= W + EPS64), (R, r['hours'])


def check_constant_at_threshold(run):
    """A constant equal to the threshold is neither above nor below it (strict): NEVER, no time, no excess, no hour."""
    ev = fields(lambda h, p: {T: np.full_like(h, 282.5)})
    r = run(ev, 2, ['T:above:282.5', 'T:below:282.5'], (4.0, 10.0), 1.0, 5)
    assert r['status'].tolist() == [[S.NEVER, S.NEVER]] * 2 and r['crossings'].tolist() == [[0, 0]] * 2
    assert r['hours'].tolist() == [[0.0, 0.0]] * 2 and r['excess'].tolist() == [[0.0, 0.0]] * 2
    assert all(np.isnan(r[k]).all() for k in ('first', 'last', 'first_lo', 'last_hi'))


def check_constant_above(run):
    """A constant above the threshold: in from t0 to t1, both HOLDS flags, hours = t1 - t0 and excess = margin * (t1 - t0) exactly (whole steps of
    1 h); the below column of the same threshold: NEVER."""
    ev = fields(lambda h, p: {T: np.full_like(h, 285.0)})
    r = run(ev, 3, ['T:above:282.5', 'T:below:282.5'], (4.0, 10.0), 1.0, 5)
    assert r['status'].tolist() == [[START | END, S.NEVER]] * 3 and r['crossings'].tolist() == [[0, 0]] * 3
    assert r['hours'].tolist() == [[6.0, 0.0]] * 3 and r['excess'].tolist() == [[15.0, 0.0]] * 3
    assert r['first'][:, 0].tolist() == [4.0] * 3 and r['last'][:, 0].tolist() == [10.0] * 3 and r['first_lo'][:, 0].tolist() == [4.0] * 3


# two spells of a piecewise-linear series with its kinks on scan nodes: the scan's interpolated crossings are the true ones (to rounding), so the two
# inner crossings, which are not refined, do not limit the bar of `hours`
_KNOTS = (np.array([0.0, 3.0, 4.0, 7.0, 8.0, 12.0, 13.0, 16.0, 17.0, 24.0]), np.array([278.0, 278.0, 283.0, 283.0, 279.0, 279.0, 281.0, 281.0, 277.0, 277.0]))


def check_two_spells(run):
    """In for 3.4 < h < 7.75 and for 12.5 < h < 16.25 (above 280): four crossings, first from the first spell, last from the second, 8.1 hours in;
    the first entry's share of its step (0.6 h) differs from the second's (0.5 h)."""
    ev = fields(lambda h, p: {T: np.interp(h, *_KNOTS)})
    for R in (0, 10):
        r = run(ev, 1, ['T:above:280'], (0.0, 24.0), 1.0, R, dtype=np.float64)
        W = 1.0 / 2 ** R
        assert r['crossings'][0, 0] == 4 and r['status'][0, 0] == 0
        assert 3.4 - EPS64 <= r['first'][0, 0] <= 3.4 + W + EPS64 and 16.25 - W - EPS64 <= r['last'][0, 0] <= 16.25 + EPS64, (R, r['first'], r['last'])
        assert abs(r['hours'][0, 0] - 8.1) <= 2 * W + EPS64, (R, r['hours'])
        assert abs(r['excess'][0, 0] - clipped_trapezoid(r['scan'][:, :, 0], 280.0, 'above', 1.0)[0]) <= EPS64 * 24


def check_single_node(run):
    """T = 281 - 2.5 |h - a| against 280, a on a scan node: in for |h - a| < 0.4, so node a alone is in (k_first == k_last); the entry bracket is the
    step before it, the exit bracket the step after it."""
    a = np.array([7.0, 12.0])
    ev = fields(lambda h, p: {T: 281.0 - 2.5 * np.abs(h - a[p])})
    for R in (0, 2, 10):
        r = run(ev, 2, ['T:above:280'], (0.0, 24.0), 1.0, R, dtype=np.float64)
        W = 1.0 / 2 ** R
        assert r['status'][:, 0].tolist() == [0, 0] and r['crossings'][:, 0].tolist() == [2, 2]
        assert np.all(r['first'][:, 0] >= a - 0.4 - EPS64) and np.all(r['first'][:, 0] <= a - 0.4 + W + EPS64), (R, r['first'])
        assert np.all(r['last'][:, 0] <= a + 0.4 + EPS64) and np.all(r['last'][:, 0] >= a + 0.4 - W - EPS64), (R, r['last'])
        assert np.all(np.abs(r['hours'][:, 0] - 0.8) <= 2 * W + EPS64), (R, r['hours'])
        if R == 0:
            assert r['first'][:, 0].tolist() == a.tolist() and r['last'][:, 0].tolist() == a.tolist() and np.all(np.abs(r['hours'][:, 0]) <= EPS64)


def check_below(run):
    """Frost hours: T = 274 - 4 cos((h - 14.3) pi / 12) below 273.15 (as float32 holds it): in where cos > (274 - thr) / 4, a spell inside the window
    around hour 14.3.  In float32 plus 5e-5 h per crossing (one float32 step of 273.15, 3.1e-5 K, over the slope there, 1.02 K/h)."""
    thr = float(np.float32(273.15))
    half = np.arccos((274.0 - thr) / 4.0) * 12.0 / np.pi
    t_in, t_out = 14.3 - half, 14.3 + half
    assert 9.0 < t_in < 9.2 and 19.4 < t_out < 19.6
    ev = fields(lambda h, p: {T: 274.0 - 4.0 * np.cos((h - 14.3) * np.pi / 12.0)})
    for dtype, flat in ((np.float64, EPS64), (np.float32, 5e-5)):
        r = run(ev, 1, ['T:below:273.15', 'T:above:273.15'], (0.0, 24.0), 1.0, 10, dtype=dtype)
        W = 1.0 / 2 ** 10
        assert r['status'][0].tolist() == [0, START | END] and r['crossings'][0].tolist() == [2, 2]
        assert t_in - flat <= r['first'][0, 0] <= t_in + W + flat and t_out - W - flat <= r['last'][0, 0] <= t_out + flat, (dtype, r['first'], r['last'])
        assert abs(r['hours'][0, 0] - 2.0 * half) <= 2 * W + 2 * flat and r['excess'][0, 0] > 0.0
        assert r['first'][0, 1] == 0.0 and r['last'][0, 1] == 24.0
        for c, side in enumerate(('below', 'above')):
            want = clipped_trapezoid(r['scan'][:, :, c], np.asarray(thr, dtype=dtype), side, 1.0)[0]
            assert abs(r['excess'][0, c] - want) <= 1e-12 * want, (dtype, side)


def check_speed(run):
    """u = 3 + 0.5 h, v = 4: the speed passes 10 where u * u = 84, at h = 12.3303; above: one entry, in at t1; below: in at t0, one exit."""
    truth = (np.sqrt(84.0) - 3.0) / 0.5
    ev = fields(lambda h, p: {U: 3.0 + 0.5 * h, V: np.full_like(h, 4.0)})
    r = run(ev, 1, ['speed:above:10', 'speed:below:10'], (0.0, 24.0), 1.0, 10, dtype=np.float64)
    W = 1.0 / 2 ** 10
    assert r['status'][0].tolist() == [END, START] and r['crossings'][0].tolist() == [1, 1]
    assert truth - EPS64 <= r['first'][0, 0] <= truth + W + EPS64 and r['last'][0, 0] == 24.0
    assert truth - W - EPS64 <= r['last'][0, 1] <= truth + EPS64 and r['first'][0, 1] == 0.0
    assert abs(r['hours'][0, 0] - (24.0 - truth)) <= W + EPS64 and abs(r['hours'][0, 1] - truth) <= W + EPS64


def check_nan_in_scan(run):
    """A NaN at one scan node of one point: that point's columns end with BAD_SCAN and NaN everywhere, the other point is untouched."""
    ev = fields(lambda h, p: {T: np.where((p == 1) & (h == 7.0), np.nan, 280.0 + np.sin(h / 1.5))})
    r = run(ev, 2, ['T:above:280', 'T:below:280'], (0.0, 12.0), 1.0, 3)
    assert r['status'][1].tolist() == [S.BAD_SCAN] * 2 and not (r['status'][0] & S.BAD_SCAN).any()
    for key in ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess'):
        assert np.isnan(r[key][1]).all() and np.isfinite(r[key][0]).all(), key


def check_nan_at_probe(run):
    """Point 0's value is NaN away from the whole hours: the scan passes, the first round stops the column with STOPPED and both brackets stand as the
    scan left them -- first and last are scan nodes, hours the whole steps in between; point 1 goes on."""
    def fn(h, p):
        return {T: np.where((p == 0) & (h != np.round(h)), np.nan, 280.0 + 5.0 * np.cos((h - 6.3) * np.pi / 12.0))}
    r = run(fields(fn), 2, ['T:above:282.5'], (0.0, 12.0), 1.0, 6, dtype=np.float64)
    assert r['status'][:, 0].tolist() == [S.STOPPED, 0]
    assert (r['first'][0, 0], r['first_lo'][0, 0], r['last'][0, 0], r['last_hi'][0, 0]) == (3.0, 2.0, 10.0, 11.0) and abs(r['hours'][0, 0] - 7.0) <= EPS64
    assert 2.3 - EPS64 <= r['first'][1, 0] <= 2.3 + 1.0 / 2 ** 6 + EPS64 and abs(r['hours'][1, 0] - 8.0) <= 2.0 / 2 ** 6 + EPS64


def check_small(run):
    """K = 1 with R = 0 and R = 1: two nodes, T = h against 3.25 over (3, 4): node 0 out, node 1 in.  R = 0: first is node 1, nothing of the step counts;
    R = 1: the probe at 3.5 is in."""
    ev = fields(lambda h, p: {T: h})
    r0 = run(ev, 1, ['T:above:3.25'], (3.0, 4.0), 1.0, 0, dtype=np.float64)
    assert r0['scan'].shape == (2, 1, 1) and r0['status'].tolist() == [[END]] and r0['crossings'].tolist() == [[1]]
    assert (r0['first'][0, 0], r0['first_lo'][0, 0], r0['last'][0, 0], r0['last_hi'][0, 0], r0['hours'][0, 0]) == (4.0, 3.0, 4.0, 4.0, 0.0)
    assert abs(r0['excess'][0, 0] - 0.5 * 0.75 * 0.75) <= EPS64
    r1 = run(ev, 1, ['T:above:3.25'], (3.0, 4.0), 1.0, 1, dtype=np.float64)
    assert (r1['first'][0, 0], r1['first_lo'][0, 0], r1['hours'][0, 0]) == (3.5, 3.0, 0.5) and r1['excess'][0, 0] == r0['excess'][0, 0]


def check_excess(run):
    """excess against the closed-form clipped trapezoid of the scan's own nodes (clipped_trapezoid: one expression per step, no state), both sides, in
    fp64 and float32, to 1e-12 of it (K = 24 additions); the refinement does not change it; and against the integral of the series itself,
    (60 sqrt(3) - 20 pi) / pi = 13.08 K h, which the chords of an hourly scan under-estimate by less than 2 %."""
    a, w = SINE_PEAKS, np.pi / 12.0
    ev = fields(lambda h, p: {T: 280.0 + 5.0 * np.cos((h - a[p]) * w)})
    for dtype in (np.float64, np.float32):
        r = run(ev, a.size, ['T:above:282.5', 'T:below:282.5'], (0.0, 24.0), 1.0, 4, dtype=dtype)
        r0 = run(ev, a.size, ['T:above:282.5', 'T:below:282.5'], (0.0, 24.0), 1.0, 0, dtype=dtype)
        for c, side in enumerate(('above', 'below')):
            want = clipped_trapezoid(r['scan'][:, :, c], 282.5, side, 1.0)
            assert np.all(np.abs(r['excess'][:, c] - want) <= 1e-12 * want), (dtype, side, r['excess'][:, c], want)
            assert np.array_equal(r['excess'][:, c], r0['excess'][:, c])
        exact = (60.0 * np.sqrt(3.0) - 20.0 * np.pi) / np.pi
        assert np.all(r['excess'][:, 0] <= exact) and np.all(r['excess'][:, 0] >= 0.98 * exact), r['excess'][:, 0]


CHECKS = (check_sine, check_ramp, check_constant_at_threshold, check_constant_above, check_two_spells, check_single_node, check_below, check_speed,
          check_nan_in_scan, check_nan_at_probe, check_small, check_excess)
# the check that catches each seeded mistake of deepphysinet_amd.spells.MISTAKES
CAUGHT_BY = {'non_strict': check_constant_at_threshold, 'fractions_swapped': check_excess, 'part_first_overwritten': check_two_spells,
             'k_last_not_reset': check_single_node, 'below_not_negated': check_below, 'exit_moves_k_last': check_sine,
             'refine_sides_swapped': check_sine, 'parts_not_replaced': check_sine}


def mistaken(kind):
    return functools.partial(S.spells_reference, _mistakes=(kind,))


# ------------------------------------------------------------------------------------------------ the dense-route comparison
# The world, the eight stations and the seed are extremes_cases' (DENSE_SEED, DENSE_STATIONS); the thresholds are the 5 % / 95 % quantiles of the fp64
# oracle's one-minute series over the eight stations (to six digits), so that most station-columns have few crossings.  Conditions, all read off the
# one-minute series alone (tests/test_spells_cpu.py asserts them on the oracle): at least half of the 40 station-columns have a crossing; at most a
# quarter have another crossing count on the hourly nodes than on the minutes (a spell hidden inside a scan step: left out of the comparison); and no
# compared station-column with two crossings is in at both ends of the window -- there the gap's two ends are neither the first entry nor the last
# exit, the refinement does not touch them, and `hours` keeps the scan's interpolation error, which no bar in dt / 2**R covers.
DENSE_COLUMNS = ('T:above:260.979', 'T:below:179.17', 'speed:above:17.6396', 'q:below:0.0467692', 'v:above:-0.945796')
DENSE_WINDOW, DENSE_SCAN, DENSE_ROUNDS = (0.0, 24.0), 1.0, 10
MINUTES = np.arange(1441) / 60.0


def dense_series(values, names):
    """The series of the columns `names` [C] of [1441, n] from de-normalised one-minute rows values [1441, n, 6]."""
    speed = np.sqrt(values[..., 0] * values[..., 0] + values[..., 1] * values[..., 1])
    return [speed if name.split(':')[0] == 'speed' else values[..., S.PRODUCTS.index(name.split(':')[0])] for name in names]


def dense_spells(series, request):
    """The dense route's counting on one-minute series (a list of [1441, n], one per column of `request`): per column and station the first and the
    last minute that is in (NaN: none), the time in (every minute step counts the share of its two ends that is in), the crossings between
    consecutive minutes, the crossings between consecutive hourly nodes, and whether minute 0 and minute 1440 are in -- each [n, C]."""
    out = {k: [] for k in ('first', 'last', 'hours', 'crossings', 'hourly', 'in_first', 'in_last')}
    for x, thr, side in zip(series, request.thr, request.sides):
        t = x.dtype.type(thr)
        inn = x < t if side == S.BELOW else x > t
        some = inn.any(axis=0)
        out['first'].append(np.where(some, MINUTES[np.argmax(inn, axis=0)], np.nan))
        out['last'].append(np.where(some, MINUTES[len(MINUTES) - 1 - np.argmax(inn[::-1], axis=0)], np.nan))
        out['hours'].append((0.5 * (inn[1:].astype(np.float64) + inn[:-1])).sum(axis=0) / 60.0)
        out['crossings'].append((inn[1:] != inn[:-1]).sum(axis=0))
        out['hourly'].append((inn[::60][1:] != inn[::60][:-1]).sum(axis=0))
        out['in_first'].append(inn[0])
        out['in_last'].append(inn[-1])
    return {k: np.stack(v, axis=1) for k, v in out.items()}


def dense_conditions(d):
    """(compared [n, C] bool, the three conditions' counts) of dense_spells' dict: compared = the same crossing count on minutes and hourly nodes."""
    compared = d['crossings'] == d['hourly']
    gap_only = compared & (d['crossings'] == 2) & d['in_first'] & d['in_last']
    return compared, int((d['crossings'] > 0).sum()), int((~compared).sum()), int(gap_only.sum())


def check_against_dense(r, d, W):
    """The bars of the comparison, for a result dict r (numpy, [n, C]) and dense_spells' d: on every compared station-column the crossing counts
    agree, first and last agree to 1/60 h + W (both NaN where never in), and with at most two crossings hours agrees to crossings / 60 h + 2 W.
    A refined end lies within W behind (before) the crossing, on the in side, the dense one within a minute of it on the same side.  -> the number of
    station-columns whose hours were compared."""
    compared, _, _, _ = dense_conditions(d)
    n_hours = 0
    for i, c in zip(*np.nonzero(compared)):
        where = (int(i), int(c))
        assert r['crossings'][i, c] == d['crossings'][i, c], (where, r['crossings'][i, c], d['crossings'][i, c])
        for key in ('first', 'last'):
            if np.isnan(d[key][i, c]):
                assert np.isnan(r[key][i, c]) and r['status'][i, c] == S.NEVER, (where, key)
            else:
                assert abs(r[key][i, c] - d[key][i, c]) <= 1.0 / 60.0 + W, (where, key, r[key][i, c], d[key][i, c])
        if d['crossings'][i, c] <= 2:
            n_hours += 1
            assert abs(r['hours'][i, c] - d['hours'][i, c]) <= d['crossings'][i, c] / 60.0 + 2 * W, (where, r['hours'][i, c], d['hours'][i, c])
    return n_hours
