"""Shared by tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py: hand-written member sequences with their expected statistics, a plain
loop restatement with seeded mistakes, the bar of the comparison with numpy, and the members of the GPU tests.

A case is (values [M, n, P], thr_col, thr_val, expected): expected holds, per output name, the array the statistics must equal exactly (NaN where
NaN is expected).  Every expected number is written out by hand from the closed forms, not computed by the code under test."""
import numpy as np

NAN = float('nan')
INF = float('inf')


def _case(columns, thr_col=(), thr_val=(), **expected):
    """columns: one member sequence per column (one point); expected: mean, spread, min, max, count (per column), prob (per threshold)."""
    v = np.asarray(columns, dtype=np.float32).T[:, None, :]                     # [M, 1, P]
    exp = {k: np.asarray(a, dtype=np.int32 if k == 'count' else np.float32).reshape(1, -1) for k, a in expected.items()}
    return v, list(thr_col), list(thr_val), exp


def hand_cases():
    s2 = np.sqrt(np.float64(2.0))
    return {
        # one member: the mean is that value bit for bit (0.1f is not a double's 0.1), no spread, min = max = the value
        'one member': _case([[0.1], [-3.0]], mean=[np.float32(0.1), -3.0], spread=[NAN, NAN], min=[np.float32(0.1), -3.0],
                            max=[np.float32(0.1), -3.0], count=[1, 1]),
        # the same member three times: the deviations are exactly 0
        'same member three times': _case([[0.1, 0.1, 0.1], [7.25, 7.25, 7.25]], mean=[np.float32(0.1), 7.25], spread=[0.0, 0.0],
                                         min=[np.float32(0.1), 7.25], max=[np.float32(0.1), 7.25], count=[3, 3]),
        # two members a, b: mean (a + b) / 2, sample standard deviation |a - b| / sqrt(2) (ddof = 1; the population form gives |a - b| / 2)
        'two members': _case([[1.0, 3.0], [-4.0, 4.0]], mean=[2.0, 0.0], spread=[np.float32(2.0 / s2), np.float32(8.0 / s2)], min=[1.0, -4.0],
                             max=[3.0, 4.0], count=[2, 2]),
        # a NaN or an infinite member is skipped in its column only; all-positive and all-negative columns show a min / max that started at 0
        'non-finite members': _case([[2.0, NAN, 4.0, 6.0], [5.0, 6.0, INF, 7.0], [-1.0, -2.0, -3.0, -INF], [1.0, 2.0, 3.0, 4.0]],
                                    thr_col=[0, 1, 3], thr_val=[3.0, 5.5, 2.0],
                                    mean=[4.0, 6.0, -2.0, 2.5], spread=[2.0, 1.0, 1.0, np.float32(np.sqrt(np.float64(5.0) / 3.0))],
                                    min=[2.0, 5.0, -3.0, 1.0], max=[6.0, 7.0, -1.0, 4.0], count=[3, 3, 3, 4],
                                    prob=[np.float32(2.0 / 3.0), np.float32(2.0 / 3.0), 0.5]),            # of the finite members, not of M = 4
        # no finite member: everything NaN, count 0
        'no finite member': _case([[NAN, INF, -INF], [1.0, 2.0, 3.0]], thr_col=[0, 1], thr_val=[0.0, 0.0], mean=[NAN, 2.0], spread=[NAN, 1.0],
                                  min=[NAN, 1.0], max=[NAN, 3.0], count=[0, 3], prob=[NAN, 1.0]),
        # the comparison is strict: a member equal to the threshold does not count; two thresholds on one column
        'strict threshold': _case([[1.0, 2.0, 3.0, 2.0]], thr_col=[0, 0], thr_val=[2.0, 1.5], mean=[2.0], spread=[np.float32(np.sqrt(2.0 / 3.0))],
                                  min=[1.0], max=[3.0], count=[4], prob=[0.25, 0.75]),
    }


MISTAKES = ('population variance', '>= for >', 'NaN member counted', 'prob over M', 'min and max start at 0')


def loop_statistics(values, thr_col=(), thr_val=(), mistake=None):
    """The statistics by a plain two-pass loop over the finite members of every (point, column) -- not Welford, not the code under test --, with one of
    MISTAKES seeded on request."""
    v = np.asarray(values, dtype=np.float32)
    M, n, P = v.shape
    E = len(thr_col)
    out = dict(mean=np.full((n, P), np.nan, np.float32), spread=np.full((n, P), np.nan, np.float32), min=np.full((n, P), np.nan, np.float32),
               max=np.full((n, P), np.nan, np.float32), count=np.zeros((n, P), np.int32), prob=np.full((n, E), np.nan, np.float32))
    for i in range(n):
        for j in range(P):
            col = v[:, i, j]
            x = col.astype(np.float64) if mistake == 'NaN member counted' else col[np.isfinite(col)].astype(np.float64)
            c = x.size
            out['count'][i, j] = c
            if c == 0:
                continue
            mean = x.sum() / c
            out['mean'][i, j] = mean
            if c > 1:
                with np.errstate(invalid='ignore'):
                    out['spread'][i, j] = np.sqrt(((x - mean) ** 2).sum() / (c if mistake == 'population variance' else c - 1))
            lo, hi = x.min(), x.max()
            if mistake == 'min and max start at 0':
                lo, hi = min(lo, 0.0), max(hi, 0.0)
            out['min'][i, j], out['max'][i, j] = lo, hi
            for e in range(E):
                if thr_col[e] != j:
                    continue
                with np.errstate(invalid='ignore'):
                    above = (x >= np.float32(thr_val[e])) if mistake == '>= for >' else (x > np.float32(thr_val[e]))
                out['prob'][i, e] = above.sum() / (M if mistake == 'prob over M' else c)
    return out


def same(a, b):
    """Equal arrays, a NaN equal to a NaN, and a float32 +0 equal to -0 told apart from nothing else."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))


def matches(got, expected):
    """Every output named in `expected` equals it exactly."""
    return all(same(np.asarray(got[k]), expected[k]) for k in expected)


def against_numpy(values, ref):
    """The Welford result `ref` (ensemble_reference on `values` [M, n, P], all finite) against numpy's own fp64 two-pass mean and std(ddof=1), per
    statistic: (error, bar, welford_vs_rounded), each the largest over the columns of max |difference| / the column's max |two-pass| (the products
    differ by nine orders of magnitude).  error: ref against the two-pass fp64 result.  The bar comes from the number formats alone, computed here:
    the result is stored as float32, so the two-pass result rounded to float32 already deviates from the fp64 one by `rounding`; bar = 4 x rounding,
    the project's factor for a reference's own rounding.  welford_vs_rounded: float32(two-pass) against ref, printed beside them: it is 0 wherever
    Welford's fp64 state and the two-pass fp64 result round to the same float32, which is why it cannot itself be the bar of a comparison with an
    fp64 number."""
    v = np.asarray(values, dtype=np.float64)
    out = {}
    for key, two in (('mean', v.mean(axis=0)), ('spread', v.std(axis=0, ddof=1))):
        top = np.abs(two).max(axis=0)
        got, rounded = ref[key].astype(np.float64), two.astype(np.float32).astype(np.float64)
        worst = lambda a, b: float((np.abs(a - b).max(axis=0) / top).max())
        out[key] = (worst(got, two), 4.0 * worst(rounded, two), worst(rounded, got))
    return out
