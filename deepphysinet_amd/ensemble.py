"""Ensemble statistics over field samples (csrc/dpn_ensemble.inc): the product names of the ensemble calls, the threshold table
and the host restatement of what dpn_ensemble_accumulate + dpn_ensemble_finish define, in numpy.

The members of a lagged ensemble (forecasts from different initialisation dates that cover the same window) or of a perturbed one are folded one by
one into a state that stays on the device: per point and product a count, Welford's running mean and sum of squared deviations in fp64, minimum,
maximum, and per threshold the number of members above it.  After the last member the state becomes mean, spread (the sample standard deviation,
ddof = 1), min, max, count and the exceedance probabilities.  A member whose value is not finite is skipped in that column alone.  `ensemble_reference`
performs the same operations in the same order, one rounding per operation, so the kernels agree with it bit for bit.  Nothing here runs in inference.
"""
import numpy as np

from . import diagnostics

ENSEMBLE_PRODUCTS = diagnostics.PRODUCTS + diagnostics.VARIABLES          # ids 0..27: dpn_diagnostics_out's; 28..33: u, v, p, T, q, rho
MAX_THRESHOLDS = 16                                                        # DPN_ENS_MAX_THRESHOLDS
_IDS = {name: i for i, name in enumerate(ENSEMBLE_PRODUCTS)}


def ensemble_ids(names):
    """The ids (column selectors of dpn_ensemble_accumulate) of a sequence of product names, repeats and order kept; KeyError on an unknown name."""
    ids = []
    for n in names:
        if n not in _IDS:
            raise KeyError('ensemble product %r: one of %s' % (n, ', '.join(ENSEMBLE_PRODUCTS)))
        ids.append(_IDS[n])
    if not ids:
        raise KeyError('no ensemble product named; known: %s' % ', '.join(ENSEMBLE_PRODUCTS))
    return ids


def reads_jacobian(ids):
    """Whether a selection needs the forward kernel's Jacobian: ids 0..24 and 27 read it (25 speed, 26 rel_humidity and the six variables do not)."""
    return any(i <= 24 or i == 27 for i in ids)


def reads_coriolis(ids):
    """Whether a selection reads the Coriolis parameter f: abs_vorticity (19) alone does."""
    return 19 in ids


def check_thresholds(products, thresholds):
    """thresholds: None or a dict name -> value or list of values, every name one of `products`.  Returns (thr_col, thr_val): for every threshold the
    column of `products` it applies to (the first with that name) and its value, in the products' order, then in the listed order.  ValueError: a name
    that is not in the request, more than 16 thresholds in all, a value that is not finite."""
    products = list(products)
    thresholds = dict(thresholds or {})
    for name in thresholds:
        if name not in products:
            raise ValueError('threshold on %r, which is not among the requested products %s' % (name, products))
    thr_col, thr_val = [], []
    for j, name in enumerate(products):
        if name not in thresholds or products.index(name) != j:
            continue
        for v in np.atleast_1d(np.asarray(thresholds[name], dtype=np.float64)).reshape(-1):
            with np.errstate(over='ignore'):
                finite = np.isfinite(v) and np.isfinite(np.float32(v))          # the kernel compares in float32
            if not finite:
                raise ValueError('threshold %r on %r is not finite' % (v, name))
            thr_col.append(j)
            thr_val.append(float(np.float32(v)))
    if len(thr_col) > MAX_THRESHOLDS:
        raise ValueError('%d thresholds; at most %d in one request' % (len(thr_col), MAX_THRESHOLDS))
    return thr_col, thr_val


def ensemble_reference(values, thr_col=(), thr_val=()):
    """dpn_ensemble_accumulate over the members of values [M, n, P] (float32, members in order), then dpn_ensemble_finish: a dict of mean, spread, min,
    max [n, P] float32, count [n, P] int32 and prob [n, E] float32.  Per column, a member x that is not finite changes nothing; otherwise, every
    operation an fp64 operation rounded on its own: c = count + 1; d = x - mean; mean = mean + d / c; m2 = m2 + d * (x - mean); count = c; min and max
    start at the first finite member; exceed[e] += x > thr_val[e] (strict, compared in float32).  Finish: mean, min, max NaN when count == 0, spread =
    sqrt(m2 / (count - 1)) NaN when count < 2, prob[e] = exceed[e] / count[thr_col[e]] NaN when that count is 0; each cast to float32 once."""
    v = np.asarray(values, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError('values must be [M, n, P], got %s' % (v.shape,))
    M, n, P = v.shape
    thr_col = [int(c) for c in thr_col]
    thr_val = np.asarray(thr_val, dtype=np.float32).reshape(-1)
    E = len(thr_col)
    count = np.zeros((n, P), dtype=np.int32)
    mean, m2 = np.zeros((n, P), dtype=np.float64), np.zeros((n, P), dtype=np.float64)
    vmin, vmax = np.zeros((n, P), dtype=np.float32), np.zeros((n, P), dtype=np.float32)
    exceed = np.zeros((n, E), dtype=np.int32)
    for m in range(M):
        x = v[m]
        ok = np.isfinite(x)
        xd = np.where(ok, x, np.float32(0)).astype(np.float64)
        c = count + 1
        d = xd - mean
        new_mean = mean + d / c.astype(np.float64)
        new_m2 = m2 + d * (xd - new_mean)
        first = ok & (c == 1)
        with np.errstate(invalid='ignore'):                    # fminf / fmaxf as comparisons: of +0 and -0 the earlier member's stays
            vmin = np.where(first | (ok & (x < vmin)), x, vmin)
            vmax = np.where(first | (ok & (x > vmax)), x, vmax)
        mean, m2, count = np.where(ok, new_mean, mean), np.where(ok, new_m2, m2), np.where(ok, c, count).astype(np.int32)
        for e in range(E):
            with np.errstate(invalid='ignore'):
                exceed[:, e] += (ok[:, thr_col[e]] & (x[:, thr_col[e]] > thr_val[e])).astype(np.int32)
    nan = np.float32(np.nan)
    with np.errstate(invalid='ignore', divide='ignore'):
        spread = np.sqrt(m2 / (count - 1).astype(np.float64)).astype(np.float32)
        prob = (exceed.astype(np.float64) / count[:, thr_col].astype(np.float64)).astype(np.float32) if E else np.zeros((n, 0), dtype=np.float32)
    none = count == 0
    out = dict(mean=np.where(none, nan, mean.astype(np.float32)), spread=np.where(count < 2, nan, spread), min=np.where(none, nan, vmin),
               max=np.where(none, nan, vmax), count=count)
    out['prob'] = np.where(count[:, thr_col] == 0, nan, prob) if E else prob
    return out
