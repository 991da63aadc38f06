"""Forecast verification against observations (csrc/dpn_verify.inc): the product names of the verification calls, the
threshold table, the plan of a pooling, the ctypes structs and the host restatement of what dpn_verify_accumulate, dpn_verify_pool and
dpn_verify_finish define, in numpy.

The cases (forecast dates) are folded one by one into a state that stays on the device: per point and column the number of (forecast, baseline,
report) triples that are all finite, Welford's co-moments of forecast and report, the error sums of the forecast and of the baseline -- the
interpolated coarse forecast, the sampler's coord_data -- and per threshold the contingency counts of both.  States pool over groups of points (per
station, per lead hour, over everything) in one fixed order, and a state becomes bias, MAE, RMSE, largest error, correlation, the baseline's three
and the MSE skill against it, and POD, FAR, CSI, frequency bias and ETS per threshold.  The three `*_reference` functions perform the same
operations in the same order on np.float64, one rounding per operation, so the kernels agree with them bit for bit.  Nothing here runs in inference
but the request checks."""
from ctypes import Structure, c_void_p

import numpy as np

from . import diagnostics
from .ensemble import ENSEMBLE_PRODUCTS

VERIFY_PRODUCTS = diagnostics.VARIABLES + ('speed', 'rel_humidity')       # the value products: ids 28..33, 25, 26 of the ensemble's table
MAX_COLUMNS, MAX_THRESHOLDS = 16, 16                                       # DPN_VERIFY_MAX_COLUMNS, DPN_VERIFY_MAX_THRESHOLDS
ABOVE, BELOW = 0, 1                                                        # DPN_VERIFY_ABOVE, DPN_VERIFY_BELOW
SIDES = {'above': ABOVE, 'below': BELOW}
LANES = 64                                                                 # the strided folds of dpn_verify_pool: one per lane of a wave
_IDS = {name: ENSEMBLE_PRODUCTS.index(name) for name in VERIFY_PRODUCTS}

STATE_F64 = ('mean_f', 'mean_o', 'm2_f', 'm2_o', 'c_fo', 'sum_d', 'sum_ad', 'sum_d2', 'sum_e', 'sum_ae', 'sum_e2')
STATE_FIELDS = ('n',) + STATE_F64 + ('max_ad', 'cont')                     # DpnVerifyState, in its order
SCORES = ('bias', 'mae', 'rmse', 'max_abs_error', 'corr', 'base_bias', 'base_mae', 'base_rmse', 'skill')
TABLE_SCORES = ('pod', 'far', 'csi', 'fbias', 'ets')
THRESHOLD_SCORES = TABLE_SCORES + tuple('base_' + k for k in TABLE_SCORES)
OUT_FIELDS = ('count',) + SCORES + THRESHOLD_SCORES                        # DpnVerifyOut, in its order
RESULT_KEYS = ('names', 'thresholds', 'point')                             # of verify_at's dict: no grouping may take these names


class DpnVerifyState(Structure):
    """include/dpn_hip.h DpnVerifyState: the fourteen product-major arrays of a verification state."""
    _fields_ = [(n, c_void_p) for n in STATE_FIELDS]


class DpnVerifyOut(Structure):
    """include/dpn_hip.h DpnVerifyOut: the twenty destinations of dpn_verify_finish, rows [n][P] and [n][E]."""
    _fields_ = [(n, c_void_p) for n in OUT_FIELDS]


def verify_ids(names):
    """The ids (column selectors of dpn_verify_accumulate) of a sequence of product names, repeats and order kept; KeyError on a name that is not a
    value product (a derivative, a vorticity: the reports hold no such thing) and on an empty list."""
    ids = []
    for n in names:
        if n not in _IDS:
            raise KeyError('verification product %r: one of %s' % (n, ', '.join(VERIFY_PRODUCTS)))
        ids.append(_IDS[n])
    if not ids:
        raise KeyError('no verification product named; known: %s' % ', '.join(VERIFY_PRODUCTS))
    return ids


def _threshold_items(spec):
    """(side, value) pairs of one name's entry: V, [V, ...] (above), ('below' | 'above', V or [V, ...]), or a list that mixes numbers and such pairs."""
    if isinstance(spec, (tuple, list)) and len(spec) > 0 and isinstance(spec[0], str):
        if len(spec) != 2 or spec[0] not in SIDES:
            raise ValueError("threshold %r: ('below', value) or ('above', value)" % (spec,))
        return [(SIDES[spec[0]], v) for v in np.atleast_1d(np.asarray(spec[1], dtype=np.float64)).reshape(-1)]
    if isinstance(spec, (tuple, list)):
        return [p for item in spec for p in _threshold_items(item)]
    return [(ABOVE, v) for v in np.atleast_1d(np.asarray(spec, dtype=np.float64)).reshape(-1)]


def check_thresholds(products, thresholds):
    """thresholds: None or a dict name -> value or list of values (the event is `above`: strictly greater), or name -> ('below', value(s)) (strictly
    less); every name one of `products`.  Returns (thr_col, thr_val, thr_side): for every threshold the column of `products` it applies to (the first
    with that name), its value and its side, in the products' order, then in the listed order.  ValueError: a name that is not in the request, more
    than 16 thresholds in all, a value that is not finite (in float32: the kernel compares there), a malformed entry."""
    products = list(products)
    thresholds = dict(thresholds or {})
    for name in thresholds:
        if name not in products:
            raise ValueError('threshold on %r, which is not among the requested products %s' % (name, products))
    thr_col, thr_val, thr_side = [], [], []
    for j, name in enumerate(products):
        if name not in thresholds or products.index(name) != j:
            continue
        try:
            items = _threshold_items(thresholds[name])
        except (TypeError, ValueError) as err:
            raise ValueError('threshold on %r: %s' % (name, err))
        for side, v in items:
            with np.errstate(over='ignore'):
                finite = np.isfinite(v) and np.isfinite(np.float32(v))
            if not finite:
                raise ValueError('threshold %r on %r is not finite' % (v, name))
            thr_col.append(j)
            thr_val.append(float(np.float32(v)))
            thr_side.append(side)
    if len(thr_col) > MAX_THRESHOLDS:
        raise ValueError('%d thresholds; at most %d in one request' % (len(thr_col), MAX_THRESHOLDS))
    return thr_col, thr_val, thr_side


def pool_plan(groups, n_groups=None):
    """The plan of dpn_verify_pool for `groups`, an int group id >= 0 per point [N]: (order [N] int32, a stable sort of the points by group;
    seg_start [G + 1] int64, the first place of every group in it).  G = n_groups, or the largest id + 1; a group without a point is an empty
    segment.  ValueError: no point, an id that is negative, not an integer or >= n_groups, N >= 2^31."""
    g = np.asarray(groups)
    if g.ndim != 1 or g.size == 0 or g.size >= 2 ** 31:
        raise ValueError('pool_plan: one group id per point, [N] with 0 < N < 2^31, got shape %s' % (g.shape,))
    if g.dtype.kind not in 'iu':
        if g.dtype.kind != 'f' or not bool(np.all(np.isfinite(g) & (g == np.floor(g)))):
            raise ValueError('pool_plan: the group ids must be integers')
    g = g.astype(np.int64)
    if int(g.min()) < 0:
        raise ValueError('pool_plan: a group id is negative (%d)' % int(g.min()))
    G = int(g.max()) + 1 if n_groups is None else int(n_groups)
    if G < 1 or int(g.max()) >= G:
        raise ValueError('pool_plan: group id %d with %d groups' % (int(g.max()), G))
    order = np.argsort(g, kind='stable').astype(np.int32)
    seg_start = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=G))]).astype(np.int64)
    return order, seg_start


GROUPINGS = ('station', 'hour', 'all')                                     # what a report file can be pooled by


def read_observations(source, products):
    """The report file of the inference loop: `source` is the path of an .npz (or a mapping) with lon [S], lat [S] (degrees east, north), hours [H]
    (inside a sample's window), names [P'] and obs [M, H, S, P'] (M cases in the order of the sample source, physical units, NaN = no report).
    Returns dict(lon, lat, hours fp64, obs [M, H, S, P] fp32 with the columns of `products` in their order).  ValueError: a missing key, shapes
    that do not fit; KeyError: a product the file does not hold."""
    if not isinstance(source, dict):
        with np.load(source, allow_pickle=False) as z:
            source = {k: z[k] for k in z.files}
    missing = [k for k in ('lon', 'lat', 'hours', 'names', 'obs') if k not in source]
    if missing:
        raise ValueError('verification reports: missing %s (lon [S], lat [S], hours [H], names [P], obs [M, H, S, P])' % ', '.join(missing))
    lon, lat, hours = (np.asarray(source[k], dtype=np.float64) for k in ('lon', 'lat', 'hours'))
    held = [str(n) for n in np.asarray(source['names']).reshape(-1)]
    obs = np.asarray(source['obs'])
    if lon.ndim != 1 or lat.shape != lon.shape or hours.ndim != 1 or lon.size == 0 or hours.size == 0:
        raise ValueError('verification reports: lon %s and lat %s must be [S], hours %s [H]' % (lon.shape, lat.shape, hours.shape))
    if obs.ndim != 4 or obs.shape[1:] != (hours.size, lon.size, len(held)) or obs.shape[0] == 0 or obs.dtype.kind != 'f':
        raise ValueError('verification reports: obs %s %s must be floating point [M, %d, %d, %d]' % (obs.shape, obs.dtype, hours.size, lon.size, len(held)))
    for name in products:
        if name not in held:
            raise KeyError('verification reports hold %s, not %r' % (', '.join(held), name))
    cols = [held.index(name) for name in products]
    return dict(lon=lon, lat=lat, hours=hours, obs=np.ascontiguousarray(obs[..., cols], dtype=np.float32))


def report_points(reports, by=GROUPINGS):
    """The point list of a report file, point i = h * S + s: (lon [N], lat [N], hours [N], {name: group id per point}) for the names of `by` out
    of GROUPINGS ('station' groups by s, 'hour' by h, 'all' is one group).  ValueError on another name."""
    S, H = reports['lon'].size, reports['hours'].size
    ids = {'station': np.tile(np.arange(S), H), 'hour': np.repeat(np.arange(H), S), 'all': np.zeros(H * S, dtype=np.int64)}
    for name in by:
        if name not in ids:
            raise ValueError('verification grouping %r: one of %s' % (name, ', '.join(GROUPINGS)))
    return np.tile(reports['lon'], H), np.tile(reports['lat'], H), np.repeat(reports['hours'], S), {name: ids[name] for name in by}


def verify_state_zeros(n_total, P, E):
    """A zeroed state of n_total points, P columns and E thresholds, as a dict of numpy arrays by DpnVerifyState's names: n [P, n_total] int32, the
    eleven fp64 arrays, max_ad fp32, cont [E, 6, n_total] int32 (hits, false alarms, misses of the forecast, then of the baseline)."""
    st = {'n': np.zeros((P, n_total), dtype=np.int32), 'max_ad': np.zeros((P, n_total), dtype=np.float32),
          'cont': np.zeros((E, 6, n_total), dtype=np.int32)}
    st.update({k: np.zeros((P, n_total), dtype=np.float64) for k in STATE_F64})
    return st


def _event(z, thr, side):
    with np.errstate(invalid='ignore'):
        return z > np.float32(thr) if side == ABOVE else z < np.float32(thr)


def verify_accumulate_reference(state, x, b, o, thr_col=(), thr_val=(), thr_side=(), first=0):
    """dpn_verify_accumulate for ONE case: forecast values x, baseline values b and reports o, each [n, P] float32, folded into `state` (a dict as
    verify_state_zeros makes it; changed in place and returned) at its points first .. first + n.  A (point, column) pair counts only when x, b and
    o are all finite.  Per counted pair, in fp64, one rounding per operation, X, O, B the three as doubles:
    c = n + 1; df = X - mean_f; mean_f = mean_f + df / c; dq = O - mean_o; mean_o = mean_o + dq / c; m2_f = m2_f + df * (X - mean_f);
    m2_o = m2_o + dq * (O - mean_o); c_fo = c_fo + df * (O - mean_o); d = X - O; sum_d += d; sum_ad += |d|; sum_d2 += d * d; max_ad = the larger of it
    and float32(|d|); e = B - O; sum_e += e; sum_ae += |e|; sum_e2 += e * e; per threshold on the column the six contingency counts, the event
    tested strictly in float32."""
    x, b, o = (np.asarray(v, dtype=np.float32) for v in (x, b, o))
    if x.ndim != 2 or b.shape != x.shape or o.shape != x.shape or state['n'].shape[0] != x.shape[1]:
        raise ValueError('x, b, o must be [n, P] with the P of the state, got %s, %s, %s' % (x.shape, b.shape, o.shape))
    n = x.shape[0]
    sl = slice(int(first), int(first) + n)
    if first < 0 or sl.stop > state['n'].shape[1]:
        raise ValueError('points %d .. %d of a state of %d' % (first, sl.stop, state['n'].shape[1]))
    ok = (np.isfinite(x) & np.isfinite(b) & np.isfinite(o)).T                                    # [P, n]
    X, B, O = (np.where(ok, v.T, np.float32(0)).astype(np.float64) for v in (x, b, o))
    s = {k: state[k][:, sl] for k in STATE_FIELDS if k != 'cont'}
    new = {}
    c = s['n'] + 1
    cd = c.astype(np.float64)
    df = X - s['mean_f']
    new['mean_f'] = s['mean_f'] + df / cd
    dq = O - s['mean_o']
    new['mean_o'] = s['mean_o'] + dq / cd
    new['m2_f'] = s['m2_f'] + df * (X - new['mean_f'])
    new['m2_o'] = s['m2_o'] + dq * (O - new['mean_o'])
    new['c_fo'] = s['c_fo'] + df * (O - new['mean_o'])
    d = X - O
    new['sum_d'] = s['sum_d'] + d
    new['sum_ad'] = s['sum_ad'] + np.abs(d)
    new['sum_d2'] = s['sum_d2'] + d * d
    with np.errstate(over='ignore'):
        ad = np.abs(d).astype(np.float32)
    new['max_ad'] = np.where(ad > s['max_ad'], ad, s['max_ad'])
    e = B - O
    new['sum_e'] = s['sum_e'] + e
    new['sum_ae'] = s['sum_ae'] + np.abs(e)
    new['sum_e2'] = s['sum_e2'] + e * e
    new['n'] = c
    for k, v in new.items():
        state[k][:, sl] = np.where(ok, v, s[k])
    for t, (j, thr, side) in enumerate(zip(thr_col, thr_val, thr_side)):
        ex, eb, eo = (_event(v[:, j], thr, side) for v in (x, b, o))
        for slot, hit in enumerate((ex & eo, ex & ~eo, ~ex & eo, eb & eo, eb & ~eo, ~eb & eo)):
            state['cont'][t, slot, sl] += (ok[j] & hit).astype(np.int32)
    return state


def _merge(A, B):
    """An earlier state A and a later state B (dicts of arrays of one shape, without cont) -> the merged state: B empty: A as it is; A empty: B;
    otherwise Chan's pairwise merge in the order include/dpn_hip.h states."""
    nA, nB = A['n'], B['n']
    n = nA + nB
    out = {'n': n}
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        nd = n.astype(np.float64)
        w = (nA.astype(np.float64) * nB.astype(np.float64)) / nd
        r = nB.astype(np.float64) / nd
        gf = B['mean_f'] - A['mean_f']
        go = B['mean_o'] - A['mean_o']
        out['m2_f'] = (A['m2_f'] + B['m2_f']) + (gf * gf) * w
        out['m2_o'] = (A['m2_o'] + B['m2_o']) + (go * go) * w
        out['c_fo'] = (A['c_fo'] + B['c_fo']) + (gf * go) * w
        out['mean_f'] = A['mean_f'] + gf * r
        out['mean_o'] = A['mean_o'] + go * r
        for k in ('sum_d', 'sum_ad', 'sum_d2', 'sum_e', 'sum_ae', 'sum_e2'):
            out[k] = A[k] + B[k]
    out['max_ad'] = np.where(B['max_ad'] > A['max_ad'], B['max_ad'], A['max_ad'])
    keep_a, take_b = nB == 0, (nA == 0) & (nB != 0)
    return {k: np.where(keep_a, A[k], np.where(take_b, B[k], v)) for k, v in out.items()}


def verify_pool_reference(state, order, seg_start, thr_col=()):
    """dpn_verify_pool: the states of N points -> the states of G = len(seg_start) - 1 groups (a new dict of the same layout).  Per group and column,
    fold l of 64 left-folds the points order[seg_start[g] + l], order[.. + l + 64], .. in that order with `_merge`, then the 64 results are
    left-folded in the order of l; the contingency counts of a threshold are added over the group.  An order entry outside 0..N - 1 is skipped."""
    order, seg_start = np.asarray(order, dtype=np.int64), np.asarray(seg_start, dtype=np.int64)
    P, N = state['n'].shape
    G = seg_start.size - 1
    if G < 1 or seg_start[0] != 0 or seg_start[-1] != N or bool(np.any(np.diff(seg_start) < 0)) or order.shape != (N,):
        raise ValueError('seg_start must be non-decreasing from 0 to N = %d and order [N]' % N)
    keys = [k for k in STATE_FIELDS if k != 'cont']
    out = verify_state_zeros(G, P, state['cont'].shape[0])
    for g in range(G):
        seg = order[seg_start[g]:seg_start[g + 1]]
        if seg.size == 0:
            continue
        lanes = min(LANES, seg.size)
        acc = {k: np.zeros((P, lanes), dtype=state[k].dtype) for k in keys}
        for r in range(0, seg.size, LANES):
            idx = seg[r:r + LANES]
            valid = (idx >= 0) & (idx < N)
            at = np.where(valid, idx, 0)
            nxt = {k: np.zeros((P, lanes), dtype=state[k].dtype) for k in keys}
            for k in keys:
                nxt[k][:, :idx.size] = np.where(valid, state[k][:, at], 0)
            acc = _merge(acc, nxt)
        total = {k: acc[k][:, 0] for k in keys}
        for l in range(1, lanes):
            total = _merge(total, {k: acc[k][:, l] for k in keys})
        for k in keys:
            out[k][:, g] = total[k]
        ok = seg[(seg >= 0) & (seg < N)]
        for t in range(len(thr_col)):
            out['cont'][t, :, g] = state['cont'][t][:, ok].sum(axis=1, dtype=np.int32)
    return out


def _table(h, f, m, n):
    """pod, far, csi, fbias, ets of the counts h, f, m among n pairs (int arrays), float32, NaN where a denominator is 0."""
    nan = np.float32(np.nan)
    h, f, m, N = (v.astype(np.float64) for v in (h, f, m, n))
    hm, hf, hfm = h + m, h + f, (h + f) + m
    with np.errstate(divide='ignore', invalid='ignore'):
        hr = (hf * hm) / N
        den = hfm - hr
        return (np.where(hm != 0, (h / hm).astype(np.float32), nan), np.where(hf != 0, (f / hf).astype(np.float32), nan),
                np.where(hfm != 0, (h / hfm).astype(np.float32), nan), np.where(hm != 0, (hf / hm).astype(np.float32), nan),
                np.where((n > 0) & (den != 0), ((h - hr) / den).astype(np.float32), nan))


def verify_finish_reference(state, thr_col=()):
    """dpn_verify_finish over a whole state: a dict of count [N, P] int32, the nine scores [N, P] float32 and, per threshold, pod, far, csi, fbias,
    ets and their base_ forms [N, E] float32.  With c = count as a double: bias = sum_d / c; mae = sum_ad / c; rmse = sqrt(sum_d2 / c);
    max_abs_error = max_ad; corr = c_fo / sqrt(m2_f * m2_o), NaN below two pairs or when either m2 is 0; base_* from the e sums; skill = 1 - sum_d2 /
    sum_e2, NaN when sum_e2 is 0; every score NaN at count 0; each cast to float32 once."""
    nan = np.float32(np.nan)
    n = state['n']
    c = n.astype(np.float64)
    any_ = n > 0
    out = {'count': np.ascontiguousarray(n.T)}
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        sc = {'bias': (state['sum_d'] / c).astype(np.float32), 'mae': (state['sum_ad'] / c).astype(np.float32),
              'rmse': np.sqrt(state['sum_d2'] / c).astype(np.float32), 'max_abs_error': state['max_ad'],
              'base_bias': (state['sum_e'] / c).astype(np.float32), 'base_mae': (state['sum_ae'] / c).astype(np.float32),
              'base_rmse': np.sqrt(state['sum_e2'] / c).astype(np.float32)}
        corr = (state['c_fo'] / np.sqrt(state['m2_f'] * state['m2_o'])).astype(np.float32)
        skill = (1.0 - state['sum_d2'] / state['sum_e2']).astype(np.float32)
    for k, v in sc.items():
        out[k] = np.ascontiguousarray(np.where(any_, v, nan).T)
    out['corr'] = np.ascontiguousarray(np.where((n > 1) & (state['m2_f'] != 0) & (state['m2_o'] != 0), corr, nan).T)
    out['skill'] = np.ascontiguousarray(np.where(any_ & (state['sum_e2'] != 0), skill, nan).T)
    E, N = len(thr_col), n.shape[1]
    for k in THRESHOLD_SCORES:
        out[k] = np.zeros((N, E), dtype=np.float32)
    for t, j in enumerate(thr_col):
        cont = state['cont'][t]
        for prefix, base in (('', 0), ('base_', 3)):
            for k, v in zip(TABLE_SCORES, _table(cont[base], cont[base + 1], cont[base + 2], n[j])):
                out[prefix + k][:, t] = v
    return out
