"""Window extremes and means in time (csrc/dpn_extreme.inc): the column table of a request ('T:max', 'speed:max', 'T:mean'),
its host checks, and the numpy restatement of what dpn_extreme_scan, dpn_extreme_begin and dpn_extreme_refine define.

The network is continuous in time and its forward returns the exact d/dt of every field.  The maximum (minimum) of a product over a window of hours
is found by a coarse scan of K + 1 nodes, one fields-only forward each, and then by bisection on the sign of d/dt around the best node: round 0 probes
the best node itself and chooses the side, every later round halves the bracket, one forward with the Jacobian per round.  The window mean is the
trapezoid sum of the scan nodes in fp64.  `scan_reference`, `begin_reference` and `refine_reference` perform the kernels' operations in their order,
one rounding per operation, so the device state agrees with them bit for bit; `extremes_reference` drives them over any callable in place of the
network: for tests without a GPU, and for users without one.  Nothing here runs in the device path except the column table and check_request.
"""
from collections import namedtuple

import numpy as np

from . import diagnostics
from .ensemble import ENSEMBLE_PRODUCTS

MAX, MIN, MEAN = 0, 1, 2                                      # DPN_EXT_MAX, _MIN, _MEAN (include/dpn_hip.h)
OK, BAD_SCAN, STOPPED, AT_START, AT_END = 0, 1, 2, 3, 4      # DPN_EXT_*: a column's status
SENSES = {'max': MAX, 'min': MIN, 'mean': MEAN}
PRODUCTS = diagnostics.VARIABLES + ('speed',)                 # what a column may name; their ids are the ensemble's (28..33 and 25)
_IDS = {name: ENSEMBLE_PRODUCTS.index(name) for name in PRODUCTS}
MAX_COLUMNS = 32                                              # DPN_EXT_MAX_COLUMNS
MAX_REFINE = 32
MAX_SCAN_STEPS = 4096                                         # the cap on K: a scan node is two launches per chunk
MIN_SCAN_HOURS = 2.0 ** -10                                   # 32 halvings of it stay above the spacing of fp64 hours: a bracket closes on a face only
MISTAKES = ('min_sign', 'tie_takes_later', 'bracket_off_by_one', 'best_not_kept', 'speed_slope_drops_v', 'mean_end_weights', 'face_not_detected')

Request = namedtuple('Request', 'names ids senses t0 dt K R')
# a physics table under which a normalised field is the physical one: analytic evaluators hand out_n = the value, jac_n[:, k, 2] = its d/dt
Identity = namedtuple('Identity', 'mean std clip_lo clip_hi clip_on sq_on sq_add')
IDENTITY = Identity((0.0,) * 6, (1.0,) * 6, (0.0,) * 6, (0.0,) * 6, (0,) * 6, (0,) * 6, (0.0,) * 6)


def parse_columns(columns):
    """(names, ids, senses) of a request's columns: a sequence of 'product:sense' strings, or one string of them joined by commas ('T:max,T:min');
    product one of PRODUCTS, sense one of max, min, mean; repeats and order kept.  KeyError: an unknown product or sense, a column without a sense, no
    column.  ValueError: more than MAX_COLUMNS."""
    if isinstance(columns, str):
        columns = [c for c in columns.split(',') if c]
    names, ids, senses = [], [], []
    for col in columns:
        name, sep, sense = str(col).partition(':')
        if not sep or name not in _IDS or sense not in SENSES:
            raise KeyError('extremes column %r: PRODUCT:SENSE, product one of %s, sense one of %s' % (col, ', '.join(PRODUCTS), ', '.join(SENSES)))
        names.append('%s:%s' % (name, sense))
        ids.append(_IDS[name])
        senses.append(SENSES[sense])
    if not names:
        raise KeyError('no extremes column named; PRODUCT:SENSE, product one of %s, sense one of %s' % (', '.join(PRODUCTS), ', '.join(SENSES)))
    if len(names) > MAX_COLUMNS:
        raise ValueError('%d extremes columns; at most %d in one request' % (len(names), MAX_COLUMNS))
    return names, ids, senses


def refined_columns(senses):
    """The columns that are refined, in request order: the max / min ones."""
    return [c for c, s in enumerate(senses) if s != MEAN]


def node_hour(t0, dt, k):
    """The hour of scan node k: t0 + (double)k * dt, two fp64 roundings (host and kernels form the same expression)."""
    return np.float64(t0) + np.asarray(k, dtype=np.float64) * np.float64(dt)


def check_clock(word, window, scan_hours=1.0, refine=10, hours_top=24):
    """The window, scan-step and round rules of a time-window request, as check_request states them, for extremes and spells alike: -> (t0, dt, K,
    R).  Every refusal is a ValueError whose text begins with `word` ('extremes', 'spells')."""
    try:
        t0, t1 = (float(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError('%s: window = (first hour, last hour), got %r' % (word, window))
    top = float(hours_top)
    if not (np.isfinite(t0) and np.isfinite(t1) and 0.0 <= t0 < t1 <= top):
        raise ValueError('%s: window %r must satisfy 0 <= t0 < t1 <= %g hours (one field sample\'s window)' % (word, window, top))
    step = float(scan_hours)
    if not (np.isfinite(step) and step >= MIN_SCAN_HOURS):
        raise ValueError('%s: scan_hours must be finite and at least 2**-10 hours, got %r' % (word, scan_hours))
    K = int(round((t1 - t0) / step))
    if not 1 <= K <= MAX_SCAN_STEPS:
        raise ValueError('%s: window %r in scan steps of %r hours is %d steps; 1..%d' % (word, window, scan_hours, K, MAX_SCAN_STEPS))
    dt = step if node_hour(t0, step, K) == t1 else (t1 - t0) / K
    while node_hour(t0, dt, K) > t1:
        dt = float(np.nextafter(dt, 0.0))
    if isinstance(refine, bool) or int(refine) != refine or not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError('%s: refine must be a whole number of rounds in 0..%d, got %r' % (word, MAX_REFINE, refine))
    return t0, float(dt), K, int(refine)


def check_request(columns, window, scan_hours=1.0, refine=10, hours_top=24):
    """The host checks of a request, once, before anything is launched: -> Request(names, ids, senses, t0, dt, K, R).  window = (t0, t1) hours inside
    [0, hours_top] (one field sample's window, input_time_step * input_time_step_nums), t1 > t0; K = round((t1 - t0) / scan_hours) >= 1 scan steps,
    at most MAX_SCAN_STEPS; dt = scan_hours when K of them end on t1, otherwise (t1 - t0) / K, shortened by single fp64 steps until node K does not
    pass t1 (a node beyond the window's end would leave the coarse cube); R = refine in 0..MAX_REFINE, whole.  KeyError: an unknown column name
    (parse_columns); ValueError: everything else."""
    names, ids, senses = parse_columns(columns)
    return Request(names, ids, senses, *check_clock('extremes', window, scan_hours, refine, hours_top))


def new_state(n_columns, n, dtype=np.float32, fill=0):
    """The state of a chunk of n points and C columns, every array [C, n]: best_v (dtype), best_t, acc, lo, hi fp64, best_k, status int32.  The scan's
    node 0 sets what it reads; `fill` is what the rest holds until then."""
    f64 = lambda: np.full((n_columns, n), fill, dtype=np.float64)
    i32 = lambda: np.full((n_columns, n), fill, dtype=np.int32)
    return {'best_v': np.full((n_columns, n), fill, dtype=dtype), 'best_t': f64(), 'best_k': i32(), 'acc': f64(), 'status': i32(), 'lo': f64(), 'hi': f64()}


def products_reference(out_n, jac_n, physics, with_clip, ids, n, dtype=np.float32, mistakes=()):
    """(x, s) [len(ids), n]: the value and the slope in time (up to a positive factor) of the products `ids` as the kernels form them.  out_n [n, 6]:
    every column reads the same rows (the scan; jac_n may be None, s is then 0); out_n [len(ids) * n, 6], jac_n [.., 6, 3]: column r reads rows
    r * n .. (r + 1) * n (the probes).  The residual body's val and J (diagnostics.denorm_reference, with_clip as dpn_diagnostics_out takes it),
    speed = sqrt(u * u + v * v) with slope u * J[0][2] + v * J[1][2], a variable's slope J[k][2]; a row with a NaN among its six out_n is NaN."""
    dt = np.dtype(dtype).type
    out_n = np.asarray(out_n, dtype=np.float32 if dt is np.float32 else np.float64).reshape(-1, 6)
    rows = out_n.shape[0]
    if rows not in (n, len(ids) * n):
        raise ValueError('out_n has %d rows; %d (shared) or %d (one block per column)' % (rows, n, len(ids) * n))
    jn = np.zeros((rows, 6, 3), dtype=out_n.dtype) if jac_n is None else np.asarray(jac_n, dtype=out_n.dtype).reshape(rows, 6, 3)
    if dt is np.float32:
        val, _, J = diagnostics.denorm_reference(out_n, jn, physics, with_clip, dtype)
    else:
        val, J = _denorm_wide(out_n, jn, physics, with_clip, dt)
    poisoned = np.isnan(out_n).any(axis=1)
    x, s = np.empty((len(ids), n), dtype=val.dtype), np.empty((len(ids), n), dtype=val.dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for r, i in enumerate(ids):
            sl = slice(r * n, (r + 1) * n) if rows != n or len(ids) == 1 else slice(0, n)
            if i == _IDS['speed']:
                u, v = val[sl, 0], val[sl, 1]
                xv = np.sqrt(u * u + v * v)
                sv = u * J[sl, 0, 2] if 'speed_slope_drops_v' in mistakes else u * J[sl, 0, 2] + v * J[sl, 1, 2]
            else:
                xv, sv = val[sl, i - 28], J[sl, i - 28, 2]
            x[r], s[r] = np.where(poisoned[sl], np.nan, xv), sv
    return x, s


def _denorm_wide(o, jn, physics, with_clip, dt):
    """diagnostics.denorm_reference for inputs that are not float32 (a truth evaluated in fp64): val [n, 6], J [n, 6, 3], the same expressions in `dt`
    without the cast of the inputs to float32."""
    val, J = np.empty(o.shape, dtype=dt), np.empty(jn.shape, dtype=dt)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(6):
            std, mean = dt(physics.std[k]), dt(physics.mean[k])
            v = o[:, k].astype(dt) * std + mean
            dv = np.full_like(v, std)
            if physics.sq_on[k]:
                dv = dt(2.0) * v * std
                v = v * v + dt(physics.sq_add[k])
            m = np.ones_like(v)
            if with_clip and physics.clip_on[k]:
                lo, hi = dt(physics.clip_lo[k]), dt(physics.clip_hi[k])
                m = ((v >= lo) & (v <= hi)).astype(dt)
                v = np.fmin(np.fmax(v, lo), hi)
            val[:, k] = v
            J[:, k] = jn[:, k].astype(dt) * (m * dv)[:, None]
    return val, J


def scan_reference(x, state, senses, k, K, mistakes=()):
    """dpn_extreme_scan's fold of node k's values x [C, n] into `state` (not modified) -> the new state.  Per column: sticky status, a value that is
    not finite -> BAD_SCAN and nothing else; node 0 sets best_v, best_k, acc = 0.5 x; later nodes replace on strictly better (a tie keeps the
    earlier node) and add (k == K ? 0.5 : 1.0) * (double)x to acc."""
    st = {key: a.copy() for key, a in state.items()}
    x = np.asarray(x)
    live = np.ones(x.shape, dtype=bool) if k == 0 else state['status'] == OK
    fin = np.isfinite(x)
    st['status'] = np.where(live & ~fin, BAD_SCAN, np.where(live & (k == 0), OK, state['status'])).astype(np.int32)
    upd = live & fin
    xd = x.astype(np.float64)
    w_end = np.float64(1.0 if 'mean_end_weights' in mistakes else 0.5)
    if k == 0:
        st['best_v'] = np.where(upd, x, state['best_v']).astype(state['best_v'].dtype)
        st['best_k'] = np.where(upd, 0, state['best_k']).astype(np.int32)
        st['acc'] = np.where(upd, w_end * xd, state['acc'])
        return st
    sense = np.asarray(senses).reshape(-1, 1)
    with np.errstate(invalid='ignore'):
        if 'tie_takes_later' in mistakes:
            up, down = x >= state['best_v'], x <= state['best_v']
        else:
            up, down = x > state['best_v'], x < state['best_v']
        if 'min_sign' in mistakes:
            down = up
    better = upd & (((sense == MAX) & up) | ((sense == MIN) & down))
    st['best_v'] = np.where(better, x, state['best_v']).astype(state['best_v'].dtype)
    st['best_k'] = np.where(better, k, state['best_k']).astype(np.int32)
    w = w_end if k == K else np.float64(1.0)
    st['acc'] = np.where(upd, state['acc'] + w * xd, state['acc'])
    return st


def begin_reference(state, senses, K, t0, dt, mistakes=()):
    """dpn_extreme_begin -> (the new state, m [Cr, n]: the hour of every refined column's first probe).  A mean column: best_v = acc / K cast once, NaN
    under a non-zero status, best_t = lo = hi = NaN.  A max / min column: the bracket [node best_k - 1, node best_k + 1] clamped to the window,
    best_t = m = the hour of node best_k; under BAD_SCAN everything NaN and m = t0."""
    st = {key: a.copy() for key, a in state.items()}
    nan = np.float64(np.nan)
    ms = []
    for c, sense in enumerate(senses):
        ok = state['status'][c] == OK
        if sense == MEAN:
            with np.errstate(invalid='ignore', over='ignore'):
                mean = (state['acc'][c] / np.float64(K)).astype(state['best_v'].dtype)
            st['best_v'][c] = np.where(ok, mean, np.nan)
            st['best_t'][c], st['lo'][c], st['hi'][c] = nan, nan, nan
            continue
        kb = np.where(ok, state['best_k'][c], 0).astype(np.int64)
        left = 0 if 'bracket_off_by_one' in mistakes else 1
        klo, khi = np.maximum(kb - left, 0), np.minimum(kb + 1, K)
        m = np.where(ok, node_hour(t0, dt, kb), np.float64(t0))
        st['lo'][c] = np.where(ok, node_hour(t0, dt, klo), nan)
        st['hi'][c] = np.where(ok, node_hour(t0, dt, khi), nan)
        st['best_t'][c] = np.where(ok, m, nan)
        st['best_v'][c] = np.where(ok, state['best_v'][c], np.nan)
        ms.append(m)
    n = state['status'].shape[1]
    return st, (np.stack(ms) if ms else np.empty((0, n)))


def refine_reference(g, s, state, senses, rnd, t0, dt, mistakes=()):
    """One dpn_extreme_refine launch: g, s [Cr, n] the probes' values and slopes (products_reference on the forward with the Jacobian at the probes),
    rnd the round -> (the new state, (m_next [Cr, n], moved [Cr, n] bool): the hours the probes' sampler inputs were rewritten at, where moved)."""
    st = {key: a.copy() for key, a in state.items()}
    cols = refined_columns(senses)
    n = state['status'].shape[1]
    m_next, moved = np.full((len(cols), n), np.nan), np.zeros((len(cols), n), dtype=bool)
    for r, c in enumerate(cols):
        live = state['status'][c] == OK
        lo, hi, kb = state['lo'][c], state['hi'][c], state['best_k'][c]
        with np.errstate(invalid='ignore', over='ignore'):
            m = node_hour(t0, dt, kb) if rnd == 0 else lo + np.float64(0.5) * (hi - lo)
            fin = np.isfinite(g[r]) & np.isfinite(s[r])
            is_max = senses[c] == MAX
            if 'min_sign' in mistakes:
                is_max = True
            better = g[r] > state['best_v'][c] if is_max else g[r] < state['best_v'][c]
            if 'best_not_kept' in mistakes:
                better = np.ones(n, dtype=bool)
            later = s[r] > 0 if senses[c] == MAX else s[r] < 0
        go = live & fin
        st['best_v'][c] = np.where(go & better, g[r], state['best_v'][c]).astype(state['best_v'].dtype)
        st['best_t'][c] = np.where(go & better, m, state['best_t'][c])
        lo2, hi2 = np.where(go & later, m, lo), np.where(go & ~later, m, hi)
        st['lo'][c], st['hi'][c] = lo2, hi2
        face = go & (lo2 == hi2)
        if 'face_not_detected' in mistakes:
            face = np.zeros(n, dtype=bool)
        status = np.where(live & ~fin, STOPPED, np.where(face, np.where(kb == 0, AT_START, AT_END), state['status'][c]))
        st['status'][c] = status.astype(np.int32)
        moved[r] = go & ~face
        with np.errstate(invalid='ignore'):
            m_next[r] = np.where(moved[r], lo2 + np.float64(0.5) * (hi2 - lo2), np.nan)
    return st, (m_next, moved)


def results_of(state, names):
    """The result dict of a finished state: value [n, C] (best_v), hour, lo, hi [n, C] fp64, status [n, C] int32 -- rows, the state transposed."""
    return {'names': list(names), 'value': state['best_v'].T.copy(), 'hour': state['best_t'].T.copy(), 'lo': state['lo'].T.copy(),
            'hi': state['hi'].T.copy(), 'status': state['status'].T.copy()}


def extremes_reference(evaluate, n, columns, window, scan_hours=1.0, refine=10, physics=IDENTITY, with_clip=False, hours_top=24, dtype=np.float32,
                       _mistakes=()):
    """InterfacePhysics.extremes_at with a callable in place of the network: evaluate(hours [m] fp64, points [m] int) -> (out_n [m, 6], jac_n [m, 6, 3]),
    the normalised fields of `physics` (default: the fields themselves) and their Jacobian at point points[j], hour hours[j]; only jac_n[:, :, 2],
    d/dt, is read.  Same host checks (check_request), same kernels (their restatements, in `dtype`: float32 is what the device computes, float64
    serves as a truth), same outputs: {'names', 'value' [n, C], 'hour', 'lo', 'hi' [n, C] fp64, 'status' [n, C] int32}, plus 'scan' [K + 1, n, C], the
    values of the scan nodes.  K + 1 calls for the scan, R + 1 for the refinement (rows ordered [refined column][point])."""
    req = check_request(columns, window, scan_hours, refine, hours_top)
    C, cols = len(req.ids), refined_columns(req.senses)
    pts = np.arange(n)
    state = new_state(C, n, dtype)
    scan = np.empty((req.K + 1, n, C), dtype=dtype)
    for k in range(req.K + 1):
        out_n, _ = evaluate(np.full(n, node_hour(req.t0, req.dt, k)), pts)
        x, _ = products_reference(out_n, None, physics, with_clip, req.ids, n, dtype)
        scan[k] = x.T
        state = scan_reference(x, state, req.senses, k, req.K, _mistakes)
    state, m = begin_reference(state, req.senses, req.K, req.t0, req.dt, _mistakes)
    if cols:
        ids_r = [req.ids[c] for c in cols]
        for rnd in range(req.R + 1):
            out_n, jac_n = evaluate(m.reshape(-1), np.tile(pts, len(cols)))
            g, s = products_reference(out_n, jac_n, physics, with_clip, ids_r, n, dtype, _mistakes)
            state, (m_next, moved) = refine_reference(g, s, state, req.senses, rnd, req.t0, req.dt, _mistakes)
            m = np.where(moved, m_next, m)
    return dict(results_of(state, req.names), scan=scan)
