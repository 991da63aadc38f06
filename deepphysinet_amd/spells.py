"""Threshold spells in time (csrc/dpn_spell.inc): the column table of a request ('T:below:273.15', 'speed:above:15'), its host
checks, and the numpy restatement of what dpn_spell_scan, dpn_spell_begin, dpn_spell_refine and dpn_spell_finish define.

How long does a product stay above (below) a threshold in a window of hours, from when until when?  The network is continuous in time, so a crossing
is bracketed by the window extremes' coarse scan of K + 1 nodes (one fields-only forward each) and closed by bisection on the sign of value - threshold:
every round halves the scan step of the first entry and the scan step of the last exit, one fields-only forward per round.  The scan also gives the
time in (`hours`) and the integral of the margin (`excess`, degree-hours) of the piecewise-linear series through its nodes; `hours` then has its two
interpolated ends replaced by the refined ones, `excess` stays the scan's clipped trapezoid, as the extremes' mean stays the scan's trapezoid.
`scan_reference`, `begin_reference`, `refine_reference` and `finish_reference` perform the kernels' operations in their order, one rounding per
operation, so the device state agrees with them bit for bit; `spells_reference` drives them over any callable in place of the network.  Nothing here
runs in the device path except the column table and check_request.
"""
from collections import namedtuple

import numpy as np

from . import extremes as X
from .ensemble import ENSEMBLE_PRODUCTS

ABOVE, BELOW = 0, 1                                           # DPN_SPELL_ABOVE, _BELOW (include/dpn_hip.h)
BAD_SCAN, STOPPED, NEVER, HOLDS_AT_START, HOLDS_AT_END = 1, 2, 4, 8, 16      # DPN_SPELL_*: the bits of a column's status
SIDES = {'above': ABOVE, 'below': BELOW}
PRODUCTS = X.PRODUCTS                                         # what a column may name: u, v, p, T, q, rho, speed (ids 28..33 and 25)
MAX_COLUMNS = 16                                              # DPN_SPELL_MAX_COLUMNS
STATE_KEYS = ('prev_x', 'hours', 'excess', 'crossings', 'k_first', 'k_last', 'status', 'part_first', 'part_last', 'f_lo', 'f_hi', 'l_lo', 'l_hi')
_I32 = ('crossings', 'k_first', 'k_last', 'status')
MISTAKES = ('non_strict', 'fractions_swapped', 'part_first_overwritten', 'k_last_not_reset', 'below_not_negated', 'exit_moves_k_last',
            'refine_sides_swapped', 'parts_not_replaced')

Request = namedtuple('Request', 'names ids sides thr t0 dt K R')
IDENTITY = X.IDENTITY


def parse_columns(columns):
    """(names, ids, sides, thr) of a request's columns: a sequence of 'product:side:threshold' strings, or one string of them joined by commas
    ('T:below:273.15,speed:above:15'); product one of PRODUCTS, side above or below, threshold a finite number in the product's unit, rounded to
    float32 once (the kernels compare in float32); repeats and order kept.  KeyError: an unknown product or side, a column without a side or a
    threshold, no column.  ValueError: a threshold that is not a finite float32, more than MAX_COLUMNS."""
    if isinstance(columns, str):
        columns = [c for c in columns.split(',') if c]
    usage = 'PRODUCT:SIDE:THRESHOLD, product one of %s, side one of %s' % (', '.join(PRODUCTS), ', '.join(SIDES))
    names, ids, sides, thr = [], [], [], []
    for col in columns:
        parts = str(col).split(':')
        if len(parts) != 3 or parts[0] not in PRODUCTS or parts[1] not in SIDES or not parts[2].strip():
            raise KeyError('spells column %r: %s' % (col, usage))
        try:
            with np.errstate(over='ignore'):
                value = float(np.float32(float(parts[2])))
        except ValueError:
            raise ValueError('spells column %r: the threshold is not a number' % (col,)) from None
        if not np.isfinite(value):
            raise ValueError('spells column %r: the threshold must be a finite float32' % (col,))
        names.append('%s:%s:%s' % (parts[0], parts[1], parts[2].strip()))
        ids.append(ENSEMBLE_PRODUCTS.index(parts[0]))
        sides.append(SIDES[parts[1]])
        thr.append(value)
    if not names:
        raise KeyError('no spells column named; ' + usage)
    if len(names) > MAX_COLUMNS:
        raise ValueError('%d spells columns; at most %d in one request' % (len(names), MAX_COLUMNS))
    return names, ids, sides, thr


node_hour = X.node_hour


def check_request(columns, window, scan_hours=1.0, refine=10, hours_top=24):
    """The host checks of a request, once, before anything is launched: -> Request(names, ids, sides, thr, t0, dt, K, R).  The window, the scan step
    and the rounds follow extremes.check_request's rules unchanged (window inside [0, hours_top], K = round((t1 - t0) / scan_hours) in
    1..MAX_SCAN_STEPS, node K never past t1, R in 0..MAX_REFINE).  R rounds leave brackets dt / 2**R wide.  KeyError: a malformed column
    (parse_columns); ValueError: everything else."""
    names, ids, sides, thr = parse_columns(columns)
    return Request(names, ids, sides, thr, *X.check_clock('spells', window, scan_hours, refine, hours_top))


def new_state(n_columns, n, dtype=np.float32, fill=0):
    """The state of a chunk of n points and C columns, every array [C, n]: prev_x (dtype); hours, excess, part_first, part_last, f_lo, f_hi, l_lo, l_hi
    fp64; crossings, k_first, k_last, status int32.  The scan's node 0 sets what it reads; `fill` is what the rest holds until then."""
    st = {key: np.full((n_columns, n), fill, dtype=np.int32 if key in _I32 else np.float64) for key in STATE_KEYS}
    st['prev_x'] = np.full((n_columns, n), fill, dtype=dtype)
    return st


def products_reference(out_n, physics, with_clip, ids, n, dtype=np.float32):
    """x [len(ids), n]: the products `ids` as the kernels form them (extremes.products_reference without the Jacobian).  out_n [n, 6]: every column
    reads the same rows (the scan); out_n [len(ids) * n, 6]: column r reads rows r * n .. (r + 1) * n (the probes: ids repeated per probe)."""
    return X.products_reference(out_n, None, physics, with_clip, ids, n, dtype)[0]


def _margin(x, sides, thr, mistakes=()):
    """d(x) [C, n] fp64: (double)x - (double)thr, negated for a below column."""
    dt = x.dtype.type
    d = x.astype(np.float64) - np.array([dt(v) for v in thr], dtype=x.dtype).astype(np.float64).reshape(-1, 1)
    if 'below_not_negated' in mistakes:
        return d
    return np.where(np.asarray(sides).reshape(-1, 1) == BELOW, -d, d)


def _is_in(x, sides, thr, mistakes=()):
    """x [C, n] in: x > thr (above) or x < thr (below), strict, compared in x's own type."""
    t = np.array([x.dtype.type(v) for v in thr], dtype=x.dtype).reshape(-1, 1)
    below = np.asarray(sides).reshape(-1, 1) == BELOW
    if 'below_not_negated' in mistakes:
        below = np.zeros_like(below)
    with np.errstate(invalid='ignore'):
        if 'non_strict' in mistakes:
            return np.where(below, x <= t, x >= t)
        return np.where(below, x < t, x > t)


def scan_reference(x, state, sides, thr, k, dt, mistakes=()):
    """dpn_spell_scan's fold of node k's values x [C, n] into `state` (not modified) -> the new state.  Per column: sticky status, a value that is
    not finite -> BAD_SCAN and nothing else; node 0 sets the state; a later node takes the step from prev_x to x by the signs of the two margins
    (both in, both out, entry, exit: include/dpn_hip.h)."""
    st = {key: a.copy() for key, a in state.items()}
    x = np.asarray(x)
    live = np.ones(x.shape, dtype=bool) if k == 0 else state['status'] == 0
    fin = np.isfinite(x)
    st['status'] = np.where(live & ~fin, BAD_SCAN, np.where(live & (k == 0), 0, state['status'])).astype(np.int32)
    upd = live & fin
    put = lambda key, mask, value: st.__setitem__(key, np.where(mask, value, st[key]).astype(st[key].dtype))
    if k == 0:
        at = np.where(_is_in(x, sides, thr, mistakes), 0, -1)
        for key in ('hours', 'excess', 'part_first', 'part_last', 'crossings'):
            put(key, upd, 0)
        put('k_first', upd, at)
        put('k_last', upd, at)
        put('prev_x', upd, x)
        return st
    dt = np.float64(dt)
    half = np.float64(0.5)
    a, b = _margin(state['prev_x'], sides, thr, mistakes), _margin(x, sides, thr, mistakes)
    pos = (lambda v: v >= 0) if 'non_strict' in mistakes else (lambda v: v > 0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        both, entry, leave = upd & pos(a) & pos(b), upd & ~pos(a) & pos(b), upd & pos(a) & ~pos(b)
        w_in, w_out = b / (b - a) * dt, a / (a - b) * dt
        if 'fractions_swapped' in mistakes:
            w_in, w_out = -a / (b - a) * dt, -b / (a - b) * dt
        put('hours', both, state['hours'] + dt)
        put('excess', both, state['excess'] + half * (a + b) * dt)
        put('hours', entry, state['hours'] + w_in)
        put('excess', entry, state['excess'] + half * b * w_in)
        put('hours', leave, state['hours'] + w_out)
        put('excess', leave, state['excess'] + half * a * w_out)
    put('crossings', entry | leave, state['crossings'] + 1)
    put('k_last', both if 'k_last_not_reset' in mistakes else both | entry, k)
    put('part_last', both if 'k_last_not_reset' in mistakes else both | entry, 0)
    first = entry if 'part_first_overwritten' in mistakes else entry & (state['k_first'] < 0)
    put('k_first', entry & (state['k_first'] < 0), k)
    put('part_first', first, w_in)
    put('part_last', leave, w_out)
    if 'exit_moves_k_last' in mistakes:
        put('k_last', leave, k)
    put('prev_x', upd, x)
    return st


def brackets_of(state, K):
    """(has_entry, has_exit) [C, n] bool: the probes that are refined -- a live column (no BAD_SCAN, STOPPED or NEVER) with k_first >= 1 / k_last < K."""
    live = (state['status'] & (BAD_SCAN | STOPPED | NEVER)) == 0
    return live & (state['k_first'] >= 1), live & (state['k_last'] < K)


def begin_reference(state, K, t0, dt, mistakes=()):
    """dpn_spell_begin -> (the new state, m [2 * C, n]: the hours of the probes, row 2 * c + e, e = 0 entry, 1 exit; t0 without a bracket)."""
    st = {key: a.copy() for key, a in state.items()}
    nan, t0 = np.float64(np.nan), np.float64(t0)
    bad = (state['status'] & BAD_SCAN) != 0
    kf, kl = state['k_first'].astype(np.int64), state['k_last'].astype(np.int64)
    never = ~bad & (kf < 0)
    some = ~bad & ~never
    entry, start = some & (kf >= 1), some & (kf < 1)
    leave, end = some & (kl < K), some & (kl >= K)
    st['hours'], st['excess'] = np.where(bad, nan, state['hours']), np.where(bad, nan, state['excess'])
    st['status'] = (state['status'] | np.where(never, NEVER, 0) | np.where(start, HOLDS_AT_START, 0) | np.where(end, HOLDS_AT_END, 0)).astype(np.int32)
    st['f_lo'] = np.where(entry, node_hour(t0, dt, np.maximum(kf - 1, 0)), np.where(start, t0, nan))
    st['f_hi'] = np.where(entry, node_hour(t0, dt, np.maximum(kf, 0)), np.where(start, t0, nan))
    st['l_lo'] = np.where(leave, node_hour(t0, dt, np.maximum(kl, 0)), np.where(end, node_hour(t0, dt, K), nan))
    st['l_hi'] = np.where(leave, node_hour(t0, dt, np.maximum(kl, 0) + 1), np.where(end, node_hour(t0, dt, K), nan))
    half = np.float64(0.5)
    with np.errstate(invalid='ignore'):
        m_entry = np.where(entry, st['f_lo'] + half * (st['f_hi'] - st['f_lo']), t0)
        m_exit = np.where(leave, st['l_lo'] + half * (st['l_hi'] - st['l_lo']), t0)
    C, n = state['status'].shape
    return st, np.stack([m_entry, m_exit], axis=1).reshape(2 * C, n)


def refine_reference(g, state, sides, thr, K, mistakes=()):
    """One dpn_spell_refine launch: g [2 * C, n] the probes' values (products_reference on the fields-only forward at the probes, ids repeated per
    probe) -> (the new state, (m_next [2 * C, n], moved [2 * C, n] bool): the hours the probes' sampler inputs were rewritten at, where moved)."""
    st = {key: a.copy() for key, a in state.items()}
    C, n = state['status'].shape
    g = np.asarray(g).reshape(C, 2, n)
    has_entry, has_exit = brackets_of(state, K)
    stop = (has_entry & ~np.isfinite(g[:, 0])) | (has_exit & ~np.isfinite(g[:, 1]))
    st['status'] = np.where(stop, state['status'] | STOPPED, state['status']).astype(np.int32)
    half = np.float64(0.5)
    m_next, moved = np.full((C, 2, n), np.nan), np.zeros((C, 2, n), dtype=bool)
    swap = 'refine_sides_swapped' in mistakes
    for e, (lo_key, hi_key, has) in enumerate((('f_lo', 'f_hi', has_entry), ('l_lo', 'l_hi', has_exit))):
        go = has & ~stop
        lo, hi = state[lo_key], state[hi_key]
        with np.errstate(invalid='ignore'):
            m = lo + half * (hi - lo)
            is_in = _is_in(g[:, e], sides, thr, mistakes)
            to_hi = is_in if (e == 0) != swap else ~is_in      # entry: in -> f_hi = m; exit: out -> l_hi = m
            lo2, hi2 = np.where(go & ~to_hi, m, lo), np.where(go & to_hi, m, hi)
            st[lo_key], st[hi_key] = lo2, hi2
            m_next[:, e] = np.where(go, lo2 + half * (hi2 - lo2), np.nan)
        moved[:, e] = go
    return st, (m_next.reshape(2 * C, n), moved.reshape(2 * C, n))


def finish_reference(state, K, t0, dt, mistakes=()):
    """dpn_spell_finish -> the new state: hours with the scan's interpolated ends replaced by the refined ones, each term only where its bracket
    exists; NEVER: hours = excess = 0; BAD_SCAN: nothing.  excess stays the scan's clipped trapezoid."""
    st = {key: a.copy() for key, a in state.items()}
    bad, never = (state['status'] & BAD_SCAN) != 0, (state['status'] & NEVER) != 0
    some = ~bad & ~never
    kf, kl = state['k_first'].astype(np.int64), state['k_last'].astype(np.int64)
    entry, leave = some & (kf >= 1), some & (kl < K)
    h = state['hours']
    with np.errstate(invalid='ignore'):
        if 'parts_not_replaced' not in mistakes:
            h = np.where(entry, h - state['part_first'], h)
            h = np.where(entry, h + (node_hour(t0, dt, np.maximum(kf, 0)) - state['f_hi']), h)
            h = np.where(leave, h - state['part_last'], h)
            h = np.where(leave, h + (state['l_lo'] - node_hour(t0, dt, np.maximum(kl, 0))), h)
    st['hours'] = np.where(never, 0.0, h)
    st['excess'] = np.where(never, 0.0, state['excess'])
    return st


def results_of(state, names):
    """The result dict of a finished state, rows [n, C]: hours, first (= f_hi), last (= l_lo), first_lo (= f_lo), last_hi (= l_hi), excess fp64,
    crossings, status int32 -- the state transposed."""
    t = lambda key: state[key].T.copy()
    return {'names': list(names), 'hours': t('hours'), 'first': t('f_hi'), 'last': t('l_lo'), 'first_lo': t('f_lo'), 'last_hi': t('l_hi'),
            'excess': t('excess'), 'crossings': t('crossings'), 'status': t('status')}


def spells_reference(evaluate, n, columns, window, scan_hours=1.0, refine=10, physics=IDENTITY, with_clip=False, hours_top=24, dtype=np.float32,
                     _mistakes=()):
    """InterfacePhysics.spells_at with a callable in place of the network: evaluate(hours [m] fp64, points [m] int) -> out_n [m, 6] (or a tuple whose
    first entry it is, as extremes_reference's evaluators return), the normalised fields of `physics` (default: the fields themselves) at point
    points[j], hour hours[j].  Same host checks (check_request), same kernels (their restatements, in `dtype`: float32 is what the device computes,
    float64 serves as a truth), same outputs: {'names', 'hours', 'first', 'last', 'first_lo', 'last_hi', 'excess' [n, C] fp64, 'crossings', 'status'
    [n, C] int32}, plus 'scan' [K + 1, n, C], the values of the scan nodes.  K + 1 calls for the scan, R for the refinement (rows ordered
    [column][entry, exit][point]).  `excess` is the scan's clipped trapezoid: the refinement does not change it."""
    req = check_request(columns, window, scan_hours, refine, hours_top)
    C = len(req.ids)
    pts = np.arange(n)
    fields = lambda out: out[0] if isinstance(out, tuple) else out
    state = new_state(C, n, dtype)
    scan = np.empty((req.K + 1, n, C), dtype=dtype)
    for k in range(req.K + 1):
        x = products_reference(fields(evaluate(np.full(n, node_hour(req.t0, req.dt, k)), pts)), physics, with_clip, req.ids, n, dtype)
        scan[k] = x.T
        state = scan_reference(x, state, req.sides, req.thr, k, req.dt, _mistakes)
    state, m = begin_reference(state, req.K, req.t0, req.dt, _mistakes)
    ids2 = [i for i in req.ids for _ in range(2)]
    for _ in range(req.R):
        g = products_reference(fields(evaluate(m.reshape(-1), np.tile(pts, 2 * C))), physics, with_clip, ids2, n, dtype)
        state, (m_next, moved) = refine_reference(g, state, req.sides, req.thr, req.K, _mistakes)
        m = np.where(moved, m_next, m)
    state = finish_reference(state, req.K, req.t0, req.dt, _mistakes)
    return dict(results_of(state, req.names), scan=scan)
