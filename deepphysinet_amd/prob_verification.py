"""Probabilistic verification of ensembles against observations (csrc/dpn_pverify.inc): the request checks, the ctypes
structs and the host restatement of what dpn_pverify_stage, dpn_pverify_case, dpn_pverify_pool and dpn_pverify_finish define, in numpy.

A case is one forecast date with M members.  The members' forecast and baseline values are staged member by member into two planes [M, P, N] that
stay on the device; after the last member the case is folded into a resident state: per point and column the number of pairs whose M forecast
values, M baseline values and report are all finite, the sums of CRPS, fair CRPS, error of the ensemble mean, its square and the ensemble variance,
the rank histogram, and per threshold the reliability table (per probability level k / M: pairs, and pairs whose report is an event) -- each for the
forecast (side 0) and the baseline (side 1).  States pool over groups of points in one fixed order (verification.pool_plan), and a state becomes
CRPS, fair CRPS, bias, RMSE, spread, spread / skill, the rank histogram, the CRPS skill against the baseline, and per threshold the Brier score
with reliability, resolution and uncertainty, the Brier skill score, the ROC area and the reliability diagram.  The `*_reference` functions perform
the same operations in the same order on np.float64, one rounding per operation, so the kernels agree with them bit for bit.  Nothing here runs in
inference but the request checks."""
from ctypes import Structure, c_void_p

import numpy as np

from . import verification as VF
from .verification import ABOVE, BELOW, LANES, _event, check_thresholds, pool_plan  # (re-exported: the request is checked by the same code)

MAX_MEMBERS = 64                                                           # DPN_PV_MAX_MEMBERS
MAX_COLUMNS, MAX_THRESHOLDS = VF.MAX_COLUMNS, VF.MAX_THRESHOLDS
MAX_ELEMENTS = 2 ** 31 - 1                                                 # of any one array of a state or of the planes

STATE_F64 = ('sum_crps', 'sum_fair', 'sum_d', 'sum_d2', 'sum_var')
STATE_FIELDS = ('n',) + STATE_F64 + ('rank', 'rel')                        # DpnPVerifyState, in its order
SIDE_SCORES = ('crps', 'fair_crps', 'bias', 'rmse', 'spread', 'spread_skill')
SCORES = SIDE_SCORES + tuple('base_' + k for k in SIDE_SCORES) + ('crpss', 'fair_crpss')
HISTS = ('rank_hist', 'base_rank_hist')
SIDE_THRESHOLD_SCORES = ('brier', 'reliability', 'resolution', 'bss', 'roc_area')
THRESHOLD_SCORES = SIDE_THRESHOLD_SCORES + tuple('base_' + k for k in SIDE_THRESHOLD_SCORES) + ('uncertainty',)
DIAGRAMS = ('rel_n', 'rel_o', 'base_rel_n', 'base_rel_o')
OUT_FIELDS = ('count',) + SCORES + HISTS + THRESHOLD_SCORES + DIAGRAMS     # DpnPVerifyOut, in its order
RESULT_KEYS = ('names', 'thresholds', 'members', 'point')                  # of verify_ensemble_at's dict: no grouping may take these names


class DpnPVerifyState(Structure):
    """include/dpn_hip.h DpnPVerifyState: the eight arrays of a probabilistic verification state."""
    _fields_ = [(n, c_void_p) for n in STATE_FIELDS]


class DpnPVerifyOut(Structure):
    """include/dpn_hip.h DpnPVerifyOut: the thirty-two destinations of dpn_pverify_finish."""
    _fields_ = [(n, c_void_p) for n in OUT_FIELDS]


def check_members(M):
    """M as an int; ValueError unless 1 <= M <= 64."""
    if int(M) != M or not 1 <= int(M) <= MAX_MEMBERS:
        raise ValueError('verify_ensemble: %r members per case; 1 to %d' % (M, MAX_MEMBERS))
    return int(M)


def state_elements(n_total, P, E, M):
    """The element counts of the arrays of a state and of one plane: dict(n, sums, rank, rel, plane)."""
    N, M = int(n_total), int(M)
    return dict(n=P * N, sums=2 * P * N, rank=2 * P * (M + 1) * N, rel=E * 4 * (M + 1) * N, plane=M * P * N)


def check_state_size(n_total, P, E, M):
    """ValueError when an array of the state (or a plane) of this request would pass 2^31 - 1 elements, or a size is out of range."""
    M = check_members(M)
    if int(n_total) < 1 or not 1 <= P <= MAX_COLUMNS or not 0 <= E <= MAX_THRESHOLDS:
        raise ValueError('ProbVerifyState: %d points, %d products (1..%d), %d thresholds (0..%d)' % (n_total, P, MAX_COLUMNS, E, MAX_THRESHOLDS))
    for name, count in state_elements(n_total, P, E, M).items():
        if count > MAX_ELEMENTS:
            raise ValueError('ProbVerifyState: %d points, %d products, %d thresholds, %d members: %s would hold %d elements, more than 2^31 - 1'
                             % (n_total, P, E, M, name, count))


def prob_verify_state_zeros(n_total, P, E, M):
    """A zeroed state of n_total points, P columns, E thresholds and M members, as a dict of numpy arrays by DpnPVerifyState's names: n [P, N]
    int32, the five fp64 sums [2, P, N], rank [2, P, M + 1, N] int32, rel [E, 2, 2, M + 1, N] int32."""
    check_state_size(n_total, P, E, M)
    N = int(n_total)
    st = {'n': np.zeros((P, N), dtype=np.int32), 'rank': np.zeros((2, P, M + 1, N), dtype=np.int32),
          'rel': np.zeros((E, 2, 2, M + 1, N), dtype=np.int32)}
    st.update({k: np.zeros((2, P, N), dtype=np.float64) for k in STATE_F64})
    return st


def planes_zeros(n_total, P, M):
    """The two staging planes [M, P, n_total] float32 (forecast, baseline)."""
    return np.zeros((M, P, int(n_total)), dtype=np.float32), np.zeros((M, P, int(n_total)), dtype=np.float32)


def pverify_stage_reference(plane_f, plane_b, x, b, member, first=0):
    """dpn_pverify_stage for ONE member's chunk: its forecast values x and baseline values b, each [n, P] float32 (what dpn_fields_out /
    dpn_diagnostics_out write for out_n, and for coord_data in its place), into plane_f, plane_b [M, P, N] at [member, :, first .. first + n]."""
    x, b = (np.asarray(v, dtype=np.float32) for v in (x, b))
    M, P, N = plane_f.shape
    if x.ndim != 2 or x.shape[1] != P or b.shape != x.shape or plane_b.shape != plane_f.shape:
        raise ValueError('x, b must be [n, %d], got %s, %s' % (P, x.shape, b.shape))
    if not 0 <= member < M or first < 0 or first + x.shape[0] > N or x.shape[0] < 1:
        raise ValueError('member %d of %d, points %d .. %d of %d' % (member, M, first, first + x.shape[0], N))
    plane_f[member, :, first:first + x.shape[0]] = x.T
    plane_b[member, :, first:first + x.shape[0]] = b.T
    return plane_f, plane_b


def pverify_case_reference(state, plane_f, plane_b, o, thr_col=(), thr_val=(), thr_side=(), first=0):
    """dpn_pverify_case for ONE case: the staged planes [M, P, N] at points first .. first + n against the reports o [n, P] float32, folded into
    `state` (a dict as prob_verify_state_zeros makes it; changed in place and returned).  A (point, column) pair counts only when all M forecast
    values, all M baseline values and the report are finite.  Per counted pair and side, in fp64, one rounding per operation, every sum from 0.0
    with m ascending: a = sum |X_m - O|; s = sum X_m; g = sum_{i < k} |X_i - X_k| (i outside, k inside); mean = s / M; d = mean - O; v = sum
    (X_m - mean)^2; crps = a / M - g / (M * M); fair = a / M - g / (M * (M - 1)), a when M == 1; var = v / (M - 1), 0 when M == 1; the five sums
    grow by crps, fair, d, d * d, var; rank[lt + eq // 2] += 1 with lt = #{x_m < o}, eq = #{x_m == o} in float32; per threshold on the column
    rel[.., 0, k] += 1 for k = the number of event members, rel[.., 1, k] += 1 when the report is an event."""
    o = np.asarray(o, dtype=np.float32)
    M, P, N = plane_f.shape
    if o.ndim != 2 or o.shape[1] != P or plane_b.shape != plane_f.shape or state['n'].shape != (P, N) or state['rank'].shape[2] != M + 1:
        raise ValueError('o must be [n, %d] and the state that of planes %s, got %s' % (P, plane_f.shape, o.shape))
    n = o.shape[0]
    sl = slice(int(first), int(first) + n)
    if first < 0 or sl.stop > N or n < 1:
        raise ValueError('points %d .. %d of a state of %d' % (first, sl.stop, N))
    sides = (plane_f[:, :, sl], plane_b[:, :, sl])                                              # [M, P, n] each
    oT = o.T
    ok = np.isfinite(oT) & np.isfinite(sides[0]).all(axis=0) & np.isfinite(sides[1]).all(axis=0)
    o_ = np.where(ok, oT, np.float32(0))
    O = o_.astype(np.float64)
    Md = np.float64(M)
    state['n'][:, sl] += ok.astype(np.int32)
    pts = np.arange(sl.start, sl.stop)
    for side, x in enumerate(sides):
        x = np.where(ok, x, np.float32(0))
        X = x.astype(np.float64)
        a, s = np.zeros_like(O), np.zeros_like(O)
        for m in range(M):
            a = a + np.abs(X[m] - O)
            s = s + X[m]
        g = np.zeros_like(O)
        for i in range(M):
            for k in range(i + 1, M):
                g = g + np.abs(X[i] - X[k])
        mean = s / Md
        d = mean - O
        v = np.zeros_like(O)
        for m in range(M):
            r = X[m] - mean
            v = v + r * r
        am = a / Md
        crps = am - g / (Md * Md)
        fair = am - g / (Md * (Md - 1.0)) if M > 1 else a
        var = v / (Md - 1.0) if M > 1 else np.zeros_like(O)
        for key, inc in zip(STATE_F64, (crps, fair, d, d * d, var)):
            cur = state[key][side][:, sl]
            state[key][side][:, sl] = np.where(ok, cur + inc, cur)
        bin_ = (x < o_).sum(axis=0) + (x == o_).sum(axis=0) // 2                                  # [P, n]
        for j in range(P):
            sel = ok[j]
            np.add.at(state['rank'][side, j], (bin_[j][sel], pts[sel]), 1)
        for t, (j, thr, sd) in enumerate(zip(thr_col, thr_val, thr_side)):
            sel = ok[j]
            k = _event(x[:, j], thr, sd).sum(axis=0)
            eo = _event(o_[j], thr, sd)
            np.add.at(state['rel'][t, side, 0], (k[sel], pts[sel]), 1)
            np.add.at(state['rel'][t, side, 1], (k[sel & eo], pts[sel & eo]), 1)
    return state


def pverify_pool_reference(state, order, seg_start, thr_col=()):
    """dpn_pverify_pool: the states of N points -> the states of G = len(seg_start) - 1 groups (a new dict of the same layout).  Per group, column,
    side and fp64 field, fold l of 64 adds, from 0.0, the points order[seg_start[g] + l], order[.. + l + 64], .. in that order, then the 64
    results are added to fold 0's in the order of l; the int32 fields are added over the group.  An order entry outside 0..N - 1 is skipped."""
    order, seg_start = np.asarray(order, dtype=np.int64), np.asarray(seg_start, dtype=np.int64)
    P, N = state['n'].shape
    G = seg_start.size - 1
    if G < 1 or seg_start[0] != 0 or seg_start[-1] != N or bool(np.any(np.diff(seg_start) < 0)) or order.shape != (N,):
        raise ValueError('seg_start must be non-decreasing from 0 to N = %d and order [N]' % N)
    E, M1 = state['rel'].shape[0], state['rank'].shape[2]
    out = prob_verify_state_zeros(G, P, E, M1 - 1)
    for g in range(G):
        seg = order[seg_start[g]:seg_start[g + 1]]
        acc = {k: np.zeros((2, P, LANES), dtype=np.float64) for k in STATE_F64}
        for r in range(0, seg.size, LANES):
            idx = seg[r:r + LANES]
            valid = (idx >= 0) & (idx < N)
            at = np.where(valid, idx, 0)
            for k in STATE_F64:
                cur = acc[k][:, :, :idx.size]
                acc[k][:, :, :idx.size] = np.where(valid, cur + state[k][:, :, at], cur)
        for k in STATE_F64:
            total = acc[k][:, :, 0]
            for l in range(1, LANES):
                total = total + acc[k][:, :, l]
            out[k][:, :, g] = total
        ok = seg[(seg >= 0) & (seg < N)]
        out['n'][:, g] = state['n'][:, ok].sum(axis=1, dtype=np.int32)
        out['rank'][..., g] = state['rank'][..., ok].sum(axis=-1, dtype=np.int32)
        for t in range(len(thr_col)):
            out['rel'][t, ..., g] = state['rel'][t][..., ok].sum(axis=-1, dtype=np.int32)
    return out


def pverify_finish_reference(state, thr_col=()):
    """dpn_pverify_finish over a whole state: a dict by OUT_FIELDS -- count [N, P] int32, the fourteen scores [N, P] float32, rank_hist and
    base_rank_hist [N, P, M + 1] int32, the eleven threshold scores [N, E] float32 and the four diagram tables [N, E, M + 1] int32 -- by the
    formulas of include/dpn_hip.h, each float cast to float32 once, NaN where a score is not defined."""
    nan = np.float32(np.nan)
    n = state['n']
    P, N = n.shape
    M1 = state['rank'].shape[2]
    M = M1 - 1
    Md = np.float64(M)
    c = n.astype(np.float64)
    any_ = n > 0
    out = {'count': np.ascontiguousarray(n.T)}
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for side, pre in enumerate(('', 'base_')):
            mse, mvar = state['sum_d2'][side] / c, state['sum_var'][side] / c
            rmse = np.sqrt(mse)
            sc = {'crps': state['sum_crps'][side] / c, 'fair_crps': state['sum_fair'][side] / c, 'bias': state['sum_d'][side] / c, 'rmse': rmse,
                  'spread': np.sqrt(mvar)}
            for k, v in sc.items():
                out[pre + k] = np.ascontiguousarray(np.where(any_, v.astype(np.float32), nan).T)
            ss = (np.sqrt(((Md + 1.0) / Md) * mvar) / rmse).astype(np.float32)
            out[pre + 'spread_skill'] = np.ascontiguousarray(np.where(any_ & (M > 1) & (rmse != 0), ss, nan).T)
            out[pre + 'rank_hist'] = np.ascontiguousarray(state['rank'][side].transpose(2, 0, 1))
        for key, field in (('crpss', 'sum_crps'), ('fair_crpss', 'sum_fair')):
            v = (1.0 - state[field][0] / state[field][1]).astype(np.float32)
            out[key] = np.ascontiguousarray(np.where(any_ & (state[field][1] != 0), v, nan).T)
        E = len(thr_col)
        for k in THRESHOLD_SCORES:
            out[k] = np.zeros((N, E), dtype=np.float32)
        for k in DIAGRAMS:
            out[k] = np.zeros((N, E, M1), dtype=np.int32)
        for t, j in enumerate(thr_col):
            cn, Nd, have = n[j], c[j], any_[j]
            for side, pre in enumerate(('', 'base_')):
                nk, ok = state['rel'][t, side, 0], state['rel'][t, side, 1]                      # [M + 1, N]
                out[pre + 'rel_n'][:, t, :] = nk.T
                out[pre + 'rel_o'][:, t, :] = ok.T
                events = ok.sum(axis=0, dtype=np.int32)
                bacc = np.zeros(N)
                for k in range(M1):
                    p = np.float64(k) / Md
                    q = 1.0 - p
                    bacc = bacc + (ok[k].astype(np.float64) * (q * q) + (nk[k] - ok[k]).astype(np.float64) * (p * p))
                obar = events.astype(np.float64) / Nd
                racc, sacc = np.zeros(N), np.zeros(N)
                for k in range(M1):
                    p = np.float64(k) / Md
                    nd = nk[k].astype(np.float64)
                    f = ok[k].astype(np.float64) / nd
                    u, v = p - f, f - obar
                    racc = np.where(nk[k] > 0, racc + nd * (u * u), racc)
                    sacc = np.where(nk[k] > 0, sacc + nd * (v * v), sacc)
                area, above = np.zeros(N), np.zeros(N, dtype=np.int32)
                for k in range(M, -1, -1):
                    area = area + (nk[k] - ok[k]).astype(np.float64) * (above.astype(np.float64) + (above + ok[k]).astype(np.float64))
                    above = above + ok[k]
                brier, unc = bacc / Nd, obar * (1.0 - obar)
                out[pre + 'brier'][:, t] = np.where(have, brier.astype(np.float32), nan)
                out[pre + 'reliability'][:, t] = np.where(have, (racc / Nd).astype(np.float32), nan)
                out[pre + 'resolution'][:, t] = np.where(have, (sacc / Nd).astype(np.float32), nan)
                out[pre + 'bss'][:, t] = np.where(have & (unc != 0), (1.0 - brier / unc).astype(np.float32), nan)
                roc = (area / ((2.0 * events.astype(np.float64)) * (cn - events).astype(np.float64))).astype(np.float32)
                out[pre + 'roc_area'][:, t] = np.where(have & (events > 0) & (cn - events > 0), roc, nan)
                if side == 0:
                    out['uncertainty'][:, t] = np.where(have, unc.astype(np.float32), nan)
    return {k: out[k] for k in OUT_FIELDS}
