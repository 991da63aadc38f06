"""Neighbourhood verification on lattices against gridded analyses (csrc/dpn_nbhd.inc): the scales of a request, the ctypes
structs, the reader of an analysis file and the host restatement of what dpn_nbhd_stage, dpn_nbhd_fold and dpn_nbhd_finish define, in numpy.

The fractions skill score (FSS, Roberts & Lean 2008) compares, per threshold, the fraction of event nodes in a square window around every node
of the forecast with that of the analysis, over windows of growing width: FSS = 1 - sum (Pf - Po)^2 / (sum Pf^2 + sum Po^2).  It is formed for the
model and for its baseline, the interpolated coarse forecast, per lead hour and over all hours, and the smallest scale at which each reaches
0.5 + f_o / 2 (the score of a forecast that is useful at that scale) is reported.  A case (forecast date) becomes event masks, the masks integer
summed-area tables, the tables window fractions, and their squares are folded in one fixed order into a state that stays on the device.  The
three `*_reference` functions perform the same operations in the same order on np.float64, one rounding per operation, so the kernels agree with
them bit for bit.  Nothing here runs in inference but the request checks and the reader."""
from ctypes import Structure, c_void_p

import numpy as np

from .verification import ABOVE, MAX_THRESHOLDS

MAX_SCALES = 8                                                             # DPN_NBHD_MAX_SCALES
DEFAULT_SCALES = (1, 3, 5, 9, 17, 33)                                      # the window widths of the inference loop when none are named
LANES = 64                                                              # the strided folds of dpn_nbhd_fold: one per lane of a wave
SUMS = ('sum_fo2', 'sum_f2', 'sum_o2', 'sum_bo2', 'sum_b2')                # the five fp64 sums [nt, E, K], in the order of a row partial
STATE_FIELDS = SUMS + ('windows', 'n_valid', 'n_f', 'n_b', 'n_o')          # DpnNbhdState, in its order: fp64 [nt, E, K], then int64 [nt, E, K] and [nt, E]
SCALE_FIELDS = ('fss', 'base_fss', 'windows')                              # of a table: [.., K]
OUT_FIELDS = SCALE_FIELDS + ('freq_f', 'freq_b', 'freq_o', 'fbias', 'base_fbias', 'useful', 'count', 'skilful_scale', 'base_skilful_scale')     # DpnNbhdOut
OUT_DTYPES = dict({k: np.float32 for k in OUT_FIELDS}, windows=np.int64, count=np.int64, skilful_scale=np.int32, base_skilful_scale=np.int32)
RESULT_KEYS = ('names', 'thresholds', 'scales', 'hour', 'all')             # of verify_lattice's dict


class DpnNbhdState(Structure):
    """include/dpn_hip.h DpnNbhdState: the ten arrays of a neighbourhood state."""
    _fields_ = [(n, c_void_p) for n in STATE_FIELDS]


class DpnNbhdOut(Structure):
    """include/dpn_hip.h DpnNbhdOut: the twelve destinations of one table of dpn_nbhd_finish."""
    _fields_ = [(n, c_void_p) for n in OUT_FIELDS]


def check_scales(scales):
    """scales: the window WIDTHS of a request in lattice nodes -- odd integers >= 1 (a window is centred on its node), strictly ascending, 1..8 of
    them, e.g. (1, 3, 5, 9, 17, 33).  Returns the half-widths r = (width - 1) / 2 that the kernels take.  ValueError: none, more than 8, a width
    that is even, below 1, not an integer or past 2^31 - 1, widths that do not ascend strictly."""
    try:
        w = np.atleast_1d(np.asarray(scales, dtype=np.float64)).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError('scales %r: odd window widths in lattice nodes, e.g. 1,3,5,9,17,33' % (scales,))
    if not 1 <= w.size <= MAX_SCALES:
        raise ValueError('%d scales; 1 to %d window widths in one request' % (w.size, MAX_SCALES))
    if not bool(np.all(np.isfinite(w) & (w == np.floor(w)) & (w >= 1) & (w < 2.0 ** 31))) or bool(np.any(w.astype(np.int64) % 2 == 0)):
        raise ValueError('scales %s: every window width must be an odd integer >= 1 (the window is centred on its node)' % (w.tolist(),))
    if bool(np.any(np.diff(w) <= 0)):
        raise ValueError('scales %s: the window widths must ascend strictly' % (w.tolist(),))
    return [int(v) // 2 for v in w]


def read_analysis(source, products):
    """The analysis file of the inference loop: `source` is the path of an .npz (or a mapping) with names [P'], hours [H] (inside a sample's window)
    and analysis [M, H, P', ny, nx] (M cases in the order of the sample source, on the fine grid's nodes, physical units, NaN = none).  Returns
    dict(hours fp64 [H], analysis [M, H, P, ny, nx] fp32 with the columns of `products` in their order).  ValueError: a missing key, shapes that do
    not fit; KeyError: a product the file does not hold."""
    if not isinstance(source, dict):
        with np.load(source, allow_pickle=False) as z:
            source = {k: z[k] for k in z.files}
    missing = [k for k in ('names', 'hours', 'analysis') if k not in source]
    if missing:
        raise ValueError('gridded analysis: missing %s (names [P], hours [H], analysis [M, H, P, ny, nx])' % ', '.join(missing))
    hours = np.asarray(source['hours'], dtype=np.float64)
    held = [str(n) for n in np.asarray(source['names']).reshape(-1)]
    an = np.asarray(source['analysis'])
    if hours.ndim != 1 or hours.size == 0:
        raise ValueError('gridded analysis: hours %s must be [H]' % (hours.shape,))
    if an.ndim != 5 or an.shape[1:3] != (hours.size, len(held)) or 0 in an.shape or an.dtype.kind != 'f':
        raise ValueError('gridded analysis: analysis %s %s must be floating point [M, %d, %d, ny, nx]' % (an.shape, an.dtype, hours.size, len(held)))
    for name in products:
        if name not in held:
            raise KeyError('the gridded analysis holds %s, not %r' % (', '.join(held), name))
    cols = [held.index(name) for name in products]
    return dict(hours=hours, analysis=np.ascontiguousarray(an[:, :, cols], dtype=np.float32))


def nbhd_state_zeros(nt, E, K):
    """A zeroed state of nt hours, E thresholds and K scales, as a dict of numpy arrays by DpnNbhdState's names."""
    st = {k: np.zeros((nt, E, K), dtype=np.float64) for k in SUMS}
    st['windows'] = np.zeros((nt, E, K), dtype=np.int64)
    st.update({k: np.zeros((nt, E), dtype=np.int64) for k in ('n_valid', 'n_f', 'n_b', 'n_o')})
    return st


def _event(z, thr, side):
    with np.errstate(invalid='ignore'):
        return z > np.float32(thr) if side == ABOVE else z < np.float32(thr)


def nbhd_stage_reference(x, b, o, thresholds):
    """dpn_nbhd_stage over a whole lattice: forecast values x, baseline values b and analysis o, each [nt, P, ny, nx] float32; thresholds =
    (thr_col, thr_val, thr_side).  Returns mask [nt, E, ny, nx] uint8: bit 0 valid & ev(x), bit 1 valid & ev(b), bit 2 valid & ev(o), bit 3 valid,
    a node of a column being valid when x, b and o are all finite there."""
    x, b, o = (np.asarray(v, dtype=np.float32) for v in (x, b, o))
    thr_col, thr_val, thr_side = thresholds
    if x.ndim != 4 or b.shape != x.shape or o.shape != x.shape:
        raise ValueError('x, b, o must be [nt, P, ny, nx], got %s, %s, %s' % (x.shape, b.shape, o.shape))
    if not 1 <= len(thr_col) <= MAX_THRESHOLDS:
        raise ValueError('%d thresholds; 1 to %d' % (len(thr_col), MAX_THRESHOLDS))
    nt, _, ny, nx = x.shape
    mask = np.zeros((nt, len(thr_col), ny, nx), dtype=np.uint8)
    for e, (j, thr, side) in enumerate(zip(thr_col, thr_val, thr_side)):
        valid = np.isfinite(x[:, j]) & np.isfinite(b[:, j]) & np.isfinite(o[:, j])
        bits = [valid & _event(v[:, j], thr, side) for v in (x, b, o)] + [valid]
        mask[:, e] = sum((bit.astype(np.uint8) << np.uint8(k)) for k, bit in enumerate(bits))
    return mask


def nbhd_table_reference(mask):
    """The summed-area tables of mask planes [.., ny, nx] uint8: S [.., ny + 1, nx + 1, 4] int32, exclusive (row 0 and column 0 are zero), the
    counts of bits 0..3 (f, b, o, valid) interleaved."""
    mask = np.asarray(mask, dtype=np.uint8)
    counts = np.stack([(mask >> np.uint8(k)) & np.uint8(1) for k in range(4)], axis=-1).astype(np.int32)
    S = np.zeros(mask.shape[:-2] + (mask.shape[-2] + 1, mask.shape[-1] + 1, 4), dtype=np.int32)
    S[..., 1:, 1:, :] = counts.cumsum(axis=-3, dtype=np.int32).cumsum(axis=-2, dtype=np.int32)
    return S


def _strided_fold(v):
    """The two-level fold of a wave over the last axis of v [.., n]: lane l adds, from zero, the entries l, l + 64, .. in that order; then the
    lane results are added to lane 0's in lane order (a lane without an entry holds zero)."""
    n = v.shape[-1]
    pad = (-n) % LANES
    if pad:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,), dtype=v.dtype)], axis=-1)
    v = v.reshape(v.shape[:-1] + (-1, LANES))
    acc = np.zeros(v.shape[:-2] + (LANES,), dtype=v.dtype)
    for s in range(v.shape[-2]):
        acc = acc + v[..., s, :]
    total = acc[..., 0]
    for l in range(1, LANES):
        total = total + acc[..., l]
    return total


def nbhd_window_counts(S, r):
    """The four counts [.., ny, nx, 4] int32 of the windows of half-width r, clamped to the plane, from tables S [.., ny + 1, nx + 1, 4]."""
    ny, nx = S.shape[-3] - 1, S.shape[-2] - 1
    iy, ix = np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64)
    y0, y1 = np.maximum(iy - r, 0)[:, None], np.minimum(iy + r + 1, ny)[:, None]
    x0, x1 = np.maximum(ix - r, 0)[None, :], np.minimum(ix + r + 1, nx)[None, :]
    return S[..., y1, x1, :] - S[..., y0, x1, :] - S[..., y1, x0, :] + S[..., y0, x0, :]


def nbhd_fold_reference(state, mask, radius, p0=0, n_planes=None):
    """dpn_nbhd_fold for ONE staged case: planes p0 .. p0 + n_planes (default: to the last) of mask [nt, E, ny, nx], plane = it * E + e, at the K
    half-widths `radius`, folded into `state` (a dict as nbhd_state_zeros makes it; changed in place).  Returns the scratch of the launch: (S
    [np, ny + 1, nx + 1, 4] int32, part [np, K, ny, 5] fp64, rows [np, K, ny] int32).  Per window with c_valid > 0, in fp64, one rounding per
    operation: V = c_valid; Pf = c_f / V; Pb = c_b / V; Po = c_o / V; the terms (Pf - Po)^2, Pf^2, Po^2, (Pb - Po)^2, Pb^2 and one window; the
    nodes of a row fold over ix and the rows over iy as `_strided_fold` states; the case's total is added to the state with one addition per
    sum, the plane totals S[ny, nx] to n_f, n_b, n_o, n_valid."""
    mask = np.asarray(mask, dtype=np.uint8)
    nt, E, ny, nx = mask.shape
    K = len(radius)
    planes = mask.reshape(nt * E, ny, nx)
    n_planes = nt * E - p0 if n_planes is None else n_planes
    if p0 < 0 or n_planes <= 0 or p0 + n_planes > nt * E:
        raise ValueError('planes %d .. %d of %d' % (p0, p0 + n_planes, nt * E))
    S = nbhd_table_reference(planes[p0:p0 + n_planes])
    part = np.zeros((n_planes, K, ny, 5), dtype=np.float64)
    rows = np.zeros((n_planes, K, ny), dtype=np.int32)
    for k, r in enumerate(radius):
        c = nbhd_window_counts(S, int(r))
        counted = c[..., 3] > 0
        V = np.where(counted, c[..., 3], 1).astype(np.float64)
        Pf, Pb, Po = (np.where(counted, c[..., q].astype(np.float64) / V, 0.0) for q in (0, 1, 2))
        a, g = Pf - Po, Pb - Po
        for q, term in enumerate((a * a, Pf * Pf, Po * Po, g * g, Pb * Pb)):
            part[:, k, :, q] = _strided_fold(term)
        rows[:, k] = _strided_fold(counted.astype(np.int32))
    flat = {key: state[key].reshape(nt * E, K) for key in SUMS + ('windows',)}
    for q, key in enumerate(SUMS):
        flat[key][p0:p0 + n_planes] = flat[key][p0:p0 + n_planes] + _strided_fold(part[..., q])
    flat['windows'][p0:p0 + n_planes] += _strided_fold(rows.astype(np.int64))
    for q, key in enumerate(('n_f', 'n_b', 'n_o', 'n_valid')):
        state[key].reshape(nt * E)[p0:p0 + n_planes] += S[:, ny, nx, q]
    return S, part, rows


def _table(st):
    """One table from state arrays whose leading axes are the table's ([.., K] and [..])."""
    nan = np.float32(np.nan)
    nv, nf, nb, no = (st[k] for k in ('n_valid', 'n_f', 'n_b', 'n_o'))
    V, F, B, O = (v.astype(np.float64) for v in (nv, nf, nb, no))
    out = {'count': nv.astype(np.int64), 'windows': st['windows'].astype(np.int64)}
    with np.errstate(divide='ignore', invalid='ignore'):
        freq_o = O / V
        useful = 0.5 + freq_o * 0.5
        out['freq_f'] = np.where(nv != 0, (F / V).astype(np.float32), nan)
        out['freq_b'] = np.where(nv != 0, (B / V).astype(np.float32), nan)
        out['freq_o'] = np.where(nv != 0, freq_o.astype(np.float32), nan)
        out['fbias'] = np.where(no != 0, (F / O).astype(np.float32), nan)
        out['base_fbias'] = np.where(no != 0, (B / O).astype(np.float32), nan)
        out['useful'] = np.where(nv != 0, useful.astype(np.float32), nan)
        for name, err, own in (('fss', 'sum_fo2', 'sum_f2'), ('base_fss', 'sum_bo2', 'sum_b2')):
            den = st[own] + st['sum_o2']
            score = 1.0 - st[err] / den
            out[name] = np.where(den != 0.0, score.astype(np.float32), nan)
            reached = (nv != 0)[..., None] & (den != 0.0) & (score >= useful[..., None])
            first = np.where(reached.any(axis=-1), reached.argmax(axis=-1), -1).astype(np.int32)
            out['skilful_scale' if name == 'fss' else 'base_skilful_scale'] = first
    return {k: np.ascontiguousarray(out[k], dtype=OUT_DTYPES[k]) for k in OUT_FIELDS}


def nbhd_finish_reference(state):
    """dpn_nbhd_finish: {'hour': table, 'all': table}; a table is a dict by OUT_FIELDS -- fss, base_fss fp32 and windows int64 [.., K]; freq_f,
    freq_b, freq_o, fbias, base_fbias, useful fp32, count int64 and skilful_scale, base_skilful_scale int32 [..] -- with the leading axes [nt, E]
    (hour) and [E] (all: the state's entries added over it = 0 .. nt - 1 in that order).  fss = 1 - sum_fo2 / (sum_f2 + sum_o2); base_fss from
    sum_bo2 and sum_b2; freq_. = n_. / n_valid; fbias = n_f / n_o; base_fbias = n_b / n_o; useful = 0.5 + freq_o * 0.5; each cast to float32
    once, NaN where its denominator is 0; the skilful scales are the smallest k whose fp64 score is defined and >= the fp64 useful, or -1."""
    pooled = {}
    for key in STATE_FIELDS:
        acc = state[key][0].copy()
        for it in range(1, state[key].shape[0]):
            acc = acc + state[key][it]
        pooled[key] = acc
    return {'hour': _table(state), 'all': _table(pooled)}
