"""Regional statistics in space (csrc/dpn_region.inc): the plan of a region set -- the region-sorted list of the selected
positions of a plane or of a station list --, its host checks, and the numpy restatement of what dpn_region_accumulate and dpn_region_finish define.

A region set over a plane of candidate positions is an int label plane [ny, nx] (-1: in no region, ids 0..R - 1, an id without a point is an empty
region) or a list of R boolean masks, which may overlap (a point in k regions is listed k times).  Only listed points are ever evaluated.  The flat
point list of a request with nt time nodes is time-major, i = it * n_sel + j; point i belongs to cell c = it * R + seg[j] and to group g = i // 64,
and its partial sums go to slot s = g + c, which no other (group, cell) pair shares.  `regions_reference` performs the kernels' operations in their
order, one rounding per operation, partials included, so the device agrees with it bit for bit.  Nothing here runs in inference but the plan builder.
"""
from dataclasses import dataclass

import numpy as np

from .ensemble import MAX_THRESHOLDS

GROUP = 64                                                   # DPN_REG_GROUP
MAX_COLUMNS = 16                                             # DPN_REG_MAX_COLUMNS
assert MAX_THRESHOLDS == 16                                  # DPN_REG_MAX_THRESHOLDS: the ensemble's check_thresholds serves both
FLOAT_OUTPUTS = ('mean', 'total', 'weight', 'min', 'max')
INT_OUTPUTS = ('where_min', 'where_max', 'count')
OUTPUTS = FLOAT_OUTPUTS + INT_OUTPUTS                        # + 'frac': the nine destinations of dpn_region_finish, in DpnRegionOut's order
PARTIALS = (('w', np.float64), ('wx', np.float64), ('count', np.int32), ('vmin', np.float32), ('vmax', np.float32), ('imin', np.int32),
            ('imax', np.int32))                              # + wexc [E, S] fp64: DpnRegionState's order


@dataclass
class RegionPlan:
    """order [n_sel] int64: the plane index iy * nx + ix (or the station index) of entry j, grouped by region, ascending inside a region; seg [n_sel]
    int32: its region, non-decreasing; wgt [n_sel] float32; offs [R + 1] int32: the first entry of every region.  shape: (ny, nx) of the plane, or None
    for a station list; n_candidates: ny * nx, or the number of stations."""
    order: np.ndarray
    seg: np.ndarray
    wgt: np.ndarray
    offs: np.ndarray
    n_regions: int
    shape: tuple
    n_candidates: int

    @property
    def n_sel(self):
        return int(self.order.size)

    def where(self, j):
        """Entries j (where_min / where_max; -1: no counted point) -> the station index [...] of a station plan, or (ix, iy) [..., 2] of a plane; -1
        stays -1."""
        j = np.asarray(j)
        at = np.where(j >= 0, self.order[np.clip(j, 0, self.n_sel - 1)], -1)
        if self.shape is None:
            return at
        nx = self.shape[1]
        return np.where((j >= 0)[..., None], np.stack([at % nx, at // nx], axis=-1), -1)


def _host(a):
    """A numpy view of an array-like or of a torch tensor on any device."""
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def row_latitudes(cfg, y_idx):
    """Degrees north of fine-grid rows y_idx (index units, fractional allowed) in fp64: begin_lat + y * out_res_deg, the inverse of lonlat_to_index."""
    return float(cfg.begin_lat) + np.asarray(y_idx, dtype=np.float64) * float(cfg.out_res_deg)


def area_weights(lat_deg):
    """float32(cos(latitude)), formed in fp64."""
    return np.cos(np.deg2rad(np.asarray(lat_deg, dtype=np.float64))).astype(np.float32)


def n_slots(plan, nt):
    """S = ceil(nt * n_sel / 64) + nt * R; ValueError unless nt >= 1 and nt * n_sel < 2^31."""
    nt = int(nt)
    if nt < 1:
        raise ValueError('regions: nt must be at least 1, got %d' % nt)
    if nt * plan.n_sel >= 2 ** 31:
        raise ValueError('regions: %d time nodes x %d selected points is 2^31 or more; split the request' % (nt, plan.n_sel))
    return -(-nt * plan.n_sel // GROUP) + nt * plan.n_regions


def _weights(weights, shape, lat_deg, what):
    """The weight of every candidate as a float32 array of `shape` ((ny, nx) or (N,)); ValueError where one is negative or not finite."""
    if weights is None:
        return np.ones(shape, dtype=np.float32)
    if isinstance(weights, str):
        if weights != 'area':
            raise ValueError("%s: weights = %r; None, 'area' or an array" % (what, weights))
        if lat_deg is None:
            raise ValueError("%s: weights = 'area' needs lat_deg, the latitude of every row (station)" % what)
        lat = np.asarray(lat_deg, dtype=np.float64).reshape(-1)
        if lat.size != shape[0] or not np.all(np.isfinite(lat)):
            raise ValueError('%s: lat_deg must be %d finite latitudes, got %s' % (what, shape[0], lat.shape))
        if np.any(np.abs(lat) > 90.0):
            raise ValueError('%s: a latitude outside +-90 degrees' % what)
        w = area_weights(lat)                                  # (cos of fp64 +-90 degrees is 6e-17: never negative)
        return np.ascontiguousarray(np.broadcast_to(w[:, None], shape)) if len(shape) == 2 else w
    w = np.asarray(weights)
    if w.shape != tuple(shape) or w.dtype.kind not in 'fiu':
        raise ValueError('%s: weights must be a real array of shape %s, got %s %s' % (what, tuple(shape), w.dtype, w.shape))
    with np.errstate(over='ignore'):
        w32 = w.astype(np.float32)
    if not np.all(np.isfinite(w32)) or np.any(w32 < 0):
        raise ValueError('%s: a weight is negative or not finite (in float32)' % what)
    return np.ascontiguousarray(w32)


def region_plan(regions=None, weights=None, lat_deg=None, groups=None, n_regions=None):
    """The plan of a region set.  Exactly one of
      regions: an int label plane [ny, nx] (-1: in no region; ids 0..R - 1) or a sequence of R boolean masks [ny, nx] (they may overlap);
      groups:  [N] int, the group of every station (-1: in none).
    weights: None (ones), 'area' (float32(cos(lat_deg)); lat_deg [ny] the rows' latitudes -- row_latitudes -- or [N] the stations') or a non-negative
    finite plane [ny, nx] (array [N]).  n_regions: R where the labels do not reach it (trailing empty regions); default max label + 1.  ValueError: a
    label below -1, a label >= n_regions, labels that are not integers, masks of different shapes or not boolean, no region at all, no point in any
    region, a bad weight."""
    if (regions is None) == (groups is None):
        raise ValueError('region_plan: give a label plane or a list of masks (regions), or station groups (groups), not both')
    what = 'region_plan'
    lab = masks = shape = None
    if groups is not None:
        lab = _host(groups)
        if lab.ndim != 1 or lab.size == 0:
            raise ValueError('%s: groups must be a non-empty 1-d array, got shape %s' % (what, lab.shape))
    elif isinstance(regions, (list, tuple)) and (len(regions) == 0 or np.ndim(_host(regions[0])) == 2):
        masks = [_host(m) for m in regions]                    # a sequence of planes
    else:
        arr = _host(regions)
        if arr.dtype == np.bool_ and arr.ndim in (2, 3):       # one mask, or the masks stacked
            masks = list(arr.reshape((-1,) + arr.shape[-2:]))
        elif arr.ndim == 2:
            lab, shape = arr, arr.shape
        else:
            raise ValueError('%s: a label plane is [ny, nx], got shape %s' % (what, arr.shape))
    if masks is not None:
        if not masks:
            raise ValueError('%s: no region (an empty list of masks)' % what)
        shape = masks[0].shape
        for m in masks:
            if m.dtype != np.bool_ or m.ndim != 2 or m.shape != shape:
                raise ValueError('%s: the masks must be boolean planes of one shape, got %s %s against %s' % (what, m.dtype, m.shape, shape))
    if lab is not None:
        if lab.dtype.kind not in 'iu':
            raise ValueError('%s: labels must be integers, got %s' % (what, lab.dtype))
        if lab.size == 0:
            raise ValueError('%s: an empty label plane' % what)
        lab = lab.astype(np.int64)
        if lab.min() < -1:
            raise ValueError('%s: a label below -1 (-1 means "in no region")' % what)
        R = int(lab.max()) + 1 if n_regions is None else int(n_regions)
        if lab.max() >= R:
            raise ValueError('%s: label %d with n_regions = %d' % (what, lab.max(), R))
    else:
        R = len(masks)
        if n_regions is not None and int(n_regions) != R:
            raise ValueError('%s: %d masks with n_regions = %d' % (what, R, n_regions))
    if R < 1:
        raise ValueError('%s: no region (every label is -1)' % what)
    cand_shape = tuple(shape) if shape is not None else (lab.size,)
    if min(cand_shape) < 1:
        raise ValueError('%s: an empty plane' % what)
    w = _weights(weights, cand_shape, lat_deg, what).reshape(-1)
    if lab is not None:
        flat = lab.reshape(-1)
        order = np.argsort(flat, kind='stable')                # grouped by region, ascending inside a region
        order = order[flat[order] >= 0]
        seg = flat[order]
    else:
        parts = [np.flatnonzero(m.reshape(-1)) for m in masks]
        order = np.concatenate(parts)
        seg = np.concatenate([np.full(p.size, r, dtype=np.int64) for r, p in enumerate(parts)])
    if order.size == 0:
        raise ValueError('%s: no point in any region' % what)
    if order.size >= 2 ** 31:
        raise ValueError('%s: 2^31 or more selected points' % what)
    offs = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg, minlength=R), out=offs[1:])
    return RegionPlan(order.astype(np.int64), seg.astype(np.int32), np.ascontiguousarray(w[order]), offs.astype(np.int32), R,
                      None if shape is None else (int(shape[0]), int(shape[1])), int(np.prod(cand_shape)))


def regions_reference(values, plan, nt, thr_col=(), thr_val=()):
    """dpn_region_accumulate over values [nt * n_sel, P] (float32: the products of the flat point list, time-major), then dpn_region_finish.  Returns
    a dict: 'partials' = dict(w, wx [P, S] fp64, count [P, S] int32, vmin, vmax [P, S] float32, imin, imax [P, S] int32, wexc [E, S] fp64) as the
    device state holds them after the last chunk (started from zeros), and mean, total, weight, min, max [nt, R, P] float32, where_min, where_max,
    count [nt, R, P] int32, frac [nt, R, E] float32.
    Per point i = it * n_sel + j in increasing order, slot s = i // 64 + it * R + seg[j], per column with x the value and wt = wgt[j]: skipped if x is
    not finite or wt == 0; otherwise the slot's first point sets vmin = vmax = x, imin = imax = j, a later one replaces them where x < vmin (x > vmax),
    strictly; count += 1; w = w + wt; wx = wx + wt * x (fp64, the product exact); wexc[e] = wexc[e] + wt where thr_col[e] is the column and
    x > thr_val[e] (strict, in float32).  Finish, per cell and column over the cell's slots in increasing order, slots with count == 0 skipped: count,
    w, wx, wexc added one after the other, min / max merged strictly (the earlier slot stays); mean = float32(wx / w), total = float32(wx), weight =
    float32(w), frac[e] = float32(wexc[e] / w); a cell without a counted point: count = 0, weight = 0, where = -1, the rest NaN."""
    v = np.asarray(values, dtype=np.float32)
    nt, n_sel, R = int(nt), plan.n_sel, plan.n_regions
    S = n_slots(plan, nt)
    if v.ndim != 2 or v.shape[0] != nt * n_sel or not 1 <= v.shape[1] <= MAX_COLUMNS:
        raise ValueError('values must be [nt * n_sel = %d, P <= %d], got %s' % (nt * n_sel, MAX_COLUMNS, v.shape))
    P = v.shape[1]
    thr_col = np.asarray([int(c) for c in thr_col], dtype=np.int64)
    thr_val = np.asarray(thr_val, dtype=np.float32).reshape(-1)
    E = thr_col.size
    if E != thr_val.size or E > MAX_THRESHOLDS or (E and (thr_col.min() < 0 or thr_col.max() >= P)):
        raise ValueError('thresholds: %d columns, %d values (at most %d), columns in 0..%d' % (E, thr_val.size, MAX_THRESHOLDS, P - 1))
    st = {name: np.zeros((P, S), dtype=dt) for name, dt in PARTIALS}
    st['wexc'] = np.zeros((E, S), dtype=np.float64)
    finite = np.isfinite(v)
    for i in range(nt * n_sel):                                # one point after the other: the kernel's order inside a slot
        it, j = divmod(i, n_sel)
        s = i // GROUP + it * R + int(plan.seg[j])
        wt = plan.wgt[j]
        if wt == 0:
            continue
        x, ok = v[i], finite[i]
        first = ok & (st['count'][:, s] == 0)
        with np.errstate(invalid='ignore'):
            lo = first | (ok & (x < st['vmin'][:, s]))
            hi = first | (ok & (x > st['vmax'][:, s]))
            above = ok[thr_col] & (x[thr_col] > thr_val)
        st['vmin'][lo, s], st['imin'][lo, s] = x[lo], j
        st['vmax'][hi, s], st['imax'][hi, s] = x[hi], j
        st['count'][ok, s] += 1
        st['w'][ok, s] = st['w'][ok, s] + np.float64(wt)
        st['wx'][ok, s] = st['wx'][ok, s] + np.float64(wt) * x[ok].astype(np.float64)
        st['wexc'][above, s] = st['wexc'][above, s] + np.float64(wt)
    nan = np.float32(np.nan)
    out = {k: np.full((nt, R, P), nan, dtype=np.float32) for k in FLOAT_OUTPUTS}
    out.update({k: np.full((nt, R, P), -1, dtype=np.int32) for k in INT_OUTPUTS})
    out['frac'] = np.full((nt, R, E), nan, dtype=np.float32)
    for it in range(nt):
        for r in range(R):
            c = it * R + r
            o0, o1 = int(plan.offs[r]), int(plan.offs[r + 1])
            slots = range((it * n_sel + o0) // GROUP + c, (it * n_sel + o1 - 1) // GROUP + c + 1) if o1 > o0 else ()
            count = np.zeros(P, dtype=np.int32)
            w, wx, wexc = np.zeros(P), np.zeros(P), np.zeros(E)
            vmin, vmax = np.zeros(P, dtype=np.float32), np.zeros(P, dtype=np.float32)
            imin, imax = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
            for s in slots:
                ok = st['count'][:, s] != 0
                first = ok & (count == 0)
                lo = first | (ok & (st['vmin'][:, s] < vmin))
                hi = first | (ok & (st['vmax'][:, s] > vmax))
                vmin[lo], imin[lo] = st['vmin'][lo, s], st['imin'][lo, s]
                vmax[hi], imax[hi] = st['vmax'][hi, s], st['imax'][hi, s]
                count[ok] += st['count'][ok, s]
                w[ok] = w[ok] + st['w'][ok, s]
                wx[ok] = wx[ok] + st['wx'][ok, s]
                oke = ok[thr_col]
                wexc[oke] = wexc[oke] + st['wexc'][oke, s]
            some = count > 0
            out['count'][it, r] = count
            out['weight'][it, r] = w.astype(np.float32)
            with np.errstate(invalid='ignore', divide='ignore'):
                out['mean'][it, r] = np.where(some, (wx / w).astype(np.float32), nan)
                out['frac'][it, r] = np.where(some[thr_col], (wexc / w[thr_col]).astype(np.float32), nan)
            out['total'][it, r] = np.where(some, wx.astype(np.float32), nan)
            out['min'][it, r], out['max'][it, r] = np.where(some, vmin, nan), np.where(some, vmax, nan)
            out['where_min'][it, r], out['where_max'][it, r] = imin, imax
    out['partials'] = st
    return out
