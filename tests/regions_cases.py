"""Shared by tests/test_regions_cpu.py and tests/test_gpu_regions.py: hand-written tables for the regional statistics (deepphysinet_amd/regions.py,
csrc/dpn_region.inc), a plain scalar loop restatement with seeded mistakes, the bit-wise comparison and the bound against math.fsum."""
import math

import numpy as np

from deepphysinet_amd.regions import region_plan

F = np.float32
NAN, INF = float('nan'), float('inf')
KEYS = ('mean', 'total', 'weight', 'min', 'max', 'where_min', 'where_max', 'count', 'frac')


def same(got, want):
    """NaN in the same places, the same bits everywhere else (a -0 is not a +0), the same shape and type."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return bool(np.array_equal(got, want))
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(got.view(bits)[~nan], want.view(bits)[~nan]))


def _case(name, plan, nt, values, thr=((), ()), partial_count=None, **expected):
    v = np.asarray(values, dtype=F)
    if v.ndim == 1:
        v = v[:, None]
    want = {}
    for key, a in expected.items():
        dt = np.int32 if key in ('where_min', 'where_max', 'count') else F
        a = np.asarray(a, dtype=dt)
        want[key] = a.reshape(nt, plan.n_regions, -1)
    return dict(name=name, plan=plan, nt=nt, values=v, thr_col=list(thr[0]), thr_val=[float(t) for t in thr[1]],
                partial_count=None if partial_count is None else np.asarray(partial_count, dtype=np.int32), want=want)


def cases():
    """The hand-written tables.  Every expected number is written out, none is computed by the code under test."""
    out = []
    # 1. a constant field has an exact mean under dyadic weights.  Plane 3 x 4, region 0 = four points (weights 0.5, 0.25, 1, 2), region 1 = two
    #    (0.5, 4), the rest in no region
    lab = np.array([[0, 0, -1, 1], [-1, 0, -1, -1], [1, -1, 0, -1]])
    w = np.array([[0.5, 0.25, 9, 0.5], [9, 1, 9, 9], [4, 9, 2, 9]], dtype=F)
    plan = region_plan(lab, w)
    out.append(_case('constant field', plan, 1, [2.5] * 6, mean=[2.5, 2.5], total=[2.5 * 3.75, 2.5 * 4.5], weight=[3.75, 4.5], min=[2.5, 2.5],
                     max=[2.5, 2.5], where_min=[0, 4], where_max=[0, 4], count=[4, 2]))
    # 2. equal values under unit weights: the mean is the value (8 x float32(0.1) is exact in fp64), min = max, both sit at the first point
    out.append(_case('equal values', region_plan(groups=[0] * 8), 1, [0.1] * 8, mean=[F(0.1)], total=[F(8 * float(F(0.1)))], weight=[8], min=[F(0.1)],
                     max=[F(0.1)], where_min=[0], where_max=[0], count=[8]))
    # 3. a threshold met exactly is not counted (strict), two thresholds on one column
    out.append(_case('threshold met exactly', region_plan(groups=[0, 0, 0, 0]), 1, [1, 2, 3, 2], thr=([0, 0], [2.0, 0.5]), frac=[0.25, 1.0], mean=[2.0],
                     count=[4]))
    # 4. a tie in max (and in min) keeps the earlier point
    out.append(_case('tie keeps the earlier point', region_plan(groups=[0, 0, 0, 0, 0]), 1, [5, 1, 5, 1, 3], where_max=[0], where_min=[1], max=[5], min=[1]))
    # 5. +0 and -0 compare equal: the earlier zero stays, sign included (the sums start at +0, so the mean of zeros is +0)
    out.append(_case('zeros', region_plan(groups=[0, 0, 1, 1]), 1, [0.0, -0.0, -0.0, 0.0], min=[0.0, -0.0], max=[0.0, -0.0], where_min=[0, 2],
                     where_max=[0, 2], mean=[0.0, 0.0]))
    # 6. zero-weight, NaN and infinite points are skipped; frac is relative to the counted weight (3), not to the region's (6)
    out.append(_case('skipped points', region_plan(groups=[0] * 6, weights=np.array([1, 1, 0, 1, 1, 2], dtype=F)), 1, [10, NAN, 20, INF, -INF, 30],
                     thr=([0], [15.0]), count=[2], weight=[3], total=[70], mean=[F(70.0 / 3.0)], min=[10], max=[30], where_min=[0], where_max=[5],
                     frac=[F(2.0 / 3.0)]))
    # 7. a cell with no finite point, an empty region (id 1), and a second column that is fine
    out.append(_case('nothing counted', region_plan(groups=[0, 0, 2, 2], n_regions=3), 1, [[NAN, 1], [INF, 3], [4, 2], [6, NAN]], thr=([0, 1], [0.0, 0.0]),
                     count=[[0, 2], [0, 0], [2, 1]], weight=[[0, 2], [0, 0], [2, 1]], mean=[[NAN, 2], [NAN, NAN], [5, 2]],
                     total=[[NAN, 4], [NAN, NAN], [10, 2]], min=[[NAN, 1], [NAN, NAN], [4, 2]], max=[[NAN, 3], [NAN, NAN], [6, 2]],
                     where_min=[[-1, 0], [-1, -1], [2, 2]], where_max=[[-1, 1], [-1, -1], [3, 2]], frac=[[NAN, 1], [NAN, NAN], [1, 1]]))
    # 8. groups that straddle a time plane: 65 points, 3 time nodes, one region.  Points 0..194; groups of 64 end at 63, 127, 191; planes end at 64,
    #    129, 194: the (group, cell) pairs hold 64, 1, 63, 2, 62, 3 points, in slots 0..5; slot 6 is never used.  Time node it holds the value it + 1
    out.append(_case('straddle', region_plan(groups=[0] * 65), 3, np.repeat([1.0, 2.0, 3.0], 65), partial_count=[[64, 1, 63, 2, 62, 3, 0]],
                     count=[65, 65, 65], mean=[1, 2, 3], total=[65, 130, 195], weight=[65, 65, 65], where_min=[0, 0, 0], where_max=[0, 0, 0]))
    # 9. forty cells inside one group: forty regions of one point each; region r holds r
    out.append(_case('forty cells', region_plan(groups=list(range(40))), 1, np.arange(40.0), partial_count=[[1] * 40 + [0]], count=[1] * 40,
                     mean=np.arange(40.0), where_min=np.arange(40), where_max=np.arange(40)))
    # 10. overlapping masks: the point in both regions is listed twice; two time nodes
    a = np.array([[True, True, False]])
    b = np.array([[False, True, True]])
    out.append(_case('overlap', region_plan([a, b], np.array([[1, 2, 4]], dtype=F)), 2, [1, 2, 2, 3, 10, 20, 20, 30], mean=[[F(5.0 / 3.0)], [F(16.0 / 6.0)],
                                                                                                                          [F(50.0 / 3.0)], [F(160.0 / 6.0)]],
                     weight=[3, 6, 3, 6], total=[5, 16, 50, 160], where_max=[1, 3, 1, 3], count=[2, 2, 2, 2]))
    return out


MISTAKES = ('>= for >', 'later tie kept', 'zero weight counted', 'NaN counted', 'frac over the total weight', 'group of 32', 'slot without the cell')


def loop_regions(values, plan, nt, thr_col=(), thr_val=(), mistake=None):
    """The statistics and the partial counts by a plain scalar loop over the points, written apart from regions_reference; one of MISTAKES seeded on
    request.  -> dict of KEYS and 'partial_count' [P, S]."""
    assert mistake is None or mistake in MISTAKES
    v = np.asarray(values, dtype=F)
    n_sel, R, P, E = plan.n_sel, plan.n_regions, v.shape[1], len(thr_col)
    group = 32 if mistake == 'group of 32' else 64
    S = -(-nt * n_sel // group) + nt * R
    slot = lambda i, c: i // group + (0 if mistake == 'slot without the cell' else c)
    part = [[None] * S for _ in range(P)]                     # per column and slot: [w, wx, count, vmin, vmax, imin, imax, wexc per threshold]
    for i in range(nt * n_sel):
        it, j = divmod(i, n_sel)
        s = slot(i, it * R + int(plan.seg[j]))
        wt = plan.wgt[j]
        for col in range(P):
            x = v[i, col]
            if wt == 0 and mistake != 'zero weight counted':
                continue
            if not np.isfinite(x) and mistake != 'NaN counted':
                continue
            p = part[col][s]
            if p is None:
                p = part[col][s] = [0.0, 0.0, 0, x, x, j, j, [0.0] * E]
            else:
                if x < p[3] or (mistake == 'later tie kept' and x == p[3]):
                    p[3], p[5] = x, j
                if x > p[4] or (mistake == 'later tie kept' and x == p[4]):
                    p[4], p[6] = x, j
            p[0] += float(wt)
            p[1] += float(wt) * float(x)
            p[2] += 1
            for e in range(E):
                if thr_col[e] == col and (x >= F(thr_val[e]) if mistake == '>= for >' else x > F(thr_val[e])):
                    p[7][e] += float(wt)
    out = {k: np.full((nt, R, P), NAN, dtype=F) for k in ('mean', 'total', 'weight', 'min', 'max')}
    out.update({k: np.full((nt, R, P), -1, dtype=np.int32) for k in ('where_min', 'where_max', 'count')})
    out['frac'] = np.full((nt, R, E), NAN, dtype=F)
    for it in range(nt):
        for r in range(R):
            c = it * R + r
            o0, o1 = int(plan.offs[r]), int(plan.offs[r + 1])
            slots = range(slot(it * n_sel + o0, c), slot(it * n_sel + o1 - 1, c) + 1) if o1 > o0 else ()
            region_weight = float(np.sum(plan.wgt[o0:o1].astype(np.float64)))
            for col in range(P):
                w = wx = 0.0
                count, vmin, vmax, imin, imax, wexc = 0, None, None, -1, -1, [0.0] * E
                for s in slots:
                    p = part[col][s]
                    if p is None:
                        continue
                    if count == 0 or p[3] < vmin or (mistake == 'later tie kept' and p[3] == vmin):
                        vmin, imin = p[3], p[5]
                    if count == 0 or p[4] > vmax or (mistake == 'later tie kept' and p[4] == vmax):
                        vmax, imax = p[4], p[6]
                    w, wx, count = w + p[0], wx + p[1], count + p[2]
                    wexc = [a + b for a, b in zip(wexc, p[7])]
                out['count'][it, r, col], out['weight'][it, r, col] = count, w
                out['where_min'][it, r, col], out['where_max'][it, r, col] = imin, imax
                if count:
                    with np.errstate(invalid='ignore', divide='ignore'):
                        out['mean'][it, r, col], out['total'][it, r, col] = np.float64(wx) / np.float64(w), wx
                    out['min'][it, r, col], out['max'][it, r, col] = vmin, vmax
                    for e in range(E):
                        if thr_col[e] == col:
                            out['frac'][it, r, e] = wexc[e] / (region_weight if mistake == 'frac over the total weight' else w)
    out['partial_count'] = np.array([[0 if p is None else p[2] for p in row] for row in part], dtype=np.int32)
    return out


def mismatches(case, got):
    """The keys of a hand-written case that `got` (regions_reference's or loop_regions' dict) misses."""
    bad = [key for key, want in case['want'].items() if not same(got[key], want)]
    if case['partial_count'] is not None:
        pc = got['partials']['count'] if 'partials' in got else got['partial_count']
        if not same(pc, case['partial_count']):
            bad.append('partial_count')
    return bad


def fsum_bound(values, plan, nt, col=0):
    """Per cell the correctly rounded weighted mean by math.fsum (None without a counted point) and the bound
    2^-24 |mean| + 2 N 2^-52 sum|w x| / W on the error of the sequential fp64 sums with exact products, N the number of points of the cell."""
    v = np.asarray(values, dtype=F)
    out = []
    for it in range(nt):
        for r in range(plan.n_regions):
            js = range(int(plan.offs[r]), int(plan.offs[r + 1]))
            pts = [(float(plan.wgt[j]), float(v[it * plan.n_sel + j, col])) for j in js]
            pts = [(w, x) for w, x in pts if w != 0 and math.isfinite(x)]
            if not pts:
                out.append((None, None))
                continue
            W = math.fsum(w for w, _ in pts)
            mean = math.fsum(w * x for w, x in pts) / W       # (w * x is exact: two float32 factors)
            out.append((mean, 2.0 ** -24 * abs(mean) + 2 * len(pts) * 2.0 ** -52 * math.fsum(abs(w * x) for w, x in pts) / W))
    return out
