"""Shared by tests/test_prob_verify_cpu.py and tests/test_gpu_prob_verify.py: hand-written tables of the probabilistic verification of ensembles,
their expected scores computed exactly from the float32 inputs with fractions.Fraction (an independent reference, not the code under test: the
Brier score from the pairs themselves, the ROC area as the Mann-Whitney count), a plain scalar loop restatement with seeded mistakes, and the bound
of the comparison.

A table is a dict: x, b [C, M, n, P] float32 (forecast and baseline members; C cases of M members at n points), o [C, n, P] float32 (the reports),
thr = (thr_col, thr_val, thr_side), groups [n] (the pooling that is checked; a group id that no point has is an empty group).

The bound.  The scores leave as float32 casts of fp64 results, so even a perfect fp64 computation deviates from the exact value by up to half a
float32 step, 2^-24 = 5.96e-08 relative -- and by twice that where the comparison squares a score that ends in a square root (rmse, spread,
spread_skill: the exact value of the square is a rational, the root is not).  MEASURED is the worst relative deviation of the restatement from the
exact value over every table below (points and pooled groups, all scores), measured on the CPU by
test_prob_verify_cpu.test_restatement_meets_the_exact_tables, which prints it; BOUND = 8 x MEASURED, as tests/verify_cases.py has it."""
from fractions import Fraction

import numpy as np

NAN = float('nan')
INF = float('inf')
MEASURED = 1.02e-07                      # one, two 9.971e-08 (points); three 9.351e-08; eight 9.062e-08 (pooled); layout 1.018e-07 (points)
BOUND = 8 * MEASURED                     # 8.16e-07
ABOVE, BELOW = 0, 1

SIDE_SCORES = ('crps', 'fair_crps', 'bias', 'rmse', 'spread', 'spread_skill')
SCORES = SIDE_SCORES + tuple('base_' + k for k in SIDE_SCORES) + ('crpss', 'fair_crpss')
SIDE_THRESHOLD_SCORES = ('brier', 'reliability', 'resolution', 'bss', 'roc_area')
THRESHOLD_SCORES = SIDE_THRESHOLD_SCORES + tuple('base_' + k for k in SIDE_THRESHOLD_SCORES) + ('uncertainty',)
INT_KEYS = ('count', 'rank_hist', 'base_rank_hist', 'rel_n', 'rel_o', 'base_rel_n', 'base_rel_o')
SQUARED = ('rmse', 'spread', 'spread_skill', 'base_rmse', 'base_spread', 'base_spread_skill')       # compared as squares

T0 = float(np.float32(273.15))           # the float32 nearest the freezing point: a member and a report that hit the threshold exactly


def _table(points, thr, groups):
    """points: per point a list of P columns, each a list of C cases (x members, b members, o) -> the table's dict."""
    n, P, C = len(points), len(points[0]), len(points[0][0])
    M = len(points[0][0][0][0])
    x, b = (np.zeros((C, M, n, P), dtype=np.float32) for _ in range(2))
    o = np.zeros((C, n, P), dtype=np.float32)
    for i, cols in enumerate(points):
        for j, cases in enumerate(cols):
            for c, (xm, bm, ov) in enumerate(cases):
                x[c, :, i, j], b[c, :, i, j], o[c, i, j] = xm, bm, ov
    return dict(x=x, b=b, o=o, thr=thr, groups=np.asarray(groups, dtype=np.int64))


def one_member():
    """M = 1 (the CRPS is the absolute error, the fair CRPS too, no spread): three points, two cases, one column with `above 300`."""
    pts = [[[((301.5,), (299.0,), 300.25), ((298.0,), (299.5,), 299.0)]],
           [[((300.0,), (300.5,), 300.0), ((302.0,), (301.0,), 303.5)]],                          # a member that is the threshold and the report
           [[((NAN,), (299.0,), 300.0), ((297.0,), (296.0,), NAN)]]]                              # never a pair
    return _table(pts, ([0], [300.0], [ABOVE]), [0, 0, 1])


def two_members():
    """M = 2: four points, two cases; the events `above 1000` (never) and `above 0` (always) have no uncertainty; group 1 is empty."""
    pts = [[[((299.0, 301.0), (298.0, 300.0), 300.5), ((300.0, 300.0), (301.0, 299.0), 300.0)]],     # inside; all members equal the report
           [[((302.0, 303.5), (301.0, 304.0), 300.0), ((296.0, 297.25), (295.0, 299.0), 299.0)]],    # below; above (inside the baseline's)
           [[((300.0, 299.0), (300.0, 300.0), 300.0), ((301.0, 301.0), (301.0, 302.0), 298.0)]],     # equal to one member; equal members
           [[((299.0, 298.0), (NAN, 300.0), 299.5), ((299.0, 298.0), (299.5, 300.0), INF)]]]         # a NaN baseline member; an infinite report
    return _table(pts, ([0, 0, 0], [300.0, 1000.0, 0.0], [ABOVE, ABOVE, ABOVE]), [0, 2, 2, 0])


def three_members():
    """M = 3, two columns (a temperature with `above 300` and `below 273.15f`, a wind with `above 10`), three cases, eight points."""
    wind = [((8.0, 9.5, 11.0), (9.0, 9.0, 12.0), 10.25), ((12.0, 10.0, 14.5), (9.5, 10.5, 10.0), 10.0), ((3.0, 2.0, 2.5), (2.0, 4.0, 3.0), 2.5)]
    pts = [
        # 0: the report below the ensemble, inside it, above it
        [[((301.0, 302.5, 300.5), (300.0, 301.0, 303.0), 299.5), ((299.0, 301.0, 300.25), (298.0, 299.5, 302.0), 300.5),
          ((297.0, 298.5, 296.0), (299.0, 297.5, 298.0), 300.125)], wind],
        # 1: the report equal to one member, to all three, to two of three
        [[((300.0, 301.0, 299.0), (300.0, 300.0, 302.0), 300.0), ((T0, T0, T0), (272.0, T0, 274.0), T0),
          ((275.0, 274.0, 275.0), (276.0, 275.0, 275.0), 275.0)], wind],
        # 2: around freezing: members below, at and above 273.15f
        [[((272.0, T0, 274.5), (271.0, 272.5, 273.0), 272.75), ((270.0, 271.5, 272.0), (T0, 274.0, 275.0), 273.5),
          ((274.0, 275.5, 273.5), (272.0, 273.0, 274.0), T0)], wind],
        # 3: a NaN member in the first case, pairs in the other two
        [[((300.0, NAN, 301.0), (300.0, 301.0, 302.0), 300.5), ((300.5, 301.5, 299.0), (299.0, 300.0, 301.0), 301.0),
          ((302.0, 300.0, 301.0), (301.0, 301.0, 301.0), 300.75)], wind],
        # 4: a NaN baseline member in the second case: the pair is dropped on both sides
        [[((298.0, 299.0, 300.5), (297.0, 300.0, 301.0), 299.25), ((300.5, 301.5, 299.0), (299.0, NAN, 301.0), 301.0),
          ((303.0, 301.0, 302.0), (300.0, 302.0, 304.0), 302.5)], wind],
        # 5: a NaN report, an infinite report, one pair
        [[((298.0, 299.0, 300.5), (297.0, 300.0, 301.0), NAN), ((300.5, 301.5, 299.0), (299.0, 300.5, 301.0), INF),
          ((300.125, 302.75, 297.5), (298.5, 301.0, 299.25), 299.75)], wind],
        # 6: never a pair
        [[((298.0, 299.0, 300.5), (297.0, 300.0, 301.0), NAN)] * 3, [((5.0, 6.0, 7.0), (5.0, 6.0, 7.0), NAN)] * 3],
        # 7: the forecast ensemble is the report: crps 0, rmse 0, no spread / skill
        [[((300.0, 300.0, 300.0), (299.0, 300.0, 301.0), 300.0), ((301.5, 301.5, 301.5), (300.0, 301.0, 303.5), 301.5),
          ((T0, T0, T0), (T0, 272.0, 274.0), T0)], wind],
    ]
    return _table(pts, ([0, 0, 1], [300.0, T0, 10.0], [ABOVE, BELOW, ABOVE]), [0, 0, 1, 1, 1, 3, 3, 0])


def eight_members():
    """M = 8: two points, two cases; a report equal to three members (the tie bin), a report outside the ensemble."""
    pts = [[[((299.0, 300.0, 300.0, 300.0, 301.0, 302.5, 298.0, 303.0), (297.0, 298.0, 299.0, 300.0, 301.0, 302.0, 303.0, 304.0), 300.0),
             ((305.0, 304.0, 306.5, 303.0, 304.5, 305.5, 307.0, 303.5), (300.0, 301.0, 302.0, 303.0, 304.0, 305.0, 306.0, 307.0), 302.0)]],
           [[((290.0, 291.5, 292.0, 289.0, 290.5, 293.0, 291.0, 292.5), (291.0, 291.0, 291.0, 291.0, 292.0, 292.0, 292.0, 292.0), 291.75),
             ((300.5, 299.5, 301.0, 298.0, 302.0, 300.0, 299.0, 301.5), (298.0, 299.0, 300.0, 301.0, 302.0, 303.0, 304.0, 305.0), 300.0)]]]
    return _table(pts, ([0, 0], [300.0, 292.0], [ABOVE, BELOW]), [0, 0])


SEGMENTS = (65, 0, 1, 64)                                       # the points of groups 0..3 of the layout table


def layout():
    """130 points in groups of 65, 0, 1 and 64 dealt out in turn, M = 2, two cases, by formula: more than one lane round of the pooling."""
    left, groups = list(SEGMENTS), []
    while any(left):
        for g, k in enumerate(left):
            if k:
                groups.append(g)
                left[g] -= 1
    n = len(groups)
    i = np.arange(n, dtype=np.int64)
    x, b = (np.zeros((2, 2, n, 1), dtype=np.float32) for _ in range(2))
    o = np.zeros((2, n, 1), dtype=np.float32)
    for c in range(2):
        o[c, :, 0] = 300.0 + ((i * 37 + c * 11) % 41 - 20) * 0.125
        for m in range(2):
            x[c, m, :, 0] = o[c, :, 0] + ((i * 13 + c * 5 + m * 7) % 9 - 4) * 0.25
            b[c, m, :, 0] = o[c, :, 0] + ((i * 7 + c * 3 + m * 5) % 15 - 7) * 0.375
    o[0, ::17, 0] = np.nan
    x[1, 1, 5::23, 0] = np.nan
    return dict(x=x, b=b, o=o, thr=([0, 0], [300.0, 299.0], [ABOVE, BELOW]), groups=np.asarray(groups, dtype=np.int64))


_cache = {}


def tables():
    if 'tables' not in _cache:
        _cache['tables'] = {'one': one_member(), 'two': two_members(), 'three': three_members(), 'eight': eight_members(), 'layout': layout()}
    return _cache['tables']


def n_groups(case):
    return int(case['groups'].max()) + 1


def exact_of(name, pooled):
    """exact_scores of tables()[name], per point or per group of its `groups`, computed once."""
    if (name, pooled) not in _cache:
        case = tables()[name]
        _cache[name, pooled] = exact_scores(case, case['groups'] if pooled else None)
    return _cache[name, pooled]


# ------------------------------------------------------------------------------------------------ the exact reference
def _event(z, thr, side):
    return bool(z > np.float32(thr)) if side == ABOVE else bool(z < np.float32(thr))


def _frac(v):
    return Fraction(float(v))


def exact_scores(case, groups=None):
    """The scores of `case` per point (groups None) or per group (the pairs of the group's points pooled), exactly: the integer outputs as int
    arrays, every float score an object array of Fractions (None where the score is not defined), the scores of SQUARED as their squares."""
    x, b, o = case['x'], case['b'], case['o']
    thr_col, thr_val, thr_side = case['thr']
    C, M, n, P = x.shape
    groups = np.arange(n) if groups is None else np.asarray(groups)
    G, E = int(groups.max()) + 1, len(thr_col)
    out = {k: np.full((G, P), None, dtype=object) for k in SCORES}
    out.update({k: np.full((G, E), None, dtype=object) for k in THRESHOLD_SCORES})
    out['count'] = np.zeros((G, P), dtype=np.int32)
    out.update({k: np.zeros((G, P, M + 1), dtype=np.int32) for k in ('rank_hist', 'base_rank_hist')})
    out.update({k: np.zeros((G, E, M + 1), dtype=np.int32) for k in ('rel_n', 'rel_o', 'base_rel_n', 'base_rel_o')})
    for g in range(G):
        pts = np.nonzero(groups == g)[0]
        for j in range(P):
            pairs = [(x[c, :, i, j], b[c, :, i, j], o[c, i, j]) for i in pts for c in range(C)]
            pairs = [p for p in pairs if np.isfinite(p[0]).all() and np.isfinite(p[1]).all() and np.isfinite(p[2])]
            N = len(pairs)
            out['count'][g, j] = N
            sums = {}
            for side, pre in enumerate(('', 'base_')):
                s_crps = s_fair = s_d = s_d2 = s_var = Fraction(0)
                for p in pairs:
                    X, O = [_frac(v) for v in p[side]], _frac(p[2])
                    a = sum(abs(v - O) for v in X)
                    gg = sum(abs(X[i] - X[k]) for i in range(M) for k in range(i + 1, M))
                    mean = sum(X) / M
                    s_crps += a / M - gg / (M * M)
                    s_fair += a / M - gg / (M * (M - 1)) if M > 1 else a
                    s_d += mean - O
                    s_d2 += (mean - O) ** 2
                    s_var += sum((v - mean) ** 2 for v in X) / (M - 1) if M > 1 else 0
                    lt, eq = sum(bool(v < p[2]) for v in p[side]), sum(bool(v == p[2]) for v in p[side])
                    out[pre + 'rank_hist'][g, j, lt + eq // 2] += 1
                sums[side] = (s_crps, s_fair)
                if N:
                    out[pre + 'crps'][g, j], out[pre + 'fair_crps'][g, j], out[pre + 'bias'][g, j] = s_crps / N, s_fair / N, s_d / N
                    out[pre + 'rmse'][g, j], out[pre + 'spread'][g, j] = s_d2 / N, s_var / N
                    if M > 1 and s_d2 != 0:
                        out[pre + 'spread_skill'][g, j] = Fraction(M + 1, M) * s_var / s_d2
            if N:
                for k, key in enumerate(('crpss', 'fair_crpss')):
                    if sums[1][k] != 0:
                        out[key][g, j] = 1 - sums[0][k] / sums[1][k]
            for e in range(E):
                if thr_col[e] != j:
                    continue
                ev = lambda z: _event(z, thr_val[e], thr_side[e])
                for side, pre in enumerate(('', 'base_')):
                    ks = [(sum(ev(v) for v in p[side]), ev(p[2])) for p in pairs]
                    for k, eo in ks:
                        out[pre + 'rel_n'][g, e, k] += 1
                        out[pre + 'rel_o'][g, e, k] += eo
                    if not N:
                        continue
                    brier = sum((Fraction(k, M) - int(eo)) ** 2 for k, eo in ks) / N
                    obar = Fraction(sum(eo for _, eo in ks), N)
                    rel = res = Fraction(0)
                    for k in range(M + 1):
                        nk, ok = int(out[pre + 'rel_n'][g, e, k]), int(out[pre + 'rel_o'][g, e, k])
                        if nk:
                            rel += nk * (Fraction(k, M) - Fraction(ok, nk)) ** 2
                            res += nk * (Fraction(ok, nk) - obar) ** 2
                    unc = obar * (1 - obar)
                    out[pre + 'brier'][g, e], out[pre + 'reliability'][g, e], out[pre + 'resolution'][g, e] = brier, rel / N, res / N
                    out['uncertainty'][g, e] = unc
                    if unc != 0:
                        out[pre + 'bss'][g, e] = 1 - brier / unc
                    yes, no = [k for k, eo in ks if eo], [k for k, eo in ks if not eo]
                    if yes and no:                              # Mann-Whitney: an event case ranked above a non-event case, ties a half
                        wins = sum(Fraction(1) if a > c else Fraction(1, 2) if a == c else Fraction(0) for a in yes for c in no)
                        out[pre + 'roc_area'][g, e] = wins / (len(yes) * len(no))
    return out


def deviation(got, want):
    """The worst relative deviation of the float scores of `got` (float32 arrays) from the exact `want` over all its keys, a score of SQUARED squared
    first; inf where an integer output differs, a NaN stands on one side only, or a score whose exact value is 0 is not 0."""
    worst = 0.0
    for key, w in want.items():
        g = np.asarray(got[key])
        if g.shape != w.shape:
            return INF
        if key in INT_KEYS:
            if not np.array_equal(g, w):
                return INF
            continue
        for idx in np.ndindex(w.shape):
            e, v = w[idx], float(g[idx])
            if e is None or v != v:
                if (e is None) != (v != v):
                    return INF
                continue
            if not np.isfinite(v):
                return INF
            q = Fraction(v) ** 2 if key in SQUARED else Fraction(v)
            if e == 0:
                if q != 0:
                    return INF
                continue
            worst = max(worst, float(abs(q - e) / abs(e)))
    return worst


# ------------------------------------------------------------------------------------------------ a plain loop, with mistakes on request
MISTAKES = ('fair and plain divisor swapped', 'ordered pairs not halved', '<= in the rank', 'tie range not halved', 'variance divided by M',
            'non-strict event', 'roc end point missing', 'pair counted with a NaN member')
_SUMS = ('sum_crps', 'sum_fair', 'sum_d', 'sum_d2', 'sum_var')


def _cell(M, E):
    return {'n': 0, 'sums': [[0.0] * 5, [0.0] * 5], 'rank': [[0] * (M + 1), [0] * (M + 1)], 'rel': [[[[0] * (M + 1), [0] * (M + 1)] for _ in range(2)] for _ in range(E)]}


def loop_scores(case, groups=None, mistake=None):
    """dpn_pverify_stage, dpn_pverify_case, dpn_pverify_pool (groups given) and dpn_pverify_finish as a plain loop over Python floats -- IEEE
    doubles, one rounding per operation, the header's order --, with one of MISTAKES seeded on request.  Returns the outputs as
    prob_verification.pverify_finish_reference does."""
    x, b, o = case['x'], case['b'], case['o']
    thr_col, thr_val, thr_side = case['thr']
    C, M, n, P = x.shape
    E, M1, Md = len(thr_col), M + 1, float(M)
    strict = mistake != 'non-strict event'

    def event(z, thr, side):
        thr = np.float32(thr)
        if side == ABOVE:
            return bool(z > thr) if strict else bool(z >= thr)
        return bool(z < thr) if strict else bool(z <= thr)

    cells = [[_cell(M, E) for _ in range(P)] for _ in range(n)]
    for c in range(C):
        for i in range(n):
            for j in range(P):
                ov = o[c, i, j]
                members = (x[c, :, i, j], b[c, :, i, j])
                fine = np.isfinite(ov) and all(np.isfinite(v) for v in members[1])
                if mistake != 'pair counted with a NaN member':
                    fine = fine and all(np.isfinite(v) for v in members[0])
                if not fine:
                    continue
                s = cells[i][j]
                s['n'] += 1
                O = float(ov)
                for side in range(2):
                    xs = members[side]
                    X = [float(v) for v in xs]
                    a = t = 0.0
                    lt = eq = 0
                    for m in range(M):
                        a = a + abs(X[m] - O)
                        t = t + X[m]
                        lt += bool(xs[m] <= ov) if mistake == '<= in the rank' else bool(xs[m] < ov)
                        eq += bool(xs[m] == ov)
                    g = 0.0
                    for i1 in range(M):
                        for k in range(M) if mistake == 'ordered pairs not halved' else range(i1 + 1, M):
                            g = g + abs(X[i1] - X[k])
                    mean = t / Md
                    d = mean - O
                    v = 0.0
                    for m in range(M):
                        r = X[m] - mean
                        v = v + r * r
                    am = a / Md
                    plain, fair_div = Md * Md, Md * (Md - 1.0)
                    if mistake == 'fair and plain divisor swapped' and M > 1:
                        plain, fair_div = fair_div, plain
                    crps = am - g / plain
                    fair = am - g / fair_div if M > 1 else a
                    var = (v / Md if mistake == 'variance divided by M' else v / (Md - 1.0)) if M > 1 else 0.0
                    for f, inc in enumerate((crps, fair, d, d * d, var)):
                        s['sums'][side][f] = s['sums'][side][f] + inc
                    s['rank'][side][min(lt + (eq if mistake == 'tie range not halved' else eq // 2), M)] += 1
                    for e in range(E):
                        if thr_col[e] != j:
                            continue
                        k = sum(event(vv, thr_val[e], thr_side[e]) for vv in xs)
                        s['rel'][e][side][0][k] += 1
                        if event(ov, thr_val[e], thr_side[e]):
                            s['rel'][e][side][1][k] += 1
    if groups is not None:
        groups = np.asarray(groups)
        G = int(groups.max()) + 1
        order = np.argsort(groups, kind='stable')
        pooled = []
        for gi in range(G):
            seg = [int(i) for i in order[groups[order] == gi]]
            row = []
            for j in range(P):
                tot = _cell(M, E)
                for side in range(2):
                    for f in range(5):
                        lanes = []
                        for l in range(64):
                            acc = 0.0
                            for i in seg[l::64]:
                                acc = acc + cells[i][j]['sums'][side][f]
                            lanes.append(acc)
                        total = lanes[0]
                        for lane in lanes[1:]:
                            total = total + lane
                        tot['sums'][side][f] = total
                    tot['rank'][side] = [sum(cells[i][j]['rank'][side][k] for i in seg) for k in range(M1)]
                    for e in range(E):
                        for w in range(2):
                            tot['rel'][e][side][w] = [sum(cells[i][j]['rel'][e][side][w][k] for i in seg) for k in range(M1)]
                tot['n'] = sum(cells[i][j]['n'] for i in seg)
                row.append(tot)
            pooled.append(row)
        cells, n = pooled, G
    f32 = lambda: np.full((n, P), np.nan, dtype=np.float32)
    out = {'count': np.zeros((n, P), dtype=np.int32)}
    out.update({k: f32() for k in SCORES})
    out.update({k: np.zeros((n, P, M1), dtype=np.int32) for k in ('rank_hist', 'base_rank_hist')})
    out.update({k: np.full((n, E), np.nan, dtype=np.float32) for k in THRESHOLD_SCORES})
    out.update({k: np.zeros((n, E, M1), dtype=np.int32) for k in ('rel_n', 'rel_o', 'base_rel_n', 'base_rel_o')})
    for i in range(n):
        for j in range(P):
            s = cells[i][j]
            c = s['n']
            out['count'][i, j] = c
            for side, pre in enumerate(('', 'base_')):
                out[pre + 'rank_hist'][i, j] = s['rank'][side]
                if c == 0:
                    continue
                N = float(c)
                sm = s['sums'][side]
                mse, mvar = sm[3] / N, sm[4] / N
                rmse = float(np.sqrt(np.float64(mse)))
                out[pre + 'crps'][i, j], out[pre + 'fair_crps'][i, j], out[pre + 'bias'][i, j] = sm[0] / N, sm[1] / N, sm[2] / N
                out[pre + 'rmse'][i, j], out[pre + 'spread'][i, j] = rmse, np.sqrt(np.float64(mvar))
                if M > 1 and rmse != 0.0:
                    out[pre + 'spread_skill'][i, j] = float(np.sqrt(np.float64(((Md + 1.0) / Md) * mvar))) / rmse
            if c:
                for f, key in enumerate(('crpss', 'fair_crpss')):
                    if s['sums'][1][f] != 0.0:
                        out[key][i, j] = 1.0 - s['sums'][0][f] / s['sums'][1][f]
        for e in range(E):
            s = cells[i][thr_col[e]]
            c = s['n']
            N = float(c)
            for side, pre in enumerate(('', 'base_')):
                nk, ok = s['rel'][e][side]
                out[pre + 'rel_n'][i, e], out[pre + 'rel_o'][i, e] = nk, ok
                if c == 0:
                    continue
                events = sum(ok)
                bacc = 0.0
                for k in range(M1):
                    p = float(k) / Md
                    q = 1.0 - p
                    bacc = bacc + (float(ok[k]) * (q * q) + float(nk[k] - ok[k]) * (p * p))
                obar = float(events) / N
                racc = sacc = 0.0
                for k in range(M1):
                    if nk[k] <= 0:
                        continue
                    nd, p = float(nk[k]), float(k) / Md
                    f = float(ok[k]) / nd
                    u, v = p - f, f - obar
                    racc = racc + nd * (u * u)
                    sacc = sacc + nd * (v * v)
                area, above = 0.0, 0
                for k in range(M, 0 if mistake == 'roc end point missing' else -1, -1):
                    area = area + float(nk[k] - ok[k]) * (float(above) + float(above + ok[k]))
                    above += ok[k]
                brier, unc = bacc / N, obar * (1.0 - obar)
                out[pre + 'brier'][i, e], out[pre + 'reliability'][i, e], out[pre + 'resolution'][i, e] = brier, racc / N, sacc / N
                if unc != 0.0:
                    out[pre + 'bss'][i, e] = 1.0 - brier / unc
                if events > 0 and c - events > 0:
                    out[pre + 'roc_area'][i, e] = area / ((2.0 * float(events)) * float(c - events))
                if side == 0:
                    out['uncertainty'][i, e] = unc
    return out
