"""Shared by tests/test_verify_cpu.py and tests/test_gpu_verify.py: hand-written case sequences of the verification against observations, their
expected scores computed exactly from the float32 inputs with fractions.Fraction (an independent reference, not the code under test), a plain scalar
loop restatement with seeded mistakes, and the bound of the comparison.

A case is a dict: x, b, o [M, n, P] float32 (forecast, baseline, report; M forecast dates), thr = (thr_col, thr_val, thr_side), and optionally
groups [n] (the pooling that is checked), expect (hand-written numbers that must be met exactly, in the place of the exact table).

The bound.  The scores leave as float32 casts of fp64 results, so even a perfect fp64 computation deviates from the exact value by up to half a
float32 step, 2^-24 = 5.96e-08 relative.  MEASURED is the worst relative deviation of the restatement from the exact value over every table below
(points and pooled groups, all scores), measured on the CPU by test_verify_cpu.test_restatement_meets_the_exact_tables, which prints it;
BOUND = 8 x MEASURED, the margin for libm builds that round the input of a sqrt differently."""
import decimal
from fractions import Fraction

import numpy as np

NAN = float('nan')
MEASURED = 5.78e-08                      # basic 4.704e-08 (points), 4.585e-08 (pooled); layout 5.701e-08 (points), 5.774e-08 (pooled): float32's rounding
BOUND = 8 * MEASURED                     # 4.62e-07

SCORES = ('bias', 'mae', 'rmse', 'max_abs_error', 'corr', 'base_bias', 'base_mae', 'base_rmse', 'skill')
TABLE = ('pod', 'far', 'csi', 'fbias', 'ets')
ABOVE, BELOW = 0, 1


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _series(points):
    """points: per point a list of P columns, each a list of M (x, b, o) triples -> x, b, o [M, n, P] float32."""
    a = np.asarray(points, dtype=np.float64)                   # [n, P, M, 3]
    return tuple(np.ascontiguousarray(a[..., k].transpose(2, 0, 1)).astype(np.float32) for k in range(3))


T0 = float(np.float32(273.15))                                  # the float32 nearest the freezing point: a value that hits the threshold exactly


def basic_case():
    """Eight points, two columns, five dates.  Column 0 is a temperature with the thresholds `above 300` and `below 273.15f`, column 1 a wind
    with `above 10`.  Column 1 repeats a plain series at every point unless the point says otherwise."""
    wind = [(8.0, 9.0, 11.0), (12.0, 9.5, 10.0), (10.0, 10.5, 10.25), (3.0, 2.0, 2.5), (14.0, 15.0, 9.0)]         # 10.0 is not above 10
    pts = [
        # 0: never a report
        [[(290.0, 291.0, NAN)] * 5, [(5.0, 6.0, NAN)] * 5],
        # 1: one pair, in the third date
        [[(290.0, 291.0, NAN), (291.0, 292.0, NAN), (301.5, 299.0, 300.25), (290.0, 291.0, NAN), (290.0, 291.0, NAN)], wind],
        # 2: a constant report series: m2_o = 0, no correlation
        [[(299.0, 298.0, 300.0), (300.0, 301.0, 300.0), (301.0, 302.5, 300.0), (302.0, 299.0, 300.0), (300.5, 300.0, 300.0)], wind],
        # 3: the forecast equals the report: sum_d2 = 0, skill 1, correlation 1
        [[(271.0, 272.0, 271.0), (T0, 274.0, T0), (275.5, 275.0, 275.5), (300.0, 301.0, 300.0), (300.25, 299.0, 300.25)], wind],
        # 4: the baseline equals the report: sum_e2 = 0, no skill
        [[(272.0, 271.0, 271.0), (274.0, T0, T0), (275.0, 275.5, 275.5), (301.0, 300.0, 300.0), (299.0, 300.25, 300.25)], wind],
        # 5: errors of +0 and -0 only
        [[(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (-0.0, -0.0, 0.0), (0.0, 0.0, -0.0)], [(0.0, 1.0, 0.0), (-0.0, -1.0, 0.0)] * 2 + [(0.0, 0.0, 0.0)]],
        # 6: a temperature near 300 K with a spread of a few K
        [[(300.125, 298.5, 299.75), (302.75, 301.0, 303.5), (297.5, 299.25, 296.875), (301.0, 300.0, 300.0625), (299.375, 297.0, 300.5)], wind],
        # 7: a baseline that is missing once, a forecast that is missing once, an infinite report
        [[(280.0, NAN, 281.0), (NAN, 282.0, 283.0), (284.0, 283.0, 285.5), (270.0, 274.0, T0), (286.0, 285.0, float('inf'))], wind],
    ]
    x, b, o = _series(pts)
    return dict(x=x, b=b, o=o, thr=([0, 0, 1], [300.0, T0, 10.0], [ABOVE, BELOW, ABOVE]), groups=np.array([0, 0, 1, 1, 1, 2, 0, 2]))


SEGMENTS = (1, 0, 63, 64, 65, 129, 4097)                        # the points of groups 0..6


def layout_groups():
    """The group of every point of the layout case: the groups dealt out in turn (0, 2, 3, 4, 5, 6, 0?, ..), each until it is full -- an interleaved
    order, so that a stable sort has something to do."""
    left = list(SEGMENTS)
    groups = []
    while any(left):
        for g, k in enumerate(left):
            if k:
                groups.append(g)
                left[g] -= 1
    return np.asarray(groups, dtype=np.int64)


def layout_case():
    """4 419 points in groups of 1, 0, 63, 64, 65, 129 and 4 097, two columns, two dates: a temperature near 300 K and a wind, by formula."""
    g = layout_groups()
    n = g.size
    i = np.arange(n, dtype=np.int64)
    x, b, o = (np.zeros((2, n, 2), dtype=np.float32) for _ in range(3))
    for m in range(2):
        o[m, :, 0] = 300.0 + ((i * 37 + m * 11) % 41 - 20) * 0.125
        x[m, :, 0] = o[m, :, 0] + ((i * 13 + m * 5) % 9 - 4) * 0.25
        b[m, :, 0] = o[m, :, 0] + ((i * 7 + m * 3) % 15 - 7) * 0.375
        o[m, :, 1] = ((i * 29 + m * 17) % 33) * 0.5
        x[m, :, 1] = o[m, :, 1] + ((i * 5 + m) % 7 - 3) * 0.5
        b[m, :, 1] = o[m, :, 1] + ((i * 3 + m * 2) % 11 - 5) * 0.75
    o[0, ::17, 0] = np.nan                                      # reports that are missing
    o[1, 5::23, 1] = np.nan
    return dict(x=x, b=b, o=o, thr=([0, 1, 1], [300.0, 8.0, 2.0], [ABOVE, ABOVE, BELOW]), groups=g)


BIG = 2.0 ** 53


def order_cases():
    """The fold order, where it shows: errors of 2^53, 1 and -2^53, whose fp64 sum depends on the order (2^53 + 1 rounds to 2^53).  One date, one
    column, one group; the expected bias is written out by hand for the order the header prescribes."""
    def case(d):
        x = _f32(d).reshape(1, -1, 1)
        return dict(x=x, b=np.zeros_like(x), o=np.zeros_like(x), thr=([], [], []), groups=np.zeros(x.shape[1], dtype=np.int64))
    lanes = case([1.0, BIG, -BIG])                             # three lanes, one point each: (1 + 2^53) + -2^53 = 0; in reverse the sum is 1
    lanes['expect'] = dict(count=3, bias=0.0)
    d = np.zeros(65)
    d[0], d[64], d[1] = BIG, -BIG, 1.0                          # lane 0 holds places 0 and 64: (2^53 + -2^53) + 1 + 0 .. = 1; contiguous lanes lose the 1
    strided = case(d)
    strided['expect'] = dict(count=65, bias=float(np.float32(1.0 / 65.0)))
    return {'lane order': lanes, 'strided lanes': strided}


_cache = {}


def exact_cases():
    if 'cases' not in _cache:
        _cache['cases'] = {'basic': basic_case(), 'layout': layout_case()}
    return _cache['cases']


def exact_of(name, pooled):
    """exact_scores of exact_cases()[name], per point or per group of its `groups`, computed once."""
    if (name, pooled) not in _cache:
        case = exact_cases()[name]
        _cache[name, pooled] = exact_scores(case, case['groups'] if pooled else None)
    return _cache[name, pooled]


# ------------------------------------------------------------------------------------------------ the exact reference
def _sqrt(q):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float((decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt())


def _exact_table(h, f, m, n):
    nan = NAN
    out = [float(Fraction(h, h + m)) if h + m else nan, float(Fraction(f, h + f)) if h + f else nan, float(Fraction(h, h + f + m)) if h + f + m else nan,
           float(Fraction(h + f, h + m)) if h + m else nan]
    ets = nan
    if n:
        hr = Fraction((h + f) * (h + m), n)
        if h + f + m - hr != 0:
            ets = float((h - hr) / (h + f + m - hr))
    return out + [ets]


def _event(z, thr, side):
    return bool(z > np.float32(thr)) if side == ABOVE else bool(z < np.float32(thr))


def exact_scores(case, groups=None):
    """The scores of `case` per point (groups None) or per group (the pairs of the group's points pooled), exactly: dict of count [G, P] int32, the nine
    scores [G, P] float64 and the ten threshold scores [G, E] float64 (the nearest doubles of the exact rationals; a square root to 60 digits)."""
    x, b, o = case['x'], case['b'], case['o']
    thr_col, thr_val, thr_side = case['thr']
    M, n, P = x.shape
    groups = np.arange(n) if groups is None else np.asarray(groups)
    G, E = int(groups.max()) + 1, len(thr_col)
    out = {k: np.full((G, P), np.nan) for k in SCORES}
    out['count'] = np.zeros((G, P), dtype=np.int32)
    out.update({pre + k: np.full((G, E), np.nan) for pre in ('', 'base_') for k in TABLE})
    for g in range(G):
        pts = np.nonzero(groups == g)[0]
        for j in range(P):
            tr = [(x[m, i, j], b[m, i, j], o[m, i, j]) for i in pts for m in range(M)]
            tr = [t for t in tr if all(np.isfinite(v) for v in t)]
            c = len(tr)
            out['count'][g, j] = c
            for e in range(E):
                if thr_col[e] != j:
                    continue
                for pre, k in (('', 0), ('base_', 1)):
                    ev = [(_event(t[k], thr_val[e], thr_side[e]), _event(t[2], thr_val[e], thr_side[e])) for t in tr]
                    h, f, m_ = sum(a and r for a, r in ev), sum(a and not r for a, r in ev), sum(r and not a for a, r in ev)
                    for name, v in zip(TABLE, _exact_table(h, f, m_, c)):
                        out[pre + name][g, e] = v
            if c == 0:
                continue
            X, B, O = ([Fraction(float(t[k])) for t in tr] for k in range(3))
            d, e_ = [a - r for a, r in zip(X, O)], [a - r for a, r in zip(B, O)]
            sd2, se2 = sum(v * v for v in d), sum(v * v for v in e_)
            out['bias'][g, j], out['mae'][g, j], out['rmse'][g, j] = float(sum(d) / c), float(sum(abs(v) for v in d) / c), _sqrt(sd2 / c)
            out['max_abs_error'][g, j] = float(max(abs(v) for v in d))
            out['base_bias'][g, j], out['base_mae'][g, j], out['base_rmse'][g, j] = float(sum(e_) / c), float(sum(abs(v) for v in e_) / c), _sqrt(se2 / c)
            if se2 != 0:
                out['skill'][g, j] = float(1 - sd2 / se2)
            mx, mo = sum(X) / c, sum(O) / c
            vf, vo = sum((a - mx) ** 2 for a in X), sum((r - mo) ** 2 for r in O)
            if c > 1 and vf != 0 and vo != 0:
                cov = sum((a - mx) * (r - mo) for a, r in zip(X, O))
                out['corr'][g, j] = float(cov / abs(cov)) * _sqrt(cov * cov / (vf * vo)) if cov != 0 else 0.0
    return out


def deviation(got, want):
    """The worst relative deviation of the float scores of `got` from `want` over all keys of `want`; inf where a count differs, a NaN stands on one
    side only, or a score whose exact value is 0 is not 0."""
    worst = 0.0
    for key, w in want.items():
        g = np.asarray(got[key])
        if g.shape != w.shape:
            return float('inf')
        if key == 'count':
            if not np.array_equal(g, w):
                return float('inf')
            continue
        g = g.astype(np.float64)
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            return float('inf')
        ok = ~np.isnan(w)
        zero = ok & (w == 0)
        if bool(np.any(g[zero] != 0)):
            return float('inf')
        rest = ok & ~zero
        if rest.any():
            worst = max(worst, float(np.max(np.abs(g[rest] - w[rest]) / np.abs(w[rest]))))
    return worst


def meets(got, expect):
    """The hand-written numbers of an order case (group 0, column 0), exactly."""
    return all(float(np.asarray(got[k])[0, 0]) == float(v) for k, v in expect.items())


# ------------------------------------------------------------------------------------------------ a plain loop, with mistakes on request
MISTAKES = ('non-strict threshold', 'baseline and forecast swapped', 'baseline not masked', 'n - 1 in the merge', 'lanes folded in reverse',
            'contiguous lanes', 'skill sign')
_KEYS = ('n', 'mean_f', 'mean_o', 'm2_f', 'm2_o', 'c_fo', 'sum_d', 'sum_ad', 'sum_d2', 'sum_e', 'sum_ae', 'sum_e2', 'max_ad')


def _empty():
    return dict.fromkeys(_KEYS, 0.0) | {'n': 0, 'max_ad': np.float32(0)}


def _loop_merge(A, B, mistake):
    if B['n'] == 0:
        return dict(A)
    if A['n'] == 0:
        return dict(B)
    n = A['n'] + B['n']
    w = (float(A['n']) * float(B['n'])) / float(n - 1 if mistake == 'n - 1 in the merge' else n)
    r = float(B['n']) / float(n)
    gf, go = B['mean_f'] - A['mean_f'], B['mean_o'] - A['mean_o']
    out = {'n': n, 'm2_f': (A['m2_f'] + B['m2_f']) + (gf * gf) * w, 'm2_o': (A['m2_o'] + B['m2_o']) + (go * go) * w,
           'c_fo': (A['c_fo'] + B['c_fo']) + (gf * go) * w, 'mean_f': A['mean_f'] + gf * r, 'mean_o': A['mean_o'] + go * r,
           'max_ad': B['max_ad'] if B['max_ad'] > A['max_ad'] else A['max_ad']}
    for k in ('sum_d', 'sum_ad', 'sum_d2', 'sum_e', 'sum_ae', 'sum_e2'):
        out[k] = A[k] + B[k]
    return out


def _loop_table(h, f, m, n):
    h, f, m, N = float(h), float(f), float(m), float(n)
    hm, hf, hfm = h + m, h + f, (h + f) + m
    out = [h / hm if hm else NAN, f / hf if hf else NAN, h / hfm if hfm else NAN, hf / hm if hm else NAN]
    ets = NAN
    if n:
        hr = (hf * hm) / N
        if hfm - hr != 0:
            ets = (h - hr) / (hfm - hr)
    return [np.float32(v) for v in out + [ets]]


def loop_scores(case, groups=None, mistake=None):
    """dpn_verify_accumulate, dpn_verify_pool (groups given) and dpn_verify_finish as a plain loop over Python floats -- IEEE doubles, one rounding
    per operation, the header's order --, with one of MISTAKES seeded on request.  Returns the outputs as exact_scores does, float32."""
    x, b, o = case['x'], case['b'], case['o']
    if mistake == 'baseline and forecast swapped':
        x, b = b, x
    thr_col, thr_val, thr_side = case['thr']
    M, n, P = x.shape
    E = len(thr_col)
    strict = mistake != 'non-strict threshold'

    def event(z, thr, side):
        thr = np.float32(thr)
        if side == ABOVE:
            return bool(z > thr) if strict else bool(z >= thr)
        return bool(z < thr) if strict else bool(z <= thr)

    cells = [[_empty() for _ in range(P)] for _ in range(n)]
    cont = np.zeros((n, E, 6), dtype=np.int64)
    for m in range(M):
        for i in range(n):
            for j in range(P):
                xv, bv, ov = x[m, i, j], b[m, i, j], o[m, i, j]
                if not (np.isfinite(xv) and np.isfinite(ov) and (np.isfinite(bv) or mistake == 'baseline not masked')):
                    continue
                s = cells[i][j]
                X, B, O = float(xv), float(bv), float(ov)
                c = s['n'] + 1
                df = X - s['mean_f']
                s['mean_f'] = s['mean_f'] + df / float(c)
                dq = O - s['mean_o']
                s['mean_o'] = s['mean_o'] + dq / float(c)
                s['m2_f'] = s['m2_f'] + df * (X - s['mean_f'])
                s['m2_o'] = s['m2_o'] + dq * (O - s['mean_o'])
                s['c_fo'] = s['c_fo'] + df * (O - s['mean_o'])
                d = X - O
                s['sum_d'], s['sum_ad'], s['sum_d2'] = s['sum_d'] + d, s['sum_ad'] + abs(d), s['sum_d2'] + d * d
                ad = np.float32(abs(d))
                if ad > s['max_ad']:
                    s['max_ad'] = ad
                e = B - O
                s['sum_e'], s['sum_ae'], s['sum_e2'] = s['sum_e'] + e, s['sum_ae'] + abs(e), s['sum_e2'] + e * e
                s['n'] = c
                for t in range(E):
                    if thr_col[t] != j:
                        continue
                    ex, eb, eo = (event(v, thr_val[t], thr_side[t]) for v in (xv, bv, ov))
                    cont[i, t] += [ex and eo, ex and not eo, eo and not ex, eb and eo, eb and not eo, eo and not eb]
    if groups is not None:
        groups = np.asarray(groups)
        G = int(groups.max()) + 1
        order = np.argsort(groups, kind='stable')
        pooled, pooled_cont = [], np.zeros((G, E, 6), dtype=np.int64)
        for g in range(G):
            seg = [int(i) for i in order[groups[order] == g]]
            pooled_cont[g] = cont[seg].sum(axis=0) if seg else 0
            row = []
            for j in range(P):
                per = -(-len(seg) // 64)
                lanes = []
                for l in range(64):
                    mine = seg[l * per:(l + 1) * per] if mistake == 'contiguous lanes' else seg[l::64]
                    acc = _empty()
                    for i in mine:
                        acc = _loop_merge(acc, cells[i][j], mistake)
                    lanes.append(acc)
                if mistake == 'lanes folded in reverse':
                    lanes = lanes[::-1]
                total = lanes[0]
                for lane in lanes[1:]:
                    total = _loop_merge(total, lane, mistake)
                row.append(total)
            pooled.append(row)
        cells, cont, n = pooled, pooled_cont, G
    out = {k: np.full((n, P), np.nan, dtype=np.float32) for k in SCORES}
    out['count'] = np.zeros((n, P), dtype=np.int32)
    out.update({pre + k: np.full((n, E), np.nan, dtype=np.float32) for pre in ('', 'base_') for k in TABLE})
    for i in range(n):
        for j in range(P):
            s = cells[i][j]
            c = s['n']
            out['count'][i, j] = c
            if c == 0:
                continue
            N = float(c)
            with np.errstate(over='ignore', invalid='ignore'):
                out['bias'][i, j], out['mae'][i, j], out['rmse'][i, j] = s['sum_d'] / N, s['sum_ad'] / N, np.sqrt(np.float64(s['sum_d2'] / N))
                out['max_abs_error'][i, j] = s['max_ad']
                out['base_bias'][i, j], out['base_mae'][i, j] = s['sum_e'] / N, s['sum_ae'] / N
                out['base_rmse'][i, j] = np.sqrt(np.float64(s['sum_e2'] / N))
                if c > 1 and s['m2_f'] != 0 and s['m2_o'] != 0:
                    out['corr'][i, j] = s['c_fo'] / np.sqrt(np.float64(s['m2_f'] * s['m2_o']))
                if s['sum_e2'] != 0:
                    out['skill'][i, j] = (s['sum_d2'] / s['sum_e2'] - 1.0) if mistake == 'skill sign' else (1.0 - s['sum_d2'] / s['sum_e2'])
        for t in range(E):
            c = cells[i][thr_col[t]]['n']
            for pre, k in (('', 0), ('base_', 3)):
                for name, v in zip(TABLE, _loop_table(cont[i, t, k], cont[i, t, k + 1], cont[i, t, k + 2], c)):
                    out[pre + name][i, t] = v
    return out
