"""Case table, input builders, fp64 reference and bounds for the fused clip + Adam family (dpn_clip_adam, dpn_clip_adam_flat,
dpn_clip_adam_flat_dev; kernels dpn_gradnorm_kernel, dpn_gradnorm_reduce_kernel, dpn_adam_kernel).  Imports without a GPU:
tests/test_optim_cases_cpu.py runs the table through the numpy fp32 model below, tests/test_gpu_optim.py runs it through the C ABI.

The definition (fp64 throughout; the fp32 hyper-parameters of the ABI are exact numbers; t is the step counter AFTER the bump):
    S = sum over all tensors of g^2          norm = sqrt(S) gs          coef = min(max_norm / (norm + float32(1e-6)), 1) gs
    g' = wd p + g coef                       m' = b1 m + (1 - b1) g'    v' = b2 v + (1 - b2) g'^2
    dp = -(lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)      p' = p + dp       out_norm = norm      *step = t
gs = 1 for the two by-value forms, hyper[6] for the _dev form.

Bounds, from the kernel's operation count (u = 2^-24, g^ = |wd p| + |g coef|, right-hand sides from the fp64 reference), not measured:
    norm   |out_norm - norm| <= 12 u norm          per-thread fp32 fma chain of at most 8 squares, fp64 from there, one cast, one multiply
    m      |m - m'| <= 12 u (b1 |m0| + (1 - b1) g^)
    v      |v - v'| <= 24 u (b2 v0 + (1 - b2) g^^2)
    p      |p - p'| <= u |p'| + |dp| (e1 + 4u) + (lr / bc1) e_m / den + |dp| e_den / den
           e1 = (2u b1^t + u) / bc1 (the cancellation in 1 - powf, powf allowed 2 ulp), e2 the same with b2,
           e_den = (sqrt(v') / sqrt(bc2)) (e_v / (2 v') + e2 / 2 + 3u) + u eps, e_m and e_v the two moment bounds.
The constants are the ones the derivation gives; tests/test_optim_cases_cpu.py records how much of each a plain numpy fp32 evaluation uses.

Input kinds (builders below):
    'W'   workload-like: p ~ N(0, 1), |g| log-uniform over 1e-4 .. 1e2, moments from a plausible (clipped) history.
    'U'   update-resolved: |p| <= lr, so u |p'| no longer hides an error of dp.  'U0': p = 0 (run with wd = 0).
    'E'   eps regime: p = 0, zero moments, |g coef| log-uniform over 0.1 eps .. 10 eps.
    'Z'   'W' with every second tensor all zeros (g = m = v = 0, run with wd = 0): those p, m, v come back bit-identical.
    'I'   'W' with integer gradients in [-4, 4] (times `gmul`): the sum of squares is exact in any order.

Placement: every p, g, m, v is a window inside an owned arena per role, GUARD floats before and after each window -- SENTINEL (the pattern of
gemm_cases.py) where the kernel writes, NaN around the read-only g.  place = 'aligned': every window on 16 bytes; 'shifted': every window
1, 2 or 3 floats off (the scalar path of both kernels); 'mixed': per tensor one role alone is off (p, g, m, v in turn; every fifth none).
The flat forms keep the moments in two flat buffers, tensor i at chunk_start[i] * 2048, padding pre-filled with SENTINEL; there 'shifted' moves
p and g, 'mixed' moves p or g alone.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from gemm_cases import SENTINEL, SENTINEL_BITS, U

CHUNK = 2048                      # kAdamChunk: elements per block, padding unit of the flat moment buffers
PTR_TABLE, FLAT_TABLE = 72, 160   # kAdamMaxTensors, kAdamFlatMaxTensors: tensors per launch
GUARD = 8                         # floats before and after every window (a multiple of 4: aligned windows stay aligned)
MAX_CASE_ELEMENTS = 300_000
NUMEL_EDGES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6151)
STEPS = (1, 2, 3, 10, 1000, 100000)
PTR_COUNTS, FLAT_COUNTS = (1, 72, 73, 145), (1, 160, 161, 321)
FORMS = ('ptr', 'flat', 'dev')
SENTINEL64_BITS = 0xCAFEBABECAFEBABE      # a finite fp64 no partial sum can produce
F32 = np.float32


def f32(x):
    """The fp32 value the ABI receives, as an exact Python float."""
    return float(np.float32(x))


HYPER = {           # lr, b1, b2, eps, wd, max_norm
    'shipped': (1e-4, 0.9, 0.999, 1e-8, 1e-4, 2.5e7),
    'shipped_wd0': (1e-4, 0.9, 0.999, 1e-8, 0.0, 2.5e7),
    'test_inactive': (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1e9),       # test_fused_clip_adam_equals_torch's set
    'test_active': (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5),
    'test_active_wd0': (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5),
    'offdefault': (1e-2, 0.5, 0.9, 1e-3, 0.0, 1.0),
    'tiny_clip': (1e-3, 0.9, 0.999, 1e-8, 0.0, 1e-6),           # with gradients of norm ~1e-6: the 1e-6 of the clip denominator decides
}
HYPER_NAMES = ('lr', 'b1', 'b2', 'eps', 'wd', 'max_norm')
GS = (1.0, 1.0 / 8, 1.0 / 3)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    hyper: str
    t: int
    numels: tuple
    place: str = 'aligned'
    gs: float = 1.0
    gmul: int = 1             # kind 'I': the integer gradients are multiplied by this power of two
    gnorm: float = 0.0        # > 0: the gradients are rescaled to this global norm (before gs)

    @property
    def forms(self):
        """The entry points that can run the case: grad_scale exists in the _dev form only."""
        return FORMS if self.gs == 1.0 else ('dev',)


# ---------------------------------------------------------------------------------------------- tensor lists
def long_list(n, table):
    """n tensors, mostly 1 .. 7 elements, with chunk edges in the first table, on both sides of every table boundary and in the last table
    (a last table of ONE tensor gets three chunks and a tail, so its chunk offset matters)."""
    tiny = (1, 2, 3, 4, 5, 7)
    s = [tiny[i % 6] for i in range(n)]
    for i, e in zip((0, 2, 4, 6, 8), (2049, 255, 2047, 1025, 4096)):
        s[i] = e
    last0 = ((n - 1) // table) * table
    for b in range(table, n, table):          # around every table boundary
        s[b - 1] = 2048
        s[b] = 6151 if b != last0 else 4097
    if last0 and n - 1 > last0:
        s[n - 1] = 2047
    if n == table:
        s[n - 1] = 2049
    return tuple(s)


def table_starts(n, table):
    return list(range(0, n, table))


def chunks_of(numel):
    return (numel + CHUNK - 1) // CHUNK


def scratch_doubles(numels):
    """dpn_clip_adam_scratch_doubles restated: [0] the sum of squares, then one partial per 2048-element chunk."""
    return 1 + sum(chunks_of(n) for n in numels)


def flat_floats(numels):
    """dpn_clip_adam_flat_floats restated: every tensor padded to whole chunks."""
    return CHUNK * sum(chunks_of(n) for n in numels)


def flat_offsets(numels):
    off, o = [], 0
    for n in numels:
        off.append(o)
        o += chunks_of(n) * CHUNK
    return off


# ---------------------------------------------------------------------------------------------- the table
def _cases():
    c = []
    hy = ('shipped', 'test_inactive', 'test_active', 'offdefault')
    # every chunk edge alone, on both alignment paths
    for i, n in enumerate(NUMEL_EDGES):
        c.append(Case('w_single_%d_aligned' % n, 'W', hy[i % 4], STEPS[i % 6], (n,)))
        c.append(Case('w_single_%d_shifted' % n, 'W', hy[(i + 1) % 4], STEPS[(i + 2) % 6], (n,), place='shifted'))
    # every table boundary of both layouts, on every placement
    for i, (n, table) in enumerate([(72, PTR_TABLE), (73, PTR_TABLE), (145, PTR_TABLE), (160, FLAT_TABLE), (161, FLAT_TABLE), (321, FLAT_TABLE)]):
        for j, place in enumerate(('aligned', 'shifted', 'mixed')):
            c.append(Case('w_list%d_%s' % (n, place), 'W', hy[(i + j) % 4], STEPS[(i + 2 * j) % 6], long_list(n, table), place=place))
    # the clip active on lists past one table of either layout: the norm has to span the tables
    c.append(Case('w_list145_active', 'W', 'test_active', 2, long_list(145, PTR_TABLE)))
    c.append(Case('w_list321_active', 'W', 'test_active', 3, long_list(321, FLAT_TABLE)))
    # grad_scale (the _dev form)
    for i, gs in enumerate(GS[1:]):
        for j, h in enumerate(hy):
            c.append(Case('w_gs%d_%s' % (round(1 / gs), h), 'W', h, STEPS[(2 * i + j) % 6], (5, 2049, 257), gs=gs,
                          place=('aligned', 'shifted')[(i + j) % 2]))
    c.append(Case('w_list161_gs3', 'W', 'test_active', 10, long_list(161, FLAT_TABLE), gs=1.0 / 3, place='mixed'))
    # update-resolved, every step counter
    for i, t in enumerate(STEPS):
        c.append(Case('u_t%d_test' % t, 'U', 'test_inactive', t, (5, 2049, 257), place=('aligned', 'shifted', 'mixed')[i % 3]))
        c.append(Case('u_t%d_offdefault' % t, 'U', 'offdefault', t, (7, 1025, 4097), place=('shifted', 'aligned')[i % 2]))
        c.append(Case('u0_t%d_shipped' % t, 'U0', 'shipped_wd0', t, (3, 2047, 256), place=('aligned', 'shifted')[i % 2]))
    c.append(Case('u0_t2_active', 'U0', 'test_active_wd0', 2, (5, 2049, 257)))
    c.append(Case('u_t1000_gs3', 'U', 'test_active', 1000, (5, 2049, 257), gs=1.0 / 3))
    c.append(Case('u_list161_t2', 'U', 'shipped', 2, long_list(161, FLAT_TABLE)))
    c.append(Case('u_list73_t3', 'U', 'test_active', 3, long_list(73, PTR_TABLE), place='shifted'))
    # eps regime
    for h in ('shipped_wd0', 'offdefault'):
        for t in (1, 1000):
            c.append(Case('e_%s_t%d' % (h, t), 'E', h, t, (5, 2049, 257), place='aligned' if t == 1 else 'shifted'))
    c.append(Case('e_shipped_t100000_gs8', 'E', 'shipped_wd0', 100000, (4, 2048, 1023), gs=1.0 / 8))
    # zeros among nonzero tensors
    c.append(Case('z_offdefault_t1', 'Z', 'offdefault', 1, (3, 2049, 257, 5, 4096, 1)))
    c.append(Case('z_shipped_t10_shifted', 'Z', 'shipped_wd0', 10, (3, 2049, 257, 5, 4096, 1), place='shifted'))
    c.append(Case('z_list161_t2', 'Z', 'test_active_wd0', 2, long_list(161, FLAT_TABLE), place='mixed'))
    # exactness: integer gradients; the gs = 1/8 partner of a case carries the same gradients times 8
    for name, h, t, numels, place in (('i_small', 'test_active', 2, (5, 2049, 4097), 'aligned'), ('i_small_shifted', 'shipped', 10, (7, 2047, 1025), 'shifted'),
                                      ('i_list161', 'test_active', 3, long_list(161, FLAT_TABLE), 'aligned'),
                                      ('i_list145', 'test_inactive', 1, long_list(145, PTR_TABLE), 'mixed')):
        c.append(Case(name, 'I', h, t, numels, place=place))
        c.append(Case(name + '_x8_gs8', 'I', h, t, numels, place=place, gs=1.0 / 8, gmul=8))
    # a gradient norm of about 1e-6 against max_norm = 1e-6
    c.append(Case('w_norm1e-6_tiny_clip', 'W', 'tiny_clip', 2, (5, 2049, 257), gnorm=1e-6))
    c.append(Case('u_norm1e-6_tiny_clip', 'U0', 'tiny_clip', 3, (7, 1025, 2048), gnorm=1.5e-6, place='shifted'))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
I_PAIRS = [(c.name, c.name + '_x8_gs8') for c in CASES if c.kind == 'I' and c.gmul == 1]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


# ---------------------------------------------------------------------------------------------- inputs
@dataclass
class Inputs:
    """Logical fp32 values of one step: lists of 1-d arrays, the hyper-parameters as exact floats of their fp32 values."""
    numels: tuple
    p: list
    g: list
    m: list
    v: list
    hyper: dict
    gs: float
    t: int


def hyper_of(name):
    return {k: f32(x) for k, x in zip(HYPER_NAMES, HYPER[name])}


def _spread(rng, n, lo, hi):
    """Random sign, magnitude log-uniform over lo .. hi."""
    return rng.choice(np.array([-1.0, 1.0]), size=n) * 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), size=n)


def _coef64(g_list, h, gs):
    norm = math.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in g_list)) * gs
    return min(h['max_norm'] / (norm + f32(1e-6)), 1.0) * gs


def build(case, seed=0):
    seed_name = case.name[:-len('_x8_gs8')] if case.name.endswith('_x8_gs8') else case.name       # the partner of an 'I' case draws the same numbers
    rng = np.random.default_rng([seed, sum(map(ord, seed_name)), len(case.numels), case.t])
    h, gs = hyper_of(case.hyper), f32(case.gs)
    kind = case.kind
    p, g, m, v = [], [], [], []
    for n in case.numels:
        if kind == 'I':
            g.append((rng.integers(-4, 5, size=n) * case.gmul).astype(F32))
        elif kind == 'E':
            g.append((_spread(rng, n, 0.1, 10.0) * h['eps'] / gs).astype(F32))       # the clip is inactive at these magnitudes: coef = gs
        else:
            g.append(_spread(rng, n, 1e-4, 1e2).astype(F32))
        if kind == 'U':
            p.append(rng.uniform(-h['lr'], h['lr'], size=n).astype(F32))
        elif kind in ('U0', 'E'):
            p.append(np.zeros(n, F32))
        else:
            p.append(rng.standard_normal(n).astype(F32))
    if case.gnorm:
        scale = case.gnorm / math.sqrt(sum(float(np.sum(x.astype(np.float64) ** 2)) for x in g))
        g = [(x * scale).astype(F32) for x in g]
    if kind == 'Z':
        for i in range(1, len(g), 2):
            g[i] = np.zeros_like(g[i])
    coef = _coef64(g, h, gs)
    for i, n in enumerate(case.numels):
        if kind == 'E' or (kind == 'Z' and i % 2 == 1):
            m.append(np.zeros(n, F32)); v.append(np.zeros(n, F32))
        else:                                   # a history of gradients of this size, clipped like this one
            gc = g[i].astype(np.float64) * coef + h['wd'] * p[i]
            m.append((gc * rng.uniform(-1.0, 1.0, size=n)).astype(F32))
            v.append((gc * gc * rng.uniform(0.25, 1.5, size=n)).astype(F32))
    return Inputs(tuple(case.numels), p, g, m, v, h, gs, case.t)


@lru_cache(maxsize=None)
def built(name):
    """(inputs, reference) of a case, computed once and shared: nobody writes into either."""
    inp = build(case_by_name(name))
    return inp, reference(inp)


# ---------------------------------------------------------------------------------------------- fp64 reference and bounds
def reference(inp):
    """The definition in fp64.  Lists per tensor; `ghat` = |wd p| + |g coef| and `dp` for the bounds."""
    h, gs, t = inp.hyper, inp.gs, inp.t
    S = math.fsum(float(np.sum(g.astype(np.float64) ** 2)) for g in inp.g)
    norm = math.sqrt(S) * gs
    coef = min(h['max_norm'] / (norm + f32(1e-6)), 1.0) * gs
    bc1, bc2 = 1.0 - h['b1'] ** t, 1.0 - h['b2'] ** t
    out = dict(S=S, norm=norm, coef=coef, bc1=bc1, bc2=bc2, step=t, p=[], m=[], v=[], dp=[], ghat=[], den=[])
    for p, g, m, v in zip(inp.p, inp.g, inp.m, inp.v):
        p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
        gp = h['wd'] * p + g * coef
        m1 = h['b1'] * m + (1.0 - h['b1']) * gp
        v1 = h['b2'] * v + (1.0 - h['b2']) * gp * gp
        den = np.sqrt(v1) / math.sqrt(bc2) + h['eps']
        dp = -(h['lr'] / bc1) * m1 / den
        out['p'].append(p + dp); out['m'].append(m1); out['v'].append(v1); out['dp'].append(dp); out['den'].append(den)
        out['ghat'].append(np.abs(h['wd'] * p) + np.abs(g * coef))
    return out


def bounds(inp, ref, i):
    """(e_m, e_v, e_p) of tensor i, elementwise."""
    h, t = inp.hyper, inp.t
    m0, v0 = np.abs(inp.m[i].astype(np.float64)), inp.v[i].astype(np.float64)
    ghat, v1, dp, den = ref['ghat'][i], ref['v'][i], np.abs(ref['dp'][i]), ref['den'][i]
    e_m = 12 * U * (h['b1'] * m0 + (1.0 - h['b1']) * ghat)
    e_v = 24 * U * (h['b2'] * v0 + (1.0 - h['b2']) * ghat * ghat)
    e1 = (2 * U * h['b1'] ** t + U) / ref['bc1']
    e2 = (2 * U * h['b2'] ** t + U) / ref['bc2']
    with np.errstate(divide='ignore', invalid='ignore'):
        rel_v = np.where(v1 > 0, e_v / (2 * v1), 0.0)
    e_den = (np.sqrt(v1) / math.sqrt(ref['bc2'])) * (rel_v + e2 / 2 + 3 * U) + U * h['eps']
    e_p = U * np.abs(ref['p'][i]) + dp * (e1 + 4 * U) + (h['lr'] / ref['bc1']) * e_m / den + dp * e_den / den
    return e_m, e_v, e_p


def norm_bound(ref):
    return 12 * U * ref['norm']


def _ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, a positive or non-finite error over a zero bound as inf."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where((err == 0) & (bound >= 0), 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


def ratios(inp, ref, got):
    """Largest error / bound per quantity.  got: dict(p, m, v: lists of fp32 arrays, norm: float or None)."""
    out = dict(p=0.0, m=0.0, v=0.0)
    for i in range(len(inp.numels)):
        e_m, e_v, e_p = bounds(inp, ref, i)
        for k, e in (('m', e_m), ('v', e_v), ('p', e_p)):
            out[k] = max(out[k], _ratio(np.abs(np.asarray(got[k][i], np.float64) - ref[k][i]), e))
    if got.get('norm') is not None:
        out['norm'] = _ratio(abs(float(got['norm']) - ref['norm']), norm_bound(ref))
    return out


# ---------------------------------------------------------------------------------------------- fp32 model, with seeded mistakes
MISTAKES = ('bc2_dropped', 't_plus_1', 't_minus_1', 'eps_before_bc2', 'eps_inside_sqrt', 'wd_before_clip', 'clip_1e-6_dropped', 'gs_once',
            'norm_first_table', 'second_table_moments_from_zero', 'tail_chunk_skipped', 'v_not_squared')


def model_fp32(inp, mistake=None, table=FLAT_TABLE):
    """A plain numpy.float32 evaluation of the definition (squares rounded to fp32 and added in fp64, as the kernel's partials are; no fused
    multiply-add anywhere).  `mistake`: one of MISTAKES; `table`: tensors per launch, for the mistakes that depend on the tables."""
    assert mistake is None or mistake in MISTAKES
    h = {k: F32(x) for k, x in inp.hyper.items()}
    gs, one = F32(inp.gs), F32(1)
    n = len(inp.numels)
    body = [(k // CHUNK) * CHUNK if mistake == 'tail_chunk_skipped' else k for k in inp.numels]      # elements that are processed
    normed = range(min(n, table)) if mistake == 'norm_first_table' else range(n)
    S = math.fsum(float(np.sum(inp.g[i][:body[i]] * inp.g[i][:body[i]], dtype=np.float64)) for i in normed)
    total = F32(math.sqrt(S)) * gs
    coef = min(h['max_norm'] / (total + (F32(0) if mistake == 'clip_1e-6_dropped' else F32(1e-6))), one)
    if mistake != 'gs_once':
        coef = coef * gs
    st = F32(inp.t + {'t_plus_1': 1, 't_minus_1': -1}.get(mistake, 0))
    with np.errstate(all='ignore'):
        bc1 = one - np.power(h['b1'], st)
        bc2s = one if mistake == 'bc2_dropped' else np.sqrt(one - np.power(h['b2'], st))
        step_size = h['lr'] / bc1
    m0, v0 = [x.copy() for x in inp.m], [x.copy() for x in inp.v]
    mflat = vflat = None
    offs = flat_offsets(inp.numels)
    if mistake == 'second_table_moments_from_zero':       # the flat layout, every table addressing the moments from the start of the buffers
        mflat, vflat = np.full(flat_floats(inp.numels), SENTINEL, F32), np.full(flat_floats(inp.numels), SENTINEL, F32)
        for i in range(n):
            mflat[offs[i]:offs[i] + inp.numels[i]], vflat[offs[i]:offs[i] + inp.numels[i]] = m0[i], v0[i]
    P, M, V = [], [], []
    with np.errstate(all='ignore'):
        for i in range(n):
            k = body[i]
            p, g = inp.p[i][:k], inp.g[i][:k]
            if mflat is not None:
                o = offs[i] - offs[(i // table) * table]
                m, v = mflat[o:o + k].copy(), vflat[o:o + k].copy()
            else:
                m, v = m0[i][:k], v0[i][:k]
            gi = (h['wd'] * p + g) * coef if mistake == 'wd_before_clip' else h['wd'] * p + g * coef
            m1 = h['b1'] * m + (one - h['b1']) * gi
            v1 = h['b2'] * v + ((one - h['b2']) * gi if mistake == 'v_not_squared' else (one - h['b2']) * gi * gi)
            if mistake == 'eps_before_bc2':
                den = (np.sqrt(v1) + h['eps']) / bc2s
            elif mistake == 'eps_inside_sqrt':
                den = np.sqrt(v1 + h['eps']) / bc2s
            else:
                den = np.sqrt(v1) / bc2s + h['eps']
            p1 = p - step_size * m1 / den
            assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
            if mflat is not None:
                mflat[o:o + k], vflat[o:o + k] = m1, v1
            P.append(np.concatenate([p1, inp.p[i][k:]])); M.append(np.concatenate([m1, m0[i][k:]])); V.append(np.concatenate([v1, v0[i][k:]]))
    if mflat is not None:
        M = [mflat[offs[i]:offs[i] + inp.numels[i]].copy() for i in range(n)]
        V = [vflat[offs[i]:offs[i] + inp.numels[i]].copy() for i in range(n)]
    return dict(p=P, m=M, v=V, norm=float(total))


# ---------------------------------------------------------------------------------------------- placement
def shifts_of(case, form):
    """Per tensor the shift in floats of (p, g, m, v) off a 16-byte boundary.  The flat forms have no per-tensor m and v windows."""
    out = []
    for i in range(len(case.numels)):
        if case.place == 'aligned':
            s = [0, 0, 0, 0]
        elif case.place == 'shifted':
            s = [1 + i % 3, 1 + (i + 1) % 3, 1 + (i + 2) % 3, 1 + i % 3]
        elif form == 'ptr':                     # mixed: one role alone, every fifth tensor none
            s = [0, 0, 0, 0]
            if i % 5 != 4:
                s[i % 5] = 1 + i % 3
        else:                                   # mixed, flat: p alone, g alone, neither
            s = [0, 0, 0, 0]
            if i % 3 != 2:
                s[i % 3] = 1 + i % 3
        out.append(tuple(s))
    return out


def path_of(case, form):
    """Per tensor the path dpn_adam_kernel takes: 'vector' when all of p, g, m, v are on 16 bytes, else 'scalar'."""
    roles = 4 if form == 'ptr' else 2
    return ['vector' if not any(s[:roles]) else 'scalar' for s in shifts_of(case, form)]


class Arena:
    """One owned fp32 buffer holding a window per tensor: [GUARD][shift][numel values][.. up to a multiple of 4 + 4][GUARD] ..., `fill`
    everywhere outside the windows."""

    def __init__(self, values, shifts, fill):
        self.offsets, cur = [], 0
        for x, s in zip(values, shifts):
            assert 0 <= s < 4
            self.offsets.append(cur + GUARD + s)
            cur += GUARD + 4 + ((len(x) + 3) // 4) * 4
        self.numels = [len(x) for x in values]
        self.full = np.full(cur + GUARD, fill, F32)
        self.inside = np.zeros(cur + GUARD, bool)
        for o, x in zip(self.offsets, values):
            self.full[o:o + len(x)] = x
            self.inside[o:o + len(x)] = True

    def windows(self, full):
        return [full[o:o + n] for o, n in zip(self.offsets, self.numels)]

    def outside_kept(self, full_after):
        a, b = np.ascontiguousarray(full_after, F32).view(np.uint32), self.full.view(np.uint32)
        return bool((a[~self.inside] == b[~self.inside]).all())


def flat_arena(values, numels):
    """A flat moment buffer as the flat forms take it, inside guards: window i at GUARD + chunk_start[i] * 2048, SENTINEL in the padding of
    every tensor and in the guards.  The ABI's pointer is the buffer's base + GUARD floats."""
    a = Arena.__new__(Arena)
    a.offsets = [GUARD + o for o in flat_offsets(numels)]
    a.numels = list(numels)
    total = flat_floats(numels) + 2 * GUARD
    a.full = np.full(total, SENTINEL, F32)
    a.inside = np.zeros(total, bool)
    for o, x in zip(a.offsets, values):
        a.full[o:o + len(x)] = x
        a.inside[o:o + len(x)] = True
    return a


def is_sentinel(x):
    return bool((np.ascontiguousarray(x, F32).view(np.uint32) == SENTINEL_BITS).all())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
