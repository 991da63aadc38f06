"""Case table, operand builders and fp64 reference for the exact-fp32 GEMM family (dpn_sgemm, dpn_sgemm_batch(_jobs), dpn_sgemm_ln,
dpn_sum_parts).  Imports without a GPU: tests/test_gemm_cases_cpu.py runs the table through the numpy model below, tests/test_gpu_gemm.py
runs it through the C ABI.

Three kinds of operands, each with a pass condition that is derived, not measured:
  'A'   integers in [-4, 4] (bias, aux, a pre-filled C too).  With sum K_t <= 7215 every product and every partial sum, in any order, is an
        integer below 2^24 in magnitude, so fp32 is exact whatever the reduction order, split count or wave partition: bit-exact.
  'B1'  A random fp32 (all 24 mantissa bits), B a selection matrix: one power of two (2^-3 .. 2^3) per column, placed by a permutation, so
        C[m][n] = A[m][pi(n)] * 2^e exactly.  'B2': the roles swapped (one nonzero per row of A).  Bit-exact.
  'C'   standard normal operands: |C - C64| <= (K_total + 16) 2^-24 (|A| |B|)[m][n] + 2^-24 |C64| (any summation order of K_total products
        with one rounding each; 16 covers the fold over wave partials, the split-K second pass and the bias).  K_total <= 320 only.
  'G'   integer pre-activations |v| <= 6 for the GELU epilogues (A integers in [-5, 5], B a +-1 selection matrix, bias in [-1, 1]).

Every operand and output lives inside a larger owned buffer: GUARD_ROWS rows before and after, PAD guard columns (ld = cols + PAD; the
tight variant has ld = cols and the guard rows only).  Input guards are NaN, output buffers are filled with SENTINEL.
"""
import math
from dataclasses import dataclass, field

import numpy as np

GUARD_ROWS = 4                    # before and after the logical rows: 8 in all
PAD = 5
SENTINEL_BITS = 0xCAFEBABE        # a finite fp32 (-8346975.0) no case can produce
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
U = 2.0 ** -24                    # fp32 unit roundoff

EPI_NONE, EPI_GELU, EPI_MUL_GELU_GRAD, EPI_ADD = 0, 1, 2, 3
MAX_TERMS, MAX_PROBLEMS, TERM_POOL, MAX_JOBS = 12, 26, 32, 10
TT = [(0, 0), (0, 1), (1, 0), (1, 1)]


class Buf:
    """[rows][cols] fp32 inside an owned [GUARD_ROWS + rows + GUARD_ROWS][ld] buffer."""

    def __init__(self, rows, cols, pad, fill):
        self.rows, self.cols, self.ld = rows, cols, cols + (PAD if pad else 0)
        self.full = np.full((rows + 2 * GUARD_ROWS, self.ld), fill, np.float32)

    @property
    def win(self):
        return self.full[GUARD_ROWS:GUARD_ROWS + self.rows, :self.cols]

    @property
    def offset(self):             # of the logical origin, in elements
        return GUARD_ROWS * self.ld


def input_buf(values, pad):
    b = Buf(values.shape[0], values.shape[1], pad, np.nan)
    b.win[...] = values
    return b


def output_buf(rows, cols, pad):
    return Buf(rows, cols, pad, SENTINEL)


def op_read(buf, rows, cols, trans):
    """op(X)[r][c] read the way the ABI addresses it: base pointer + leading dimension, through the FLAT owned buffer."""
    flat = buf.full.reshape(-1)
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return flat[buf.offset + (c * buf.ld + r if trans else r * buf.ld + c)]


def outside_is_sentinel(full, buf):
    """`full`: the owned buffer after the launch (same shape as buf.full).  True when everything outside the logical window still holds SENTINEL."""
    bits = np.array(full, np.float32, copy=True)
    bits[GUARD_ROWS:GUARD_ROWS + buf.rows, :buf.cols] = SENTINEL
    return bool((bits.view(np.uint32) == SENTINEL_BITS).all())


# ---------------------------------------------------------------------------------------------- operand kinds
def _ints(rng, shape, lim=4):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)


def _selection(rng, k, n, signs_only):
    """[k][n], one nonzero per column at row pi(n) (pi a permutation where k >= n)."""
    s = np.zeros((k, n), np.float32)
    rows = rng.permutation(k)[:n] if k >= n else rng.integers(0, k, size=n)
    if signs_only:
        vals = rng.choice(np.array([-1.0, 1.0], np.float32), size=n)
    else:
        vals = (2.0 ** rng.integers(-3, 4, size=n)).astype(np.float32)
    s[rows, np.arange(n)] = vals
    return s


def operands(rng, kind, M, N, ks):
    """Logical op(A_t) [M][K_t] and op(B_t) [K_t][N] for every term, generated on the concatenated K and cut into the terms."""
    kt = int(sum(ks))
    if kind == 'A':
        a, b = _ints(rng, (M, kt)), _ints(rng, (kt, N))
    elif kind == 'C':
        a, b = rng.standard_normal((M, kt)).astype(np.float32), rng.standard_normal((kt, N)).astype(np.float32)
    elif kind == 'B1':
        a, b = rng.standard_normal((M, kt)).astype(np.float32), _selection(rng, kt, N, False)
    elif kind == 'B2':
        a, b = _selection(rng, kt, M, False).T.copy(), rng.standard_normal((kt, N)).astype(np.float32)
    elif kind == 'G':
        a, b = _ints(rng, (M, kt), 5), _selection(rng, kt, N, True)
    else:
        raise ValueError(kind)
    cuts = np.cumsum([0] + list(ks))
    return [(a[:, cuts[i]:cuts[i + 1]], b[cuts[i]:cuts[i + 1], :]) for i in range(len(ks))]


def round_bf16(x):
    """fp32 -> bfloat16 (round to nearest even) -> fp32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


# ---------------------------------------------------------------------------------------------- GELU in fp64
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(x):
    x = np.asarray(x, np.float64)
    return x * 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------- dpn_sgemm_batch: specs
@dataclass
class P:
    """One problem of a dpn_sgemm_batch launch.  ks: K_t per term; zero_k: the term that passes k_term = 0 (meaning the problem's K)."""
    M: int
    N: int
    ks: tuple
    ta: int = None            # None: taken from the test's (ta, tb) parameter
    tb: int = None
    bias: bool = True
    asum: bool = False
    epi: int = EPI_NONE
    aux_out: bool = False
    zero_k: int = 0


@dataclass
class Launch:
    name: str
    probs: list
    jobs: tuple = ()          # n_blocks per ride-along column-sum job
    form: str = None          # the template instantiation the host must choose: '256x1' or '64x2'
    kinds: tuple = ('A',)


def host_form(probs):
    """The host heuristic of sgemm_batch_launch, restated: <256,1> when every problem is one 256-deep k-tile and the launch has at most 512 output tiles."""
    single = all(sum((k + 255) // 256 for k in p.ks) <= 1 for p in probs)
    tiles = sum(((p.M + 31) // 32) * ((p.N + 31) // 32) for p in probs)
    return '256x1' if single and tiles <= 512 else '64x2'


def _mixed_launch():
    """Exactly 26 problems, 32 terms and 10 jobs; a 1 x 1 problem beside a 65 x 70 one (the grid is the maximum: most of the small problem's
    workgroups return early); own ta / tb, term counts and K_t per problem."""
    shapes = [(1, 1), (65, 70), (33, 32), (31, 33), (32, 1), (1, 70), (2, 65), (64, 3)]
    probs = []
    for i in range(26):
        M, N = shapes[i % len(shapes)]
        ks = {1: (64, 65, 7), 2: (200, 1), 3: (33, 31, 2, 129)}.get(i, ((1, 31, 64, 100, 256, 257)[i % 6],))
        probs.append(P(M, N, ks, ta=(i >> 1) & 1, tb=i & 1, bias=bool(i % 3), asum=len(ks) == 1 and i % 4 == 0,
                       epi=EPI_ADD if i % 5 == 2 else EPI_NONE, zero_k=len(ks) - 1))
    probs[25] = P(33, 31, (130,), ta=1, tb=1, bias=True, asum=True)
    return Launch('mixed_26_problems_32_terms_10_jobs', probs, jobs=(1, 7, 8, 9, 72, 2, 3, 16, 5, 33), form='64x2')


def batch_launches():
    L = []
    # ragged M, N at K = 256: every value of {1, 31, 32, 33, 65} x {1, 32, 33, 70} at least once per axis
    for M, N in [(1, 1), (31, 32), (32, 33), (33, 70), (65, 70), (65, 1), (1, 70), (33, 33)]:
        L.append(Launch('mn_%dx%d_k256' % (M, N), [P(M, N, (256,))], form='256x1', kinds=('A', 'C')))
    # ragged K, single tile
    for K in (1, 2, 31, 255):
        L.append(Launch('k%d_single' % K, [P(33, 33, (K,))], form='256x1', kinds=('A', 'C')))
    # ragged K, pipelined: K > 256 selects <64,2>; K <= 256 reaches it beside a 257-deep problem.  64-deep tiles: K = 64 is one tile,
    # 65 and 127 two, 129 three (the three prologue branches of the double-buffered loop), 257 and 320 five
    for K in (257, 320):
        L.append(Launch('k%d_pipelined' % K, [P(33, 33, (K,))], form='64x2', kinds=('A', 'C')))
    for K, tiles in ((64, 1), (65, 2), (127, 2), (129, 3)):
        L.append(Launch('k%d_pipelined_%dtile' % (K, tiles), [P(33, 33, (K,)), P(33, 33, (257,))], form='64x2', kinds=('A',)))
        L.append(Launch('k%d_pipelined_2term' % K, [P(33, 33, (K - 31, 31))], form='64x2', kinds=('A', 'C')))
    # multi-term, different K_t; a term that ends on a tile boundary followed by one that does not; k_term = 0 meaning K on one term
    L.append(Launch('terms2', [P(33, 33, (64, 65), zero_k=1)], form='64x2', kinds=('A', 'C')))
    L.append(Launch('terms3', [P(65, 70, (1, 64, 200), zero_k=2)], form='64x2', kinds=('A', 'C')))
    L.append(Launch('terms12', [P(33, 33, (1, 64, 65, 200, 2, 31, 128, 63, 7, 256, 33, 100), zero_k=3)], form='64x2'))
    L.append(_mixed_launch())
    # differently shaped problems in the single-tile form: the grid is the 65 x 70 problem's, so five of the 1 x 1 problem's six workgroups return early
    L.append(Launch('mixed_single_tile_1x1_beside_65x70', [P(1, 1, (200,)), P(65, 70, (256,), asum=True)], form='256x1', kinds=('A', 'C')))
    # dispatch edge: 512 output tiles of one k-tile each run <256,1>, 513 run <64,2>
    L.append(Launch('dispatch_512_tiles', [P(512, 1024, (8,), bias=False)], form='256x1'))
    L.append(Launch('dispatch_513_tiles', [P(512, 1024, (8,), bias=False), P(1, 1, (8,))], form='64x2'))
    # asum: M and K ragged, N > 32 (only the blockIdx.x == 0 tiles may write it), both forms
    L.append(Launch('asum_single', [P(33, 70, (255,), asum=True)], form='256x1', kinds=('A', 'C')))
    L.append(Launch('asum_pipelined', [P(65, 33, (129,), asum=True), P(1, 70, (300,), asum=True)], form='64x2', kinds=('A', 'C')))
    # epilogues
    L.append(Launch('epi_add', [P(33, 70, (255,), epi=EPI_ADD)], form='256x1'))
    L.append(Launch('epi_add_pipelined', [P(33, 70, (100, 29), epi=EPI_ADD)], form='64x2'))
    L.append(Launch('epi_gelu', [P(33, 70, (255,), epi=EPI_GELU)], form='256x1', kinds=('G',)))
    L.append(Launch('epi_gelu_aux_out', [P(33, 70, (255,), epi=EPI_GELU, aux_out=True), P(65, 33, (257,), epi=EPI_GELU, aux_out=True)],
                    form='64x2', kinds=('G',)))
    L.append(Launch('epi_mul_gelu_grad', [P(33, 70, (255,), epi=EPI_MUL_GELU_GRAD), P(31, 1, (80,), epi=EPI_MUL_GELU_GRAD)],
                    form='256x1', kinds=('G',)))
    # column-sum jobs: the loop over blocks is unrolled by 8
    L.append(Launch('jobs', [P(33, 33, (31,))], jobs=(1, 7, 8, 9, 72), form='256x1'))
    # full-mantissa pass-through, both instantiations
    L.append(Launch('passthrough_k256', [P(33, 70, (256,), bias=False)], form='256x1', kinds=('B1', 'B2')))
    L.append(Launch('passthrough_k320_2term', [P(33, 70, (200, 120), bias=False)], form='64x2', kinds=('B1', 'B2')))
    return L


BATCH = batch_launches()


def batch_ids(kind):
    return [l_.name for l_ in BATCH if kind in l_.kinds]


def batch_by_name(name):
    return next(l_ for l_ in BATCH if l_.name == name)


@dataclass
class BuiltProblem:
    spec: P
    ta: int
    tb: int
    A: list
    B: list
    bias: Buf
    aux: Buf
    C: Buf
    aux_out: Buf
    asum: Buf
    K: int = 0
    k_term: list = field(default_factory=list)


def build_batch(launch, kind, tt, pad, seed=0):
    """Numpy buffers of every problem and job of a launch.  Returns (problems, jobs); a job is (partial, out_a, out_b, n_blocks)."""
    rng = np.random.default_rng([seed, len(launch.name), sum(map(ord, launch.name)), tt[0], tt[1], int(pad)])
    probs = []
    for p in launch.probs:
        ta, tb = (tt[0] if p.ta is None else p.ta), (tt[1] if p.tb is None else p.tb)
        terms = operands(rng, kind, p.M, p.N, p.ks)
        q = BuiltProblem(p, ta, tb, [input_buf(a.T if ta else a, pad) for a, _ in terms], [input_buf(b.T if tb else b, pad) for _, b in terms],
                         None, None, output_buf(p.M, p.N, pad), None, None)
        if p.bias:
            q.bias = input_buf(_ints(rng, (1, p.N), 1 if kind == 'G' else 4) if kind in 'AG' else rng.standard_normal((1, p.N)).astype(np.float32), pad)
        if p.epi in (EPI_MUL_GELU_GRAD, EPI_ADD):            # aux and aux_out share the ldc of C
            q.aux = input_buf(_ints(rng, (p.M, p.N), 6 if kind == 'G' else 4), pad)
        if p.aux_out:
            q.aux_out = output_buf(p.M, p.N, pad)
        if p.asum:
            q.asum = output_buf(1, p.M, pad)
        q.K = p.ks[p.zero_k]
        q.k_term = [0 if t == p.zero_k else k for t, k in enumerate(p.ks)]
        probs.append(q)
    jobs = []
    for nb in launch.jobs:
        # partial is [n_blocks][2][256] by the ABI (no leading dimension): guard rows only
        jobs.append((input_buf(_ints(rng, (nb, 512)), False), output_buf(1, 256, pad), output_buf(1, 256, pad), nb))
    return probs, jobs


def reference_problem(q):
    """The ABI's definition in fp64, every operand read through its base offset and leading dimension.  Returns a dict with the pre-activation
    `v`, the output `C`, `asum` (or None), `absprod` = (|A| |B|)[m][n] alone, as the kind-C bound takes it, and `magnitude` = absprod + |bias|
    (+ |aux|), which bounds every partial sum of a kind-A case."""
    p = q.spec
    v = np.zeros((p.M, p.N), np.float64)
    ab = np.zeros((p.M, p.N), np.float64)
    for t, k in enumerate(p.ks):
        a = op_read(q.A[t], p.M, k, q.ta).astype(np.float64)
        b = op_read(q.B[t], k, p.N, q.tb).astype(np.float64)
        v += a @ b
        ab += np.abs(a) @ np.abs(b)
    mag = ab
    if q.bias is not None:
        bias = op_read(q.bias, 1, p.N, 0).astype(np.float64)
        v += bias
        mag = mag + np.abs(bias)
    aux = op_read(q.aux, p.M, p.N, 0).astype(np.float64) if q.aux is not None else None
    C = {EPI_NONE: lambda: v, EPI_GELU: lambda: gelu64(v), EPI_MUL_GELU_GRAD: lambda: v * gelu_grad64(aux), EPI_ADD: lambda: v + aux}[p.epi]()
    if p.epi == EPI_ADD:
        mag = mag + np.abs(aux)
    asum = op_read(q.A[0], p.M, p.ks[0], q.ta).astype(np.float64).sum(1) if p.asum else None
    return dict(v=v, C=C, asum=asum, absprod=ab, magnitude=mag)


def reference_job(job):
    part = op_read(job[0], job[3], 512, 0).astype(np.float64)
    return part[:, :256].sum(0), part[:, 256:].sum(0)


def kind_c_bound(k_total, absprod, c64):
    """(K_total + 16) 2^-24 (|A| |B|)[m][n] + 2^-24 |C64|; `absprod` is |A||B| alone, without the bias or a pre-filled C."""
    return (k_total + 16) * U * absprod + U * np.abs(c64)


def fma_chain_fp32(a, b, bias=None):
    """Sequential fp32 evaluation, one rounding per product-and-add (the fused multiply-add through an exact fp64 product)."""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a64[:, k:k + 1] * b64[k:k + 1, :]).astype(np.float32)
    if bias is not None:
        acc = (acc + bias.astype(np.float32)).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------- dpn_sgemm: specs
def sgemm_plan(M, N, K, has_ws, ws_bytes):
    """dpn_sgemm's host arithmetic restated: (splits, k_per_split)."""
    tiles = ((N + 31) // 32) * ((M + 31) // 32)
    splits = 1
    if has_ws and tiles < 256 and K >= 1024:
        splits = min((512 + tiles - 1) // tiles, K // 256, 32)
        while splits > 1 and splits * (M * N + M) * 4 > ws_bytes:
            splits -= 1
        splits = max(splits, 1)
    kps = (K + splits - 1) // splits
    kps = ((kps + 31) // 32) * 32
    return (K + kps - 1) // kps, kps


def sgemm_ws_bytes(M, N, splits):
    return splits * (M * N + M) * 4


@dataclass
class S:
    """One dpn_sgemm call.  ws: None (null workspace), 'exact' (sized for the wanted split count), 'minus1' (one byte less), 'zero' (zero
    bytes behind a non-null pointer)."""
    M: int
    N: int
    K: int
    bias: bool = True
    asum: bool = True
    accumulate: int = 0
    ws: str = None

    @property
    def name(self):
        return '%dx%dx%d_%s%s%s_ws_%s' % (self.M, self.N, self.K, 'b' if self.bias else '', 's' if self.asum else '', 'acc' if self.accumulate else '', self.ws)


def sgemm_cases():
    c = []
    for K in (1, 33, 1024, 1030):                                    # no workspace: a single pass whatever K
        for acc in (0, 1):
            c.append(S(33, 17, K, accumulate=acc))
    c.append(S(33, 17, 33, bias=False, asum=False))
    for K in (1024, 1030, 7215):                                     # the split path
        for M, N in ((1, 1), (33, 17), (159, 256)):
            c.append(S(M, N, K, accumulate=1, ws='exact'))
    for K in (1030, 7215):                                           # workspace sizes
        for M, N in ((33, 17), (159, 256)):
            c.append(S(M, N, K, accumulate=1, ws='minus1'))
            c.append(S(M, N, K, accumulate=1, ws='zero'))
    c.append(S(33, 17, 1023, accumulate=1, ws='exact'))              # just outside the split condition: K < 1024 ...
    c.append(S(512, 512, 1024, accumulate=1, ws='exact'))            # ... and 256 output tiles
    c.append(S(33, 17, 7215, bias=False, asum=False, ws='exact'))
    return c


SGEMM = sgemm_cases()
SGEMM_KIND_C = [S(33, 17, 1), S(33, 17, 33, accumulate=1), S(65, 70, 320)]


def sgemm_workspace(s):
    """(has_ws, ws_bytes, splits, kps) of a case, with the wanted split count asserted against ceil(K / kps)."""
    if s.ws is None:
        return (False, 0) + sgemm_plan(s.M, s.N, s.K, False, 0)
    wanted, kps = sgemm_plan(s.M, s.N, s.K, True, 1 << 62)
    assert wanted == -(-s.K // kps)
    ws_bytes = {'exact': sgemm_ws_bytes(s.M, s.N, wanted), 'minus1': sgemm_ws_bytes(s.M, s.N, wanted) - 1, 'zero': 0}[s.ws]
    return (True, ws_bytes) + sgemm_plan(s.M, s.N, s.K, True, ws_bytes)


def build_sgemm(s, kind, tt, pad, seed=0):
    rng = np.random.default_rng([seed, s.M, s.N, s.K, tt[0], tt[1], int(pad), s.accumulate])
    (a, b), = operands(rng, kind, s.M, s.N, (s.K,))
    A, B = input_buf(a.T if tt[0] else a, pad), input_buf(b.T if tt[1] else b, pad)
    draw = (lambda shape: _ints(rng, shape)) if kind == 'A' else (lambda shape: rng.standard_normal(shape).astype(np.float32))
    bias = input_buf(draw((1, s.N)), pad) if s.bias else None
    C = output_buf(s.M, s.N, pad)
    c0 = None
    if s.accumulate:
        c0 = draw((s.M, s.N))
        C.win[...] = c0
    asum = output_buf(1, s.M, pad) if s.asum else None
    return dict(A=A, B=B, bias=bias, C=C, c0=c0, asum=asum)


def reference_sgemm(s, tt, d):
    a = op_read(d['A'], s.M, s.K, tt[0]).astype(np.float64)
    b = op_read(d['B'], s.K, s.N, tt[1]).astype(np.float64)
    v, ab = a @ b, np.abs(a) @ np.abs(b)
    mag = ab                                # absprod stays |A||B| alone (the kind-C bound); magnitude bounds the partial sums of kind A
    if s.bias:
        bias = op_read(d['bias'], 1, s.N, 0).astype(np.float64)
        v, mag = v + bias, mag + np.abs(bias)
    if s.accumulate:
        v, mag = v + d['c0'], mag + np.abs(d['c0'])
    return dict(C=v, asum=a.sum(1) if s.asum else None, absprod=ab, magnitude=mag, asum_abs=np.abs(a).sum(1))


# ---------------------------------------------------------------------------------------------- dpn_sgemm_ln
LN_M, LN_N = (1, 31, 33, 287), (1, 33, 192)


def build_ln(mode, M, N, tb, pad, seed=0):
    """Inputs of a dpn_sgemm_ln call in the magnitudes of test_layernorm_folded_into_gemm_both_modes.  x / r / y / xhat rows are 256 wide by the
    ABI (no leading dimension): guard rows only."""
    rng = np.random.default_rng([seed, mode, M, N, tb, int(pad)])
    n32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(x=input_buf(n32(M, 256), False), r=input_buf(n32(M, 256), False), gamma=input_buf((rng.random((1, 256)) + 0.5).astype(np.float32), False),
             beta=input_buf(n32(1, 256), False), bias=input_buf(n32(1, N), pad))
    w = n32(256, N) / np.float32(16)
    d['B'] = input_buf(w.T if tb else w, pad)
    d['C'], d['y'] = output_buf(M, N, pad), output_buf(M, 256, False)
    if mode == 1:
        d['xhat'], d['rstd'], d['pre'] = output_buf(M, 256, False), output_buf(1, M, False), output_buf(M, N, pad)
    else:                                   # x is the cotangent g, r the saved xhat of some forward, rstd_in its rstd
        s = n32(M, 256).astype(np.float64)
        rstd = 1.0 / np.sqrt(s.var(1) + 1e-5)
        d['r'] = input_buf(((s - s.mean(1, keepdims=True)) * rstd[:, None]).astype(np.float32), False)
        d['rstd_in'] = input_buf(rstd.astype(np.float32)[None, :], False)
        d['partial'] = output_buf((M + 31) // 32, 512, False)
    return d


def reference_ln(mode, M, N, tb, d):
    f = lambda k, rows, cols, t=0: op_read(d[k], rows, cols, t).astype(np.float64)
    gamma, B, bias = f('gamma', 1, 256), f('B', 256, N, tb), f('bias', 1, N)
    if mode == 1:
        s = f('x', M, 256) + f('r', M, 256)
        rstd = 1.0 / np.sqrt(s.var(1) + 1e-5)
        xhat = (s - s.mean(1, keepdims=True)) * rstd[:, None]
        y = xhat * gamma + f('beta', 1, 256)
        pre = y @ B + bias
        return dict(y=y, xhat=xhat, rstd=rstd[None, :], pre=pre, C=gelu64(pre))
    g, xh, rstd = f('x', M, 256), f('r', M, 256), f('rstd_in', 1, M)[0]
    tg = g * gamma
    gs = rstd[:, None] * (tg - tg.mean(1, keepdims=True) - xh * (tg * xh).mean(1, keepdims=True))
    nb = (M + 31) // 32
    partial = np.zeros((nb, 512))
    for b in range(nb):                     # the last row block sums only the rows that exist
        rows = slice(32 * b, min(M, 32 * b + 32))
        partial[b, :256], partial[b, 256:] = (g[rows] * xh[rows]).sum(0), g[rows].sum(0)
    return dict(y=gs, C=gs @ B + bias, partial=partial)


# tolerances of test_layernorm_folded_into_gemm_both_modes (rtol, atol), applied against the fp64 values
LN_TOL = {1: dict(y=(1e-5, 1e-5), rstd=(1e-5, 1e-8), xhat=(1e-5, 1e-5), pre=(1e-4, 1e-4), C=(1e-4, 1e-4)),
          2: dict(y=(1e-4, 1e-5), C=(1e-4, 1e-4), partial=(1e-4, 1e-4))}


def within(got, ref64, rtol, atol):
    got = np.asarray(got, np.float64)
    return bool((np.abs(got - ref64) <= atol + rtol * np.abs(ref64)).all())
