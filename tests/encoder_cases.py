"""Case tables, operand builders, fp64 stage references and pass conditions for the row-local encoder launches (dpn_enc_pack, dpn_enc_fwd,
dpn_enc_bwd: csrc/dpn_encoder_chain.hip) and the attention kernels (dpn_attn_fwd, dpn_attn16_fwd, dpn_attn_bwd).  Imports without a GPU:
tests/test_encoder_cases_cpu.py runs the tables through the numpy model below, tests/test_gpu_encoder_chain.py runs them through the C ABI.

Two facts about the arithmetic make nearly every pass condition derivable ("encoder launches"):
  1. The operand split is reproducible: split22() is row_to_ximg + split8 in numpy (power-of-two row scale from the biased exponent clamped at
     4, hi = f16(x), lo' = f16(2048 (x - hi)), both round-to-nearest-even), and hi + lo'/2048 has at most 23 significant bits, so the kernel's
     fmaf(ac, 1/2048, am) is exact whenever both accumulators are.
  2. Every launch writes its intermediates, so each stage is compared with an fp64 evaluation that starts from the GPU's OWN upstream tensor:
     errors do not compound, every bound is a one-stage bound.

Operand kinds (activations / weights):
  'A'   integers in [-4, 4] everywhere.  f16 holds them exactly, lo' = 0, every product and partial sum is an integer below 2^24: a GEMM
        on them is bit-exact in any order (exact_gemm32 proves it per case from the operands' quanta).
  'AL'  integer activations against weights i + j / 1024 (|i| <= 4, |j| <= 3): the split of such a weight is lossless and has a lo' plane
        wherever |i| >= 2 and j is odd, the sums stay exact.  Bit-exact like A, and a dropped hi.lo' product changes the result at any K (the
        worst-case bound of kind C cannot see it at K = 768).
  'S'   full-mantissa fp32 activations against SELECTION weights: one power of two (2^-3 .. 2^3) per output channel, placed by a permutation
        without fixed points or 2-cycles (W != W^T), a different one per matrix.  y[n] = split22(x)[pi(n)] 2^e exactly; the fp32 additions behind
        it (bias, residual) are reproduced in their order, one rounding each.  (acc_to_global adds the bias as fmaf(..) * rs + b: rs is a power of
        two, so a contraction of the multiplication into the addition rounds once either way -- torch.equal holds for every output.)
  'C'   standard normal activations, weights at the scale of the default init (1/16): gemm_bound().
  'MS', 'MC'  kind S / C with a power-of-two factor per row (2^-100 .. 2^100 mixed inside one 16-row block), an all-zero row and a row with a
        single nonzero.  Row factors commute with the split: MS stays bit-exact.
A GEMM stage is checked bit for bit whenever exact_gemm32() can prove exactness from the operands (kinds A, S, MS; for kind A also behind a
LayerNorm backward, whose integer / power-of-two arithmetic is exact), and against gemm_bound() otherwise.
"""
import math

import numpy as np

from gemm_cases import SENTINEL, SENTINEL_BITS, gelu64, gelu_grad64      # noqa: F401  (re-exported for the tests)

D = 256
U = 2.0 ** -24                     # fp32 unit roundoff
GUARD_ROWS = 4
EPS = 1e-5

# ---------------------------------------------------------------------------------------------- named constants of the pass conditions
C1 = 4             # x 2^-22 |X||B|: activation split (1) + weight split (1) + the dropped lo'.lo' product (1) + all second-order terms (1)
C2 = 16            # x 2^-24 |X||B| beside K: the cross accumulator's own rounding (< 1), the recombining fmaf, the fold of partial tiles, slack
ABS_SPLIT = 2.0 ** -36             # f16 subnormal spacing 2^-24, half of it, through the 2^-11 of lo': absolute split error of a scaled entry
LN_ADDS = 16       # fp32 LayerNorm: 8 serial + 5 tree additions of a row reduction, the subtraction of the mean, two of slack
LNB_OPS = 20       # fp32 LayerNorm backward: the same reduction (13), two products, two subtractions, the multiplication by rstd, slack
MARGIN = 4         # on a measured yardstick (torch's fp32 evaluation against fp64): library erff / expf differ by a few ulps between implementations
SECOND_ORDER = 1.0 + 2.0 ** -8     # first-order propagation through 1 / sigma, valid while rstd E < 2^-10 (asserted)


# ---------------------------------------------------------------------------------------------- the split
class Split:
    """split22 of a [rows][K] fp32 array: sc (the power of two the row is multiplied by), inv (its inverse, the kernel's rscale), the two
    f16 planes of the SCALED row and val = hi + lo'/2048 (scaled, fp32, exact)."""

    def __init__(self, sc, inv, hi, lo):
        self.sc, self.inv, self.hi, self.lo = sc, inv, hi, lo
        self.val = (hi.astype(np.float64) + lo.astype(np.float64) / 2048.0).astype(np.float32)

    def recombined(self):
        return self.val * self.inv[:, None]


def _f16_planes(s):
    with np.errstate(over='ignore', invalid='ignore'):      # an |entry| >= 65520 becomes inf, as v_cvt_f16_f32 makes it (the status-flag case only)
        hi = s.astype(np.float16)
        lo = ((s - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def split22(x, extra_max=None):
    """row_to_ximg + split8.  x [rows][K] fp32; extra_max [rows]: a maximum the row shares with other operands (the q / k / v backward)."""
    x = np.ascontiguousarray(x, np.float32)
    m = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    if extra_max is not None:
        m = np.maximum(m, np.asarray(extra_max, np.float32))
    eb = ((m.astype(np.float32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xff)).astype(np.int64)
    eb = np.maximum(eb, 4)                                   # zero / tiny rows: any scale does
    sc = ((257 - eb).astype(np.uint32) << np.uint32(23)).view(np.float32)
    inv = ((eb - 3).astype(np.uint32) << np.uint32(23)).view(np.float32)
    hi, lo = _f16_planes(x * sc[:, None])
    return Split(sc, inv, hi, lo)


def split_w(w):
    """dpn_enc_pack's split of a weight matrix: unscaled."""
    return _f16_planes(np.ascontiguousarray(w, np.float32))


def emulate_gemm(X, B, alter=None):
    """The kernel's GEMM arithmetic in numpy: y = X B, X [M][K] activations (split22 per row), B [K][N] the weight image (split unscaled),
    three products, two fp32 accumulators advanced one 32-wide k-step at a time, fmaf(cross, 1/2048, main) * rscale.
    alter: 'no_hi_lo' drops hi.lo', 'no_lo_hi' drops lo'.hi (the teeth tests)."""
    sx = split22(X)
    bh, bl = (p.astype(np.float64) for p in split_w(B))
    xh, xl = sx.hi.astype(np.float64), sx.lo.astype(np.float64)
    m = np.zeros((X.shape[0], B.shape[1]), np.float32)
    c = np.zeros_like(m)
    for k0 in range(0, X.shape[1], 32):
        s = slice(k0, k0 + 32)
        m = (m + xh[:, s] @ bh[s]).astype(np.float32)
        if alter != 'no_hi_lo':
            c = (c + xh[:, s] @ bl[s]).astype(np.float32)
        if alter != 'no_lo_hi':
            c = (c + xl[:, s] @ bh[s]).astype(np.float32)
    y = (c.astype(np.float64) / 2048.0 + m.astype(np.float64)).astype(np.float32)
    return y * sx.inv[:, None]


def _quantum(a):
    """The largest power of two every entry of `a` is a multiple of (inf for an all-zero array)."""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return math.inf
    m, e = np.frexp(a)
    mant = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mant & -mant).astype(np.float64))
    return float(2.0 ** (e - 53 + tz).min())


def _is_pow2(a):
    m, _ = np.frexp(np.abs(a))
    return bool(np.all(m == 0.5))


def exact_gemm32(X, B):
    """The fp32 result of the kernel's y = X B when the operands PROVE that no accumulation rounds, else None.
    (a) at most one nonzero product per output and power-of-two weights: y = split22(x)[k] B[k][n], exact;
    (b) lossless splits of X and B with no lo'.lo' product, and every partial sum of each accumulator a multiple of a quantum q with
        magnitude below 2^24 q."""
    X, B = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(B, np.float32)
    sx = split22(X)
    X64, B64 = X.astype(np.float64), B.astype(np.float64)
    if ((X != 0).astype(np.float64) @ (B != 0).astype(np.float64)).max(initial=0) <= 1 and _is_pow2(B[B != 0]):
        return (sx.val.astype(np.float64) @ B64).astype(np.float32) * sx.inv[:, None]
    bh, bl = split_w(B)
    with np.errstate(over='ignore', invalid='ignore'):
        lossless = np.array_equal(sx.val.astype(np.float64), X64 * sx.sc.astype(np.float64)[:, None])
    xh, xl, b, bl = sx.hi.astype(np.float64), sx.lo.astype(np.float64), bh.astype(np.float64), bl.astype(np.float64)
    if not lossless or not np.array_equal(b + bl / 2048.0, B64) or (np.abs(xl) @ np.abs(bl)).max(initial=0) != 0:      # (the kernel drops lo'.lo')
        return None
    for pa, pb in ((xh, b), (xh, bl), (xl, b)):
        q = _quantum(pa) * _quantum(pb)
        if math.isfinite(q) and (np.abs(pa) @ np.abs(pb)).max() >= 2.0 ** 24 * q:
            return None
    qc = min(_quantum(xh) * _quantum(bl), _quantum(xl) * _quantum(b))                                                  # the cross accumulator holds both
    if math.isfinite(qc) and (np.abs(xh) @ np.abs(bl) + np.abs(xl) @ np.abs(b)).max() >= 2.0 ** 24 * qc:
        return None
    y64 = xh @ b + (xh @ bl + xl @ b) / 2048.0
    y = y64.astype(np.float32)
    if not np.array_equal(y.astype(np.float64), y64):
        return None
    return y * sx.inv[:, None]


def gemm_bound(X, B, y64):
    """Elementwise bound on |kernel(X B) - fp64(X B)| for ANY fp32 operands (|B| < 32768), X the exact fp32 input of the stage:
        C1 2^-22 S + (K + C2) 2^-24 S + 2^-24 |y| + 2^-36 (rscale_m sum_k |B[k][n]| + sum_k |X[m][k]|),   S = (|X||B|)[m][n].
    Split of a scaled entry s (|s| < 16): |s - hi| <= 2^-11 |s|, and lo' rounds 2048 (s - hi) with relative error 2^-11 or, in f16's subnormal
    range, absolute error 2^-25: |s - (hi + lo'/2048)| <= 2^-22 |s| + 2^-36; the same for an unscaled weight.  Two split errors and the dropped
    lo'.lo' (<= 2^-22 |s||w|) give three of C1, the fourth covers every product of two small terms.  f16 x f16 products are exact in fp32; K of
    them are added into the main accumulator with one rounding each in some order (K 2^-24 S); the cross accumulator holds 2 K terms 2^-11 as
    large (< 2^-24 S), the recombining fmaf rounds once (2^-24 |y|): C2 = 16 covers these with room.  The row scale is a power of two."""
    X64, B64 = np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(B, np.float64))
    S = X64 @ B64
    inv = split22(X).inv.astype(np.float64)
    return (C1 * 2.0 ** -22 + (X.shape[1] + C2) * U) * S + U * np.abs(y64) + ABS_SPLIT * (inv[:, None] * B64.sum(axis=0)[None, :] + X64.sum(axis=1)[:, None])


class Stage:
    """Reference of one output tensor: ref (fp64), bound (fp64, elementwise; None when exact is given), exact (fp32 or None)."""

    def __init__(self, ref, bound=None, exact=None):
        self.ref, self.bound, self.exact = np.asarray(ref, np.float64), bound, exact


def gemm_stage(X, B, post=()):
    """y = X B, then the fp32 additions `post` in the kernel's order (bias, residual), one rounding each."""
    y64 = np.asarray(X, np.float64) @ np.asarray(B, np.float64)      # (an fp64 X -- the CPU composition test -- is not rounded for the reference)
    X, B = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(B, np.float32)
    bound = gemm_bound(X, B, y64)
    exact = exact_gemm32(X, B)
    for p in post:
        y64 = y64 + np.asarray(p, np.float64)
        bound = bound + U * np.abs(y64)
        if exact is not None:
            exact = (exact + np.asarray(p, np.float32)).astype(np.float32)
    return Stage(y64, None if exact is not None else bound, exact)


def stage_input(st):
    """What a stage that is not written (the row block kept in registers) hands to the next one: (value fp64, elementwise error bound)."""
    if st.exact is not None:
        return st.exact.astype(np.float64), np.zeros_like(st.ref)
    return st.ref, st.bound


# ---------------------------------------------------------------------------------------------- LayerNorm stages
def ln_fwd_stage(v, E, gamma, beta):
    """(y, xhat, rstd) = LayerNorm_256(v) in fp64 and their bounds, for a kernel that evaluates it in fp32 on v + dv, |dv_i| <= E_i.
    With Em = max_i E_i + LN_ADDS 2^-24 max_i |v_i| (the fp32 mean and subtraction act like one more perturbation of the input):
        |d xhat_i| <= rstd Em (2 + |xhat_i|) SECOND_ORDER + LN_ADDS 2^-24 |xhat_i|      (|d(v_i - mean)| <= 2 Em, |d sigma| <= Em)
        |d y_i|    <= |gamma_i| |d xhat_i| + 2^-23 |y_i|                                   (one fmaf)
        |d rstd|   <= rstd (rstd Em SECOND_ORDER + LN_ADDS 2^-24)                          (variance sum, + eps, sqrt, 1 / x)"""
    v = np.asarray(v, np.float64)
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = v.mean(axis=1, keepdims=True)
    d = v - mean
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + EPS)
    xhat = d * rstd
    y = xhat * g + b
    Em = np.max(E, axis=1, keepdims=True) + LN_ADDS * U * np.abs(v).max(axis=1, keepdims=True)
    assert float((rstd * Em).max()) < 2.0 ** -10, 'the first-order LayerNorm bound needs rstd E < 2^-10'
    bx = rstd * Em * (2.0 + np.abs(xhat)) * SECOND_ORDER + LN_ADDS * U * np.abs(xhat)
    by = np.abs(g) * bx + 2 * U * np.abs(y)
    br = rstd * (rstd * Em * SECOND_ORDER + LN_ADDS * U)
    return Stage(y, by), Stage(xhat, bx), Stage(rstd[:, 0], br[:, 0])


def ln_bwd_stage(t, E, xhat, rstd, gamma, rows_per_block):
    """gx = rstd (gamma t - mean(gamma t) - xhat mean(gamma t xhat)) and the per-workgroup parameter sums partial[block] = (sum t xhat | sum t)
    over the block's rows, in fp64, with bounds for a kernel that evaluates them in fp32 on t + dt, |dt_i| <= E_i.  The map is linear in t:
        |d gx_i| <= rstd (|gamma_i| E_i + mean(|gamma| E) + |xhat_i| mean(|gamma xhat| E))   + LNB_OPS 2^-24 rstd (the same with |t| for E)
        |d partial| <= sum_rows (E |xhat| | E) + (rows_per_block + 4) 2^-24 sum_rows (|t xhat| | |t|)      (fmaf chain, half join, eight waves)
    When every operation is exact in fp32 (kind A: integers, power-of-two rstd) the fp32 evaluation is returned as `exact`."""
    t, E = np.asarray(t, np.float64), np.asarray(E, np.float64)
    xh, rs, g = np.asarray(xhat, np.float64), np.asarray(rstd, np.float64).reshape(-1, 1), np.asarray(gamma, np.float64)
    rows = t.shape[0]

    def lin(a):                                  # the map with absolute values: how a perturbation (or the magnitudes) reaches gx
        ga = np.abs(g) * a
        return np.abs(rs) * (ga + ga.mean(axis=1, keepdims=True) + np.abs(xh) * (ga * np.abs(xh)).mean(axis=1, keepdims=True))
    tg = t * g
    gx = rs * (tg - tg.mean(axis=1, keepdims=True) - xh * (tg * xh).mean(axis=1, keepdims=True))
    bgx = lin(E) + LNB_OPS * U * lin(np.abs(t))
    nb = (rows + rows_per_block - 1) // rows_per_block
    part, bpart = np.zeros((nb, 2 * D)), np.zeros((nb, 2 * D))
    for b in range(nb):
        s = slice(b * rows_per_block, min(rows, (b + 1) * rows_per_block))
        part[b, :D], part[b, D:] = (t[s] * xh[s]).sum(axis=0), t[s].sum(axis=0)
        mag = np.concatenate([np.abs(t[s] * xh[s]).sum(axis=0), np.abs(t[s]).sum(axis=0)])
        bpart[b] = np.concatenate([(E[s] * np.abs(xh[s])).sum(axis=0), E[s].sum(axis=0)]) + (rows_per_block + 4) * U * mag
    exact_gx = exact_p = None
    if not E.any():                              # no rounding anywhere in fp32?  every intermediate representable, every sum of multiples of q below 2^24 q
        m1, m2 = tg.mean(axis=1, keepdims=True), (tg * xh).mean(axis=1, keepdims=True)
        if all(_f32_exact(a) for a in (tg, tg * xh, xh * m2, tg - m1, tg - m1 - xh * m2, gx)) and _sum_exact(tg, 1) and _sum_exact(tg * xh, 1):
            exact_gx = gx.astype(np.float32)
        if _f32_exact(t * xh) and _f32_exact(part) and all(np.abs(a).sum(axis=0).max(initial=0) * (nb > 0) < 2.0 ** 24 * _quantum(a) for a in (t * xh, t)):
            exact_p = part.astype(np.float32)
    return Stage(gx, None if exact_gx is not None else bgx, exact_gx), Stage(part, None if exact_p is not None else bpart, exact_p)


def _f32_exact(a):
    with np.errstate(over='ignore'):
        return bool(np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a))


def _sum_exact(terms, axis):
    q = _quantum(terms)
    return (not math.isfinite(q)) or float(np.abs(terms).sum(axis=axis).max(initial=0)) < 2.0 ** 24 * q


# ---------------------------------------------------------------------------------------------- measured yardsticks (the only ones)
def yardstick(fn32, fn64, x, norm):
    """max |fn32(x) - fn64(x)| / (2^-24 norm(x)) of torch's fp32 evaluation on the CPU, at least 1."""
    x = np.ascontiguousarray(x, np.float32)
    err = np.abs(fn32(x).astype(np.float64) - fn64(x.astype(np.float64)))
    n = norm(x.astype(np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(n > 0, err / (U * n), 0.0)
    return max(1.0, float(np.nanmax(r, initial=0.0)))


def torch_gelu32(x):
    import torch
    return torch.nn.functional.gelu(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def torch_gelu_grad32(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return torch.ops.aten.gelu_backward(torch.ones_like(t), t).numpy()


def torch_exp32(x):
    import torch
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def gelu_stage(pre):
    """act = gelu(pre): |act - gelu64(pre)| <= MARGIN Y 2^-24 |pre|, Y = torch's fp32 GELU on the same inputs against fp64, in units of
    2^-24 |pre| (the cancellation in 1 + erf makes the error absolute in |pre|, not relative to the result)."""
    ref = gelu64(np.asarray(pre, np.float64))
    pre = np.ascontiguousarray(pre, np.float32)
    Y = yardstick(torch_gelu32, gelu64, pre, np.abs)
    return Stage(ref, MARGIN * Y * U * np.abs(pre.astype(np.float64))), Y


def gelu_grad_factor(pre):
    """gelu'(pre) in fp64 and the bound MARGIN Y 2^-24 on the kernel's fp32 value (gelu' is O(1): Y in units of 2^-24)."""
    ref = gelu_grad64(np.asarray(pre, np.float64))
    pre = np.ascontiguousarray(pre, np.float32)
    Y = yardstick(torch_gelu_grad32, gelu_grad64, pre, np.ones_like)
    return ref, MARGIN * Y * U, Y


# ---------------------------------------------------------------------------------------------- operands
N_MATS = 9
SLOT = {'q': 5, 'k': 2, 'v': 7, 'o': 0, 'c1': 8, 'c2': 3, 'p': 6}       # permuted on purpose: a wrong img_off reads another matrix; slots 1, 4 are decoys
MAT_NAMES = ('q', 'k', 'v', 'o', 'c1', 'c2', 'p')
VEC_BIAS = ('bo', 'be1', 'bc1', 'bc2', 'be2', 'bef', 'bn0', 'bn1', 'bn2')
VEC_GAIN = ('g1', 'g2', 'gf')
OPERAND_KINDS = ('A', 'AL', 'S', 'C', 'MS', 'MC')
WEIGHT_KIND = {'A': 'A', 'AL': 'AL', 'S': 'S', 'C': 'C', 'MS': 'S', 'MC': 'C'}
INTEGER_KINDS = ('A', 'AL')
M_EXPONENTS = (-100, -40, 0, 46, 100)
M_EXPONENTS_LN = (-100, -40, 0, 46)      # a launch whose first stage is a LayerNorm FORWARD: the fp32 variance of a 2^100 row is not finite (in torch neither)


def selection_matrix(rng):
    """[256][256], one power of two per row and column at W[n][pi(n)], pi without fixed points and 2-cycles: W != W^T and y = x W^T moves channels."""
    while True:
        pi = rng.permutation(D)
        if not np.any(pi == np.arange(D)) and not np.any(pi[pi] == np.arange(D)):
            break
    w = np.zeros((D, D), np.float32)
    w[np.arange(D), pi] = (2.0 ** rng.integers(-3, 4, size=D)).astype(np.float32)
    return w


def weights(kind):
    """N_MATS matrices in pack order (every slot different, the decoys too) and the twelve parameter vectors, for weight kind A / S / C."""
    rng = np.random.default_rng({'A': 11, 'S': 12, 'C': 13, 'AL': 14}[kind])
    mats = []
    for _ in range(N_MATS):
        if kind == 'A':
            mats.append(rng.integers(-4, 5, size=(D, D)).astype(np.float32))
        elif kind == 'AL':
            mats.append((rng.integers(-4, 5, size=(D, D)) + rng.integers(-3, 4, size=(D, D)) / 1024.0).astype(np.float32))
        elif kind == 'S':
            mats.append(selection_matrix(rng))
        else:
            mats.append((rng.standard_normal((D, D)) / 16.0).astype(np.float32))
    vec = {}
    for n in VEC_BIAS:
        vec[n] = rng.integers(-4, 5, size=D).astype(np.float32) if kind in INTEGER_KINDS else (0.1 * rng.standard_normal(D)).astype(np.float32)
    for n in VEC_GAIN:
        vec[n] = rng.integers(-4, 5, size=D).astype(np.float32) if kind in INTEGER_KINDS else (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    return mats, vec


def row_factors(rows, exps):
    """2^e per row, the exponents mixed inside every 16-row block (row 0 of the first block: e = 0, so that a one-row launch is no bias alone)."""
    return (2.0 ** np.array([exps[(3 * r + r // 16 + 2) % len(exps)] for r in range(rows)], np.float64)).astype(np.float32)


def activations(rng, kind, rows, n, exps=M_EXPONENTS):
    """n [rows][256] activation tensors of one launch.  Kind M: all n share the row factors; row 1 is zero and row 2 has a single nonzero."""
    if kind in INTEGER_KINDS:
        return [rng.integers(-4, 5, size=(rows, D)).astype(np.float32) for _ in range(n)]
    out = [rng.standard_normal((rows, D)).astype(np.float32) for _ in range(n)]
    if kind in ('MS', 'MC'):
        f = row_factors(rows, exps)
        for a in out:
            a *= f[:, None]
            if rows > 1:
                a[1] = 0.0
            if rows > 2:
                keep = a[2, 77]
                a[2] = 0.0
                a[2, 77] = keep
    return out


# ---------------------------------------------------------------------------------------------- case tables
ROWS_RT1 = (1, 15, 16, 17, 33, 287)
ROWS_RT2 = (1, 31, 32, 33, 65, 287)
ROWS_BIG = 2049                                  # once per launch kind, kind A: the row count at which the product picks row_tiles = 2
FWD_KINDS = ('first', 'first_emb', 'tail_next0', 'tail_next1', 'tail_next2')
BWD_KINDS = ((0, 1), (1, 1), (2, 1), (1, 0))
GX_HEAD_ROWS = (None, 1, 30, 'rows')             # (1, 0) only: without gx_head, and gx_head_rows in {1, 30, rows}
REPLICA_FWD = {'kinds': ('first', 'tail_next1'), 'rows': (1024, 1025, 1360, 1361), 'expect': (3, 3, 3, 1)}
REPLICA_BWD = {'kind': (1, 0), 'rows': (1024, 1025, 2048, 2049), 'expect': (2, 2, 2, 1)}
EMB_PARTS = {1: 1, 15: 2, 16: 10, 17: 12, 31: 19, 32: 3, 33: 19, 65: 11, 287: 19, ROWS_BIG: 2}     # slices of the token convolution (the kernel adds them nine at a time)


def rows_table(row_tiles):
    return ROWS_RT1 if row_tiles == 1 else ROWS_RT2


def fwd_cases():
    """(launch kind, row_tiles, rows, operand kind)."""
    out = [(k, rt, r, o) for k in FWD_KINDS for rt in (1, 2) for r in rows_table(rt) for o in OPERAND_KINDS]
    out += [(k, 2, ROWS_BIG, 'A') for k in FWD_KINDS]
    return out


def bwd_cases():
    """((head, body), row_tiles, rows, operand kind)."""
    out = [(k, rt, r, o) for k in BWD_KINDS for rt in (1, 2) for r in rows_table(rt) for o in OPERAND_KINDS]
    out += [(k, 2, ROWS_BIG, 'A') for k in BWD_KINDS]
    return out


def replica_cases():
    out = [('fwd', k, r, e, o) for k in REPLICA_FWD['kinds'] for r, e in zip(REPLICA_FWD['rows'], REPLICA_FWD['expect']) for o in ('A', 'S')]
    out += [('bwd', REPLICA_BWD['kind'], r, e, o) for r, e in zip(REPLICA_BWD['rows'], REPLICA_BWD['expect']) for o in ('A', 'S')]
    return out


def emb_layout(rows):
    n_tok = 30 if rows > 30 else rows // 2
    return n_tok, rows - n_tok, EMB_PARTS[rows]


# ---------------------------------------------------------------------------------------------- launches: inputs
def fwd_inputs(kind, rows, okind):
    """Host inputs of one dpn_enc_fwd launch (name -> fp32 array), seeded by the case."""
    rng = np.random.default_rng(1000 + 31 * rows + 7 * FWD_KINDS.index(kind) + OPERAND_KINDS.index(okind))
    ins = {}
    if kind == 'first':
        ins['xin'], = activations(rng, okind, rows, 1)
    elif kind == 'first_emb':
        n_tok, T, n_parts = emb_layout(rows)
        ak = 'A' if okind in INTEGER_KINDS else 'C'        # the assembly is fp32 additions: magnitudes belong to the GEMM behind it, which reads emb_out
        mk = lambda r: activations(rng, ak, max(r, 1), 1)[0]
        ins['emb_parts'] = np.stack([mk(T) for _ in range(n_parts)])
        ins['emb_token'], ins['emb_pos'] = mk(n_tok), mk(rows)
        ins['emb_bias'], ins['emb_te'] = mk(1)[0], mk(1)[0]
    else:
        ins['o'], ins['x'] = activations(rng, okind, rows, 2, M_EXPONENTS_LN)
    return ins


def bwd_inputs(kind, rows, okind):
    """Host inputs of one dpn_enc_bwd launch.  The saved tensors (xhat*, rstd*, pre) are data to the kernel: normal values / integers, rstd a
    power of two for kind A (then the whole LayerNorm backward is exact in fp32)."""
    head, body = kind
    rng = np.random.default_rng(5000 + 31 * rows + 7 * BWD_KINDS.index(kind) + OPERAND_KINDS.index(okind))
    ins = {}
    sk = 'A' if okind in INTEGER_KINDS else 'C'

    def saved(n):
        return activations(rng, sk, rows, n)

    def rstd():
        return (2.0 ** rng.integers(-2, 2, size=rows)).astype(np.float32) if okind in INTEGER_KINDS else (0.5 + rng.random(rows)).astype(np.float32)
    if head == 1:
        ins['res'], ins['dq'], ins['dk'], ins['dv'] = activations(rng, okind, rows, 4)
        if WEIGHT_KIND[okind] == 'S':            # one nonzero product per output: dq / dk / dv feed the output channels n = 0 / 1 / 2 mod 3
            mats, _ = weights('S')
            for i, n in enumerate(('q', 'k', 'v')):
                target = np.argmax(mats[SLOT[n]] != 0, axis=1)      # row o of W feeds output channel pi(o)
                ins['d' + n][:, target % 3 != i] = 0.0
    elif head == 2:
        ins['dmeta'], = activations(rng, okind, rows, 1)
        ins['xhatf'], = saved(1)
        ins['rstdf'] = rstd()
    else:
        ins['gin'], = activations(rng, okind, rows, 1)
    if body:
        ins['xhat2'], ins['pre'], ins['xhat1'] = saved(3)
        ins['rstd2'], ins['rstd1'] = rstd(), rstd()
    return ins


# ---------------------------------------------------------------------------------------------- launches: stage references
def emb_reference(ins, rows):
    """emb_out in fp32, the additions in the order include/dpn_hip.h states: bit-exact for every operand kind."""
    n_tok, T, n_parts = emb_layout(rows)
    out = np.zeros((rows, D), np.float32)
    for r in range(rows):
        if r < n_tok:
            out[r] = (ins['emb_token'][r] + ins['emb_pos'][r]) + ins['emb_te']
        else:
            v = ins['emb_parts'][0][r - n_tok].copy()
            for p in range(1, n_parts):
                v = v + ins['emb_parts'][p][r - n_tok]
            out[r] = ((v + ins['emb_bias']) + ins['emb_pos'][r]) + ins['emb_te']
    return out


def fwd_reference(kind, ins, gpu, mats, vec):
    """Stage references of one dpn_enc_fwd launch.  gpu: name -> the launch's own output (fp32 arrays): every stage starts from the upstream
    tensor the GPU wrote.  Returns name -> Stage, in stage order, and the measured yardsticks."""
    B = lambda name: mats[SLOT[name]].T         # x W^T contracts over W's columns
    st, yard = {}, {}
    if kind == 'first_emb':
        rows = gpu['emb_out'].shape[0]
        st['emb_out'] = Stage(emb_reference(ins, rows), exact=emb_reference(ins, rows))
    if kind.startswith('first'):
        t = gpu['emb_out'] if kind == 'first_emb' else ins['xin']
    else:
        f1 = gemm_stage(ins['o'], B('o'), (vec['bo'], ins['x']))                                    # F1
        st['x1'], st['xhat1'], st['rstd1'] = ln_fwd_stage(*stage_input(f1), vec['g1'], vec['be1'])
        st['pre'] = gemm_stage(gpu['x1'], B('c1'), (vec['bc1'],))                                   # F2
        st['act'], yard['gelu'] = gelu_stage(gpu['pre'])                                            # F3
        f4 = gemm_stage(gpu['act'], B('c2'), (vec['bc2'], gpu['x1']))                               # F4
        st['x2'], st['xhat2'], st['rstd2'] = ln_fwd_stage(*stage_input(f4), vec['g2'], vec['be2'])
        t = gpu['x2']
    nxt = 1 if kind.startswith('first') else int(kind[-1])
    if nxt == 1:                                                                                    # F5a
        for i, n in enumerate(('q', 'k', 'v')):
            st['y%d' % i] = gemm_stage(t, B(n), (vec['bn%d' % i],))
    elif nxt == 2:                                                                                  # F5b
        st['xf'], st['xhatf'], st['rstdf'] = ln_fwd_stage(t.astype(np.float64), np.zeros(t.shape), vec['gf'], vec['bef'])
        st['y0'] = gemm_stage(gpu['xf'], B('p'), (vec['bn0'],))
    return st, yard


def bwd_reference(kind, ins, gpu, mats, vec, row_tiles):
    """Stage references of one dpn_enc_bwd launch (gpu: the launch's own outputs).  With a body g itself is never written: B1 and partial2 start
    from the fp64 g and its bound."""
    head, body = kind
    rpb = 16 * row_tiles
    st, yard = {}, {}
    B = lambda name: mats[SLOT[name]]            # g W contracts over W's rows: the image is W as stored
    if head == 1:
        X = np.concatenate([ins['dq'], ins['dk'], ins['dv']], axis=1)
        g = gemm_stage(X, np.concatenate([B('q'), B('k'), B('v')], axis=0), (ins['res'],))
    elif head == 2:
        t = gemm_stage(ins['dmeta'], B('p'))
        g, st['partial_f'] = ln_bwd_stage(*stage_input(t), ins['xhatf'], ins['rstdf'], vec['gf'], rpb)
    else:
        g = Stage(ins['gin'], exact=ins['gin'])
    if not body:
        st['gx'] = g
        return st, yard
    st['gs2'], st['partial2'] = ln_bwd_stage(*stage_input(g), ins['xhat2'], ins['rstd2'], vec['g2'], rpb)               # B1
    b2 = gemm_stage(gpu['gs2'], B('c2'))                                                                              # B2
    gg, dgg, yard['gelu_grad'] = gelu_grad_factor(ins['pre'])
    v2, e2 = stage_input(b2)
    st['dpre'] = Stage(v2 * gg, e2 * np.abs(gg) * (1 + 4 * U) + np.abs(v2) * dgg + U * np.abs(v2 * gg))
    b3 = gemm_stage(gpu['dpre'], B('c1'), (gpu['gs2'],))                                                              # B3
    st['gs1'], st['partial1'] = ln_bwd_stage(*stage_input(b3), ins['xhat1'], ins['rstd1'], vec['g1'], rpb)
    st['dout'] = gemm_stage(gpu['gs1'], B('o'))                                                                       # B4
    return st, yard


def outputs_of(direction, kind):
    """Every tensor the launch kind writes."""
    if direction == 'fwd':
        out = ['emb_out'] if kind == 'first_emb' else []
        if kind.startswith('tail'):
            out += ['x1', 'xhat1', 'rstd1', 'pre', 'act', 'x2', 'xhat2', 'rstd2']
        nxt = 1 if kind.startswith('first') else int(kind[-1])
        return out + (['y0', 'y1', 'y2'] if nxt == 1 else ['xf', 'xhatf', 'rstdf', 'y0'] if nxt == 2 else [])
    head, body = kind
    out = ['partial_f'] if head == 2 else []
    return out + (['gs2', 'partial2', 'dpre', 'gs1', 'partial1', 'dout'] if body else ['gx'])


def exact_outputs(direction, kind, okind):
    """The outputs whose condition MUST be equality for this operand kind (GEMM-only outputs of kinds A, AL, S, MS; the embedding assembly
    always): a reference that quietly fell back to a bound there would weaken the test."""
    emb = ['emb_out'] if direction == 'fwd' and kind == 'first_emb' else []
    if okind not in ('A', 'AL', 'S', 'MS'):
        return emb
    if direction == 'fwd':
        if kind.startswith('first'):
            return emb + ['y0', 'y1', 'y2']
        if okind in INTEGER_KINDS:
            return []                            # behind the first LayerNorm the activations are no integers any more
        return ['pre'] + {'0': [], '1': ['y0', 'y1', 'y2'], '2': ['y0']}[kind[-1]]
    head, body = kind
    if not body:
        return ['gx']
    return ['dout'] if okind in ('S', 'MS') else []


def violations(got, st):
    """(number of elements outside the stage's condition, largest error / bound).  Exact stages: value equality, as torch.equal."""
    got = np.asarray(got, np.float32).reshape(st.ref.shape)
    if st.exact is not None:
        return int((got != st.exact.reshape(st.ref.shape)).sum()), 0.0
    err = np.abs(got.astype(np.float64) - st.ref)
    bad = ~(err <= st.bound)                     # a NaN in the result is a violation
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(st.bound > 0, err / st.bound, np.where(err > 0, np.inf, 0.0))
    return int(bad.sum()), float(np.nanmax(ratio, initial=0.0))


# ---------------------------------------------------------------------------------------------- the launches in numpy (CPU self-check)
def _ln32(v, g, b):
    v = v.astype(np.float32)
    mean = (v.sum(axis=1, dtype=np.float32) * np.float32(1.0 / D))[:, None]
    d = v - mean
    rstd = (np.float32(1.0) / np.sqrt((d * d).sum(axis=1, dtype=np.float32) * np.float32(1.0 / D) + np.float32(EPS)))[:, None]
    xhat = d * rstd
    return (xhat * g + b).astype(np.float32), xhat.astype(np.float32), rstd[:, 0].astype(np.float32)


def _lnb32(t, xhat, rstd, g, rpb, pad_row=False):
    t, xhat, rstd = t.astype(np.float32), xhat.astype(np.float32), rstd.astype(np.float32)[:, None]
    tg = t * g
    m1 = (tg.sum(axis=1, dtype=np.float32) * np.float32(1.0 / D))[:, None]
    m2 = ((tg * xhat).sum(axis=1, dtype=np.float32) * np.float32(1.0 / D))[:, None]
    gx = (rstd * (tg - m1 - xhat * m2)).astype(np.float32)
    rows = t.shape[0]
    nb = (rows + rpb - 1) // rpb
    part = np.zeros((nb, 2 * D), np.float32)
    for b in range(nb):
        s = slice(b * rpb, min(rows, (b + 1) * rpb))
        part[b, :D], part[b, D:] = (t[s] * xhat[s]).sum(axis=0, dtype=np.float32), t[s].sum(axis=0, dtype=np.float32)
    if pad_row:
        part[-1] += np.float32(1.0)
    return gx, part


def emulate_fwd(kind, ins, mats, vec, alter=None):
    """A dpn_enc_fwd launch in numpy fp32 with the kernel's GEMM arithmetic: what a correct kernel may write.  alter: see emulate_gemm, plus
    'w_for_wt' (the backward image in a forward GEMM) and 'slot_plus_1' (a wrong image offset)."""
    galt = alter if alter in ('no_hi_lo', 'no_lo_hi') else None

    def mm(x, name):
        w = mats[(SLOT[name] + (1 if alter == 'slot_plus_1' else 0)) % N_MATS]
        return emulate_gemm(x, w if alter == 'w_for_wt' else w.T, galt)
    out = {}
    if kind == 'first_emb':
        out['emb_out'] = emb_reference(ins, ins['emb_pos'].shape[0])
    if kind.startswith('first'):
        t = out['emb_out'] if kind == 'first_emb' else ins['xin']
    else:
        v = ins['x'] + (mm(ins['o'], 'o') + vec['bo'])
        out['x1'], out['xhat1'], out['rstd1'] = _ln32(v, vec['g1'], vec['be1'])
        out['pre'] = mm(out['x1'], 'c1') + vec['bc1']
        out['act'] = torch_gelu32(out['pre'])
        v = out['x1'] + (mm(out['act'], 'c2') + vec['bc2'])
        out['x2'], out['xhat2'], out['rstd2'] = _ln32(v, vec['g2'], vec['be2'])
        t = out['x2']
    nxt = 1 if kind.startswith('first') else int(kind[-1])
    if nxt == 1:
        for i, n in enumerate(('q', 'k', 'v')):
            out['y%d' % i] = mm(t, n) + vec['bn%d' % i]
    elif nxt == 2:
        out['xf'], out['xhatf'], out['rstdf'] = _ln32(t, vec['gf'], vec['bef'])
        out['y0'] = mm(out['xf'], 'p') + vec['bn0']
    return out


def emulate_bwd(kind, ins, mats, vec, row_tiles, alter=None):
    """A dpn_enc_bwd launch in numpy fp32.  alter: emulate_gemm's, 'w_for_wt' (the forward image), 'slot_plus_1', 'pad_row'."""
    head, body = kind
    rpb = 16 * row_tiles
    galt = alter if alter in ('no_hi_lo', 'no_lo_hi') else None

    def img(name):
        w = mats[(SLOT[name] + (1 if alter == 'slot_plus_1' else 0)) % N_MATS]
        return w.T if alter == 'w_for_wt' else w
    out = {}
    if head == 1:
        X = np.concatenate([ins['dq'], ins['dk'], ins['dv']], axis=1)
        g = ins['res'] + emulate_gemm(X, np.concatenate([img('q'), img('k'), img('v')], axis=0), galt)
    elif head == 2:
        g, out['partial_f'] = _lnb32(emulate_gemm(ins['dmeta'], img('p'), galt), ins['xhatf'], ins['rstdf'], vec['gf'], rpb, alter == 'pad_row')
    else:
        g = ins['gin']
    if not body:
        out['gx'] = g.astype(np.float32)
        return out
    out['gs2'], out['partial2'] = _lnb32(g, ins['xhat2'], ins['rstd2'], vec['g2'], rpb, alter == 'pad_row')
    out['dpre'] = (emulate_gemm(out['gs2'], img('c2'), galt) * torch_gelu_grad32(ins['pre'])).astype(np.float32)
    out['gs1'], out['partial1'] = _lnb32(emulate_gemm(out['dpre'], img('c1'), galt) + out['gs2'], ins['xhat1'], ins['rstd1'], vec['g1'], rpb, alter == 'pad_row')
    out['dout'] = emulate_gemm(out['gs1'], img('o'), galt)
    return out


# ---------------------------------------------------------------------------------------------- attention
ATTN_L = (1, 15, 16, 17, 31, 32, 33, 287, 288)
ATTN_BATCH = (1, 2, 3)
LMAX, HEADS, HD = 288, 8, 32
ATTN_SCALE = 1.0 / math.sqrt(32.0)  # (the kernels hold it in fp32: one more 2^-24 |s| in the score bound)
P_FLOOR = 2.0 ** -120              # probabilities below fp32's normal range (v_exp_f32 flushes): absolute


def heads_of(x, L, batch):
    """[batch*L][256] -> [batch][8][L][32] fp64."""
    return np.asarray(x, np.float64).reshape(batch, L, HEADS, HD).transpose(0, 2, 1, 3)


def rows_of(x):
    """[batch][8][L][32] -> [batch*L][256]."""
    b, h, L, e = x.shape
    return x.transpose(0, 2, 1, 3).reshape(b * L, h * e)


def attn_inputs(L, batch, flavour='normal'):
    """q, k, v, go [batch*L][256] fp32.  'large': scores of order +-80 (non-maximal probabilities underflow); 'zero_q'; 'one_hot': key
    (i * 7 + 3) mod L wins query i by more than 104 after scaling."""
    rng = np.random.default_rng(9000 + 17 * L + batch + 1000 * ('normal', 'large', 'zero_q', 'one_hot').index(flavour))
    q, k, v, go = (rng.standard_normal((batch * L, D)).astype(np.float32) for _ in range(4))
    if flavour == 'large':
        q *= np.float32(4.0)
        k *= np.float32(20.0)
    elif flavour == 'zero_q':
        q[...] = 0.0
    elif flavour == 'one_hot':
        # every head's 32 channels hold a one-hot code of the token index in two digits (16 + 16 channels): q_i . k_j = 2 A^2 [match], A^2 / sqrt(32) > 104
        q[...] = 0.0
        k[...] = 0.0
        A = np.float32(32.0)
        for b in range(batch):
            for i in range(L):
                j = (i * 7 + 3) % L
                for h in range(HEADS):
                    q[b * L + i, h * HD + j % 16] = A
                    q[b * L + i, h * HD + 16 + (j // 16) % 16] = A
                    k[b * L + i, h * HD + i % 16] = A
                    k[b * L + i, h * HD + 16 + (i // 16) % 16] = A
    return q, k, v, go


def one_hot_winner(L):
    """Key index that wins query i.  With L <= 256 the two-digit code is unique; L > 256 repeats codes (not used: the one-hot cases keep L <= 33)."""
    return [(i * 7 + 3) % L for i in range(L)]


def attn_forward64(q, k, v, L, batch, n_keys=None):
    """scores, P, out in fp64.  n_keys: the teeth test's wrong reference with L + 1 keys (the extra key is a copy of key 0, its value moved by 1)."""
    qh, kh, vh = heads_of(q, L, batch), heads_of(k, L, batch), heads_of(v, L, batch)
    if n_keys is not None and n_keys > L:
        kh, vh = np.concatenate([kh, kh[:, :, :1]], axis=2), np.concatenate([vh, vh[:, :, :1] + 1.0], axis=2)
    s = qh @ kh.transpose(0, 1, 3, 2) * ATTN_SCALE
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    P = e / e.sum(axis=-1, keepdims=True)
    return s, P, rows_of(P @ vh)


def attn_forward_bounds(q, k, v, L, batch, s64, P64, split, y_exp):
    """Elementwise bounds on P [batch][8][L][L] and out [batch*L][256] of a forward kernel.
    Scores: 32 products -- exact-fp32 kernel: an fmaf chain, (32 + 2) 2^-24 (|q||k|) scale (+ the multiplication by the scale); f16 hi+lo kernel:
    gemm_bound's terms with K = 32, both operands scaled per row (no absolute term beyond 2^-36 rscale_q rscale_k per product side).
    P = exp(s - max) / sum: an error ds in the scores moves every probability by at most 2 max|ds| relative (numerator and denominator); the
    argument s - max is rounded once and multiplied by log2(e) once before v_exp_f32, 2 |s - max| 2^-24 relative; the exponential itself
    MARGIN y_exp 2^-24 (y_exp: torch's fp32 exp against fp64 on the same arguments); the sum of L terms (5 + 6 additions per lane and wave
    tree), the reciprocal and the product: 16 2^-24.  Probabilities under fp32's normal range: P_FLOOR absolute.
    out = P V over 288 keys: (288 + 8) 2^-24 (|P||V|) for the exact-fp32 chain and its fold over eight waves, or the split terms
    C1 2^-22 (|P||V|) + 2^-36 (sum_j |v_j| + vmax / 8 sum_j P_ij) for the f16 kernel (P unscaled, V scaled by the wave's maximum) --
    plus |dP| |V|."""
    qa, ka, va = (np.abs(heads_of(t, L, batch)) for t in (q, k, v))
    S = qa @ ka.transpose(0, 1, 3, 2) * ATTN_SCALE
    if split:
        qmax, kmax = qa.max(axis=-1, keepdims=True), ka.max(axis=-1, keepdims=True)
        ds = (C1 * 2.0 ** -22 + (32 + C2) * U) * S + 4 * U * np.abs(s64) + \
            ABS_SPLIT * ATTN_SCALE * (qmax / 8.0 * ka.sum(axis=-1)[:, :, None, :] + qa.sum(axis=-1, keepdims=True) * (kmax / 8.0).transpose(0, 1, 3, 2))
    else:
        ds = (32 + 2) * U * S + 3 * U * np.abs(s64)
    arg = np.abs(s64 - s64.max(axis=-1, keepdims=True))
    rel = 2 * ds.max(axis=-1, keepdims=True) + (2 * arg + MARGIN * y_exp + 16) * U
    bP = P64 * rel * (1 + 2.0 ** -6) + P_FLOOR
    PV = P64 @ va
    if split:
        vmax = va.max(axis=(2, 3), keepdims=True)
        bo = (C1 * 2.0 ** -22 + (LMAX + C2) * U) * PV + ABS_SPLIT * (va.sum(axis=2, keepdims=True) + vmax / 4.0 * P64.sum(axis=-1, keepdims=True)) + 4 * U * np.abs(P64 @ heads_of(v, L, batch))
    else:
        bo = (LMAX + 8) * U * PV
    bo = bo + bP @ va
    return bP, rows_of(np.broadcast_to(bo, PV.shape))


def attn_backward64(q, k, v, o, P, go, L, batch):
    """dq, dk, dv in fp64 from the saved P and o (the kernel's formulation: D = rowsum(go o), dS = P (go V^T - D) scale) and their bounds for the
    exact-fp32 kernel: D: 8 2^-24 sum |go o|;  dP: 34 2^-24 (|go||v|^T);  dS: P scale (d dP + d D + 4 2^-24 (|dP| + |D|));
    dq = dS K, dk = dS^T Q, dv = P^T go: (288 + 8) 2^-24 of the absolute products (fmaf chains of 288 and the fold over eight waves) + the
    propagated |d dS|."""
    qh, kh, vh, oh, gh = (heads_of(t, L, batch) for t in (q, k, v, o, go))
    P = np.asarray(P, np.float64)
    Dr = (gh * oh).sum(axis=-1, keepdims=True)
    dP = gh @ vh.transpose(0, 1, 3, 2)
    dS = P * (dP - Dr) * ATTN_SCALE
    T = lambda a: a.transpose(0, 1, 3, 2)
    dq, dk, dv = dS @ kh, T(dS) @ qh, T(P) @ gh
    bD = 8 * U * np.abs(gh * oh).sum(axis=-1, keepdims=True)
    bdP = 34 * U * (np.abs(gh) @ T(np.abs(vh)))
    bdS = np.abs(P) * ATTN_SCALE * (bdP + bD + 4 * U * (np.abs(dP) + np.abs(Dr)))
    c = (LMAX + 8) * U
    bq = c * (np.abs(dS) @ np.abs(kh)) + bdS @ np.abs(kh)
    bk = c * (T(np.abs(dS)) @ np.abs(qh)) + T(bdS) @ np.abs(qh)
    bv = c * (T(np.abs(P)) @ np.abs(gh))
    return {'dq': Stage(rows_of(dq), rows_of(bq)), 'dk': Stage(rows_of(dk), rows_of(bk)), 'dv': Stage(rows_of(dv), rows_of(bv))}


# ---------------------------------------------------------------------------------------------- dpn_wgrad16
WGRAD_SHAPES = ((256, 256), (512, 256), (256, 512), (256, 96), (40, 256))      # (M, N): the ragged problem list of one launch
WGRAD_ROWS = (1, 31, 32, 33, 287)
WGRAD_SLICES = (1, 2, 3)
WGRAD_ABS = 2.0 ** -49             # 2^-36 of a scaled entry, the strip's maximum scaled into [2^13, 2^14)


def wgrad_inputs(rows, kind):
    """[(G [rows][M], X [rows][N], with_db)] for WGRAD_SHAPES.  Kind 'A': integers; 'M': normal values, the rows of one reduction 2^60 apart
    (G rows r = 1 mod 3 times 2^60, X rows r = 2 mod 5 times 2^-60); 'C': normal values."""
    rng = np.random.default_rng(7000 + rows + 100 * ('A', 'C', 'M').index(kind))
    out = []
    for i, (m, n) in enumerate(WGRAD_SHAPES):
        if kind == 'A':
            g, x = rng.integers(-4, 5, size=(rows, m)).astype(np.float32), rng.integers(-4, 5, size=(rows, n)).astype(np.float32)
        else:
            g, x = rng.standard_normal((rows, m)).astype(np.float32), rng.standard_normal((rows, n)).astype(np.float32)
        if kind == 'M':
            g[1::3] *= np.float32(2.0 ** 60)
            x[2::5] *= np.float32(2.0 ** -60)
        out.append((g, x, i % 2 == 0))
    return out


def _strip_max(a):
    """[cols]: the maximum magnitude of the 16-column strip a column belongs to (a wave's operand strip: one running scale)."""
    m = np.abs(np.asarray(a, np.float64)).max(axis=0)
    pad = np.zeros((len(m) + 15) // 16 * 16)
    pad[:len(m)] = m
    return np.repeat(pad.reshape(-1, 16).max(axis=1), 16)[:len(m)]


def wgrad_stage(G, X, slices):
    """dW = G^T X and db = column sums of G in fp64 with their conditions.  Integers (every sum below 2^24): equality.  Otherwise
        |d dW| <= (C1 2^-22 + (rows + C2 + slices) 2^-24) S + 2^-24 |dW| + 2^-49 (gmax[m] sum_r |X[r][n]| + xmax[n] sum_r |G[r][m]|),   S = |G|^T |X|:
    the split terms of gemm_bound(); every 32-row block of a 16-column operand strip is scaled by a power of two that puts the largest magnitude
    seen so far in that strip into [2^13, 2^14), so the absolute split error 2^-36 of a scaled entry is 2^-49 of the strip's maximum gmax /
    xmax -- this is what rows 2^60 below the strip's maximum cost: they vanish, and the bound says by how much; raising the scale
    rescales the accumulators by a power of two (exact); the slices are added in fp32 (one rounding each).
        |d db| <= (rows + 4 + slices) 2^-24 sum_r |G[r][m]|."""
    G64, X64 = np.asarray(G, np.float64), np.asarray(X, np.float64)
    rows = G64.shape[0]
    y, S = G64.T @ X64, np.abs(G64).T @ np.abs(X64)
    db, Sb = G64.sum(axis=0), np.abs(G64).sum(axis=0)
    ints = bool(np.all(G64 == np.rint(G64)) and np.all(X64 == np.rint(X64)) and S.max(initial=0) < 2.0 ** 24 and np.abs(G64).max(initial=0) <= 2048
                and np.abs(X64).max(initial=0) <= 2048)
    if ints:
        return Stage(y, exact=y.astype(np.float32)), Stage(db, exact=db.astype(np.float32))
    bound = (C1 * 2.0 ** -22 + (rows + C2 + slices) * U) * S + U * np.abs(y) + \
        WGRAD_ABS * (_strip_max(G64)[:, None] * np.abs(X64).sum(axis=0)[None, :] + _strip_max(X64)[None, :] * Sb[:, None])
    return Stage(y, bound), Stage(db, (rows + 4 + slices) * U * Sb)


def emulate_wgrad(G, X, slices, alter=None):
    """dpn_wgrad16's arithmetic in numpy: row slices of ceil(ceil(rows / slices) / 32) * 32 rows, 32-row blocks, one running power-of-two scale
    per 16-column strip of each operand, the f16 hi+lo split, two fp32 accumulators rescaled when a scale rises, the slices added in order."""
    G, X = np.ascontiguousarray(G, np.float32), np.ascontiguousarray(X, np.float32)
    rows, M = G.shape
    N = X.shape[1]
    rps = ((rows + slices - 1) // slices + 31) // 32 * 32
    total = np.zeros((M, N), np.float32)

    def expo(a):                                 # biased exponent of the strip maxima, floor 13
        m = _strip_max(a).astype(np.float32) if a.shape[0] else np.zeros(a.shape[1], np.float32)
        return np.maximum(((m.view(np.uint32) >> np.uint32(23)) & np.uint32(0xff)).astype(np.int64), 13)
    for sl in range(slices):
        am, ac = np.zeros((M, N), np.float64), np.zeros((M, N), np.float64)
        eg, ex = np.full(M, 13), np.full(N, 13)
        for r0 in range(sl * rps, min(rows, (sl + 1) * rps), 32):
            g, x = G[r0:min(r0 + 32, rows, (sl + 1) * rps)], X[r0:min(r0 + 32, rows, (sl + 1) * rps)]
            ng, nx = np.maximum(eg, expo(g)), np.maximum(ex, expo(x))
            f = np.ldexp(1.0, np.maximum(eg - ng, -200))[:, None] * np.ldexp(1.0, np.maximum(ex - nx, -200))[None, :]
            am, ac, eg, ex = (am * f).astype(np.float32).astype(np.float64), (ac * f).astype(np.float32).astype(np.float64), ng, nx
            gh, gl = (p.astype(np.float64) for p in _f16_planes(np.ldexp(g, 140 - eg).astype(np.float32)))
            xh, xl = (p.astype(np.float64) for p in _f16_planes(np.ldexp(x, 140 - ex).astype(np.float32)))
            am = (am + gh.T @ xh).astype(np.float32).astype(np.float64)
            if alter != 'no_hi_lo':
                ac = (ac + gh.T @ xl).astype(np.float32).astype(np.float64)
            ac = (ac + gl.T @ xh).astype(np.float32).astype(np.float64)
        part = (ac / 2048.0 + am).astype(np.float32).astype(np.float64) * np.ldexp(1.0, np.maximum(eg[:, None] + ex[None, :] - 280, -250))
        total = part.astype(np.float32) if sl == 0 else (total + part.astype(np.float32)).astype(np.float32)
    return total


# ---------------------------------------------------------------------------------------------- dpn_enc_prep
PREP_T, PREP_C, PREP_BATCH = (1, 2, 3, 159), (1, 5), (1, 3)


def im2col_circ3_model(x, T, C, batch):
    """out[b T + t][3 c + tap] = x[b T + (t + tap - 1) mod T][c], an integer index model (T = 1 and T = 2 wrap onto the same rows)."""
    x = np.asarray(x).reshape(batch, T, C)
    out = np.empty((batch, T, C, 3), x.dtype)
    for tap in range(3):
        out[:, :, :, tap] = x[:, (np.arange(T) + tap - 1) % T, :]
    return out.reshape(batch * T, 3 * C)


def lead_pe_stage(h, freqs):
    """[batch][2 n]: sin / cos in fp64 of the fp32 product h f; bound MARGIN Y 2^-24 absolute, Y = torch's fp32 sin / cos on the same products
    against fp64 in units of 2^-24 (the functions are O(1))."""
    import torch
    s = (np.asarray(h, np.float32)[:, None] * np.asarray(freqs, np.float32)[None, :]).astype(np.float32)
    ref = np.stack([np.sin(s.astype(np.float64)), np.cos(s.astype(np.float64))], axis=-1).reshape(len(h), -1)
    Y = max(yardstick(lambda a: torch.sin(torch.from_numpy(a)).numpy(), np.sin, s, np.ones_like),
            yardstick(lambda a: torch.cos(torch.from_numpy(a)).numpy(), np.cos, s, np.ones_like))
    return Stage(ref, np.full(ref.shape, MARGIN * Y * U)), Y
