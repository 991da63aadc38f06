"""Case table, fp64 reference, K-layout decoders and pass conditions for the weight side of the point path: dpn_bwd_points* (stage 1) ->
dpn_wgrad -> dpn_wgrad_finish (csrc/dpn_tiles_kernels.inc, dpn_ring_kernels.inc, dpn_wgrad.hip).  Imports without a GPU:
tests/test_wgrad_cases_cpu.py runs the table through a torch model of the kernels' arithmetic (emulate(), built on oracle/kernel_model.mm) and
seeds mistakes into it; tests/test_gpu_wgrad_fp64.py runs it through the C ABI (tools/wgrad_digest.run_case).

The method is the encoder launches' (tests/encoder_cases.py): every stage is compared with an fp64 evaluation that starts from the kernels' OWN
upstream tensors, so no error compounds and every bound is a one-stage bound.  What can be read back between the launches:
  saved state   the two ReLU masks (point_path.decode_masks) and T1 = m1 (.) y, hi [+ lo] planes in the K-layout (kmat_decode);
  operands      Z1 = m1 (.) (w1 Z0 + g b1) in the same layout, gnet = scale g_out, gJ = scale g_jxi (table form of Z0);
  partials      what dpn_wgrad hands to the finish: per point range S1 = M2^T Z1, S2 = M2^T G6, dw1 = T1^T Z0 and the vectors mv = M2^T g,
                db1 = T1^T g, q1 = colsum Z1, q6 = colsum G6, sg = sum g (decode_partials adds the ranges in fp64);
  outputs       the eleven gradients per net.
Given the masks every one of these is LINEAR in the cotangents, and because the masks are the kernels' own there are no kink flips to remove
(that the masks are the true ones is a separate statement: masks_reference()).  Stages and their references:
  'stage1'  Z1 against m1 (.) (Z0 w1^T + g b1), Z0 from fp64 sin / cos of the fp32 angles                                  stage1_reference
  'saved'   T1 against m1 (.) y, y = phase_a's formulas under the forced masks                                                 t1_reference
  'wgrad'   the eight sums against the same products of the DECODED T1, Z1 (M2 is 0 / 1: S1 has no operand error at all)       wgrad_reference
  'finish'  the 11 gradients against finish() of the kernels' own sums                                                          finish_bounds
  'chain'   the 11 gradients against reference() = kernel_model.phase_b fed the kernels' m1, m2, T1, Z1                         (the same, E of wgrad)
Every bound is element-wise: an error term is a named constant times the SAME expression evaluated on absolute values (companion() returns
those evaluations for the eight sums and, through finish() on absolute values, for the gradients; V carries them through the finish stage
operand by operand, which is never looser).  Nothing is normalised by a tensor's maximum and nothing is taken from a kernel's output.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import kernel_model as KM
from encoder_cases import MARGIN, U        # MARGIN = 4 on a measured yardstick, U = 2^-24 the fp32 unit roundoff

F64 = torch.float64
NAMES = ('w1b1', 'w2b2', 'e', 'Wd', 'bd', 'W1', 'bf1', 'W2', 'bf2', 'wo', 'bo')
SUMS = ('S1', 'S2', 'dw1', 'mv', 'db1', 'sg', 'q1', 'q6')

# ---------------------------------------------------------------------------------------------- named constants of the pass conditions
UB = 2.0 ** -8        # bf16 unit roundoff: 8 significant bits (7 stored), round to nearest even (v_cvt_pk_bf16_f32): |x - bf16(x)| <= 2^-8 |x|
C_HL = 4              # x 2^-16 |X||Y|, hi+lo operands: with hi = bf16(x), lo = bf16(x - hi), |x - hi - lo| <= UB^2 |x| = 2^-16 |x| per operand (2 of 4),
#                       the lo.lo product the kernels drop is at most UB |x| UB |y| = 2^-16 |x||y| (1), every product of two such terms (1)
C_B = 2 + 2.0 ** -6   # x 2^-8 |X||Y|, plain bf16 operands: UB per operand (2) and their product 2^-16 = 2^-8 of the unit, rounded up to 2^-6
SPLIT = {'bf16x2': UB * UB, 'bf16': UB}            # writing an fp32 value as planes: what the planes' sum misses of it
LOLO = {'bf16x2': UB * UB * (1 + 2.0 ** -6), 'bf16': 0.0}     # the dropped lo.lo of two operands that are GIVEN as planes (|lo| <= UB |x|, |hi| <= (1 + UB) |x|)
ACC_U = 2.0 ** -23    # one step of an fp32 accumulator whose rounding mode is not documented (the matrix core's adder): a truncating one loses 2 U
MFMA_TERMS = 16       # the 16 products of one v_mfma_f32_32x32x16_bf16 are added inside the instruction: at most one accumulator step each
MAX_SPLITS = 20       # kMaxSplits of dpn_wgrad.hip: point ranges per product, added by dpn_finish_rows_kernel in fp32, one step each
FORM_OPS = 4          # Z0 = fmaf(g, own, +-(gJ fr) partner): the product gJ fr, the product with the partner, the fmaf, one of slack
GH_OPS = 2            # Z0 with the second derivatives' cotangent (z0_frag_derivs): gs = fmaf(-(gH fr), fr, g) in place of g -- the product gH fr and the fmaf
FIN_SLACK = 8         # finish stage, beside the K terms of a reduction: the fold of four waves' partial tiles (3), the rank-one term's two
#                       products and its addition (3), two of slack
SC_FAST = 2.0 ** -14  # plain bf16 mode: hardware v_sin / v_cos behind __sinf / __cosf.  Not derivable here and no CPU model exists; the features are
#                       rounded to bf16 right away (UB = 2^-8 of a unit feature), this is 2^-6 of that step
SECOND = 1 + 2.0 ** -10   # products of two error terms, wherever a first-order propagation is used


def acc_steps(k_steps):
    """Accumulator steps of a bf16 MFMA reduction over k_steps 16-wide k-steps: three instructions per k-step (hi.hi, hi.lo, lo.hi; fewer in the plain
    mode and for the 0 / 1 mask), the additions inside one instruction, the accumulator's initial value and one of slack.  Worst case: each step
    loses ACC_U of the absolute-value sum, whatever the order -- which is why the summation order of the range plan needs no measured term."""
    return 3 * k_steps + MFMA_TERMS + 2


def vec_steps(n_pad):
    """fp32 steps of a vector sum over the points (mv, db1, q1, q6, sg): at most two per point (the hi and the lo plane), the half-wave fold, slack."""
    return 2 * n_pad + 4


# ---------------------------------------------------------------------------------------------- layout algebra (csrc/dpn_layout.h, checked against it on the CPU)
def drow32(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def chain_ch(ks, h, e):
    return 16 * ks + 8 * (e >> 2) + 4 * h + (e & 3)


def pe3_ch(ks, h, e):
    a = 8 * ks + 4 * h + (e >> 1)
    return (a & 31) * 6 + (e & 1) * 3 + (a >> 5)


def pe6_ch(ks, h, e):
    a = 8 * ks + 4 * h + (e >> 1)
    return (a & 15) * 12 + (e & 1) * 6 + (a >> 4)


def _of_slot(fn, n):
    """channel of slot s = 16 ks + 8 h + e (column 32 ct + jj of a K-layout matrix IS slot s: ks = 2 ct + (jj >> 4), h = (jj >> 3) & 1, e = jj & 7)"""
    return torch.tensor([fn(s >> 4, (s >> 3) & 1, s & 7) for s in range(n)])


CH_OF_SLOT, PE3_OF_SLOT, PE6_OF_SLOT = _of_slot(chain_ch, 256), _of_slot(pe3_ch, 192), _of_slot(pe6_ch, 192)
SLOT_OF_CH, SLOT_OF_PE3, SLOT_OF_PE6 = (torch.argsort(p) for p in (CH_OF_SLOT, PE3_OF_SLOT, PE6_OF_SLOT))

# dpn_wgrad.hip: kPartFloats per (point range, net) = S1 | S2 | dw1 | seven 256-vectors (slots 2 .. 6 used: mv1, db1, [sum g], q1, q6)
PART_FLOATS = 65536 + 49152 * 2 + 7 * 256
PART_VEC = 163840


def pad_points(n):
    return (n + 127) // 128 * 128


def kmat_decode(buf, offset, nets, planes, n_pad, ct):
    """A K-layout matrix (dpn_point_common.h KMat: [net][plane][tile32][kk 2][ct][lane 64][8 bf16]) from a uint8 buffer, as fp64
    [nets, planes, n_pad, 32 ct] with the columns in SLOT order.  Lane (jj = lane & 31, h = lane >> 5) holds column 32 ct + jj; its element e of
    k-step kk is point drow32(8 kk + e, h) = 16 kk + 8 (e >> 2) + 4 h + (e & 3) of the tile."""
    tiles = n_pad // 32
    nbytes = nets * planes * tiles * ct * 2048
    a = buf[offset:offset + nbytes].view(torch.int16).view(nets, planes, tiles, 2, ct, 2, 32, 2, 4)       # kk, ct, h, jj, e >> 2, e & 3
    f = (a.to(torch.int32) << 16).view(torch.float32)
    return f.permute(0, 1, 2, 3, 7, 5, 8, 4, 6).reshape(nets, planes, n_pad, 32 * ct).double()            # point bits: kk, e >> 2, h, e & 3


def kmat_encode(x, ct):
    """The inverse, for one plane of exactly representable values: x [n_pad, 32 ct] (slot order) -> uint8 bytes."""
    n_pad = x.shape[0]
    a = x.float().reshape(n_pad // 32, 2, 2, 2, 4, ct, 32).permute(0, 1, 5, 3, 6, 2, 4).contiguous()       # tile, kk, ct, h, jj, e >> 2, e & 3
    return (a.view(torch.int32) >> 16).to(torch.int16).reshape(-1).view(torch.uint8)


def decode_saved(saved, n, prec):
    """(T1 [6, n, 256] fp64 = hi + lo in natural channel order, m1, m2 bool [6, n, 256]) from the saved state of dpn_fwd_ref (what it holds for
    the padding points is never multiplied by anything but their zero cotangents and is not looked at)."""
    from deepphysinet_amd.point_path import decode_masks
    ns, n_pad = (2 if prec == 'bf16x2' else 1), pad_points(n)
    t1 = kmat_decode(saved, 0, 6, ns, n_pad, 8).sum(1)[:, :, SLOT_OF_CH]
    m1, m2 = decode_masks(saved, n, ns)
    return t1[:, :n], m1, m2


def decode_operands(operands, n, prec, table):
    """Z1 [6, n, 256] fp64 (hi + lo, natural order; the padding rows are asserted to be exactly zero), gnet [6, n_pad] and, in the table form
    of Z0, gJ [6, 3, n_pad] (fp32 as written, padding included)."""
    ns, n_pad = (2 if prec == 'bf16x2' else 1), pad_points(n)
    z1 = kmat_decode(operands, 0, 6, ns, n_pad, 8)
    assert not bool(z1[:, :, n:].any()), 'Z1 of a padding point is not zero'
    m256, m192, t192 = 6 * ns * n_pad * 512, 6 * ns * n_pad * 384, ns * n_pad * 384
    g0 = m256 + m192 + t192
    gnet = operands[g0:g0 + 6 * n_pad * 4].view(torch.float32).view(6, n_pad)
    gj = operands[m256 + t192:m256 + t192 + 18 * n_pad * 4].view(torch.float32).view(6, 3, n_pad) if table else None
    return z1.sum(1)[:, :n][:, :, SLOT_OF_CH], gnet, gj


def decode_partials(partials, k_splits):
    """The eight sums per net in natural order, the point ranges added in fp64, and the same sums of absolute values (what the finish stage's
    own fp32 addition of the ranges is bounded by).  k_splits: DpnSizes.k_splits, the ranges in front of the finish stage's scratch.  The buffer was
    zeroed before the launch: a range no product wrote adds nothing."""
    p = partials.view(torch.float32)[:k_splits * 6 * PART_FLOATS].view(k_splits, 6, PART_FLOATS).double()
    out = []
    for q in (p.sum(0), p.abs().sum(0)):
        vec = q[:, PART_VEC:].view(6, 7, 256)
        out.append({'S1': q[:, :65536].view(6, 256, 256)[:, SLOT_OF_CH][:, :, SLOT_OF_CH],
                    'S2': q[:, 65536:114688].view(6, 256, 192)[:, SLOT_OF_CH][:, :, SLOT_OF_PE6],
                    'dw1': q[:, 114688:PART_VEC].view(6, 256, 192)[:, SLOT_OF_CH][:, :, SLOT_OF_PE3],
                    'mv': vec[:, 2][:, SLOT_OF_CH], 'db1': vec[:, 3][:, SLOT_OF_CH], 'sg': vec[:, 4, 0],
                    'q1': vec[:, 5][:, SLOT_OF_CH], 'q6': vec[:, 6, :192][:, SLOT_OF_PE6]})
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------- the device's sin / cos (hi+lo mode) on the CPU
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def sincos_device(th):
    """csrc/dpn_sincos.h sincos_precise in numpy (fmaf through fp64: the product of two fp32 numbers is exact there).  A yardstick for the size of
    the device's error, not a bit-exact model (tests/test_sincos_bits_cpu.py holds the bits)."""
    th = np.asarray(th, np.float32)
    f = np.float32
    k = np.rint(th * f(0.63661977236758134)).astype(np.float32)
    r = _fma(k, f(-1.5707963705062866), th)
    r = _fma(k, f(4.371138828673793e-08), r)
    r2 = (r * r).astype(np.float32)
    sp = _fma(r2, f(2.7183114939898219064e-6), f(-1.9839334836096632576e-4))
    sp = _fma(sp, r2, f(8.3333293858894631756e-3))
    sp = _fma(sp, r2, f(-1.6666666641626524100e-1))
    sp = _fma((sp * r2).astype(np.float32), r, r)
    cp = _fma(r2, f(2.4433157826443582e-5), f(-1.3887316255057415e-3))
    cp = _fma(cp, r2, f(4.1666645683529456e-2))
    cp = _fma(cp, r2, f(-0.5))
    cp = _fma(cp, r2, f(1.0))
    q = k.astype(np.int64) & 3
    odd = (q & 1) != 0
    s, c = np.where(odd, cp, sp), np.where(odd, sp, cp)
    s = np.where((q & 2) != 0, -s, s)
    c = np.where((q == 1) | (q == 2), -c, c)
    return s.astype(np.float32), c.astype(np.float32)


def sincos_error(angles):
    """MEASURED term (MARGIN): the largest absolute error of the device's formulas against fp64 on the fp32 angles of the case."""
    worst = 0.0
    for a in angles:
        a = a.numpy().astype(np.float32)
        s, c = sincos_device(a)
        a64 = a.astype(np.float64)
        worst = max(worst, float(np.abs(s - np.sin(a64)).max()), float(np.abs(c - np.cos(a64)).max()))
    return MARGIN * worst


# ---------------------------------------------------------------------------------------------- inputs
GEOMETRY = (27000.0, 27000.0, 256.0, 144.0, 86400.0)      # dx, dy, lon - 1, lat - 1, pred_t_span of the NCEP configuration (PointConfig.geometry())


def freqs():
    from deepphysinet_amd.point_path import _freqs
    return _freqs('cpu')


class Features:
    """The coordinate and data features of n points: fp64 sin / cos of the fp32 angles the kernels form (two fp32 divisions, the fp32 product with
    point_path._freqs), in the reference's channel order (pe [n, 192]: f 6 + fn 3 + c; dpe [n, 32, 2, 3]; pe6 [n, 192]: f 12 + fn 6 + c6).
    pe_in [n, 192]: caller-encoded coordinates in place of x, y, t (no tangent).  fr [192]: the frequency of each pe channel.
    d2pe = -fr^2 pe and d3pe = -fr^2 dpe, in dpe's layout: the second and third derivatives along xi_c (tests/value_cases.py)."""

    def __init__(self, x, y, t, coord_data, geometry=GEOMETRY, pe_in=None, prec='bf16x2'):
        fr = freqs()
        n = coord_data.shape[0]
        dx, dy, lon_m1, lat_m1, span = geometry
        self.n, self.prec, self.raw = n, prec, pe_in is None
        ang6 = (coord_data.float()[:, None, :] * fr[32:, None][None]).float()                       # [n, 16, 6]
        angles = [ang6]
        self.ang6 = ang6
        self.pe6 = torch.stack([torch.sin(ang6.double()), torch.cos(ang6.double())], 2).reshape(n, -1)
        self.fr = fr[:32].double()[:, None, None].expand(32, 2, 3).reshape(-1)
        if pe_in is None:
            xi = torch.stack([x.float().reshape(-1) / dx / lon_m1, y.float().reshape(-1) / dy / lat_m1, t.float().reshape(-1) / span / 1.0], 1)
            ang = (xi[:, None, :] * fr[:32, None][None]).float()                                    # [n, 32, 3]
            angles.append(ang)
            self.ang = ang
            s, c = torch.sin(ang.double()), torch.cos(ang.double())
            f = fr[:32].double()[None, :, None]
            self.pe = torch.stack([s, c], 2).reshape(n, -1)
            self.dpe = torch.stack([c * f, -s * f], 2)
            self.d2pe, self.d3pe = torch.stack([-s * f * f, -c * f * f], 2), -self.dpe * f[:, :, None] * f[:, :, None]
        else:
            self.ang = None
            self.pe, self.dpe = pe_in.double(), torch.zeros(n, 32, 2, 3, dtype=F64)
            self.d2pe, self.d3pe = torch.zeros_like(self.dpe), torch.zeros_like(self.dpe)
        # absolute error of a feature as the kernels hold it in fp32 (before any split): measured for the hi+lo mode's formulas, SC_FAST in the plain mode
        self.sc = sincos_error(angles) if prec == 'bf16x2' else SC_FAST
        self.sc3 = self.sc if pe_in is None else 0.0

    def z0(self, g, gj, gh=None):
        """Z0 = g pe + sum_c gJ_c d pe / d xi_c [+ sum_c gH_c d2 pe / d xi_c^2] [n, 192] and its absolute-value companion; g [n], gj, gh [n, 3] fp64."""
        n = self.n
        z = g[:, None] * self.pe + (self.dpe * gj[:, None, None, :]).reshape(n, -1)
        za = g.abs()[:, None] * self.pe.abs() + (self.dpe.abs() * gj.abs()[:, None, None, :]).reshape(n, -1)
        if gh is not None:
            z = z + (self.d2pe * gh[:, None, None, :]).reshape(n, -1)
            za = za + (self.d2pe.abs() * gh.abs()[:, None, None, :]).reshape(n, -1)
        return z, za

    def z0_error(self, g, gj, za, gh=None):
        """|Z0 as the kernels form it in fp32 - Z0|: the features' error through g, gJ fr [and gH fr^2], and FORM_OPS [+ GH_OPS] roundings (one for
        caller-encoded features)."""
        n = self.n
        fr = self.fr.reshape(32, 2, 3)[None]
        gjf = (gj.abs()[:, None, None, :] * fr).reshape(n, -1)
        if gh is None:
            return self.sc3 * (g.abs()[:, None] + gjf) + (FORM_OPS if self.raw else 1) * U * za
        ghf = (gh.abs()[:, None, None, :] * fr * fr).reshape(n, -1)
        return self.sc3 * (g.abs()[:, None] + gjf + ghf) + (FORM_OPS + GH_OPS) * U * za


def weights_of(heads, evec, statics):
    """The six nets' W (fp64) from the very fp32 tensors handed to dpn_pack_weights_form: w1b1 = heads[:, 193 k : 193 k + 193], w2b2 =
    heads[:, 1158 + 257 k : ..], the eight statics per net in point_path.STATIC_SHAPES order (Wd bd W1 bf1 W2 bf2 wo bo).  No encoder."""
    out = []
    for k in range(6):
        st = [s.detach().cpu().double() for s in statics[8 * k:8 * k + 8]]
        out.append(dict(w1b1=heads[:, 193 * k:193 * k + 193].detach().cpu().double(), w2b2=heads[:, 1158 + 257 * k:1158 + 257 * k + 257].detach().cpu().double(),
                        e=evec[k].detach().cpu().double(), Wd=st[0], bd=st[1], W1=st[2], bf1=st[3], W2=st[4], bf2=st[5], wo=st[6].reshape(-1), bo=st[7].reshape(())))
    return out


_oracle_w = {}


def oracle_weights(gain):
    """The same fp32 tensors without a GPU: the oracle's state (fill_state_dict_ at `gain`) through its fp32 hyper-network, as fp64 W."""
    from oracle import dpn_oracle as O
    from oracle.fill import synthetic_inputs
    if gain not in _oracle_w:
        with torch.no_grad():
            st = O.make_state(gain=gain)
            inp = synthetic_inputs(1, tag='inter')
            meta = O.meta_net_forward(st, inp['field_data'], inp['forecast_h'])
            ws = []
            for net in O.NETS:
                w = KM.net_weights(st, net, meta, inp['forecast_h'])
                ws.append({k: (v.reshape(-1) if k == 'wo' else v).detach().float().double() for k, v in w.items()})
        _oracle_w[gain] = ws
    return _oracle_w[gain]


# ---------------------------------------------------------------------------------------------- case table
Case = namedtuple('Case', 'route n prec gain kind scale')
SIZES = (1,        # one real point among 127 padding points: every sum is one term, every padding row must stay out
         70,       # ragged tails: two full 32-point tiles and six points of a third, one 64-point workgroup and a part of the next
         129,      # the first point past a padding boundary (n_pad 256): one real point in the second 128-point block
         1037,     # the small range plan (n_pad 1152, 36 tiles): the ranges of a product are not equally long
         5197)     # the full 42-range plan of the training step's interior points
KINDS = ('dense',          # standard normal g_out and g_jxi
         'gout',           # g_jxi = 0
         'gjxi',           # g_out = 0: dw1 is reached through the gJ rows of the Z0 table alone, every g-weighted sum must vanish
         'onehot_first',   # one nonzero (point, net) pair at point 0 ..
         'onehot_last',    # .. and at point n - 1: the other five nets' gradients are exactly zero, the hit net's is rank one
         'pow2')           # dense, each net's cotangents times its own power of two
HOT_NET = 3
POW2_EXPONENTS = (-12, -7, -2, 3, 8, 12)
SCALES = (1.0, 0.75, 2.0 ** -10)


def all_cases():
    out = []
    for n in SIZES:                                                     # the product route: tile kernels, table-form Z0
        out += [Case('raw', n, 'bf16x2', 1.0, kind, 0.75) for kind in KINDS]
        out += [Case('raw', n, 'bf16x2', 1.0, 'dense', s) for s in SCALES if s != 0.75]
    for n in (70, 1037):
        out += [Case('raw', n, 'bf16x2', 5.0, kind, 0.75) for kind in KINDS]
        out.append(Case('raw', n, 'bf16', 1.0, 'dense', 0.75))          # ring kernels, stored Z0, one plane
    out += [Case('pe_in', 70, prec, 1.0, 'dense', 1.0) for prec in ('bf16x2', 'bf16')]      # ring kernels, stored Z0, g_out only (dpn_bwd_points: no scale)
    return out


def case_id(c):
    return '%s-%d-%s-g%g-%s-s%g' % c


def cotangents(c):
    """(g_out [n, 6], g_jxi [n, 6, 3] or None) fp32 on the host, from torch's CPU generator (seeds 1 and 2: run_case's own dense streams)."""
    n = c.n
    g_out = torch.randn(n, 6, generator=torch.Generator().manual_seed(1))
    g_jxi = torch.randn(n, 6, 3, generator=torch.Generator().manual_seed(2))
    if c.kind == 'gout':
        g_jxi.zero_()
    elif c.kind == 'gjxi':
        g_out.zero_()
    elif c.kind.startswith('onehot'):
        p = 0 if c.kind == 'onehot_first' else n - 1
        go, gj = g_out[p, HOT_NET].clone(), g_jxi[p, HOT_NET].clone()
        g_out.zero_(), g_jxi.zero_()
        g_out[p, HOT_NET], g_jxi[p, HOT_NET] = go, gj
    elif c.kind == 'pow2':
        f = torch.tensor([2.0 ** e for e in POW2_EXPONENTS])
        g_out, g_jxi = g_out * f[None, :], g_jxi * f[None, :, None]
    return g_out, (g_jxi if c.route == 'raw' else None)


def pe_in_of(n):
    """run_case's caller-encoded features."""
    return torch.sin(torch.randn(n, 192, generator=torch.Generator().manual_seed(4)) * 3.0)


def scaled(c, g_out, g_jxi, g_hxi=None):
    """What stage 1 multiplies: g = scale g_out, gJ = scale g_jxi, ONE fp32 product each (gnet must equal it bit for bit), as fp64 [6, n], [6, n, 3];
    with g_hxi also gH = scale g_hxi (a third value)."""
    s = torch.tensor(c.scale, dtype=torch.float32)
    g = (s * g_out.float()).double().t().contiguous()
    gj = torch.zeros(6, c.n, 3, dtype=F64) if g_jxi is None else (s * g_jxi.float()).double().permute(1, 0, 2).contiguous()
    if g_hxi is not None:
        return g, gj, (s * g_hxi.float()).double().permute(1, 0, 2).contiguous()
    return g, gj


def fused_route(c):
    return c.route == 'raw' and c.prec == 'bf16x2'       # dpn_fwd_form: the tile kernels' five-GEMM form; the ring kernels keep the seven


# ---------------------------------------------------------------------------------------------- references
def _phase_a(W, F, prec, fused, masks=None, dtype=F64):
    z = torch.zeros(F.n, dtype=dtype)
    Wd = {k: v.to(dtype) for k, v in W.items()}
    return KM.phase_a(Wd, F.pe.to(dtype), F.dpe.to(dtype), F.pe6.to(dtype), z, prec, fused=fused, masks=masks)[2]


def masks_reference(Ws, F, fused, dtype=F64):
    """(m1, m2) bool [6, n, 256] of phase_a evaluated in `dtype` on the fp32 weights and the fp64 features: the TRUE masks (fp64) or the fp32 model's."""
    S = [_phase_a(W, F, 'fp64' if dtype == F64 else 'fp32', fused, dtype=dtype) for W in Ws]
    return torch.stack([s['m1'] > 0 for s in S]), torch.stack([s['m2'] > 0 for s in S])


def flipped_points(ma, mb):
    return ((ma[0] != mb[0]) | (ma[1] != mb[1])).any(2).any(0)


def reference(W, masks, pe, dpe, pe6, g_out, g_jxi, scale, t1=None, z1=None, g_hxi=None, d2pe=None):
    """The eleven gradients of ONE net (kernel_model.phase_b's dict, fp64) under the forced masks (m1, m2) [n, 256].  g_out [n], g_jxi [n, 3]: this
    net's cotangents (fp32 values), scale: stage 1's scalar (the product is the kernels' single fp32 one).  t1 = m1 (.) y with y from phase_a's fused
    formulas under the masks, Z1 = m1 (.) (Z0 w1^T + g b1) -- or the given t1 / z1 [n, 256] (the tensors a kernel saved: the reference then
    starts from them).  g_hxi [n, 3] with d2pe (Features.d2pe): the second derivatives' cotangent, Z0 += sum_c gH_c d2 pe / d xi_c^2 -- behind a given Z1
    it reaches d w1 = T1^T Z0 alone."""
    m1, m2 = masks[0].double(), masks[1].double()
    g, gj = (torch.tensor(scale, dtype=g_out.dtype) * g_out).double(), (torch.tensor(scale, dtype=g_jxi.dtype) * g_jxi).double()     # fp32 cotangents: ONE fp32 product
    z = torch.zeros(pe.shape[0], dtype=F64)
    S = KM.phase_a(W, pe, dpe, pe6, z, 'fp64', fused=True, masks=(m1, m2))[2]
    if t1 is not None:
        S = dict(S, t1=t1)
    if g_hxi is None:
        return KM.phase_b(W, S, pe, dpe, pe6, g, gj, 'fp64', z1=z1)
    zh = (d2pe * (torch.tensor(scale, dtype=g_hxi.dtype) * g_hxi).double()[:, None, None, :]).reshape(pe.shape[0], -1)
    if z1 is None:
        z0 = g[:, None] * pe + (dpe * gj[:, None, None, :]).reshape(pe.shape[0], -1) + zh
        z1 = S['m1'] * (z0 @ W['w1b1'][:, :192].T + g[:, None] * W['w1b1'][:, 192])
    gr = KM.phase_b(W, S, pe, dpe, pe6, g, gj, 'fp64', z1=z1)
    gr['w1b1'] = torch.cat([gr['w1b1'][:, :192] + S['t1'].T @ zh, gr['w1b1'][:, 192:]], 1)
    return gr


def stage1_reference(c, W, F, m1, g, gj, gh=None):
    """(Z1, bound): Z1 = m1 (.) (Z0 w1^T + g b1) of one net and
        m1 (.) [ (HL + acc_steps(12) ACC_U) (|Z0||w1|^T + |g||b1|) + SECOND E_Z0 |w1|^T + SPLIT |pre| ]
    -- the three-product (or plain) GEMM over 12 k-steps, the features' and the forming's error E_Z0 through |w1|, and the planes Z1 is written as."""
    w1, b1 = W['w1b1'][:, :192], W['w1b1'][:, 192]
    z0, z0a = F.z0(g, gj, gh)
    pre = z0 @ w1.T + g[:, None] * b1
    prea = z0a @ w1.abs().T + g.abs()[:, None] * b1.abs()
    hl = C_HL * 2.0 ** -16 if c.prec == 'bf16x2' else C_B * 2.0 ** -8
    bound = (hl + acc_steps(12) * ACC_U) * prea + SECOND * (F.z0_error(g, gj, z0a, gh) @ w1.abs().T) + SPLIT[c.prec] * pre.abs()
    return m1 * pre, m1 * bound


class V:
    """A value and an element-wise bound on what an fp32 evaluation of the same expression may differ from it by.  Every operation adds the fp32
    roundings of its own result (k steps of U on the absolute-value evaluation) to the operands' bounds carried through absolute values."""

    def __init__(self, v, e=None):
        self.v, self.e = v, (torch.zeros_like(v) if e is None else e)


def v_mm(A, B, k):
    a, b = A.v.abs(), B.v.abs()
    return V(A.v @ B.v, A.e @ (b + B.e) + a @ B.e + (k + FIN_SLACK) * U * (a @ b))


def v_mul(A, B, k=1):
    a, b = A.v.abs(), B.v.abs()
    return V(A.v * B.v, A.e * (b + B.e) + a * B.e + k * U * (a * b))


def v_add(*ts):
    v = sum(t.v for t in ts)
    return V(v, sum(t.e for t in ts) + (len(ts) - 1) * U * sum(t.v.abs() for t in ts))


def t1_reference(c, W, F, m1, m2, fused=None):
    """(T1, bound) of one net under the forced masks (fused: the packed form, default the one of the case's route): T1 = m1 (.) y,
        fused (tile kernels):  y = (m2 (.) u) A + 2 a2,   A = W1 w2, a2 = w2^T wo, u = W2^T wo formed in fp32 by the pack kernel (256 terms each)
        ring kernels:          v = (m2 (.) u) W1 + 2 wo,  y = v w2
    each GEMM with HL of its absolute-value evaluation and acc_steps(16) accumulator steps, y written as planes."""
    w2 = W['w2b2'][:, :256]
    hl = C_HL * 2.0 ** -16 if c.prec == 'bf16x2' else C_B * 2.0 ** -8
    acc = acc_steps(16) * ACC_U
    u = V(W['W2'].T @ W['wo'], (256 + FIN_SLACK) * U * (W['W2'].abs().T @ W['wo'].abs()))
    t2, t2e = m2 * u.v, m2 * u.e
    if fused_route(c) if fused is None else fused:
        A = v_mm(V(W['W1']), V(w2), 256)
        a2 = V(w2.T @ W['wo'], (256 + FIN_SLACK) * U * (w2.abs().T @ W['wo'].abs()))
        y = t2 @ A.v + 2.0 * a2.v
        ya = t2.abs() @ A.v.abs() + 2.0 * a2.v.abs()
        e = (hl + acc) * ya + SECOND * (t2e @ A.v.abs() + t2.abs() @ A.e + 2.0 * a2.e)
    else:
        v = t2 @ W['W1'] + 2.0 * W['wo']
        va = t2.abs() @ W['W1'].abs() + 2.0 * W['wo'].abs()
        ve = (hl + acc) * va + SECOND * (t2e @ W['W1'].abs())
        y = v @ w2
        e = (hl + acc) * (va @ w2.abs()) + SECOND * (ve @ w2.abs())
    return m1 * y, m1 * (e + SPLIT[c.prec] * y.abs())


def wgrad_reference(c, F, m2, T1, Z1, g, gj, gh=None):
    """The eight sums of one net from the DECODED T1 and Z1 (fp64 values of bf16 planes: no operand error), (values, bounds, companion):
        S1 = M2^T Z1                 acc |M2|^T|Z1|                         (0 / 1 times a bf16 number: the products are exact)
        S2 = M2^T G6, G6 = g pe6     M2^T E_G6 + acc |M2|^T|G6|,            E_G6 = |g| (sc + SPLIT |pe6|) + (U + SPLIT) |G6|: the table's features and
                                                                            planes, the fp32 product, the planes of G6
        dw1 = T1^T Z0                |T1|^T (E_Z0 + (SPLIT + LOLO) |Z0|) + acc |T1|^T|Z0|
        mv, db1, q1, q6, sg          vec_steps U of the absolute-value sums (q6: + colsum E_G6)
    acc = acc_steps(n_pad / 16) ACC_U: the worst case over every summation order, the range plan's included."""
    n_pad = pad_points(c.n)
    acc, vec = acc_steps(n_pad // 16) * ACC_U, vec_steps(n_pad) * U
    sp, lolo = SPLIT[c.prec], LOLO[c.prec]
    ga = g.abs()
    g6, g6a = g[:, None] * F.pe6, ga[:, None] * F.pe6.abs()
    e_g6 = ga[:, None] * (F.sc + sp * F.pe6.abs()) + (U + sp) * g6a
    z0, z0a = F.z0(g, gj, gh)
    e_z0 = F.z0_error(g, gj, z0a, gh) + (sp + lolo) * z0a
    t1a, z1a = T1.abs(), Z1.abs()
    val = {'S1': m2.T @ Z1, 'S2': m2.T @ g6, 'dw1': T1.T @ z0, 'mv': m2.T @ g, 'db1': T1.T @ g, 'sg': g.sum(), 'q1': Z1.sum(0), 'q6': g6.sum(0)}
    comp = {'S1': m2.T @ z1a, 'S2': m2.T @ g6a, 'dw1': t1a.T @ z0a, 'mv': m2.T @ ga, 'db1': t1a.T @ ga, 'sg': ga.sum(), 'q1': z1a.sum(0), 'q6': g6a.sum(0)}
    bound = {'S1': acc * comp['S1'], 'S2': m2.T @ e_g6 + acc * comp['S2'], 'dw1': t1a.T @ e_z0 + acc * comp['dw1'],
             'mv': vec * comp['mv'], 'db1': vec * comp['db1'], 'sg': vec * comp['sg'], 'q1': vec * comp['q1'], 'q6': e_g6.sum(0) + vec * comp['q6']}
    return val, bound, comp


def finish(W, u, s):
    """phase_b's algebra behind the sums (what dpn_wgrad_finish computes from dpn_wgrad's partial sums), in the dtype of its operands."""
    w2, cvec = W['w2b2'][:, :256], W['w2b2'][:, 256] + W['bd'] + W['e']
    W1u = W['W1'].T * u[None, :]
    gcvec = W1u @ s['mv'] + 2.0 * W['wo'] * s['sg']
    G = s['S1'] @ w2.T + s['S2'] @ W['Wd'].T + s['mv'][:, None] * cvec[None, :]
    zsum = w2 @ s['q1'] + W['Wd'] @ s['q6'] + s['sg'] * cvec
    r = (W['W1'] * G).sum(1) + W['bf1'] * s['mv']
    return {'w1b1': torch.cat([s['dw1'], s['db1'][:, None]], 1),
            'w2b2': torch.cat([W1u @ s['S1'] + 2.0 * W['wo'][:, None] * s['q1'][None, :], gcvec[:, None]], 1),
            'e': gcvec, 'Wd': W1u @ s['S2'] + 2.0 * W['wo'][:, None] * s['q6'][None, :], 'bd': gcvec,
            'W1': u[:, None] * G, 'bf1': u * s['mv'], 'W2': W['wo'][:, None] * r[None, :], 'bf2': W['wo'] * s['sg'],
            'wo': W['W2'] @ r + W['bf2'] * s['sg'] + 2.0 * zsum, 'bo': s['sg']}


def companion(W, comp):
    """The absolute-value companion of the eleven gradients: finish() on |W|, |u| evaluated as |W2|^T|wo| and the sums' companions."""
    Wa = {k: v.abs() for k, v in W.items()}
    return finish(Wa, Wa['W2'].T @ Wa['wo'], comp)


def finish_bounds(W, s, e):
    """{name: V}: finish() of the sums s with element-wise bounds e on them, every fp32 operation of dpn_finish_* counted (V): u = W2^T wo from the pack
    kernel (256 terms), W1^T diag(u) (one product), the exact-fp32 GEMMs over 256 / 448 terms, the rank-one terms, cvec = (b2 + bd) + e."""
    w2 = V(W['w2b2'][:, :256])
    wo, Wd = V(W['wo']), V(W['Wd'])
    S = {k: V(s[k], e[k]) for k in SUMS}
    u = V(W['W2'].T @ W['wo'], (256 + FIN_SLACK) * U * (W['W2'].abs().T @ W['wo'].abs()))
    cvec = V(W['w2b2'][:, 256] + W['bd'] + W['e'], 2 * U * (W['w2b2'][:, 256].abs() + W['bd'].abs() + W['e'].abs()))
    W1u = v_mul(V(W['W1'].T), V(u.v[None, :], u.e[None, :]))
    two_wo = V(2.0 * wo.v)
    col = lambda x: V(x.v[:, None], x.e[:, None])
    row = lambda x: V(x.v[None, :], x.e[None, :])
    gcvec = v_add(v_mm(W1u, col(S['mv']), 256), v_mul(col(two_wo), V(S['sg'].v.reshape(1, 1), S['sg'].e.reshape(1, 1))))
    gcvec = V(gcvec.v[:, 0], gcvec.e[:, 0])
    w2g = v_add(v_mm(W1u, S['S1'], 256), v_mul(col(two_wo), row(S['q1'])))
    wdg = v_add(v_mm(W1u, S['S2'], 256), v_mul(col(two_wo), row(S['q6'])))
    G = v_add(v_mm(S['S1'], V(w2.v.T), 256), v_mm(S['S2'], V(Wd.v.T), 192), v_mul(col(S['mv']), row(cvec)))
    sg11 = V(S['sg'].v.reshape(1), S['sg'].e.reshape(1))
    zsum = v_add(v_mm(w2, col(S['q1']), 256), v_mm(Wd, col(S['q6']), 192))
    zsum = v_add(V(zsum.v[:, 0], zsum.e[:, 0]), v_mul(sg11, cvec))
    WG = v_mul(V(W['W1']), G)
    r = v_add(V(WG.v.sum(1), WG.e.sum(1) + (256 + FIN_SLACK) * U * WG.v.abs().sum(1)), v_mul(V(W['bf1']), S['mv']))
    out = {'w1b1': V(torch.cat([S['dw1'].v, S['db1'].v[:, None]], 1), torch.cat([S['dw1'].e, S['db1'].e[:, None]], 1)),
           'w2b2': V(torch.cat([w2g.v, gcvec.v[:, None]], 1), torch.cat([w2g.e, gcvec.e[:, None]], 1)),
           'e': gcvec, 'Wd': wdg, 'bd': gcvec, 'W1': v_mul(col(u), G), 'bf1': v_mul(u, S['mv']),
           'W2': v_mul(col(wo), row(r)), 'bf2': v_mul(wo, sg11),
           'wo': v_add(V(*_mv(V(W['W2']), r)), v_mul(V(W['bf2']), sg11), V(2.0 * zsum.v, 2.0 * zsum.e)),
           'bo': V(S['sg'].v, S['sg'].e)}
    return out


def _mv(A, x):
    r = v_mm(A, V(x.v[:, None], x.e[:, None]), A.v.shape[1])
    return r.v[:, 0], r.e[:, 0]


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic in torch (CPU stand-in)
ALTERS = ('s1_no_hi_lo',      # S1 without M2 . Z1_lo (the hi.lo product)
          's1_no_lo_hi',      # S1 without M2_lo . Z1_hi: M2 is 0 / 1 and HAS no lo plane -- the kernel issues no such product; see NULL_ALTERS
          'dw1_no_lo_hi',     # the product that has one: dw1 without T1_lo . Z0_hi
          'z1_no_lo', 'g6_no_lo', 'z0_no_lo', 't1_no_lo',       # a lost lo plane of one operand of the weight-gradient kernel
          'last_point',       # the last real point left out of every sum (a range that ends one point early)
          'no_wo_q1')         # d w2 without the rank-one term 2 wo (x) q1
NULL_ALTERS = ('s1_no_lo_hi',)                     # provably no change: asserted to be bit-identical to the faithful emulation, not to break a bound
HILO_ALTERS = ('s1_no_hi_lo', 'dw1_no_lo_hi', 'z1_no_lo', 'g6_no_lo', 'z0_no_lo', 't1_no_lo')       # need a lo plane: the hi+lo mode only


def _planes(x, prec):
    return KM._split(x, prec) if prec == 'bf16x2' else [KM._split(x, 'bf16')[0]]


def emulate(c, Ws, x, y, t, coord_data, g_out, g_jxi, pe_in=None, alters=(None,), g_hxi=None, z0_seed=None, geometry=GEOMETRY):
    """One pass of the kernels' arithmetic for case c in fp32 torch: kernel_model.phase_a / mm in the case's precision for the forward pass and
    stage 1, the planes of T1, Z1, G6, Z0 as the kernels write them, the weight-gradient products plane by plane, the finish in fp32.  Returns
    {alter: what the GPU test reads back, as fp64: {'m1', 'm2', 'T1', 'Z1', 'gnet', 'sums', 'sums_abs', 'grads', 'features'}} for every alter in
    `alters` (None: the faithful pass; the others: ALTERS, the seeded mistakes -- all of them sit behind stage 1, which is evaluated once).
    g_hxi [n, 6, 3]: the second derivatives' cotangent in the seed, Z0 = fmaf(gs, own, +-(gJ fr) partner) with gs = fmaf(-(gH fr), fr, g) as z0_frag_derivs
    forms it; the pass then also holds 'Z0' [6, n, 192], the stored rows (hi + lo).  z0_seed (with g_hxi), a mistake IN the seed: 'gh_fr' (gH fr for
    gH fr^2) | 'z0_lo_no_gh' (the stored lo plane taken from the Z0 without the gH term; the multiplied Z0 is right)."""
    F = Features(x, y, t, coord_data, geometry=geometry, pe_in=pe_in, prec=c.prec)
    n, prec = c.n, c.prec
    g_all, gj_all = scaled(c, g_out, g_jxi)
    gh_all = None if g_hxi is None else scaled(c, g_out, g_jxi, g_hxi)[2]
    fr = freqs()
    if pe_in is None:                       # the features as the device forms them: its own sin / cos in the hi+lo mode
        if prec == 'bf16x2':
            s3, c3 = (torch.from_numpy(a) for a in sincos_device(F.ang.numpy()))
        else:
            s3, c3 = torch.sin(F.ang), torch.cos(F.ang)
        pe32 = torch.stack([s3, c3], 2).reshape(n, -1)
        f = fr[:32][None, :, None]
        dpe32 = torch.stack([c3 * f, -s3 * f], 2)
    else:
        pe32, dpe32 = pe_in.float(), torch.zeros(n, 32, 2, 3)
    if prec == 'bf16x2':
        s6, c6 = (torch.from_numpy(a) for a in sincos_device(F.ang6.numpy()))
    else:
        s6, c6 = torch.sin(F.ang6), torch.cos(F.ang6)
    pe6_32 = torch.stack([s6, c6], 2).reshape(n, -1)
    passes = {a: {'m1': [], 'm2': [], 'T1': [], 'Z1': [], 'Z0': [], 'gnet': [], 'grads': [], 'sums': {k: [] for k in SUMS}} for a in alters}
    for k in range(6):
        W = {kk: v.float() for kk, v in Ws[k].items()}
        S = KM.phase_a(W, pe32, dpe32, pe6_32, torch.zeros(n), prec, fused=fused_route(c))[2]
        m1, m2 = S['m1'], S['m2']
        g, gj = g_all[k].float(), gj_all[k].float()
        z0 = g[:, None] * pe32 + (dpe32 * gj[:, None, None, :]).reshape(n, -1)
        if gh_all is not None:
            f3 = fr[:32][None, :, None, None].expand(n, 32, 2, 3)
            ghf = gh_all[k].float()[:, None, None, :] * f3
            gs = (g[:, None, None, None] - ghf * (1.0 if z0_seed == 'gh_fr' else f3)).reshape(n, -1)
            z0_plain, z0 = z0, gs * pe32 + (dpe32 * gj[:, None, None, :]).reshape(n, -1)
        w1, b1 = W['w1b1'][:, :192], W['w1b1'][:, 192]
        z1 = m1 * (KM.mm(z0, w1.T, prec) + g[:, None] * b1)
        T1p, Z1p, Z0p = _planes(S['t1'], prec), _planes(z1, prec), _planes(z0, prec)
        if gh_all is not None and z0_seed == 'z0_lo_no_gh' and prec == 'bf16x2':
            Z0p = [Z0p[0], _planes(z0_plain, prec)[1]]
        G6p = _planes(g[:, None] * sum(_planes(pe6_32, prec)), prec)
        for alter in alters:
            res = passes[alter]
            res['m1'].append(m1 > 0), res['m2'].append(m2 > 0)
            res['T1'].append(sum(p.double() for p in T1p)), res['Z1'].append(sum(p.double() for p in Z1p)), res['gnet'].append(g.double())
            res['Z0'].append(sum(p.double() for p in Z0p))
            # ---- dpn_wgrad: the products plane by plane, fp32 accumulation
            keep = torch.ones(n, 1)
            if alter == 'last_point':
                keep[n - 1] = 0.0
            X2, XT = (m2 * keep).T, [(p * keep).T for p in T1p]
            z1_s1 = Z1p[:1] if alter in ('z1_no_lo', 's1_no_hi_lo') else Z1p
            z1_q1 = Z1p[:1] if alter == 'z1_no_lo' else Z1p
            g6_used = G6p[:1] if alter == 'g6_no_lo' else G6p
            s = {'S1': sum(X2 @ p for p in z1_s1), 'S2': sum(X2 @ p for p in g6_used)}
            dw1 = XT[0] @ Z0p[0]
            if prec == 'bf16x2':
                if alter != 'z0_no_lo':
                    dw1 = dw1 + XT[0] @ Z0p[1]
                if alter not in ('t1_no_lo', 'dw1_no_lo_hi'):
                    dw1 = dw1 + XT[1] @ Z0p[0]
            s['dw1'] = dw1
            xt_vec = XT[:1] if alter == 't1_no_lo' else XT
            s['mv'], s['db1'], s['sg'] = X2 @ g, sum(p @ g for p in xt_vec), (g * keep[:, 0]).sum()
            s['q1'], s['q6'] = sum((p * keep).sum(0) for p in z1_q1), sum((p * keep).sum(0) for p in g6_used)
            for kk in SUMS:
                res['sums'][kk].append(s[kk].double())
            # ---- dpn_wgrad_finish
            gr = finish(W, S['u'], s)
            if alter == 'no_wo_q1':
                gr['w2b2'] = torch.cat([(W['W1'].T * S['u'][None, :]) @ s['S1'], gr['w2b2'][:, 256:]], 1)
            res['grads'].append({kk: v.double() for kk, v in gr.items()})
    out = {}
    for a, res in passes.items():
        o = {k: torch.stack(res[k]) for k in ('m1', 'm2', 'T1', 'Z1', 'Z0', 'gnet')}
        o['grads'], o['features'] = res['grads'], F
        o['sums'] = {k: torch.stack(v) for k, v in res['sums'].items()}
        o['sums_abs'] = {k: v.abs() for k, v in o['sums'].items()}            # one range
        out[a] = o
    return out


# ---------------------------------------------------------------------------------------------- the pass conditions
def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is zero the values must agree exactly (inf otherwise)."""
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def check(c, Ws, F, obs, g_out, g_jxi, stages=('stage1', 'saved', 'wgrad', 'finish', 'chain'), g_hxi=None):
    """{(stage, tensor): worst error-to-bound ratio over the six nets} of what a pass `obs` (emulate() or the GPU's read-back) holds.  g_hxi [n, 6, 3]:
    the second derivatives' cotangent (dpn_bwd_points_derivs), carried through every stage; stage 'z0' (only where asked for): the stored Z0 rows
    obs['Z0'] [6, n, 192] against Z0 itself, bound: the forming's error and the planes it is written as."""
    g_all, gj_all = scaled(c, g_out, g_jxi)
    gh_all = [None] * 6 if g_hxi is None else scaled(c, g_out, g_jxi, g_hxi)[2]
    out = {}

    def put(stage, name, r):
        out[(stage, name)] = max(out.get((stage, name), 0.0), r)
    for k in range(6):
        W, g, gj, gh = Ws[k], g_all[k], gj_all[k], gh_all[k]
        m1, m2 = obs['m1'][k].double(), obs['m2'][k].double()
        T1, Z1 = obs['T1'][k], obs['Z1'][k]
        if 'z0' in stages:
            z0, z0a = F.z0(g, gj, gh)
            put('z0', 'Z0', ratio(obs['Z0'][k], z0, F.z0_error(g, gj, z0a, gh) + SPLIT[c.prec] * z0a))
        if 'stage1' in stages:
            ref, bound = stage1_reference(c, W, F, m1, g, gj, gh)
            put('stage1', 'Z1', ratio(Z1, ref, bound))
        if 'saved' in stages:
            ref, bound = t1_reference(c, W, F, m1, m2)
            put('saved', 'T1', ratio(T1, ref, bound))
        val, bound, comp = wgrad_reference(c, F, m2, T1, Z1, g, gj, gh)
        got = {kk: obs['sums'][kk][k] for kk in SUMS}
        if 'wgrad' in stages:
            for kk in SUMS:
                put('wgrad', kk, ratio(got[kk], val[kk], bound[kk]))
        if 'finish' in stages:      # from the pass's OWN sums: the fp32 addition of the ranges is the only error they carry into the finish
            fb = finish_bounds(W, got, {kk: MAX_SPLITS * U * obs['sums_abs'][kk][k] for kk in SUMS})
            for nm in NAMES:
                put('finish', nm, ratio(obs['grads'][k][nm], fb[nm].v, fb[nm].e))
        if 'chain' in stages:       # the oracle's phase_b on the pass's m1, m2, T1, Z1: the weight kernels' own bounds, carried through the finish
            ref = reference(W, (m1, m2), F.pe, F.dpe, F.pe6, g_out[:, k], g_jxi[:, k] if g_jxi is not None else torch.zeros(c.n, 3), c.scale, t1=T1, z1=Z1,
                            g_hxi=None if g_hxi is None else g_hxi[:, k], d2pe=F.d2pe)
            fb = finish_bounds(W, val, {kk: bound[kk] + MAX_SPLITS * U * comp[kk] for kk in SUMS})
            for nm in NAMES:
                put('chain', nm, ratio(obs['grads'][k][nm], ref[nm].reshape(fb[nm].v.shape), fb[nm].e))
    return out
