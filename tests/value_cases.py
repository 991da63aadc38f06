"""Case table, fp64 references and pass conditions for the VALUE side of the point path: what the forward point kernels return -- dpn_fwd, dpn_fwd_ref,
dpn_fwd_ref_nets, dpn_fwd_ref_derivs (csrc/dpn_tiles_kernels.inc, dpn_ring_kernels.inc): fields, Jacobian, second and third coordinate derivatives and
the two ReLU masks -- and what dpn_bwd_points_derivs feeds into the weight side when the second derivatives carry a cotangent (g_hxi).  Imports
without a GPU: tests/test_value_cases_cpu.py runs the table through emulate_value(), a torch model of the kernels' fp32 / plane arithmetic, and seeds
mistakes into it; tests/test_gpu_value_fp64.py runs it through the C ABI (tools/value_digest.run_case).

The method is the weight side's (tests/wgrad_cases.py, which this module builds on): every stage starts from the kernels' OWN upstream tensors -- the
saved masks and, where named, the decoded T1 planes -- so that no kink flips have to be removed and every bound is a one-stage bound; every bound is a
named constant times the same expression on absolute values; nothing is normalised by a tensor's maximum.  Weights are the fp32 tensors handed to the
pack call, features are fp64 sin / cos of the fp32 angles (wgrad_cases.Features).  Stages:
  'masks'  wherever a saved mask bit differs from pre64 > 0, |pre64| <= E_pre at that element (pre2 under the kernels' own m1): a differing bit needs a
           pre-activation within rounding of zero.  No cap, no removed point.
  'out'    out_n against the fields of kernel_model.phase_a under the kernels' masks, + ref_data (coord_data for dpn_fwd)
  'stage'  jac_n, hess_n, d3_n against gpe = T1 w1 of the DECODED T1 planes (the kernels multiply exactly those planes: frag_set2 -> x_store_all ->
           gemm in the tile kernels, frag_set2 -> actA -> mma_chunk in the ring kernels), contracted with d pe, d2 pe, d3 pe per coordinate and divided
           by the fp32 geometry values in fp64
  'chain'  the same outputs against phase_a under the masks, T1 from wgrad_cases.t1_reference with ITS bound: does not depend on T1 being right
and, for g_hxi, wgrad_cases.check() with the cotangent carried through ('z0': the stored Z0 rows themselves, then 'stage1', 'wgrad', 'finish', 'chain').
"""
from collections import namedtuple

import torch

import wgrad_cases as WC
from wgrad_cases import ACC_U, C_B, C_HL, F64, FIN_SLACK, LOLO, SECOND, SPLIT, U, V, acc_steps, v_add, v_mm

# ---------------------------------------------------------------------------------------------- named constants (counts read off the kernels' text)
PACK_TERMS = 256      # the pack kernels' fp32 products A = W1 w2, B = W1 Wd, W1 cvec (v_mfma_f32_32x32x2f32 over 256 terms, four waves folded) and the
#                       256-term fmaf chains of u = W2^T wo, a2 = w2^T wo, bv = Wd^T wo (eight groups of 32, folded): + FIN_SLACK as in the finish stage
DOT_TILES = 32        # tile kernels: adot, hdot (and ddot: 24) are fmaf chains over the lane's 2 tiles x 16 accumulator registers
DOT_RING = 128        # ring kernels: adot and cdot run over the lane's 8 tiles x 16 registers
OUT_FOLD_TILES = 2 + 1 + 2 + 2     # o = adot + 2 (hdot + ddot): two additions; the half-wave fold; four waves in two levels; + const0, + ref
OUT_FOLD_RING = 1 + 1 + 2          # o = adot + 2 cdot; the half-wave fold; + const0, + ref
OUT_SLACK = 1
JAC_STEPS = 64 + 1    # one coordinate's 64 features: at most 64 fmaf steps (32 per lane in either kernel) and the half-wave fold
DERIV_OPS = (1, 2, 3)  # roundings that form the k-th derivative feature from (s, co): fr co | fr fr, f2 s | fr co, fr fr, f2 d
DIV_OPS = 2           # one fp32 division: correctly rounded (U) in this build; one unit of slack for a division that is only faithful


# ---------------------------------------------------------------------------------------------- case table
GEOMETRIES = {'ncep': WC.GEOMETRY,                                         # dx == dy: a dx <-> dy mix-up is invisible here
              'odd': (25000.0, 31000.0, 100.0, 60.0, 43200.0)}            # every factor distinct and no power of two
VCase = namedtuple('VCase', 'route n prec gain geo coords entry kernel')
SIZES = (1,       # one real point
         63, 64, 65,   # around the tile forward's 64-point workgroup (and the second 32-point tile's last / first lanes)
         70,      # ragged: two 32-point tiles and six points
         129,     # the first point behind the ring kernels' 128-point workgroup
         1037)    # many workgroups and a ragged tail of 13
COORDS = ('interior',     # oracle.fill.synthetic_inputs (NCEP) or uniform xi in [0, 1)
          'edges',        # the first eight points: every combination of xi_c exactly 0 and exactly 1 (t = 0 among them)
          'beyond')       # xi uniform in [-0.5, 1.5): the angles reach 24; the sin / cos yardstick is measured on the case's own angles
ENTRIES = ('fwd',         # dpn_fwd: coord_data is what is added to the fields
           'ref',         # dpn_fwd_ref with a distinct random ref_data
           'derivs')      # dpn_fwd_ref_derivs, hess_n and d3_n on, the same ref_data
GH_SIZES = (70, 1037)
GH_KINDS = ('dense', 'gh_only')
GH_INPUTS = VCase('raw', 0, 'bf16x2', 1.0, 'odd', 'interior', 'derivs', None)       # the g_hxi passes' geometry and coordinates (n filled in): stage 1 forms xi itself


def all_cases():
    out = [VCase('raw', n, 'bf16x2', 1.0, 'ncep', 'interior', 'derivs', None) for n in SIZES]               # tile kernels, fused form
    for n in (70, 1037):
        out += [VCase('raw', n, 'bf16x2', gain, 'odd', co, 'derivs', None) for gain in (1.0, 5.0) for co in COORDS]
        out.append(VCase('raw', n, 'bf16', 1.0, 'odd', 'interior', 'derivs', None))                         # ring kernels, plain bf16
    out += [VCase('raw', 65, 'bf16x2', 5.0, 'ncep', 'edges', 'fwd', None), VCase('raw', 129, 'bf16x2', 1.0, 'odd', 'beyond', 'ref', None),
            VCase('raw', 70, 'bf16', 5.0, 'odd', 'beyond', 'derivs', None), VCase('raw', 70, 'bf16', 1.0, 'ncep', 'edges', 'fwd', None),
            VCase('raw', 70, 'bf16x2', 1.0, 'odd', 'interior', 'derivs', 'ring')]                           # hi+lo on the ring kernels (DPN_FWD_KERNEL=ring)
    out += [VCase('pe_in', 70, prec, 1.0, 'ncep', 'interior', 'ref', None) for prec in ('bf16x2', 'bf16')]  # fields and masks only
    return out


def case_id(c):
    return '%s-%d-%s-g%g-%s-%s-%s-%s' % (c.route, c.n, c.prec, c.gain, c.geo, c.coords, c.entry, c.kernel or 'default')


def fused(c):
    """dpn_fwd_form under the case's kernel choice: the tile kernels multiply the five-GEMM stream, the ring kernels the seven-GEMM one."""
    return c.route == 'raw' and c.prec == 'bf16x2' and c.kernel != 'ring'


def inputs(c):
    """Host inputs of case c (fp32): x, y, t [n] generated as xi and multiplied out in fp32, coord_data, ref_data [n, 6] (None for dpn_fwd), pe_in."""
    from oracle.fill import synthetic_inputs, unit_uniform
    n = c.n
    inp = synthetic_inputs(n, tag='inter')
    dx, dy, lon_m1, lat_m1, span = (torch.tensor(v, dtype=torch.float32) for v in GEOMETRIES[c.geo])
    if c.geo == 'ncep' and c.coords == 'interior':
        x, y, t = (inp[k].reshape(-1).clone() for k in ('x', 'y', 't'))
    else:
        u = [(torch.from_numpy(unit_uniform('value.' + k, n)) + 1.0) * 0.5 for k in 'xyt']
        if c.coords == 'beyond':
            u = [2.0 * v - 0.5 for v in u]
        if c.coords == 'edges':
            for i in range(min(n, 8)):
                u[0][i], u[1][i], u[2][i] = float(i & 1), float((i >> 1) & 1), float((i >> 2) & 1)
        x, y, t = (u[0] * lon_m1) * dx, (u[1] * lat_m1) * dy, u[2] * span
    ref = None if c.entry == 'fwd' else torch.randn(n, 6, generator=torch.Generator().manual_seed(7))
    pe_in = WC.pe_in_of(n) if c.route == 'pe_in' else None
    return dict(x=x.float().contiguous(), y=y.float().contiguous(), t=t.float().contiguous(), coord_data=inp['coord_data'].contiguous(), ref_data=ref,
                pe_in=pe_in)


def features(c, inp):
    return WC.Features(inp['x'], inp['y'], inp['t'], inp['coord_data'], geometry=GEOMETRIES[c.geo], pe_in=inp['pe_in'], prec=c.prec)


def gh_case(n, gain=1.0):
    """The weight-side case of the g_hxi passes: raw coordinates, hi+lo, the tile kernels, Z0 in the STORED form (dpn_bwd_tiles_deriv_kernel)."""
    return WC.Case('raw', n, 'bf16x2', gain, 'dense', 0.75)


def gh_cotangents(n, kind):
    """(g_out [n, 6], g_jxi [n, 6, 3], g_hxi [n, 6, 3]): wgrad_cases' dense streams and a third one for the second derivatives; 'gh_only': the others zero."""
    g_out, g_jxi = WC.cotangents(gh_case(n))
    g_hxi = torch.randn(n, 6, 3, generator=torch.Generator().manual_seed(3))
    if kind == 'gh_only':
        g_out, g_jxi = torch.zeros_like(g_out), torch.zeros_like(g_jxi)
    return g_out, g_jxi, g_hxi


# ---------------------------------------------------------------------------------------------- references and bounds, one net
def _hl(prec):
    return C_HL * 2.0 ** -16 if prec == 'bf16x2' else C_B * 2.0 ** -8


def _pack_vec(M, x):
    """M^T x as a pack kernel forms it in fp32: a 256-term fmaf chain in eight folded groups."""
    return V(M.T @ x, (PACK_TERMS + FIN_SLACK) * U * (M.abs().T @ x.abs()))


def packed_products(W, is_fused):
    """The fp32 quantities the pack kernels derive from the weights, as values with bounds (V): u, cvec and const0 in both forms; A, B, C2, a2, bv in the
    fused one (dpn_pack_fused_kernel, pack_vectors)."""
    b2 = W['w2b2'][:, 256]
    w2 = W['w2b2'][:, :256]
    cabs = b2.abs() + W['bd'].abs() + W['e'].abs()
    P = {'u': _pack_vec(W['W2'], W['wo']), 'cvec': V(b2 + W['bd'] + W['e'], 2 * U * cabs)}
    c0 = W['wo'] @ W['bf2'] + W['bo']
    c0a = W['wo'].abs() @ W['bf2'].abs() + W['bo'].abs()
    if is_fused:
        c0, c0a = c0 + 2.0 * (W['wo'] @ P['cvec'].v), c0a + 2.0 * (W['wo'].abs() @ cabs)
        P['A'], P['B'] = v_mm(V(W['W1']), V(w2), PACK_TERMS), v_mm(V(W['W1']), V(W['Wd']), PACK_TERMS)
        wc = v_mm(V(W['W1']), V(P['cvec'].v[:, None], P['cvec'].e[:, None]), PACK_TERMS)
        P['C2'] = v_add(V(wc.v[:, 0], wc.e[:, 0]), V(W['bf1']))
        P['a2'], P['bv'] = _pack_vec(w2, W['wo']), _pack_vec(W['Wd'], W['wo'])
    P['const0'] = V(c0, (PACK_TERMS + FIN_SLACK) * U * c0a)        # a product, the two additions of cvec, an eight-level tree, + bo: far fewer than 256 steps
    P['const0_abs'] = c0a
    return P


def forward_reference(c, W, F, m1, m2, ref):
    """One net under the forced masks m1, m2 [n, 256] (fp64 0 / 1), ref [n]: {'pre1', 'e_pre1', 'pre2', 'e_pre2', 'out', 'e_out'}.
        E_pre1 = (HL + acc_steps(12) ACC_U) (|pe||w1|^T + |b1|) + sc sum|w1|
      fused (tile kernels):
        pre2 = (m1 pre1) A^T + pe6 B^T + C2         E_pre2 = (HL + acc_steps(28) ACC_U) |.| + E_pre1 |A|^T + sc sum|B| + the pack kernel's E_A, E_B, E_C2
        out  = (m2 u) . pre2 + 2 (a2 . h1 + bv . pe6) + const0 + ref
      ring kernels:
        c = h1 w2^T + pe6 Wd^T + cvec  (28 k-steps),  pre2 = c W1^T + bf1  (16 k-steps),  out = (m2 u) . pre2 + 2 wo . c + const0 + ref
    E_out carries E_pre2, E_pre1, the features' error and the pack kernel's errors through absolute values and adds the fp32 steps of the dot products'
    fmaf chains and folds (DOT_*, OUT_FOLD_*) on the absolute-value evaluation of out."""
    w1, b1, w2 = W['w1b1'][:, :192], W['w1b1'][:, 192], W['w2b2'][:, :256]
    hl, is_fused = _hl(c.prec), fused(c)
    P = packed_products(W, is_fused)
    pe, pe6 = F.pe, F.pe6
    pre1 = pe @ w1.T + b1
    e_pre1 = (hl + acc_steps(12) * ACC_U) * (pe.abs() @ w1.abs().T + b1.abs()) + SECOND * F.sc3 * w1.abs().sum(1)[None, :]
    h1, eh1 = m1 * pre1, m1 * e_pre1
    u = P['u']
    t2, t2e = m2 * u.v, m2 * u.e
    if is_fused:
        A, B, C2, a2, bv = P['A'], P['B'], P['C2'], P['a2'], P['bv']
        pre2 = h1 @ A.v.T + pe6 @ B.v.T + C2.v
        pre2a = h1.abs() @ A.v.abs().T + pe6.abs() @ B.v.abs().T + C2.v.abs()
        e_pre2 = (hl + acc_steps(28) * ACC_U) * pre2a + SECOND * (eh1 @ A.v.abs().T + h1.abs() @ A.e.T + F.sc * B.v.abs().sum(1)[None, :] + pe6.abs() @ B.e.T + C2.e)
        side = 2.0 * (h1 @ a2.v + pe6 @ bv.v)
        sidea = 2.0 * (h1.abs() @ a2.v.abs() + pe6.abs() @ bv.v.abs())
        e_side = 2.0 * (eh1 @ a2.v.abs() + h1.abs() @ a2.e + F.sc * bv.v.abs().sum() + pe6.abs() @ bv.e)
        steps = DOT_TILES + OUT_FOLD_TILES + OUT_SLACK
    else:
        cv = P['cvec']
        cc = h1 @ w2.T + pe6 @ W['Wd'].T + cv.v
        cca = h1.abs() @ w2.abs().T + pe6.abs() @ W['Wd'].abs().T + cv.v.abs()
        e_c = (hl + acc_steps(28) * ACC_U) * cca + SECOND * (eh1 @ w2.abs().T + F.sc * W['Wd'].abs().sum(1)[None, :] + cv.e)
        pre2 = cc @ W['W1'].T + W['bf1']
        pre2a = cc.abs() @ W['W1'].abs().T + W['bf1'].abs()
        e_pre2 = (hl + acc_steps(16) * ACC_U) * pre2a + SECOND * (e_c @ W['W1'].abs().T)
        side, sidea, e_side = 2.0 * (cc @ W['wo']), 2.0 * (cc.abs() @ W['wo'].abs()), 2.0 * (e_c @ W['wo'].abs())
        steps = DOT_RING + OUT_FOLD_RING + OUT_SLACK
    out = (pre2 * t2).sum(1) + side + P['const0'].v + ref
    outa = (pre2.abs() * t2.abs()).sum(1) + sidea + P['const0_abs'] + ref.abs()
    e_out = steps * U * outa + SECOND * ((e_pre2 * t2.abs() + pre2.abs() * t2e).sum(1) + e_side + P['const0'].e)
    return dict(pre1=pre1, e_pre1=e_pre1, pre2=pre2, e_pre2=e_pre2, out=out, e_out=e_out)


def mask_condition(mask, pre, e_pre):
    """(ratio, differing bits): max |pre64| / E_pre over the elements where the saved bit is not pre64 > 0 (0.0 where none differs)."""
    diff = mask.bool() != (pre > 0)
    if not bool(diff.any()):
        return 0.0, 0
    return float((pre.abs()[diff] / e_pre[diff]).max()), int(diff.sum())


def deriv_reference(c, W, F, T1, e_t1=None):
    """{'jac' | 'hess' | 'd3': (reference, bound)} [n, 3] of one net from T1 [n, 256] -- the decoded planes (e_t1 None: they are the operand, no error) or
    t1_reference's value with its bound e_t1:
        gpe = T1 w1                              E_gpe = (SPLIT + LOLO + acc_steps(16) ACC_U) |T1||w1|  (+ e_t1 |w1|)
        raw_k = sum_f gpe . d^k pe / d xi_c^k     E_raw = E_gpe . |d^k| + G . E_dk + JAC_STEPS U G . |d^k|,  G = |gpe| + E_gpe,
                                                 E_dk = fr^k sc + DERIV_OPS[k] U |d^k|
        out_k = raw_k / (g1 g2)^k                 + 2 k DIV_OPS U (|raw_k| + E_raw), all of it divided by the fp64 (g1 g2)^k
    g1 = (lon - 1, lat - 1, span), g2 = (dx, dy, 1): the fp32 geometry values."""
    n = F.n
    w1 = W['w1b1'][:, :192]
    dx, dy, lon_m1, lat_m1, span = (float(torch.tensor(v, dtype=torch.float32)) for v in GEOMETRIES[c.geo])
    gg = torch.tensor([lon_m1 * dx, lat_m1 * dy, span], dtype=F64)
    t1a = T1.abs() if e_t1 is None else T1.abs() + e_t1
    gpe = (T1 @ w1).reshape(n, 32, 2, 3)
    e_gpe = (SPLIT[c.prec] + LOLO[c.prec] + acc_steps(16) * ACC_U) * (t1a @ w1.abs())
    if e_t1 is not None:
        e_gpe = e_gpe + SECOND * (e_t1 @ w1.abs())
    e_gpe = e_gpe.reshape(n, 32, 2, 3)
    G = gpe.abs() + e_gpe
    fr = F.fr.reshape(32, 2, 3)[None]
    out = {}
    for k, (name, d) in enumerate((('jac', F.dpe), ('hess', F.d2pe), ('d3', F.d3pe)), 1):
        e_d = fr ** k * F.sc3 + DERIV_OPS[k - 1] * U * d.abs()
        raw = (gpe * d).sum(dim=(1, 2))
        e_raw = (e_gpe * d.abs() + G * e_d + JAC_STEPS * U * G * d.abs()).sum(dim=(1, 2))
        out[name] = (raw / gg ** k, SECOND * (e_raw + 2 * k * DIV_OPS * U * (raw.abs() + e_raw)) / gg ** k)
    return out


STAGES = ('masks', 'out', 'stage', 'chain')
DERIV_NAMES = ('jac', 'hess', 'd3')


def check_value(c, Ws, F, obs, ref6, stages=STAGES):
    """{(stage, tensor): worst ratio over the six nets} of what a pass holds: obs = {'m1', 'm2' bool [6, n, 256], 'T1' [6, n, 256] fp64, 'out' [n, 6],
    'jac' / 'hess' / 'd3' [n, 6, 3] or None}; ref6 [n, 6]: what the entry point adds to the fields.  Also ('masks', 'bits'): the differing bits (a count,
    printed, not a condition)."""
    res = {}

    def put(stage, name, r):
        res[(stage, name)] = max(res.get((stage, name), 0.0), r)
    for k in range(6):
        W = Ws[k]
        m1, m2 = obs['m1'][k].double(), obs['m2'][k].double()
        R = forward_reference(c, W, F, m1, m2, ref6[:, k].double())
        if 'masks' in stages:
            r1, n1 = mask_condition(obs['m1'][k], R['pre1'], R['e_pre1'])
            r2, n2 = mask_condition(obs['m2'][k], R['pre2'], R['e_pre2'])
            put('masks', 'm1', r1), put('masks', 'm2', r2)
            res[('masks', 'bits')] = res.get(('masks', 'bits'), 0) + n1 + n2
        if 'out' in stages:
            put('out', 'out', WC.ratio(obs['out'][:, k].double(), R['out'], R['e_out']))
        names = [nm for nm in DERIV_NAMES if obs.get(nm) is not None]
        if names and 'stage' in stages:
            D = deriv_reference(c, W, F, obs['T1'][k])
            for nm in names:
                put('stage', nm, WC.ratio(obs[nm][:, k].double(), *D[nm]))
        if names and 'chain' in stages:
            t1, e_t1 = WC.t1_reference(c, W, F, m1, m2, fused=fused(c))
            D = deriv_reference(c, W, F, t1, e_t1)
            for nm in names:
                put('chain', nm, WC.ratio(obs[nm][:, k].double(), *D[nm]))
    return res


def conditions(r):
    """the entries of check_value's result that are pass conditions (all but the printed bit count)"""
    return {k: v for k, v in r.items() if k != ('masks', 'bits')}


def z0_reference(F, g, gj, gh):
    """(Z0, bound) of the stored rows of one net: Z0 = (g - gH fr^2) pe + gJ fr (cos, -sin) and what forming it in fp32 and writing it as hi+lo planes may miss."""
    z0, z0a = F.z0(g, gj, gh)
    return z0, F.z0_error(g, gj, z0a, gh) + SPLIT[F.prec] * z0a


def decode_z0_stored(operands, n, prec):
    """The stored Z0 rows (OperandView.Z0: a K-layout matrix of 6 column tiles behind Z1) as ([6, n, 192] fp64 = hi + lo in the reference's channel order,
    the planes [6, planes, n, 192]); the padding rows are asserted to be exactly zero."""
    ns, n_pad = (2 if prec == 'bf16x2' else 1), WC.pad_points(n)
    z = WC.kmat_decode(operands, 6 * ns * n_pad * 512, 6, ns, n_pad, 6)
    assert not bool(z[:, :, n:].any()), 'Z0 of a padding point is not zero'
    planes = z[:, :, :n][:, :, :, WC.SLOT_OF_PE3]
    return planes.sum(1), planes


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic in torch (CPU stand-in)
SEEDS = ('l1_no_lo_hi',        # layer 1 without pe_lo . w1_hi
         'gpe_no_hi_lo',       # gpe without t1_hi . w1_lo
         'no_wd_wo',           # the fields without 2 (Wd^T wo) . pe6
         'no_wo_cvec',         # const0 without 2 wo . cvec
         'coord_as_ref',       # coord_data added where ref_data was given
         'dx_dy',              # dx <-> dy in the chain rule of all three derivative outputs
         'hess_one_division',  # hess_n with one / g1 / g2 too few
         'd3_from_pe',         # d3 contracted with -fr^2 pe instead of -fr^2 d pe
         'd2_swapped',         # the sin / cos slots of d2 swapped
         'last_from_padding',  # the derivative outputs of the last real point taken from the padding row behind it
         'masks_next_net')     # at two points, the masks of net k + 1 exported for net k
HILO_SEEDS = ('l1_no_lo_hi', 'gpe_no_hi_lo')
FUSED_SEEDS = ('no_wd_wo', 'no_wo_cvec')        # terms of the five-GEMM form only: the ring kernels take 2 wo . c from the accumulators of c itself


def mm_planes(a, b, prec, drop=None):
    """a @ b on bf16 planes, fp32 accumulation; drop: 'lo_hi' (a_lo . b_hi) | 'hi_lo' (a_hi . b_lo) left out (hi+lo mode)."""
    from oracle.kernel_model import _split
    if prec == 'bf16':
        return _split(a, 'bf16')[0] @ _split(b, 'bf16')[0]
    (ah, al), (bh, bl) = _split(a, 'bf16x2'), _split(b, 'bf16x2')
    out = ah @ bh
    if drop != 'hi_lo':
        out = out + ah @ bl
    if drop != 'lo_hi':
        out = out + al @ bh
    return out


def emulate_value(c, Ws, inp, seeds=(None,)):
    """One forward pass of case c in fp32 torch as the kernels run it -- the device's sin / cos formulas (hi+lo mode), bf16 planes of every GEMM operand, the
    pack kernels' fp32 products, fp32 dot products and divisions -- for every seed in `seeds` (None: the faithful pass).  Returns {seed: obs} in
    check_value's form.  The pass runs on n + 1 points: the extra one, all coordinates zero, is what a padding row behind the last point holds."""
    from oracle.kernel_model import _split
    n, prec, is_fused = c.n, c.prec, fused(c)
    f32 = torch.float32
    ext = {k: (None if v is None else torch.cat([v.float(), torch.zeros(1, *v.shape[1:])])) for k, v in inp.items()}
    ext_ref = ext['coord_data'] if ext['ref_data'] is None else ext['ref_data']
    F = WC.Features(ext['x'], ext['y'], ext['t'], ext['coord_data'], geometry=GEOMETRIES[c.geo], pe_in=ext['pe_in'], prec=prec)
    fr = WC.freqs()
    sincos = (lambda a: tuple(torch.from_numpy(v) for v in WC.sincos_device(a.numpy()))) if prec == 'bf16x2' else (lambda a: (torch.sin(a), torch.cos(a)))
    s6, c6 = sincos(F.ang6)
    pe6 = torch.stack([s6, c6], 2).reshape(n + 1, -1)
    raw = c.route == 'raw'
    if raw:
        s3, c3 = sincos(F.ang)
        pe = torch.stack([s3, c3], 2).reshape(n + 1, -1)
        f = fr[:32][None, :, None]
        f2 = f * f
        d1 = torch.stack([f * c3, -(f * s3)], 2)
        d2 = torch.stack([-(f2 * s3), -(f2 * c3)], 2)
        d3 = torch.stack([-(f2 * d1[:, :, 0]), -(f2 * d1[:, :, 1])], 2)
    else:
        pe = ext['pe_in']
    dx, dy, lon_m1, lat_m1, span = (torch.tensor(v, dtype=f32) for v in GEOMETRIES[c.geo])
    one = torch.tensor(1.0)
    passes = {s: {'m1': [], 'm2': [], 'T1': [], 'out': [], 'jac': [], 'hess': [], 'd3': []} for s in seeds}
    for k in range(6):
        W = {kk: v.float() for kk, v in Ws[k].items()}
        w1, b1, w2, b2 = W['w1b1'][:, :192], W['w1b1'][:, 192], W['w2b2'][:, :256], W['w2b2'][:, 256]
        cvec = (b2 + W['bd']) + W['e']
        u = W['W2'].T @ W['wo']
        if is_fused:
            A, B, C2, a2, bv = W['W1'] @ w2, W['W1'] @ W['Wd'], W['W1'] @ cvec + W['bf1'], w2.T @ W['wo'], W['Wd'].T @ W['wo']
        for seed in seeds:
            res = passes[seed]
            pre1 = mm_planes(pe, w1.T, prec, 'lo_hi' if seed == 'l1_no_lo_hi' else None) + b1
            m1 = (pre1 > 0).float()
            h1 = pre1 * m1
            if is_fused:
                pre2 = mm_planes(h1, A.T, prec) + mm_planes(pe6, B.T, prec) + C2
                m2 = (pre2 > 0).float()
                const0 = W['wo'] @ W['bf2'] + W['bo'] + (0.0 if seed == 'no_wo_cvec' else 2.0 * (W['wo'] @ cvec))
                side = h1 @ a2 + (0.0 if seed == 'no_wd_wo' else pe6 @ bv)
                y = mm_planes(m2 * u, A, prec) + 2.0 * a2
            else:
                cc = mm_planes(h1, w2.T, prec) + mm_planes(pe6, W['Wd'].T, prec) + cvec
                pre2 = mm_planes(cc, W['W1'].T, prec) + W['bf1']
                m2 = (pre2 > 0).float()
                const0 = W['wo'] @ W['bf2'] + W['bo']
                side = cc @ W['wo']
                y = mm_planes(mm_planes(m2 * u, W['W1'], prec) + 2.0 * W['wo'], w2, prec)
            added = ext['coord_data'] if seed == 'coord_as_ref' else ext_ref
            out = ((pre2 * (m2 * u)).sum(1) + 2.0 * side) + const0 + added[:, k]
            t1 = m1 * y
            res['T1'].append(sum(p.double() for p in WC._planes(t1, prec))[:n])
            em1, em2 = (m1 > 0)[:n].clone(), (m2 > 0)[:n].clone()
            res['m1'].append(em1), res['m2'].append(em2), res['out'].append(out[:n].double())
            if raw:
                gpe = mm_planes(t1, w1, prec, 'hi_lo' if seed == 'gpe_no_hi_lo' else None).reshape(n + 1, 32, 2, 3)
                e2 = d2.flip(2) if seed == 'd2_swapped' else d2
                e3 = d2 if seed == 'd3_from_pe' else d3
                r1, r2, r3 = ((gpe * d).sum(dim=(1, 2)) for d in (d1, e2, e3))
                g1 = torch.stack([lon_m1, lat_m1, span])
                g2 = torch.stack([dy, dx, one]) if seed == 'dx_dy' else torch.stack([dx, dy, one])
                jac = r1 / g1 / g2
                hess = r2 / g1 / g2 if seed == 'hess_one_division' else r2 / g1 / g2 / g1 / g2
                dd3 = r3 / g1 / g2 / g1 / g2 / g1 / g2
                for nm, v in (('jac', jac), ('hess', hess), ('d3', dd3)):
                    v = v.double()
                    if seed == 'last_from_padding':
                        v[n - 1] = v[n]
                    res[nm].append(v[:n])
    out = {}
    for seed, res in passes.items():
        o = {kk: torch.stack(res[kk]) for kk in ('m1', 'm2', 'T1')}
        if seed == 'masks_next_net':
            for nm in ('m1', 'm2'):
                wrong = o[nm].roll(-1, 0)
                for p in {0, n - 1}:
                    o[nm][:, p] = wrong[:, p]
        o['out'] = torch.stack(res['out'], 1)
        for nm in DERIV_NAMES:
            o[nm] = torch.stack(res[nm], 1) if raw else None
        o['features'] = WC.Features(inp['x'], inp['y'], inp['t'], inp['coord_data'], geometry=GEOMETRIES[c.geo], pe_in=inp['pe_in'], prec=prec)
        o['ref6'] = (inp['coord_data'] if inp['ref_data'] is None else inp['ref_data']).float()
        out[seed] = o
    return out
