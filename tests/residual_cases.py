"""Case table, input builders, fp64 reference and bounds for the residual and loss family of csrc/dpn_residual.hip (dpn_residual_points,
dpn_residual, dpn_residual_weighted, dpn_step_residual, dpn_step_finish_batch, dpn_residual_finish[_batch], dpn_smooth_l1, dpn_contract_gpe).
Imports without a GPU: tests/test_residual_cases_cpu.py checks the reference and the bounds, tests/test_gpu_residual.py runs the kernels.

The reference restates none of the kernel's analytic derivative.  Point by point it hands the oracle fields that are affine in the coordinates,
    o_k = A[:, k] + B[:, k, 0] x + B[:, k, 1] y + B[:, k, 2] t        A = out_n, B = jac_n: fp64 leaves;  x = y = t = 0: leaves,
de-normalises them (`denorm`: oracle.inverse_norm line for line, over a table that can also say what a C caller's DpnPhysics can and the
oracle's norm_cfg cannot; the CPU test proves the two bit-identical on the three shipped tables), takes the six signed residuals from
oracle.residual_losses(crit = a - b, unit factors), the six losses from oracle.pde_criterion and both cotangents from torch.autograd.grad.
g_jxi is the cotangent of jac_n times (1 / lon_m1 / dx, 1 / lat_m1 / dy, 1 / pred_t_span), applied in fp64.  The table's constants are the fp32
values the ABI receives, as exact floats.

Inputs: physical-scale random fields (out_n ~ N(0, 1) against the shipped mean and std, Jacobian N(0, 1) (3e-6, 3e-6, 3e-5) per normalised unit,
f uniform in +-1.4e-4) behind a block of forced rows (every clipped field on both sides of its bounds, saturated and unsaturated points with omega
of either sign, q_s on its 1e-6 floor, a small in-bounds density, a squared field whose root is negative).  A point whose fp64 value comes within
GUARD_REL of a switch -- relative to the magnitude of the terms that form the compared value -- is redrawn from the case's own generator, so
that no point is ever left out of a comparison; the switches are the clip bounds, omega = 0, q = q_s, |r_e| = beta (SmoothL1) and r_e = 0 (L1).
The 'exact' table (std 1, mean 0: val = out_n exactly) carries the rows that sit ON a switch in exact arithmetic.

Bounds.  Every comparison is elementwise, bar = K 2^-24 scale, against a scale that cancellation cannot hide behind:
    residual e at point i     A_e,i: the sum of the absolute values of the products that equation adds (`term_scales`), plus the residual's
                              first-order sensitivity to the rounding of the fields' own formation (`input_condition`: val = out std + mean
                              carries u (|out std| + |mean|), unbounded relative to val where the two cancel -- v = 0, a small density)
    cotangent entry           sum over the six equations of |that equation's own autograd contribution| (six passes), the contribution of an
                              equation whose slope is proportional to r (MSE; SmoothL1 inside its kink) times A_e / |r_e|: the slope inherits
                              the residual's absolute error, not its relative one; plus the entry's sensitivity to the same rounding of the
                              fields and to the one rounding of every chained J = jac_n msk (a second autograd pass per entry: an equation's
                              contribution that adds several such products, g_3 omega / (rho + 1e-6)^2, cancels inside itself)
    block row                 sum over the block's points of wt (|rho'(r)| A + rho)
    loss                      factor / n times the sum over the points of wt ((|rho'| + c bar_r) bar_r + 3 u rho), c the curvature of rho
                              (MSE 1, SmoothL1 inside the kink 1 / (2 beta), else 0), plus the two fp32 roundings of the finish
Without the two sensitivity terms the fp32 torch evaluation itself needs K = 17 (residuals) to 2190 (g_jxi) at the handful of points where a field
cancels, and that K would loosen the bars of every other point; with them it needs 1.5 to 3.8 everywhere.  K is what the plain fp32 torch
evaluation of this same reference needs against its fp64 evaluation, one per kind, recorded in K_RECORDED; the CPU test measures it on every case
and asserts it has not grown.  The GPU test allows GPU_FACTOR x the record (the kernel contracts to fma, adds in another order and calls the
device expf).  The finish, SmoothL1 and contraction kernels have bounds from their operation counts alone.
"""
import math
from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from gemm_cases import SENTINEL, U
from oracle import dpn_oracle as O

F32 = np.float32
GUARD = 8                         # elements before and after every window (windows stay 16-byte aligned)
SENTINEL64_BITS = 0xCAFEBABECAFEBABE
SENTINEL64 = np.array([SENTINEL64_BITS], np.uint64).view(np.float64)[0]
GUARD_REL = 1e-4
GPU_FACTOR = 4.0
KPE = 192                         # kPe: encoded coordinate width of dpn_contract_gpe
C_P, L_V, R_V, R_D = 1005.0, 2.5e6, 461.5, 287.0
UNIT_FACTORS = {k: 1.0 for k in ('motion_u_factor', 'motion_v_factor', 'continuous_factor', 'energy_factor', 'vapor_factor', 'gas_factor')}
SHIPPED_FACTORS = (1e3, 1e3, 1e10, 1e1, 1e14, 1e-7)
CRIT_CODE = {'mse': 0, 'l1': 1, 'sl1': 2}
CRIT_NAME = {'mse': 'MSELoss', 'l1': 'L1Loss', 'sl1': 'WeightSmoothL1Loss'}
GEO = dict(dx=27000.0, dy=27000.0, lon_m1=256.0, lat_m1=144.0, pred_t_span=86400.0)        # every value an exact fp32
SC = (1.0 / GEO['lon_m1'] / GEO['dx'], 1.0 / GEO['lat_m1'] / GEO['dy'], 1.0 / GEO['pred_t_span'])
JAC_SCALE = (3e-6, 3e-6, 3e-5)
# largest |fp32 torch - fp64| / (2^-24 scale) over the whole case table, per kind (measured by test_residual_cases_cpu.py, rounded up)
K_RECORDED = dict(res=3.5, row=2.0, g_out=3.5, g_jxi=5.0)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------- physics tables
@dataclass(frozen=True)
class Table:
    """DpnPhysics' de-normalisation, field order (u, v, p, T, q, rho): val = out * std + mean [squared, + sq_add] [clipped]; `ident`: the value
    untouched (use_norm False: mean 0, std 1 in the ABI, never clipped)."""
    name: str
    mean: tuple
    std: tuple
    lo: tuple
    hi: tuple
    clip_on: tuple
    sq_on: tuple = (False,) * 6
    sq_add: tuple = (0.0,) * 6
    ident: tuple = (False,) * 6
    factor: tuple = SHIPPED_FACTORS

    def rounded(self):
        r = lambda t: tuple(f32(x) for x in t)
        return replace(self, mean=r(self.mean), std=r(self.std), lo=r(self.lo), hi=r(self.hi), sq_add=r(self.sq_add), factor=r(self.factor))

    def without_clip(self):
        return replace(self, clip_on=(False,) * 6)


def table_from_norm_cfg(name, cfg, with_clip=True, factor=SHIPPED_FACTORS):
    """The table oracle.inverse_norm(norm_cfg = cfg, with_clip) applies (interface.point_config's mapping)."""
    mean, std, lo, hi, clip, sq, add, ident = [], [], [], [], [], [], [], []
    for k, c in enumerate(cfg):
        nf = c['norm_factor']
        if not c['use_norm']:
            mean.append(0.0), std.append(1.0), sq.append(False), add.append(0.0), ident.append(True)
        elif c['norm_type'].lower() == 'min_max':
            mean.append(nf[0]), std.append(nf[1] - nf[0]), sq.append(len(nf) != 2), add.append(nf[2] if len(nf) != 2 else 0.0), ident.append(False)
        else:
            mean.append(nf[0]), std.append(nf[1]), sq.append(False), add.append(0.0), ident.append(False)
        lo.append(float(c['bound'][0])), hi.append(float(c['bound'][1]))
        clip.append(bool(with_clip and k >= 2 and c['use_norm']))
    return Table(name, tuple(mean), tuple(std), tuple(lo), tuple(hi), tuple(clip), tuple(sq), tuple(add), tuple(ident), tuple(factor))


def _tables():
    t = {}
    t['shipped'] = table_from_norm_cfg('shipped', O.shipped_norm_cfg())
    t['noclip'] = table_from_norm_cfg('noclip', O.shipped_norm_cfg(), with_clip=False)
    t['f12'] = table_from_norm_cfg('f12', O.f12_norm_cfg())
    t['f12sq'] = table_from_norm_cfg('f12sq', O.f12_norm_sq_cfg())
    s = t['shipped']
    # a DpnPhysics that PointConfig.physics() never builds: the squared form on a clipped field other than q (T) and on an unclipped one (u),
    # non-unit factors
    t['custom'] = replace(s, name='custom', mean=(0.5, s.mean[1], s.mean[2], 16.8, s.mean[4], s.mean[5]), std=(1.2, s.std[1], s.std[2], 0.45, s.std[4], s.std[5]),
                          sq_on=(True, False, False, True, False, False), sq_add=(-3.0, 0.0, 0.0, 1.0, 0.0, 0.0),
                          factor=(3e2, 7e3, 3e9, 0.7, 3e13, 5e-7))
    # val = out_n exactly: the rows that sit on a switch
    t['exact'] = replace(s, name='exact', mean=(0.0,) * 6, std=(1.0,) * 6)
    return {k: v.rounded() for k, v in t.items()}


TABLES = _tables()


def denorm(fields, table):
    """oracle.inverse_norm line for line over a Table."""
    out = []
    for k, v in enumerate(fields):
        if not table.ident[k]:
            v = v * table.std[k] + table.mean[k]
            if table.sq_on[k]:
                v = v ** 2
                v = v + table.sq_add[k]
            if table.clip_on[k]:
                v = torch.clip(v, table.lo[k], table.hi[k])
        out.append(v)
    return tuple(out)


def _denorm_mistaken(parts, table, mistake):
    """denorm over (A_k, B_k . coords) pairs with one seeded mistake of the squared form."""
    out = []
    for k, (a, bx) in enumerate(parts):
        if table.ident[k]:
            out.append(a + bx)
            continue
        if table.sq_on[k] and mistake == 'sq_correction_dropped':        # the chained Jacobian 2 (A std + mean) std B loses its dependence on A
            va = a * table.std[k] + table.mean[k]
            v = va ** 2 + 2.0 * va.detach() * table.std[k] * bx + table.sq_add[k]
            lin = va
        else:
            lin = (a + bx) * table.std[k] + table.mean[k]
            v = lin ** 2 + table.sq_add[k] if table.sq_on[k] else lin
        if table.clip_on[k]:
            v = torch.clip(v, table.lo[k], table.hi[k])
            if table.sq_on[k] and mistake == 'clip_mask_before_square':
                inside = (lin >= table.lo[k]) & (lin <= table.hi[k])
                v = torch.where(inside, v, v.detach())
        out.append(v)
    return tuple(out)


def inverse_table(table, k, phys):
    """out_n that de-normalises to the physical value `phys` (fp64; the positive root of a squared form)."""
    if table.ident[k]:
        return phys
    if table.sq_on[k]:                                            # a value the squared form cannot reach: a small root instead (inside the bounds)
        phys = np.sqrt(np.maximum(phys - table.sq_add[k], 1e-4))
    return (phys - table.mean[k]) / table.std[k]


def dval_dout(table, k, out):
    if table.ident[k]:
        return np.ones_like(out)
    lin = out * table.std[k] + table.mean[k]
    return 2.0 * lin * table.std[k] if table.sq_on[k] else np.full_like(out, table.std[k])


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                     # 'points' | 'residual' | 'weighted' | 'step'
    table: str
    n: int
    crit: str = 'mse'
    reduce_sum: bool = False
    beta_eq: int = -1             # SmoothL1: the equation whose median |r| is beta
    up: str = 'none'              # upstream weights: 'none' | 'gl' | 'gtot' | 'both'
    out: str = 'both'             # 'both' | 'loss' | 'cot'
    weights: str = ''             # weighted: 'w' | 'bin' | 'both'
    n_inter: int = 0              # step: interior rows (n = all rows)
    B: int = 1                    # step: fields


POINT_N = (1, 63, 64, 65, 255, 256, 257, 1037)
RES_N = (1, 255, 257, 1037)
STEP_SPLITS = ((1, 1), (255, 257), (256, 1), (300, 513))


def _cases():
    c = []
    for tb in ('shipped', 'noclip', 'f12', 'f12sq'):
        for n in POINT_N:
            c.append(Case('points_%s_%d' % (tb, n), 'points', tb, n))
    c.append(Case('points_exact', 'points', 'exact', 0))
    # dpn_residual: every value of every axis at n = 257
    for crit, red in (('mse', False), ('mse', True), ('l1', False), ('l1', True)):
        for i, tb in enumerate(('shipped', 'noclip', 'f12', 'f12sq', 'custom')):
            c.append(Case('res_%s_%s%s_257' % (tb, crit, '_sum' if red else ''), 'residual', tb, 257, crit=crit, reduce_sum=red,
                          up=('none', 'gl', 'gtot', 'both')[(i + (crit == 'l1') + 2 * red) % 4]))
    for e in range(6):
        c.append(Case('res_%s_sl1_eq%d_257' % (('shipped', 'custom', 'f12sq')[e % 3], e), 'residual', ('shipped', 'custom', 'f12sq')[e % 3], 257,
                      crit='sl1', beta_eq=e, up=('both', 'none', 'gl', 'gtot')[e % 4]))
    for up in ('none', 'gl', 'gtot', 'both'):
        for out in ('loss', 'cot'):
            c.append(Case('res_custom_mse_%s_%s_257' % (up, out), 'residual', 'custom', 257, up=up, out=out))
    for n in RES_N:
        c.append(Case('res_shipped_mse_%d' % n, 'residual', 'shipped', n, up='both'))
    c.append(Case('res_exact_mse', 'residual', 'exact', 0, up='gl'))
    c.append(Case('res_exact_l1', 'residual', 'exact', 0, crit='l1', up='gtot'))
    c.append(Case('res_exact_sl1', 'residual', 'exact', 0, crit='sl1', beta_eq=3))
    # dpn_residual_weighted
    for wk in ('w', 'bin', 'both'):
        for n in (257, 1037):
            c.append(Case('wt_%s_mse_%d' % (wk, n), 'weighted', 'shipped', n, weights=wk, up='both' if n == 257 else 'none'))
            c.append(Case('wt_%s_sl1_%d' % (wk, n), 'weighted', 'custom' if n == 257 else 'shipped', n, crit='sl1', beta_eq=3, weights=wk, up='gtot'))
    # dpn_step_residual + dpn_step_finish_batch
    for ni, nm in STEP_SPLITS:
        for B in (1, 3):
            c.append(Case('step_%d_%d_B%d' % (ni, nm, B), 'step', 'shipped', ni + nm, n_inter=ni, B=B, up='gtot',
                          crit='sl1' if (ni, nm) == (255, 257) else 'mse', beta_eq=0 if (ni, nm) == (255, 257) else -1))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def cases_of(*kinds):
    return [c.name for c in CASES if c.kind in kinds]


# ---------------------------------------------------------------------------------------------- inputs
@dataclass
class Inputs:
    """One launch's logical fp32 arguments."""
    table: Table
    crit: str
    beta: float
    reduce_sum: bool
    out_n: np.ndarray             # [n][6]
    jac_n: np.ndarray             # [n][6][3]
    f: np.ndarray                 # [n]
    gl: np.ndarray = None         # [6]
    gtot: np.ndarray = None       # [1]
    w: np.ndarray = None          # [n]
    bin: np.ndarray = None        # [n] int32
    bin_w: np.ndarray = None
    exact: bool = False

    @property
    def n(self):
        return len(self.f)

    def wt(self):
        """The point weight w[i] * bin_w[bin[i]] as the kernel forms it: one fp32 product."""
        if self.w is None and self.bin is None:
            return None
        a = self.w if self.w is not None else np.ones(self.n, F32)
        b = self.bin_w[self.bin] if self.bin is not None else np.ones(self.n, F32)
        return (a * b).astype(F32)

    def rows(self, sl):
        pick = lambda a: None if a is None else a[sl]
        return replace(self, out_n=self.out_n[sl], jac_n=self.jac_n[sl], f=self.f[sl], w=pick(self.w), bin=pick(self.bin))


def _forced_rows(table):
    """(physical targets {field: value}, Jacobian override {(k, c): value per normalised unit}) per forced row."""
    rows = []
    for k, lo, hi in ((2, 5000.0, 6e5), (3, 40.0, 510.0), (4, -1e-3, 11.0), (5, -0.1, 11.0)):       # below / above the bounds: mask 0 where clipped
        rows += [({k: lo}, {}), ({k: hi}, {})]
    for q in (0.03, 1e-3):                                                                        # saturated / unsaturated at T = 283.58, p = 89741
        for sign in (-1.0, 1.0):
            rows.append(({2: 89741.0, 3: 283.58, 4: q}, {(2, 0): 0.0, (2, 1): 0.0, (2, 2): sign * 1.5e-4}))
    rows.append(({2: 89741.0, 3: 150.0, 4: 2e-3}, {(2, 0): 0.0, (2, 1): 0.0, (2, 2): -1.5e-4}))   # q_s on its 1e-6 floor, saturated, omega < 0
    rows.append(({5: 0.02}, {}))                                                                  # 1 / rho against 1 / (rho + 1e-6)
    rows.append(({5: 0.05, 0: 4.0, 1: -3.0}, {}))
    if table.name == 'f12sq':                                                                     # a squared field with a negative root (out_n given
        rows.append(({-4: -4.0}, {}))                                                             # as it is): inside the bounds after squaring only
    return rows


def _draw(rng, table, n_rand, forced):
    n = len(forced) + n_rand
    out = rng.standard_normal((n, 6))
    for k in range(6):                                            # N(0, 1) against the shipped mean and std, through this table's own form
        if not table.sq_on[k] and (table.ident[k] or (table.mean[k], table.std[k]) != (f32(O.OBS_MEAN[k]), f32(O.OBS_STD[k]))):
            out[:, k] = inverse_table(table, k, out[:, k] * O.OBS_STD[k] + O.OBS_MEAN[k])
    for i, (tgt, _) in enumerate(forced):
        for k, val in tgt.items():                                # a negative key: out_n[-k] itself
            out[i, abs(k)] = inverse_table(table, k, np.float64(val)) if k >= 0 else val
    out = out.astype(F32)
    jac = rng.standard_normal((n, 6, 3)) * np.array(JAC_SCALE)
    for i, (_, jo) in enumerate(forced):
        for (k, c), val in jo.items():
            jac[i, k, c] = val
    for k in range(6):                                            # the physical Jacobian keeps the shipped scale whatever the table's form
        jac[:, k, :] *= (O.OBS_STD[k] / np.abs(dval_dout(table, k, out[:, k].astype(np.float64))))[:, None]
    f = rng.uniform(-1.4e-4, 1.4e-4, size=n)
    return out, jac.astype(F32), f.astype(F32)


def _exact_rows():
    """val = out_n: rows that sit ON a switch, every number an exact fp32."""
    lo, hi = TABLES['exact'].lo, TABLES['exact'].hi
    base = np.array([2.0, -1.5, 90000.0, 283.5, 0.0078125, 1.125])
    jbase = np.array([[2.0 ** -18, -2.0 ** -19, 2.0 ** -15]] * 6) * np.array([3.0, 3.0, 8192.0, 16.0, 2.0 ** -7, 0.125])[:, None]
    out, jac, f = [], [], []
    for k in (2, 3, 4, 5):
        for b in (lo[k], hi[k]):                                  # v == clip_lo, v == clip_hi: mask 1
            o = base.copy(); o[k] = b
            out.append(o); jac.append(jbase.copy()); f.append(2.0 ** -13)
    for q in (0.03125, 0.0009765625):                             # omega == 0 exactly: a zero pressure row, and p_t = -u p_x
        j = jbase.copy(); j[2] = 0.0
        o = base.copy(); o[4] = q
        out.append(o); jac.append(j); f.append(-2.0 ** -13)
        j = jbase.copy(); j[2] = (0.5, 0.0, -1.0)
        out.append(o.copy()); jac.append(j); f.append(2.0 ** -14)
    o = base.copy(); o[5] = 2.0 ** -6                             # a small density free of rounding: 1 / rho against 1 / (rho + 1e-6) is 1000 u here
    out.append(o); jac.append(jbase.copy()); f.append(2.0 ** -13)
    for q in (0.03125, 0.0009765625):                             # all-zero Jacobian, f = 0: five residuals exactly 0
        o = base.copy(); o[4] = q
        out.append(o); jac.append(np.zeros((6, 3))); f.append(0.0)
    out, jac, f = np.array(out), np.array(jac), np.array(f)
    assert (out.astype(F32) == out).all() and (jac.astype(F32) == jac).all()
    return out.astype(F32), jac.astype(F32), f.astype(F32)


N_EXACT_ZERO = 2                  # the trailing all-zero-Jacobian rows of the 'exact' inputs
EXACT_SMALL_RHO_ROW = 12           # rho = 2^-6


def _upstream(rng, up):
    gl = rng.uniform(0.3, 2.7, size=6).astype(F32) if up in ('gl', 'both') else None
    gtot = rng.uniform(0.3, 2.7, size=1).astype(F32) if up in ('gtot', 'both') else None
    return gl, gtot


def build(case):
    """Inputs of a case: drawn, beta set from the first draw's fp64 median, then every point inside a guard band redrawn."""
    rng = np.random.default_rng([sum(map(ord, case.name)), case.n, len(case.name)])
    table = TABLES[case.table]
    gl, gtot = _upstream(rng, case.up)
    if case.table == 'exact':
        out, jac, f = _exact_rows()
        inp = Inputs(table, case.crit, 0.0, case.reduce_sum, out, jac, f, gl, gtot, exact=True)
        if case.crit == 'sl1':
            inp.beta = f32(np.median(np.abs(evaluate(inp, scales=False).r[:, case.beta_eq])))
        return inp
    forced = _forced_rows(table) if case.n >= 63 else []
    out, jac, f = _draw(rng, table, case.n - len(forced), forced)
    inp = Inputs(table, case.crit, 0.0, case.reduce_sum, out, jac, f, gl, gtot)
    n = case.n
    if case.weights in ('w', 'both'):
        inp.w = (10.0 ** rng.uniform(-1.0, 1.0, size=n)).astype(F32)
    if case.weights in ('bin', 'both'):
        inp.bin, inp.bin_w = rng.integers(0, 7, size=n).astype(np.int32), rng.uniform(0.05, 1.0, size=7).astype(F32)
    if case.crit == 'sl1':
        inp.beta = f32(np.median(np.abs(evaluate(inp, scales=False).r[:, case.beta_eq])))
    for _ in range(40):
        bad = np.flatnonzero(guard_violations(inp, evaluate(inp, scales=False)))
        if not len(bad):
            return inp
        for i in bad:                                             # the forced values of a forced row stay, everything drawn is drawn again
            o, j, ff = _draw(rng, table, 0 if i < len(forced) else 1, [forced[i]] if i < len(forced) else [])
            inp.out_n[i], inp.jac_n[i], inp.f[i] = o[0], j[0], ff[0]
    raise AssertionError('%s: points inside a guard band after 40 redraws' % case.name)


# ---------------------------------------------------------------------------------------------- the fp64 reference
@dataclass
class Eval:
    pre: np.ndarray               # [n][6] de-normalised, before the clip
    val: np.ndarray               # [n][6]
    J: np.ndarray                 # [n][6][3] chained Jacobian d val / d (x, y, t)
    r: np.ndarray                 # [n][6] signed residuals, unscaled
    omega: np.ndarray
    q_s: np.ndarray
    delta: np.ndarray
    Fv: np.ndarray
    losses: np.ndarray = None     # [6] scaled
    total: float = 0.0            # their sum, the reference's order of additions
    g_out: np.ndarray = None      # [n][6]
    g_jxi: np.ndarray = None      # [n][6][3]
    cA: np.ndarray = None         # [6][n][6]: equation e's own contribution to g_out
    cB: np.ndarray = None         # [6][n][6][3]: to g_jxi
    head: np.ndarray = None       # [n][6] d total / d r_e
    dvdo: np.ndarray = None       # [n][6] d val / d out_n
    cond_res: np.ndarray = None   # [n][6], [n][6], [n][6][3]: |d output / d out_n| . input_condition (evaluate(cond = True))
    cond_out: np.ndarray = None
    cond_jxi: np.ndarray = None


def rho_elem(r, crit, beta):
    if crit == 'mse':
        return r ** 2
    if crit == 'l1':
        return torch.abs(r)
    return F.smooth_l1_loss(r, torch.zeros_like(r), beta=beta, reduction='none')


def input_condition(table, out_n):
    """[n][6]: the perturbation of out_n[k] (in units of 2^-24) that stands for the rounding of val[k]'s own formation: val = out std + mean has
    the absolute error u (|out std| + |mean|) -- a relative error that grows without bound where the two cancel (v = 0, a small density) and that
    every residual and cotangent reading val inherits; the squared form adds the rounding of lin^2 + sq_add.  0 for an untouched field."""
    o = np.asarray(out_n, np.float64)
    d = np.zeros_like(o)
    for k in range(6):
        if table.ident[k]:
            continue
        lin_mag = np.abs(o[:, k] * table.std[k]) + abs(table.mean[k])
        d[:, k] = lin_mag / abs(table.std[k])
        if table.sq_on[k]:
            lin = o[:, k] * table.std[k] + table.mean[k]
            with np.errstate(divide='ignore'):
                d[:, k] += (lin * lin + abs(table.sq_add[k])) / (2 * np.abs(lin) * abs(table.std[k]))
    return d


def evaluate(inp, dtype=torch.float64, mistake=None, scales=True, cond=False):
    """The reference in `dtype` (fp64: the reference; fp32: the evaluation K is measured on).  scales = False stops after the residuals and the
    switch quantities; cond adds the sensitivities `reference` puts into the scales."""
    tb, n = inp.table, inp.n
    np64 = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dtype)
    A, Bj = np64(inp.out_n).requires_grad_(True), np64(inp.jac_n).requires_grad_(True)
    f = np64(inp.f)[:, None]
    x, y, t = (torch.zeros(n, 1, dtype=dtype, requires_grad=True) for _ in range(3))
    parts = [(A[:, k:k + 1], Bj[:, k, 0:1] * x + Bj[:, k, 1:2] * y + Bj[:, k, 2:3] * t) for k in range(6)]
    if mistake in ('sq_correction_dropped', 'clip_mask_before_square'):
        fields = _denorm_mistaken(parts, tb, mistake)
    else:
        fields = denorm([a + bx for a, bx in parts], tb)
    pre = torch.cat(denorm([a.detach() for a, _ in parts], tb.without_clip()), 1)
    r = O.residual_losses(x, y, t, f, *fields, factors=UNIT_FACTORS, crit=lambda a, b: a - b)
    J = O.jacobian_fields(x, y, t, fields).detach()
    u, v, p, T, q, rho = (z.detach() for z in fields)
    # the switch quantities, in the oracle's own expressions and order (residual_losses keeps them to itself)
    omega = J[:, 2, 2:3] + u * J[:, 2, 0:1] + v * J[:, 2, 1:2]
    tc = T - 273.15
    e_s = 6.112 * torch.exp(17.67 * tc / (tc + 243.5)) * 100
    q_s = 0.622 * e_s / (p - 0.378 * e_s)
    q_s = torch.maximum(q_s, torch.ones_like(q_s) * 1e-6)
    delta = torch.logical_and(omega < 0, torch.ge(q, q_s)).to(dtype)
    Fv = ((L_V * (1 + 0.608 * q) * R_D - C_P * R_V * T) / (C_P * R_V + T * T + L_V * L_V * q_s)) * q_s * T
    host = lambda z: z.detach().to(torch.float64).numpy()
    ev = Eval(pre=host(pre), val=host(torch.cat(fields, 1)), J=host(J), r=host(torch.cat(r, 1)), omega=host(omega)[:, 0], q_s=host(q_s)[:, 0],
              delta=host(delta)[:, 0], Fv=host(Fv)[:, 0])
    if not scales:
        return ev
    wt = inp.wt()
    losses = []
    for e in range(6):
        if wt is None:
            crit = O.pde_criterion(CRIT_NAME[inp.crit], beta=inp.beta, reduction='sum' if inp.reduce_sum else 'mean')
            losses.append(crit(r[e], torch.zeros_like(r[e])) * tb.factor[e])
        else:
            losses.append((np64(wt)[:, None] * rho_elem(r[e], inp.crit, inp.beta)).sum() / (1.0 if inp.reduce_sum else float(n)) * tb.factor[e])
    if inp.gl is None and inp.gtot is None:
        up = [1.0] * 6
    else:
        up = [(float(inp.gl[e]) if inp.gl is not None else 0.0) + (float(inp.gtot[0]) if inp.gtot is not None else 0.0) for e in range(6)]
    total = sum(up[e] * losses[e] for e in range(6))
    cA, cB = [], []
    for e in range(6):
        ga, gb = torch.autograd.grad(up[e] * losses[e], [A, Bj], retain_graph=True, allow_unused=True)
        cA.append(host(ga) if ga is not None else np.zeros((n, 6)))
        cB.append(host(gb) if gb is not None else np.zeros((n, 6, 3)))
    ga, gb = torch.autograd.grad(total, [A, Bj], retain_graph=True, create_graph=cond)
    if cond:                                                      # first-order sensitivity of every output to the rounding of the fields' formation
        dA = torch.from_numpy(input_condition(tb, inp.out_n))


        def sens(y, jac=True):
            """sum_k |dy / d out_n[k]| dA[k] (+ sum_kc |dy / d jac_n[k][c]| |jac_n[k][c]|: the one rounding of every chained J = jac_n msk, which a
            cotangent entry that adds several such products -- g_3 omega / (rho + 1e-6)^2 -- inherits term by term)"""
            if not y.requires_grad:
                return np.zeros(n)
            sa, sb = torch.autograd.grad(y.sum(), [A, Bj], retain_graph=True, allow_unused=True)
            out = (sa.abs() * dA).sum(1) if sa is not None else torch.zeros(n, dtype=dtype)
            if jac and sb is not None:
                out = out + (sb.abs() * Bj.detach().abs()).sum((1, 2))
            return out.numpy()
        ev.cond_res = np.stack([sens(r[e], jac=False) for e in range(6)], 1)          # term_scales holds the residuals' own products
        ev.cond_out = np.stack([sens(ga[:, k]) for k in range(6)], 1)
        ev.cond_jxi = np.stack([np.stack([sens(gb[:, k, c]) for c in range(3)], 1) for k in range(6)], 1) * np.array(SC)
        ga, gb = ga.detach(), gb.detach()
    head = torch.autograd.grad(total, list(r), retain_graph=True)
    dv = torch.autograd.grad(torch.cat(fields, 1).sum(), A)[0]
    ev.losses = np.array([float(l.detach()) for l in losses])
    mu, mv, co, en, va, ga_ = ev.losses
    ev.total = mu + mv + en + co + va + ga_
    ev.g_out, ev.g_jxi = host(ga), host(gb) * np.array(SC)
    ev.cA, ev.cB = np.array(cA), np.array(cB) * np.array(SC)
    ev.head, ev.dvdo = host(torch.cat(head, 1)), host(dv)
    if mistake == 'gv4_sign':                                     # + instead of - on the 0.608 R_d T term of d r_5 / d q
        ev.g_out[:, 4] += 2.0 * ev.head[:, 5] * ev.val[:, 5] * 0.608 * R_D * ev.val[:, 3] * ev.dvdo[:, 4]
    elif mistake == 'gJ2_without_eps':                            # 1 / rho where the energy equation has 1 / (rho + 1e-6)
        d = 1.0 / ev.val[:, 5] - 1.0 / (ev.val[:, 5] + 1e-6)
        coef = np.stack([ev.val[:, 0], ev.val[:, 1], np.ones(n)], 1)
        ev.g_jxi[:, 2, :] += (-ev.head[:, 3] * d * ev.dvdo[:, 2])[:, None] * coef * np.array(SC)
    elif mistake == 'slope_without_beta':                         # SmoothL1 inside the kink: r instead of r / beta
        m = np.where(np.abs(ev.r) < inp.beta, inp.beta, 1.0).T
        ev.g_out, ev.g_jxi = (ev.cA * m[:, :, None]).sum(0), (ev.cB * m[:, :, None, None]).sum(0)
    return ev


MISTAKES = ('gv4_sign', 'sq_correction_dropped', 'gJ2_without_eps', 'clip_mask_before_square', 'slope_without_beta')


def term_scales(ev, f):
    """A_e,i: per equation the sum of the absolute values of the products it adds, from the reference's fields and chained Jacobian."""
    a = np.abs
    u, v, p, T, q, rho = ev.val.T
    J = ev.J
    adv = lambda k: a(J[:, k, 2]) + a(u * J[:, k, 0]) + a(v * J[:, k, 1])
    A0 = adv(0) + a(J[:, 2, 0] / rho) + a(f * v)
    A1 = adv(1) + a(J[:, 2, 1] / rho) + a(f * u)
    A2 = adv(5) + a(rho * J[:, 0, 0]) + a(rho * J[:, 1, 1])
    A3 = C_P * adv(3) + adv(2) / a(rho + 1e-6) + L_V * adv(4)
    A4 = adv(2) * ev.delta * a(ev.Fv) / a(p + 1e-6) + adv(4)
    A5 = a(p) + a(rho * (1 + 0.608 * q) * R_D * T)
    return np.stack([A0, A1, A2, A3, A4, A5], 1)


def sides(inp, ev):
    """The side of every switch each point takes: [n][14] = 6 clip sides (-1 below, 0 inside, +1 above), omega < 0, q >= q_s, 6 criterion sides."""
    tb = inp.table
    s = np.zeros((inp.n, 14), np.int8)
    for k in range(6):
        if tb.clip_on[k]:
            s[:, k] = (ev.pre[:, k] > tb.hi[k]).astype(np.int8) - (ev.pre[:, k] < tb.lo[k]).astype(np.int8)
    s[:, 6], s[:, 7] = ev.omega < 0, ev.val[:, 4] >= ev.q_s
    if inp.crit == 'sl1':
        s[:, 8:] = np.abs(ev.r) < inp.beta
    elif inp.crit == 'l1':
        s[:, 8:] = np.sign(ev.r)
    return s


def guard_violations(inp, ev):
    """[n] bool: the point's fp64 value lies within GUARD_REL of a switch, relative to the magnitude of the terms that form the compared value."""
    tb = inp.table
    o = inp.out_n.astype(np.float64)
    bad = np.zeros(inp.n, bool)
    for k in range(6):
        if tb.clip_on[k]:
            lin = np.abs(o[:, k] * tb.std[k]) + abs(tb.mean[k])
            mag = lin * lin + abs(tb.sq_add[k]) if tb.sq_on[k] else lin
            for b in (tb.lo[k], tb.hi[k]):
                bad |= np.abs(ev.pre[:, k] - b) < GUARD_REL * (mag + abs(b))
    u, v = ev.val[:, 0], ev.val[:, 1]
    bad |= np.abs(ev.omega) < GUARD_REL * (np.abs(ev.J[:, 2, 2]) + np.abs(u * ev.J[:, 2, 0]) + np.abs(v * ev.J[:, 2, 1]))
    qmag = np.abs(o[:, 4] * tb.std[4]) + abs(tb.mean[4])
    bad |= np.abs(ev.val[:, 4] - ev.q_s) < GUARD_REL * (qmag + np.abs(ev.q_s))
    A = term_scales(ev, inp.f.astype(np.float64))
    if inp.crit == 'sl1':
        bad |= (np.abs(np.abs(ev.r) - inp.beta) < GUARD_REL * A).any(1)
    elif inp.crit == 'l1':
        bad |= (np.abs(ev.r) < GUARD_REL * A).any(1)
    return bad


# ---------------------------------------------------------------------------------------------- scales and bars
def rho_parts(inp, r):
    """(rho, |rho'|, curvature c, slope proportional to r) per element, fp64."""
    ar = np.abs(r)
    if inp.crit == 'mse':
        return r * r, 2 * ar, np.ones_like(r), np.ones_like(r, bool)
    if inp.crit == 'l1':
        return ar, np.ones_like(r) * (ar > 0), np.zeros_like(r), np.zeros_like(r, bool)
    quad = ar < inp.beta
    return np.where(quad, 0.5 * r * r / inp.beta, ar - 0.5 * inp.beta), np.where(quad, ar / inp.beta, 1.0), np.where(quad, 0.5 / inp.beta, 0.0), quad


def blocks(n):
    return (n + 255) // 256


def block_sums(x):
    """[n][c] -> [ceil(n / 256)][c], math.fsum per block."""
    n = len(x)
    return np.array([[math.fsum(x[b * 256:min(n, b * 256 + 256), c]) for c in range(x.shape[1])] for b in range(blocks(n))])


@dataclass
class Ref:
    ev: Eval
    A: np.ndarray                 # residual scales [n][6]
    rows: np.ndarray              # block rows [nblk][6]
    row_scale: np.ndarray
    g_out_scale: np.ndarray
    g_jxi_scale: np.ndarray
    wt: np.ndarray


def reference(inp):
    ev = evaluate(inp, cond=True)
    A = term_scales(ev, inp.f.astype(np.float64)) + ev.cond_res
    rho, slope, _, prop = rho_parts(inp, ev.r)
    wt = inp.wt()
    wt = np.ones(inp.n) if wt is None else wt.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        amp = np.where(prop, np.where(ev.r != 0, A / np.abs(ev.r), 0.0), 1.0).T          # [6][n]
    return Ref(ev, A, block_sums(wt[:, None] * rho), block_sums(wt[:, None] * (slope * A + rho)),
               (np.abs(ev.cA) * amp[:, :, None]).sum(0) + ev.cond_out, (np.abs(ev.cB) * amp[:, :, None, None]).sum(0) + ev.cond_jxi, wt)


def loss_bars(inp, ref, K_res):
    """[6] bars of the finished losses and the bar of their fp32 total."""
    rho, slope, curv, _ = rho_parts(inp, ref.ev.r)
    bar_r = K_res * U * ref.A
    per = ref.wt[:, None] * ((slope + curv * bar_r) * bar_r + 3 * U * rho)
    div = 1.0 if inp.reduce_sum else float(inp.n)
    fac = np.array(inp.table.factor)
    bars = np.array([math.fsum(per[:, e]) for e in range(6)]) * fac / div + 2.01 * U * np.abs(ref.ev.losses)
    return bars, float(bars.sum() + 5.01 * U * np.abs(ref.ev.losses).sum())


def ratio(err, scale):
    """max |err| / (2^-24 scale); 0 / 0 counts as 0, a nonzero or non-finite error over a zero scale as inf."""
    err, scale = np.abs(np.asarray(err, np.float64)), np.asarray(scale, np.float64) * U
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where((err == 0) & (scale >= 0), 0.0, err / scale)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


def measure(inp, ref, got):
    """Largest error / (2^-24 scale) per kind.  got: dict with any of res [n][6], rows [nblk][6], g_out, g_jxi."""
    out = {}
    if got.get('res') is not None:
        out['res'] = ratio(got['res'] - ref.ev.r, ref.A)
    if got.get('rows') is not None:
        out['row'] = ratio(got['rows'] - ref.rows, ref.row_scale)
    if got.get('g_out') is not None:
        out['g_out'] = ratio(got['g_out'] - ref.ev.g_out, ref.g_out_scale)
    if got.get('g_jxi') is not None:
        out['g_jxi'] = ratio(got['g_jxi'] - ref.ev.g_jxi, ref.g_jxi_scale)
    return out


def fp32_outputs(inp, mistake=None, dtype=torch.float32):
    """The reference evaluated in `dtype`, in the shape `measure` takes (block rows summed in fp64 from the evaluation's own rho)."""
    ev = evaluate(inp, dtype=dtype, mistake=mistake)
    rho = rho_parts(inp, ev.r)[0]
    wt = inp.wt()
    wt = np.ones(inp.n) if wt is None else wt.astype(np.float64)
    return dict(res=ev.r, rows=block_sums(wt[:, None] * rho), g_out=ev.g_out, g_jxi=ev.g_jxi, ev=ev)


@lru_cache(maxsize=None)
def built(name):
    """(inputs, reference) of a residual / points / weighted case, computed once and shared: nobody writes into either."""
    inp = build(case_by_name(name))
    return inp, reference(inp)


# ---------------------------------------------------------------------------------------------- the step body
@dataclass
class StepRef:
    groups: tuple                 # (interior Ref, margin Ref)
    data_rows: np.ndarray         # [nb_m] column 6 of the margin rows
    data_row_bar: np.ndarray
    data: float                   # mean SmoothL1 * margin_factor
    data_bar: float
    g_data: np.ndarray            # [n_m][6] data cotangent
    g_data_bar: np.ndarray


STEP_BETA, MARGIN_FACTOR = f32(0.1), f32(1e6)


def smooth_l1_reference(out_n, labels, beta):
    """fp64 F.smooth_l1_loss elementwise and its autograd slope; the fp32 bar of an element: the rounded difference, then at most four operations."""
    o = torch.from_numpy(np.asarray(out_n, np.float64)).requires_grad_(True)
    l = F.smooth_l1_loss(o, torch.from_numpy(np.asarray(labels, np.float64)), beta=beta, reduction='none')
    slope = torch.autograd.grad(l.sum(), o)[0].numpy()
    l = l.detach().numpy()
    d = np.abs(np.asarray(out_n, np.float64) - np.asarray(labels, np.float64))
    return l, slope, 5 * U * l + 2 * U * U * np.maximum(d, beta)


@lru_cache(maxsize=None)
def built_step(name, b):
    """Field b of a step case: (inputs of all rows, labels [n_m][6], StepRef)."""
    case = case_by_name(name)
    inp = build(replace(case, name='%s_field%d' % (case.name, b)))
    rng = np.random.default_rng([b, case.n, 99])
    ni = case.n_inter
    labels = (inp.out_n[ni:].astype(np.float64) + rng.uniform(-0.3, 0.3, size=(case.n - ni, 6))).astype(F32)
    gi, gm = inp.rows(slice(0, ni)), inp.rows(slice(ni, None))
    refs = (reference(gi), reference(gm))
    n_m = case.n - ni
    l, slope, bar = smooth_l1_reference(gm.out_n, labels, STEP_BETA)
    per = np.stack([l.sum(1), bar.sum(1)], 1)
    bs = block_sums(per)
    data = math.fsum(l.ravel()) / (6.0 * n_m) * MARGIN_FACTOR
    scale = f32(MARGIN_FACTOR / (6.0 * n_m)) * float(inp.gtot[0])
    g_data = scale * slope
    return inp, labels, StepRef(refs, bs[:, 0], bs[:, 1] + 300 * 2.0 ** -53 * bs[:, 0], data,
                                float(bar.sum()) / (6.0 * n_m) * MARGIN_FACTOR + 2.01 * U * data, g_data, 5 * U * np.abs(g_data))


# ---------------------------------------------------------------------------------------------- the finish kernels on given rows
FINISH_BLOCKS, FINISH_FIELDS = (1, 63, 64, 65, 129), (1, 3)


def finish_rows(nblk, n_fields, cols=6):
    """Synthetic fp64 block rows, column e around 10^(-20 + 8 e): 1e-20 .. 1e+20 over the six equations (a seventh column around 1e3)."""
    rng = np.random.default_rng([nblk, n_fields, cols])
    mag = 10.0 ** np.array([-20.0, -12.0, -4.0, 4.0, 12.0, 20.0, 3.0][:cols])
    return rng.uniform(0.25, 4.0, size=(n_fields, nblk, cols)) * mag


def finish_reference(rows, n, factor, reduce_sum):
    """rows [nblk][6] -> (six losses, their bars, total, its bar): math.fsum, the mean rounded to fp32, times the factor, rounded; the bar is nblk
    fp64 additions and the two fp32 roundings, the total's five more fp32 additions of positive terms."""
    nblk = len(rows)
    l = np.array([math.fsum(rows[:, e]) / (1.0 if reduce_sum else float(n)) * factor[e] for e in range(6)])
    bars = np.abs(l) * (2 * U + U * U + (nblk + 2) * 2.0 ** -53)
    mu, mv, co, en, va, ga = l
    return l, bars, mu + mv + en + co + va + ga, float(bars.sum() + 5.01 * U * np.abs(l).sum())


def total_in_order(l):
    """((((l0 + l1) + l3) + l2) + l4) + l5 in fp32: the reference's order of additions over the kernel's own six terms."""
    l = np.asarray(l, F32)
    return F32(F32(F32(F32(F32(l[0] + l[1]) + l[3]) + l[2]) + l[4]) + l[5])


# ---------------------------------------------------------------------------------------------- placement
class Arena:
    """One owned buffer holding a window per named array: [GUARD][values .. padded to a multiple of 4][GUARD] ..., `fill` everywhere outside the
    windows (SENTINEL where the kernel writes, NaN around what it only reads)."""

    def __init__(self, dtype, fill, items):
        self.dtype, self.offsets, self.shapes, cur = np.dtype(dtype), {}, {}, 0
        for k, x in items.items():
            x = np.asarray(x)
            self.offsets[k], self.shapes[k] = cur + GUARD, x.shape
            cur += GUARD + ((x.size + 3) // 4) * 4
        self.full = np.full(cur + GUARD, fill, self.dtype)
        self.inside = np.zeros(cur + GUARD, bool)
        for k, x in items.items():
            x = np.asarray(x)
            o = self.offsets[k]
            self.full[o:o + x.size] = x.ravel()
            self.inside[o:o + x.size] = True

    def byte_offset(self, k):
        return self.offsets[k] * self.dtype.itemsize

    def window(self, full, k):
        o, shape = self.offsets[k], self.shapes[k]
        return np.asarray(full)[o:o + int(np.prod(shape, dtype=np.int64))].reshape(shape).copy()

    def _bits(self, a):
        return np.ascontiguousarray(a, self.dtype).view({4: np.uint32, 8: np.uint64}[self.dtype.itemsize])

    def outside_kept(self, full_after):
        return bool((self._bits(full_after)[~self.inside] == self._bits(self.full)[~self.inside]).all())

    def untouched(self, full_after):
        return bool((self._bits(full_after) == self._bits(self.full)).all())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
