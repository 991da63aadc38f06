"""Case table, fp64 reference, bounds and fp32 model for clip + Adam with PARAMETER GROUPS (dpn_clip_adam_flat_groups; kernels
dpn_gradnorm_kernel<AdamFlatPlain>, dpn_gradnorm_reduce_kernel, dpn_adam_kernel<AdamFlat<false / true, true, false>>).  Imports without
a GPU: tests/test_group_optim_cases_cpu.py runs the table through the numpy fp32 model below, tests/test_gpu_group_optim.py through the C ABI.

The definition is the one in the header of tests/optim_cases.py with the hyper-parameters of tensor i taken from the row of its group k(i),
rows = [lr, b1, b2, eps, wd] per group; the sum of squares S, the norm, max_norm, grad_scale and therefore the clip coefficient are GLOBAL (all
tensors of all groups, as clip_grad_norm_ over every trainable parameter), t is the one shared step counter:
    S = sum over ALL tensors of g^2          norm = sqrt(S) gs          coef = min(max_norm / (norm + float32(1e-6)), 1) gs
    g' = wd_k p + g coef                     m' = b1_k m + (1 - b1_k) g'                 v' = b2_k v + (1 - b2_k) g'^2
    p' = p - (lr_k / (1 - b1_k^t)) m' / (sqrt(v') / sqrt(1 - b2_k^t) + eps_k)
    s' = d s + (1 - d) p'                    (the weight EMA of tests/ema_cases.py, d global)
So tensor i of the grouped step IS tensor i of the one-group step over the same list with row k(i) as its hyper-parameters: the fp64 reference
and the derived bounds are optim_cases.reference / optim_cases.bounds of that one-group step (nothing is restated or measured here), the
shadow's are ema_cases.reference / ema_cases.bound on the kernel's own p'.

Inputs are optim_cases.build's for the case's base row (the row the 'U' and 'E' kinds scale p and g by); placements, arenas and guards are
optim_cases' too.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import ema_cases as E
import optim_cases as O
from optim_cases import CHUNK, F32, FLAT_TABLE, long_list  # noqa: F401

MAX_GROUPS = 16
ROW_NAMES = ('lr', 'b1', 'b2', 'eps', 'wd')

# rows: (lr, b1, b2, eps, wd)
R_POINT = (1e-3, 0.9, 0.999, 1e-8, 1e-2)          # test_fused_clip_adam_equals_torch's
R_HEADS = (1e-4, 0.9, 0.999, 1e-8, 1e-4)          # a smaller learning rate for the hyper-network heads
R_OFF = (1e-2, 0.5, 0.9, 1e-3, 0.0)               # every value off its default
ROWS3 = (R_POINT, R_HEADS, R_OFF)
ROWS = {
    'three': ROWS3,
    'one': (R_POINT,),
    'sixteen': tuple((1e-3 * 2.0 ** -k, 0.9 - 0.02 * k, 0.999 - 0.005 * k, 1e-8 * 2.0 ** k, 1e-3 * (k % 4)) for k in range(16)),
    'empty_group': ROWS3,                          # group 1 holds no tensor
    'lr0': (R_POINT, (0.0, 0.9, 0.999, 1e-8, 1e-2), R_OFF),
    'wd_only': (R_POINT, R_POINT[:4] + (0.0,), R_POINT[:4] + (0.1,)),
    'betas_only': (R_POINT, (1e-3, 0.5, 0.9, 1e-8, 1e-2), (1e-3, 0.8, 0.99, 1e-8, 1e-2)),
    'eps_only': ((1e-4, 0.9, 0.999, 1e-8, 0.0), (1e-4, 0.9, 0.999, 1e-3, 0.0), (1e-4, 0.9, 0.999, 1e-6, 0.0)),
}
MAX_NORM = {'active': 0.5, 'inactive': 1e9}
SHORT = (1, 2049, 5, 4096, 255, 7)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    rows: str                 # key of ROWS
    groups: tuple             # group of every tensor
    t: int
    numels: tuple
    clip: str = 'inactive'
    place: str = 'aligned'
    gs: float = 1.0
    ema: object = None        # None, or (decay, base, warmup)

    @property
    def n_groups(self):
        return len(ROWS[self.rows])

    @property
    def adam(self):
        """The optim_cases.Case that builds p, g, m, v (base row: group 0's) and places p and g ('dev' form)."""
        return O.Case(self.name, self.kind, 'group_base', self.t, self.numels, place=self.place, gs=self.gs)


def _interleaved(n, k):
    return tuple(i % k for i in range(n))


def _cases():
    c = []
    emas = (None, (0.9, 0, False), (0.9999, 5, True))
    # the short list, groups interleaved (0, 1, 2, 0, 1, 2): every placement, step, grad_scale, with and without EMA
    i = 0
    for place in ('aligned', 'shifted', 'mixed'):
        for t in (1, 2, 1000):
            for gs in (1.0, 1.0 / 3):
                c.append(Case('short_%s_t%d_gs%d_%s' % (place, t, round(1 / gs), ('plain', 'ema', 'emawarm')[i % 3]), 'W', 'three', _interleaved(6, 3), t, SHORT,
                              clip=('inactive', 'active')[i % 2], place=place, gs=gs, ema=emas[i % 3]))
                i += 1
    # a table boundary inside the list: the second (and third) launch must index group_of from its own first tensor
    for n in (161, 321):
        for j, place in enumerate(('aligned', 'shifted', 'mixed')):
            c.append(Case('list%d_%s' % (n, place), 'W', 'three', _interleaved(n, 3), (2, 1, 1000)[j], long_list(n, FLAT_TABLE), clip=('active', 'inactive')[j % 2],
                          place=place, gs=(1.0, 1.0 / 3)[j % 2], ema=emas[(j + (n == 321)) % 3]))
    # one group: the entry point is dpn_clip_adam_flat_dev / _ema
    c.append(Case('one_group_short', 'W', 'one', (0,) * 6, 2, SHORT, clip='active'))
    c.append(Case('one_group_list161_ema', 'W', 'one', (0,) * 161, 1, long_list(161, FLAT_TABLE), place='mixed', ema=emas[2]))
    # sixteen groups, every one used; on a list past a table boundary too
    c.append(Case('sixteen_short', 'W', 'sixteen', _interleaved(32, 16), 2, SHORT * 5 + (3, 2047), clip='active', place='mixed'))
    c.append(Case('sixteen_list161_ema', 'W', 'sixteen', tuple((i * 7 + i // 160) % 16 for i in range(161)), 1000, long_list(161, FLAT_TABLE), gs=1.0 / 3, ema=emas[1]))
    # a group without tensors, a group with lr = 0 (its p stays, its moments move)
    c.append(Case('empty_group', 'W', 'empty_group', (0, 2, 0, 2, 2, 0), 2, SHORT, clip='active', place='shifted'))
    c.append(Case('lr0_group', 'W', 'lr0', _interleaved(6, 3), 1, SHORT, ema=emas[1]))
    c.append(Case('lr0_group_u', 'U', 'lr0', _interleaved(6, 3), 2, SHORT, clip='active'))
    # groups that differ in one thing only
    c.append(Case('wd_only', 'W', 'wd_only', _interleaved(6, 3), 2, SHORT, clip='active'))
    c.append(Case('wd_only_t1000_shifted', 'W', 'wd_only', _interleaved(6, 3), 1000, SHORT, place='shifted', gs=1.0 / 3))
    c.append(Case('betas_only_t1', 'U', 'betas_only', _interleaved(6, 3), 1, SHORT))
    c.append(Case('betas_only_t2', 'U', 'betas_only', _interleaved(6, 3), 2, SHORT, clip='active', place='mixed', ema=emas[2]))
    c.append(Case('betas_only_t1000', 'U', 'betas_only', _interleaved(6, 3), 1000, SHORT, gs=1.0 / 3))
    c.append(Case('eps_only_t1', 'E', 'eps_only', _interleaved(6, 3), 1, SHORT))
    c.append(Case('eps_only_t1000_shifted', 'E', 'eps_only', _interleaved(6, 3), 1000, SHORT, place='shifted', ema=emas[1]))
    # update-resolved (|p| <= lr of the base row) on the short list and past a table boundary
    c.append(Case('u_short_t2', 'U', 'three', _interleaved(6, 3), 2, SHORT, clip='active'))
    c.append(Case('u_list161_t2', 'U', 'three', _interleaved(161, 3), 2, long_list(161, FLAT_TABLE)))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def rows_of(case):
    """[n_groups] dicts of the five per-group values plus the global max_norm, as exact floats of their fp32 values (the rows of hyper_dev)."""
    return [dict({k: O.f32(x) for k, x in zip(ROW_NAMES, row)}, max_norm=O.f32(MAX_NORM[case.clip])) for row in ROWS[case.rows]]


def hyper_rows(case):
    """hyper_dev as the ABI takes it: float32 [n_groups][8] = [lr, b1, b2, eps, wd, max_norm, grad_scale, ema_decay].  Rows past 0 carry POISON in
    the three values the kernel must read from row 0 only."""
    rows = rows_of(case)
    out = np.zeros((len(rows), 8), F32)
    for k, r in enumerate(rows):
        out[k, :5] = [r[n] for n in ROW_NAMES]
        out[k, 5:] = (r['max_norm'], case.gs, 0.0 if case.ema is None else case.ema[0]) if k == 0 else (3.0e-3, 7.0, 0.25)
    return out


@lru_cache(maxsize=None)
def built(name):
    """(inputs with the base row as their hyper-parameters, shadow before the step or None): computed once, shared, never written to."""
    case = case_by_name(name)
    base = rows_of(case)[0]
    O.HYPER['group_base'] = tuple(base[k] for k in O.HYPER_NAMES)
    try:
        inp = O.build(case.adam)
    finally:
        del O.HYPER['group_base']
    s0 = None
    if case.ema is not None:
        rng = np.random.default_rng([13, sum(map(ord, name)), len(case.numels)])
        s0 = [(p * (1.0 + 0.1 * rng.standard_normal(len(p))) + 1e-3 * rng.standard_normal(len(p))).astype(F32) for p in inp.p]
    return inp, s0


def with_row(inp, row):
    """The same step with ONE group whose row is `row`: what dpn_clip_adam_flat_dev runs with that row as hyper_dev."""
    return O.Inputs(inp.numels, inp.p, inp.g, inp.m, inp.v, dict(row), inp.gs, inp.t)


@lru_cache(maxsize=None)
def references(name):
    """Per group k: (one-group inputs, optim_cases.reference of them).  Tensor i of the grouped step is tensor i of references[k(i)]."""
    case = case_by_name(name)
    inp, _ = built(name)
    out = []
    for row in rows_of(case):
        one = with_row(inp, row)
        out.append((one, O.reference(one)))
    return out


def ratios(case, got):
    """Largest error / bound per quantity, every tensor against its own group's one-group reference and bounds."""
    refs = references(case.name)
    out = dict(p=0.0, m=0.0, v=0.0)
    for i, k in enumerate(case.groups):
        one, ref = refs[k]
        e_m, e_v, e_p = O.bounds(one, ref, i)
        for q, e in (('m', e_m), ('v', e_v), ('p', e_p)):
            out[q] = max(out[q], O._ratio(np.abs(np.asarray(got[q][i], np.float64) - ref[q][i]), e))
    if got.get('norm') is not None:
        ref0 = refs[0][1]                                      # the norm is global: every group's reference holds the same one
        out['norm'] = O._ratio(abs(float(got['norm']) - ref0['norm']), O.norm_bound(ref0))
    return out


def shadow_ratio(case, s0, got):
    """|s - s'| / bound against the fp64 recursion on the kernel's own p' (ema_cases)."""
    decay, base, warmup = case.ema
    args = (decay, case.t, base, warmup)
    return E.ratio(got['s'], E.reference(s0, got['p'], *args), E.bound(s0, got['p'], *args))


def shifts_of(case):
    """(per tensor (p, g, 0, 0) shifts as optim_cases gives them for the flat forms, shift of the shadow buffer)."""
    sshift = {'aligned': 0, 'shifted': 1 + len(case.numels) % 3, 'mixed': 0}[case.place] if case.ema is not None else 0
    return O.shifts_of(case.adam, 'dev'), sshift


# ---------------------------------------------------------------------------------------------- fp32 model, with seeded mistakes
MISTAKES = ('row0_everywhere', 'norm_per_group', 'second_table_group_from_0', 'bias_correction_row0')


def model_fp32(case, inp, s0=None, mistake=None, table=FLAT_TABLE):
    """A plain numpy.float32 evaluation of the grouped definition (squares rounded to fp32 and added in fp64, as the kernel's partials are; no
    fused multiply-add).  `mistake`: one of MISTAKES; `table`: tensors per launch."""
    assert mistake is None or mistake in MISTAKES
    rows = [{k: F32(x) for k, x in r.items()} for r in rows_of(case)]
    gs, one = F32(inp.gs), F32(1)
    n = len(inp.numels)
    group_of = list(case.groups)
    if mistake == 'row0_everywhere':
        group_of = [0] * n
    if mistake == 'second_table_group_from_0':
        group_of = [case.groups[i % table] for i in range(n)]

    def coef_over(idx):
        S = float(np.sum([np.sum(inp.g[i] * inp.g[i], dtype=np.float64) for i in idx]))
        total = F32(np.sqrt(S)) * gs
        return total, min(rows[0]['max_norm'] / (total + F32(1e-6)), one) * gs
    total, coef_all = coef_over(range(n))
    coef_grp = {k: coef_over([i for i in range(n) if case.groups[i] == k])[1] for k in set(case.groups)} if mistake == 'norm_per_group' else None
    st = F32(inp.t)
    P, M, V = [], [], []
    with np.errstate(all='ignore'):
        for i in range(n):
            h = rows[group_of[i]]
            hb = rows[0] if mistake == 'bias_correction_row0' else h
            coef = coef_all if coef_grp is None else coef_grp[case.groups[i]]
            bc1 = one - np.power(hb['b1'], st)
            bc2s = np.sqrt(one - np.power(hb['b2'], st))
            step_size = h['lr'] / bc1
            p, g, m, v = inp.p[i], inp.g[i], inp.m[i], inp.v[i]
            gi = h['wd'] * p + g * coef
            m1 = h['b1'] * m + (one - h['b1']) * gi
            v1 = h['b2'] * v + (one - h['b2']) * gi * gi
            p1 = p - step_size * m1 / (np.sqrt(v1) / bc2s + h['eps'])
            assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
            P.append(p1); M.append(m1); V.append(v1)
    out = dict(p=P, m=M, v=V, norm=float(total))
    if case.ema is not None:
        decay, base, warmup = case.ema
        out['s'] = E.model_fp32(s0, inp.p, P, decay, inp.t, base, warmup)
    return out
