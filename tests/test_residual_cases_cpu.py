"""CPU: the reference, the inputs and the bounds of tests/residual_cases.py, which tests/test_gpu_residual.py holds the kernels of
csrc/dpn_residual.hip to.  Shown here without a GPU: the de-normalisation restatement is oracle.inverse_norm bit for bit on the shipped tables;
no point of any case lies inside a guard band and the plain fp32 torch evaluation takes the fp64 side of every switch at every point (the cap on
excluded points is zero); the recorded K constants hold; the forced and exact rows reach every branch; each seeded mistake of the kernel's
hand-written derivative lands outside the GPU test's bars.
"""
import math

import numpy as np
import pytest
import torch

import residual_cases as R
from oracle import dpn_oracle as O

_K = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nfp32 torch against fp64, largest |error| / (2^-24 scale): ' + ', '.join('%s %.2f' % kv for kv in sorted(_K.items()))
          + '   recorded: ' + ', '.join('%s %.1f' % kv for kv in sorted(R.K_RECORDED.items())))


def _bits(t):
    return t.detach().numpy().tobytes()


@pytest.mark.parametrize('with_clip', [True, False])
@pytest.mark.parametrize('cfg', ['shipped_norm_cfg', 'f12_norm_cfg', 'f12_norm_sq_cfg'])
def test_denorm_restatement_is_inverse_norm_bit_for_bit(cfg, with_clip):
    norm_cfg = getattr(O, cfg)()
    table = R.table_from_norm_cfg(cfg, norm_cfg, with_clip=with_clip)
    g = torch.Generator().manual_seed(3)
    fields = [torch.randn(4096, 1, dtype=torch.float64, generator=g) * s for s in (3.0, 3.0, 8.0, 20.0, 4.0, 9.0)]
    want, got = O.inverse_norm(fields, with_clip=with_clip, norm_cfg=norm_cfg), R.denorm(fields, table)
    for k in range(6):
        assert _bits(want[k]) == _bits(got[k]), (cfg, with_clip, k)
    if cfg == 'shipped_norm_cfg':                                 # and the oracle's default table
        want = O.inverse_norm(fields, with_clip=with_clip)
        assert all(_bits(want[k]) == _bits(got[k]) for k in range(6))


def test_tables_hold_fp32_values_and_the_case_table_covers_the_issue():
    for tb in R.TABLES.values():
        for t in (tb.mean, tb.std, tb.lo, tb.hi, tb.sq_add, tb.factor):
            assert all(R.f32(x) == x for x in t), tb.name
    c = R.TABLES['custom']
    assert c.sq_on[0] and not c.clip_on[0] and c.sq_on[3] and c.clip_on[3] and not c.sq_on[4]
    at257 = [x for x in R.CASES if x.kind == 'residual' and x.n == 257]
    assert {x.table for x in at257} == {'shipped', 'noclip', 'f12', 'f12sq', 'custom'}
    assert {(x.crit, x.reduce_sum) for x in at257} == {('mse', False), ('mse', True), ('l1', False), ('l1', True), ('sl1', False)}
    assert {x.beta_eq for x in at257 if x.crit == 'sl1'} == set(range(6))
    assert {x.up for x in at257} == {'none', 'gl', 'gtot', 'both'} and {x.out for x in at257} == {'both', 'loss', 'cot'}
    assert {x.n for x in R.CASES if x.kind == 'residual' and x.table == 'shipped' and x.crit == 'mse'} >= set(R.RES_N)
    assert {(x.table, x.n) for x in R.CASES if x.kind == 'points'} >= {(t, n) for t in ('shipped', 'noclip', 'f12', 'f12sq') for n in R.POINT_N}
    assert {(x.weights, x.n, x.crit) for x in R.CASES if x.kind == 'weighted'} == {(w, n, c) for w in ('w', 'bin', 'both') for n in (257, 1037) for c in ('mse', 'sl1')}
    assert {(x.n_inter, x.n - x.n_inter, x.B) for x in R.CASES if x.kind == 'step'} == {(a, b, B) for a, b in R.STEP_SPLITS for B in (1, 3)}
    assert max(x.n for x in R.CASES) <= 1037


def _groups(name):
    """The (inputs, reference) pairs a case is compared on: itself, or both groups of every field of a step."""
    case = R.case_by_name(name)
    if case.kind != 'step':
        return [R.built(name)]
    out = []
    for b in range(case.B):
        inp, _, sref = R.built_step(name, b)
        out += [(inp.rows(slice(0, case.n_inter)), sref.groups[0]), (inp.rows(slice(case.n_inter, None)), sref.groups[1])]
    return out


@pytest.mark.parametrize('name', R.CASE_IDS)
def test_fp32_torch_takes_every_switch_as_fp64_and_stays_inside_the_recorded_k(name):
    """No point inside a guard band; the fp32 evaluation on the fp64 side of every clip bound, of omega = 0, q = q_s and the criterion's kink at
    every point (nothing is excluded from any comparison); its error within the recorded K of every kind."""
    for inp, ref in _groups(name):
        if not inp.exact:
            assert not R.guard_violations(inp, ref.ev).any(), name
        got = R.fp32_outputs(inp)
        assert (R.sides(inp, got['ev']) == R.sides(inp, ref.ev)).all(), name
        assert got['ev'].delta.tolist() == ref.ev.delta.tolist()
        m = R.measure(inp, ref, got)
        for k, x in m.items():
            _K[k] = max(_K.get(k, 0.0), x)
            assert x <= R.K_RECORDED[k], (name, k, x)
        bars, total_bar = R.loss_bars(inp, ref, R.K_RECORDED['res'])
        assert (np.abs(got['ev'].losses - ref.ev.losses) <= bars).all(), name
        assert np.isfinite(bars).all() and np.isfinite(total_bar)


@pytest.mark.parametrize('name', [c.name for c in R.CASES if c.crit == 'sl1' and c.table != 'exact'])
def test_smooth_l1_beta_puts_its_equation_on_both_sides_of_the_kink(name):
    case = R.case_by_name(name)
    for inp, ref in _groups(name)[:1] if case.kind != 'step' else [(R.built_step(name, 0)[0], None)]:
        ev = ref.ev if ref is not None else R.evaluate(inp, scales=False)
        quad = float((np.abs(ev.r[:, case.beta_eq]) < inp.beta).mean())
        assert 0.2 <= quad <= 0.8, (name, quad)


@pytest.mark.parametrize('table', ['shipped', 'f12', 'f12sq', 'custom'])
def test_forced_rows_reach_every_branch(table):
    name = next(c.name for c in R.CASES if c.kind == 'residual' and c.table == table and c.n == 257)
    inp, ref = R.built(name)
    s, tb = R.sides(inp, ref.ev), inp.table
    for k in range(2, 6):
        if tb.clip_on[k]:
            reach = {-1, 1} if not tb.sq_on[k] or tb.sq_add[k] < tb.lo[k] else {1}         # a squared form cannot go below its shift
            assert reach <= set(s[:, k].tolist()), (table, k)
            assert not ref.ev.dvdo[s[:, k] != 0, k].any()                                   # mask 0 outside the bounds
    assert {(a, b) for a, b in s[:, 6:8].tolist()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(ref.ev.delta.tolist()) == {0.0, 1.0}
    assert ((ref.ev.q_s == 1e-6) & (ref.ev.delta == 1)).any(), 'q_s on its floor at a saturated point'
    if table == 'f12sq':                                          # a negative root inside the bounds after squaring
        lin = inp.out_n[:, 4].astype(np.float64) * tb.std[4] + tb.mean[4]
        assert ((lin < tb.lo[4]) & (s[:, 4] == 0)).any()


@pytest.mark.parametrize('name', ['res_exact_mse', 'res_exact_l1', 'res_exact_sl1'])
def test_exact_rows_sit_on_their_switches(name):
    inp, ref = R.built(name)
    ev, tb = ref.ev, inp.table
    assert (ev.val == inp.out_n.astype(np.float64)).all(), 'val = out_n exactly'
    row = 0
    for k in (2, 3, 4, 5):                                        # v == clip_lo, v == clip_hi: mask 1, the gradient passes as torch.clip's does
        for b in (tb.lo[k], tb.hi[k]):
            assert ev.pre[row, k] == b and ev.dvdo[row, k] == 1.0, (row, k)
            row += 1
    for i in range(row, row + 4):                                 # omega == 0 exactly: delta = 0 whatever q
        assert ev.omega[i] == 0.0 and ev.delta[i] == 0.0
    assert (ev.val[[row, row + 1], 4] >= ev.q_s[[row, row + 1]]).all(), 'saturated: omega < 0 alone keeps delta at 0'
    z = slice(inp.n - R.N_EXACT_ZERO, None)
    assert not ev.r[z, :5].any() and not ev.cA[:5, z].any() and not ev.cB[:5, z].any() and not ev.g_jxi[z].any()
    got = R.fp32_outputs(inp)['ev']
    assert not got.r[z, :5].any() and not got.g_jxi[z].any() and (got.omega[row:row + 4] == 0).all()


@pytest.mark.parametrize('name', ['res_shipped_mse_257', 'res_shipped_sl1_eq3_257', 'wt_both_mse_257'])
def test_elementwise_criterion_equals_pde_criterion(name):
    """The weighted reference's own elementwise criterion against oracle.pde_criterion with every weight 1."""
    inp, ref = R.built(name)
    plain = R.Inputs(inp.table, inp.crit, inp.beta, inp.reduce_sum, inp.out_n, inp.jac_n, inp.f, inp.gl, inp.gtot)
    ones = R.Inputs(inp.table, inp.crit, inp.beta, inp.reduce_sum, inp.out_n, inp.jac_n, inp.f, inp.gl, inp.gtot, w=np.ones(inp.n, np.float32))
    a, b = R.evaluate(plain), R.evaluate(ones)
    assert np.allclose(a.losses, b.losses, rtol=1e-13, atol=0) and np.allclose(a.g_out, b.g_out, rtol=1e-12, atol=0)


_MISTAKE_CASES = dict(gv4_sign=('res_shipped_mse_257', 'res_shipped_l1_257'), sq_correction_dropped=('res_f12sq_mse_257', 'res_custom_mse_257'),
                      gJ2_without_eps=('res_shipped_mse_257', 'res_custom_l1_257'), clip_mask_before_square=('res_f12sq_mse_257', 'res_custom_mse_257'),
                      slope_without_beta=('res_shipped_sl1_eq0_257', 'res_custom_sl1_eq4_257'))


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_seeded_mistake_lands_outside_the_bars(mistake):
    """The reference in fp64 with one mistake of the kind the kernel's hand-written derivative could hold: outside GPU_FACTOR x K at some element
    of every case listed for it, while the unperturbed fp64 evaluation sits at 0."""
    for name in _MISTAKE_CASES[mistake]:
        inp, ref = R.built(name)
        m = R.measure(inp, ref, R.fp32_outputs(inp, mistake=mistake, dtype=torch.float64))
        worst = max(m[k] / (R.GPU_FACTOR * R.K_RECORDED[k]) for k in m)
        print('%s on %s: %.3g x the GPU bar' % (mistake, name, worst))
        assert worst > 1.0, (mistake, name, m)
        clean = R.measure(inp, ref, R.fp32_outputs(inp, dtype=torch.float64))
        assert max(clean.values()) < 1e-3, clean


@pytest.mark.parametrize('name', ['res_exact_mse', 'res_exact_l1', 'res_exact_sl1'])
def test_gJ2_without_eps_is_seen_on_an_in_bounds_density(name):
    """1e-6 / rho is 2^-24-sized at rho = 1 and hides behind the rounding of out std + mean at a small shipped density: the 'exact' row with
    rho = 2^-6, inside its bounds and free of rounding, is where the bars see it at full strength."""
    inp, ref = R.built(name)
    i = R.EXACT_SMALL_RHO_ROW
    assert ref.ev.val[i, 5] == 2.0 ** -6 and R.sides(inp, ref.ev)[i, 5] == 0
    bad = R.fp32_outputs(inp, mistake='gJ2_without_eps', dtype=torch.float64)
    r = np.abs(bad['g_jxi'] - ref.ev.g_jxi)[i] / (R.U * ref.g_jxi_scale[i] + 1e-300)
    assert r.max() > R.GPU_FACTOR * R.K_RECORDED['g_jxi'], r.max()


def test_finish_reference_bars_hold_for_a_numpy_fp32_model():
    for nblk in R.FINISH_BLOCKS:
        rows = R.finish_rows(nblk, 1)[0]
        n = nblk * 256 - 3
        fac = R.TABLES['shipped'].factor
        l, bars, total, total_bar = R.finish_reference(rows, n, fac, False)
        model = np.array([np.float32(float(np.float32(rows[:, e].sum() / n)) * fac[e]) for e in range(6)], np.float32)
        assert (np.abs(model.astype(np.float64) - l) <= bars).all()
        assert abs(float(R.total_in_order(model)) - total) <= total_bar
        assert bars.max() / l.max() < 4 * R.U


def test_arena_windows_and_guards():
    a = R.Arena(np.float32, R.SENTINEL, dict(x=np.arange(6, dtype=np.float32).reshape(2, 3), y=np.ones(5, np.float32)))
    assert a.offsets['x'] % 4 == 0 and a.offsets['y'] % 4 == 0 and a.offsets['x'] >= R.GUARD
    full = a.full.copy()
    assert a.untouched(full) and (a.window(full, 'x') == np.arange(6).reshape(2, 3)).all()
    full[a.offsets['y'] + 1] = 7.0
    assert a.outside_kept(full) and not a.untouched(full)
    full[a.offsets['y'] + 5] = 7.0
    assert not a.outside_kept(full)
