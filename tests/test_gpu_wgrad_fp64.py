"""The weight side of the point path -- dpn_bwd_points* (stage 1) -> dpn_wgrad -> dpn_wgrad_finish -- against fp64, stage by stage, each stage
from the GPU's OWN upstream tensors (tests/wgrad_cases.py holds the cases, references and bounds; tests/test_wgrad_cases_cpu.py shows on the CPU
that the bounds hold for a faithful model of the kernels and break for each of a list of seeded mistakes).  One pass per case through
pack -> dpn_fwd_ref -> stage 1 -> dpn_wgrad -> dpn_wgrad_finish at the C ABI (tools/wgrad_digest.run_case), one synchronisation, one read-back.
Every pass condition is element-wise; no tensor maximum, no removed points: the masks are the GPU's own, and that they are the true masks
is asserted separately."""
import os
import sys

import pytest
import torch

import wgrad_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'tools') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu

_ratios = {}            # case id -> {(stage, tensor): worst error-to-bound ratio}


def gpu_pass(c, cot=None):
    """One pass of case c (cotangents cot, default the case's own), read back: (W, Features, obs as wgrad_cases.check() takes it, the raw outputs)."""
    import wgrad_digest as WD
    g_out, g_jxi = WC.cotangents(c) if cot is None else cot
    res = WD.run_case(c.route, c.n, c.prec, cotangents=(g_out, g_jxi), scale=c.scale, gain=c.gain, keep=True)
    cpu = lambda v: v.detach().cpu()
    inp = res['inputs']
    W = WC.weights_of(cpu(inp['heads']), cpu(inp['evec']), [cpu(s) for s in inp['statics']])
    F = WC.Features(cpu(inp['x']), cpu(inp['y']), cpu(inp['t']), cpu(inp['coord_data']), geometry=inp['geometry'],
                    pe_in=None if inp['pe_in'] is None else cpu(inp['pe_in']), prec=c.prec)
    T1, m1, m2 = WC.decode_saved(cpu(res['saved']), c.n, c.prec)
    Z1, gnet, gj = WC.decode_operands(cpu(res['operands']), c.n, c.prec, table=WC.fused_route(c))
    sums, sums_abs = WC.decode_partials(cpu(res['partials']), inp['k_splits'])
    outs = {'g_heads': cpu(res['g_heads']), 'g_evec': cpu(res['g_evec']), 'statics': [cpu(res['static_%02d' % i]) for i in range(48)]}
    obs = {'m1': m1, 'm2': m2, 'T1': T1, 'Z1': Z1, 'gnet': gnet, 'gj': gj, 'sums': sums, 'sums_abs': sums_abs,
           'grads': WC.weights_of(outs['g_heads'], outs['g_evec'], outs['statics'])}
    return W, F, obs, outs, (g_out, g_jxi)


def flat_outputs(outs):
    return [outs['g_heads'], outs['g_evec']] + outs['statics']


@pytest.mark.parametrize('c', WC.all_cases(), ids=WC.case_id)
def test_every_stage_against_fp64_from_the_gpus_own_upstream_tensors(c):
    W, F, obs, outs, (g_out, g_jxi) = gpu_pass(c)
    n, n_pad = c.n, WC.pad_points(c.n)
    # ---- stage 1's cotangent streams: ONE fp32 product with the scale, zero at the padding points (Z1's padding rows: decode_operands)
    s = torch.tensor(c.scale, dtype=torch.float32)
    want = torch.zeros(6, n_pad)
    want[:, :n] = (s * g_out).t()
    assert torch.equal(obs['gnet'], want), 'gnet is not scale * g_out'
    if obs['gj'] is not None:
        want = torch.zeros(6, 3, n_pad)
        want[:, :, :n] = (s * g_jxi).permute(1, 2, 0)
        assert torch.equal(obs['gj'], want), 'gJ is not scale * g_jxi'
    # ---- every stage, element-wise (stage 1: Z1; saved state: T1; dpn_wgrad: the eight sums; the finish and the whole weight side: all 50 outputs)
    r = WC.check(c, W, F, obs, g_out, g_jxi)
    _ratios[WC.case_id(c)] = r
    for key in sorted(r):
        print('%-8s %-5s %.3g' % (key[0], key[1], r[key]))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    # ---- dpn_finish_sides_kernel writes d bd, d evec and column 256 of d w2b2 from ONE value (finish_vside_body: the `else` branch of its store)
    for k in range(6):
        gcvec = outs['g_heads'][:, 1158 + 257 * k + 256]
        assert torch.equal(outs['g_evec'][k], gcvec) and torch.equal(outs['statics'][8 * k + 1], gcvec), k
    # ---- a net without cotangents has exact zeros; the hit net's gradient is the rank-one fp64 value (checked above, as every case's)
    if c.kind.startswith('onehot'):
        for k in range(6):
            vals = list(obs['grads'][k].values())
            if k == WC.HOT_NET:
                assert any(bool(v.any()) for v in vals)
            else:
                assert all(not bool(v.any()) for v in vals), k
    if c.kind == 'gjxi':                                    # reached through the gJ rows alone: every g-weighted sum vanishes, dw1 does not
        assert not bool(obs['sums']['S2'].any()) and not bool(obs['sums']['mv'].any()) and bool(obs['sums']['dw1'].any())


@pytest.mark.parametrize('n', [70, 1037])
def test_the_weight_side_is_linear_in_the_cotangents_bit_for_bit(n):
    """All cotangents times 2^8 or 2^-8: every gradient times exactly that factor.  The header's stated limit (dpn_point_common.h) is normal values
    only -- a bf16 part below 2^-126 may be flushed -- so the inputs are the dense normal streams, whose hi and lo parts stay normal at these factors.
    Zero cotangents for one net: exact zeros for that net, the other nets' bits unchanged."""
    c = WC.Case('raw', n, 'bf16x2', 1.0, 'dense', 0.75)
    g_out, g_jxi = WC.cotangents(c)
    base = flat_outputs(gpu_pass(c)[3])
    assert all(bool(torch.isfinite(v).all()) for v in base) and min(float(v.abs()[v != 0].min()) for v in base) * 2.0 ** -8 > 2.0 ** -100
    for f in (2.0 ** 8, 2.0 ** -8):
        got = flat_outputs(gpu_pass(c, cot=(g_out * f, g_jxi * f))[3])
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.equal(a, b * f), (f, i)
    dead = 2
    go, gj = g_out.clone(), g_jxi.clone()
    go[:, dead], gj[:, dead] = 0.0, 0.0
    W, F, obs, outs, _ = gpu_pass(c, cot=(go, gj))
    ref = WC.weights_of(base[0], base[1], base[2:])
    for k in range(6):
        for nm in WC.NAMES:
            if k == dead:
                assert not bool(obs['grads'][k][nm].any()), nm
            else:
                assert torch.equal(obs['grads'][k][nm], ref[k][nm]), (k, nm)


@pytest.mark.parametrize('route,n,gain', [('raw', n, 1.0) for n in WC.SIZES] + [('raw', 70, 5.0), ('raw', 1037, 5.0), ('pe_in', 70, 1.0)])
def test_the_gpus_masks_are_the_true_masks(route, n, gain):
    """'The GPU's own masks' must not hide a wrong mask export: the decoded masks differ from the fp64 masks (the same fp32 weights, fp64 features
    and arithmetic) at no more than max(3, n // 100) points -- test_gpu_parity's cap; tests/test_wgrad_cases_cpu.py shows the fp32 kernel model
    inside it on these inputs at both gains."""
    c = WC.Case(route, n, 'bf16x2', gain, 'dense', 0.75 if route == 'raw' else 1.0)
    W, F, obs, _, _ = gpu_pass(c)
    true = WC.masks_reference(W, F, WC.fused_route(c))
    flipped = WC.flipped_points(true, (obs['m1'], obs['m2']))
    print('%s n = %d gain %g: %d points carry a mask bit that differs from fp64: %s' % (route, n, gain, int(flipped.sum()), torch.nonzero(flipped).flatten().tolist()[:20]))
    assert int(flipped.sum()) <= max(3, n // 100)
    assert bool(obs['m1'].any()) and bool(obs['m2'].any()) and not bool(obs['m1'].all()) and not bool(obs['m2'].all())


def test_zz_summary_of_error_to_bound_ratios():
    """The worst error-to-bound ratio per stage and tensor over the cases above that ran in this process (the table of DESIGN.md section 5,
    'weight side'; profiles/wgrad_fp64_ratios.txt is this output on an MI355X)."""
    worst = {}
    for cid, r in _ratios.items():
        for key, v in r.items():
            if key not in worst or v > worst[key][0]:
                worst[key] = (v, cid)
    print('\nstage    tensor  worst |error| / bound   case  (%d cases)' % len(_ratios))
    order = {s: i for i, s in enumerate(('stage1', 'saved', 'wgrad', 'finish', 'chain'))}
    for key in sorted(worst, key=lambda k: (order[k[0]], k[1])):
        print('%-8s %-6s  %-8.3g               %s' % (key[0], key[1], worst[key][0], worst[key][1]))
    assert all(v[0] <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v[0] <= 1.0}
