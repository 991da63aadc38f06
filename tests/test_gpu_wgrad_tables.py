"""GPU (MI355X): dpn_wgrad_kernel forms product 2's operand G6 = g pe6 once per workgroup, in LDS, from the per-point table -- and computes what it
computed before.

The weight side is driven through the C ABI as tests/test_gpu_custom_residuals.py drives it (tools/wgrad_digest.py: pack, dpn_fwd_ref,
dpn_bwd_points_scaled with CPU-seeded random g_out, g_jxi and a scale of 0.75, dpn_wgrad, dpn_wgrad_finish) at n = 1 (one real point in 128 padded),
70 and 1037 (ragged 64- and 32-point tiles, the small range plan) and 5197 (the full 42-range plan), in both precisions.

tests/golden/wgrad_tables_parent.json holds the SHA-256 of every gradient as the commit BEFORE the cooperative forming computes it (written by
tools/wgrad_digest.py with that commit's library selected through DPN_LIB).  The range plan is that commit's at every size and in both modes, the
summation order with it, so every digest has to be EQUAL, at n = 5197 too.  (A re-swept plan was measured and not adopted, csrc/dpn_wgrad.hip at
choose_plan.  A change that does adopt one compares a strided sample of g_heads instead -- tools/wgrad_digest.py --sample writes it -- within twice
what the same change of plan does on the commit before: one build, two plans, -DDPN_EXPERIMENT_SPLITS with DPN_WGRAD_PLAN=0,13,14,15 against
0,15,13,14, moves g_heads by 2.692e-07 of its largest magnitude in this case, 1.153e-06 on the worst of the 50 gradient tensors:
tools/wgrad_plan_bound.py, profiles/wgrad_coop_forming_plans.txt.)"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('wgrad_digest', os.path.join(ROOT, 'tools', 'wgrad_digest.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

_cache = {}


def _fixture():
    if 'fx' not in _cache:
        with open(D.FIXTURE) as f:
            _cache['fx'] = json.load(f)
    return _cache['fx']


def _run(route, n, prec, **kw):
    key = (route, n, prec, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = D.run_case(route, n, prec, **kw)
    return _cache[key]


@pytest.mark.parametrize('prec', D.PRECS)
@pytest.mark.parametrize('n', D.SIZES)
def test_gradients_are_the_parent_commits(n, prec):
    res = _run('raw', n, prec)
    ref = _fixture()['cases'][D.case_key('raw', n, prec)]
    got = D.digest(res, with_sample=False)
    diff = [k for k in got if got[k] != ref[k]]
    assert len(got) == 50 and not diff, diff


@pytest.mark.parametrize('prec', D.PRECS)
@pytest.mark.parametrize('n', [1, 5197])
def test_ring_and_tile_split_stage_1_write_the_same_operands(n, prec):
    """(tests/test_gpu_parity.py::test_tile_split_kernels_against_the_ring_kernels has n = 70 and 1037)"""
    ring = _run('raw', n, prec, bwd_kernel='ring')
    tiles = _run('raw', n, prec, bwd_kernel='tiles')
    assert torch.equal(ring['operands'], tiles['operands'])
    assert int(ring['operands'].count_nonzero()) > 0
    for k in ring:
        assert torch.equal(ring[k], tiles[k]), k


@pytest.mark.parametrize('prec', D.PRECS)
def test_zero_cotangents_form_exact_zeros(prec):
    """n = 1: 127 padding points and one real one whose cotangents are zero: whatever the table holds there is finite, every formed element is 0."""
    res = D.run_case('raw', 1, prec, zero_cotangents=True)
    for k, v in res.items():
        if k == 'operands':
            continue
        assert bool(torch.isfinite(v).all()), k
        assert int(v.count_nonzero()) == 0, k


@pytest.mark.parametrize('prec', D.PRECS)
def test_caller_encoded_route_still_works(prec):
    """dpn_bwd_points with pe_in (the ring kernels, no coordinate cotangent) -> dpn_wgrad, n = 70."""
    got = D.digest(_run('pe_in', 70, prec), with_sample=False)
    ref = _fixture()['cases'][D.case_key('pe_in', 70, prec)]
    diff = [k for k in got if got[k] != ref[k]]
    assert not diff, diff
    assert int(_run('pe_in', 70, prec)['g_heads'].count_nonzero()) > 0
