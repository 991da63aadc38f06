"""GPU (MI355X): loss balancing by gradient norms -- dpn_balance_sumsq / dpn_balance_update / dpn_balance_combine through
the C ABI, point_path.balanced_total, InterfacePhysics.training_step(balance=...) and the training loops' option.

Yardsticks: the host references of deepphysinet_amd.balance; a numpy fp32 loop for the combine; torch.autograd.grad norms in fp64 for the step.

Bound of test 1.  Every element enters as (double)x * (double)x, and a product of two fp32 values (24-bit significands) is exact in fp64 (53 bits): the
only roundings are additions.  All summands are >= 0, so every partial sum on either side is <= the exact sum S, and one addition errs by at most
2^-53 of its result.  The reference adds the n squares sequentially: n - 1 additions, |ref - S| <= (n - 1) 2^-53 S to first order.  The kernel adds
the same n numbers in a tree of n - 1 additions (zero-initialised accumulators add exactly): |gpu - S| <= (n - 1) 2^-53 S.  Together
|gpu - ref| <= (n - 1) 2^-52 S, and the remaining 2^-52 S covers the second-order terms and S against ref: |gpu - ref| <= n 2^-52 ref."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_adaptive import _dev, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dpn_balance_sumsq', 'dpn_balance_update', 'dpn_balance_combine')
U32, U64 = 2.0 ** -23, 2.0 ** -53


def _lib():
    from deepphysinet_amd import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ 1. sum of squares
def _wide(n, seed):
    """n fp32 values of either sign with magnitudes log-uniform over 1e-18 .. 1e15."""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-18.0, 15.0, n)) * rng.choice([-1.0, 1.0], n)
    if n >= 2:
        v[0], v[-1] = 1e-18, -1e15                         # both ends of the range are present
    return v.astype(np.float32)


def _call_sumsq(arrays):
    L, lib = _lib()
    dev = _dev()
    tensors = [None if a[1] is None else torch.from_numpy(a[1]).to(dev) for a in arrays]          # (numel, values or None: a NULL pointer)
    numel = (ctypes.c_int64 * len(arrays))(*[a[0] for a in arrays])
    table = (ctypes.c_void_p * len(arrays))(*[None if t is None else t.data_ptr() for t in tensors])
    n_scratch = int(lib.dpn_balance_scratch_doubles(len(arrays), numel))
    assert n_scratch == sum((a[0] + 2047) // 2048 for a in arrays)
    scratch = torch.full((n_scratch,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=dev)            # the slot and a guard on either side
    rc = lib.dpn_balance_sumsq(len(arrays), table, numel, _p(scratch), ctypes.c_void_p(out.data_ptr() + 8), _s())
    torch.cuda.synchronize()
    assert rc == 0 and out[0] == -7.0 and out[2] == -7.0
    return float(out[1])


@pytest.mark.parametrize('lengths', [(1,), (2047, 2049), (2048, None, 1), (5000, 2049, 2048, 2047), (5000,), (1,) * 161 + (2049, 2047)],
                         ids=lambda v: '-'.join(map(str, v)) if len(v) < 6 else '163-tensors')
def test_sumsq_equals_the_sequential_fp64_sum_within_n_ulps_and_is_deterministic(lengths):
    """Tables of 1 to 4 tensors with lengths from {1, 2047, 2048, 2049, 5000}, one with a NULL entry (counted as 5000 zeros), and one of 163 tensors
    (more than the 160 of one launch: the entry point cuts the table), values over 1e-18 .. 1e15; bound: the module docstring's n 2^-52 ref, n the number of elements; two runs agree bitwise."""
    from deepphysinet_amd.balance import sumsq_reference
    arrays = [(5000, None) if n is None else (n, _wide(n, 10 * i + len(lengths))) for i, n in enumerate(lengths)]
    ref = sumsq_reference([a[1] for a in arrays])
    got = _call_sumsq(arrays)
    again = _call_sumsq(arrays)
    n = sum(a[0] for a in arrays if a[1] is not None)
    print('lengths %.40s: gpu %.17g ref %.17g |diff| / ref %.3g (bound %.3g)' % (lengths, got, ref, abs(got - ref) / ref, n * 2.0 ** -52))
    assert ref > 0.0 and abs(got - ref) <= n * 2.0 ** -52 * ref
    assert got == again


def test_sumsq_rejects_tables_it_does_not_take():
    L, lib = _lib()
    dev = _dev()
    t = torch.ones(8, dtype=torch.float32, device=dev)
    out = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    scratch = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    table = (ctypes.c_void_p * 1)(t.data_ptr())
    for n_t, numel in ((0, 8), (4097, 8), (1, 0), (1, -3), (1, 2 ** 31)):
        nm = (ctypes.c_int64 * 1)(numel)
        assert lib.dpn_balance_scratch_doubles(n_t, nm) == 0
        assert lib.dpn_balance_sumsq(n_t, table, nm, _p(scratch), _p(out), _s()) == -1
    nm = (ctypes.c_int64 * 1)(8)
    assert lib.dpn_balance_sumsq(1, table, nm, None, _p(out), _s()) == -1 and lib.dpn_balance_sumsq(1, table, nm, _p(scratch), None, _s()) == -1
    torch.cuda.synchronize()
    assert out[0] == -7.0 and (scratch == -7.0).all()
    assert lib.dpn_balance_sumsq(1, table, nm, _p(scratch), _p(out), _s()) == 0
    torch.cuda.synchronize()
    assert out[0] == 8.0


# ------------------------------------------------------------------------------------------------ 2. update
def _call_update(sumsq, lam, momentum, lam_min, lam_max):
    L, lib = _lib()
    dev = _dev()
    K = len(sumsq)
    s = torch.tensor(np.asarray(sumsq, dtype=np.float64), device=dev)
    lam_dev = torch.full((K + 2,), -7.0, dtype=torch.float32, device=dev)
    lam_dev[1:K + 1] = torch.tensor(np.asarray(lam, dtype=np.float32), device=dev)
    diag = torch.full((3 * K + 4,), -7.0, dtype=torch.float64, device=dev)
    rc = lib.dpn_balance_update(_p(s), K, momentum, lam_min, lam_max, ctypes.c_void_p(lam_dev.data_ptr() + 4), ctypes.c_void_p(diag.data_ptr() + 8), _s())
    torch.cuda.synchronize()
    if rc == 0:
        assert lam_dev[0] == -7.0 and lam_dev[-1] == -7.0 and diag[0] == -7.0 and diag[-1] == -7.0          # nothing written past the ends
    return rc, lam_dev[1:K + 1].cpu().numpy(), diag[1:-1].cpu().numpy()


def _update_cases():
    cases = [([4.0, 4.0, 4.0], [1.0, 1.0, 1.0], 0.9, 1e-3, 1e3),                  # equal norms
             ([1.0, 9.0], [1.0, 1.0], 0.5, 1e-3, 1e3),
             ([1.0, 0.0, 9.0], [1.0, 7.0, 1.0], 0.0, 1e-3, 1e3),                  # one zero norm: inactive
             ([0.0, 5.0, 0.0], [2.0, 3.0, 4.0], 0.0, 1e-3, 1e3),                  # one active term only: flag
             ([1.0, float('nan'), 9.0], [2.0, 3.0, 4.0], 0.0, 1e-3, 1e3),         # NaN: flag
             ([1.0, float('inf'), 9.0], [2.0, 3.0, 4.0], 0.0, 1e-3, 1e3),
             ([1e-8, 1e8], [1.0, 1.0], 0.0, 0.75, 100.0),                        # both clamps
             ([1.0, 9.0], [5.0, 5.0], 0.0, 1e-3, 1e3),                            # momentum 0
             ([1.0, 9.0], [5.0, 0.25], 1.0, 1e-3, 1e3)]                           # momentum 1
    rng = np.random.default_rng(5)
    for K in (3, 7, 3, 7, 7, 16):
        s = 10.0 ** rng.uniform(-30.0, 30.0, K)
        if K == 7 and len(cases) % 2:
            s[rng.integers(K)] = 0.0
        lam = (10.0 ** rng.uniform(-2.0, 2.0, K)).astype(np.float32)
        cases.append((list(s), list(lam), float(rng.uniform(0.0, 1.0)), 1e-3, 1e3))
    return cases


def test_update_equals_the_reference_on_the_hand_worked_and_on_random_cases():
    """The new lambda within one fp32 ulp (2^-23 relative: a handful of fp64 roundings, then one rounding to fp32), n_k and the mean within 8 * 2^-53
    relative, the flag exact; inactive terms and flagged cases leave lambda bitwise untouched."""
    from deepphysinet_amd.balance import update_reference
    for sumsq, lam, momentum, lo, hi in _update_cases():
        K = len(sumsq)
        want, flag, wdiag = update_reference(sumsq, lam, momentum, lo, hi, with_diag=True)
        rc, got, diag = _call_update(sumsq, lam, momentum, lo, hi)
        assert rc == 0 and diag.shape == (3 * K + 2,)
        assert diag[3 * K + 1] == float(flag), (sumsq, diag)
        lam32 = np.asarray(lam, dtype=np.float32)
        n_ref, n_got = wdiag[:K], diag[:K]
        fin = np.isfinite(n_ref)
        assert (np.isfinite(n_got) == fin).all() and (np.abs(n_got[fin] - n_ref[fin]) <= 8 * U64 * n_ref[fin]).all()
        assert abs(diag[3 * K] - wdiag[3 * K]) <= 8 * U64 * wdiag[3 * K]
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= U32 * np.abs(want.astype(np.float64))).all(), (sumsq, got, want)
        assert (diag[2 * K:3 * K] == got.astype(np.float64)).all()                              # diag's new lambda is the fp32 value
        active = np.isfinite(n_ref) & (n_ref > 0.0)
        untouched = np.ones(K, dtype=bool) if flag else ~active
        assert (got[untouched].view(np.uint32) == lam32[untouched].view(np.uint32)).all()
        assert (diag[K:2 * K][untouched] == 0.0).all()
        if not flag:
            assert (np.abs(diag[K:2 * K][active] - wdiag[K:2 * K][active]) <= 16 * U64 * wdiag[K:2 * K][active]).all()
            if momentum == 1.0:
                assert (got.view(np.uint32) == lam32.view(np.uint32)).all()
    # equal norms give exactly 1
    rc, got, diag = _call_update([4.0, 4.0, 4.0], [1.0, 1.0, 1.0], 0.9, 1e-3, 1e3)
    assert (got == 1.0).all() and diag[9] == 2.0


def test_update_and_combine_reject_bad_arguments_and_launch_nothing():
    L, lib = _lib()
    for K, momentum, lo, hi in ((17, 0.5, 1e-3, 1e3), (3, -0.1, 1e-3, 1e3), (3, 1.5, 1e-3, 1e3), (3, float('nan'), 1e-3, 1e3), (3, 0.5, 0.0, 1e3),
                                (3, 0.5, 2.0, 1e3), (3, 0.5, 1e-3, 0.5), (3, 0.5, 1e-3, float('inf'))):
        rc, lam, diag = _call_update([1.0] * 17, [3.0] * 17, momentum, lo, hi) if K == 17 else _call_update([1.0, 4.0, 9.0], [3.0] * 3, momentum, lo, hi)
        assert rc == -1 and (lam == 3.0).all() and (diag == -7.0).all(), (K, momentum, lo, hi)
    dev = _dev()
    terms = torch.ones(13, dtype=torch.float32, device=dev)
    table = (ctypes.c_void_p * 13)(*[terms.data_ptr() + 4 * i for i in range(13)])
    lam = torch.ones(3, dtype=torch.float32, device=dev)
    out = torch.full((14,), -7.0, dtype=torch.float32, device=dev)
    ok, bad = (ctypes.c_int * 13)(*([1] * 6 + [2] * 6 + [0])), (ctypes.c_int * 13)(*([1] * 6 + [3] * 6 + [0]))
    assert lib.dpn_balance_combine(table, 3, bad, _p(lam), None, _p(out), None, _s()) == -1               # a map entry outside 0..K - 1
    assert lib.dpn_balance_combine(table, 3, ok, _p(lam), None, None, None, _s()) == -1                   # no output
    assert lib.dpn_balance_combine(table, 3, ok, _p(lam), None, None, _p(out), _s()) == -1                # cot_out without cot_in
    assert lib.dpn_balance_combine(None, 3, ok, _p(lam), None, _p(out), None, _s()) == -1                 # total without terms
    assert lib.dpn_balance_combine(table, 17, ok, _p(lam), None, _p(out), None, _s()) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ------------------------------------------------------------------------------------------------ 3. combine
def _call_combine(terms, lam, term_map, cot_in):
    L, lib = _lib()
    dev = _dev()
    # the 13 scalars live in three separate tensors, as step_losses returns them
    it, mt, d = (torch.tensor(np.asarray(v, dtype=np.float32), device=dev) for v in (terms[:6], terms[6:12], terms[12:]))
    table = (ctypes.c_void_p * 13)(*([it.data_ptr() + 4 * i for i in range(6)] + [mt.data_ptr() + 4 * i for i in range(6)] + [d.data_ptr()]))
    lam_dev = torch.tensor(np.asarray(lam, dtype=np.float32), device=dev)
    cmap = (ctypes.c_int * 13)(*term_map)
    total = torch.full((3,), -7.0, dtype=torch.float32, device=dev)
    cot = torch.full((15,), -7.0, dtype=torch.float32, device=dev)
    g = torch.tensor([cot_in], dtype=torch.float32, device=dev)
    assert lib.dpn_balance_combine(table, len(lam), cmap, _p(lam_dev), _p(g), ctypes.c_void_p(total.data_ptr() + 4), ctypes.c_void_p(cot.data_ptr() + 4),
                                   _s()) == 0
    torch.cuda.synchronize()
    assert total[0] == -7.0 and total[2] == -7.0 and cot[0] == -7.0 and cot[14] == -7.0
    # the two directions as launches of their own, as the autograd function issues them
    total2 = torch.empty(1, dtype=torch.float32, device=dev)
    cot2 = torch.empty(13, dtype=torch.float32, device=dev)
    assert lib.dpn_balance_combine(table, len(lam), cmap, _p(lam_dev), None, _p(total2), None, _s()) == 0
    assert lib.dpn_balance_combine(None, len(lam), cmap, _p(lam_dev), _p(g), None, _p(cot2), _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(total2, total[1:2]) and torch.equal(cot2, cot[1:14])
    return total[1].cpu().numpy(), cot[1:14].cpu().numpy()


def test_combine_is_the_fp32_sum_in_the_stated_order_and_scales_the_cotangent_bitwise():
    from deepphysinet_amd.balance import group_map
    rng = np.random.default_rng(11)
    for groups, K in (('equations', 7), ('parts', 3)):
        tmap = group_map(groups)
        for trial in range(4):
            terms = (10.0 ** rng.uniform(-7.0, 14.0, 13)).astype(np.float32)           # the loss factors' span
            lam = (10.0 ** rng.uniform(-3.0, 3.0, K)).astype(np.float32)
            cot_in = np.float32(rng.uniform(0.1, 3.0))
            total, cot = _call_combine(terms, lam, tmap, float(cot_in))
            acc = lam[tmap[12]] * terms[12]                                              # numpy fp32 scalars: every product and sum rounded once
            for i in range(12):
                acc = np.float32(acc + np.float32(lam[tmap[i]] * terms[i]))
            assert total.view(np.uint32) == np.float32(acc).view(np.uint32), (groups, trial, total, acc)
            want = np.asarray([np.float32(cot_in * lam[tmap[i]]) for i in range(13)], dtype=np.float32)
            assert (cot.view(np.uint32) == want.view(np.uint32)).all()
        # every lambda 1.0f: the cotangent goes through unchanged to all 13 slots
        total, cot = _call_combine(terms, np.ones(K, dtype=np.float32), tmap, 0.3)
        assert (cot.view(np.uint32) == np.float32(0.3).view(np.uint32)).all() and cot.shape == (13,)


def test_balanced_total_is_an_autograd_function_over_the_combine():
    from deepphysinet_amd.point_path import balanced_total
    dev = _dev()
    it = torch.rand(6, device=dev).requires_grad_(True)
    mt = torch.rand(6, device=dev).requires_grad_(True)
    d = torch.rand((), device=dev).requires_grad_(True)
    lam = torch.tensor([0.5, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], device=dev)
    total = balanced_total(it, mt, d, lam, 'equations')
    g_it, g_mt, g_d = torch.autograd.grad(total, [it, mt, d], grad_outputs=torch.tensor(2.0, device=dev))
    assert torch.equal(g_it, 2.0 * lam[1:]) and torch.equal(g_mt, 2.0 * lam[1:]) and torch.equal(g_d, 2.0 * lam[0]) and g_d.shape == d.shape
    want = (lam[0] * d + (lam[1:] * it).sum() + (lam[1:] * mt).sum()).item()
    assert abs(total.item() - want) <= 16 * 2.0 ** -24 * want
    with pytest.raises(ValueError):
        balanced_total(it, mt, d, lam, 'parts')                                          # seven weights for three terms
    with pytest.raises(ValueError):
        balanced_total(it, mt, d, lam.double(), 'equations')


# ------------------------------------------------------------------------------------------------ 4, 5. the step
def _batch(n_inter=257, n_margin=300, seed=3):
    from deepphysinet_amd.sampler import SyntheticSamples
    return SyntheticSamples(_dev(), n_margin=n_margin, n_inter=n_inter, leads=2, seed=seed)[0]


def _own_norms(m, batch, groups, causal=None):
    """The K gradient norms formed by the test: step_losses on the batch and the model's weights, torch.autograd.grad of each group's terms over all
    parameters, the sum of squares in torch fp64.  -> (norms [K], the 13 terms in dpn_balance_combine's order as fp32, the number of parameter
    elements)."""
    from deepphysinet_amd.point_path import step_losses
    lf = m.train_cfg['losses']['loss_factor']
    net = m.physics_net
    params = list(net.parameters())
    assert len(params) == 155
    cfg = m.point_config(lf)
    n_inter, pts = m._eval_inputs(batch, True)
    norms = []
    for k in range(7 if groups == 'equations' else 3):
        net.clear_field_cache()
        meta_out = net.encode_field(batch['field_data'], batch['forecast_h'])
        heads, evec, statics = net.field_weights(batch['field_data'], batch['forecast_h'], meta_out=meta_out)
        it, _, mt, _, data = step_losses(cfg, n_inter, *pts, batch['margin_data'], heads, evec, statics, beta=0.1, margin_factor=lf['margin_factor'],
                                         inter_weights=batch.get('inter_w'), causal=causal)
        term = data if k == 0 else (it[k - 1] + mt[k - 1] if groups == 'equations' else (it, mt)[k - 1].sum())
        grads = torch.autograd.grad(term, params, allow_unused=True)
        norms.append(float(sum(g.double().pow(2).sum() for g in grads if g is not None).sqrt()))
    terms = torch.cat([it.detach().reshape(6), mt.detach().reshape(6), data.detach().reshape(1)]).float().cpu().numpy()
    net.clear_field_cache()
    return np.asarray(norms), terms, sum(p.numel() for p in params)


@pytest.mark.parametrize('groups,weighted', [('equations', False), ('parts', False), ('equations', True)])
def test_a_refresh_step_measures_the_terms_gradient_norms_and_sets_lambda_by_the_rule(groups, weighted):
    """257 interior + 300 margin points, hi+lo mode; `weighted`: the step composes with causal time weights and the batch's inter_w.
    diag's n_k against the norms the test forms itself: 1e-6 relative (the gradients come from the same deterministic kernels; only the summation
    differs).  lambda against update_reference of those norms: test 2's bound, 2^-23, plus what the two summation orders can move the fp64 target
    by before it is rounded to fp32 -- each sum of N squares is within N 2^-53 of the exact one (test 1's argument), a norm within half of that,
    lambda-hat = mean / n_k a ratio of such norms: 4 N 2^-53 covers both sides (N = 6.6e6 parameter elements: 3e-9).  lambda against
    update_reference of diag's own n_k squared: 2^-23 (n_k^2 is within two fp64 roundings of the sum the kernel read).  train_loss: bitwise the fp32
    loop over the 13 terms of the test's own step_losses call in the stated order, under the lambda read back."""
    from deepphysinet_amd.balance import LossBalance, update_reference
    from deepphysinet_amd.causal import CausalWeights
    m = _model('fill')
    batch = dict(_batch())
    causal = None
    if weighted:
        causal = CausalWeights(eps=1.0, bins=8)
        batch['inter_w'] = (0.25 + torch.rand(257, generator=torch.Generator().manual_seed(7))).to(_dev())
    own, terms, n_elem = _own_norms(m, batch, groups, causal)   # before an optimiser exists: the gradients are ordinary tensors
    before = [p.detach().clone() for p in m.physics_net.parameters()]
    opt = m.build_optimizer()
    bal = LossBalance(every=1, momentum=0.0, groups=groups)
    K = bal.n_terms
    loss, parts, gnorm = m.training_step(batch, opt, with_pde=True, causal=causal, balance=bal)
    st = m.loss_balance_state
    diag = st['diag'].cpu().numpy()
    assert diag.shape == (3 * K + 2,) and st['step'] == 1 and st['groups'] == groups and st['lam'].dtype == torch.float32
    print('%s%s: n_k %s, own %s, max rel %.3g, lambda %s' % (groups, ' + causal + inter_w' if weighted else '', diag[:K], own,
                                                            (np.abs(diag[:K] - own) / own).max(), diag[2 * K:3 * K]))
    assert (own > 0.0).all() and (np.abs(diag[:K] - own) <= 1e-6 * own).all()
    ones = np.ones(K, dtype=np.float32)
    want, flag = update_reference(own ** 2, ones, 0.0, bal.lam_min, bal.lam_max)
    lam = st['lam'].cpu().numpy()
    assert flag == 0 and diag[3 * K + 1] == 0.0 and (lam.astype(np.float64) == diag[2 * K:3 * K]).all()
    assert (np.abs(lam.astype(np.float64) - want) <= (U32 + 4 * n_elem * U64) * want).all(), (lam, want)
    want_diag, flag = update_reference(diag[:K] ** 2, ones, 0.0, bal.lam_min, bal.lam_max)
    assert flag == 0 and (np.abs(lam.astype(np.float64) - want_diag) <= U32 * want_diag).all(), (lam, want_diag)
    assert (lam > bal.lam_min).any() and (lam < bal.lam_max).any() and not (lam == 1.0).all()
    # the step itself: the balanced total under the new lambda, the unweighted parts, parameters moved
    tmap = bal.term_map()
    acc = lam[tmap[12]] * terms[12]                             # numpy fp32 scalars: every product and sum rounded once
    for i in range(12):
        acc = np.float32(acc + np.float32(lam[tmap[i]] * terms[i]))
    got = np.float32(float(loss))
    print('train_loss %.9g, the loop over the 13 terms %.9g' % (got, acc))
    assert got.view(np.uint32) == np.float32(acc).view(np.uint32)
    vals = {k: float(v) for k, v in parts.items()}
    assert set(vals) == {'margin_loss', 'inter_pde_loss', 'margin_pde_loss'} and torch.isfinite(loss)
    assert vals['margin_loss'] == float(terms[12])              # the parts stay unweighted
    assert abs(vals['inter_pde_loss'] - float(terms[:6].astype(np.float64).sum())) <= 8 * 2.0 ** -24 * vals['inter_pde_loss']
    if weighted:
        assert set(m.last_causal) == {'inter', 'margin'}
    moved = sum(int(not torch.equal(p, q)) for p, q in zip(m.physics_net.parameters(), before))
    assert moved > 0 and all(torch.isfinite(p).all() for p in m.physics_net.parameters()) and torch.isfinite(torch.as_tensor(gnorm)).all()


def test_with_momentum_one_lambda_stays_one_and_the_step_is_the_plain_step():
    """train_loss within 4 * 2^-24 relative of the plain step's (thirteen fp32 terms added instead of three; measured 1.5e-7).  The gradient norm and
    every parameter after the step are bitwise the plain step's: with lambda = 1.0f the 13 cotangents are the incoming one, and the residual
    kernel's per-term cotangent gl[e] + 0 equals its total cotangent 0 + gtot (the bound asked for was 1e-6 relative; bitwise is what holds)."""
    from deepphysinet_amd.balance import LossBalance
    out = []
    for bal in (None, LossBalance(every=1, momentum=1.0)):
        m = _model('fill')
        batch = _batch()
        opt = m.build_optimizer()
        kw = {} if bal is None else {'balance': bal}
        loss, parts, gnorm = m.training_step(batch, opt, with_pde=True, **kw)
        out.append((m, loss, parts, torch.as_tensor(gnorm).clone()))
    (m0, loss0, parts0, gnorm0), (m1, loss1, parts1, gnorm1) = out
    assert m0.loss_balance_state is None and (m1.loss_balance_state['lam'] == 1.0).all() and m1.loss_balance_state['diag'][-1] == 0.0
    rel = abs(float(loss1) - float(loss0)) / float(loss0)
    print('train_loss %.9g against %.9g: %.3g relative (bound %.3g); gnorm %.9g against %.9g'
          % (float(loss1), float(loss0), rel, 4 * 2.0 ** -24, float(gnorm1), float(gnorm0)))
    assert rel <= 4 * 2.0 ** -24
    for k in parts0:
        assert torch.equal(parts1[k], parts0[k]), k                                   # the parts stay the unweighted three
    assert torch.equal(gnorm1, gnorm0)
    for (name, p), q in zip(m1.physics_net.named_parameters(), m0.physics_net.parameters()):
        assert torch.equal(p, q), name


# ------------------------------------------------------------------------------------------------ 6. the option off is undisturbed
class _Spy:
    """Counts calls of the new entry points of the loaded library, tagged with the step the test says it is in."""

    def __init__(self):
        _, self.lib = _lib()
        self.inner = {k: getattr(self.lib, k) for k in NEW}
        self.calls = []
        self.step = None

    def __enter__(self):
        for k in NEW:
            setattr(self.lib, k, (lambda name: lambda *a: (self.calls.append((name, self.step)), self.inner[name](*a))[1])(k))
        return self

    def __exit__(self, *exc):
        for k in NEW:
            setattr(self.lib, k, self.inner[k])


def test_the_new_kernels_run_only_with_the_option_and_the_update_only_on_refresh_steps(tmp_path):
    from deepphysinet_amd.balance import LossBalance
    from deepphysinet_amd.sampler import SyntheticSamples
    with _Spy() as spy:
        # the option off: the loop (data-only step 1, PDE steps 2 and 3, log steps, validation) and the step itself call none of them
        m = _model('fill')
        m.train_cfg.setdefault('log', {})['log_step'] = 2
        src = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=4, seed=0)
        val = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=2, seed=1)
        out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path / 'off'), max_steps=3, num_epoch=1, pde_start_step=1)
        assert out['global_step'] == 3 and spy.calls == [] and m.loss_balance_state is None
        events = [json.loads(l) for l in open(tmp_path / 'off' / 'metrics.jsonl')]
        assert all('balance_lambda' not in e and 'balance_norm' not in e for e in events)
        opt = out['optimizer']
        m.training_step(src[0], opt, with_pde=True)
        m.training_step(src[0], opt, with_pde=False, balance=LossBalance(every=1))           # without the PDE losses the option is ignored
        assert spy.calls == [] and m.loss_balance_state is None
        # every = 3 over 7 steps
        bal = LossBalance(every=3, groups='parts')
        for step in range(1, 8):
            spy.step = step
            m.training_step(src[step % 4], opt, with_pde=True, balance=bal)
        by = lambda name: [s for n, s in spy.calls if n == name]
        assert by('dpn_balance_update') == [1, 4, 7]
        assert by('dpn_balance_sumsq') == [1] * 3 + [4] * 3 + [7] * 3                         # K = 3 sums per refresh
        assert by('dpn_balance_combine') == [s for s in range(1, 8) for _ in range(2)]        # one launch per direction, every step
        assert m.loss_balance_state['step'] == 7


# ------------------------------------------------------------------------------------------------ 7. the loop
def test_the_loop_logs_lambda_and_a_resume_continues_with_the_saved_weights_and_counter(tmp_path):
    from deepphysinet_amd.sampler import SyntheticSamples
    src = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=4, seed=0)
    val = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=2, seed=1)
    ckpt = str(tmp_path / 'ckpt')
    m = _model('fill')
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path / 'log'), checkpoint_path=ckpt, max_steps=4, num_epoch=1,
                                pde_start_step=0, balance_losses={'every': 2})
    assert out['global_step'] == 4 and torch.isfinite(out['last']['loss'])
    events = [json.loads(l) for l in open(tmp_path / 'log' / 'metrics.jsonl') if '"training"' in l]
    assert [e['global_step'] for e in events] == [1, 3]
    for e in events:
        assert len(e['balance_lambda']) == 7 and len(e['balance_norm']) == 7
        assert np.isfinite(e['balance_lambda']).all() and np.isfinite(e['balance_norm']).all() and min(e['balance_lambda']) > 0.0
    assert events[0]['balance_lambda'] != [1.0] * 7                                          # step 1 refreshed
    saved = m.loss_balance_state
    assert saved['step'] == 4 and saved['groups'] == 'equations'
    # a resume: the checkpoint's lambda and counter, bitwise; with every = 3 the counter 4 means no refresh on the resumed step, lambda stays
    m2 = _model('fill')
    m2.load_model(ckpt, prefix='physics')
    assert m2.loss_balance_state['step'] == 4 and torch.equal(m2.loss_balance_state['lam'].cpu(), saved['lam'].cpu())
    m3 = _model('fill')
    out3 = m3.run_train_interface(samples=src, checkpoint_path=ckpt, max_steps=5, num_epoch=2, pde_start_step=0, balance_losses={'every': 3})
    assert out3['global_step'] == 5 and m3.loss_balance_state['step'] == 5
    assert torch.equal(m3.loss_balance_state['lam'].cpu(), saved['lam'].cpu()) and m3.loss_balance_state['lam'].is_cuda
    # a run without the option does not carry the checkpoint's weights along
    m4 = _model('fill')
    m4.run_train_interface(samples=src, checkpoint_path=ckpt, max_steps=5, num_epoch=2, pde_start_step=0)
    assert m4.loss_balance_state is None


# ------------------------------------------------------------------------------------------------ 8. two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


_RANK_SCRIPT = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from deepphysinet_amd import distributed as D
from deepphysinet_amd.balance import LossBalance
from deepphysinet_amd.configs import ncep_config
from deepphysinet_amd.interface import builder_models
from deepphysinet_amd.sampler import SyntheticSamples
from oracle.fill import fill_state_dict_
rank, world, _ = D.init_from_env('gloo')          # two ranks share the one GPU of the test box: gloo carries the collectives through the host
dev = torch.device('cuda:0')
m = builder_models(**ncep_config(), precision='bf16x2')
sd = m.physics_net.state_dict(); fill_state_dict_(sd); m.physics_net.load_state_dict(sd)
m = m.to(dev)
D.broadcast_parameters(m.physics_net)
opt = m.build_optimizer()
sync = D.GradientAllReduce(opt)
batch = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=2, seed=10 + rank)[rank]        # each rank: its own field sample and points
m.training_step(batch, opt, with_pde=True, grad_sync=sync, balance=LossBalance(every=1, momentum=0.5))
torch.cuda.synchronize()
st = m.loss_balance_state
np.savez({out!r} % rank, lam=st['lam'].cpu().numpy(), diag=st['diag'].cpu().numpy(), field=batch['field_data'].cpu().numpy())
torch.distributed.barrier()
torch.distributed.destroy_process_group()
'''


def test_two_ranks_fed_different_batches_hold_the_same_lambda_after_a_refresh(tmp_path):
    script = tmp_path / 'rank.py'
    pattern = str(tmp_path / 'balance_rank%d.npz')
    script.write_text(_RANK_SCRIPT.format(root=ROOT, out=pattern))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [np.load(pattern % k) for k in range(2)]
    assert not np.array_equal(got[0]['field'], got[1]['field'])                             # the ranks were fed different batches
    assert got[0]['lam'].shape == (7,) and got[0]['lam'].dtype == np.float32
    assert np.array_equal(got[0]['lam'].view(np.uint32), got[1]['lam'].view(np.uint32))      # bitwise the same lambda
    assert np.array_equal(got[0]['diag'], got[1]['diag']) and got[0]['diag'][-1] == 0.0
    assert np.isfinite(got[0]['lam']).all() and not (got[0]['lam'] == 1.0).all()
