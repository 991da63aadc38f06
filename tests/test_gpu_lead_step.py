"""GPU (MI355X): the trained lead-batch step -- dpn_step_residual / dpn_step_finish_batch through the C ABI, point_path.step_losses_batch,
InterfacePhysics.training_step_batch, the loops' lead_batch option and train.py --lead_batch.

Yardsticks: today's launches of one field's step (dpn_residual per group, dpn_residual_finish, dpn_smooth_l1), bitwise wherever the new kernels form
the same sums in the same order; step_losses / training-step bodies run sample by sample.

Bounds that are not bitwise:
  column 6 of a block row   an fp64 sum of at most 256 * 6 non-negative fp32 values in a fixed order, against numpy's fp64 sum of the same values: both
                            are within 1536 * 2^-53 = 1.7e-13 of the exact sum; 1e-12 relative.
  the data loss             S / (6 n_m) in fp64 from two different fp64 orders (2e-13 apart at most), then ONE rounding to fp32 on either side: the two
                            fp32 values are equal or neighbours; times the same fp32 factor: 2 ulp = 2.4e-7 relative.
  gradients                 the bars of tests/test_gpu_step.py::test_lead_batch_backward_paths_agree (2e-5 of each tensor's maximum: the eager path
                            multiplies by the cotangent after the reductions) and ::test_config2_lead_batch_in_one_step_equals_the_loop."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import TOL
from tests.test_gpu_adaptive import _dev, _model
from tests.test_gpu_causal import _cfg, _fields, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ((1, 1), (255, 257), (256, 256), (300, 513))          # one point per group; the ragged last block on either side of the boundary; exact multiples
CASES = ('mse', 'l1', 'sl1', 'sum', 'noclip', 'sq')
BETA, MARGIN_FACTOR = 0.1, 3.0

_cache = {}


def _case_cfg(case):
    return _cfg('mse', reduce_sum=True) if case == 'sum' else _cfg(case)


def _labels(n_m, seed=0):
    key = ('lab', n_m, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(100 + seed)
        # around the fields' own scale, so that both branches of SmoothL1(0.1) occur
        _cache[key] = (torch.randn(n_m, 6, generator=g) * 0.3).to(_dev())
    return _cache[key]


def _blocks(k):
    return (k + 255) // 256


def _step_residual(cfg, F, labels, n_inter, gtot, grad=True, fill=-7.0, **bad):
    """dpn_step_residual on pre-filled buffers -> (rc, rows [blocks, 7], g_out, g_jxi).  bad: arguments replaced for the refusal cases."""
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    n, dev = F['n'], _dev()
    geo, ph = cfg.geometry(), cfg.physics()
    if 'criterion' in bad:
        ph.criterion = bad['criterion']
    if 'phys_beta' in bad:
        ph.beta = bad['phys_beta']
    n_inter_arg, n_arg = bad.get('n_inter_arg', n_inter), bad.get('n_arg', n)
    rows = torch.full((_blocks(n_inter) + _blocks(n - n_inter), 7), fill, dtype=torch.float64, device=dev)
    g_out, g_jxi = torch.full((n, 6), fill, device=dev), torch.full((n, 6, 3), fill, device=dev)
    gt = torch.tensor([gtot], dtype=torch.float32, device=dev)
    ptrs = dict(out_n=_ptr(F['out_n']), jac_n=_ptr(F['jac_n']), f=_ptr(F['f']), labels=_ptr(labels), gtot=_ptr(gt), rows=_ptr(rows),
                g_out=_ptr(g_out) if grad else None, g_jxi=_ptr(g_jxi) if grad else None)
    for k in bad.get('null', ()):
        ptrs[k] = None
    rc = lib.dpn_step_residual(ptrs['out_n'], ptrs['jac_n'], ptrs['f'], ptrs['labels'], n_inter_arg, n_arg, ctypes.byref(geo), ctypes.byref(ph),
                               bad.get('beta', BETA), MARGIN_FACTOR / (6.0 * (n - n_inter)), ptrs['gtot'], ptrs['rows'], ptrs['g_out'], ptrs['g_jxi'],
                               _stream())
    return rc, rows, g_out, g_jxi


def _todays_launches(cfg, F, labels, n_inter, gtot):
    """One field's step as it is launched today: dpn_residual per group (block rows and the cotangents of gtot), dpn_smooth_l1 for the data sums,
    dpn_smooth_l1(accumulate) for the data cotangent -> (rows_inter [b, 6], rows_margin [b, 6], dsum, g_out, g_jxi)."""
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    n, dev = F['n'], _dev()
    n_m = n - n_inter
    geo, ph = cfg.geometry(), cfg.physics()
    gt = torch.tensor([gtot], dtype=torch.float32, device=dev)
    g_out, g_jxi = torch.full((n, 6), -7.0, device=dev), torch.full((n, 6, 3), -7.0, device=dev)
    sums = []
    for a0, m in ((0, n_inter), (n_inter, n_m)):
        s = torch.empty((_blocks(m), 6), dtype=torch.float64, device=dev)
        L.check(lib.dpn_residual(_ptr(F['out_n'][a0:]), _ptr(F['jac_n'][a0:]), _ptr(F['f'][a0:]), m, ctypes.byref(geo), ctypes.byref(ph), None, _ptr(gt),
                                 _ptr(s), _ptr(g_out[a0:]), _ptr(g_jxi[a0:]), _stream()), 'dpn_residual')
        sums.append(s)
    dsum = torch.empty(_blocks(n_m * 6), dtype=torch.float64, device=dev)
    L.check(lib.dpn_smooth_l1(_ptr(F['out_n'][n_inter:]), _ptr(labels), n_m, BETA, 1.0, _ptr(dsum), None, 0, None, _stream()), 'dpn_smooth_l1')
    L.check(lib.dpn_smooth_l1(_ptr(F['out_n'][n_inter:]), _ptr(labels), n_m, BETA, MARGIN_FACTOR / (6.0 * n_m), None, _ptr(g_out[n_inter:]), 1, _ptr(gt),
                              _stream()), 'dpn_smooth_l1(grad)')
    return sums[0], sums[1], dsum, g_out, g_jxi


def _smooth_l1_host(out_n, labels):
    """The fp32 per-element SmoothL1(BETA) values [n_m, 6], formed on the host by the kernel's fp32 operations."""
    o, l = out_n.cpu().numpy().astype(np.float32), labels.cpu().numpy().astype(np.float32)
    d = o - l
    ad, beta = np.abs(d), np.float32(BETA)
    return np.where(ad < beta, np.float32(0.5) * d * d / beta, ad - np.float32(0.5) * beta).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), '%s: %d of %d elements differ, first at %s' % (what, int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())


# ------------------------------------------------------------------------------------------------ 1. dpn_step_residual
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('split', SPLITS, ids=lambda s: '%d+%d' % s)
def test_step_residual_equals_todays_launches(split, case):
    n_inter, n_m = split
    cfg, F, labels = _case_cfg(case), _fields(n_inter + n_m), _labels(n_m)
    per_elem = _smooth_l1_host(F['out_n'][n_inter:], labels).astype(np.float64)
    for gtot in (1.0, 0.37):
        rc, rows, g_out, g_jxi = _step_residual(cfg, F, labels, n_inter, gtot)
        assert rc == 0
        r_i, r_m, _, g_out_ref, g_jxi_ref = _todays_launches(cfg, F, labels, n_inter, gtot)
        nb_i = _blocks(n_inter)
        _same_bits(rows[:nb_i, :6], r_i, 'interior block rows')
        _same_bits(rows[nb_i:, :6], r_m, 'margin block rows')
        _same_bits(g_out, g_out_ref, 'g_out (gtot %g)' % gtot)
        _same_bits(g_jxi, g_jxi_ref, 'g_jxi (gtot %g)' % gtot)
        col6 = rows[:, 6].cpu().numpy()
        assert (col6[:nb_i] == 0.0).all() and not np.signbit(col6[:nb_i]).any()
        host = np.array([per_elem[256 * j:256 * (j + 1)].sum() for j in range(_blocks(n_m))])
        print('column 6:', col6[nb_i:], 'host:', host)
        np.testing.assert_allclose(col6[nb_i:], host, rtol=1e-12, atol=0.0)
    # rows without cotangents: the same rows, the cotangent buffers untouched
    rc, rows2, g_out, g_jxi = _step_residual(cfg, F, labels, n_inter, 1.0, grad=False)
    assert rc == 0 and bool((g_out == -7.0).all()) and bool((g_jxi == -7.0).all())
    _same_bits(rows2, rows, 'rows of a call without cotangents')


def test_step_residual_refuses_bad_arguments_and_writes_nothing():
    n_inter, n_m = 255, 257
    cfg, F, labels = _case_cfg('mse'), _fields(n_inter + n_m), _labels(n_m)
    L, lib = _lib()
    bad = [dict(null=(k,)) for k in ('out_n', 'jac_n', 'f', 'labels', 'gtot', 'rows', 'g_jxi')]
    bad += [dict(n_inter_arg=0), dict(n_inter_arg=-3), dict(n_inter_arg=n_inter + n_m), dict(n_inter_arg=n_inter + n_m + 1), dict(n_arg=0), dict(criterion=3),
            dict(criterion=-1), dict(criterion=L.CRIT_SMOOTH_L1, phys_beta=0.0), dict(beta=0.0), dict(beta=-0.1), dict(beta=float('nan'))]
    for b in bad:
        rc, rows, g_out, g_jxi = _step_residual(cfg, F, labels, n_inter, 1.0, **b)
        assert rc == -1, b
        assert bool((rows == -7.0).all()) and bool((g_out == -7.0).all()) and bool((g_jxi == -7.0).all()), b
    assert lib.dpn_step_rows_doubles(255, 512) == 21 and lib.dpn_step_rows_doubles(0, 512) == 0 and lib.dpn_step_rows_doubles(512, 512) == 0


# ------------------------------------------------------------------------------------------------ 2. dpn_step_finish_batch
def _finish_reference(cfg, rows, n_inter, n):
    """[14] = two dpn_residual_finish calls on one field's rows [blocks, 7] (its columns 0..5, group by group)."""
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    ph = cfg.physics()
    out = torch.empty(14, dtype=torch.float32, device=_dev())
    nb_i = _blocks(n_inter)
    for g, (part, m) in enumerate(((rows[:nb_i, :6], n_inter), (rows[nb_i:, :6], n - n_inter))):
        L.check(lib.dpn_residual_finish(_ptr(part.contiguous()), m, ctypes.byref(ph), _ptr(out[7 * g:]), _stream()), 'dpn_residual_finish')
    return out


def _host_finish(cfg, rows, n_inter, n):
    """The package's numpy restatement of the finish kernel on one field's rows: all 16 values (the same orders of addition, so bitwise)."""
    from deepphysinet_amd.lead_step import finish_reference
    return torch.from_numpy(finish_reference(rows.cpu().numpy(), n_inter, n, cfg.factors, MARGIN_FACTOR, reduce_sum=cfg.reduce_sum))


def _finish(cfg, rows, n_inter, n, B, **bad):
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    ph = cfg.physics()
    losses = torch.full((B, 16), -7.0, dtype=torch.float32, device=_dev())
    rc = lib.dpn_step_finish_batch(None if bad.get('null') == 'rows' else _ptr(rows), bad.get('n_inter_arg', n_inter), n, bad.get('B_arg', B), ctypes.byref(ph),
                                   MARGIN_FACTOR, None if bad.get('null') == 'losses' else _ptr(losses), _stream())
    return rc, losses


@pytest.mark.parametrize('case', ('mse', 'sum'))
@pytest.mark.parametrize('B', (1, 3))
def test_step_finish_batch_equals_two_finish_calls_per_field(B, case):
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    cfg = _case_cfg(case)
    for n_inter, n_m in SPLITS:
        n = n_inter + n_m
        F = _fields(n)
        rows, dsums = [], []
        for b in range(B):
            labels = _labels(n_m, seed=b)
            rc, r, _, _ = _step_residual(cfg, F, labels, n_inter, 1.0, grad=False)
            assert rc == 0
            rows.append(r)
            dsums.append(_todays_launches(cfg, F, labels, n_inter, 1.0)[2])
        rows = torch.stack(rows).contiguous()
        assert rows[0].numel() == lib.dpn_step_rows_doubles(n_inter, n)
        rc, losses = _finish(cfg, rows, n_inter, n, B)
        assert rc == 0
        for b in range(B):
            _same_bits(losses[b, :14], _finish_reference(cfg, rows[b], n_inter, n), 'field %d, the 14 PDE values' % b)
            data = (dsums[b].sum() / (6.0 * n_m)).float() * MARGIN_FACTOR
            print('data loss', float(losses[b, 14]), 'reference', float(data))
            assert abs(float(losses[b, 14]) - float(data)) <= 2.4e-7 * abs(float(data))
            _same_bits(losses[b, 15], (losses[b, 14] + losses[b, 6]) + losses[b, 13], 'field %d, the total' % b)
            _same_bits(losses[b].cpu(), _host_finish(cfg, rows[b], n_inter, n), 'field %d against lead_step.finish_reference' % b)
    for b in (dict(null='rows'), dict(null='losses'), dict(n_inter_arg=0), dict(n_inter_arg=n), dict(B_arg=0)):
        rc, losses = _finish(cfg, rows, n_inter, n, B, **b)
        assert rc == -1 and bool((losses == -7.0).all()), b


def test_step_finish_batch_adds_more_than_64_block_rows_in_the_order_of_residual_finish():
    """Lane l takes rows l, l + 64, ...: only more than 64 blocks per group (16 384 points) reach the second round.  Rows made up here: the finish
    launches read nothing else."""
    cfg = _case_cfg('mse')
    n_inter, n_m = 70 * 256 - 3, 130 * 256 - 200
    n, B = n_inter + n_m, 2
    g = torch.Generator().manual_seed(5)
    rows = (torch.rand(B, 200, 7, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 7, (B, 200, 7), generator=g).double()).to(_dev())
    rc, losses = _finish(cfg, rows, n_inter, n, B)
    assert rc == 0
    for b in range(B):
        _same_bits(losses[b, :14], _finish_reference(cfg, rows[b], n_inter, n), 'field %d' % b)
        data = (rows[b, 70:, 6].sum() / (6.0 * n_m)).float() * MARGIN_FACTOR
        assert abs(float(losses[b, 14]) - float(data)) <= 2.4e-7 * abs(float(data))
        _same_bits(losses[b, 15], (losses[b, 14] + losses[b, 6]) + losses[b, 13], 'the total')
        _same_bits(losses[b].cpu(), _host_finish(cfg, rows[b], n_inter, n), 'field %d against lead_step.finish_reference' % b)


# ------------------------------------------------------------------------------------------------ 3. step_losses_batch
def _lead_samples(B, n_inter, n_margin, seed=3):
    """B training batches (distinct fields and lead times, equal point counts) of one synthetic source; made once per shape."""
    key = ('smp', B, n_inter, n_margin, seed)
    if key not in _cache:
        from deepphysinet_amd.sampler import SyntheticSamples
        src = SyntheticSamples(_dev(), n_margin=n_margin, n_inter=n_inter, leads=B, seed=seed)
        _cache[key] = [src[i] for i in range(B)]
    return _cache[key]


def _stacked(m, samples):
    parts = [m._eval_inputs(b, True) for b in samples]
    pts = tuple(torch.stack([p[1][c] for p in parts], dim=0) for c in range(5))
    return parts[0][0], pts, torch.stack([b['margin_data'] for b in samples], dim=0)


def test_step_losses_batch_equals_step_losses_per_field():
    from deepphysinet_amd import point_path as PP
    B, n_inter, n_margin = 3, 257, 300
    m = _model()
    samples = _lead_samples(B, n_inter, n_margin)
    assert len({float(b['forecast_h'].reshape(-1)[0]) for b in samples}) == B
    cfg = m.point_config(m.train_cfg['losses']['loss_factor'])
    with torch.no_grad():
        hw = [m.physics_net.field_weights(b['field_data'], b['forecast_h']) for b in samples]
    heads0, evec0 = torch.stack([h[0] for h in hw]), torch.stack([h[1] for h in hw])
    statics = [s_.detach().clone().requires_grad_(True) for s_ in hw[0][2]]
    n_i, pts, labels = _stacked(m, samples)
    w = torch.tensor([0.5, 2.0, 1.25], device=_dev())
    heads, evec = heads0.clone().requires_grad_(True), evec0.clone().requires_grad_(True)
    terms, parts, totals = PP.step_losses_batch(cfg, n_i, *pts, labels, heads, evec, statics, beta=BETA, margin_factor=MARGIN_FACTOR)
    assert terms.shape == (B, 2, 6) and parts.shape == (B, 3) and totals.shape == (B,)
    assert totals.requires_grad and not terms.requires_grad and not parts.requires_grad
    obj = (totals * w).sum()
    got = torch.autograd.grad(obj, [heads, evec, statics[0], statics[2]], retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        torch.autograd.grad(obj, [heads])
    # the same scalar from three step_losses calls
    heads_r, evec_r = heads0.clone().requires_grad_(True), evec0.clone().requires_grad_(True)
    ref_obj = 0.0
    for b in range(B):
        it, itot, mt, mtot, data = PP.step_losses(cfg, n_i, *(p[b] for p in pts), labels[b], heads_r[b], evec_r[b], statics, beta=BETA,
                                                  margin_factor=MARGIN_FACTOR)
        _same_bits(terms[b, 0], it.detach(), 'field %d interior terms' % b)
        _same_bits(terms[b, 1], mt.detach(), 'field %d margin terms' % b)
        _same_bits(parts[b, 1], itot.detach(), 'field %d interior total' % b)
        _same_bits(parts[b, 2], mtot.detach(), 'field %d margin total' % b)
        print('field %d data loss %r, step_losses %r' % (b, float(parts[b, 0]), float(data.detach())))
        assert abs(float(parts[b, 0]) - float(data.detach())) <= 2.4e-7 * abs(float(data.detach()))
        _same_bits(totals[b].detach(), (parts[b, 0] + parts[b, 1]) + parts[b, 2], 'field %d total' % b)
        ref_obj = ref_obj + w[b] * ((data + itot) + mtot)
    ref = torch.autograd.grad(ref_obj, [heads_r, evec_r, statics[0], statics[2]])
    for name, a_, b_ in zip(('heads', 'evec', 'static 0', 'static 2'), got, ref):
        d_ = float((a_ - b_).abs().max())
        print('%s: max difference %.3e of max %.3e' % (name, d_, float(b_.abs().max())))
        assert d_ <= 2e-5 * float(b_.abs().max()), name
    # no-grad: the same values, nothing saved, nothing to backpropagate
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        t2, p2, tot2 = PP.step_losses_batch(cfg, n_i, *pts, labels, heads, evec, statics, beta=BETA, margin_factor=MARGIN_FACTOR)
    assert not tot2.requires_grad
    _same_bits(t2.contiguous(), terms.contiguous(), 'no-grad terms')
    _same_bits(p2, parts, 'no-grad parts')
    _same_bits(tot2, totals.detach(), 'no-grad totals')
    del t2, p2, tot2
    assert torch.cuda.memory_allocated() <= before
    with pytest.raises(ValueError, match='n_inter'):
        PP.step_losses_batch(cfg, n_i, *pts, labels[:, 1:], heads, evec, statics)


# ------------------------------------------------------------------------------------------------ 4. training_step_batch
@pytest.mark.parametrize('with_pde', (True, False))
def test_training_step_batch_equals_the_loop_of_single_sample_steps(with_pde):
    from deepphysinet_amd import point_path as PP
    B = 5                                                    # 5 x 287 encoder rows: the batched encoder takes the long-reduction (split-K) path
    samples = _lead_samples(B, 128, 128, seed=7)
    ma, mb = _model(), _model()
    lf = ma.train_cfg['losses']['loss_factor']
    # A: one step on the five samples; lr 0, so that .grad survives the step
    opt = torch.optim.SGD(ma.physics_net.parameters(), lr=0.0)
    # (max_norm out of reach: clip_grad_norm_ would scale the gradients that are compared below; the clip itself is the fused optimiser's leg)
    loss, parts, gnorm, per = ma.training_step_batch(samples, opt, with_pde=with_pde, max_norm=1e30)
    assert ma.last_causal is None and per['totals'].shape == (B,) and per['totals'].is_cuda
    got = {n_: p.grad.detach().clone() for n_, p in ma.physics_net.named_parameters()}
    # B: the same loss accumulated sample by sample
    cfg = mb.point_config(lf)
    mb.physics_net.zero_grad(set_to_none=True)
    total, ref_parts = 0.0, []
    for k_, b in enumerate(samples):
        heads, evec, statics = mb.physics_net.field_weights(b['field_data'], b['forecast_h'])
        if with_pde:
            n_i, pts = mb._eval_inputs(b, True)
            it, itot, mt, mtot, data = PP.step_losses(cfg, n_i, *pts, b['margin_data'], heads, evec, statics, beta=0.1, margin_factor=lf['margin_factor'])
            _same_bits(per['terms'][k_, 0], it.detach(), 'sample %d interior terms' % k_)
            _same_bits(per['terms'][k_, 1], mt.detach(), 'sample %d margin terms' % k_)
            l_b = (data + itot) + mtot
            ref_parts.append(torch.stack((data, itot, mtot)).detach())
        else:
            l_b = mb.data_loss(b['margin_x'], b['margin_y'], b['margin_t'], b['field_data'], b['margin_input_data'], b['margin_data'], b['forecast_h'],
                               lf['margin_factor'])
            ref_parts.append(l_b.detach().reshape(1))
        (l_b / B).backward()
        total += float(l_b.detach()) / B
    print('with_pde %s: loss %r, loop %r' % (with_pde, float(loss), total))
    assert abs(float(loss) - total) <= 1e-6 * abs(total)
    ref_mean = torch.stack(ref_parts).mean(dim=0)
    assert list(parts) == ['margin_loss', 'inter_pde_loss', 'margin_pde_loss'][:3 if with_pde else 1]
    for i, k_ in enumerate(parts):
        assert abs(float(parts[k_]) - float(ref_mean[i])) <= 1e-6 * abs(float(ref_mean[i])), k_
    num = den = 0.0
    for n_, p in mb.physics_net.named_parameters():
        if n_.endswith('key_projection.bias'):
            continue
        a_, b_ = got[n_], p.grad
        d_ = (a_ - b_).abs()
        num += float(d_.double().pow(2).sum())
        den += float(b_.double().pow(2).sum())
        assert float(d_.max()) <= 0.02 * TOL['bf16x2']['grad'] * float(b_.abs().max()) + 1e-30, (n_, float(d_.max()), float(b_.abs().max()))
    print('all gradients: relative L2 difference %.3e' % (num / den) ** 0.5)
    assert (num / den) ** 0.5 <= 1e-5
    if not with_pde:
        return
    # the fused optimiser: the norm it clips by is the loop gradients' norm; the parameters move and stay finite
    loop_norm = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in mb.physics_net.parameters())))
    mc = _model()
    fused = mc.build_optimizer()
    before = [p.detach().clone() for p in mc.physics_net.parameters()]
    loss_c, _, gnorm_c, _ = mc.training_step_batch(samples, fused, with_pde=True)
    print('gnorm %r, loop gradients %r' % (float(gnorm_c), loop_norm))
    assert float(loss_c) == float(loss) and abs(float(gnorm_c) - loop_norm) <= 1e-5 * loop_norm
    after = list(mc.physics_net.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after) and any(not torch.equal(a_, b_) for a_, b_ in zip(before, after))
    # a list of one sample: the same path with B = 1
    md = _model()
    loss_1, parts_1, _, per_1 = md.training_step_batch(samples[:1], torch.optim.SGD(md.physics_net.parameters(), lr=0.0), with_pde=True)
    _same_bits(per_1['terms'][0], per['terms'][0], 'B = 1 terms')
    assert float(loss_1) == float(per_1['totals'][0])


# ------------------------------------------------------------------------------------------------ 5. a captured step
_CAPTURE = r'''
import sys
sys.path.insert(0, %r)
import torch
from tests.test_gpu_adaptive import _dev, _model
from deepphysinet_amd.sampler import SyntheticSamples
src = SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=2, seed=7)
samples = [src[0], src[1]]

def make():
    m = _model()
    opt = m.build_optimizer(lr=1e-3)
    return m, opt, lambda: m.training_step_batch(samples, opt, with_pde=True)[0]

m1, opt1, step1 = make()
eager = [float(step1()) for _ in range(2 + 3)]
m2, opt2, step2 = make()
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    for _ in range(2):
        step2()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    static_loss = step2()
replayed = []
for _ in range(3):
    graph.replay()
    torch.cuda.synchronize()
    replayed.append(float(static_loss))
assert int(opt1.step_count) == int(opt2.step_count) == 5, (int(opt1.step_count), int(opt2.step_count))
assert replayed == eager[2:], (replayed, eager)
for (n_, a_), (_, b_) in zip(m1.physics_net.named_parameters(), m2.physics_net.named_parameters()):
    assert torch.equal(a_, b_), n_
print('CAPTURE OK', replayed)
'''


def test_captured_training_step_batch_replays_equal_eager_steps():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, '-c', _CAPTURE % ROOT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and 'CAPTURE OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ 6. loop and launcher
def test_the_loop_groups_leads_counts_optimiser_steps_and_resumes(tmp_path):
    from deepphysinet_amd.sampler import SyntheticSamples
    src = SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=5)
    m = _model()
    seen, single = [], []
    batch_step, one_step = m.training_step_batch, m.training_step
    m.training_step_batch = lambda batches, *a, **k: (seen.append((len(batches), k.get('with_pde'))), batch_step(batches, *a, **k))[1]
    m.training_step = lambda *a, **k: (single.append(1), one_step(*a, **k))[1]
    ck = str(tmp_path / 'ck')
    out = m.run_train_interface(samples=src, lead_batch=2, pde_start_step=1, num_epoch=1, checkpoint_path=ck, device=str(_dev()))
    assert seen == [(2, False), (2, True), (1, True)] and single == [] and out['global_step'] == 3
    assert os.path.exists(os.path.join(ck, 'physics_latest.pth'))
    m2 = _model()
    seen2 = []
    step2 = m2.training_step_batch
    m2.training_step_batch = lambda batches, *a, **k: (seen2.append(len(batches)), step2(batches, *a, **k))[1]
    out2 = m2.run_train_interface(samples=src, lead_batch=2, pde_start_step=1, num_epoch=2, checkpoint_path=ck, device=str(_dev()))
    assert seen2 == [2, 2, 1] and out2['global_step'] == 6                   # resumed behind epoch 0: one more epoch of three steps
    for a_, b_ in zip(m.physics_net.parameters(), m2.physics_net.parameters()):
        assert a_.shape == b_.shape
    # lead_batch 1 / unset: the single-sample step, never the batched one
    for kw in (dict(lead_batch=1), dict()):
        m3 = _model()
        calls = []
        one3 = m3.training_step
        m3.training_step = lambda *a, **k: (calls.append(1), one3(*a, **k))[1]
        m3.training_step_batch = lambda *a, **k: pytest.fail('training_step_batch called with %r' % (kw,))
        out3 = m3.run_train_interface(samples=src, pde_start_step=1, num_epoch=1, max_steps=2, device=str(_dev()), **kw)
        assert calls == [1, 1] and out3['global_step'] == 2


def test_train_py_lead_batch_runs_end_to_end(tmp_path):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    ck = str(tmp_path / 'ck')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--checkpoint_path', ck, '--max_steps', '2', '--synthetic', '--lead_batch', '2'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'global_step 2' in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(ck, 'physics_latest.pth'))
