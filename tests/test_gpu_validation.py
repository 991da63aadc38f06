"""GPU (MI355X): the validation pass -- the label-evaluation kernel (csrc/dpn_eval.hip), the no-grad step (point_path.eval_step),
InterfacePhysics.validation_step / validate and the training loops' validation branch.
Reference: interface/interface_physics.py:518-530 (training batch's six errors), :629-745 (validation sample), fixture F14."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from oracle.fill import fill_state_dict_, synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ('u10', 'v10', 'pres', 't2', 'q2', 'rio')


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _model(seed=None, norm=None):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    if norm is not None:
        cfg['obs_norm_cfg'] = {k: dict(cfg['obs_norm_cfg'][k], **c) for k, c in zip(ORDER, norm)}
    if seed is not None:
        torch.manual_seed(seed)
    m = builder_models(**cfg, precision='bf16x2')
    if seed is None:
        sd = m.physics_net.state_dict()
        fill_state_dict_(sd)
        m.physics_net.load_state_dict(sd)
    return m.to(_dev())


def _batch(n_inter, n_margin, tag=''):
    inter = synthetic_inputs(n_inter, tag='inter' + tag)
    margin = synthetic_inputs(n_margin, tag='margin' + tag, margin=True)
    b = dict(field_data=inter['field_data'], forecast_h=inter['forecast_h'],
             margin_x=margin['x'], margin_y=margin['y'], margin_t=margin['t'], margin_f=margin['f'], margin_data=margin['labels'],
             margin_input_data=margin['coord_data'], inter_x=inter['x'], inter_y=inter['y'], inter_t=inter['t'], inter_f=inter['f'],
             inter_data=inter['coord_data'])
    return {k: v.to(_dev()) for k, v in b.items()}


# ------------------------------------------------------------------------------------------------ 6. the kernel alone
def _expected_stats(out_n, labels, norm_cfg, with_clip, beta=0.1):
    """torch on the same device tensors: every element-wise operation in fp32, one kernel per operation (nothing can be contracted), in the
    reference's order (inverse_norm :232-262, nn.MSELoss, SmoothL1 weights_loss.py:17-20); sums in fp64."""
    d = out_n - labels
    ad = d.abs()
    # (a tensor divisor: torch turns a division by a Python scalar into a multiplication by its rounded reciprocal, which is another fp32 operation)
    sl1 = torch.where(ad < beta, (0.5 * d) * d / torch.full_like(d, beta), ad - 0.5 * beta)
    rows = []
    for seg in range(out_n.shape[0]):
        p = O.inverse_norm([out_n[seg, :, k:k + 1] for k in range(6)], with_clip=with_clip, norm_cfg=norm_cfg)
        l = O.inverse_norm([labels[seg, :, k:k + 1] for k in range(6)], with_clip=with_clip, norm_cfg=norm_cfg)
        diff = torch.cat(p, 1) - torch.cat(l, 1)
        sq = diff * diff
        rows.append(torch.cat([sl1[seg].double().sum().reshape(1), sq.double().sum(0), diff.abs().double().sum(0), diff.double().sum(0),
                               diff.abs().max(0).values.double()]))
    return torch.stack(rows)


@pytest.mark.parametrize('norm', ['shipped', 'f12_norm_cfg', 'f12_norm_sq_cfg'])
@pytest.mark.parametrize('with_clip', [False, True])
def test_label_errors_kernel_against_torch(norm, with_clip):
    """Inputs are identical on both sides and every fp32 operation is rounded on its own on both sides, so the only admissible difference is the
    ORDER of an fp64 sum.  Bound: a sum of n terms in fp64 in any order is within (n - 1) u sum|x_i| of the exact one (u = 2^-53 = 1.1e-16); two orders
    differ by at most twice that.  sum d^2, sum |d| and the SmoothL1 sum have terms of one sign (sum|x_i| = the sum itself): 2 * 6 * 20 480 * 1.1e-16 =
    2.7e-11 worst case, and the error of pairwise / blocked sums grows like log n, not n: 1e-12 relative is asked.  sum d has mixed signs: the same
    bound holds relative to sum |d|.  Maxima and segment boundaries are exact."""
    from deepphysinet_amd.point_path import label_errors
    norm_cfg = None if norm == 'shipped' else getattr(O, norm)()
    m = _model(seed=1, norm=norm_cfg)
    cfg = m.point_config()
    g = torch.Generator().manual_seed(5)
    wide = 40.0 if with_clip else 1.0            # wide enough that about half of P, T, q, rho sit on a bound (as fixture F9's gain does)
    for shape in ((1, 1), (1, 70), (1, 256), (1, 1037), (1, 20480), (3, 1037)):
        out_n = (torch.randn(*shape, 6, generator=g) * wide).to(_dev())
        labels = (torch.randn(*shape, 6, generator=g) * wide).to(_dev())
        if with_clip and shape == (1, 20480):
            lo = torch.tensor(cfg.clip_lo, device=_dev())
            hi = torch.tensor(cfg.clip_hi, device=_dev())
            phys = torch.cat(O.inverse_norm([out_n[0, :, k:k + 1] for k in range(6)], with_clip=False, norm_cfg=norm_cfg), 1)
            frac = float(((phys[:, 2:] <= lo[2:]) | (phys[:, 2:] >= hi[2:])).float().mean())
            assert 0.2 < frac < 0.8, frac
        got = label_errors(cfg, out_n, labels, beta=0.1, with_clip=with_clip)
        want = _expected_stats(out_n, labels, norm_cfg if norm_cfg is not None else O.shipped_norm_cfg(), with_clip)
        assert got.shape == (shape[0], 25)
        assert torch.equal(got[:, 19:], want[:, 19:]), (shape, got[:, 19:], want[:, 19:])
        one_sign = torch.cat([got[:, :13], want[:, :13]])
        rel = ((got[:, :13] - want[:, :13]).abs() / want[:, :13].abs().clamp_min(1e-300)).max()
        rel_d = ((got[:, 13:19] - want[:, 13:19]).abs() / want[:, 7:13].clamp_min(1e-300)).max()
        print('label_errors %s clip %d %s: sums rel %.2e, sum d rel (to sum |d|) %.2e' % (norm, with_clip, shape, float(rel), float(rel_d)))
        assert float(rel) <= 1e-12 and float(rel_d) <= 1e-12, (shape, float(rel), float(rel_d))
        assert torch.isfinite(one_sign).all()
        assert torch.equal(got, label_errors(cfg, out_n, labels, beta=0.1, with_clip=with_clip))          # two runs
        if out_n.dim() == 3 and shape[0] == 1:                                                          # [N, 6] is the S = 1 case
            assert torch.equal(got, label_errors(cfg, out_n[0], labels[0], beta=0.1, with_clip=with_clip))
        if shape[0] == 3:
            # a segment never leaks into its neighbour: an offset of 1e6 on segment 1 leaves segments 0 and 2 bitwise unchanged; and every
            # segment equals the single-sample run of its own rows (an odd N puts segment 1 on an 8-byte boundary: the narrow loads)
            shifted = out_n.clone()
            shifted[1] += 1e6
            got2 = label_errors(cfg, shifted, labels, beta=0.1, with_clip=with_clip)
            assert torch.equal(got2[0], got[0]) and torch.equal(got2[2], got[2]) and not torch.equal(got2[1], got[1])
            for s_ in range(3):
                assert torch.equal(got[s_], label_errors(cfg, out_n[s_].clone(), labels[s_].clone(), beta=0.1, with_clip=with_clip)[0]), s_


def test_variable_errors_keys_and_values():
    m = _model(seed=1)
    g = torch.Generator().manual_seed(2)
    out_n, labels = torch.randn(1037, 6, generator=g).to(_dev()), torch.randn(1037, 6, generator=g).to(_dev())
    ve = m.variable_errors(out_n, labels)
    p = torch.cat(O.inverse_norm([out_n[:, k:k + 1] for k in range(6)], with_clip=False), 1).double()
    l = torch.cat(O.inverse_norm([labels[:, k:k + 1] for k in range(6)], with_clip=False), 1).double()
    assert tuple(ve) == ('u', 'v', 'p', 'T', 'q', 'rio')
    for k, v in enumerate(ve):
        d = p[:, k] - l[:, k]
        assert set(ve[v]) == {'mse', 'rmse', 'mae', 'bias', 'max_abs'}
        assert abs(ve[v]['mse'] - float((d * d).mean())) <= 1e-6 * float((d * d).mean())
        assert abs(ve[v]['rmse'] - ve[v]['mse'] ** 0.5) <= 1e-12 * ve[v]['rmse']
        assert abs(ve[v]['mae'] - float(d.abs().mean())) <= 1e-6 * float(d.abs().mean())
        assert abs(ve[v]['bias'] - float(d.mean())) <= 1e-6 * float(d.abs().mean())
        assert ve[v]['max_abs'] == float(d.float().abs().max()) or abs(ve[v]['max_abs'] - float(d.abs().max())) <= 1e-6 * float(d.abs().max())


# ------------------------------------------------------------------------------------------------ 7. the numbers the training step reports
@pytest.mark.parametrize('with_pde', [True, False])
@pytest.mark.parametrize('sizes', [(4096, 20480), (1037, 5197)])
def test_validation_step_reports_the_training_steps_numbers(with_pde, sizes):
    """validation_step(batch) before training_step(batch): same kernels, same tiles, same fixed-order sums -> the PDE totals and the twelve terms are
    torch.equal; margin_loss is equal or one fp32 ulp away (its fp64 block sums are partitioned into 512-point blocks here, 256-element blocks in
    dpn_smooth_l1, before the single rounding to fp32)."""
    from deepphysinet_amd.point_path import step_losses
    m = _model()
    b = _batch(*sizes)
    opt = m.build_optimizer()
    res = m.validation_step(b, with_pde=with_pde)
    terms = None
    if with_pde:                                  # the twelve terms of the very same parameters, through the training step's own function
        cfg = m.point_config()
        heads, evec, statics = m.physics_net.field_weights(b['field_data'], b['forecast_h'])
        n_i, pts = m._eval_inputs(b, True)
        ia, it, ma, mt, _ = step_losses(cfg, n_i, *pts, b['margin_data'], heads, evec, statics, beta=0.1,
                                        margin_factor=m.train_cfg['losses']['loss_factor']['margin_factor'])
        terms = torch.stack([ia.detach(), ma.detach()])
        m.physics_net.clear_field_cache()
    loss, parts, _ = m.training_step(b, opt, with_pde=with_pde)
    assert set(parts) == ({'margin_loss', 'inter_pde_loss', 'margin_pde_loss'} if with_pde else {'margin_loss'})
    if with_pde:
        assert torch.equal(res['inter_pde_loss'], parts['inter_pde_loss']) and torch.equal(res['margin_pde_loss'], parts['margin_pde_loss'])
        assert torch.equal(res['terms'], terms)
        assert torch.equal(it.detach(), parts['inter_pde_loss']) and torch.equal(mt.detach(), parts['margin_pde_loss'])
    else:
        assert res['terms'] is None and 'inter_pde_loss' not in res
    a, c = float(res['margin_loss']), float(parts['margin_loss'])
    ulp = float(np.spacing(np.float32(abs(c))))
    print('margin_loss validation %r training %r (ulp %g)' % (a, c, ulp))
    assert abs(a - c) <= ulp
    assert abs(float(res['valid_loss']) - float(loss)) <= 2 * float(np.spacing(np.float32(abs(float(loss)))))


# ------------------------------------------------------------------------------------------------ 8. against the reference (F14)
def test_f14_validation_against_the_reference(golden_dir):
    """Losses and terms at the bars test_gpu_parity.py holds for the same quantities (1e-4 on the PDE terms with its identified-flip rule and its cap
    of max(3, n / 150) removed points, _f14_terms; its DATA_LOSS_TOL = 5e-5 on the data loss) on 256 + 256 points, the inputs of F5 / F8 / F13.  Per-variable MSEs against the reference's fp64 ones: with the fields bar
    delta_k = 5e-5 max|out_n,k| every prediction moves by at most delta_k std_k in physical units, the mean square then by at
    most 2 delta_k std_k sqrt(mse_k) + (delta_k std_k)^2 (Cauchy-Schwarz; the clip is a contraction, so it holds clipped too), plus the distance
    of the reference's own fp32 run from its fp64 run.  Every number of the bar comes from the fixture."""
    d = np.load(os.path.join(golden_dir, 'f14_validation.npz'))
    n = int(d['n_points'])
    m = _model()
    b = _batch(n, n)
    std = np.array(m.point_config().std, np.float64)
    for with_pde in (True, False):
        pre = 'pde%d.' % int(with_pde)
        for clip, key in ((False, 'mse_noclip'), (True, 'mse')):          # the default, and what the reference's loop computes (it clips)
            res = m.validation_step(b, with_pde=with_pde, with_clip=clip)
            ref64 = d[key + '_fp64']
            fp32_gap = np.abs(d[pre + key] - ref64)
            delta = 5e-5 * d['out_n_abs_max'] * std
            bar = 2.0 * delta * np.sqrt(ref64) + delta ** 2 + fp32_gap
            mine = np.array([res['variables'][v]['mse'] for v in ('u', 'v', 'p', 'T', 'q', 'rio')])
            dist = np.abs(mine - ref64)
            print('F14 pde %d clip %d: |mse - fp64 reference| / bar = %s (relative distance %s)' % (with_pde, clip, dist / bar, dist / ref64))
            assert np.all(dist <= bar), (dist, bar)
        rel = abs(float(res['margin_loss']) - float(d[pre + 'margin_loss'])) / float(d[pre + 'margin_loss'])
        print('F14 pde %d: margin_loss rel %.2e' % (with_pde, rel))
        assert rel <= 5e-5                          # test_gpu_parity.py DATA_LOSS_TOL
        if with_pde:
            _f14_terms(m, d, pre, res, n)
        else:
            assert abs(float(res['valid_loss']) - float(d[pre + 'valid_loss'])) <= 5e-5 * float(d[pre + 'valid_loss'])


def _f14_terms(m, d, pre, res, n):
    """The rule of test_gpu_parity.py (test_grid_node_points_long_lead): 1e-4 per term against the REFERENCE's numbers for a group none of whose
    points carries a switch bit (ReLU / clip / vapour) that differs from the fp32 oracle arithmetic's; otherwise those points -- at most
    max(3, n / 150) -- are named and removed from both sides and the remaining points' terms are held to 1e-4 against the oracle (which
    tests/test_validation_cpu.py pins to this fixture), while the un-removed group stays within 1e-2."""
    from test_gpu_parity import _flipped_points, _without
    terms = res['terms'].double().cpu().numpy()
    rel_t = np.abs(terms - d[pre + 'terms']) / np.abs(d[pre + 'terms'])
    groups = (synthetic_inputs(n, tag='inter'), synthetic_inputs(n, tag='margin', margin=True))
    flips = [_flipped_points(m, inp)[0] for inp in groups]
    idx = [torch.nonzero(f).flatten().tolist() for f in flips]
    print('F14 terms rel (all points)', rel_t, 'points with a differing switch bit: interior %s, margin %s' % tuple(idx))
    assert np.all(rel_t <= 1e-2), rel_t
    assert all(len(i) <= max(3, n // 150) for i in idx), idx
    clean = True
    for gi, key in enumerate(('inter_pde_loss', 'margin_pde_loss')):
        if not idx[gi]:
            assert np.all(rel_t[gi] <= 1e-4), (key, rel_t[gi])
            assert abs(float(res[key]) - float(d[pre + key])) <= 1e-4 * float(d[pre + key]), key
        else:
            clean = False
    if clean:
        assert abs(float(res['valid_loss']) - float(d[pre + 'valid_loss'])) <= 1e-4 * float(d[pre + 'valid_loss'])
        return
    # the flip-free batch through validation_step itself, against the oracle on the same points
    sub = [_without(inp, f) if i else inp for inp, f, i in zip(groups, flips, idx)]
    inter, margin = ({k: v.to(_dev()) for k, v in g_.items()} for g_ in sub)
    b = dict(field_data=inter['field_data'], forecast_h=inter['forecast_h'],
             margin_x=margin['x'], margin_y=margin['y'], margin_t=margin['t'], margin_f=margin['f'], margin_data=margin['labels'],
             margin_input_data=margin['coord_data'], inter_x=inter['x'], inter_y=inter['y'], inter_t=inter['t'], inter_f=inter['f'],
             inter_data=inter['coord_data'])
    mine = m.validation_step(b)
    st = O.make_state()
    for gi, (inp, key) in enumerate(zip(sub, ('inter_pde_loss', 'margin_pde_loss'))):
        x, y, t = (inp[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
        total, parts, _, _ = O.place_one_batch(st, x, y, t, inp['f'], inp['field_data'], inp['coord_data'], inp['forecast_h'], O.Geometry(), return_parts=True)
        ref = np.array([float(p_.detach()) for p_ in parts])
        got = mine['terms'][gi].double().cpu().numpy()
        print('F14 %s without %s: rel %s' % (key, idx[gi], np.abs(got - ref) / np.abs(ref)))
        assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref)), (key, got, ref)
        assert abs(float(mine[key]) - float(total.detach())) <= 1e-4 * abs(float(total.detach())), key


# ------------------------------------------------------------------------------------------------ 9. no trace
def _snapshot(m, opt):
    snap = {'p.' + k: p.detach().clone() for k, p in m.physics_net.named_parameters()}
    snap.update({'g.' + k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.physics_net.named_parameters()})
    for i, (k, v) in enumerate(sorted(((str(k_), v_) for k_, v_ in opt.__dict__.items() if torch.is_tensor(v_)))):
        snap['o.%s' % k] = v.detach().clone()
    for i, st in enumerate(opt.state.values()):
        for k, v in st.items():
            if torch.is_tensor(v):
                snap['s.%d.%s' % (i, k)] = v.detach().clone()
    return snap


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), k


def test_validation_leaves_no_trace():
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model()
    opt = m.build_optimizer()
    b = _batch(300, 700)
    s0 = _snapshot(m, opt)                         # before any step: every .grad is None
    m.validation_step(b)
    _same(s0, _snapshot(m, opt))
    m.training_step(b, opt)
    s1 = _snapshot(m, opt)
    assert any(k.startswith(('o.', 's.')) for k in s1), 'the snapshot holds no optimiser state'
    m.validation_step(b)
    m.validation_step(b, with_pde=False)
    m.validate([b, _batch(300, 700, tag='2'), _batch(300, 700, tag='3')], lead_batch=2)
    _same(s1, _snapshot(m, opt))
    assert m.physics_net._meta_cache is None
    # six training steps on fixed batches, a validation after every second one: the parameters end where they end without validation
    finals = []
    for with_valid in (False, True):
        mm = _model()
        oo = mm.build_optimizer()
        for i in range(6):
            mm.training_step(_batch(300, 700, tag=str(i % 3)), oo)
            if with_valid and i % 2 == 1:
                mm.validation_step(_batch(300, 700, tag='v'))
                mm.validate([_batch(300, 700, tag='v'), _batch(300, 700, tag='w')], lead_batch=2)
        finals.append({k: p.detach().clone() for k, p in mm.physics_net.named_parameters()})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
    # a synthetic validation source owns its own CollocationSampler: drawing from it leaves the training source's draws what they are
    tr_a, tr_b = SyntheticSamples(_dev(), n_margin=256, n_inter=128, leads=2, seed=0), SyntheticSamples(_dev(), n_margin=256, n_inter=128, leads=2, seed=0)
    va = SyntheticSamples(_dev(), n_margin=256, n_inter=128, leads=2, seed=1)
    first = tr_a[0]
    _ = va[0], va[1]
    second_a, _, second_b = tr_a[1], tr_b[0], tr_b[1]
    for k in second_a:
        assert torch.equal(second_a[k], second_b[k]), k
    assert not torch.equal(first['field_data'], va[0]['field_data'])


# ------------------------------------------------------------------------------------------------ 10. no backward state
def test_validation_step_allocates_no_backward_state():
    import ctypes
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import step_losses
    m = _model()
    b = _batch(4096, 20480)
    n = 4096 + 20480
    sizes = L.DpnSizes()
    L.check(L.load().dpn_sizes(n, int(m.precision), ctypes.byref(sizes)), 'dpn_sizes')

    def peak(fn):
        fn()                                       # warm-up
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out
        return p

    def train_forward():
        cfg = m.point_config()
        heads, evec, statics = m.physics_net.field_weights(b['field_data'], b['forecast_h'])
        n_i, pts = m._eval_inputs(b, True)
        return step_losses(cfg, n_i, *pts, b['margin_data'], heads, evec, statics, beta=0.1, margin_factor=1e6)

    p_valid = peak(lambda: m.validation_step(b))
    p_train = peak(train_forward)
    print('peak device memory: validation_step %.1f MB, training forward %.1f MB, saved state %.1f MB, operands %.1f MB, partials %.1f MB'
          % (p_valid / 1e6, p_train / 1e6, sizes.saved / 1e6, sizes.operands / 1e6, sizes.partials / 1e6))
    assert p_valid <= p_train - int(sizes.saved)
    assert p_valid < min(int(sizes.operands), int(sizes.partials), int(sizes.saved))       # no tensor of those sizes can have been allocated


# ------------------------------------------------------------------------------------------------ 11. batched sweep = loop
@pytest.mark.parametrize('with_pde', [True, False])
def test_validate_equals_the_loop_of_validation_steps(with_pde):
    from deepphysinet_amd import validation as V
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model()
    src = SyntheticSamples(_dev(), n_margin=1037, n_inter=300, leads=5, seed=3)
    samples = [src[i] for i in range(5)]
    out = m.validate(samples, with_pde=with_pde, lead_batch=3)              # groups of 3 and 2
    assert len(out['samples']) == 5
    for row, smp in zip(out['samples'], samples):
        one = m.validation_step(smp, with_pde=with_pde)
        assert row.keys() == one.keys()
        for k in ('valid_loss', 'margin_loss', 'inter_pde_loss', 'margin_pde_loss', 'terms'):
            if one.get(k) is not None:
                assert torch.equal(row[k], one[k]), k
        assert torch.equal(row['stats'], one['stats']) and row['variables'] == one['variables'] and row['forecast_h'] == one['forecast_h']
    assert len({r['forecast_h'] for r in out['samples']}) == 5
    merged = V.merge_stats([r['stats'] for r in out['samples']])
    assert torch.equal(out['pooled']['stats'], merged)
    want = V.metrics_from_stats(merged)
    assert {k: v for k, v in out['pooled'].items() if k != 'stats'} == want
    assert want['n_points'] == 5 * 1037 and want['n_samples'] == 5
    default = m.validate(samples, with_pde=with_pde)                        # the 256 MiB rule: one group here
    assert m.lead_batch_size(1337, 5) == 5
    for row, ref in zip(default['samples'], out['samples']):
        assert torch.equal(row['stats'], ref['stats']) and torch.equal(row['valid_loss'], ref['valid_loss'])


# ------------------------------------------------------------------------------------------------ 12. the loop
LINE = re.compile(r'^epoch \d+ step \d+ loss \S+( \w+ \S+)+$')


def test_training_loop_with_and_without_a_validation_source(tmp_path, capsys):
    """`last_validation` is checked for being finite and complete (every key of validation_step's dict), not against a re-run."""
    from deepphysinet_amd import validation as V
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model()
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    train_src = lambda: SyntheticSamples(_dev(), n_margin=512, n_inter=256, leads=4, seed=0)      # a fresh one per run: its sampler counts its draws
    src = train_src()
    val = SyntheticSamples(_dev(), n_margin=512, n_inter=256, leads=3, seed=1)
    logs = tmp_path / 'logs'
    capsys.readouterr()
    out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(logs), max_steps=7, num_epoch=2, pde_start_step=3)
    with_valid = capsys.readouterr().out
    assert out['global_step'] == 7
    lv = out['last_validation']
    one = m.validation_step(val[0])
    assert set(one) <= set(lv) and lv['global_step'] == 7
    assert np.isfinite(float(lv['valid_loss'])) and all(np.isfinite(list(v.values())).all() for v in lv['variables'].values())
    text = [f for f in os.listdir(logs) if re.fullmatch(r'log_.*\.txt', f)]
    assert len(text) == 1
    lines = open(logs / text[0]).read().splitlines()
    assert len(lines) == 8                                  # global_step 1, 3, 5, 7: a training line and a validation line each
    head = r'^epoch:\d+/\d+,batch:\d+/\d+,iter:\d+/\d+,'
    num = r'-?\d+\.\d{6}'
    for i, ln in enumerate(lines):
        which = 'train loss' if i % 2 == 0 else 'valid loss'
        assert re.fullmatch(head + r'%s:%s,(\w+:%s,)+forecast:\d{3}h,fps:%s' % (which, num, num, num), ln), ln
    assert 'inter_pde_loss' not in lines[0] and 'inter_pde_loss' in lines[-1] and 'inter_pde_loss' in lines[-2]       # PDE losses from step 4 on
    events = [json.loads(l) for l in open(logs / 'metrics.jsonl')]
    assert [e['event'] for e in events] == ['training', 'validation'] * 4
    assert set(one) <= set(events[-1]) and set(events[0]['variables']) == set(V.VARIABLES)
    # without a source: the loop of before -- same stdout format, no log directory, no `last_validation`
    m2 = _model()
    m2.train_cfg.setdefault('log', {})['log_step'] = 2
    capsys.readouterr()
    out2 = m2.run_train_interface(samples=train_src(), log_path=str(tmp_path / 'unused'), max_steps=7, num_epoch=2, pde_start_step=3)
    plain = capsys.readouterr().out
    assert 'last_validation' not in out2 and not os.path.exists(tmp_path / 'unused')
    rows = [l for l in plain.splitlines() if l.startswith('epoch ')]
    assert len(rows) == 4 and all(LINE.match(l) for l in rows), rows
    assert [l for l in with_valid.splitlines() if l.startswith('epoch ')] == rows       # validation changes neither the line nor a digit of it
    # validate_every_epoch: the whole source after each epoch's checkpoint
    out3 = _model().run_train_interface(samples=train_src(), valid_samples=val, max_steps=4, num_epoch=1, validate_every_epoch=True, valid_lead_batch=2)
    assert out3['last_epoch_validation']['pooled']['n_samples'] == 3 and len(out3['last_epoch_validation']['samples']) == 3


def test_train_py_with_a_synthetic_validation_source(tmp_path):
    """train.py --synthetic --valid_synthetic end to end in a fresh child process."""
    cfg = tmp_path / 'cfg.py'
    cfg.write_text('from deepphysinet_amd.configs import ncep_config\nconfig = ncep_config()\n'
                   "config['train_cfg'].setdefault('log', {})['log_step'] = 2\nconfig['train_cfg']['train_data'].update(label_batch_size=1024, batch_size_inter=512)\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--config_file', str(cfg), '--synthetic', '--valid_synthetic', '--max_steps', '3',
                        '--log_path', str(tmp_path / 'logs'), '--checkpoint_path', str(tmp_path / 'ckpt')], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'last validation: valid loss' in r.stdout
    events = [json.loads(l) for l in open(tmp_path / 'logs' / 'metrics.jsonl')]
    assert [e['event'] for e in events] == ['training', 'validation'] * 2
