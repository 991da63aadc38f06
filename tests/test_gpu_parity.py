"""GPU (MI355X): the HIP point path, called through the C ABI (ctypes -> libdpn_hip.so), against the CPU oracle on the
same closed-form inputs, against the golden vectors captured from the reference, and -- at the full 0.25-degree size --
through size-independent properties.

Tolerances:
  bf16x2 (hi+lo split operands)  : PDE losses 1e-4 rel (north-star bar), fields 5e-5, Jacobian 2e-4, gradients 1e-3 of max
  bf16   (plain bf16 operands)   : PDE losses 5e-2 rel, fields 2e-2 of max, gradients 0.25 of max (8-bit operand mantissa)
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from oracle.fill import fill_state_dict_, synthetic_inputs

GEO = O.Geometry()
TOL = {'bf16x2': dict(loss=1e-4, field=5e-5, jac=2e-4, grad=1e-3), 'bf16': dict(loss=5e-2, field=2e-2, jac=0.35, grad=0.25)}


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _model(prec, gain=1.0, with_clip=True):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config(), precision=prec)
    sd = m.physics_net.state_dict()
    fill_state_dict_(sd, gain=gain)
    m.physics_net.load_state_dict(sd)
    m.with_clip = with_clip
    return m.to(_dev())


def _oracle(inp, gain=1.0, with_clip=True, want_grads=True):
    st = O.make_state(requires_grad=True, gain=gain)
    x, y, t = (inp[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    total, parts, fn, ph = O.place_one_batch(st, x, y, t, inp['f'], inp['field_data'], inp['coord_data'], inp['forecast_h'], GEO,
                                             with_clip=with_clip, return_parts=True)
    jac_n = O.jacobian_fields(x, y, t, fn).detach()
    grads = None
    if want_grads:
        names = O.param_names(st)
        grads = dict(zip(names, torch.autograd.grad(total, [st[n] for n in names])))
    return dict(total=float(total.detach()), parts=np.array([float(p.detach()) for p in parts]), fields=torch.cat(fn, 1).detach(),
                jac_n=jac_n, grads=grads)


def _gpu(batch):
    return {k: v.to(_dev()) for k, v in batch.items()}


def test_library_is_the_hip_one_and_layout_selftest_passes():
    from deepphysinet_amd import _lib
    lib = _lib.load()
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.__file__), 'libdpn_hip.so'))
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device=_dev())
    assert lib.dpn_selftest(ctypes.c_void_p(scratch.data_ptr()), torch.cuda.current_stream().cuda_stream) == 0


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
@pytest.mark.parametrize('n', [5197, 1037, 256, 200, 1])   # 5197: all ten weight-gradient splits, 41 workgroups per net; 1037: nine workgroups, a ragged tail of 13
def test_fields_jacobian_losses_gradients_vs_oracle(prec, n):
    import deepphysinet_amd as dpn
    if prec == 'bf16x2' and n >= 200:
        # parity-grade mode, hundreds of points: no outlier / L2 allowances -- the points whose switch bits differ are identified and removed,
        # everything else is held to the tight bars (sizes 5197 and 1037 run in test_kink_flips_are_listed_and_every_other_point_is_tight)
        if n in (5197, 1037):
            pytest.skip('covered by test_kink_flips_are_listed_and_every_other_point_is_tight[%d]' % n)
        return _assert_tight_after_removing_flips(n)
    tol = TOL[prec]
    inp = synthetic_inputs(n, tag='inter')
    ref = _oracle(inp)
    m = _model(prec)
    g = _gpu(inp)
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        out_n, jac_n = dpn.pde_fields_and_jacobian(cfg, g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
    assert float((out_n.cpu() - ref['fields']).abs().max() / ref['fields'].abs().max()) < tol['field']
    for k in range(6):
        r = ref['jac_n'][:, k]
        err = (jac_n.cpu()[:, k] - r).abs()
        bound = tol['jac'] * float(r.abs().max())
        if n < 200:
            assert float(err.max()) < bound, k
        else:
            # plain-bf16 mode only (NOT the parity-grade mode, whose checks above carry no such allowance): operands rounded to 8 bits flip
            # many ReLU signs, and the Jacobian of a ReLU network is piecewise constant in them; isolated rows beyond the (already loose)
            # bound are tolerated here -- at most one point per net, or 0.2 % of the points.
            bad_points = int((err > bound).any(dim=1).sum())
            assert bad_points <= max(1, (2 * n + 999) // 1000), (k, bad_points)
            assert float(torch.quantile(err.flatten(), 0.99)) < bound, k
    m.physics_net.zero_grad()
    terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'])
    terms.sum().backward()
    mine = terms.detach().cpu().numpy()
    # the 1e-4 bar is for batch means; a single point's squared residual has no averaging of the per-point rounding (x20)
    ltol = tol['loss'] * (20.0 if n == 1 else 1.0)
    assert np.all(np.abs(mine - ref['parts']) <= ltol * np.abs(ref['parts'])), (mine, ref['parts'])
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue                      # mathematically zero gradient (softmax shift invariance): rounding noise on both sides
        r = ref['grads'][name]
        d = (p.grad.cpu() - r).abs()
        err = float(d.max() / (r.abs().max() + 1e-30))
        if n < 200:
            assert err < tol['grad'] * (20.0 if n == 1 else 1.0), (name, err)
        else:
            # plain-bf16 mode only: flipped mask bits move single elements of a bias / weight-row gradient by a point's whole contribution;
            # the bound holds in the tensor's L2 norm and 5x on the single worst element (the parity-grade mode has no such fallback).
            l2 = float(d.pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-30))
            assert l2 < tol['grad'] and err < 5.0 * tol['grad'], (name, l2, err)


def test_place_one_batch_matches_reference_golden(golden_dir):
    """The drop-in entry point against the scalar the REFERENCE returned for the same inputs (fixture F5)."""
    d = np.load(os.path.join(golden_dir, 'f345_pde_clip1_fp32.npz'))
    inp = synthetic_inputs(256, tag='inter')
    m = _model('bf16x2')
    g = _gpu(inp)
    lf = m.train_cfg['losses']['loss_factor']
    total = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.MSELoss(), lf,
                              global_step=2, local_rank=0, device=_dev())
    assert abs(float(total.detach()) - float(d["total"])) <= 1e-4 * abs(float(d["total"]))
    terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).detach().cpu().numpy()
    assert np.all(np.abs(terms - d['parts']) <= 1e-4 * np.abs(d['parts']))


@pytest.mark.parametrize('case', ['l1', 'sl1', 'sl1_b2', 'mse_sum', 'norm', 'norm_sq'])
def test_other_pde_criteria_and_norm_branches_match_reference_golden(golden_dir, case):
    """Fixture F12 -- the REFERENCE run on the branches its shipped config does not take: `pde_loss` = L1Loss / WeightSmoothL1Loss(beta) (the other two
    criteria its loss builder offers, interface_physics.py:384) and inverse_norm's use_norm False / two-factor min_max branches (:238-243).
    place_one_batch's scalar and the six terms at 1e-4, the gradient of every parameter against the oracle's (pinned to the same fixture on CPU)."""
    from deepphysinet_amd.losses import builder_loss
    d = np.load(os.path.join(golden_dir, 'f12_criteria_and_norm_branches.npz'))
    inp = synthetic_inputs(256, tag='inter')
    m = _model('bf16x2')
    g = _gpu(inp)
    lf = m.train_cfg['losses']['loss_factor']
    crit_cfg = {'l1': dict(name='L1Loss'), 'sl1': dict(name='WeightSmoothL1Loss', beta=0.1), 'sl1_b2': dict(name='WeightSmoothL1Loss', beta=2.0),
                'mse_sum': dict(name='MSELoss', reduction='sum')}.get(case)
    crit = builder_loss(**crit_cfg) if crit_cfg else torch.nn.MSELoss()
    norm_cfg = None
    if case in ('norm', 'norm_sq'):
        norm_cfg = O.f12_norm_cfg() if case == 'norm' else O.f12_norm_sq_cfg()
        for name, c in zip(('u10', 'v10', 'pres', 't2', 'q2', 'rio'), norm_cfg):
            m.obs_norm_cfg[name].update(norm_type=c['norm_type'], norm_factor=c['norm_factor'], use_norm=c['use_norm'])
    m.physics_net.zero_grad()
    total = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], crit, lf, global_step=2,
                              local_rank=0, device=_dev())
    total.backward()
    assert abs(float(total.detach()) - float(d[case + '.total'])) <= 1e-4 * abs(float(d[case + '.total'])), (float(total.detach()), float(d[case + '.total']))
    # the config-file route (`builder_loss(**train_cfg.losses.pde_loss)`) gives the same kernel configuration as the module
    if crit_cfg:
        m.train_cfg['losses']['pde_loss'] = crit_cfg
    terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).detach().cpu().numpy()
    assert np.all(np.abs(terms - d[case + '.parts']) <= 1e-4 * np.abs(d[case + '.parts'])), (terms, d[case + '.parts'])
    # gradients: the oracle on the same branch (tests/test_oracle_golden.py holds it to F12's gradient norms)
    st = O.make_state(requires_grad=True)
    x, y, t = (inp[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    o_total = O.place_one_batch(st, x, y, t, inp['f'], inp['field_data'], inp['coord_data'], inp['forecast_h'], GEO,
                                crit=O.pde_criterion(crit_cfg['name'], beta=crit_cfg.get('beta', 0.1), reduction=crit_cfg.get('reduction', 'mean')) if crit_cfg else None,
                                norm_cfg=norm_cfg)
    names = O.param_names(st)
    ref = dict(zip(names, torch.autograd.grad(o_total, [st[n] for n in names])))
    worst = 0.0
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        r = ref[name]
        diff = (p.grad.cpu() - r).abs()
        # the slope of |r| and of SmoothL1 is discontinuous / steep in r: a residual within rounding of 0 (or of +-beta) moves one point's whole
        # contribution, so the bound is on the tensor's L2 norm, with 5x on the single worst element (as for the mask flips of the plain-bf16 mode)
        l2 = float(diff.pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-30))
        err = float(diff.max() / (r.abs().max() + 1e-30))
        worst = max(worst, err)
        assert l2 < TOL['bf16x2']['grad'] and err < 5.0 * TOL['bf16x2']['grad'], (case, name, l2, err)
    print('F12 %s: total %.6e (reference %.6e), worst gradient element error %.2e' % (case, float(total.detach()), float(d[case + '.total']), worst))
    if norm_cfg is not None:
        # the full-grid maps kernel (inverse_norm + scatter of the visualisation branch) takes the same table: against the module's torch expression
        from deepphysinet_amd import _lib as L
        from deepphysinet_amd.point_path import _ptr, _stream
        lon, lat = 8, 4
        out_n = torch.randn(lon * lat, 6, device=_dev())
        maps = torch.empty((6, lat, lon), dtype=torch.float32, device=_dev())
        ph = m.point_config().physics()
        for wc in (0, 1):
            L.check(L.load().dpn_grid_maps(_ptr(out_n), lon, lat, ctypes.byref(ph), wc, _ptr(maps), _stream()), 'dpn_grid_maps')
            m.with_clip = bool(wc)
            ref6 = m.inverse_norm(*[out_n[:, k] for k in range(6)], obs_norm_cfg=m.obs_norm_cfg)
            m.with_clip = True
            for k in range(6):
                want = ref6[k].view(lon, lat).t()                      # node order: x outer, y inner -> [lat][lon]
                assert torch.allclose(maps[k], want, rtol=2e-7, atol=0.0), (case, wc, k, float((maps[k] - want).abs().max()))


def test_grid_node_points_longest_lead_match_reference_golden(golden_dir):
    """Fixture F10 -- the REFERENCE on 200 grid-node points (x, y exact multiples of the cell size, both domain corners: xi = 0 and 1)
    at the longest lead time (336 h): the six losses and their sum within the north-star 1e-4, fields and Jacobian within the mode's bars."""
    import deepphysinet_amd as dpn
    d = np.load(os.path.join(golden_dir, 'f10_grid_nodes_h336_fp32.npz'))
    inp = synthetic_inputs(200, tag='f10', margin=True, forecast_h=336.0 / 360.0)
    inp['x'][0, 0], inp['y'][0, 0] = 0.0, 0.0
    inp['x'][1, 0], inp['y'][1, 0] = 256 * 27000.0, 144 * 27000.0
    assert np.array_equal(inp['x'].numpy(), d['x']) and np.array_equal(inp['y'].numpy(), d['y'])
    m = _model('bf16x2')
    g = _gpu(inp)
    lf = m.train_cfg['losses']['loss_factor']
    total = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.MSELoss(), lf,
                              global_step=2, local_rank=0, device=_dev())
    assert abs(float(total.detach()) - float(d["total"])) <= 1e-4 * abs(float(d["total"]))
    terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).detach().cpu().numpy()
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        out_n, jac_n = dpn.pde_fields_and_jacobian(cfg, g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
    # per term: 1e-4, the north-star bar, against the REFERENCE's numbers when no point of the batch carries a switch bit (ReLU / clip /
    # vapour) that differs from the oracle arithmetic's; otherwise those points are named and removed from both sides, and the terms of
    # the remaining points are held to 1e-4 against the oracle (which tests/test_oracle_golden.py pins to this very fixture)
    flipped, _ = _flipped_points(m, inp)
    rel = np.abs(terms - d['parts']) / np.abs(d['parts'])
    print('F10: points with a differing switch bit:', torch.nonzero(flipped).flatten().tolist(), 'per-term rel. error (all points)', rel)
    # the UN-removed batch is bounded too: one flipped switch moves a mean over N points by O(1 / N) of the term's spread -- N = 200 here
    assert np.all(rel <= 1e-2), rel
    if int(flipped.sum()) == 0:
        assert np.all(rel <= 1e-4), (terms, d['parts'])
    else:
        mine, ref_parts, idx = _terms_vs_oracle_flip_free(m, inp)
        assert np.all(np.abs(mine - ref_parts) <= 1e-4 * np.abs(ref_parts)), (idx, mine, ref_parts)
    ref_n = torch.from_numpy(d['fields_norm'])
    assert float((out_n.cpu() - ref_n).abs().max() / ref_n.abs().max()) < TOL['bf16x2']['field']


@pytest.mark.parametrize('with_clip', [True, False])
def test_clip_masks_wide_outputs(golden_dir, with_clip):
    """out_fc gain 5: many P/T/q/rho points sit on a clip bound -> zero Jacobian rows, zero gradient there (fixture F9)."""
    import deepphysinet_amd as dpn
    d = np.load(os.path.join(golden_dir, 'f9_wide_clip%d_fp32.npz' % int(with_clip)))
    inp = synthetic_inputs(128, tag='f9')
    m = _model('bf16x2', gain=5.0, with_clip=with_clip)
    g = _gpu(inp)
    terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).detach().cpu().numpy()
    ok = np.isfinite(d['parts'])
    assert np.array_equal(np.isfinite(terms), ok)           # the unclipped vapour term is NaN in the reference as well
    flipped, _ = _flipped_points(m, inp, gain=5.0, with_clip=with_clip)
    raw = np.abs(terms[ok] - d['parts'][ok]) / np.abs(d['parts'][ok])
    print('F9 (clip %d): points with a differing switch bit: %s; per-term rel. error (all points) %s' % (with_clip, torch.nonzero(flipped).flatten().tolist(), raw))
    assert np.all(raw <= 1e-2), raw            # the UN-removed batch (N = 128, half of the points on a clip bound): bounded, not only printed
    sub = inp
    # with the clip: the north-star 1e-4.  Without it the fields are unbounded (rho and q reach zero and below: the reference's own vapour
    # term is NaN there) and the residuals divide by them -- an ill-conditioned evaluation in ANY arithmetic, not a switch flip: 2e-4 holds
    # (measured 1.3e-4 on the u-momentum term, whose p_x / rho has rho within 1e-3 of zero at two points)
    bar = 1e-4 if with_clip else 2e-4
    if int(flipped.sum()) == 0:
        assert np.all(np.abs(terms[ok] - d['parts'][ok]) <= bar * np.abs(d['parts'][ok])), (terms, d['parts'])
    else:                                                     # named points removed from both sides, the rest at the north-star bar
        assert int(flipped.sum()) <= 3
        mine, ref_parts, _ = _terms_vs_oracle_flip_free(m, inp, gain=5.0, with_clip=with_clip)
        assert np.all(np.abs(mine[ok] - ref_parts[ok]) <= bar * np.abs(ref_parts[ok])), (mine, ref_parts)
        sub = _without(inp, flipped)
    if with_clip:
        ref = _oracle(sub, gain=5.0, with_clip=True)
        gs = _gpu(sub)
        m.physics_net.zero_grad()
        m.pde_loss_terms(gs['x'], gs['y'], gs['t'], gs['f'], gs['field_data'], gs['coord_data'], gs['forecast_h']).sum().backward()
        for name in ('T_net.out_fc.weight', 'P_net.cat_fc1.fc.0.weight', 'q_net.coord_hidden_fc.weight'):
            r = ref['grads'][name]
            p = dict(m.physics_net.named_parameters())[name]
            assert float((p.grad.cpu() - r).abs().max() / r.abs().max()) < TOL['bf16x2']['grad'], name


def test_data_loss_and_reference_forward_surface(golden_dir):
    """Data ("margin") loss + gradients, through forward_xyt (kernel-side encoding) and through the reference-shaped
    PhysicsNet.forward(field, coord_pe, coord_data, forecast_h) that receives already-encoded coordinates."""
    d = np.load(os.path.join(golden_dir, 'f6_data_loss.npz'))
    inp = synthetic_inputs(256, tag='margin', margin=True)
    m = _model('bf16x2')
    g = _gpu(inp)
    m.physics_net.zero_grad()
    loss = m.data_loss(g['x'], g['y'], g['t'], g['field_data'], g['coord_data'], g['labels'], g['forecast_h'])
    loss.backward()
    assert abs(float(loss.detach()) - float(d['loss'])) <= 5e-5 * float(d['loss']), (float(loss.detach()), float(d['loss']))
    ref_norm = dict(zip([str(n) for n in d['names']], d['norms']))
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        assert abs(float(p.grad.double().norm()) - ref_norm[name]) <= 5e-3 * ref_norm[name] + 1e-9, name   # SmoothL1' has slope 1/beta = 10
    # element-wise (fixture F13 = sampled entries of the REFERENCE's data-loss gradients, every tensor).  All 256 points first: printed and bounded at 5e-3 of the
    # tensor's largest entry -- one point whose ReLU bit differs from the oracle arithmetic's moves an entry of a 256-point mean by up to 1 / 256 of that point's
    # share.  Then the mode's gradient bar, 1e-3: against the reference's numbers when no point carries such a bit, else with the named points removed from both
    # sides against the oracle (which tests/test_oracle_golden.py pins to this very fixture, element by element).
    e = np.load(os.path.join(golden_dir, 'f13_elementwise_data_loss_and_step.npz'))
    worst = 0.0
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        mine = p.grad.flatten()[::max(1, p.numel() // 128)].cpu().numpy()
        worst = max(worst, float(np.abs(mine - e['dl.g.' + name]).max() / (float(e['dl.gmax.' + name]) + 1e-30)))
    flipped, _ = _flipped_points(m, inp)
    relu_flips = torch.nonzero(flipped).flatten().tolist()
    print('data-loss gradients, sampled entries of all tensors vs the reference, all 256 points: worst %.2e of the tensor maximum; points with a differing '
          'switch bit: %s' % (worst, relu_flips))
    assert worst < 5e-3, worst
    if relu_flips:
        sub = _without(inp, flipped)
        st = O.make_state(requires_grad=True)
        ref_loss = O.data_loss(st, sub['x'], sub['y'], sub['t'], sub['field_data'], sub['coord_data'], sub['labels'], sub['forecast_h'], GEO)
        names_ = O.param_names(st)
        ref_g = dict(zip(names_, torch.autograd.grad(ref_loss, [st[k] for k in names_])))
        gs = _gpu(sub)
        m.physics_net.zero_grad()
        m.data_loss(gs['x'], gs['y'], gs['t'], gs['field_data'], gs['coord_data'], gs['labels'], gs['forecast_h']).backward()
        worst = 0.0
        for name, p in m.physics_net.named_parameters():
            if name.endswith('key_projection.bias'):
                continue
            r = ref_g[name]
            worst = max(worst, float((p.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-30)))
        print('with them removed from both sides, EVERY entry vs the oracle: worst %.2e of the tensor maximum' % worst)
    assert worst < TOL['bf16x2']['grad'], worst
    with torch.no_grad():
        pe = m.encoding_coord(g['x'], g['y'], g['t'], m.pred_t_span)
        fields = torch.cat(m.physics_net(g['field_data'], pe, g['coord_data'], g['forecast_h']), dim=1).cpu().numpy()
    assert np.abs(fields - d['fields_norm']).max() <= 5e-5 * np.abs(d['fields_norm']).max()
    crit = __import__('deepphysinet_amd').losses.builder_loss('WeightSmoothL1Loss', beta=0.1)
    assert abs(float(crit(torch.from_numpy(fields).to(_dev()), g['labels'])) * 1e6 - float(d['loss'])) <= 5e-5 * float(d['loss'])


def test_training_step_matches_reference_optimiser_step(golden_dir):
    """Fixture F8: data loss + PDE(inter) + PDE(margin) -> clip_grad_norm_(2.5e7) -> Adam(1e-4, wd 1e-4), one step."""
    d = np.load(os.path.join(golden_dir, 'f8_step.npz'))
    m = _model('bf16x2')
    inter, margin = _gpu(synthetic_inputs(256, tag='inter')), _gpu(synthetic_inputs(256, tag='margin', margin=True))
    batch = dict(field_data=inter['field_data'], forecast_h=inter['forecast_h'],
                 margin_x=margin['x'], margin_y=margin['y'], margin_t=margin['t'], margin_f=margin['f'], margin_data=margin['labels'],
                 margin_input_data=margin['coord_data'], inter_x=inter['x'], inter_y=inter['y'], inter_t=inter['t'], inter_f=inter['f'],
                 inter_data=inter['coord_data'])
    before = {k: v.detach().clone() for k, v in m.physics_net.named_parameters()}
    opt = torch.optim.Adam(m.physics_net.parameters(), lr=1e-4, weight_decay=1e-4)
    loss, parts, gnorm = m.training_step(batch, opt, with_pde=True)
    assert abs(float(loss) - float(d['loss'])) <= 1e-4 * float(d['loss'])
    assert abs(float(gnorm) - float(d['gnorm'])) <= 1e-3 * float(d['gnorm'])
    ref_post = dict(zip([str(n) for n in d['names']], d['post_norms']))
    ref_delta = dict(zip([str(n) for n in d['names']], d['delta_norms']))
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue          # zero gradient up to rounding noise; Adam turns that noise into +-lr steps of arbitrary sign
        # the first Adam step is ~lr*sign(g): entries whose gradient is at rounding-noise level may flip, so norms agree to ~lr
        assert abs(float(p.detach().double().norm()) - ref_post[name]) <= 1e-4 * ref_post[name] + 1e-12, name
        dn = float((p.detach() - before[name]).double().norm())
        assert abs(dn - ref_delta[name]) <= 2e-2 * ref_delta[name] + 1e-12, name
    # element-wise (fixture F13): sampled entries of (post - pre).  The first Adam step is -lr * sign(g) wherever the gradient is clear of zero: entries whose
    # REFERENCE gradient exceeds 1e-3 of the tensor's largest (the mode's gradient bar: below it the two arithmetics need not agree on a sign) must match
    # within 2 % of lr, at most 0.5 % of them may differ (a gradient entry of either sign within the bar of zero); every step is bounded by lr
    e = np.load(os.path.join(golden_dir, 'f13_elementwise_data_loss_and_step.npz'))
    checked = differing = 0
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        stride = max(1, p.numel() // 128)
        mine = (p.detach() - before[name]).flatten()[::stride].cpu().numpy()
        ref_d, ref_g, gmax = e['step.delta.' + name], e['step.g.' + name], float(e['step.gmax.' + name])
        assert np.all(np.abs(mine) <= 1.05e-4), name
        big = np.abs(ref_g) > 1e-3 * gmax
        bad = np.abs(mine - ref_d)[big] > 0.02 * 1e-4
        checked += int(big.sum())
        differing += int(bad.sum())
    print('optimiser step: %d sampled entries with a clear gradient, %d differ from the reference step by more than 2 %% of lr' % (checked, differing))
    assert checked > 5000 and differing <= 0.005 * checked, (checked, differing)


# ------------------------------------------------------------------------------------------------ the fused step loss against the oracle
# training_step takes its three losses from ONE point pass (point_path._StepLossFn): rows [0, n_inter) are the interior points, the rest
# the margin points, and the group boundary lives entirely in offsets and counts.  F8 above cannot see it: two equal groups of whole
# 256-row blocks, one unit cotangent for everything.  These tests use unequal and ragged groups, a different cotangent per output, and
# the reference's own batch sizes (cfg batch_size_inter 4 096 interior, label_batch_size 20 480 margin points).
STEP_BETA = 0.1                       # the data loss's SmoothL1 beta (training_step)
STEP_KEYS = ('data', 'inter_terms', 'inter_total', 'margin_terms', 'margin_total')
DATA_LOSS_TOL = 5e-5                  # the data loss's bar (test_data_loss_and_reference_forward_surface)


def _smooth_l1_flips(m, inp, beta=STEP_BETA):
    """Points at which some |out - label| lies on different sides of the SmoothL1 beta for the HIP fields and for the fp32 oracle's
    (the data loss's own switch), bool [N]."""
    import deepphysinet_amd as dpn
    g = _gpu(inp)
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        out_n, _ = dpn.pde_fields_and_jacobian(m.point_config(), g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
        pe = O.encoding_coord(inp['x'], inp['y'], inp['t'], GEO)
        ref = torch.cat(O.physics_net_forward(O.make_state(), inp['field_data'], pe, inp['coord_data'], inp['forecast_h']), 1)
    lab = inp['labels']
    return ((out_n.cpu() - lab).abs() < beta).ne((ref - lab).abs() < beta).any(dim=1)


def _replace_flipped(m, inp, group, data_loss=False):
    """`inp` with every point whose switch differs from the fp32 oracle arithmetic's (_flipped_points; for the margin group also the
    data loss's beta switch) REPLACED by a copy of the group's first unflipped point, labels included: the group keeps its size, and
    the group sizes are what these tests are about.  Returns (inputs, number replaced)."""
    flipped, _ = _flipped_points(m, inp)
    if data_loss:
        flipped = flipped | _smooth_l1_flips(m, inp)
    idx = torch.nonzero(flipped).flatten().tolist()
    n = flipped.shape[0]
    print('%-6s group, %5d points: %d flipped points replaced %s' % (group, n, len(idx), idx[:12]))
    assert len(idx) <= max(3, n // 100), (group, len(idx))
    if not idx:
        return inp, 0
    keep = torch.nonzero(~flipped).flatten()
    assert keep.numel() > 0, (group, 'no unflipped point to copy')
    src = int(keep[0])
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
    for k in ('x', 'y', 't', 'f', 'coord_data', 'labels'):
        c[k][idx] = c[k][src].clone()
    return c, len(idx)


def _step_scalar(spec, outs):
    """sum of weight * output over the step's outputs; `spec` maps keys of STEP_KEYS to a weight (one number, or six for the terms).
    Outputs that a spec leaves out are not in the scalar's graph: their cotangents reach _StepLossFn.backward as None."""
    s = 0
    for k, w in spec.items():
        v = outs[k]
        s = s + (v * torch.as_tensor(w, dtype=v.dtype, device=v.device)).sum()
    return s


def _oracle_step(sd, inter, margin, specs):
    """The reference's step body on the oracle (its interface_physics.py:464-503): meta_out once, then data_loss(margin) +
    place_one_batch(inter) + place_one_batch(margin) in its order of additions.  Returns (fp32 outputs {STEP_KEYS}, fp32 loss,
    [fp64 gradient dict of each spec's scalar], fp64 state): the losses from the fp32 oracle on the closed-form state (as everywhere in
    this file), the gradients from an fp64 oracle on `sd`, the model's own weights (a state dict)."""
    def run(st, dt):
        field, fh = inter['field_data'].to(dt), inter['forecast_h'].to(dt)
        meta = O.meta_net_forward(st, field, fh)
        leaf = lambda b: [b[k].to(dt).clone().requires_grad_(True) for k in ('x', 'y', 't')]
        xm, ym, tm = leaf(margin)
        data = O.data_loss(st, xm, ym, tm, field, margin['coord_data'].to(dt), margin['labels'].to(dt), fh, GEO, beta=STEP_BETA, meta_out=meta)
        xi, yi, ti = leaf(inter)
        it, ip, _, _ = O.place_one_batch(st, xi, yi, ti, inter['f'].to(dt), field, inter['coord_data'].to(dt), fh, GEO, meta_out=meta,
                                         return_parts=True)
        mt, mp, _, _ = O.place_one_batch(st, xm, ym, tm, margin['f'].to(dt), field, margin['coord_data'].to(dt), fh, GEO, meta_out=meta,
                                         return_parts=True)
        outs = dict(data=data, inter_terms=torch.stack(ip), inter_total=it, margin_terms=torch.stack(mp), margin_total=mt)
        return outs, data + it + mt
    outs32, loss32 = run(O.make_state(), torch.float32)
    outs32 = {k: v.detach().double().numpy() for k, v in outs32.items()}
    st64 = {k: v.detach().cpu().to(torch.float64 if v.is_floating_point() else v.dtype).clone().requires_grad_(v.is_floating_point() and not k.endswith('.pe'))
            for k, v in sd.items()}
    outs64, _ = run(st64, torch.float64)
    names = O.param_names(st64)
    grads = []
    for i, spec in enumerate(specs):
        g = torch.autograd.grad(_step_scalar(spec, outs64), [st64[k] for k in names], retain_graph=i + 1 < len(specs))
        grads.append(dict(zip(names, g)))
    return outs32, float(loss32.detach()), grads, st64


def _hip_step_losses(m, inter, margin):
    """point_path.step_losses called the way training_step calls it: [interior | margin] rows, one encoder pass, the cfg loss factors."""
    from deepphysinet_amd.point_path import step_losses
    gi, gm = _gpu(inter), _gpu(margin)
    lf = m.train_cfg['losses']['loss_factor']
    cfg = m.point_config(lf)
    meta = m.physics_net.encode_field(gi['field_data'], gi['forecast_h'])
    heads, evec, statics = m.physics_net.field_weights(gi['field_data'], gi['forecast_h'], meta_out=meta)
    cat = lambda k: torch.cat([gi[k].reshape(gi[k].shape[0], -1), gm[k].reshape(gm[k].shape[0], -1)], dim=0)
    outs = step_losses(cfg, gi['x'].shape[0], cat('x'), cat('y'), cat('t'), cat('f'), cat('coord_data'), gm['labels'], heads, evec, statics,
                       beta=STEP_BETA, margin_factor=lf['margin_factor'])
    li, ti, lm, tm, data = outs
    return dict(data=data, inter_terms=li, inter_total=ti, margin_terms=lm, margin_total=tm)


def _hip_step_grads(m, inter, margin, spec):
    """d(spec's scalar) / d(every parameter) through a fresh step_losses pass, fp64 on the host."""
    m.physics_net.zero_grad(set_to_none=True)
    outs = _hip_step_losses(m, inter, margin)
    _step_scalar(spec, outs).backward()
    return outs, {k: p.grad.detach().cpu().double() for k, p in m.physics_net.named_parameters()}


def _grad_rows(mine, ref):
    """[(worst element error / the tensor's max |ref|, L2 error / |ref|, name)] for every tensor but key_projection.bias, worst first."""
    rows = []
    for name, g in mine.items():
        if name.endswith('key_projection.bias'):
            continue                      # mathematically zero gradient (softmax shift invariance): rounding noise on both sides
        r = ref[name].double()
        d = g - r
        rows.append((float(d.abs().max() / (r.abs().max() + 1e-300)), float(d.norm() / (r.norm() + 1e-300)), name))
    rows.sort(reverse=True)
    return rows


@pytest.mark.parametrize('n_inter,n_margin', [(1037, 1965), (300, 4096), (1, 700), (700, 1)])
def test_step_losses_unequal_and_ragged_groups_vs_oracle(n_inter, n_margin):
    """The fused step loss at group sizes where the boundary matters: (1037, 1965) both ragged, the boundary inside a 256-row block;
    (300, 4096) a short group in front of a long one; (1, 700) / (700, 1) a one-point group on either side.  Losses against the fp32
    oracle on their own group (PDE terms and totals 1e-4, data loss 5e-5), against separate pde_loss_terms / data_loss calls on the same
    weights (bitwise: the forward is per-point arithmetic and each group's block sums start at its own row 0), and the gradients of
    data + inter total + margin total against the fp64 oracle (every element within 1e-3 of its tensor's maximum).  A one-point group
    gets the x20 of test_fields_jacobian_losses_gradients_vs_oracle's n == 1: a single point's residual has no averaging of rounding."""
    tol = TOL['bf16x2']
    m = _model('bf16x2')
    inter, _ = _replace_flipped(m, synthetic_inputs(n_inter, tag='inter'), 'inter')
    margin, _ = _replace_flipped(m, synthetic_inputs(n_margin, tag='margin', margin=True), 'margin', data_loss=True)
    spec = dict(data=1.0, inter_total=1.0, margin_total=1.0)
    ref, _, (g64,), _ = _oracle_step(m.physics_net.state_dict(), inter, margin, [spec])
    outs, grads = _hip_step_grads(m, inter, margin, spec)
    outs = {k: v.detach() for k, v in outs.items()}
    gi, gm = _gpu(inter), _gpu(margin)
    with torch.no_grad():
        sep_li, sep_ti = m.pde_loss_terms(gi['x'], gi['y'], gi['t'], gi['f'], gi['field_data'], gi['coord_data'], gi['forecast_h'], with_total=True)
        sep_lm, sep_tm = m.pde_loss_terms(gm['x'], gm['y'], gm['t'], gm['f'], gm['field_data'], gm['coord_data'], gm['forecast_h'], with_total=True)
        sep_d = m.data_loss(gm['x'], gm['y'], gm['t'], gm['field_data'], gm['coord_data'], gm['labels'], gm['forecast_h'], beta=STEP_BETA)
    sep = dict(data=sep_d, inter_terms=sep_li, inter_total=sep_ti, margin_terms=sep_lm, margin_total=sep_tm)
    one = lambda n_: 20.0 if n_ == 1 else 1.0
    bars = dict(data=DATA_LOSS_TOL * one(n_margin), inter_terms=tol['loss'] * one(n_inter), inter_total=tol['loss'] * one(n_inter),
                margin_terms=tol['loss'] * one(n_margin), margin_total=tol['loss'] * one(n_margin))
    errs, equal = {}, {}
    for k in STEP_KEYS:
        mine = outs[k].double().cpu().numpy()
        errs[k] = float(np.max(np.abs(mine - ref[k]) / np.abs(ref[k])))
        equal[k] = torch.equal(outs[k], sep[k])
        print('%4d + %4d  %-12s rel. error vs fp32 oracle %.2e (bar %.0e) | bitwise the separate call: %s'
              % (n_inter, n_margin, k, errs[k], bars[k], equal[k]))
    gbar = tol['grad'] * max(one(n_inter), one(n_margin))
    rows = _grad_rows(grads, g64)
    for err, l2, name in rows[:3]:
        print('%4d + %4d  gradient %-52s %.2e of the tensor maximum (L2 %.2e), bar %.0e' % (n_inter, n_margin, name, err, l2, gbar))
    for k in STEP_KEYS:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
        assert equal[k], (k, outs[k], sep[k])
    assert len(rows) == sum(1 for k, _ in m.physics_net.named_parameters() if not k.endswith('key_projection.bias'))
    for err, l2, name in rows:
        assert err < gbar, (name, err, gbar)


def test_step_losses_cotangents_reach_their_own_rows():
    """Backward of _StepLossFn from four scalars, each against the fp64 oracle's gradient of the same scalar (1037 + 1965 points, every
    element within 1e-3 of its tensor's maximum): the data loss alone (both PDE groups take the zero-cotangent branch), six distinct
    weights on the inter terms plus the margin total (per-term and total cotangents on different groups), six other weights on the margin
    terms (the inter group takes the zero-cotangent branch), the inter total alone (no data-loss cotangent on the margin rows)."""
    n_inter, n_margin = 1037, 1965
    tol = TOL['bf16x2']
    m = _model('bf16x2')
    inter, _ = _replace_flipped(m, synthetic_inputs(n_inter, tag='inter'), 'inter')
    margin, _ = _replace_flipped(m, synthetic_inputs(n_margin, tag='margin', margin=True), 'margin', data_loss=True)
    specs = [('data loss alone', dict(data=1.0)),
             ('w . inter terms + margin total', dict(inter_terms=[0.5, 1.75, 0.25, 1.25, 2.0, 0.75], margin_total=1.0)),
             ("w' . margin terms", dict(margin_terms=[1.5, 0.375, 2.5, 0.625, 1.125, 3.0])),
             ('inter total alone', dict(inter_total=1.0))]
    _, _, g64s, _ = _oracle_step(m.physics_net.state_dict(), inter, margin, [s for _, s in specs])
    results = []
    for (what, spec), g64 in zip(specs, g64s):
        _, grads = _hip_step_grads(m, inter, margin, spec)
        rows = _grad_rows(grads, g64)
        err, l2, name = rows[0]
        print('%-32s worst gradient %-52s %.2e of the tensor maximum (L2 %.2e), bar %.0e' % (what, name, err, l2, tol['grad']))
        results.append((what, rows))
    for what, rows in results:
        for err, l2, name in rows:
            assert err < tol['grad'], (what, name, err)


def test_training_step_at_the_reference_batch_sizes_vs_the_oracle():
    """training_step at the reference's batch sizes (4 096 interior + 20 480 margin points), parity-grade mode, closed-form weights,
    against the oracle's step body: the three losses and their sum (fp32 oracle, 1e-4; data loss 5e-5), every pre-step gradient
    element (fp64 oracle, 1e-3 of its tensor's maximum), gnorm (1e-3 of the fp64 oracle's; the clip is active here: the oracle's gnorm is
    above 2.5e7), and the step of the fused optimiser against clip_and_adam_step on the fp64 gradients (F13's rule).  Copy A steps with
    build_optimizer() (FusedClipAdam, bucket layout), copy B with torch.optim.Adam; after each of two steps they agree to the bars of
    test_fused_clip_adam_equals_torch.  Before the second step B takes A's parameters, so that both optimisers see the same gradients
    and what is compared is their moment state and step counter (a gradient element at rounding-noise level, e.g. key_projection.bias,
    is not a function of the parameters' last bits)."""
    tol = TOL['bf16x2']
    lr, wd, max_norm = 1e-4, 1e-4, 2.5e7
    A, B = _model('bf16x2'), _model('bf16x2')
    opt_a = A.build_optimizer()
    assert opt_a.param_groups[0]['lr'] == lr and opt_a.param_groups[0]['weight_decay'] == wd
    opt_b = torch.optim.Adam(B.physics_net.parameters(), lr=lr, weight_decay=wd)
    inter, n_fi = _replace_flipped(A, synthetic_inputs(4096, tag='inter'), 'inter')
    margin, n_fm = _replace_flipped(A, synthetic_inputs(20480, tag='margin', margin=True), 'margin', data_loss=True)

    def batch(i_, m_):
        i_, m_ = _gpu(i_), _gpu(m_)
        return dict(field_data=i_['field_data'], forecast_h=i_['forecast_h'],
                    margin_x=m_['x'], margin_y=m_['y'], margin_t=m_['t'], margin_f=m_['f'], margin_data=m_['labels'],
                    margin_input_data=m_['coord_data'], inter_x=i_['x'], inter_y=i_['y'], inter_t=i_['t'], inter_f=i_['f'],
                    inter_data=i_['coord_data'])
    b1 = batch(inter, margin)
    before = {k: v.detach().clone() for k, v in A.physics_net.state_dict().items()}
    loss_a, parts_a, gn_a = A.training_step(b1, opt_a, with_pde=True, max_norm=max_norm)
    loss_b, parts_b, gn_b = B.training_step(b1, opt_b, with_pde=True, max_norm=max_norm)
    gn_a, gn_b = float(gn_a), float(gn_b)
    # the pre-step gradients are read from p.grad: neither optimiser may have cleared it (torch's clip scales B's in place, A's is untouched)
    assert all(p.grad is not None for p in A.physics_net.parameters()) and all(p.grad is not None for p in B.physics_net.parameters())
    grads = {k: p.grad.detach().cpu().double() for k, p in A.physics_net.named_parameters()}

    ref, ref_loss, (g64,), st64 = _oracle_step(before, inter, margin, [dict(data=1.0, inter_total=1.0, margin_total=1.0)])
    gn64 = float(torch.sqrt(sum((g ** 2).sum() for g in g64.values())))
    coef = min(1.0, max_norm / (gn64 + 1e-6))
    # losses
    pairs = [('margin_loss', 'data', DATA_LOSS_TOL), ('inter_pde_loss', 'inter_total', tol['loss']), ('margin_pde_loss', 'margin_total', tol['loss'])]
    lerr = {}
    for part, key, bar in pairs:
        lerr[part] = (abs(float(parts_a[part]) - float(ref[key])) / abs(float(ref[key])), bar)
    lerr['loss'] = (abs(float(loss_a) - ref_loss) / abs(ref_loss), tol['loss'])
    print('4096 + 20480 points: %d + %d flipped points replaced' % (n_fi, n_fm))
    for k, (e, bar) in lerr.items():
        print('  %-16s rel. error vs fp32 oracle %.2e (bar %.0e)' % (k, e, bar))
    print('  gnorm %.6e vs fp64 oracle %.6e: rel. error %.2e (bar 1e-3); clip coefficient %.4e (max_norm %.1e)'
          % (gn_a, gn64, abs(gn_a - gn64) / gn64, coef, max_norm))
    rows = _grad_rows(grads, g64)
    print('  per-tensor gradient error vs the fp64 oracle (worst element / tensor max, L2), bar %.0e on the element:' % tol['grad'])
    for err, l2, name in rows:
        print('    %-58s %.2e  L2 %.2e' % (name, err, l2))
    # the optimiser step: F13's rule against clip_and_adam_step on the fp64 oracle gradients.  The first Adam step is -lr * sign(g_eff) wherever
    # the effective gradient coef * g + wd * p is clear of zero: entries above 1e-3 of the tensor's largest must match within 2 % of lr, at most
    # 0.5 % of them may differ, every step is bounded by 1.05 lr
    names = [k for k, _ in A.physics_net.named_parameters()]
    pre = {k: st64[k].detach().clone() for k in names}
    post = {k: st64[k].detach().clone() for k in names}
    O.clip_and_adam_step(post, {k: g64[k] for k in names}, {}, lr=lr, weight_decay=wd, max_norm=max_norm)
    checked = differing = 0
    too_big = []
    for name, p in A.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue                      # zero gradient up to rounding noise; Adam turns that noise into +-lr steps of arbitrary sign
        mine = (p.detach() - before[name]).double().cpu()
        ref_d = post[name] - pre[name]
        geff = (coef * g64[name] + wd * pre[name]).abs()
        big = geff > 1e-3 * geff.max()
        checked += int(big.sum())
        differing += int(((mine - ref_d).abs() > 0.02 * lr)[big].sum())
        if float(mine.abs().max()) > 1.05 * lr:
            too_big.append((name, float(mine.abs().max())))
    print('  optimiser step: %d entries with a clear effective gradient, %d differ from the oracle step by more than 2 %% of lr' % (checked, differing))
    # A against B, step 1
    agree = [(n_, float((pa - pb).abs().max())) for (n_, pa), pb in zip(A.physics_net.named_parameters(), B.physics_net.parameters())
             if not torch.allclose(pa, pb, rtol=2e-5, atol=2e-7)]
    print('  FusedClipAdam vs torch.optim.Adam, step 1: gnorm %.7e vs %.7e; %d tensors outside allclose' % (gn_a, gn_b, len(agree)))
    for k, (e, bar) in lerr.items():
        assert e <= bar, (k, e, bar)
    assert gn64 > max_norm, gn64
    assert abs(gn_a - gn64) <= 1e-3 * gn64, (gn_a, gn64)
    assert len(rows) == len(names) - sum(1 for k in names if k.endswith('key_projection.bias'))
    for err, l2, name in rows:
        assert err < tol['grad'], (name, err)
    assert not too_big, too_big
    assert checked > 5000 and differing <= 0.005 * checked, (checked, differing)
    assert abs(gn_a - gn_b) <= 1e-5 * gn_b, (gn_a, gn_b)
    assert not agree, agree
    # step 2 on another batch: Adam's moments and the device-side step counter at full size
    with torch.no_grad():
        for pa, pb in zip(A.physics_net.parameters(), B.physics_net.parameters()):
            pb.copy_(pa)
    b2 = batch(synthetic_inputs(4096, tag='inter_b'), synthetic_inputs(20480, tag='margin_b', margin=True))
    _, _, gn_a = A.training_step(b2, opt_a, with_pde=True, max_norm=max_norm)
    _, _, gn_b = B.training_step(b2, opt_b, with_pde=True, max_norm=max_norm)
    gn_a, gn_b = float(gn_a), float(gn_b)
    agree = [(n_, float((pa - pb).abs().max())) for (n_, pa), pb in zip(A.physics_net.named_parameters(), B.physics_net.parameters())
             if not torch.allclose(pa, pb, rtol=2e-5, atol=2e-7)]
    print('  FusedClipAdam vs torch.optim.Adam, step 2: gnorm %.7e vs %.7e; %d tensors outside allclose' % (gn_a, gn_b, len(agree)))
    assert int(opt_a.step_count) == 2
    assert abs(gn_a - gn_b) <= 1e-5 * gn_b, (gn_a, gn_b)
    assert not agree, agree


def test_step_losses_rejects_a_bad_split():
    """_StepLossFn takes every launch's row count from the interior / margin split: a split that leaves a group empty, or a label count
    that is not the margin group's, raises ValueError (not an assert, which `python -O` removes) before anything is launched."""
    from deepphysinet_amd.point_path import step_losses
    m = _model('bf16x2')
    g = _gpu(synthetic_inputs(64, tag='margin', margin=True))
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        for n_inter, n_lab in ((0, 64), (64, 0), (40, 23)):
            with pytest.raises(ValueError, match='n_inter = %d of 64 points' % n_inter):
                step_losses(cfg, n_inter, g['x'], g['y'], g['t'], g['f'], g['coord_data'], g['labels'][:n_lab], heads, evec, statics)


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
def test_full_grid_properties(prec):
    """N = 37 265 (BASELINE config[1]): the oracle is too slow there, so check what must hold at any size:
    (1) mean-of-residuals is additive over a partition of the points; (2) permuting the points changes nothing;
    (3) a 2048-point prefix agrees with the oracle run on that prefix."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synth_batch
    n = 257 * 145
    m = _model(prec)
    b = synth_batch(n, _dev(), seed=3)

    def terms(sel):
        return m.pde_loss_terms(b['x'][sel], b['y'][sel], b['t'][sel], b['f'][sel], b['field_data'], b['coord_data'][sel],
                                b['forecast_h']).detach().double().cpu().numpy()
    full = terms(slice(None))
    assert np.all(np.isfinite(full))
    cut = 20001
    a, c = terms(slice(0, cut)), terms(slice(cut, n))
    comb = (a * cut + c * (n - cut)) / n
    assert np.all(np.abs(comb - full) <= 2e-5 * np.abs(full)), (comb, full)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(_dev())
    assert np.all(np.abs(terms(perm) - full) <= 2e-5 * np.abs(full))
    # gradients: additive as well (checked on two tensors of different kinds)
    def grads(sel, scale):
        m.physics_net.zero_grad()
        (m.pde_loss_terms(b['x'][sel], b['y'][sel], b['t'][sel], b['f'][sel], b['field_data'], b['coord_data'][sel],
                          b['forecast_h']).sum() * scale).backward()
        p = dict(m.physics_net.named_parameters())
        return [p[k].grad.detach().double().cpu() for k in ('U_net.cat_fc1.fc.0.weight', 'q_net.coord_hidden_fc.weight', 'meta_net.model.projection.weight')]
    gf = grads(slice(None), 1.0)
    ga, gc = grads(slice(0, cut), cut / n), grads(slice(cut, n), (n - cut) / n)
    for f_, a_, c_ in zip(gf, ga, gc):
        assert float((a_ + c_ - f_).abs().max() / f_.abs().max()) < (2e-4 if prec == 'bf16x2' else 2e-2)
    # oracle on a prefix of the same synthetic batch
    k = 2048
    cpu = {kk: v[:k].cpu() if v.shape[0] == n else v.cpu() for kk, v in b.items()}
    st = {kk: v.detach().cpu() for kk, v in m.physics_net.state_dict().items()}
    x, y, t = (cpu[kk].clone().requires_grad_(True) for kk in ('x', 'y', 't'))
    _, parts, _, _ = O.place_one_batch(st, x, y, t, cpu['f'], cpu['field_data'], cpu['coord_data'], cpu['forecast_h'], GEO, return_parts=True)
    ref = np.array([float(p.detach()) for p in parts])
    if prec == 'bf16x2':
        # parity-grade mode: the prefix's points whose switch bits differ from the oracle arithmetic's are named and removed from both sides
        # (default-init weights put many P / T / q / rho values near a clip bound), the remaining points' six terms are held to 1e-4
        mine, ref_ff, idx = _terms_vs_oracle_flip_free(m, cpu, st=st)
        print('full grid, 2048-point prefix: removed points', idx)
        assert np.all(np.abs(mine - ref_ff) <= TOL[prec]['loss'] * np.abs(ref_ff)), (mine, ref_ff, idx)
    else:
        assert np.all(np.abs(terms(slice(0, k)) - ref) <= 3 * TOL[prec]['loss'] * np.abs(ref)), (terms(slice(0, k)), ref)


def test_fused_clip_adam_equals_torch():
    """FusedClipAdam (dpn_clip_adam_flat_dev on the optimiser's flat buffers) vs clip_grad_norm_ + torch.optim.Adam(weight_decay) over three
    steps, with the clip active and inactive: parameters and both moments.  The fp64 bounds, the other two entry points and the multi-table
    launches are tests/test_gpu_optim.py's."""
    from deepphysinet_amd.optim import FusedClipAdam
    dev = _dev()
    for max_norm in (1e9, 0.5):
        torch.manual_seed(0)
        shapes = [(256, 193), (7,), (1, 128, 256), (300, 17), (1,)] * 20            # 100 tensors: ONE table of the flat form (160 per launch)
        a = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes]
        b = [t.detach().clone().requires_grad_(True) for t in a]
        ref = torch.optim.Adam(a, lr=1e-3, weight_decay=1e-2)
        mine = FusedClipAdam(b, lr=1e-3, weight_decay=1e-2, max_norm=max_norm)
        for it in range(3):
            gs = [torch.randn_like(t) * (1 + it) for t in a]
            for t, u, g in zip(a, b, gs):
                t.grad = g.clone(); u.grad = g.clone()
            n_ref = torch.nn.utils.clip_grad_norm_(a, max_norm=max_norm)
            ref.step()
            n_mine = mine.step()
            assert abs(float(n_mine) - float(n_ref)) <= 1e-5 * float(n_ref)
            for t, u, m, v in zip(a, b, mine.exp_avg, mine.exp_avg_sq):
                assert torch.allclose(t, u, rtol=2e-5, atol=2e-7)
                assert torch.allclose(ref.state[t]['exp_avg'], m, rtol=2e-5, atol=2e-7)
                assert torch.allclose(ref.state[t]['exp_avg_sq'], v, rtol=2e-5, atol=2e-7)
        assert int(mine.step_count) == 3


def test_config0_one_degree_grid_data_loss_only():
    """BASELINE configs[0]: 1-degree grid (65 x 37, dx = dy = 108 km), 2405 grid nodes at one lead time, data loss only."""
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    lon, lat, dx = 65, 37, 108000.0
    inp = synthetic_inputs(lon * lat, lon=lon, lat=lat, dx=dx, dy=dx, tag='cfg0', margin=True)
    geo = O.Geometry(lon=lon, lat=lat, dx=dx, dy=dx)
    st = O.make_state(requires_grad=True)
    ref = O.data_loss(st, inp['x'], inp['y'], inp['t'], inp['field_data'], inp['coord_data'], inp['labels'], inp['forecast_h'], geo)
    names = O.param_names(st)
    ref_g = dict(zip(names, torch.autograd.grad(ref, [st[n] for n in names])))
    m = builder_models(**ncep_config(img_size=(lat, lon), dx=dx, dy=dx), precision='bf16x2')
    sd = m.physics_net.state_dict(); fill_state_dict_(sd); m.physics_net.load_state_dict(sd)
    m = m.to(_dev())
    g = _gpu(inp)
    loss = m.data_loss(g['x'], g['y'], g['t'], g['field_data'], g['coord_data'], g['labels'], g['forecast_h'])
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 5e-5 * float(ref.detach())
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        r = ref_g[name]
        assert float((p.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-30)) < 5e-3, name


def test_config2_forecast_lead_batch_is_a_loop_of_single_fields(golden_dir):
    """BASELINE configs[2] (61 forecast leads): the reference cannot batch fields, so parity is a loop of
    single-field calls.  Three leads of the 61 (0 h, 24 h, 336 h): encoder output vs fixture F2 and PDE losses vs the oracle."""
    d = np.load(os.path.join(golden_dir, 'f2_encoder.npz'))
    m = _model('bf16x2')
    inp = synthetic_inputs(1024, tag='inter')
    for h in (0, 24, 336):
        fh = torch.full((1, 1, 1), h / 360.0)
        with torch.no_grad():
            mo = m.physics_net.meta_net(inp['field_data'].to(_dev()), fh.to(_dev())).cpu().numpy()
        ref_mo = d['meta_out_h%d' % h]
        assert np.abs(mo - ref_mo).max() <= 5e-6 * np.abs(ref_mo).max()
        b = dict(inp, forecast_h=fh)
        ref = _oracle(b, want_grads=False)
        g = _gpu(b)
        terms = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).detach().cpu().numpy()
        # The clip in inverse_norm makes the loss discontinuous: a point whose q / T / P sits on a bound to within the 16-bit
        # operand precision can land on the other side (the CPU emulation of the split arithmetic, oracle/kernel_model.py with
        # prec='bf16x2', reproduces the very same deviations: 2e-3 on `energy` at h = 0 for the first 192 points).  One such
        # point moves a batch mean by O(1/N); everything continuous (fields, losses of the other leads) stays at 1e-5.
        rel = np.abs(terms - ref['parts']) / np.abs(ref['parts'])
        if not np.all(rel <= 1e-4):                          # name the points that changed sides, hold the rest to the north-star bar
            mine, ref_ff, idx = _terms_vs_oracle_flip_free(m, b)
            print('lead %d h: removed points %s' % (h, idx))
            assert idx and np.all(np.abs(mine - ref_ff) <= 1e-4 * np.abs(ref_ff)), (h, idx, mine, ref_ff)
        import deepphysinet_amd as dpn
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
            out_n, _ = dpn.pde_fields_and_jacobian(m.point_config(), g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
        assert float((out_n.cpu() - ref['fields']).abs().max() / ref['fields'].abs().max()) < 5e-5


def test_encoder_kernels_gradients_vs_torch():
    """dpn_attn_* / dpn_add_ln_* / dpn_sgemm_batch against the same expressions in torch autograd on the GPU."""
    from deepphysinet_amd.encoder_ops import add_layer_norm, attention
    from deepphysinet_amd.linear import linear, linear_multi
    dev = _dev()
    torch.manual_seed(0)
    L_ = 287
    q, k, v = (torch.randn(1, L_, 8, 32, device=dev, requires_grad=True) for _ in range(3))
    o = attention(q, k, v)
    o_ref = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
    assert torch.allclose(o, o_ref, rtol=1e-4, atol=1e-5)
    go = torch.randn_like(o)
    g1 = torch.autograd.grad(o, (q, k, v), go)
    g2 = torch.autograd.grad(o_ref, (q, k, v), go)
    for a_, b_ in zip(g1, g2):
        assert float((a_ - b_).abs().max() / b_.abs().max()) < 2e-4
    x = torch.randn(1, L_, 256, device=dev, requires_grad=True)
    r = torch.randn(1, L_, 256, device=dev, requires_grad=True)
    ln = torch.nn.LayerNorm(256).to(dev)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5); ln.bias.uniform_(-0.5, 0.5)
    y = add_layer_norm(x, r, ln)
    y_ref = ln(x + r)
    assert torch.allclose(y, y_ref, rtol=1e-5, atol=1e-5)
    gy = torch.randn_like(y)
    g1 = torch.autograd.grad(y, (x, r, ln.weight, ln.bias), gy)
    g2 = torch.autograd.grad(y_ref, (x, r, ln.weight, ln.bias), gy)
    for a_, b_ in zip(g1, g2):
        assert float((a_ - b_).abs().max() / b_.abs().max()) < 1e-4
    ws = [torch.randn(256, 256, device=dev, requires_grad=True) for _ in range(3)]
    bs = [torch.randn(256, device=dev, requires_grad=True) for _ in range(3)]
    x2 = torch.randn(L_, 256, device=dev, requires_grad=True)
    ys = linear_multi(x2, ws, bs)
    ys_ref = [torch.nn.functional.linear(x2, w, b) for w, b in zip(ws, bs)]
    gs = [torch.randn_like(y_) for y_ in ys]
    g1 = torch.autograd.grad(ys, [x2] + ws + bs, gs)
    g2 = torch.autograd.grad(ys_ref, [x2] + ws + bs, gs)
    for a_, b_ in zip(ys, ys_ref):
        assert torch.allclose(a_, b_, rtol=1e-4, atol=1e-4)
    for a_, b_ in zip(g1, g2):
        assert float((a_ - b_).abs().max() / b_.abs().max()) < 1e-4
    # long-K path (token embedding shape): deterministic two-pass split-K
    xa = torch.randn(159, 7215, device=dev); wa = torch.randn(256, 7215, device=dev, requires_grad=True); ba = torch.randn(256, device=dev)
    ya = linear(xa, wa, ba)
    assert float((ya - torch.nn.functional.linear(xa, wa, ba)).abs().max() / ya.abs().max()) < 1e-5
    assert torch.equal(ya, linear(xa, wa, ba))


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
def test_batched_weight_packing_and_loss_finish_are_bitwise_the_per_field_launches(prec):
    """Lead batches (configs[2]) pack the weight blocks of all fields in ONE dpn_pack_weights_batch launch and finish the losses of all fields in ONE
    dpn_residual_finish_batch launch (round 6; per field before: 61 x (17 + 4.6) us of a 51-ms step).  Same arithmetic, other grid: every field's
    packed block must equal dpn_pack_weights_form's byte for byte (both packed forms), and pde_losses_batch must give torch.equal losses and
    gradients with the switch on and off (DPN_BATCH_PACK)."""
    import ctypes
    from deepphysinet_amd import _lib as L, config as C, point_path as PP
    dev = _dev()
    B, n = 3, 700
    g = torch.Generator(device='cpu').manual_seed(5)
    heads = (torch.randn(B, 256, PP.HEADS_COLS, generator=g) * 0.05).to(dev)
    evec = (torch.randn(B, 6, 256, generator=g) * 0.05).to(dev)
    statics = [(torch.randn(*PP.STATIC_SHAPES[j % 8], generator=g) * 0.05).to(dev) for j in range(48)]
    lib = L.load()
    pr = 2 if prec == 'bf16x2' else 1
    sizes = L.DpnSizes()
    L.check(lib.dpn_sizes(n, pr, ctypes.byref(sizes)), 'dpn_sizes')
    stride = (int(sizes.packed) + 255) // 256 * 256
    for form in (0, 1):
        if form == 1 and pr != 2:
            continue
        batch = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
        L.check(lib.dpn_pack_weights_batch(PP._net_ptrs(heads[0], evec[0], statics), B, heads.stride(0), evec.stride(0), pr, form, PP._ptr(batch), stride,
                                           PP._stream()), 'batch')
        for b in range(B):
            one = torch.zeros(int(sizes.packed), dtype=torch.uint8, device=dev)
            L.check(lib.dpn_pack_weights_form(PP._net_ptrs(heads[b], evec[b], statics), pr, form, PP._ptr(one), PP._stream()), 'one')
            assert torch.equal(batch[b, :int(sizes.packed)], one), (form, b)
    # the step on top of it: losses and every parameter gradient with the switch on and off
    Bm, N = 3, 300
    m = _model(prec)
    lf = m.train_cfg['losses']['loss_factor']
    samples = [_gpu(synthetic_inputs(N, GEO.lon, GEO.lat, GEO.dx, GEO.dy, tag='lead%d' % b, forecast_h=24.0 * b / 360.0)) for b in range(Bm)]
    stack = lambda k: torch.stack([g_[k].reshape(-1) if g_[k].dim() == 2 and g_[k].shape[1] == 1 else g_[k] for g_ in samples])
    x, y, t, f = (stack(k) for k in ('x', 'y', 't', 'f'))
    field = torch.cat([g_['field_data'] for g_ in samples], dim=0)
    cd = torch.stack([g_['coord_data'] for g_ in samples])
    fh = torch.cat([g_['forecast_h'] for g_ in samples], dim=0)
    res = []
    for on in (True, False):
        with C.override(batch_pack=on):
            m.physics_net.zero_grad(set_to_none=True)
            loss, terms = m.place_lead_batch(x, y, t, f, field, cd, fh, torch.nn.MSELoss(), lf, reduction='sum')
            loss.backward()
            res.append((loss.detach().clone(), terms.detach().clone(), {n_: p.grad.detach().clone() for n_, p in m.physics_net.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for n_ in res[0][2]:
        assert torch.equal(res[0][2][n_], res[1][2][n_]), n_


def test_embedding_assembled_inside_the_stacks_first_launch_is_bitwise_the_separate_launch():
    """Round 6: for one field on the fused path the encoder stack's first launch assembles x0 = cat(learnable_token, token convolution) + positional table +
    lead-time embedding from the convolution's split-K slices itself (DpnEncFwd.emb_*) instead of reading what dpn_embed_assemble wrote in a launch of its
    own (DPN_EMBED_DEFER=0).  Same additions in the same order: x0, the encoder output, the loss and every parameter gradient must be torch.equal; the
    standalone embedding (nobody to take the assembly over) and a batch of fields must not defer."""
    from deepphysinet_amd import config as C, encoder_ops as E
    m = _model('bf16x2')
    net = m.physics_net
    g = _gpu(synthetic_inputs(300, GEO.lon, GEO.lat, GEO.dx, GEO.dy, tag='inter'))
    lf = m.train_cfg['losses']['loss_factor']
    res = []
    for on in (True, False):
        with C.override(embed_defer=on):
            net.zero_grad(set_to_none=True)
            meta = net.encode_field(g['field_data'], g['forecast_h'], keep_embedding=True)
            x0 = net.meta_net.model.last_embedding
            assert x0 is not None
            x0c, metac = x0.detach().clone(), meta.detach().clone()
            net.clear_field_cache()
            loss = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.MSELoss(), lf, 0, 0,
                                     g['x'].device)
            loss.backward()
            res.append((x0c, metac, loss.detach().clone(), {n_: p.grad.detach().clone() for n_, p in net.named_parameters()}))
    assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    for n_ in res[0][3]:
        assert torch.equal(res[0][3][n_], res[1][3][n_]), n_
    # the embedding alone: assembled by its own launch whatever the switch says (its output must be valid when it returns)
    tn = net.meta_net.model
    with C.override(embed_defer=True):
        alone = E.data_embedding_fused(g['field_data'], tn.enc_embedding, tn.learnable_token, g['forecast_h'])
        torch.cuda.synchronize()
    assert alone is not None and torch.equal(alone.detach().reshape(res[0][0].shape), res[0][0])


@pytest.mark.parametrize('rows', [287, 2 * 287, 61 * 287])
def test_wgrad16_mixed_problem_lists_vs_fp64(rows):
    """dpn_wgrad16 (dW = G^T X, db = column sums of G; f16 hi+lo MFMA with running power-of-two scales): lists whose problems differ in tile
    counts -- the launch's grid is the LIST of the tiles that exist (round 6), so every problem of a ragged list must still be decoded to its
    own tiles: equal 4 x 4 problems, 8 x 4 and 4 x 8 ones among them, the stack's 25 + the token convolution's 4 x 113, the convolution
    alone; one row slice (a single field), two, and a lead batch's row count (slices joined by the reduce launch).  Bound: 2e-6 of the
    tensor's maximum (measured 2e-7 .. 6e-7), bias sums 3e-6 of theirs (fp32 sums over the rows: measured 5e-7)."""
    from deepphysinet_amd.encoder_ops import wgrad16
    dev = _dev()
    g = torch.Generator(device='cpu').manual_seed(11)
    lists = ([(256, 256)] * 6, [(256, 256)] * 4 + [(512, 256), (256, 512)], [(256, 256)] * 25 + [(256, 7215)], [(256, 7215)])
    if rows > 1000:
        lists = lists[1:2]                                        # the lead-batch row count: one ragged list (an 8-MB X per 7 215-column problem otherwise)
    for shapes in lists:
        G = [torch.randn(rows, m, generator=g).to(dev) for m, n in shapes]
        X = [torch.randn(rows, n, generator=g).to(dev) for m, n in shapes]
        dW = [torch.full((m, n), float('nan'), device=dev) for m, n in shapes]
        db = [torch.full((m,), float('nan'), device=dev) for m, n in shapes]
        keep = wgrad16(list(zip(G, X, dW, db)))
        torch.cuda.synchronize()
        del keep
        for i, (g_, x_, w_, b_) in enumerate(zip(G, X, dW, db)):
            ref = g_.double().T @ x_.double()
            bref = g_.double().sum(0)
            ew = float((w_.double() - ref).abs().max() / ref.abs().max())
            eb = float((b_.double() - bref).abs().max() / bref.abs().max())
            assert ew < 2e-6 and eb < 3e-6, (rows, len(shapes), i, ew, eb)
    if rows == 287:
        # the ride-along jobs (LayerNorm parameter sums: out_a[c] = sum_b partial[b][c], out_b[c] = sum_b partial[b][256 + c]) sit BEHIND the list of tiles:
        # with problems in front of them, and alone (a launch that carries only jobs)
        nb = 18
        parts = [torch.randn(nb, 512, generator=g).to(dev) for _ in range(3)]
        outs = [(torch.full((256,), float('nan'), device=dev), torch.full((256,), float('nan'), device=dev)) for _ in range(3)]
        G = [torch.randn(rows, 256, generator=g).to(dev) for _ in range(2)]
        X = [torch.randn(rows, 256, generator=g).to(dev) for _ in range(2)]
        dW = [torch.empty(256, 256, device=dev) for _ in range(2)]
        db = [torch.empty(256, device=dev) for _ in range(2)]
        wgrad16(list(zip(G, X, dW, db)), [(parts[0], outs[0][0], outs[0][1], nb), (parts[1], outs[1][0], outs[1][1], nb)])
        wgrad16([], [(parts[2], outs[2][0], outs[2][1], nb)])
        torch.cuda.synchronize()
        for p_, (oa, ob) in zip(parts, outs):
            assert torch.allclose(oa, p_[:, :256].sum(0), rtol=1e-5, atol=1e-5) and torch.allclose(ob, p_[:, 256:].sum(0), rtol=1e-5, atol=1e-5)
        assert float((dW[1].double() - G[1].double().T @ X[1].double()).abs().max()) < 1e-4


@pytest.mark.parametrize('B', [1, 3])
def test_fused_encoder_nodes_vs_torch_autograd(B):
    """The hand-scheduled autograd nodes of encoder_ops (whole EncoderLayer, data embedding, hyper-network heads) against the reference's
    own torch expressions (transformer_net.py:28-44, embed.py:36-64, variable_net.py:57-65,75-78) evaluated by torch autograd on the GPU,
    for one field sample and for a batch of B field samples (BASELINE configs[2]: distinct fields / lead times in one step)."""
    import torch.nn.functional as F
    from deepphysinet_amd.model import meta_net as MN
    from deepphysinet_amd.model.variable_net import VariableNet
    from deepphysinet_amd.encoder_ops import _HeadsFn, lead_time_pe
    dev = _dev()
    torch.manual_seed(3)

    def rel(a_, b_):
        return float(((a_ - b_).abs().max() / b_.abs().max().clamp_min(1e-30)).detach())

    # ---- EncoderLayer: fused node vs the per-op expression in plain torch
    layer = MN.EncoderLayer(MN.AttentionLayer(MN.FullAttention(False), 256, 8), 256, 256, activation='gelu').to(dev)
    x = torch.randn(B, 287, 256, device=dev, requires_grad=True)
    y, _ = layer(x)

    def layer_ref(x):
        a = layer.attention
        q, k, v = (F.linear(x, m.weight, m.bias).view(B, 287, 8, 32).transpose(1, 2) for m in (a.query_projection, a.key_projection, a.value_projection))
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, 287, 256)
        x1 = layer.norm1(x + F.linear(o, a.out_projection.weight, a.out_projection.bias))
        h = F.gelu(F.linear(x1, layer.conv1.weight.squeeze(-1), layer.conv1.bias))
        return layer.norm2(x1 + F.linear(h, layer.conv2.weight.squeeze(-1), layer.conv2.bias))
    y_ref = layer_ref(x)
    assert y.shape == y_ref.shape and rel(y, y_ref) < 2e-5
    gy = torch.randn_like(y)
    names = ['x'] + [n_ for n_, _ in layer.named_parameters()]
    params = [x] + list(layer.parameters())
    for n_, a_, b_ in zip(names, torch.autograd.grad(y, params, gy), torch.autograd.grad(y_ref, params, gy)):
        if n_ == 'attention.key_projection.bias':
            continue                                            # mathematically zero (softmax shift invariance): pure rounding noise
        assert a_.shape == b_.shape and rel(a_, b_) < 3e-4, (n_, rel(a_, b_))

    # ---- DataEmbedding + learnable tokens: fused node vs Conv1d(circular) + cat + pos + time embedding
    emb = MN.DataEmbedding(2405, 256).to(dev)
    token = torch.rand(1, 128, 256, device=dev, requires_grad=True)
    field = torch.randn(B, 159, 2405, device=dev)
    h = torch.linspace(0.1, 0.9, B, device=dev).view(B, 1, 1)
    e = emb(field, h, token)
    conv = emb.value_embedding.tokenConv
    e_ref = torch.cat([token.expand(B, -1, -1), conv(field.permute(0, 2, 1)).transpose(1, 2)], dim=1)
    e_ref = e_ref + emb.position_embedding(e_ref) + emb.time_embending(h)
    assert e.shape == e_ref.shape and rel(e, e_ref) < 1e-5
    ge = torch.randn_like(e)
    for a_, b_ in zip(torch.autograd.grad(e, [token, conv.weight, conv.bias], ge), torch.autograd.grad(e_ref, [token, conv.weight, conv.bias], ge)):
        assert a_.shape == b_.shape and rel(a_, b_) < 1e-4
    assert torch.equal(lead_time_pe(h, emb.time_embending.freq_bands).reshape(-1), emb.time_embending(h).reshape(-1))     # same sin/cos, same order

    # ---- hyper-network heads + lead-time embeddings of six VariableNets
    nets = [VariableNet(256, 192, 256).to(dev) for _ in range(6)]
    meta = torch.randn(B, 287, 256, device=dev, requires_grad=True)
    pe_h = lead_time_pe(h, nets[0].pe_fore_h.freq_bands).reshape(B, 192)
    args = ([n.coord_input_fc.weight for n in nets] + [n.coord_hidden_fc.weight for n in nets] + [n.coord_input_fc.bias for n in nets]
            + [n.coord_hidden_fc.bias for n in nets] + [n.fore_h_fc.weight for n in nets] + [n.fore_h_fc.bias for n in nets])
    heads, evec = _HeadsFn.apply(meta, pe_h, *args)
    heads_ref = torch.stack([torch.cat([n.coord_input_fc(meta[f, :256].T) for n in nets] + [n.coord_hidden_fc(meta[f, :256].T) for n in nets], dim=1)
                             for f in range(B)])
    evec_ref = torch.stack([torch.stack([n.fore_h_fc(n.pe_fore_h(h[f].reshape(1, 1)))[0] for n in nets]) for f in range(B)])
    assert heads.shape == (B, 256, 2700) and rel(heads, heads_ref) < 1e-5 and rel(evec, evec_ref) < 1e-5
    gh, gv = torch.randn_like(heads), torch.randn_like(evec)
    g1 = torch.autograd.grad([heads, evec], [meta] + args, [gh, gv])
    g2 = torch.autograd.grad([heads_ref, evec_ref], [meta] + args, [gh, gv])
    for a_, b_ in zip(g1, g2):
        assert a_.shape == b_.shape and rel(a_, b_) < 1e-4
    assert float(g1[0][:, 256:].abs().max()) == 0.0            # tokens 256..286 feed no VariableNet (variable_net.py:58)


def test_full_grid_step_is_bitwise_deterministic():
    """No kernel on the path uses atomics (loss, weight-gradient and gradient-norm reductions are fixed-order): two executions of the
    full-size step from the same state give bit-identical losses and gradients -- a size-independent property at BASELINE's size."""
    m = _model('bf16')
    g = _gpu(synthetic_inputs(257 * 145, GEO.lon, GEO.lat, GEO.dx, GEO.dy))
    lf = m.train_cfg['losses']['loss_factor']
    outs = []
    for _ in range(2):
        m.physics_net.zero_grad(set_to_none=True)
        loss = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.MSELoss(), lf, 0, 0,
                                 _dev())
        loss.backward()
        outs.append((loss.detach().clone(), [p.grad.detach().clone() for p in m.physics_net.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a_, b_ in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a_, b_)


def test_lead_batch_backward_paths_agree():
    """pde_losses_batch runs each field's point backward right behind its forward (unit cotangent of the field's total, scaled when the real
    cotangent arrives).  Against it: the same function with the state parked until the backward pass (DPN_BATCH_EAGER_BACKWARD=0 path), and
    the general path a cotangent on the individual loss terms takes (forward again) -- gradients of the heads, the lead-time embeddings and
    two static tensors, all three ways."""
    from deepphysinet_amd import point_path as PP
    B, N = 3, 300
    m = _model('bf16x2')
    samples = [synthetic_inputs(N, GEO.lon, GEO.lat, GEO.dx, GEO.dy, tag='eager%d' % b, forecast_h=24.0 * b / 360.0) for b in range(B)]
    g = [_gpu(s_) for s_ in samples]
    x, y, t, f = (torch.stack([g_[k].reshape(-1) for g_ in g]) for k in ('x', 'y', 't', 'f'))
    cd = torch.stack([g_['coord_data'] for g_ in g])
    cfg = m.point_config()
    with torch.no_grad():
        hw = [m.physics_net.field_weights(g_['field_data'], g_['forecast_h']) for g_ in g]
    heads0 = torch.stack([h[0] for h in hw])
    evec0 = torch.stack([h[1] for h in hw])
    statics = [s_.detach().clone().requires_grad_(True) for s_ in hw[0][2]]
    wts = torch.tensor([0.5, 2.0, 1.25], device=_dev())

    def run(eager, through_terms):
        heads, evec = heads0.clone().requires_grad_(True), evec0.clone().requires_grad_(True)
        from deepphysinet_amd import config
        with config.override(batch_eager_backward=eager):
            losses, totals = PP.pde_losses_batch(cfg, x, y, t, f, cd, heads, evec, statics)
            obj = (losses.sum(dim=1) * wts).sum() if through_terms else (totals * wts).sum()
            got = torch.autograd.grad(obj, [heads, evec, statics[0], statics[2]])
        return [v.detach().clone() for v in got]

    base = run(False, False)                                 # state parked, cotangents known before the point backward runs
    for name, other in (('eager', run(True, False)), ('terms', run(True, True)), ('terms, parked', run(False, True))):
        for a_, b_ in zip(base, other):
            # the same kernels; the eager path multiplies by the cotangent AFTER the reductions instead of before (one rounding per element),
            # the per-term path adds six cotangents where the other adds one total (the reference's summation order of the total differs
            # from sum(dim=1) in the last bit)
            assert float((a_ - b_).abs().max()) <= 2e-5 * float(a_.abs().max()), name


def test_config2_lead_batch_in_one_step_equals_the_loop():
    """BASELINE configs[2] as ONE step: place_lead_batch over B field samples (batched encoder, per-field point kernels, fixed-order
    sums of the per-field parameter gradients) against (i) the CPU oracle per field and (ii) the same samples pushed one by one through
    place_one_batch -- losses and all parameter gradients."""
    B, N = 5, 256                                            # 5 x 287 rows: the batched encoder takes the long-reduction (split-K) path
    m = _model('bf16x2')
    lf = m.train_cfg['losses']['loss_factor']
    crit = torch.nn.MSELoss()
    samples = [synthetic_inputs(N, GEO.lon, GEO.lat, GEO.dx, GEO.dy, tag='lead%d' % b, forecast_h=24.0 * b / 360.0) for b in range(B)]
    g = [_gpu(s_) for s_ in samples]
    stack = lambda k: torch.stack([g_[k].reshape(-1) if g_[k].dim() == 2 and g_[k].shape[1] == 1 else g_[k] for g_ in g])
    x, y, t, f = (stack(k) for k in ('x', 'y', 't', 'f'))
    field = torch.cat([g_['field_data'] for g_ in g], dim=0)
    cd = torch.stack([g_['coord_data'] for g_ in g])
    fh = torch.cat([g_['forecast_h'] for g_ in g], dim=0)
    m.physics_net.zero_grad(set_to_none=True)
    loss, terms = m.place_lead_batch(x, y, t, f, field, cd, fh, crit, lf, reduction='sum')
    loss.backward()
    got = {n_: p.grad.detach().clone() for n_, p in m.physics_net.named_parameters()}
    assert terms.shape == (B, 6)
    # (i) oracle, field by field
    for b in range(B):
        ref = _oracle(samples[b], want_grads=False)
        rel = np.abs(terms[b].detach().cpu().numpy() - ref['parts']) / np.abs(ref['parts'])
        if not np.all(rel <= 1e-4):                          # name the points that changed sides (single-field path, same point kernels), rest at 1e-4
            mine, ref_ff, idx = _terms_vs_oracle_flip_free(m, samples[b])
            print('lead batch field %d: removed points %s' % (b, idx))
            assert idx and np.all(np.abs(mine - ref_ff) <= 1e-4 * np.abs(ref_ff)), (b, idx, mine, ref_ff)
    # (ii) the loop of single-field steps on the same kernels
    m.physics_net.zero_grad(set_to_none=True)
    total = 0.0
    for b in range(B):
        l_b = m.place_one_batch(g[b]['x'], g[b]['y'], g[b]['t'], g[b]['f'], g[b]['field_data'], g[b]['coord_data'], g[b]['forecast_h'], crit, lf, 0, 0,
                                _dev())
        l_b.backward()
        total += float(l_b.detach())
    # Since round 4 the encoder's arithmetic does not depend on the batch: the row-local fused nodes scale and multiply row by row, the token
    # convolution runs the same split-K form for one field and for five, the hyper-network heads of a batch are bit-identical to a single
    # field's.  So the forward pass -- every loss term of every field -- is IDENTICAL, no switch can change sides, and what is left is the
    # order in which parameter gradients are summed over fields and row blocks (fp32 reassociation): every gradient element within
    # TOL['bf16x2']['grad'] of its tensor's maximum with two orders of margin, all gradients together within 1e-5.
    assert abs(float(loss.detach()) - total) <= 1e-6 * abs(total)
    for b in range(B):
        t_b = m.pde_loss_terms(g[b]['x'], g[b]['y'], g[b]['t'], g[b]['f'], g[b]['field_data'], g[b]['coord_data'], g[b]['forecast_h']).detach()
        assert torch.equal(t_b.float().cpu(), terms[b].detach().float().cpu()), (b, t_b, terms[b])
    num = den = 0.0
    for n_, p in m.physics_net.named_parameters():
        if n_.endswith('key_projection.bias'):
            continue
        a_, b_ = got[n_], p.grad
        d_ = (a_ - b_).abs()
        num += float(d_.double().pow(2).sum())
        den += float(b_.double().pow(2).sum())
        assert float(d_.max()) <= 0.02 * TOL['bf16x2']['grad'] * float(b_.abs().max()) + 1e-30, (n_, float(d_.max()), float(b_.abs().max()))
    assert (num / den) ** 0.5 <= 1e-5, (num / den) ** 0.5


def test_error_behaviour_matches_the_reference_convention():
    """Plain Python exceptions (the reference's convention, interface/build.py:20): RuntimeError for what the kernels cannot take,
    NotImplementedError for unsupported configuration -- never a silent fallback."""
    import deepphysinet_amd as dpn
    m = _model('bf16x2')
    g = _gpu(synthetic_inputs(64, GEO.lon, GEO.lat, GEO.dx, GEO.dy))
    lf = m.train_cfg['losses']['loss_factor']
    with pytest.raises(NotImplementedError):
        m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.HuberLoss(), lf, 0, 0, _dev())
    with pytest.raises(RuntimeError):                       # zero collocation points: the C ABI refuses n <= 0
        e = torch.empty(0, device=_dev())
        m.place_one_batch(e, e, e, e, g['field_data'], torch.empty(0, 6, device=_dev()), g['forecast_h'], torch.nn.MSELoss(), lf, 0, 0, _dev())
    with pytest.raises(RuntimeError):                       # host tensors: no CPU fallback
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        dpn.pde_fields_and_jacobian(m.point_config(), g['x'].cpu(), g['y'].cpu(), g['t'].cpu(), g['coord_data'].cpu(), heads, evec, statics)
    with pytest.raises(ValueError):
        m.predict_grid(g['field_data'], g['x'], g['y'], g['t'], g['coord_data'], g['forecast_h'])      # needs all lon x lat nodes


def test_hipgraph_replays_equal_eager_steps():
    """bench.py times replays of ONE captured step.  Three replays must leave the model exactly where three eager steps from the same
    state leave it (the Adam step counter lives on the device; nothing is cached between replays): bitwise equal parameters."""
    from deepphysinet_amd.optim import FusedClipAdam
    dev = _dev()
    g = _gpu(synthetic_inputs(1024, GEO.lon, GEO.lat, GEO.dx, GEO.dy))
    crit = torch.nn.MSELoss()

    def make():
        m = _model('bf16')
        opt = FusedClipAdam(m.physics_net.parameters(), lr=1e-3, weight_decay=1e-4, max_norm=2.5e7)
        lf = m.train_cfg['losses']['loss_factor']
        one = torch.ones((), device=dev)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], crit, lf, 0, 0, dev)
            loss.backward(one)
            opt.step()
            return loss
        return m, opt, step
    # eager: 2 (warm-up) + 1 (the step a capture executes... it does not: capture only records) + 3 steps
    m1, opt1, step1 = make()
    for _ in range(2 + 3):
        step1()
    # graph: 2 eager warm-up steps on a side stream (as bench.py does), capture, 3 replays
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
        step2()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt1.step_count) == int(opt2.step_count) == 5
    for (n_, a_), (_, b_) in zip(m1.physics_net.named_parameters(), m2.physics_net.named_parameters()):
        assert torch.equal(a_, b_), n_


def test_layernorm_folded_into_gemm_both_modes():
    """dpn_sgemm_ln through the C ABI against torch: mode 1 (LayerNorm forward of x + r feeds the GEMM; the backward of the encoder layer
    uses mode 2, the forward keeps the two-launch form because it measured faster) and mode 2 (LayerNorm backward feeds the GEMM)."""
    import torch.nn.functional as F
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.linear import _launch_ln
    dev = _dev()
    torch.manual_seed(11)
    M, N = 287, 192
    x, r = torch.randn(M, 256, device=dev), torch.randn(M, 256, device=dev)
    gamma, beta = torch.rand(256, device=dev) + 0.5, torch.randn(256, device=dev)
    W, b = torch.randn(N, 256, device=dev) / 16, torch.randn(N, device=dev)
    y, xhat, rstd, C, pre = (torch.empty(s_, device=dev) for s_ in ((M, 256), (M, 256), (M,), (M, N), (M, N)))
    _launch_ln(1, M, N, x, r, gamma, beta, None, y, xhat, rstd, None, W, 1, 256, C, N, bias=b, epi=L.EPI_GELU, aux_out=pre)
    s = x + r
    y_ref = F.layer_norm(s, (256,), gamma, beta, 1e-5)
    rstd_ref = 1.0 / torch.sqrt(s.var(dim=1, unbiased=False) + 1e-5)
    pre_ref = y_ref @ W.T + b
    assert torch.allclose(y, y_ref, rtol=1e-5, atol=1e-5) and torch.allclose(rstd, rstd_ref, rtol=1e-5)
    assert torch.allclose(xhat, (s - s.mean(1, keepdim=True)) * rstd_ref[:, None], rtol=1e-5, atol=1e-5)
    assert torch.allclose(pre, pre_ref, rtol=1e-4, atol=1e-4) and torch.allclose(C, F.gelu(pre_ref), rtol=1e-4, atol=1e-4)
    # mode 2: gs = LayerNorm input gradient of g; C = gs . B (B stored [256][N]); partial sums of g * xhat and g per 32-row block
    g = torch.randn(M, 256, device=dev)
    Bm = torch.randn(256, N, device=dev) / 16
    gs, C2 = torch.empty(M, 256, device=dev), torch.empty(M, N, device=dev)
    nb = (M + 31) // 32
    partial = torch.empty(nb, 2, 256, device=dev)
    xh = (s - s.mean(1, keepdim=True)) * rstd_ref[:, None]
    _launch_ln(2, M, N, g, xh.contiguous(), gamma, None, rstd_ref.contiguous(), gs, None, None, partial, Bm, 0, N, C2, N)
    tg = g * gamma
    gs_ref = rstd_ref[:, None] * (tg - tg.mean(1, keepdim=True) - xh * (tg * xh).mean(1, keepdim=True))
    assert torch.allclose(gs, gs_ref, rtol=1e-4, atol=1e-5) and torch.allclose(C2, gs_ref @ Bm, rtol=1e-4, atol=1e-4)
    assert torch.allclose(partial[:, 0].sum(0), (g * xh).sum(0), rtol=1e-4, atol=1e-4) and torch.allclose(partial[:, 1].sum(0), g.sum(0), rtol=1e-4, atol=1e-4)


def test_reference_equation_methods_on_hip_module_outputs():
    """The reference's own call pattern (interface_physics.py:276-300): fields = physics_net(field, encoding_coord(x, y, t), ...),
    de-normalise, then the six *_equation methods, each taking its derivatives with gradient() = autograd.grad(..., create_graph=True).
    PhysicsNet.forward is differentiable w.r.t. the encoded coordinates (the kernel hands back d out / d pe), so the methods evaluate on
    the HIP outputs and reproduce the oracle's six losses; differentiating such a loss again raises (place_one_batch is the training path)."""
    N = 256
    m = _model('bf16x2')
    inp = synthetic_inputs(N, GEO.lon, GEO.lat, GEO.dx, GEO.dy)
    ref = _oracle(inp, want_grads=False)
    g = _gpu(inp)
    x, y, t = (g[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    lf = m.train_cfg['losses']['loss_factor']
    crit = torch.nn.MSELoss()
    pe = m.encoding_coord(x, y, t, m.pred_t_span)
    fields = m.physics_net(g['field_data'], pe, g['coord_data'], g['forecast_h'])
    u, v, p, T, q, rio = m.inverse_norm(*fields, m.obs_norm_cfg)
    f = g['f']
    losses = [m.montion_equation_u(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_u_factor']),
              m.montion_equation_v(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_v_factor']),
              m.continuous_equation(x, y, t, u, v, rio, crit, factor=lf['continuous_factor']),
              m.energy_equation(x, y, t, u, v, p, T, rio, q, crit, factor=lf['energy_factor']),
              m.vapor_equation(x, y, t, u, v, p, T, q, crit, factor=lf['vapor_factor']),
              m.gas_equation(p, T, rio, q, crit, factor=lf['gas_factor'])]
    got = np.array([float(l_.detach()) for l_ in losses])
    rel = np.abs(got - ref['parts']) / np.abs(ref['parts'])
    assert np.all(rel <= 5e-4), (got, ref['parts'], rel)      # first derivatives through torch's fp32 sin/cos chain + bf16x2 kernel
    with pytest.raises(RuntimeError):
        losses[0].backward()                                   # second-order through the standalone methods: refused loudly


def test_full_grid_all_gradients_vs_oracle():
    """configs[1] at FULL size (all 37 265 grid nodes of the bench workload's synthetic batch, closed-form weights as in every other parity
    test): the oracle's six losses and all 155 parameter gradients on every point (gradients had only been oracle-checked up
    to 5 197 points).  (With PyTorch-default weights the raw outputs have std 7-14, a fifth of the points sit within rounding distance of
    the rho >= 1e-6 clip bound where 1 / rho^2 ~ 1e12 enters the gradient, and the fp32 oracle itself is 2e-2 from the fp64 one on the
    rho net: that case is checked on its six losses only, test_default_init_full_grid_losses.)
    Bars: losses 1e-4 against the fp32 oracle (the north-star bar).  Gradients: L2 error per tensor within 1e-3 and the worst element
    within 2e-3 of the tensor's maximum -- measured against the fp64 oracle; the fp32 oracle's own distance from it is printed beside ours, and
    (since round 6) no allowance is derived from it."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synth_batch
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    tol = TOL['bf16x2']
    n = 257 * 145
    m = _model('bf16x2')
    b = synth_batch(n, _dev(), seed=3)
    m.physics_net.zero_grad(set_to_none=True)
    terms = m.pde_loss_terms(b['x'], b['y'], b['t'], b['f'], b['field_data'], b['coord_data'], b['forecast_h'])
    terms.sum().backward()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    cpu = {k: v.cpu() for k, v in b.items()}

    def oracle(dtype):
        st = {k: v.detach().cpu().to(dtype if v.is_floating_point() else v.dtype).clone().requires_grad_(v.is_floating_point() and not k.endswith('.pe'))
              for k, v in m.physics_net.state_dict().items()}
        x, y, t = (cpu[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'y', 't'))
        total, parts, _, _ = O.place_one_batch(st, x, y, t, cpu['f'].to(dtype), cpu['field_data'].to(dtype), cpu['coord_data'].to(dtype),
                                               cpu['forecast_h'].to(dtype), GEO, return_parts=True)
        names = O.param_names(st)
        return np.array([float(p.detach()) for p in parts]), dict(zip(names, torch.autograd.grad(total, [st[k] for k in names])))
    ref, g32 = oracle(torch.float32)
    _, g64 = oracle(torch.float64)
    mine = terms.detach().cpu().numpy()
    assert np.all(np.abs(mine - ref) <= tol['loss'] * np.abs(ref)), (mine, ref)
    assert len(g32) == 155

    def dist(a_, r):
        d = (a_.double() - r).abs()
        return float(d.pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-300)), float(d.max() / (r.abs().max() + 1e-300))
    rows = []
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        l2, mx = dist(p.grad.cpu(), g64[name])
        o2, ox = dist(g32[name], g64[name])
        rows.append((l2, mx, o2, ox, name))
    rows.sort(reverse=True)
    for l2, mx, o2, ox, name in rows[:6]:
        print('%-58s HIP vs fp64: L2 %.2e max %.2e | fp32 oracle vs fp64: L2 %.2e max %.2e' % (name, l2, mx, o2, ox))
    worst_mx = max(rows, key=lambda r_: r_[1])
    print('worst element of any tensor: %-44s HIP vs fp64: max %.2e | fp32 oracle vs fp64: max %.2e' % (worst_mx[4], worst_mx[1], worst_mx[3]))
    # Round 6: NO allowance derived from the fp32 oracle's own distance any more -- it never bound on these weights (measured: worst L2 5.7e-4,
    # worst element 1.36e-3; the fp32 oracle 3.1e-4 / 6.0e-4).  The element bar at this size is 2e-3, not 1e-3: nothing is removed here, and ~230 of the 37 265
    # points carry a switch bit that differs from the oracle arithmetic's (the sizes where such points ARE removed hold 1e-3 per element)
    for l2, mx, o2, ox, name in rows:
        assert l2 < tol['grad'] and mx < 2.0 * tol['grad'], (name, l2, mx, o2, ox)


def test_default_init_full_grid_losses():
    """The bench workload itself (PyTorch-default weights, seed 1, all 37 265 nodes): the six PDE losses against the fp32 oracle."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synth_batch
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    n = 257 * 145
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(_dev())
    b = synth_batch(n, _dev(), seed=1)
    with torch.no_grad():
        mine = m.pde_loss_terms(b['x'], b['y'], b['t'], b['f'], b['field_data'], b['coord_data'], b['forecast_h']).cpu().numpy()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    st = {k: v.detach().cpu() for k, v in m.physics_net.state_dict().items()}
    cpu = {k: v.cpu() for k, v in b.items()}
    x, y, t = (cpu[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    _, parts, _, _ = O.place_one_batch(st, x, y, t, cpu['f'], cpu['field_data'], cpu['coord_data'], cpu['forecast_h'], GEO, return_parts=True)
    ref = np.array([float(p.detach()) for p in parts])
    assert np.all(np.abs(mine - ref) <= TOL['bf16x2']['loss'] * np.abs(ref)), (mine, ref)


def test_config2_full_size_61_leads():
    """BASELINE configs[2] at FULL size: 61 forecast-lead field samples x 37 265 points in one step (2 273 165 points).  The oracle does
    not fit there; what must hold at any size: finite losses, the step's loss = the mean over fields, each field's six terms = what
    place_one_batch gives for that field alone (checked on the first and the last lead), finite gradients for all 155 tensors."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synth_batch
    B, n = 61, 257 * 145
    m = _model('bf16x2')
    dev = _dev()
    many = [synth_batch(n, dev, seed=1000 + k) for k in range(B)]
    lead = {k: torch.stack([b_[k].reshape(-1) for b_ in many]) for k in ('x', 'y', 't', 'f')}
    cd = torch.stack([b_['coord_data'] for b_ in many])
    field = torch.cat([b_['field_data'] for b_ in many], dim=0)
    fh = torch.arange(B, device=dev, dtype=torch.float32).mul_(6.0 / 360.0).view(-1, 1, 1)
    lf = m.train_cfg['losses']['loss_factor']
    m.physics_net.zero_grad(set_to_none=True)
    loss, terms = m.place_lead_batch(lead['x'], lead['y'], lead['t'], lead['f'], field, cd, fh, torch.nn.MSELoss(), lf)
    loss.backward()
    t_ = terms.detach().double().cpu().numpy()
    assert t_.shape == (B, 6) and np.all(np.isfinite(t_))
    totals = ((((t_[:, 0] + t_[:, 1]) + t_[:, 3]) + t_[:, 2]) + t_[:, 4]) + t_[:, 5]
    assert abs(float(loss) - totals.mean()) <= 1e-5 * abs(totals.mean())
    for k in (0, B - 1):
        single = m.pde_loss_terms(lead['x'][k], lead['y'][k], lead['t'][k], lead['f'][k], field[k:k + 1], cd[k], fh[k:k + 1]).detach().double().cpu().numpy()
        assert np.all(np.abs(single - t_[k]) <= 2e-5 * np.abs(t_[k])), (k, single, t_[k])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.physics_net.parameters())


def test_config2_eight_leads_of_4096_points_vs_the_oracle_loop():
    """`place_lead_batch` against the oracle at 8 leads x 4 096 points (was 3 x 1 024, single-field calls): eight DISTINCT field
    samples and lead times in ONE step.  The reference cannot batch fields, so the oracle side is its loop: per lead the six terms, the step's loss =
    the mean of the per-lead totals, every parameter gradient = the mean of the per-lead gradients.  Points whose ReLU / clip / vapour switch differs
    from the oracle arithmetic's are identified per lead (as everywhere in this file) and REPLACED on both sides by a copy of that lead's first
    unflipped point, so that every lead keeps its 4 096 points; the un-replaced terms are printed and bounded too."""
    from oracle.fill import unit_normalish, unit_uniform
    B, n = 8, 4096
    tol = TOL['bf16x2']
    m = _model('bf16x2')
    dev = _dev()
    # Eight DISTINCT field samples (the closed-form field with a 25 % closed-form perturbation of its 155 forecast rows) at lead times 0, 12, ..., 84 h.
    # Why not longer leads / unrelated fields: with the closed-form weights the density net's output then reaches the rho >= 1e-6 clip bound at a few of
    # the 4 096 points, p_x / rho = 1e6 p_x makes those points the whole gradient (|g| 1e9 against 1e2), and what is compared is the Jacobian's 2e-4 at
    # three points, not the lead batch (seen: lead 144 h, every rho_net gradient off by the same 1.8e-3).  Here min rho >= 0.07 on every lead while q, p
    # still sit on their clip bounds at 8 ... 330 points per lead.
    base_field = synthetic_inputs(8, tag='inter')['field_data']
    leads = []
    for k in range(B):
        b = synthetic_inputs(n, tag='lead%d' % k, forecast_h=12.0 * k / 360.0)
        pert = torch.from_numpy(unit_normalish('field_pert_lead%d' % k, 159 * 2405).reshape(1, 159, 2405).copy())
        field = base_field.clone()
        field[:, :155] = (field[:, :155] + 0.25 * pert[:, :155]) / np.sqrt(1.0 + 0.25 ** 2)
        b['field_data'] = field
        leads.append(b)

    def stack(bs):
        lead = {k_: torch.stack([b_[k_].reshape(-1) for b_ in bs]).to(dev) for k_ in ('x', 'y', 't', 'f')}
        return lead, torch.stack([b_['coord_data'] for b_ in bs]).to(dev), torch.cat([b_['field_data'] for b_ in bs], 0).to(dev), \
            torch.cat([b_['forecast_h'] for b_ in bs], 0).to(dev)
    lf = m.train_cfg['losses']['loss_factor']
    # (1) all points, nothing replaced: printed and bounded (5e-3; the six-size oracle tests of this file measure <= 2e-3 on better-conditioned batches)
    lead, cd, field, fh = stack(leads)
    with torch.no_grad():
        _, terms_all = m.place_lead_batch(lead['x'], lead['y'], lead['t'], lead['f'], field, cd, fh, torch.nn.MSELoss(), lf)
    terms_all = terms_all.double().cpu().numpy()
    clean, n_flipped = [], []
    for k, b in enumerate(leads):
        ref_all = _oracle(b, want_grads=False)['parts']
        raw = np.abs(terms_all[k] - ref_all) / np.abs(ref_all)
        flipped, _ = _flipped_points(m, b)
        idx = torch.nonzero(flipped).flatten().tolist()
        n_flipped.append(len(idx))
        print('lead %d (%3d h): all points: six terms off by %s; %d flipped points %s' % (k, 12 * k, ' '.join('%.1e' % v for v in raw), len(idx), idx[:12]))
        assert np.all(raw <= 5e-3), (k, raw)       # nothing removed: bounded (measured 3.5e-3 on one term of one lead: min rho 0.09 there, a flipped point's p_x / rho weighs more)
        assert len(idx) <= max(3, n // 100), (k, len(idx))
        if idx:
            src = int(torch.nonzero(~flipped).flatten()[0])
            c = {k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in b.items()}
            for k_ in ('x', 'y', 't', 'f', 'coord_data', 'labels'):
                c[k_][idx] = c[k_][src].clone()
            b = c
        clean.append(b)
    # (2) the north-star bars on the batch whose flipped points are replaced
    lead, cd, field, fh = stack(clean)
    m.physics_net.zero_grad(set_to_none=True)
    loss, terms = m.place_lead_batch(lead['x'], lead['y'], lead['t'], lead['f'], field, cd, fh, torch.nn.MSELoss(), lf)
    loss.backward()
    terms = terms.detach().double().cpu().numpy()
    # losses: against the fp32 oracle (the north-star bar is stated against the reference's fp32 run).  Gradients: every ELEMENT within 1e-3 of its tensor's
    # maximum of the FP64 oracle's gradient -- a sum over 8 x 4 096 points and 256 channels with cancellation is where the fp32 oracle's own rounding shows
    # (its distance from the fp64 one is printed beside ours for the worst tensors; no allowance is derived from it)
    def oracle64_grads(b):
        st = {k_: v.detach().cpu().to(torch.float64 if v.is_floating_point() else v.dtype).clone().requires_grad_(v.is_floating_point() and not k_.endswith('.pe'))
              for k_, v in m.physics_net.state_dict().items()}
        x, y, t = (b[k_].double().clone().requires_grad_(True) for k_ in ('x', 'y', 't'))
        total = O.place_one_batch(st, x, y, t, b['f'].double(), b['field_data'].double(), b['coord_data'].double(), b['forecast_h'].double(), GEO)
        names = O.param_names(st)
        return dict(zip(names, torch.autograd.grad(total, [st[k_] for k_ in names])))
    tot_ref, g32, g64 = 0.0, None, None
    for k, b in enumerate(clean):
        ref = _oracle(b)
        rel = np.abs(terms[k] - ref['parts']) / np.abs(ref['parts'])
        assert np.all(rel <= tol['loss']), (k, rel, terms[k], ref['parts'])
        tot_ref += ref['total'] / B
        g32 = ref['grads'] if g32 is None else {k_: g32[k_] + v for k_, v in ref['grads'].items()}
        r64 = oracle64_grads(b)
        g64 = r64 if g64 is None else {k_: g64[k_] + v for k_, v in r64.items()}
    assert abs(float(loss) - tot_ref) <= tol['loss'] * abs(tot_ref), (float(loss), tot_ref)
    rows = []
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        r = g64[name] / B
        err = float((p.grad.cpu().double() - r).abs().max() / (r.abs().max() + 1e-300))
        o32 = float((g32[name].double() / B - r).abs().max() / (r.abs().max() + 1e-300))
        rows.append((err, o32, name))
    rows.sort(reverse=True)
    for err, o32, name in rows[:5]:
        print('%-58s HIP vs fp64 oracle: %.2e of the tensor maximum | fp32 oracle vs fp64 oracle: %.2e' % (name, err, o32))
    print('8 leads x 4096 points: %s flipped points per lead replaced' % (n_flipped,))
    for err, o32, name in rows:
        assert err < tol['grad'], (name, err, o32)


# ------------------------------------------------------------------------------------------------ kink-aware parity, as a proof
def _oracle_masks(inp, st=None, gain=1.0, with_clip=True):
    """ReLU masks [6, N, 256] x 2, clip mask [N, 6] and the vapour switch delta [N] of the fp32 oracle arithmetic (oracle/kernel_model.py)."""
    from oracle import kernel_model as KM
    st = O.make_state(gain=gain) if st is None else st
    with torch.no_grad():
        meta = O.meta_net_forward(st, inp['field_data'], inp['forecast_h'])
        xi = torch.cat([inp['x'] / GEO.dx / (GEO.lon - 1), inp['y'] / GEO.dy / (GEO.lat - 1), inp['t'] / GEO.pred_t_span], 1)
        pe, dpe = KM.pe_and_tangent(xi)
        pe6 = O.sine_cos_pe(inp['coord_data'], 16)
        m1, m2, outs, jx = [], [], [], []
        for k, net in enumerate(O.NETS):
            W = KM.net_weights(st, net, meta, inp['forecast_h'])
            out, jxi, S = KM.phase_a(W, pe, dpe, pe6, inp['coord_data'][:, k], 'fp32')
            m1.append(S['m1'] > 0), m2.append(S['m2'] > 0), outs.append(out), jx.append(jxi)
        out_n = torch.stack(outs, 1)
        scale = torch.tensor([1.0 / GEO.dx / (GEO.lon - 1), 1.0 / GEO.dy / (GEO.lat - 1), 1.0 / GEO.pred_t_span])
        clip, delta = _clip_and_delta(out_n, torch.stack(jx, 1) * scale, with_clip)
    return torch.stack(m1), torch.stack(m2), clip, delta


def _flipped_points(m, inp, st=None, gain=1.0, with_clip=True):
    """Points of the batch at which ANY switch of the computation -- one of the 6 x 512 ReLU bits the forward kernel saves, a clip mask of
    inverse_norm, the condensation switch of the vapour equation -- differs between the HIP arithmetic and the fp32 oracle arithmetic.
    Two fp32-class arithmetics agree to ~1e-6 except where a pre-activation / bound / switch argument sits within rounding distance of
    its threshold; those points are IDENTIFIED here (bool [N]) instead of being covered by a blanket tolerance."""
    import deepphysinet_amd as dpn
    from deepphysinet_amd.point_path import relu_masks
    g = _gpu(inp)
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        m1, m2 = relu_masks(cfg, g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
        out_n, jac_n = dpn.pde_fields_and_jacobian(cfg, g['x'], g['y'], g['t'], g['coord_data'], heads, evec, statics)
    clip, delta = _clip_and_delta(out_n, jac_n, with_clip)
    o1, o2, oclip, odelta = _oracle_masks(inp, st=st, gain=gain, with_clip=with_clip)
    flip_relu = ((m1.cpu() != o1) | (m2.cpu() != o2)).any(dim=2).any(dim=0)
    return flip_relu | (clip != oclip).any(dim=1) | (delta != odelta), (m1, m2)


def _without(inp, flipped):
    n = flipped.shape[0]
    keep = ~flipped
    return {k: (v[keep] if (torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == n and k not in ('field_data', 'forecast_h')) else v) for k, v in inp.items()}


def _terms_vs_oracle_flip_free(m, inp, st=None, gain=1.0, with_clip=True, max_flipped=None):
    """The six loss terms of the HIP path and of the oracle on the batch WITHOUT its flipped points (named in the output): returns
    (hip terms, oracle terms, indices of the removed points).  With no flipped point this is the plain full-batch comparison."""
    flipped, _ = _flipped_points(m, inp, st=st, gain=gain, with_clip=with_clip)
    idx = torch.nonzero(flipped).flatten().tolist()
    n = flipped.shape[0]
    assert len(idx) <= (max(3, n // 150) if max_flipped is None else max_flipped), idx        # measured: 32 of 5 197 points (0.62 %), 3 of 200
    sub = _without(inp, flipped) if idx else inp
    gs = _gpu(sub)
    terms = m.pde_loss_terms(gs['x'], gs['y'], gs['t'], gs['f'], gs['field_data'], gs['coord_data'], gs['forecast_h']).detach().double().cpu().numpy()
    if st is None:
        ref = _oracle(sub, gain=gain, with_clip=with_clip, want_grads=False)['parts']
    else:
        x, y, t = (sub[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
        _, parts, _, _ = O.place_one_batch(st, x, y, t, sub['f'], sub['field_data'], sub['coord_data'], sub['forecast_h'], GEO, with_clip=with_clip,
                                           return_parts=True)
        ref = np.array([float(p.detach()) for p in parts])
    return terms, ref, idx


def _clip_and_delta(out_n, jac_n, with_clip=True):
    """Which points sit inside the clip bounds (P, T, q, rho) and have the vapour switch on (interface_physics.py:165-168), from
    normalised fields [N, 6] and their Jacobian [N, 6, 3]."""
    std, mean = torch.tensor(O.OBS_STD), torch.tensor(O.OBS_MEAN)
    val = out_n.cpu() * std + mean
    clip = torch.ones_like(val, dtype=torch.bool)
    for k in range(2, 6 if with_clip else 2):
        clip[:, k] = (val[:, k] >= O.CLIP_LO[k]) & (val[:, k] <= O.CLIP_HI[k])
        val[:, k] = val[:, k].clamp(O.CLIP_LO[k], O.CLIP_HI[k])
    J = jac_n.cpu() * (std * clip)[:, :, None]
    u, v, p, T, q = val[:, 0], val[:, 1], val[:, 2], val[:, 3], val[:, 4]
    omega = J[:, 2, 2] + u * J[:, 2, 0] + v * J[:, 2, 1]
    tc = T - 273.15
    e_s = 6.112 * torch.exp(17.67 * tc / (tc + 243.5)) * 100
    q_s = torch.clamp(0.622 * e_s / (p - 0.378 * e_s), min=1e-6)
    return clip, (omega < 0) & (q >= q_s)


def _assert_tight_after_removing_flips(n):
    """The parity statement of the hi+lo mode for a batch of n points: the points where a switch bit differs from the oracle arithmetic's
    are listed and bounded in number (<= 1 % of the points, at least 3; measured 0.6 %: 32 of 5 197, each point carries 6 x 512 ReLU
    bits); with them removed from BOTH sides every loss term is within 1e-4, every Jacobian row within 2e-4 of the field's largest entry,
    every field value within 5e-5 and every gradient ELEMENT within 1e-3 of its tensor's maximum -- no outlier allowance, no L2 fallback."""
    import deepphysinet_amd as dpn
    tol = TOL['bf16x2']
    inp = synthetic_inputs(n, tag='inter')
    m = _model('bf16x2')
    flipped, (m1, m2) = _flipped_points(m, inp)
    nf = int(flipped.sum())
    print('n = %d: %d points carry a switch bit that differs from the oracle arithmetic: %s' % (n, nf, torch.nonzero(flipped).flatten().tolist()[:20]))
    assert nf <= max(3, n // 100), nf
    # the masks themselves: everything else identical, and the bit counts plausible (about half of the units are on)
    assert 0.2 < float(m1.float().mean()) < 0.8 and 0.2 < float(m2.float().mean()) < 0.8
    # The UN-REMOVED batch first: what the six losses of all n points differ by from the oracle's, printed and bounded.  A flipped switch
    # moves its point's residual by O(1) of that point's term, i.e. a mean over n points by up to ~1 / n of the term's spread: 2e-3 at the ~1 k
    # points where it is largest (the reference's own fp32 run against its fp64 run moves the same terms by as much).
    if nf:
        ref_all = _oracle(inp, want_grads=False)
        g_all = _gpu(inp)
        with torch.no_grad():
            t_all = m.pde_loss_terms(g_all['x'], g_all['y'], g_all['t'], g_all['f'], g_all['field_data'], g_all['coord_data'], g_all['forecast_h']).cpu().numpy()
        raw = np.abs(t_all - ref_all['parts']) / np.abs(ref_all['parts'])
        print('n = %d, all points (nothing removed): six loss terms off by %s (bound 2e-3)' % (n, ' '.join('%.1e' % v for v in raw)))
        assert np.all(raw <= 2e-3), raw
    sub = _without(inp, flipped) if nf else inp
    ref = _oracle(sub)
    gs = _gpu(sub)
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(gs['field_data'], gs['forecast_h'])
        out_k, jac_k = dpn.pde_fields_and_jacobian(cfg, gs['x'], gs['y'], gs['t'], gs['coord_data'], heads, evec, statics)
    assert float((out_k.cpu() - ref['fields']).abs().max() / ref['fields'].abs().max()) < tol['field']
    for k in range(6):
        r = ref['jac_n'][:, k]
        assert float((jac_k.cpu()[:, k] - r).abs().max()) < tol['jac'] * float(r.abs().max()), k
    m.physics_net.zero_grad(set_to_none=True)
    terms = m.pde_loss_terms(gs['x'], gs['y'], gs['t'], gs['f'], gs['field_data'], gs['coord_data'], gs['forecast_h'])
    terms.sum().backward()
    mine = terms.detach().cpu().numpy()
    assert np.all(np.abs(mine - ref['parts']) <= tol['loss'] * np.abs(ref['parts'])), (mine, ref['parts'])
    worst = 0.0
    for name, p in m.physics_net.named_parameters():
        if name.endswith('key_projection.bias'):
            continue
        r = ref['grads'][name]
        err = float((p.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-30))
        worst = max(worst, err)
        assert err < tol['grad'], (name, err)
    print('after removing them: worst gradient element %.2e of its tensor maximum' % worst)


@pytest.mark.parametrize('n', [5197, 1037])
def test_kink_flips_are_listed_and_every_other_point_is_tight(n):
    """tolerances that allow 'isolated outliers because of ReLU kinks' must identify them.  See
    _assert_tight_after_removing_flips; test_fields_jacobian_losses_gradients_vs_oracle runs the same statement for its other sizes."""
    _assert_tight_after_removing_flips(n)


def test_variable_net_standalone_forward_matches_oracle():
    """VariableNet.forward with the reference's own signature (model/variable_net.py:49: meta_out, coord [N,192] encoded, coord_data,
    ref_data [N,1], fore_h) on one net at a time -- the surface a caller holding a single VariableNet uses -- against the oracle's
    restatement of the same lines, values and the gradient of a weight."""
    n = 300
    inp = synthetic_inputs(n, tag='inter')
    m = _model('bf16x2')
    g = _gpu(inp)
    st = O.make_state()
    with torch.no_grad():
        meta_ref = O.meta_net_forward(st, inp['field_data'], inp['forecast_h'])
        coord_ref = O.encoding_coord(inp['x'], inp['y'], inp['t'], GEO)
    meta = m.physics_net.meta_net(g['field_data'], g['forecast_h'])
    coord = m.encoding_coord(g['x'], g['y'], g['t'], m.pred_t_span)
    for k, name in ((0, 'U_net'), (4, 'q_net')):
        net = getattr(m.physics_net, name)
        ref_data = g['coord_data'][:, k:k + 1] * 0.5 + 0.25                  # NOT the column the fused path would add
        out = net(meta, coord, g['coord_data'], ref_data, g['forecast_h'])
        with torch.no_grad():
            want = O.variable_net_forward(st, name, meta_ref, coord_ref, inp['coord_data'], ref_data.cpu(), inp['forecast_h'])
        assert out.shape == (n, 1)
        assert float((out.detach().cpu() - want).abs().max() / want.abs().max()) < TOL['bf16x2']['field'], name
        with torch.no_grad():                                                   # inference: the one-net launch (dpn_fwd_ref_nets), same values
            out1 = net(meta.detach(), coord, g['coord_data'], ref_data, g['forecast_h'])
        assert torch.equal(out1, out.detach()), name
    net.zero_grad(set_to_none=True)
    out.sum().backward()
    assert net.out_fc.weight.grad is not None and bool(torch.isfinite(net.out_fc.weight.grad).all())


def test_fp8_gemm_experiment_kernel_matches_its_definition():
    """A SHELVED experiment kernel (csrc/dpn_fp8.hip, compiled only into the experiment library, include/dpn_hip_experiments.h): the non-scaled
    fp8 GEMM, C = s_a s_w q(A / s_a) q(W / s_w)^T + bias with one scale per row and OCP e4m3 operands -- against the same definition written
    with torch's float8_e4m3fn casts; and its distance from the exact product (a few percent).  The product library does not export it."""
    import ctypes
    from deepphysinet_amd import _lib as L
    assert not hasattr(L.load(), 'dpn_gemm_fp8')
    from deepphysinet_amd.build import build_experiments
    build_experiments()
    lib = L.load_experiments()
    dev = _dev()
    torch.manual_seed(0)
    for M, N, K, epi in ((287, 256, 256, 0), (1000, 256, 256, 1), (64, 96, 32, 0)):
        A = torch.randn(M, K, device=dev) * 1.7
        W = torch.randn(N, K, device=dev) / K ** 0.5
        bias = torch.randn(N, device=dev) * 0.1
        C = torch.empty(M, N, device=dev)
        pre = torch.empty(M, N, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lib.dpn_gemm_fp8(M, N, K, p(A), K, p(W), K, p(bias), p(C), N, epi, p(pre) if epi else None, torch.cuda.current_stream().cuda_stream) == 0
        sa = A.abs().amax(dim=1, keepdim=True).clamp_min(1e-30) * (1.0 / 448.0)
        sw = W.abs().amax(dim=1, keepdim=True).clamp_min(1e-30) * (1.0 / 448.0)
        qa = (A * (1.0 / sa)).to(torch.float8_e4m3fn).float()
        qw = (W * (1.0 / sw)).to(torch.float8_e4m3fn).float()
        want = (qa @ qw.t()) * sa * sw.t() + bias
        exact = A @ W.t() + bias
        if epi:
            assert float((pre - want).abs().max() / want.abs().max()) < 2e-3
            want, exact = torch.nn.functional.gelu(want), torch.nn.functional.gelu(exact)
        assert float((C - want).abs().max() / want.abs().max()) < 2e-3, (M, N, K)          # same quantised operands, other summation order / rounding ties
        err = float((C - exact).abs().max() / exact.abs().max())
        assert 1e-3 < err < 0.2, err                                                       # the fp8 operand rounding itself: percent level



def test_fp8_mx_gemm_kernel_matches_the_mx_definition():
    """The block-scaled form (v_mfma_scale_f32_32x32x64_f8f6f4, csrc/dpn_fp8.hip dpn_gemm_fp8_mx): one power-of-two scale per 32 consecutive
    k of a row (OCP MX: E8M0), e4m3 elements -- against the same definition written with torch casts.  Pins the instruction's operand
    layout (which k a lane's 32 bytes are, whose scale applies to them) with unequal block magnitudes along K."""
    import ctypes
    from deepphysinet_amd import _lib as L
    lib = L.load()
    dev = _dev()
    torch.manual_seed(0)

    def mx(t):                                               # [R, K] -> dequantised MX image
        R, K = t.shape
        b = t.view(R, K // 32, 32)
        amax = b.abs().amax(dim=2, keepdim=True)
        e = torch.ceil(torch.log2(amax.clamp_min(1e-38) / 448.0))
        scale = torch.where(amax > 0, torch.exp2(e), torch.ones_like(e))
        return ((b / scale).to(torch.float8_e4m3fn).float() * scale).view(R, K)

    for M, N, K, epi in ((287, 256, 256, 0), (1000, 256, 256, 1), (64, 96, 64, 0)):
        ramp = torch.exp2(torch.arange(K // 32, device=dev, dtype=torch.float32) * 1.5 - 3.0).repeat_interleave(32)   # blocks 2^-3 .. 2^7.5
        A = torch.randn(M, K, device=dev) * 1.7 * ramp
        W = torch.randn(N, K, device=dev) / K ** 0.5 * ramp.flip(0)
        bias = torch.randn(N, device=dev) * 0.1
        C = torch.empty(M, N, device=dev)
        pre = torch.empty(M, N, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lib.dpn_gemm_fp8_mx(M, N, K, p(A), K, p(W), K, p(bias), p(C), N, epi, p(pre) if epi else None, torch.cuda.current_stream().cuda_stream) == 0
        want = (mx(A).double() @ mx(W).double().t()).float() + bias
        exact = A @ W.t() + bias
        if epi:
            assert float((pre - want).abs().max() / want.abs().max()) < 1e-4
            want, exact = torch.nn.functional.gelu(want), torch.nn.functional.gelu(exact)
        # same operands and scales; the instruction's 64-term sum is not an fp32 fmaf chain (measured 3e-5 of the largest entry against the
        # fp64 sum of the same quantised operands) -- a wrong block / scale assignment shows up at 1e-1 (it did: 0.75 before the layout probe)
        assert float((C - want).abs().max() / want.abs().max()) < 1e-4, (M, N, K)
        err = float((C - exact).abs().max() / exact.abs().max())
        assert 1e-3 < err < 0.2, err                                                       # the e4m3 rounding itself

def test_config4_fp8_encoder_workload():
    """BASELINE configs[4] as a CONFIGURATION (bench.py --encoder-fp8): the encoder layers' forward GEMMs on fp8 (OCP e4m3) MFMA, everything
    behind them -- hyper-network heads, fused forward + Jacobian in bf16x2, residuals -- as in the product, on the configs[1] workload
    (0.25-degree grid nodes).  The six PDE losses are held to the ORACLE at the tolerance this precision buys, 0.5 relative (measured
    2e-2 ... 4e-1 on this sample, 1.4e-2 ... 1.8e-1 on the full grid: the hyper-network turns the encoder output into the point MLPs' weights), and must be strictly worse than the
    product's 1e-4 -- the test pins both that the configuration runs end to end and what it costs."""
    import os
    from bench import synth_batch
    n = 4096                                                        # grid nodes of the configs[1] workload the oracle finishes in seconds
    inp = {k: v.cpu() for k, v in synth_batch(n, 'cpu', seed=1).items()}
    ref = _oracle(inp, want_grads=False)
    m = _model('bf16x2')
    g = _gpu(inp)
    got = {}
    from deepphysinet_amd import config
    for fp8 in ('0', '1'):
        with config.override(encoder_fp8='mx' if fp8 == '1' else ''), torch.no_grad():      # configs[4] = the block-scaled (MX) fp8 form
            got[fp8] = m.pde_loss_terms(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h']).double().cpu().numpy()
    err_prod = np.abs(got['0'] - ref['parts']) / np.abs(ref['parts'])
    err_fp8 = np.abs(got['1'] - ref['parts']) / np.abs(ref['parts'])
    assert np.all(np.isfinite(got['1']))
    if err_prod.max() > 1e-4:                                        # the product path on the same inputs: 1e-4 once the points whose switches differ
        mine, ref_ff, idx = _terms_vs_oracle_flip_free(m, inp)       # from the oracle arithmetic's are named and removed (like every other test)
        print('config4 sample: removed points %s' % idx)
        assert idx and np.all(np.abs(mine - ref_ff) <= 1e-4 * np.abs(ref_ff)), (idx, mine, ref_ff)
    # configs[4]'s stated tolerance is what fp8 operands in the encoder buy: the hyper-network turns the encoder's output into the point MLPs' weights,
    # so a 3 % output error moves the six losses by 13 ... 55 % on this sample in the block-scaled (MX) form (the shelved non-scaled form: 2 ... 40 %)
    print('configs[4], MX fp8 encoder GEMMs: six PDE losses off by %s' % ' '.join('%.2f' % v for v in err_fp8))
    assert err_fp8.max() <= 0.8, err_fp8
    assert err_fp8.max() > 10 * err_prod.max(), (err_fp8, err_prod)  # ... and it is a real precision loss, not noise


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
@pytest.mark.parametrize('n', [1037, 70])
def test_tile_split_kernels_against_the_ring_kernels(n, prec):
    """The point kernels exist in two decompositions: the ring form (one 512-register wave per SIMD owns 32 points and all output tiles, weights
    shared through an LDS-DMA ring; plain bf16 and caller-encoded coordinates) and the tile-split form (the hi+lo mode's default: output tiles
    split over the waves, activations shared through LDS, weights L2 -> VGPR, two workgroups per CU; csrc/dpn_fwd_tiles.h).
    BACKWARD stage 1: same products in the same order per output tile -- the operands Z1, Z0, G6, gnet agree BIT FOR BIT.
    FORWARD: since round 5 the tile-split kernel runs the FUSED algebra (A = W1 w2, B = W1 Wd formed once per net: five GEMMs per point and net,
    csrc/dpn_layout.h) and the ring kernel the seven GEMMs of variable_net.py:49-87 as they stand -- the same function in two arithmetics, so
    fields, Jacobian and saved state agree to operand rounding, and the ReLU bits except at pre-activations within rounding distance of zero.
    Ragged sizes: 1037 = 16 full 64-point workgroups + 13 points, 70 = one full + 6 points."""
    import ctypes
    from deepphysinet_amd import _lib as L, point_path as PP
    inp = synthetic_inputs(n, tag='inter')
    m = _model(prec)                                          # plain bf16 defaults to the ring kernels; its tile-split instantiation is pinned here too
    g = _gpu(inp)
    cfg = m.point_config()
    lib = L.load()
    dev = _dev()
    old = {k: os.environ.get(k) for k in ('DPN_FWD_KERNEL', 'DPN_BWD_KERNEL')}
    try:
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
            x_, y_, t_, f_ = (PP._f32c(g[k]).reshape(-1) for k in ('x', 'y', 't', 'f'))
            cd_ = PP._f32c(g['coord_data'])
            st = [PP._f32c(s_) for s_ in statics]
            ws = PP._Workspace(n, cfg.prec, dev)
            nets = PP._net_ptrs(PP._f32c(heads), PP._f32c(evec), st)
            s = PP._stream()
            geo, ph, fr = cfg.geometry(), cfg.physics(), PP._freqs(dev)
            res = {}
            for kind in ('ring', 'tiles'):
                os.environ['DPN_FWD_KERNEL'] = os.environ['DPN_BWD_KERNEL'] = kind
                form = lib.dpn_fwd_form(cfg.prec, 0)
                assert form == (1 if kind == 'tiles' else 0)
                L.check(lib.dpn_pack_weights_form(nets, cfg.prec, form, PP._ptr(ws.packed), s), 'pack')
                out_n = torch.zeros((n, 6), device=dev); jac_n = torch.zeros((n, 6, 3), device=dev)
                saved = torch.zeros(ws.sizes.saved, dtype=torch.uint8, device=dev)
                L.check(lib.dpn_fwd(PP._ptr(x_), PP._ptr(y_), PP._ptr(t_), None, PP._ptr(cd_), n, PP._ptr(fr), ctypes.byref(geo), PP._ptr(ws.packed),
                                    cfg.prec, PP._ptr(out_n), PP._ptr(jac_n), PP._ptr(saved), s), 'fwd')
                g_out = torch.empty((n, 6), device=dev); g_jxi = torch.empty((n, 6, 3), device=dev)
                L.check(lib.dpn_residual(PP._ptr(out_n), PP._ptr(jac_n), PP._ptr(f_), n, ctypes.byref(geo), ctypes.byref(ph), None, None, None,
                                         PP._ptr(g_out), PP._ptr(g_jxi), s), 'res')
                operands = torch.zeros(ws.sizes.operands, dtype=torch.uint8, device=dev)
                # the backward kernels of BOTH forms read the ring forward's cotangents and saved state, so that only the kernel under test differs
                # (they read w1 and the b1 vector: at the same place in either packed form)
                if kind == 'ring':
                    go, gj, sv = g_out.clone(), g_jxi.clone(), saved.clone()
                L.check(lib.dpn_bwd_points(PP._ptr(x_), PP._ptr(y_), PP._ptr(t_), None, PP._ptr(cd_), n, PP._ptr(fr), ctypes.byref(geo), PP._ptr(ws.packed),
                                           cfg.prec, PP._ptr(go), PP._ptr(gj), PP._ptr(sv), PP._ptr(operands), s), 'bwd')
                torch.cuda.synchronize()
                res[kind] = (out_n, jac_n, saved, operands)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    (o0, j0, s0, p0), (o1, j1, s1, p1) = res['ring'], res['tiles']
    assert torch.equal(p0, p1)                                                  # backward stage 1: bit for bit
    n_pad, ns = int(ws.sizes.n_pad), int(cfg.prec)
    # forward: two arithmetics of one function
    tol_f, tol_j = (2e-5, 5e-4) if prec == 'bf16x2' else (3e-2, 0.35)
    assert float((o0 - o1).abs().max()) <= tol_f * float(o0.abs().max())
    dj = (j0 - j1).abs() / j0.abs().amax(dim=(0, 2), keepdim=True)
    off = int((dj.amax(dim=(1, 2)) > tol_j).sum())                              # points whose Jacobian differs: those with a flipped ReLU bit
    if prec == 'bf16x2':
        t1_bytes, m2_bytes = 6 * ns * n_pad * 512, 6 * n_pad * 512
        m2a, m2b = s0[t1_bytes:t1_bytes + m2_bytes], s1[t1_bytes:t1_bytes + m2_bytes]
        m1a, m1b = s0[t1_bytes + m2_bytes:t1_bytes + m2_bytes + 6 * n_pad * 32], s1[t1_bytes + m2_bytes:t1_bytes + m2_bytes + 6 * n_pad * 32]
        flipped2 = int((m2a.view(torch.int16) != m2b.view(torch.int16)).sum())
        flipped1 = int(((m1a.view(torch.int32) ^ m1b.view(torch.int32)) != 0).sum())
        print('ring vs tile-split forward (n = %d): %d differing relu-2 mask entries of %d, %d differing relu-1 words, %d points with a Jacobian row off by > %g'
              % (n, flipped2, 6 * n * 256, flipped1, off, tol_j))
        assert flipped2 <= max(4, 6 * n * 256 // 20000) and flipped1 <= max(4, n // 100)
        assert off <= max(3, n // 100)
    else:
        assert off <= n // 4


def test_encoder_guards_of_the_fused_path():
    """(1) a weight outside the f16 hi+lo split's range (|w| >= 32768) raises at the next check_enc_status() -- which the training loop
    and bench.py call where they synchronise anyway -- instead of surfacing later as inf / NaN; (2) a model whose parameters are not fp32 on the
    input's device never reaches the fused kernels (they read raw pointers as fp32): the fit checks send it to the per-op path, which rejects it;
    (3) a second consumer of the data embedding's output (the cut of the staged backward) gets correct gradients: the weight gradients the stack
    node computed from ITS d x0 are used only when that is the cotangent that arrives."""
    from deepphysinet_amd import encoder_ops as EO
    dev = _dev()
    m = _model('bf16x2')
    g = _gpu(synthetic_inputs(64, GEO.lon, GEO.lat, GEO.dx, GEO.dy))
    net = m.physics_net
    # (1)
    EO.check_enc_status()
    w = net.meta_net.model.encoder.attn_layers[0].conv1.weight
    keep = w.detach().clone()
    with torch.no_grad():
        w[3, 5, 0] = 1.0e5
    with torch.no_grad():
        net.encode_field(g['field_data'], g['forecast_h'])
    with pytest.raises(RuntimeError, match='32768'):
        EO.check_enc_status()
    with torch.no_grad():
        w.copy_(keep)
        EO.enc_status(dev).zero_()
    EO.check_enc_status()
    # (2)
    tn = net.meta_net.model
    layers = list(tn.encoder.attn_layers)
    assert EO._stack_fits(layers, tn.encoder.norm, tn.projection, dev)
    p = layers[1].conv2.bias
    old = p.data
    p.data = old.double()
    try:
        assert not EO._stack_fits(layers, tn.encoder.norm, tn.projection, dev)
        assert EO.encoder_forward_fused(tn, g['field_data'], g['forecast_h']) is None
    finally:
        p.data = old
    # (3) loss = sum(meta_out * c) + sum(x0 * d): x0 has two consumers, so the embedding node receives d x0 (stack) + d
    net.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    meta = net.encode_field(g['field_data'], g['forecast_h'], keep_embedding=True)
    x0 = tn.last_embedding
    object.__setattr__(tn, 'last_embedding', None)
    c, d = torch.randn_like(meta), torch.randn_like(x0)
    ((meta * c).sum() + (x0 * d).sum()).backward()
    got = {k: v.grad.detach().clone() for k, v in (('w', tn.enc_embedding.value_embedding.tokenConv.weight), ('b', tn.enc_embedding.value_embedding.tokenConv.bias),
                                                      ('tok', tn.learnable_token))}
    # the same by linearity: two backward passes with a single consumer each
    want = {}
    for only_meta in (True, False):
        net.zero_grad(set_to_none=True)
        meta = net.encode_field(g['field_data'], g['forecast_h'], keep_embedding=True)
        x0 = tn.last_embedding
        object.__setattr__(tn, 'last_embedding', None)
        ((meta * c).sum() if only_meta else (x0 * d).sum()).backward()
        for k, v in (('w', tn.enc_embedding.value_embedding.tokenConv.weight), ('b', tn.enc_embedding.value_embedding.tokenConv.bias), ('tok', tn.learnable_token)):
            want[k] = want.get(k, 0) + (v.grad.detach().clone() if v.grad is not None else 0)
    for k in got:
        err = float((got[k] - want[k]).abs().max() / want[k].abs().max())
        assert err < 2e-5, (k, err)
    # (4) ADVICE r5: an IN-PLACE tensor hook on x0 keeps the cotangent's pointer and changes its values: the node must notice (version counter) and
    # compute the gradients from what arrives -- here exactly twice the single-consumer ones
    single = {}
    for hooked in (False, True):
        net.zero_grad(set_to_none=True)
        meta = net.encode_field(g['field_data'], g['forecast_h'], keep_embedding=True)
        x0 = tn.last_embedding
        object.__setattr__(tn, 'last_embedding', None)
        if hooked:
            x0.register_hook(lambda gr: gr.mul_(2.0))
        (meta * c).sum().backward()
        for k, v in (('w', tn.enc_embedding.value_embedding.tokenConv.weight), ('b', tn.enc_embedding.value_embedding.tokenConv.bias), ('tok', tn.learnable_token)):
            if hooked:
                err = float((v.grad - 2.0 * single[k]).abs().max() / single[k].abs().max())
                assert err < 2e-5, ('in-place hook', k, err)
            else:
                single[k] = v.grad.detach().clone()
