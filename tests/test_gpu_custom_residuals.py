"""GPU (MI355X): user-written residuals train on the HIP point kernels -- InterfacePhysics.fields_at / point_path.point_fields_xyt.

The fields come back attached to x, y, t: the reference's own `*_equation` composition (gradient() = autograd.grad(create_graph=True)) and
residuals with second derivatives evaluate on them and train.  Checked against the CPU oracle (oracle/dpn_oracle.py, autograd through the
reference's formulas, double-backward included), against place_one_batch on the same batch (the same point kernels), and bit for bit against
the fused step's entry points where the derivative outputs are off.  Points whose ReLU / clip / vapour switch differs from the oracle
arithmetic's are removed first, as everywhere in tests/test_gpu_parity.py (whose helpers are reused)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from oracle.fill import synthetic_inputs
from tests.test_gpu_parity import GEO, TOL, _flipped_points, _gpu, _model, _without

GRAD_L2, GRAD_MAX = 1e-3, 2e-3          # the suite's gradient bars against the fp64 oracle (test_full_grid_all_gradients_vs_oracle)
SAME_KERNELS_L2 = 1e-4                  # fields_at + autograd vs place_one_batch: both through the same point kernels


def _clean_batch(m, n, tag='inter'):
    inp = synthetic_inputs(n, tag=tag)
    flipped, _ = _flipped_points(m, inp)
    idx = torch.nonzero(flipped).flatten().tolist()
    assert len(idx) <= max(3, n // 100), idx
    return _without(inp, flipped) if idx else inp


def _grad(v, w):
    return torch.autograd.grad(v, w, grad_outputs=torch.ones_like(v), create_graph=True, only_inputs=True, allow_unused=False)[0]


def _reference_losses(m, x, y, t, fields, f):
    """interface_physics.py:276-301 verbatim: inverse_norm, the six *_equation methods, their sum in the reference's order."""
    lf = m.train_cfg['losses']['loss_factor']
    crit = torch.nn.MSELoss()
    u, v, p, T, q, rio = m.inverse_norm(*fields, m.obs_norm_cfg)
    mu = m.montion_equation_u(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_u_factor'])
    mv = m.montion_equation_v(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_v_factor'])
    co = m.continuous_equation(x, y, t, u, v, rio, crit, factor=lf['continuous_factor'])
    en = m.energy_equation(x, y, t, u, v, p, T, rio, q, crit, factor=lf['energy_factor'])
    va = m.vapor_equation(x, y, t, u, v, p, T, q, crit, factor=lf['vapor_factor'])
    ga = m.gas_equation(p, T, rio, q, crit, factor=lf['gas_factor'])
    return (mu, mv, co, en, va, ga), mu + mv + en + co + va + ga


def _second_order_loss(fields, x, y, t, g=_grad):
    """A residual of one's own with second derivatives: u_xx + u_yy, T_xx + T_yy, u_tt (normalised fields; derivatives scaled to the domain
    so that every term is O(1)), plus the advection of u."""
    Lx, Ly, Lt = GEO.dx * (GEO.lon - 1), GEO.dy * (GEO.lat - 1), GEO.pred_t_span
    u, v, T = fields[0], fields[1], fields[3]
    lap_u = g(g(u, x), x) * Lx * Lx + g(g(u, y), y) * Ly * Ly
    lap_T = g(g(T, x), x) * Lx * Lx + g(g(T, y), y) * Ly * Ly
    adv_u = g(u, t) * Lt + u * g(u, x) * Lx + v * g(u, y) * Ly
    u_tt = g(g(u, t), t) * Lt * Lt
    return torch.mean((adv_u - 1e-2 * lap_u) ** 2) + 1e-3 * torch.mean(lap_T ** 2) + 1e-3 * torch.mean(u_tt ** 2)


def _oracle64(m, b, loss_fn):
    """fp64 oracle: the loss, every parameter gradient and the coordinate gradients, double-backward through the reference's formulas."""
    st = {k: v.detach().cpu().to(torch.float64 if v.is_floating_point() else v.dtype).clone().requires_grad_(v.is_floating_point() and not k.endswith('.pe'))
          for k, v in m.physics_net.state_dict().items()}
    x, y, t = (b[k].double().clone().requires_grad_(True) for k in ('x', 'y', 't'))
    pe = O.encoding_coord(x, y, t, GEO)
    fields = O.physics_net_forward(st, b['field_data'].double(), pe, b['coord_data'].double(), b['forecast_h'].double())
    loss = loss_fn(fields, x, y, t)
    names = O.param_names(st)
    g = torch.autograd.grad(loss, [st[k] for k in names] + [x, y, t], retain_graph=True, allow_unused=True)    # (a residual of some fields only)
    g = [torch.zeros_like(w) if gw is None else gw for gw, w in zip(g, [st[k] for k in names] + [x, y, t])]
    return float(loss.detach()), dict(zip(names, g[:len(names)])), g[len(names):], (st, x, y, t, fields)


def _dist(a_, r):
    d = (a_.double() - r.double()).abs()
    return float(d.pow(2).mean().sqrt() / (r.double().pow(2).mean().sqrt() + 1e-300)), float(d.max() / (r.double().abs().max() + 1e-300))


def _param_grads(m):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone() for k, p in m.physics_net.named_parameters()
            if not k.endswith('key_projection.bias')}


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
@pytest.mark.parametrize('n', [256, 4096])
def test_reference_equation_composition_trains_on_fields_at(prec, n):
    """fields_at -> inverse_norm -> the six *_equation methods -> sum -> backward: the losses of the fp32 oracle, the gradients of place_one_batch
    on the same batch (same point kernels) and -- parity-grade mode -- of the fp64 oracle."""
    m = _model(prec)
    # parity-grade mode: the flipped points removed (tests/test_gpu_parity.py); plain bf16 flips many ReLU signs and is held to its own bars there
    b = _clean_batch(m, n) if prec == 'bf16x2' else synthetic_inputs(n, tag='inter')
    g = _gpu(b)
    lf = m.train_cfg['losses']['loss_factor']
    m.physics_net.zero_grad(set_to_none=True)
    fused = m.place_one_batch(g['x'], g['y'], g['t'], g['f'], g['field_data'], g['coord_data'], g['forecast_h'], torch.nn.MSELoss(), lf, 0, 0, g['x'].device)
    fused.backward()
    ref_fused = _param_grads(m)
    m.physics_net.zero_grad(set_to_none=True)
    x, y, t = (g[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    fields = m.fields_at(x, y, t, g['field_data'], g['coord_data'], g['forecast_h'])
    parts, total = _reference_losses(m, x, y, t, fields, g['f'])
    total.backward()
    mine = _param_grads(m)
    assert len(mine) == 151 and sum(1 for _ in m.physics_net.parameters()) == 155     # (less the four key_projection biases: zero gradient)
    # the six losses against the fp32 oracle
    st = O.make_state(requires_grad=True)
    xo, yo, to = (b[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    _, ref_parts, _, _ = O.place_one_batch(st, xo, yo, to, b['f'], b['field_data'], b['coord_data'], b['forecast_h'], GEO, return_parts=True)
    got = np.array([float(p_.detach()) for p_ in parts])
    ref = np.array([float(p_.detach()) for p_ in ref_parts])
    assert np.all(np.abs(got - ref) <= TOL[prec]['loss'] * np.abs(ref)), (got, ref)
    # every gradient against place_one_batch's (the fused residual kernel's cotangents vs autograd's: the same point kernels behind both)
    worst = max((_dist(mine[k], ref_fused[k])[0], k) for k in mine)
    print('n = %d %s: worst L2 distance fields_at vs place_one_batch gradients %.2e (%s)' % (n, prec, worst[0], worst[1]))
    assert worst[0] < SAME_KERNELS_L2, worst
    if prec != 'bf16x2':
        return
    def reference_total(fl, x_, y_, t_):
        mu, mv, co, en, va, ga = O.residual_losses(x_, y_, t_, b['f'].double(), *O.inverse_norm(fl))
        return mu + mv + en + co + va + ga
    _, g64, _, _ = _oracle64(m, b, reference_total)
    for k, v in mine.items():
        l2, mx = _dist(v, g64[k])
        assert l2 < GRAD_L2 and mx < GRAD_MAX, (k, l2, mx)


def test_second_derivatives_and_their_training_vs_the_fp64_oracle():
    """A residual with u_xx, u_yy, T_xx + T_yy and u_tt: its value, all 155 parameter gradients and x.grad, y.grad, t.grad (these read the third
    derivatives) against the fp64 oracle's double-backward; the kernel's second derivatives (all 6 x 3) against the oracle's; mixed partials zero."""
    n = 1024
    m = _model('bf16x2')
    b = _clean_batch(m, n, tag='second')
    g = _gpu(b)
    m.physics_net.zero_grad(set_to_none=True)
    x, y, t = (g[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    fields = m.fields_at(x, y, t, g['field_data'], g['coord_data'], g['forecast_h'])
    loss = _second_order_loss(fields, x, y, t)
    u_xy = _grad(_grad(fields[0], x), y)
    assert torch.equal(u_xy, torch.zeros_like(u_xy))                  # mixed partials: exactly zero, as autograd gives on the oracle
    loss.backward()
    mine = _param_grads(m)
    ref_loss, g64, gxyt, (st, xo, yo, to, fo) = _oracle64(m, b, _second_order_loss)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-4 * abs(ref_loss), (float(loss.detach()), ref_loss)
    rows = []
    for k, v in mine.items():
        l2, mx = _dist(v, g64[k])
        rows.append((l2, mx, k))
    rows.sort(reverse=True)
    print('second-order loss: worst gradient L2 %.2e (%s), worst element %.2e' % (rows[0][0], rows[0][2], max(r_[1] for r_ in rows)))
    for l2, mx, k in rows:
        assert l2 < GRAD_L2 and mx < GRAD_MAX, (k, l2, mx)
    for mine_c, ref_c, nm in zip((x.grad, y.grad, t.grad), gxyt, 'xyt'):
        l2, mx = _dist(mine_c.cpu(), ref_c)
        print('%s.grad: L2 %.2e, worst element %.2e' % (nm, l2, mx))
        assert l2 < GRAD_L2 and mx < GRAD_MAX, (nm, l2, mx)
    # the kernel's second derivatives, all 6 x 3, against the oracle's (physical units; bar: the Jacobian's)
    from deepphysinet_amd import point_path as P
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        ws = P._Workspace(n, cfg.prec, x.device)
        _, jac_n, hess_n, _ = P._forward_derivs(cfg, ws, P._net_ptrs(heads, evec, [s.detach() for s in statics]), g['x'].reshape(-1), g['y'].reshape(-1),
                                                g['t'].reshape(-1), g['coord_data'], want_saved=False)
    hess = hess_n.cpu().double()
    for k in range(6):
        for c, w in enumerate((xo, yo, to)):
            r = _grad(_grad(fo[k], w), w).detach().reshape(-1)
            err = float((hess[:, k, c] - r).abs().max() / r.abs().max())
            assert err < TOL['bf16x2']['jac'], (k, c, err)


def test_one_point_backward_per_loss_backward_and_none_for_first_derivatives(monkeypatch):
    from deepphysinet_amd import point_path as P
    calls = []
    real = P._backward_points

    def counted(*a, **k):
        calls.append(k.get('g_hxi') is not None)
        return real(*a, **k)
    monkeypatch.setattr(P, '_backward_points', counted)
    m = _model('bf16x2')
    g = _gpu(synthetic_inputs(512, tag='inter'))
    x, y, t = (g[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    fields = m.fields_at(x, y, t, g['field_data'], g['coord_data'], g['forecast_h'])
    parts, total = _reference_losses(m, x, y, t, fields, g['f'])     # 28 create_graph gradient() calls
    assert calls == []
    loss = total + _second_order_loss(fields, x, y, t) * 1e-9
    assert calls == []
    loss.backward()
    assert calls == [True], calls                                      # ONE point backward, with the second-derivative cotangent


@pytest.mark.parametrize('prec', ['bf16x2', 'bf16'])
def test_derivative_entries_without_derivatives_are_the_fused_steps(prec):
    """dpn_fwd_ref_derivs / dpn_bwd_points_derivs with hess_n = d3_n = g_hxi = NULL give bit for bit what dpn_fwd_ref + dpn_bwd_points_scaled give
    (fields, Jacobian, saved state, operands, every weight gradient); with the derivative outputs on, fields / Jacobian / saved state are unchanged."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as P
    n = 1037
    m = _model(prec)
    g = _gpu(synthetic_inputs(n, tag='inter'))
    cfg = m.point_config()
    lib = L.load()
    dev = g['x'].device
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        statics = [s.detach().contiguous() for s in statics]
    nets = P._net_ptrs(heads, evec, statics)
    x, y, t = (g[k].reshape(-1).contiguous() for k in ('x', 'y', 't'))
    cd = g['coord_data'].contiguous()
    geo, fr = cfg.geometry(), P._freqs(dev)
    ws = P._Workspace(n, cfg.prec, dev)
    L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0), P._ptr(ws.packed), P._stream()), 'pack')
    g_out = torch.randn(n, 6, device=dev)
    g_jxi = torch.randn(n, 6, 3, device=dev)
    scale = torch.full((1,), 0.75, device=dev)

    def run(new, derivs=False):
        out = torch.empty(n, 6, device=dev)
        jac = torch.empty(n, 6, 3, device=dev)
        hess, d3 = (torch.empty(n, 6, 3, device=dev) for _ in range(2)) if derivs else (None, None)
        saved = torch.zeros(ws.sizes.saved, dtype=torch.uint8, device=dev)           # (zeroed: the buffers have bytes no kernel writes)
        operands = torch.zeros(ws.sizes.operands, dtype=torch.uint8, device=dev)
        partials = torch.empty(ws.sizes.partials, dtype=torch.uint8, device=dev)
        args = (P._ptr(x), P._ptr(y), P._ptr(t), None, P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac))
        if new:
            L.check(lib.dpn_fwd_ref_derivs(*args, P._ptr(hess), P._ptr(d3), P._ptr(saved), P._stream()), 'fwd derivs')
        else:
            L.check(lib.dpn_fwd_ref(*args, P._ptr(saved), P._stream()), 'fwd')
        bargs = (P._ptr(x), P._ptr(y), P._ptr(t), None, P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(g_out), P._ptr(g_jxi))
        if new:
            L.check(lib.dpn_bwd_points_derivs(*bargs, None, P._ptr(scale), P._ptr(saved), P._ptr(operands), P._stream()), 'bwd derivs')
        else:
            L.check(lib.dpn_bwd_points_scaled(*bargs, P._ptr(scale), P._ptr(saved), P._ptr(operands), P._stream()), 'bwd')
        g_heads = torch.empty(256, P.HEADS_COLS, device=dev)
        g_evec = torch.empty(6, 256, device=dev)
        g_stat = [torch.empty(P.STATIC_SHAPES[i % 8], device=dev) for i in range(48)]
        L.check(lib.dpn_wgrad(n, cfg.prec, P._ptr(g_out), P._ptr(saved), P._ptr(operands), P._ptr(partials), P._stream()), 'wgrad')
        L.check(lib.dpn_wgrad_finish(nets, P._ptr(ws.packed), n, cfg.prec, P._ptr(partials), P._net_ptrs(g_heads, g_evec, g_stat, cls=L.DpnNetGradPtrs),
                                     P._stream()), 'finish')
        torch.cuda.synchronize()
        return [out, jac, saved, operands, g_heads, g_evec] + g_stat
    old, new = run(False), run(True)
    for i, (a_, b_) in enumerate(zip(old, new)):
        assert torch.equal(a_, b_), i
    with_derivs = run(True, derivs=True)
    for i in range(3):
        assert torch.equal(old[i], with_derivs[i]), i
    # the new entries validate their arguments as their neighbours do
    bad = lib.dpn_fwd_ref_derivs(P._ptr(x), P._ptr(y), P._ptr(t), P._ptr(torch.zeros(n, 192, device=dev)), P._ptr(cd), None, n, P._ptr(fr),
                                 ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(old[0]), P._ptr(old[1]), None, None, None, P._stream())
    assert bad == -1
    bad = lib.dpn_fwd_ref_derivs(P._ptr(x), P._ptr(y), P._ptr(t), None, P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed),
                                 cfg.prec, P._ptr(old[0]), None, P._ptr(old[1]), None, None, P._stream())
    assert bad == -1                                                    # a second derivative without the Jacobian


def test_a_third_derivative_does_not_train():
    m = _model('bf16x2')
    g = _gpu(synthetic_inputs(256, tag='inter'))
    x, y, t = (g[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    u = m.fields_at(x, y, t, g['field_data'], g['coord_data'], g['forecast_h'])[0]
    u_xxx = _grad(_grad(_grad(u, x), x), x)
    assert bool(torch.isfinite(u_xxx).all())
    with pytest.raises(RuntimeError, match='third derivative'):
        u_xxx.sum().backward()
