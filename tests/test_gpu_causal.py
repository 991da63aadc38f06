"""GPU (MI355X): per-point weights and causal time weighting of the PDE losses -- dpn_causal_bins / dpn_causal_weights / dpn_residual_weighted through the
C ABI, point_path.pde_losses / step_losses, InterfacePhysics.pde_loss_terms / training_step and the training loops' option.

Yardsticks: the host references of deepphysinet_amd.causal fed the kernels' own per-point residual rows (dpn_residual_points) and the same t; the
unweighted dpn_residual (bitwise where the weights are 1 or a power of two); eager runs (graph replays: bitwise).

Bounds of test 1, u = 2^-52 (twice the unit roundoff, so every "rounding" below is at most u / 2 relative):
  l_k   the kernel and the reference add the same <= n non-negative s_i of bin k in different orders: each side is within (n - 1) u / 2 of the exact sum,
        together (n - 1) u; the s_i themselves are formed by the same twelve fp64 operations on both sides (a slack of 12 u covers a library that
        contracts one of them); the division adds u / 2 per side: (n + 16) u relative.
  W_k   cum_k is a sum of at most `bins` terms l_j (/ norm), each within (n + 16) u, the normaliser within (n + bins) u, the prefix sum itself the
        same sequential order on both sides: x_k = eps * cum_k is within (n + bins + 16) u relative (rounded up), so exp(-x_k) moves by the factor
        exp(x_k delta), i.e. x_k (n + bins + 16) u relative; exp's own error is below one unit in the last place on either side and the product
        eps * cum_k rounds once per side: 4 u.  Where W_k < 1e-300 (subnormal results keep no relative accuracy) the same number bounds the absolute
        difference."""
import copy
import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from oracle.fill import synthetic_inputs
from tests.test_gpu_adaptive import _dev, _model
from tests.test_sampler import _sampler

U = 2.0 ** -52
SIZES = (1, 255, 257, 1000, 4096)
T_SPAN = 86400.0
TINY = 2.0 ** -126

_cache = {}


def _lib():
    from deepphysinet_amd import _lib as L
    return L, L.load()


def _weights_of_field():
    """(model, heads, evec, statics) of one synthetic field: built once, read-only."""
    if 'm' not in _cache:
        m = _model()
        inp = synthetic_inputs(8)
        with torch.no_grad():
            hw = m.physics_net.field_weights(inp['field_data'].to(_dev()), inp['forecast_h'].to(_dev()))
        _cache['m'] = (m, inp) + tuple(hw)
    return _cache['m']


def _fields(n, same_t=False):
    """n interior points and the forward kernel's fields and Jacobian at them: dict(x, y, t, f, cd, out_n, jac_n); computed once per size."""
    key = ('f', n, same_t)
    if key not in _cache:
        from deepphysinet_amd.point_path import pde_fields_and_jacobian
        m, _, heads, evec, statics = _weights_of_field()
        s, _, _ = _sampler(with_labels=False)
        x, y, t, cd, f = s.get_inter_data(n)
        if same_t:
            t = torch.full_like(t, 3.0 * 3600.0)
        out_n, jac_n = pde_fields_and_jacobian(m.point_config(), x, y, t, cd, heads, evec, statics)
        _cache[key] = dict(x=x, y=y, t=t.contiguous(), f=f.reshape(-1).contiguous(), cd=cd, out_n=out_n, jac_n=jac_n, n=n)
    return _cache[key]


def _cfg(case='mse', reduce_sum=False):
    """The point configuration of a criterion / physics case.  clip and the squared form go through the model's obs_norm_cfg, as test_gpu_parity builds
    them; the criterion and its reduction are fields of the configuration."""
    from deepphysinet_amd import _lib as L
    m = _weights_of_field()[0]
    saved, clip = copy.deepcopy(m.obs_norm_cfg), m.with_clip
    try:
        if case == 'sq':
            for name, c in zip(('u10', 'v10', 'pres', 't2', 'q2', 'rio'), O.f12_norm_sq_cfg()):
                m.obs_norm_cfg[name].update(norm_type=c['norm_type'], norm_factor=c['norm_factor'], use_norm=c['use_norm'])
        m.with_clip = case != 'noclip'
        cfg = m.point_config()
    finally:
        m.obs_norm_cfg.clear()
        m.obs_norm_cfg.update(saved)
        m.with_clip = clip
        m.point_config()
    crit, beta = {'l1': (L.CRIT_L1, 0.0), 'sl1': (L.CRIT_SMOOTH_L1, 0.1)}.get(case, (L.CRIT_MSE, 0.0))
    return dataclasses.replace(cfg, criterion=crit, beta=beta, reduce_sum=reduce_sum)


def _residual_rows(cfg, F):
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    res = torch.empty((F['n'], 6), dtype=torch.float32, device=_dev())
    geo, ph = cfg.geometry(), cfg.physics()
    L.check(lib.dpn_residual_points(_ptr(F['out_n']), _ptr(F['jac_n']), _ptr(F['f']), F['n'], ctypes.byref(geo), ctypes.byref(ph), _ptr(res), _stream()),
            'dpn_residual_points')
    return res.cpu().numpy()


def _call_bins(cfg, F, bins, t_lo=0.0, t_hi=T_SPAN):
    """-> (return code, bin, rows); the buffers are sized for 64 bins whatever `bins` says, so that a rejected call could not write past them."""
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    n = F['n']
    geo, ph = cfg.geometry(), cfg.physics()
    fac = (ctypes.c_double * 6)(*[float(v) for v in cfg.factors])
    bin_ = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    rows = torch.full((((n + 255) // 256) * 64 * 2,), -7.0, dtype=torch.float64, device=_dev())
    rc = lib.dpn_causal_bins(_ptr(F['out_n']), _ptr(F['jac_n']), _ptr(F['f']), _ptr(F['t']), n, ctypes.byref(geo), ctypes.byref(ph), fac, float(t_lo),
                             float(t_hi), int(bins), _ptr(bin_), _ptr(rows), _stream())
    return rc, bin_, rows


def _call_weights(rows, n, bins, eps, relative):
    from deepphysinet_amd.point_path import _ptr, _stream
    L, lib = _lib()
    w32 = torch.full((64,), -7.0, dtype=torch.float32, device=_dev())
    diag = torch.full((3 * 64 + 2,), -7.0, dtype=torch.float64, device=_dev())
    rc = lib.dpn_causal_weights(_ptr(rows), n, int(bins), float(eps), int(relative), _ptr(w32), _ptr(diag), _stream())
    return rc, w32, diag


def _call_residual(cfg, F, w=None, bin_=None, bin_w=None, weighted=True):
    """dpn_residual(_weighted) with loss rows and the cotangents of a unit total -> (return code, sums, g_out, g_jxi, finished losses [7])."""
    from deepphysinet_amd.point_path import _one, _ptr, _stream
    L, lib = _lib()
    n, dev = F['n'], _dev()
    geo, ph = cfg.geometry(), cfg.physics()
    sums = torch.full((((n + 255) // 256) * 6,), -7.0, dtype=torch.float64, device=dev)
    g_out, g_jxi = torch.full((n, 6), -7.0, device=dev), torch.full((n, 6, 3), -7.0, device=dev)
    args = (_ptr(F['out_n']), _ptr(F['jac_n']), _ptr(F['f']), n, ctypes.byref(geo), ctypes.byref(ph), None, _ptr(_one(dev)), _ptr(sums), _ptr(g_out),
            _ptr(g_jxi))
    if weighted:
        rc = lib.dpn_residual_weighted(*args, _ptr(w), _ptr(bin_), _ptr(bin_w), _stream())
    else:
        rc = lib.dpn_residual(*args, _stream())
    losses = torch.empty(7, dtype=torch.float32, device=dev)
    if rc == 0:
        L.check(lib.dpn_residual_finish(_ptr(sums), n, ctypes.byref(ph), _ptr(losses), _stream()), 'dpn_residual_finish')
    return rc, sums, g_out, g_jxi, losses


# ------------------------------------------------------------------------------------------------ 1. bins and weights against the host reference
def _check_bins_and_weights(F, bins):
    from deepphysinet_amd.causal import bin_index, bin_weights_reference, point_loss_reference
    cfg = _cfg()
    n = F['n']
    rc, bin_, rows = _call_bins(cfg, F, bins)
    assert rc == 0
    s = point_loss_reference(_residual_rows(cfg, F), cfg.factors)
    assert np.isfinite(s).all()
    t = F['t'].cpu().numpy()
    want_bin = bin_index(t, 0.0, T_SPAN, bins)
    got_bin = bin_.cpu().numpy()
    np.testing.assert_array_equal(got_bin, want_bin)
    for eps in (0.0, 0.5, 5.0):
        for relative in (True, False):
            rc, w32, diag = _call_weights(rows, n, bins, eps, relative)
            assert rc == 0
            W, l, count = bin_weights_reference(s, want_bin, bins, eps, relative)
            d = diag.cpu().numpy()
            gW, gl, gc, gmin, gnorm = d[:bins], d[bins:2 * bins], d[2 * bins:3 * bins], d[3 * bins], d[3 * bins + 1]
            np.testing.assert_array_equal(gc, count)
            assert (gl[count == 0] == 0.0).all()
            rel_l = np.abs(gl - l) / np.where(l > 0, l, 1.0)
            norm = l[count > 0].sum() / (count > 0).sum() if relative else 1.0
            x = eps * np.concatenate([[0.0], np.cumsum(l / norm)[:-1]])
            with np.errstate(invalid='ignore', over='ignore'):
                bound = x * (n + bins + 16) * U + 4 * U
                err = np.where(W < 1e-300, np.abs(gW - W), np.abs(gW - W) / np.where(W > 0, W, 1.0))
            print('n %d bins %d eps %g relative %d: occupied %d, max rel l error %.3g (bound %.3g), max W error / bound %.3g, min W %.6g' %
                  (n, bins, eps, relative, (count > 0).sum(), rel_l.max(), (n + 16) * U, np.nanmax(err / bound), gmin))
            assert (rel_l <= (n + 16) * U).all()
            assert np.isfinite(gW).all() and (err <= bound).all()
            assert gW[0] == 1.0 and (np.diff(gW) <= 0).all() and gmin == gW.min()
            assert abs(gnorm - norm) <= (n + bins) * U * norm
            np.testing.assert_array_equal(w32.cpu().numpy()[:bins], gW.astype(np.float32))
            assert (w32[bins:] == -7.0).all() and (diag[3 * bins + 2:] == -7.0).all()           # nothing past n_bins is written
            if eps == 0.0:
                assert (w32[:bins] == 1.0).all()
    return count


@pytest.mark.parametrize('bins', [1, 5, 64])
@pytest.mark.parametrize('n', SIZES)
def test_bins_and_weights_equal_the_host_reference(n, bins):
    count = _check_bins_and_weights(_fields(n), bins)
    if n < bins:
        assert (count == 0).any()


def test_all_points_at_one_time_occupy_one_bin():
    count = _check_bins_and_weights(_fields(1000, same_t=True), 5)
    assert (count > 0).sum() == 1 and count.sum() == 1000


# ------------------------------------------------------------------------------------------------ 2. the weighted residual kernel
CASES = [('mse', False), ('mse', True), ('l1', False), ('l1', True), ('sl1', False), ('sl1', True), ('noclip', False), ('sq', False)]


@pytest.mark.parametrize('case,reduce_sum', CASES)
def test_unit_weights_are_bitwise_the_unweighted_kernel(case, reduce_sum):
    cfg = _cfg(case, reduce_sum)
    if case == 'sq':
        assert cfg.physics().sq_on[4] == 1
    for n in (257, 1000):
        F = _fields(n)
        rc0, s0, go0, gj0, l0 = _call_residual(cfg, F, weighted=False)
        ones = torch.ones(n, device=_dev())
        rc1, s1, go1, gj1, l1 = _call_residual(cfg, F, w=ones)
        zero_bin, one_w = torch.zeros(n, dtype=torch.int32, device=_dev()), torch.ones(1, device=_dev())
        rc2, s2, go2, gj2, l2 = _call_residual(cfg, F, bin_=zero_bin, bin_w=one_w)
        rc3, s3, go3, gj3, l3 = _call_residual(cfg, F, w=ones, bin_=zero_bin, bin_w=one_w)
        assert rc0 == rc1 == rc2 == rc3 == 0
        for s, go, gj, l in ((s1, go1, gj1, l1), (s2, go2, gj2, l2), (s3, go3, gj3, l3)):
            assert torch.equal(s.view(torch.int64), s0.view(torch.int64)), (case, n)
            assert torch.equal(go.view(torch.int32), go0.view(torch.int32)) and torch.equal(gj.view(torch.int32), gj0.view(torch.int32)), (case, n)
            assert torch.equal(l.view(torch.int32), l0.view(torch.int32))


@pytest.mark.parametrize('case,reduce_sum', [('mse', False), ('sl1', False), ('sq', False)])
def test_power_of_two_weights_scale_each_points_cotangent_rows_bitwise(case, reduce_sum):
    cfg = _cfg(case, reduce_sum)
    F = _fields(1000)
    g = torch.Generator().manual_seed(5)
    w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (1000,), generator=g)].to(_dev())
    _, _, go0, gj0, _ = _call_residual(cfg, F, weighted=False)
    rc, _, go, gj, _ = _call_residual(cfg, F, w=w)
    assert rc == 0
    for got, base in ((go, go0), (gj, gj0)):
        want = base * w.view(-1, *([1] * (base.dim() - 1)))
        assert torch.isfinite(want).all()
        assert ((want == 0) | (want.abs() >= TINY)).all() and ((base == 0) | (base.abs() >= TINY)).all(), 'a compared value is subnormal'
        assert torch.equal(got, want)
        assert (got[w == 0] == 0).all()


@pytest.mark.parametrize('case,reduce_sum', [('mse', False), ('l1', True), ('sl1', False)])
def test_weighted_losses_equal_the_host_reference(case, reduce_sum):
    from deepphysinet_amd.causal import weighted_losses_reference
    cfg = _cfg(case, reduce_sum)
    for n in (257, 4096):
        F = _fields(n)
        res = _residual_rows(cfg, F)
        g = torch.Generator().manual_seed(n)
        w = (2.0 * torch.rand(n, generator=g)).to(_dev())
        rc, bin_, _ = _call_bins(cfg, F, 5)
        bw = (2.0 * torch.rand(5, generator=g)).to(_dev())
        assert rc == 0
        for kw, eff in ((dict(w=w), w), (dict(w=w, bin_=bin_, bin_w=bw), w * bw[bin_.long()]), (dict(bin_=bin_, bin_w=bw), bw[bin_.long()])):
            rc, _, _, _, losses = _call_residual(cfg, F, **kw)
            assert rc == 0
            want = weighted_losses_reference(res, eff.cpu().numpy(), cfg.factors, cfg.criterion, cfg.beta, reduce_sum)
            got = losses.cpu().numpy().astype(np.float64)
            rel = np.abs(got[:6] - want) / np.abs(want)
            print('%s n %d %s: max rel error %.3g (bound %.3g)' % (case, n, sorted(kw), rel.max(), 4 * 2.0 ** -24))
            assert (rel <= 4 * 2.0 ** -24).all()


# ------------------------------------------------------------------------------------------------ 3. through autograd
def _terms_and_grads(m, F, inp, idx=None, **kw):
    dev = _dev()
    pick = (lambda v: v) if idx is None else (lambda v: v[idx].contiguous())
    m.physics_net.zero_grad()
    terms, total = m.pde_loss_terms(pick(F['x']), pick(F['y']), pick(F['t']), pick(F['f']), inp['field_data'].to(dev), pick(F['cd']),
                                    inp['forecast_h'].to(dev), with_total=True, **kw)
    total.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in m.physics_net.named_parameters()}
    assert len(grads) == 155
    return terms.detach().clone(), total.detach().clone(), grads


@pytest.mark.parametrize('n', [257, 1000])
def test_point_weights_through_autograd(n):
    m, inp = _weights_of_field()[:2]
    F = _fields(n)
    dev = _dev()
    t0, tot0, g0 = _terms_and_grads(m, F, inp)
    # ones: bitwise
    t1, tot1, g1 = _terms_and_grads(m, F, inp, point_weights=torch.ones(n, 1, device=dev))
    assert torch.equal(t1, t0) and torch.equal(tot1, tot0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # 0.5: losses within one fp32 ulp of half, gradients bitwise half
    t2, tot2, g2 = _terms_and_grads(m, F, inp, point_weights=torch.full((n,), 0.5, device=dev))
    half = (t0.double() * 0.5)
    assert ((t2.double() - half).abs() <= 2.0 ** -23 * half.abs()).all()
    for k in g0:
        want = g0[k] * 0.5
        assert ((want == 0) | (want.abs() >= TINY)).all(), 'subnormal: ' + k
        assert torch.equal(g2[k], want), k
    # a 0/1 mask against the existing path on the kept points alone, times |S| / n
    gen = torch.Generator().manual_seed(n)
    keep = torch.rand(n, generator=gen) < 0.6
    idx = torch.nonzero(keep).flatten().to(dev)
    frac = float(keep.sum()) / n
    t3, tot3, g3 = _terms_and_grads(m, F, inp, point_weights=keep.float().to(dev))
    ts, tots, gs = _terms_and_grads(m, F, inp, idx=idx)
    rel = ((t3.double() - ts.double() * frac).abs() / (ts.double() * frac).abs()).max().item()
    worst = 0.0
    for k in g0:
        if k.endswith('key_projection.bias'):
            continue
        want = gs[k].double() * frac
        d = ((g3[k].double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
        worst = max(worst, d)
        assert d <= 1e-3, (k, d)
    print('n %d, %d kept: max rel loss error %.3g (bound %.3g), max gradient error / max-abs %.3g (bound 1e-3)' % (n, idx.numel(), rel, 4 * 2.0 ** -24, worst))
    assert rel <= 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 4, 5. the causal step, determinism, capture
def _step(causal=None):
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model('fill')
    batch = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=2, seed=3)[0]
    before = [p.detach().clone() for p in m.physics_net.parameters()]
    opt = m.build_optimizer()
    kw = {} if causal is None else {'causal': causal}
    loss, parts, gnorm = m.training_step(batch, opt, with_pde=True, **kw)
    return m, loss, parts, gnorm, before


def test_causal_step_with_eps_zero_is_the_plain_step_and_with_eps_two_weights_the_losses():
    from deepphysinet_amd.causal import CausalWeights
    m0, loss0, parts0, gnorm0, _ = _step()
    assert m0.last_causal is None
    m1, loss1, parts1, gnorm1, _ = _step(CausalWeights(eps=0))
    assert torch.equal(loss1, loss0) and torch.equal(torch.as_tensor(gnorm1), torch.as_tensor(gnorm0))
    for k in parts0:
        assert torch.equal(parts1[k], parts0[k]), k
    for (name, p), q in zip(m1.physics_net.named_parameters(), m0.physics_net.parameters()):
        assert torch.equal(p, q), name
    assert set(m1.last_causal) == {'inter', 'margin'} and (m1.last_causal['inter'][:16] == 1.0).all()
    m2, loss2, parts2, gnorm2, before = _step(CausalWeights(eps=2, bins=8))
    for group, key in (('inter', 'inter_pde_loss'), ('margin', 'margin_pde_loss')):
        d = m2.last_causal[group].cpu().numpy()
        assert d.shape == (26,)
        W, l, count = d[:8], d[8:16], d[16:24]
        assert count.sum() == 256 and W[0] == 1.0 and d[24] == W.min() < 1.0
        want = (W * count * l).sum() / 256.0
        got = float(parts2[key])
        print('%s: %s %.9g, sum_k W_k count_k l_k / n %.9g, unweighted %.9g' % (group, key, got, want, float(parts0[key])))
        assert abs(got - want) <= 16 * 2.0 ** -24 * want
        assert got < float(parts0[key])
    assert torch.equal(parts2['margin_loss'], parts0['margin_loss'])            # the data loss is not weighted
    moved = 0
    for p, q in zip(m2.physics_net.parameters(), before):
        assert torch.isfinite(p).all()
        moved += int(not torch.equal(p, q))
    assert moved > 0 and torch.isfinite(loss2)
    # 5. a second eager run agrees bitwise
    m3, loss3, parts3, gnorm3, _ = _step(CausalWeights(eps=2, bins=8))
    assert torch.equal(loss3, loss2) and torch.equal(m3.last_causal['inter'], m2.last_causal['inter'])
    for (name, p), q in zip(m3.physics_net.named_parameters(), m2.physics_net.parameters()):
        assert torch.equal(p, q), name


def test_causal_pde_losses_replayed_from_a_graph_equal_the_eager_results():
    from deepphysinet_amd.causal import CausalWeights
    from deepphysinet_amd.point_path import pde_losses
    m, _, heads, evec, statics = _weights_of_field()
    cfg = m.point_config()
    causal = CausalWeights(eps=2.0, bins=8)
    n, dev = 1000, _dev()
    src = [_fields(1000), _fields(1000, same_t=True)]
    keys = ('x', 'y', 't', 'f', 'cd')
    w_src = [torch.rand(n, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(2)]
    hd, ev = heads.detach().clone().requires_grad_(True), evec.detach().clone().requires_grad_(True)
    st = [s.detach().clone().requires_grad_(True) for s in statics]

    def run(buf, w):
        diag = []
        terms, total = pde_losses(cfg, buf['x'], buf['y'], buf['t'], buf['f'], buf['cd'], hd, ev, st, with_total=True, point_weights=w, causal=causal,
                                  diag=diag)
        grads = torch.autograd.grad(total, [hd, ev] + st)
        return (terms, total, diag[0]) + tuple(grads)

    eager = []
    for F, w in zip(src, w_src):
        eager.append([v.detach().clone() for v in run(F, w)])
    static = {k: src[0][k].clone() for k in keys}
    w_static = w_src[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static, w_static)
        run(static, w_static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(static, w_static)
    for F, w, want in zip(src, w_src, eager):
        for k in keys:
            static[k].copy_(F[k])
        w_static.copy_(w)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


# ------------------------------------------------------------------------------------------------ 6. the option off is undisturbed
NEW = ('dpn_causal_bins', 'dpn_causal_weights', 'dpn_residual_weighted')


class _Spy:
    """Counts calls of the three new entry points of the loaded library, tagged with what the loop's current step says about the PDE losses."""

    def __init__(self):
        _, self.lib = _lib()
        self.inner = {k: getattr(self.lib, k) for k in NEW}
        self.calls = []
        self.with_pde = None

    def __enter__(self):
        for k in NEW:
            setattr(self.lib, k, (lambda name: lambda *a: (self.calls.append((name, self.with_pde)), self.inner[name](*a))[1])(k))
        return self

    def __exit__(self, *exc):
        for k in NEW:
            setattr(self.lib, k, self.inner[k])


def _loop(spy, tmp_path, **kw):
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model('fill')
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    inner = m.training_step

    def step(*a, **k):
        spy.with_pde = k.get('with_pde')
        return inner(*a, **k)
    m.training_step = step
    src = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=4, seed=0)
    val = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=2, seed=1)
    out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path), max_steps=3, num_epoch=1, pde_start_step=1, **kw)
    assert out['global_step'] == 3
    return m, out


def test_loops_call_the_new_kernels_only_with_the_option_and_only_with_the_pde_losses(tmp_path):
    with _Spy() as spy:
        _loop(spy, tmp_path / 'off')
        assert spy.calls == []
        events = [json.loads(l) for l in open(tmp_path / 'off' / 'metrics.jsonl')]
        assert all('causal_min_w' not in e for e in events)
        m, out = _loop(spy, tmp_path / 'on', causal_weights=dict(eps=1.0))
        assert spy.calls and all(with_pde for _, with_pde in spy.calls)
        # steps 2 and 3 carry the PDE losses: per step two groups' bins and weights, and the weighted kernel in the forward and the backward pass
        assert [c[0] for c in spy.calls].count('dpn_causal_bins') == 4 and [c[0] for c in spy.calls].count('dpn_residual_weighted') == 8
    events = [json.loads(l) for l in open(tmp_path / 'on' / 'metrics.jsonl') if '"training"' in l]
    assert [e['global_step'] for e in events] == [1, 3]
    assert 'causal_min_w' not in events[0]                                  # step 1: before pde_start_step
    assert 0.0 <= events[1]['causal_min_w'] <= 1.0 and len(events[1]['causal_w']) == 16 and events[1]['causal_w'][0] == 1.0
    assert torch.isfinite(out['last']['loss'])
    with pytest.raises(ValueError, match='unknown keys'):
        m._causal_option({'causal_weights': dict(eps=1.0, bin=3)})
    m.train_cfg['losses']['causal_weights'] = dict(eps=0.5, bins=4, relative=False)          # the configuration's route
    opt = m._causal_option({})
    assert (opt.eps, opt.bins, opt.relative) == (0.5, 4, False) and m._causal_option({'causal_weights': None}) is None


def test_lead_batches_refuse_the_options():
    from deepphysinet_amd.causal import CausalWeights
    from deepphysinet_amd.point_path import pde_losses_batch
    m, _, heads, evec, statics = _weights_of_field()
    F = _fields(257)
    args = [F[k].unsqueeze(0) for k in ('x', 'y', 't', 'f', 'cd')] + [heads.unsqueeze(0), evec.unsqueeze(0), statics]
    with pytest.raises(NotImplementedError):
        pde_losses_batch(m.point_config(), *args, causal=CausalWeights(eps=1.0))
    with pytest.raises(NotImplementedError):
        pde_losses_batch(m.point_config(), *args, point_weights=torch.ones(1, 257, device=_dev()))


# ------------------------------------------------------------------------------------------------ 7. rejected arguments
def test_rejected_arguments_return_minus_one_and_launch_nothing():
    cfg = _cfg()
    F = _fields(257)
    untouched = lambda *ts: all(bool((t == -7).all()) for t in ts)
    for bins, t_lo, t_hi in ((0, 0.0, T_SPAN), (65, 0.0, T_SPAN), (8, 5.0, 5.0), (8, 0.0, float('inf')), (8, float('nan'), 1.0)):
        rc, bin_, rows = _call_bins(cfg, F, bins, t_lo, t_hi)
        torch.cuda.synchronize()
        assert rc == -1 and untouched(bin_, rows), (bins, t_lo, t_hi)
    rc, bin_, rows = _call_bins(cfg, F, 8)
    assert rc == 0
    for bins, eps in ((8, -1.0), (8, float('nan')), (8, float('inf')), (0, 1.0), (65, 1.0)):
        rc, w32, diag = _call_weights(rows, 257, bins, eps, True)
        torch.cuda.synchronize()
        assert rc == -1 and untouched(w32, diag), (bins, eps)
    rc, sums, g_out, g_jxi, _ = _call_residual(cfg, F)
    torch.cuda.synchronize()
    assert rc == -1 and untouched(sums, g_out, g_jxi)
    rc, sums, g_out, g_jxi, _ = _call_residual(cfg, F, bin_=bin_)               # bin without bin_w
    torch.cuda.synchronize()
    assert rc == -1 and untouched(sums, g_out, g_jxi)
