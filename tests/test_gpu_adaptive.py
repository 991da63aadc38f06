"""GPU (MI355X): residual-weighted interior collocation points -- dpn_adaptive_scores / dpn_adaptive_select through PackedField.residual_scores,
CollocationSampler.select_weighted / get_inter_data_adaptive, InterfacePhysics.adaptive_interior and the training loops' option.

Yardsticks: torch fp64 on the same residual buffer (scores: 1e-14 relative -- six fp64 products and sums), the host reference
deepphysinet_amd.adaptive.select_reference fed the kernel's own scores and uniforms (indices: equal wherever u * total is farther than eps = m 2^-52, the
worst-case relative reordering error of a sum of m non-negative fp64 terms, from a boundary of the prefix sum; at most 1 of 4096 draws inside that band),
the pool's own rows (gather: bitwise), and eager host-offset runs (graph replays: bitwise)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.fill import fill_state_dict_, synthetic_inputs
from tests.test_sampler import _sampler

N, POOL = 4096, 32768
KC = ((1.0, 1.0), (2.0, 0.0), (0.5, 0.1), (0.0, 0.0))


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _model(init='scaled'):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config(), precision='bf16x2')
    if init == 'scaled':
        from deepphysinet_amd.utils.init import scaled_init_
        scaled_init_(m.physics_net, seed=1)
    else:
        sd = m.physics_net.state_dict()
        fill_state_dict_(sd)
        m.physics_net.load_state_dict(sd)
    return m.to(_dev())


def _factors(m):
    from deepphysinet_amd.point_path import LOSS_ORDER
    lf = m.train_cfg['losses']['loss_factor']
    return [float(lf[k]) for k in LOSS_ORDER]


_cache = {}


def _field_and_model():
    """(model, PackedField of one synthetic field for POOL points, factors): built once, read-only."""
    if 'm' not in _cache:
        m = _model()
        inp = synthetic_inputs(8)
        with torch.no_grad():
            field = m._inference_weights(inp['field_data'].to(_dev()), inp['forecast_h'].to(_dev()), POOL)
        _cache['m'] = (m, field, _factors(m))
    return _cache['m']


def _check_selection(score, u, idx, k, c):
    """The kernel's indices against select_reference on the kernel's own scores and uniforms (module docstring).

    The cap on draws inside the eps band: 1, as long as such a draw is a rare event.  A uniform target lies within eps (relative) of a boundary of the
    prefix sum with probability sum_i 2 eps cdf_i / total ~ eps m = m^2 2^-52 per draw: 1e-3 expected among 4096 draws from 32 768 candidates, where
    the cap of 1 holds; at m = 2^20 the same count is a Poisson variable of mean lambda ~ 1 (more than one with probability 0.26 whatever the kernel
    does), so there -- wherever lambda >= 0.01 -- the cap is that distribution's 1 - 1e-6 quantile, lambda computed from the reference's own prefix sum.
    Nothing else is relaxed: every index satisfies the interval condition, and equals the reference's outside the band."""
    from scipy import stats
    from deepphysinet_amd.adaptive import select_reference
    score, u, idx = (v.cpu().numpy() for v in (score, u, idx))
    m = score.size
    eps = m * 2.0 ** -52
    ref, w, cdf = select_reference(score, u, k, c)
    target = u * cdf[-1]
    assert idx.min() >= 0 and idx.max() < m
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    assert np.all(lo * (1 - eps) <= target) and np.all(target <= cdf[idx] * (1 + eps))
    lo_ref = np.where(ref > 0, cdf[np.maximum(ref - 1, 0)], 0.0)
    band = ((target < lo_ref * (1 + eps)) & (ref > 0)) | (target > cdf[ref] * (1 - eps))
    print('k %g c %g m %d: %d draws, %d inside the eps band, %d differ from the reference' % (k, c, m, u.size, band.sum(), (idx != ref).sum()))
    lam = u.size * 2.0 * eps * cdf.sum() / cdf[-1]
    cap = 1 if lam < 0.01 else max(1, int(stats.poisson.ppf(1.0 - 1e-6, lam)))
    assert band.sum() <= cap, (band.sum(), cap, lam)
    np.testing.assert_array_equal(idx[~band], ref[~band])
    assert np.all(w[idx] > 0.0)
    return ref, w, cdf


# ------------------------------------------------------------------------------------------------ 5. scores
def test_scores_equal_the_fp64_sum_of_the_same_residuals():
    m, field, fac = _field_and_model()
    s, _, _ = _sampler(with_labels=False)
    x, y, t, cd, f = s.get_inter_data(POOL)
    for k in (1.0, 2.0, 0.5):
        score, stats, res, _ = field.residual_scores(x, y, t, f.reshape(-1), cd, fac, k)
        r = res.double()
        want = torch.zeros(POOL, dtype=torch.float64, device=res.device)
        for e in range(6):
            want = want + fac[e] * (r[:, e] * r[:, e])
        bad = ~torch.isfinite(want)
        want = torch.where(bad, torch.zeros_like(want), want)
        rel = ((score - want).abs() / want.clamp_min(1e-300)).max().item()
        sk = (want ** k).sum().item()
        print('k %g: max rel score error %.3g, sum s^k %.17g (kernel %.17g), non-finite %d, max %.6g' % (k, rel, sk, stats[0].item(), int(bad.sum()), stats[2].item()))
        assert rel <= 1e-14
        assert abs(stats[0].item() - sk) <= POOL * 2.0 ** -52 * sk
        assert stats[1].item() == float(bad.sum()) and stats[2].item() == score.max().item()
    # non-finite residuals: the score is 0 and counted
    res2 = res.clone()
    res2[5, 2], res2[77, 0], res2[POOL - 1, 5] = float('nan'), float('inf'), 3e38
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    import ctypes
    lib = L.load()
    score2, stats2 = torch.empty_like(score), torch.empty_like(stats)
    scratch = torch.empty(int(lib.dpn_adaptive_scratch_doubles(POOL)), dtype=torch.float64, device=res.device)
    big = (ctypes.c_double * 6)(*[1e280] * 6)
    L.check(lib.dpn_adaptive_scores(_ptr(res2), POOL, big, 1.0, _ptr(score2), _ptr(stats2), _ptr(scratch), _stream()), 'dpn_adaptive_scores')
    r2 = res2.double()
    want2 = torch.zeros(POOL, dtype=torch.float64, device=res.device)
    for e in range(6):
        want2 = want2 + 1e280 * (r2[:, e] * r2[:, e])
    n_bad = int((~torch.isfinite(want2)).sum())
    assert n_bad >= 3 and stats2[1].item() == float(n_bad)
    assert score2[5].item() == 0.0 and score2[77].item() == 0.0 and score2[POOL - 1].item() == 0.0
    assert torch.isfinite(score2).all() and torch.isfinite(stats2).all()


# ------------------------------------------------------------------------------------------------ 6, 7, 9. selection against the host reference
@pytest.mark.parametrize('k,c', KC)
def test_selection_matches_the_host_reference_and_gathers_the_pool_rows(k, c):
    from deepphysinet_amd.adaptive import probabilities
    m, field, fac = _field_and_model()
    s, _, _ = _sampler(with_labels=False)
    x, y, t, cd, f, d = s.get_inter_data_adaptive(field, fac, n=N, pool=POOL, k=k, c=c, with_details=True)
    assert s.offset == POOL and x.shape == (N,) and cd.shape == (N, 6) and f.shape == (N, 1)
    assert d['idx'].dtype == torch.int32 and d['u'].dtype == torch.float64 and d['score'].shape == (POOL,)
    assert d['nonfinite'].item() == float((~torch.isfinite((d['res'].double() ** 2 * torch.tensor(fac, dtype=torch.float64, device=x.device)).sum(1))).sum())
    ref, w, cdf = _check_selection(d['score'], d['u'], d['idx'], k, c)
    # the kernel's prefix sum itself: within eps of the sequential one, its last entry the total
    got = d['cdf'].cpu().numpy()
    assert np.all(np.diff(got) >= 0.0) and np.all(np.abs(got - cdf) <= POOL * 2.0 ** -52 * cdf)
    # 7. the drawn rows are rows idx of the pool, bitwise; t is still whole hours
    idx = d['idx'].long()
    px, py, pt, pf, pcd = d['pool']
    for a, b in ((x, px[idx]), (y, py[idx]), (t, pt[idx]), (f.reshape(-1), pf[idx]), (cd, pcd[idx])):
        assert torch.equal(a, b)
    hours = t.double() / 3600.0
    assert torch.equal(hours, hours.round()) and hours.min() >= 0 and hours.max() <= 24
    assert torch.equal(d['picked_score'], d['score'][idx])
    # 9. the draws concentrate where the residual is large: mean picked score = sum p s within 6 standard errors; sum p s >= mean s (Chebyshev's sum
    # inequality: s and the weights are similarly ordered)
    sc = d['score'].cpu().numpy()
    p = probabilities(sc, k, c)
    mean_p = (p * sc).sum()
    se = np.sqrt(((p * sc * sc).sum() - mean_p ** 2) / N)
    got_mean = d['picked_score'].mean().item()
    print('k %g c %g: mean score of the pool %.6g, expected of the draws %.6g, drawn %.6g (%.2f standard errors)' %
          (k, c, sc.mean(), mean_p, got_mean, (got_mean - mean_p) / se))
    assert abs(got_mean - mean_p) <= 6.0 * se
    assert mean_p >= sc.mean() * (1.0 - POOL * 2.0 ** -52)
    if k > 0:
        assert mean_p > sc.mean()


@pytest.mark.parametrize('m', [1, 1023, 1025, 3071, 3073, 1 << 20])
def test_selection_on_given_scores_with_zeros_and_block_boundary_sizes(m):
    s, _, _ = _sampler(with_labels=False)
    dev = s.cube.device
    g = torch.Generator().manual_seed(m)
    score = torch.exp(3.0 * torch.randn(m, generator=g, dtype=torch.float64))
    score[torch.rand(m, generator=g) < 0.25] = 0.0
    if m > 1:
        score[0], score[m - 1] = 0.0, 0.0                                 # zero weights at both ends (c = 0)
        if m > 1024:
            score[1023:1026] = 0.0                                        # ... and across a block boundary
        score[m // 2] = 1.0
    score = score.to(dev)
    rows = tuple(torch.rand(m, generator=g).to(dev) for _ in range(4)) + (torch.rand(m, 6, generator=g).to(dev),)
    for k, c in KC:
        x, y, t, f, cd, idx, u, picked, scratch = s.select_weighted(score, rows, N, k, c, offset=123, with_details=True)
        if m == 1:
            assert (idx == 0).all()
        _check_selection(score, u, idx, k, c)
        if c == 0.0 and k > 0.0 and m > 1:
            assert (picked > 0).all()                                     # a zero weight is never drawn
        assert torch.equal(cd, rows[4][idx.long()]) and torch.equal(x, rows[0][idx.long()])
    # all scores zero: uniform, with c = 0 as well
    x, y, t, f, cd, idx, u, picked, scratch = s.select_weighted(torch.zeros_like(score), rows, N, 1.0, 0.0, with_details=True)
    assert torch.equal(idx.long(), (u * m).long().clamp_max(m - 1))
    # refused, not truncated
    with pytest.raises(ValueError, match='2\\*\\*20'):
        s.select_weighted(torch.zeros((1 << 20) + 1, dtype=torch.float64, device=dev), tuple(torch.zeros(1, device=dev) for _ in range(5)), 4)


# ------------------------------------------------------------------------------------------------ 8. the uniforms
def test_uniforms_are_uniform_and_independent_of_the_pools_own_draws():
    from scipy import stats
    s, _, _ = _sampler(with_labels=False)
    n = 1 << 20
    x, y, t, cd, f, raw = s.get_inter_data(n, with_raw=True)               # counters 0 .. n - 1, streams 0 and 1
    score = torch.ones(n, dtype=torch.float64, device=x.device)
    out = s.select_weighted(score, (x, y, t, f.reshape(-1), cd), n, 1.0, 1.0, offset=0, with_details=True)
    u = out[6].cpu().numpy()
    assert u.min() >= 0.0 and u.max() < 1.0
    us = np.sort(u)
    grid = np.arange(1, n + 1) / n
    ks = max((grid - us).max(), (us - (grid - 1.0 / n)).max())
    ux = raw[:, 0].cpu().numpy() / 256.0
    corr = np.corrcoef(u, ux)[0, 1]
    print('KS statistic %.3g (bound %.3g), correlation with the x draw %.3g (bound %.3g)' % (ks, stats.kstwo.isf(1e-6, n), corr, 6 / np.sqrt(n)))
    assert ks < stats.kstwo.isf(1e-6, n)
    assert abs(corr) <= 6.0 / np.sqrt(n)
    assert not np.array_equal(u, ux)


# ------------------------------------------------------------------------------------------------ 10. determinism and replay
def test_two_runs_agree_bitwise_and_graph_replays_equal_the_eager_steps():
    m, field, fac = _field_and_model()
    keys = ('idx', 'u', 'picked_score', 'score', 'cdf')

    def run(s):
        s.begin_step()
        x, y, t, cd, f, d = s.get_inter_data_adaptive(field, fac, n=N, pool=POOL, with_details=True)
        return (x, y, t, cd, f) + tuple(d[k] for k in keys)

    a, b = run(_sampler(with_labels=False)[0]), run(_sampler(with_labels=False)[0])
    for v, w in zip(a, b):
        assert torch.equal(v, w)
    s, _, _ = _sampler(with_labels=False)
    step = torch.zeros(1, dtype=torch.int32, device=_dev())
    s.bind_step_counter(step, POOL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s)
        run(s)                                                            # two warm-ups on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(s)                                                      # pool draw + residuals + scores + select, one stream
    seen = []
    for kstep in (1, 2, 3):
        step.fill_(kstep)
        g.replay()
        torch.cuda.synchronize()
        seen.append([v.clone() for v in out])
    for kstep, got in zip((1, 2, 3), seen):
        ref, _, _ = _sampler(with_labels=False)
        ref.offset = kstep * POOL                                         # the host-offset run of the same step
        for v, w in zip(got, run(ref)):
            assert torch.equal(v, w), kstep
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0]) and not torch.equal(seen[0][5], seen[2][5])
    with pytest.raises(RuntimeError, match='reserved'):                   # the pool counts against the reservation
        s.begin_step()
        s.get_inter_data(1)
        s.get_inter_data_adaptive(field, fac, n=N, pool=POOL)


# ------------------------------------------------------------------------------------------------ 11. adaptive_interior and the loops
def test_adaptive_interior_returns_a_trainable_batch_and_touches_nothing():
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model('fill')
    src = SyntheticSamples(_dev())
    batch = src[0]
    params = [p.detach().clone() for p in m.physics_net.parameters()]
    new = m.adaptive_interior(batch, src.sampler, pool_factor=8, k=1.0, c=1.0)
    assert set(new) == set(batch)
    for key in batch:
        if key.startswith('inter_'):
            assert new[key].shape == batch[key].shape and new[key].dtype == batch[key].dtype and not torch.equal(new[key], batch[key]), key
        else:
            assert new[key] is batch[key]
    assert all(torch.equal(p, q) for p, q in zip(params, m.physics_net.parameters())) and all(p.grad is None for p in m.physics_net.parameters())
    assert m.physics_net._meta_cache is None
    hours = new['inter_t'].double() / 3600.0
    assert torch.equal(hours, hours.round()) and torch.isfinite(new['inter_data']).all()
    opt = m.build_optimizer()
    loss, parts, gnorm = m.training_step(new, opt, with_pde=True)
    assert torch.isfinite(loss) and all(torch.isfinite(v) for v in parts.values())
    assert set(parts) == {'margin_loss', 'inter_pde_loss', 'margin_pde_loss'}
    with pytest.raises(ValueError, match='pool_factor'):
        m.adaptive_interior(batch, src.sampler, pool_factor=0)


def _loop(adaptive=None, spy=None):
    m = _model('fill')
    if spy is not None:
        inner_a, inner_s = m.adaptive_interior, m.training_step
        m.adaptive_interior = lambda *a, **k: (spy.append('adaptive'), inner_a(*a, **k))[1]
        m.training_step = lambda *a, **k: (spy.append('step'), inner_s(*a, **k))[1]
    kw = {} if adaptive is None else {'adaptive_interior': adaptive}
    out = m.run_train_interface(samples='synthetic', pde_start_step=0, max_steps=3, num_epoch=1, samples_per_epoch=4, **kw)
    assert out['global_step'] == 3
    return m, out


def test_loop_with_the_option_trains_and_without_it_is_undisturbed():
    spy = []
    m, out = _loop(dict(pool_factor=4, k=1.0, c=1.0), spy)
    assert spy == ['adaptive', 'step'] * 3
    assert torch.isfinite(out['last']['loss']) and all(torch.isfinite(v) for v in out['last']['parts'].values())
    spy = []
    m, out = _loop(dict(every=2), spy)
    assert spy == ['adaptive', 'step', 'step', 'adaptive', 'step'] and torch.isfinite(out['last']['loss'])
    # the option unset: not one call, and two such runs end in the same parameters bitwise
    spy = []
    m1, out1 = _loop(None, spy)
    assert spy == ['step'] * 3
    m2, out2 = _loop(None)
    for (name, p), q in zip(m1.physics_net.named_parameters(), m2.physics_net.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(out1['last']['loss'], out2['last']['loss'])
    assert not all(torch.equal(p, q) for p, q in zip(m.physics_net.parameters(), m1.physics_net.parameters()))      # ... and the option does change the run
