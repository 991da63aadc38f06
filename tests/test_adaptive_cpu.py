"""CPU: residual-weighted interior collocation points -- the C surface of csrc/dpn_adaptive.hip, the properties of the host reference
(deepphysinet_amd/adaptive.py) that the GPU tests hold the kernels to, and the training loops' `adaptive_interior` option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('dpn_adaptive_scratch_doubles', 'dpn_adaptive_scores', 'dpn_adaptive_select')


# ------------------------------------------------------------------------------------------------ 1. symbols and argument checks
def test_adaptive_symbols_unit_and_argument_checks():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import build
    lib = L.load()
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r'^\s*(?:int|int64_t)\s+%s\s*\(' % name, header, flags=re.M), name
    units = {obj: src for src, _, obj in build.UNITS}
    assert os.path.basename(units['dpn_adaptive.o']) == 'dpn_adaptive.hip' and len(units) == len(build.UNITS)
    assert units['dpn_adaptive.o'] in build.DEPS
    # scratch: cdf [m] + five rows per block of 1024 candidates; 0 = refused (never truncated)
    sizes = [lib.dpn_adaptive_scratch_doubles(m) for m in (-1, 0, 1, 1024, 1025, 32768, 1 << 20, (1 << 20) + 1)]
    assert sizes == [0, 0, 6, 1029, 1035, 32768 + 160, (1 << 20) + 5120, 0]
    # argument checks come before any launch (no device is touched here)
    buf = ctypes.c_void_p(4096)
    fac = (ctypes.c_double * 6)(*[1.0] * 6)
    sc = lambda **k_: lib.dpn_adaptive_scores(k_.get('res', buf), k_.get('m', 8), k_.get('fac', fac), k_.get('k', 1.0), k_.get('score', buf), k_.get('stats', buf),
                                              k_.get('scratch', buf), None)
    for bad in (dict(res=None), dict(fac=None), dict(score=None), dict(stats=None), dict(scratch=None), dict(m=0), dict(m=(1 << 20) + 1), dict(k=-1.0),
                dict(k=float('nan')), dict(k=float('inf'))):
        assert sc(**bad) == -1, bad

    def sel(**k_):
        g = lambda n, d=buf: k_.get(n, d)
        return lib.dpn_adaptive_select(g('score'), g('m', 8), g('k', 1.0), g('c', 1.0), g('x'), g('y'), g('t'), g('f'), g('cd'), g('n', 4), 1, 0, None, 0,
                                       g('ox'), g('oy'), g('ot'), g('of'), g('ocd'), None, None, None, g('scratch'), None)
    for bad in [dict([(p, None)]) for p in ('score', 'x', 'y', 't', 'f', 'cd', 'ox', 'oy', 'ot', 'of', 'ocd', 'scratch')] + \
               [dict(m=0), dict(m=-3), dict(m=(1 << 20) + 1), dict(n=0), dict(n=-1), dict(k=-0.5), dict(c=-1e-300), dict(k=float('nan')), dict(c=float('nan')),
                dict(k=float('inf')), dict(c=float('inf'))]:
        assert sel(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------ 2. the definition's properties
def _scores(m, seed, zeros=0.0):
    g = np.random.default_rng(seed)
    s = np.exp(3.0 * g.standard_normal(m))                    # residual-like: several decades wide
    if zeros:
        s[g.random(m) < zeros] = 0.0
    return s


def test_select_reference_properties():
    from deepphysinet_amd.adaptive import probabilities, select_reference, weights
    g = np.random.default_rng(0)
    s = _scores(5000, 1, zeros=0.3)
    u = g.random(20000)
    # k = 0: uniform weights (1 + c each), whatever the scores
    for c in (0.0, 1.0, 0.25):
        np.testing.assert_array_equal(weights(s, 0.0, c), np.full(s.size, 1.0 + c))
    idx, w, cdf = select_reference(s, u, 0.0, 0.0)
    np.testing.assert_array_equal(idx, np.minimum((u * s.size).astype(np.int64), s.size - 1))
    # c = 0: an index whose score is 0 is never returned
    for k in (1.0, 2.0, 0.5, 1.3):
        idx, w, cdf = select_reference(s, u, k, 0.0)
        assert np.all(w[s == 0.0] == 0.0) and np.all(s[idx] > 0.0)
    # all-zero scores: uniform, with c = 0 as well
    for c in (0.0, 1.0):
        np.testing.assert_array_equal(weights(np.zeros(77), 1.0, c), np.ones(77))
    idx, _, _ = select_reference(np.zeros(77), u, 2.0, 0.0)
    assert idx.min() == 0 and idx.max() == 76
    # u = 0 picks the first, u -> 1- the last index of positive weight
    z = s.copy()
    z[:3] = 0.0
    z[-5:] = 0.0
    first, last = np.flatnonzero(z > 0)[[0, -1]]
    idx, _, _ = select_reference(z, [0.0, np.nextafter(1.0, 0.0), 1.0 - 2.0 ** -30], 1.0, 0.0)
    assert idx[0] == first == 3 and idx[1] == last == z.size - 6
    idx, _, _ = select_reference(z, [0.0, np.nextafter(1.0, 0.0)], 1.0, 0.5)             # c > 0: every index has positive weight
    assert idx[0] == 0 and idx[1] == z.size - 1
    # the weights sum to m (1 + c) when the mean is positive
    for k, c in ((1.0, 1.0), (2.0, 0.0), (0.5, 0.1), (1.7, 3.0)):
        w = weights(s, k, c)
        np.testing.assert_allclose(w.sum(), s.size * (1.0 + c), rtol=s.size * 2.0 ** -52)
        np.testing.assert_allclose(probabilities(s, k, c).sum(), 1.0, rtol=s.size * 2.0 ** -52)
    # negative / non-finite scores count as 0; bad exponents are refused
    np.testing.assert_array_equal(weights([1.0, -2.0, np.nan, np.inf, 3.0], 1.0, 0.0), np.array([1.0, 0, 0, 0, 3.0]) / 0.8)
    for bad in ((-1.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            weights(s, *bad)
    with pytest.raises(ValueError):
        select_reference(s, [1.0], 1.0, 1.0)


def test_select_reference_frequencies_follow_the_weights():
    """Chi-square on 64 candidates and 2^20 uniforms: the statistic lies below the 1 - 1e-6 quantile of chi2 with 63 degrees of freedom."""
    from scipy import stats
    from deepphysinet_amd.adaptive import probabilities, select_reference
    s = _scores(64, 3)
    u = np.random.default_rng(4).random(1 << 20)
    for k, c in ((1.0, 1.0), (2.0, 0.05), (0.5, 0.1)):
        idx, _, _ = select_reference(s, u, k, c)
        want = probabilities(s, k, c) * u.size
        assert want.min() > 5.0                                       # the statistic's approximation holds
        chi2 = (((np.bincount(idx, minlength=64) - want) ** 2) / want).sum()
        assert chi2 < stats.chi2.ppf(1.0 - 1e-6, 63), (k, c, chi2)


def test_summation_order_moves_at_most_one_draw_of_4096():
    """What the GPU test asks of the kernel, asked of the reference alone first: with eps = m 2^-52 (the worst-case relative reordering error of a sum of
    m non-negative fp64 terms) at most 1 of 4096 draws from 32 768 candidates lies within eps of a boundary of the prefix sum, and a prefix sum formed
    in another order (pairwise block sums + local scans, as a parallel scan forms it) gives the same index everywhere else."""
    from deepphysinet_amd.adaptive import select_reference, weights
    m, n = 32768, 4096
    eps = m * 2.0 ** -52
    for seed, (k, c) in enumerate(((1.0, 1.0), (2.0, 0.0), (0.5, 0.1), (0.0, 0.0))):
        s = _scores(m, 10 + seed, zeros=0.1)
        u = np.random.default_rng(20 + seed).random(n)
        idx, w, cdf = select_reference(s, u, k, c)
        blocks = w.reshape(-1, 1024)
        offs = np.concatenate([[0.0], np.cumsum([b.sum() for b in blocks])[:-1]])           # np.sum: pairwise
        other = (np.cumsum(blocks, axis=1) + offs[:, None]).reshape(-1)
        target = u * cdf[-1]
        lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
        band = (target < lo * (1 + eps)) & (idx > 0) | (target > cdf[idx] * (1 - eps))
        assert band.sum() <= 1
        idx2 = np.searchsorted(other, u * other[-1], side='right')
        assert np.array_equal(idx2[~band], idx[~band])
        assert abs(other[-1] - cdf[-1]) <= eps * cdf[-1]


# ------------------------------------------------------------------------------------------------ 4. the loops' option
def _interface():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    return builder_models(**ncep_config(), precision='bf16x2')


def _stub_loop(m, monkeypatch, calls):
    monkeypatch.setattr(m, 'training_step', lambda batch, opt, **k: (calls.append(('step', batch.get('tag'))),
                                                                     (torch.tensor(1.0), {'margin_loss': torch.tensor(1.0)}, torch.tensor(0.0)))[1])

    def _optimizer(**k):
        opt = torch.optim.SGD(m.physics_net.parameters(), lr=1e-3)
        opt.sync_hyper = lambda: None
        return opt
    monkeypatch.setattr(m, 'build_optimizer', _optimizer)
    from deepphysinet_amd import encoder_ops
    monkeypatch.setattr(encoder_ops, 'check_enc_status', lambda: None)


def test_loop_option_unset_adds_no_call_and_set_needs_a_sampler(monkeypatch):
    m = _interface()
    calls = []
    _stub_loop(m, monkeypatch, calls)
    monkeypatch.setattr(m, 'adaptive_interior', lambda batch, sampler, **k: (calls.append(('adaptive', sampler, k)), dict(batch, tag='redrawn'))[1])
    batches = [{'forecast_h': torch.zeros(1, 1, 1)}] * 3
    out = m.run_train_interface(samples=batches, device='cpu', num_epoch=1, pde_start_step=0)
    assert out['global_step'] == 3 and calls == [('step', None)] * 3                     # unset: not one extra call
    assert m._adaptive_option({}) is None and m._adaptive_option({'adaptive_interior': None}) is None
    # set, but no sampler in any of the three places: an error that names them
    calls.clear()
    with pytest.raises(RuntimeError, match=r"adaptive_interior\['sampler'\].*'sampler' entry.*\.sampler"):
        m.run_train_interface(samples=batches, device='cpu', num_epoch=1, pde_start_step=0, adaptive_interior={'pool_factor': 4})
    assert calls == []
    # the three places, in order: the option's, the batch's, the source's
    class Source(list):
        sampler = 'of the source'
    src = Source(batches)
    with_entry = Source([dict(b, sampler='of the batch') for b in batches])
    for kw, want in ((dict(samples=with_entry, adaptive_interior={'sampler': 'of the option'}), 'of the option'),
                     (dict(samples=with_entry, adaptive_interior={}), 'of the batch'), (dict(samples=with_entry, adaptive_interior=True), 'of the batch'),
                     (dict(samples=src, adaptive_interior={'k': 2.0, 'c': 0.0, 'pool_factor': 16}), 'of the source')):
        calls.clear()
        m.run_train_interface(device='cpu', num_epoch=1, pde_start_step=0, **kw)
        assert [c_[0] for c_ in calls] == ['adaptive', 'step'] * 3 and all(c_[1] == want for c_ in calls[::2])
        assert all(c_ == ('step', 'redrawn') for c_ in calls[1::2])                         # the step trains on what adaptive_interior returned
    assert calls[0][2] == {'pool_factor': 16, 'k': 2.0, 'c': 0.0}
    # every = 2: steps 1 and 3; only once the PDE losses are on; the configuration is read too
    calls.clear()
    m.train_cfg['train_data']['adaptive_interior'] = {'every': 2}
    m.run_train_interface(samples=src, device='cpu', num_epoch=1, pde_start_step=0)
    assert [c_[0] for c_ in calls] == ['adaptive', 'step', 'step', 'adaptive', 'step']
    assert calls[0][2] == {'pool_factor': 8, 'k': 1.0, 'c': 1.0}
    calls.clear()
    m.run_train_interface(samples=src, device='cpu', num_epoch=1)                          # pde_start_step = 2000: no PDE losses, no redraw
    assert [c_[0] for c_ in calls] == ['step'] * 3
    with pytest.raises(ValueError, match='unknown keys'):
        m.run_train_interface(samples=src, device='cpu', num_epoch=1, adaptive_interior={'pool': 8})
    with pytest.raises(ValueError, match='every'):
        m.run_train_interface(samples=src, device='cpu', num_epoch=1, adaptive_interior={'every': 0})


def test_adaptive_calls_need_device_tensors():
    from deepphysinet_amd.sampler import CollocationSampler
    m = _interface()
    b = {'field_data': torch.zeros(1, 159, 2405), 'forecast_h': torch.zeros(1, 1, 1), 'inter_x': torch.zeros(8, 1)}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.adaptive_interior(b, sampler=None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CollocationSampler.select_weighted(None, torch.zeros(8, dtype=torch.float64), (), 4)
    assert callable(CollocationSampler.get_inter_data_adaptive)
