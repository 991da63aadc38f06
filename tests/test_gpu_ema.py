"""GPU (MI355X): the weight EMA fused into clip + Adam -- dpn_clip_adam_flat_ema and dpn_ema_swap through the C ABI, FusedClipAdam(ema_decay=...),
ema_weights(), and the loops' `ema_weights` option with train.py --ema / infer.py --ema.

Kernel level: every case of tests/ema_cases.py runs dpn_clip_adam_flat_ema and dpn_clip_adam_flat_dev on copies of the same inputs.  p, m, v,
out_norm and the step counter must have the same bits; the shadow must lie inside the derived bound of ema_cases.py against the fp64 recursion on
the kernel's own p' (nothing measured); decay 0 leaves the shadow bit-equal to p'.  Every buffer sits inside guards of a sentinel bit pattern (NaN
around the read-only g), the padding of the flat buffers included.  Each case is launched once and shared by the tests that read it.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_cases as E
import optim_cases as O
from test_gpu_optim import STEP_GUARD, _Run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dpn_clip_adam_flat_ema', 'dpn_ema_swap')
_RATIO = [0.0]                    # largest |s - s'| / bound over everything this module ran: printed, never asserted


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report_ratio():
    yield
    print('\nema bound ratio (largest |s - s\'| / bound): %.3f' % _RATIO[0])


def _shadow_arena(values, numels, sshift, fill=O.SENTINEL):
    """The shadow as the entry points take it: optim_cases.flat_arena's layout (window i at chunk_start[i] * 2048, SENTINEL in the padding and
    the guards), the whole buffer `sshift` floats off a 16-byte boundary.  The ABI's pointer is the buffer's base + GUARD + sshift floats."""
    a = O.Arena.__new__(O.Arena)
    a.offsets = [O.GUARD + sshift + o for o in O.flat_offsets(numels)]
    a.numels = list(numels)
    total = O.flat_floats(numels) + 2 * O.GUARD + 4
    a.full = np.full(total, fill, np.float32)
    a.inside = np.zeros(total, bool)
    for o, x in zip(a.offsets, values):
        a.full[o:o + len(x)] = x
        a.inside[o:o + len(x)] = True
    return a


class _EmaRun(_Run):
    """test_gpu_optim._Run in the _dev form plus the shadow (its own guarded flat buffer), the decay in hyper[7] and ema_base inside guards."""

    def __init__(self, inp, shifts, s0, sshift, decay, base, null_base=False):
        super().__init__(inp, shifts, 'dev')
        dev = _dev()
        self.S = _shadow_arena(s0, inp.numels, sshift)
        self.sshift, self.warm = sshift, 0
        self.base0 = np.full(9, STEP_GUARD, np.int32)
        self.base0[4] = base
        self.d.update(S=torch.from_numpy(self.S.full).to(dev), base=torch.from_numpy(self.base0).to(dev),
                      hyper=torch.tensor(self.hyper + [inp.gs, decay], dtype=torch.float32, device=dev))
        assert self.d['S'].data_ptr() % 16 == 0
        self.args.update(hyper=ctypes.c_void_p(self.d['hyper'].data_ptr()), s=ctypes.c_void_p(self.d['S'].data_ptr() + 4 * (O.GUARD + sshift)),
                         base=None if null_base else ctypes.c_void_p(self.d['base'].data_ptr() + 16))

    def launch(self, n_tensors=None, warmup=None, **override):
        from deepphysinet_amd import _lib
        lib = _lib.load()
        a = dict(self.args, **override)
        n = self.n if n_tensors is None else n_tensors
        return lib.dpn_clip_adam_flat_ema(n, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], a['hyper'], a['norm'],
                                          a['s'], a['base'], int(self.warm if warmup is None else warmup), torch.cuda.current_stream().cuda_stream)

    def swap(self, n_tensors=None, **override):
        from deepphysinet_amd import _lib
        a = dict(self.args, **override)
        return _lib.load().dpn_ema_swap(self.n if n_tensors is None else n_tensors, a['params'], a['numel'], a['s'], torch.cuda.current_stream().cuda_stream)

    def fetch(self):
        out = super().fetch()
        S, base = self.d['S'].cpu().numpy(), self.d['base'].cpu().numpy()
        out['s'] = [w.copy() for w in self.S.windows(S)]
        out['guards'].update(s=self.S.outside_kept(S), base=bool((base == self.base0).all()))
        out['untouched'].update(s=O.bits_equal(S, self.S.full), base=bool((base == self.base0).all()))
        return out


_RESULTS = {}


def _null_base(case):
    return case.base == 0 and case.t in (1, 10)           # a null ema_base_dev means 0: half of the base-0 cases pass none


def _result(name):
    """(rc and state after dpn_clip_adam_flat_ema, rc and state after dpn_clip_adam_flat_dev on copies of the same inputs): launched once."""
    if name not in _RESULTS:
        case = E.case_by_name(name)
        inp, s0 = E.built(name)
        shifts, sshift = E.shifts_of(case)
        run = _EmaRun(inp, shifts, s0, sshift, O.f32(case.decay), case.base, null_base=_null_base(case))
        run.warm = int(case.warmup)
        plain = _Run(inp, shifts, 'dev')
        rc, rc_plain = run.launch(), plain.launch()
        _RESULTS[name] = (rc, run.fetch(), rc_plain, plain.fetch())
    return _RESULTS[name]


# ---------------------------------------------------------------------------------------------- dpn_clip_adam_flat_ema
@pytest.mark.parametrize('name', E.CASE_IDS)
def test_ema_entry_point_equals_the_plain_step_and_keeps_the_shadow_inside_its_bound(name):
    case = E.case_by_name(name)
    inp, s0 = E.built(name)
    rc, got, rc_plain, plain = _result(name)
    assert rc == 0 and rc_plain == 0
    assert got['step'] == plain['step'] == case.t
    for k in 'pmv':                                           # the Adam side: the same bits as the entry point without EMA
        for i, (x, y) in enumerate(zip(got[k], plain[k])):
            assert O.bits_equal(x, y), (name, k, 'tensor', i)
    assert O.bits_equal(got['norm_bits'], plain['norm_bits']), (name, got['norm'], plain['norm'])
    for k, kept in got['guards'].items():
        assert kept, '%s: a store outside the windows of %s (or into the read-only gradients / ema_base)' % (name, k)
    # the NaN guards around g reach no result
    assert all(np.isfinite(x).all() for k in 'pmvs' for x in got[k]) and np.isfinite(got['norm'])
    args = (case.decay, case.t, case.base, case.warmup)
    r = E.ratio(got['s'], E.reference(s0, got['p'], *args), E.bound(s0, got['p'], *args))
    print('%s: |s - s\'| / bound %.3f' % (name, r))
    _RATIO[0] = max(_RATIO[0], r)
    assert r <= 1.0, (name, r)
    if case.decay == 0.0:
        assert all(O.bits_equal(s, p) for s, p in zip(got['s'], got['p'])), name


def _refusals():
    args = ('params', 'grads', 'numel', 'scratch', 'step', 'm', 'v', 'hyper', 's')
    return ['null_' + a for a in args] + ['n_tensors_0', 'numel_0_first', 'numel_0_last_table', 'numel_2^31_first', 'numel_2^31_last_table']


@pytest.mark.parametrize('why', _refusals())
def test_ema_refusal_returns_minus_one_and_writes_nothing(why):
    name = 'list161_aligned'
    case = E.case_by_name(name)
    inp, s0 = E.built(name)
    shifts, sshift = E.shifts_of(case)
    run = _EmaRun(inp, shifts, s0, sshift, O.f32(0.9), 5)
    if why.startswith('null_'):
        rc = run.launch(warmup=1, **{why[5:]: None})
    elif why == 'n_tensors_0':
        rc = run.launch(n_tensors=0, warmup=1)
    else:
        numel = list(case.numels)
        assert len(O.table_starts(len(numel), O.FLAT_TABLE)) == 2
        numel[0 if why.endswith('first') else -1] = 0 if why.startswith('numel_0') else 2 ** 31        # a host-side value only: nothing is launched
        rc = run.launch(warmup=1, numel=(ctypes.c_int64 * len(numel))(*numel))
    got = run.fetch()
    assert rc == -1
    assert all(got['untouched'].values()) and got['guards']['g'], (why, got['untouched'])
    assert got['step'] == case.t - 1


# ---------------------------------------------------------------------------------------------- dpn_ema_swap
SWAP_CASES = [c.name for c in E.CASES if not c.name.startswith('combo_')]
ODD_BITS = np.array([0x80000000, 0x7FC01234, 0xFF800000, 0x00000001], np.uint32).view(np.float32)     # -0, a NaN with a payload, -inf, a denormal


@pytest.mark.parametrize('name', SWAP_CASES)
def test_swap_exchanges_the_bits_and_twice_is_the_identity(name):
    case = E.case_by_name(name)
    inp, s0 = E.built(name)
    p = [x.copy() for x in inp.p]
    k = min(len(p[0]), 4)
    p[0][:k] = ODD_BITS[:k]                                   # moved as bits, not as numbers
    shifts, sshift = E.shifts_of(case)
    run = _EmaRun(O.Inputs(inp.numels, p, inp.g, inp.m, inp.v, inp.hyper, inp.gs, inp.t), shifts, s0, sshift, 0.0, 0)
    assert run.swap() == 0
    once = run.fetch()
    assert all(O.bits_equal(a, b) for a, b in zip(once['p'], s0)) and all(O.bits_equal(a, b) for a, b in zip(once['s'], p)), name
    assert once['guards']['p'] and once['guards']['s'] and all(once['untouched'][k] for k in ('m', 'v', 'scratch', 'step', 'norm', 'base')), name
    assert run.swap() == 0
    twice = run.fetch()
    assert twice['untouched']['p'] and twice['untouched']['s'], name


@pytest.mark.parametrize('why', ['null_params', 'null_numel', 'null_s', 'n_tensors_0', 'numel_0_last_table', 'numel_2^31_first'])
def test_swap_refusal_returns_minus_one_and_writes_nothing(why):
    name = 'list161_shifted'
    case = E.case_by_name(name)
    inp, s0 = E.built(name)
    shifts, sshift = E.shifts_of(case)
    run = _EmaRun(inp, shifts, s0, sshift, 0.0, 0)
    if why.startswith('null_'):
        rc = run.swap(**{why[5:]: None})
    elif why == 'n_tensors_0':
        rc = run.swap(n_tensors=0)
    else:
        numel = list(case.numels)
        numel[0 if why.endswith('first') else -1] = 0 if why.startswith('numel_0') else 2 ** 31
        rc = run.swap(numel=(ctypes.c_int64 * len(numel))(*numel))
    got = run.fetch()
    assert rc == -1 and all(got['untouched'].values())


# ---------------------------------------------------------------------------------------------- FusedClipAdam
SHAPES = ((5,), (2049,), (16, 17), (3,), (4096,), (7, 3))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(_dev()).requires_grad_(True) for s in SHAPES]


def _grads(k):
    g = torch.Generator().manual_seed(100 + k)
    return [(torch.randn(*s, generator=g) * 0.1).to(_dev()) for s in SHAPES]


def _opt(params, **kw):
    from deepphysinet_amd.optim import FusedClipAdam
    return FusedClipAdam(params, lr=1e-2, weight_decay=1e-4, max_norm=1.0, **kw)


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.clone()


def _np(ts):
    return [t.detach().cpu().numpy().reshape(-1).copy() for t in ts]


def test_three_steps_equal_the_plain_optimiser_and_the_shadow_follows_the_fp64_recursion():
    pa, pb = _params(), _params()
    a, b = _opt(pa, ema_decay=0.9, ema_warmup=False), _opt(pb)
    assert a._hyper_values()[7] == 0.9 and b._hyper_values()[7] == 0.0
    assert 'ema_decay' not in a.param_groups[0] and set(a.state_dict()['param_groups'][0]) == set(b.state_dict()['param_groups'][0])
    assert a.ema_base.dtype == torch.int32 and a.ema_base.shape == (1,) and a.ema_base.is_cuda and b.ema is None
    assert all(torch.equal(s, p) for s, p in zip(a.ema, pa))                  # filled with the parameters at construction
    d = O.f32(0.9)
    s64 = [x.astype(np.float64) for x in _np(pa)]
    bounds = []
    for k in range(3):
        s_before = _np(a.ema)
        _set_grads(pa, _grads(k)); _set_grads(pb, _grads(k))
        na, nb = a.step(), b.step()
        torch.cuda.synchronize()
        assert torch.equal(na, nb)
        assert all(torch.equal(x, y) for x, y in zip(pa, pb))
        assert all(torch.equal(x, y) for x, y in zip(a.exp_avg, b.exp_avg)) and all(torch.equal(x, y) for x, y in zip(a.exp_avg_sq, b.exp_avg_sq))
        p_new = _np(pa)
        s64 = [d * s + (1.0 - d) * p.astype(np.float64) for s, p in zip(s64, p_new)]
        bounds.append(E.bound(s_before, p_new, 0.9, k + 1, 0, False))
        # one step against the recursion from the kernel's own previous shadow: the one-step bound
        assert E.ratio(_np(a.ema), E.reference(s_before, p_new, 0.9, k + 1, 0, False), bounds[-1]) <= 1.0, k
    total = E.propagated_bound(bounds, [d] * 3)
    r = E.ratio(_np(a.ema), s64, total)
    print('three steps: |s - s64| / propagated bound %.3f' % r)
    assert r <= 1.0
    assert int(a.step_count) == 3 and a.ema_updates() == 3
    pad = a._ema_flat.clone()
    for o, p in zip(a._offsets, a.params):
        pad[o:o + p.numel()] = 0
    assert not pad.any()                                       # the padding of the shadow stays zero
    for bad in (1.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            _opt(_params(), ema_decay=bad)
    with pytest.raises(RuntimeError):
        b.ema_weights().__enter__()
    a.reset_ema()
    assert all(torch.equal(s, p) for s, p in zip(a.ema, pa)) and a.ema_updates() == 3


def test_captured_step_replayed_three_times_equals_three_eager_steps():
    from deepphysinet_amd import grad_arena
    pa, pb = _params(1), _params(1)
    a, b = _opt(pa, ema_decay=0.9999, ema_warmup=True), _opt(pb, ema_decay=0.9999, ema_warmup=True)
    _set_grads(pa, _grads(0)); _set_grads(pb, _grads(0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.step()                                               # the eager step in front of the capture
    torch.cuda.current_stream().wait_stream(s)
    b.step()
    torch.cuda.synchronize()
    was = grad_arena.captured_step[0]
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            a.step()
            with pytest.raises(RuntimeError, match='capture'):
                a.ema_weights().__enter__()
        for _ in range(3):
            graph.replay()
            b.step()
        torch.cuda.synchronize()
    finally:
        grad_arena.captured_step[0] = was
    assert int(a.step_count) == int(b.step_count) == 4
    assert all(torch.equal(x, y) for x, y in zip(pa, pb)) and all(torch.equal(x, y) for x, y in zip(a.ema, b.ema))
    assert not any(torch.equal(s_, p) for s_, p in zip(a.ema, pa))           # the warm-up decays 2/11 .. 5/14 moved the shadow, not onto p


def test_state_dict_round_trips_with_and_without_ema_on_either_side():
    pa = _params(2)
    a = _opt(pa, ema_decay=0.9)
    a.ema_base.fill_(5)
    for k in range(2):
        _set_grads(pa, _grads(k))
        a.step()
    sd = a.state_dict()
    assert sd['ema_updates'] == 7 and all('ema' in st for st in sd['state'].values())
    assert all(torch.equal(sd['state'][i]['ema'], s) for i, s in enumerate(a.ema))       # (no layout: given order = kernel order)
    # EMA -> EMA: the shadow and the update count come back
    pb = _params(3)
    b = _opt(pb, ema_decay=0.9)
    b.load_state_dict(sd)
    assert all(torch.equal(x, y) for x, y in zip(a.ema, b.ema)) and int(b.step_count) == 2 and int(b.ema_base) == 5 and b.ema_updates() == 7
    assert all(torch.equal(x, y) for x, y in zip(a.exp_avg, b.exp_avg))
    assert set(b.state[pb[0]]) == {'step', 'exp_avg', 'exp_avg_sq'}
    # EMA -> no EMA: today's optimiser loads it and keeps today's keys
    pc = _params(3)
    c = _opt(pc)
    c.load_state_dict(sd)
    assert int(c.step_count) == 2 and all(torch.equal(x, y) for x, y in zip(a.exp_avg_sq, c.exp_avg_sq))
    plain = c.state_dict()
    assert 'ema_updates' not in plain and all(set(st) == {'step', 'exp_avg', 'exp_avg_sq'} for st in plain['state'].values())
    # no EMA -> EMA: the shadow becomes the current parameters, base 0
    pd = _params(4)
    d = _opt(pd, ema_decay=0.5)
    d.ema_base.fill_(9)
    d.ema[0].zero_()
    d.load_state_dict(plain)
    assert all(torch.equal(s, p) for s, p in zip(d.ema, pd)) and int(d.ema_base) == 0 and int(d.step_count) == 2
    # a torch.optim.Adam state dict still loads, on both kinds
    ref_p = [p.detach().clone().requires_grad_(True) for p in pd]
    ref = torch.optim.Adam(ref_p, lr=1e-2, weight_decay=1e-4)
    _set_grads(ref_p, _grads(0))
    ref.step()
    for opt, ps in ((d, pd), (c, pc)):
        opt.load_state_dict(ref.state_dict())
        assert int(opt.step_count) == 1 and opt.max_norm == 1.0
        assert all(torch.equal(m, ref.state[q]['exp_avg']) for m, q in zip(opt.exp_avg, ref_p))
    assert all(torch.equal(s, p) for s, p in zip(d.ema, pd)) and int(d.ema_base) == 0


# ---------------------------------------------------------------------------------------------- ema_weights() on the model
def _model():
    from test_gpu_adaptive import _model as make
    return make('scaled')


def _bits(params):
    return [p.detach().clone().view(torch.int32) for p in params]


def test_ema_weights_validates_on_the_shadow_and_restores_the_parameters():
    from deepphysinet_amd import grad_arena
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model()
    src = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=3, seed=0)
    opt = m.build_optimizer(lr=1e-3, ema_decay=0.9, ema_warmup=False)
    for k in range(2):
        m.training_step(src[k], opt, with_pde=True)
    vb = src[2]
    params = list(m.physics_net.parameters())
    raw_bits = _bits(params)
    before = m.validation_step(vb)
    epoch = grad_arena.param_epoch[0]
    with opt.ema_weights() as inner:
        assert inner is opt and grad_arena.param_epoch[0] == epoch + 1
        inside = m.validation_step(vb)
        with pytest.raises(RuntimeError, match='nest'):
            opt.ema_weights().__enter__()
        with pytest.raises(RuntimeError, match='ema_weights'):
            opt.step()
    assert grad_arena.param_epoch[0] == epoch + 2
    after = m.validation_step(vb)
    assert all(torch.equal(a, b) for a, b in zip(_bits(params), raw_bits))
    assert torch.equal(after['stats'], before['stats']) and torch.equal(after['valid_loss'], before['valid_loss'])
    # a second model that carries the shadow as its weights: same kernels, same weights, same bits
    sd = opt.ema_state_dict(m.physics_net)
    own = m.physics_net.state_dict()
    assert list(sd) == list(own) and all(sd[k].shape == own[k].shape and sd[k].data_ptr() != own[k].data_ptr() for k in sd)
    m2 = _model()
    m2.physics_net.load_state_dict(sd, strict=True)
    ref = m2.validation_step(vb)
    assert torch.equal(inside['stats'], ref['stats']) and torch.equal(inside['valid_loss'], ref['valid_loss'])
    assert torch.equal(inside['terms'], ref['terms'])
    assert not torch.equal(inside['stats'], before['stats'])
    # load_ema: strict on the names, and the update count becomes the base
    opt2 = m2.build_optimizer(ema_decay=0.9)
    opt2.load_ema(sd, 12)
    assert all(torch.equal(a, b) for a, b in zip(opt2.ema_state_dict(m2.physics_net).values(), sd.values())) and int(opt2.ema_base) == 12
    first = next(iter(dict(m2.physics_net.named_parameters())))
    with pytest.raises(KeyError):
        opt2.load_ema({k: v for k, v in sd.items() if k != first}, 0)


# ---------------------------------------------------------------------------------------------- the loops
class _Spy:
    """Counts calls of the two new entry points of the loaded library."""

    def __init__(self):
        from deepphysinet_amd import _lib
        self.lib = _lib.load()
        self.inner = {k: getattr(self.lib, k) for k in NEW}
        self.calls = []

    def __enter__(self):
        for k in NEW:
            setattr(self.lib, k, (lambda name: lambda *a: (self.calls.append(name), self.inner[name](*a))[1])(k))
        return self

    def __exit__(self, *exc):
        for k in NEW:
            setattr(self.lib, k, self.inner[k])


def _loop(tmp_path, **kw):
    from deepphysinet_amd.sampler import SyntheticSamples
    m = _model()
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    src = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=4, seed=0)
    val = SyntheticSamples(_dev(), n_margin=256, n_inter=256, leads=2, seed=1)
    out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path / 'log'), checkpoint_path=str(tmp_path / 'ck'), max_steps=3,
                                num_epoch=1, pde_start_step=1, log_step=2, validate_every_epoch=True, **kw)
    events = [json.loads(l) for l in open(tmp_path / 'log' / 'metrics.jsonl')]
    ck = torch.load(tmp_path / 'ck' / 'physics_latest.pth', map_location='cpu')
    return m, out, events, ck


def test_loop_validates_and_checkpoints_on_the_ema_and_resumes_it(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.model.physics_net import PhysicsNet
    with _Spy() as spy:
        m, out, events, ck = _loop(tmp_path, ema_weights=0.9)
    assert out['global_step'] == 3
    # three steps; two log-step validations and the epoch's, a swap in and a swap out each
    assert spy.calls.count('dpn_clip_adam_flat_ema') == 3 and spy.calls.count('dpn_ema_swap') == 6
    valid = [e for e in events if e['event'] in ('validation', 'validation_epoch')]
    assert [e['event'] for e in valid] == ['validation', 'validation', 'validation_epoch'] and all(e['weights'] == 'ema' for e in valid)
    assert all('weights' not in e for e in events if e['event'] == 'training')
    assert ck['ema'] == dict(decay=0.9, warmup=True, updates=3)
    cfg = ncep_config()
    fresh = PhysicsNet(cfg['meta_cfg'], cfg['net_cfg'])
    fresh.load_state_dict(ck['model_ema'], strict=True)
    assert list(ck['model_ema']) == list(ck['model'])
    assert any(not torch.equal(ck['model_ema'][k], ck['model'][k]) for k in ck['model'])
    opt = out['optimizer']
    live = opt.ema_state_dict(m.physics_net)
    assert all(torch.equal(live[k].cpu(), ck['model_ema'][k]) for k in live)
    # a resumed run (the epoch is complete: no step is taken) starts from the saved shadow and the saved update count
    m2 = _model()
    out2 = m2.run_train_interface(samples=[], checkpoint_path=str(tmp_path / 'ck'), num_epoch=1, ema_weights=0.9)
    opt2 = out2['optimizer']
    assert int(opt2.ema_base) == 3 and int(opt2.step_count) == 0 and opt2.ema_updates() == 3
    again = opt2.ema_state_dict(m2.physics_net)
    assert all(torch.equal(again[k].cpu(), ck['model_ema'][k]) for k in again)
    assert any(not torch.equal(again[k], v) for k, v in m2.physics_net.state_dict().items())       # not overwritten by the raw weights


def test_loop_with_lead_batches_keeps_the_ema(tmp_path):
    with _Spy() as spy:
        m, out, events, ck = _loop(tmp_path, ema_weights=dict(decay=0.9, warmup=False), lead_batch=2)
    assert out['global_step'] == 2                           # four samples, two per optimiser step
    assert spy.calls.count('dpn_clip_adam_flat_ema') == 2
    assert ck['ema'] == dict(decay=0.9, warmup=False, updates=2) and 'model_ema' in ck
    assert all(e['weights'] == 'ema' for e in events if e['event'].startswith('validation'))


def test_loop_without_the_option_is_the_loop_of_before(tmp_path):
    with _Spy() as spy:
        m, out, events, ck = _loop(tmp_path)
    assert spy.calls == []
    assert 'model_ema' not in ck and 'ema' not in ck
    assert all('weights' not in e for e in events)
    assert out['optimizer'].ema is None and 'ema_updates' not in out['optimizer'].state_dict()


def test_train_py_ema_then_infer_py_ema_in_child_processes(tmp_path):
    cfg = tmp_path / 'cfg.py'
    cfg.write_text('from deepphysinet_amd.configs import ncep_config\nconfig = ncep_config()\n'
                   "config['train_cfg']['train_data'].update(label_batch_size=256, batch_size_inter=256)\n"
                   "config.setdefault('inference_cfg', {})['dt'] = 21600\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    ck = str(tmp_path / 'ck')
    run = lambda *a: subprocess.run([sys.executable, *a], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    r = run(os.path.join(ROOT, 'train.py'), '--config_file', str(cfg), '--synthetic', '--ema', '0.9', '--max_steps', '2', '--checkpoint_path', ck)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    saved = torch.load(os.path.join(ck, 'physics_latest.pth'), map_location='cpu')
    assert saved['ema'] == dict(decay=0.9, warmup=True, updates=2) and 'model_ema' in saved
    r = run(os.path.join(ROOT, 'infer.py'), '--config_file', str(cfg), '--checkpoint_path', ck, '--synthetic', '--ema')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'finite True' in r.stdout
    # a checkpoint without the averaged weights: the named error
    bare = tmp_path / 'bare'
    bare.mkdir()
    torch.save({k: v for k, v in saved.items() if k not in ('model_ema', 'ema')}, bare / 'physics_latest.pth')
    r = run(os.path.join(ROOT, 'infer.py'), '--config_file', str(cfg), '--checkpoint_path', str(bare), '--synthetic', '--ema')
    assert r.returncode != 0 and 'KeyError' in r.stderr and 'model_ema' in r.stderr and str(bare) in r.stderr, r.stderr[-2000:]
