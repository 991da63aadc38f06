"""GPU (MI355X): the step guard -- dpn_clip_adam_flat_guard through the C ABI, FusedClipAdam(skip_nonfinite / spike_factor), the loops' step_guard.

Kernel level: tensor lists drawn from the numels 1, 3 (the scalar tail), 2047 / 2048 / 2049 (the chunk edges) and 4100, one tensor whose p and g sit one
float off a 16-byte boundary (the misaligned scalar path), and a list of 161 one-element tensors (two update launches under one verdict).  Every
buffer is compared WHOLE, as int32 words: the windows, the padding of the flat buffers and the sentinel guards around them.  The unguarded entry
points are the reference: bit for bit, nothing is bounded or measured here.  The guard's struct is compared with guard.guard_reference run on the
fp32 norms the device wrote to out_norm.
"""
import ctypes

import numpy as np
import pytest
import torch

import guard_cases as GC
import optim_cases as O
from test_guard_cases_cpu import REFUSALS, guard_call_args

pytestmark = pytest.mark.gpu

GUARD = O.GUARD
CONFIGS = {'dev': (False, False), 'ema': (False, True), 'groups': (True, False), 'groups_ema': (True, True)}       # (several groups, EMA)
LISTS = {'small': GC.NUMELS_SMALL + (257,), 'list161': GC.NUMELS_161}
MISALIGNED = {'small': 6, 'list161': None}           # the tensor of the list whose p and g are one float off


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _lib():
    from deepphysinet_amd import _lib
    return _lib.load()


def _ptr(t, floats=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


class _State:
    """Everything one call reads and writes, on the device: p and g in an arena each (GUARD sentinel floats around every window), m, v and the shadow as
    flat buffers inside guards, scratch, the step counter, out_norm, ema_base, hyper rows [n_groups][8] and the DpnStepGuard struct."""

    def __init__(self, list_name, config, seed=0, step=0, base=3):
        self.numels = LISTS[list_name]
        self.grouped, self.ema = CONFIGS[config]
        n = self.n = len(self.numels)
        rng = np.random.default_rng([seed, n])
        self.off, cur = [], 0
        for i, k in enumerate(self.numels):
            self.off.append(cur + GUARD + (1 if i == MISALIGNED[list_name] else 0))
            cur += GUARD + 4 + ((k + 3) // 4) * 4
        self.arena = cur + GUARD
        self.foff = O.flat_offsets(self.numels)
        flat = O.flat_floats(self.numels) + 2 * GUARD
        host = {k: np.full(self.arena, O.SENTINEL, np.float32) for k in 'PG'}
        host.update({k: np.full(flat, O.SENTINEL, np.float32) for k in 'MVS'})
        self.g0 = []
        for i, k in enumerate(self.numels):
            p = rng.standard_normal(k).astype(np.float32)
            g = (0.1 * rng.standard_normal(k)).astype(np.float32)
            self.g0.append(g)
            host['P'][self.off[i]:self.off[i] + k] = p
            host['G'][self.off[i]:self.off[i] + k] = g
            o = GUARD + self.foff[i]
            host['M'][o:o + k] = (0.01 * rng.standard_normal(k)).astype(np.float32)
            host['V'][o:o + k] = (1e-3 * rng.random(k)).astype(np.float32)
            host['S'][o:o + k] = p + (0.01 * rng.standard_normal(k)).astype(np.float32)
        dev = _dev()
        self.d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        self.n_groups = 3 if self.grouped else 1
        self.groups = [i % 3 for i in range(n)] if self.grouped else [0] * n
        rows = np.array([[1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, 1.0, 0.9], [1e-2, 0.8, 0.99, 1e-6, 0.0, 7.0, 9.0, 0.1],
                         [3e-4, 0.5, 0.9, 1e-3, 1e-3, 7.0, 9.0, 0.1]], np.float32)[:self.n_groups]      # rows past 0: other max_norm, grad_scale, decay
        self.d.update(hyper=torch.from_numpy(rows).to(dev), scratch=torch.zeros(O.scratch_doubles(self.numels), dtype=torch.float64, device=dev),
                      step=torch.full((1,), step, dtype=torch.int32, device=dev), norm=torch.zeros(1, dtype=torch.float32, device=dev),
                      base=torch.full((1,), base, dtype=torch.int32, device=dev), guard=torch.zeros(5, dtype=torch.int64, device=dev))
        self._pointers()

    def _pointers(self):
        self.params = (ctypes.c_void_p * self.n)(*[self.d['P'].data_ptr() + 4 * o for o in self.off])
        self.grads = (ctypes.c_void_p * self.n)(*[self.d['G'].data_ptr() + 4 * o for o in self.off])
        self.numel = (ctypes.c_int64 * self.n)(*self.numels)
        self.group_of = (ctypes.c_uint8 * self.n)(*self.groups)

    def clone(self, step_delta=0):
        other = object.__new__(_State)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != 'd'})
        other.d = {k: v.clone() for k, v in self.d.items()}
        other.d['step'] += step_delta
        other._pointers()
        return other

    def set_gradients(self, scale=1.0, seed=None, plant=None):
        """The gradients of a call: the base gradients (seed: fresh ones) times `scale`; plant = (tensor, element, value)."""
        rng = None if seed is None else np.random.default_rng([77, seed, self.n])
        full = np.full(self.arena, O.SENTINEL, np.float32)
        for i, k in enumerate(self.numels):
            g = self.g0[i] if rng is None else (0.1 * rng.standard_normal(k)).astype(np.float32)
            full[self.off[i]:self.off[i] + k] = g * np.float32(scale)
        if plant is not None:
            ti, e, value = plant
            full[self.off[ti] + (e if e >= 0 else self.numels[ti] + e)] = value
        self.d['G'].copy_(torch.from_numpy(full))

    def args(self):
        d = self.d
        return dict(n=self.n, params=self.params, grads=self.grads, numel=list(self.numels), m=_ptr(d['M'], GUARD), v=_ptr(d['V'], GUARD),
                    scratch=_ptr(d['scratch']), step=_ptr(d['step']), group_of=list(self.groups) if self.grouped else None, n_groups=self.n_groups,
                    hyper=_ptr(d['hyper']), norm=_ptr(d['norm']), s=_ptr(d['S'], GUARD) if self.ema else None, base=_ptr(d['base']) if self.ema else None,
                    warm=1, guard=_ptr(d['guard']))

    def guarded(self, factor=0.0, decay=0.99, warmup=1, patience=1):
        a = self.args()
        return _lib().dpn_clip_adam_flat_guard(a['n'], a['params'], a['grads'], self.numel, a['m'], a['v'], a['scratch'], a['step'],
                                               self.group_of if self.grouped else None, a['n_groups'], a['hyper'], a['norm'], a['s'], a['base'], 1,
                                               a['guard'], factor, decay, warmup, patience, torch.cuda.current_stream().cuda_stream)

    def unguarded(self):
        """The entry point FusedClipAdam runs for this configuration without the guard."""
        a, lib, stream = self.args(), _lib(), torch.cuda.current_stream().cuda_stream
        head = (a['n'], a['params'], a['grads'], self.numel, a['m'], a['v'], a['scratch'], a['step'])
        if self.grouped:
            return lib.dpn_clip_adam_flat_groups(*head, self.group_of, a['n_groups'], a['hyper'], a['norm'], a['s'], a['base'], 1, stream)
        if self.ema:
            return lib.dpn_clip_adam_flat_ema(*head, a['hyper'], a['norm'], a['s'], a['base'], 1, stream)
        return lib.dpn_clip_adam_flat_dev(*head, a['hyper'], a['norm'], stream)

    def words(self):
        """Every buffer whole, as int32 words."""
        torch.cuda.synchronize()
        out = {k: self.d[k].cpu().numpy().view(np.int32).copy() for k in ('P', 'M', 'V', 'S', 'G', 'norm', 'base')}
        out['step'] = int(self.d['step'])
        return out

    def norm(self):
        return self.d['norm'].cpu().numpy()[0]

    def struct(self):
        from deepphysinet_amd.guard import FIELDS
        raw = self.d['guard'].cpu().numpy()
        out = {k: int(raw.view(np.int32)[i]) for i, k in enumerate(FIELDS[:6])}
        out.update(running=raw.view(np.float64)[3], last=raw.view(np.float64)[4])
        return out


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


STATE = ('P', 'M', 'V', 'S')


# ---------------------------------------------------------------------------------------------- 1. finite gradients
@pytest.mark.parametrize('list_name', sorted(LISTS))
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_finite_gradients_three_calls_equal_the_unguarded_entry_bit_for_bit(config, list_name):
    from deepphysinet_amd import guard as G
    a = _State(list_name, config, seed=1, step=4)
    b = a.clone()
    norms = []
    for k in range(3):
        a.set_gradients(seed=k)
        b.set_gradients(seed=k)
        assert a.guarded(factor=1e6, warmup=1, patience=2) == 0 and b.unguarded() == 0
        wa, wb = a.words(), b.words()
        _same(wa, wb, STATE + ('norm', 'G', 'base'), (config, list_name, k))
        assert wa['step'] == wb['step'] == 5 + k
        norms.append(a.norm())
        st = a.struct()
        assert st['verdict'] == 0 and st['skipped_nonfinite'] == st['skipped_spike'] == 0 and st['seen'] == k + 1
    _, ref = G.guard_reference(norms, 1e6, 0.99, 1, 2)
    assert G.state_equal(a.struct(), ref[-1]), (a.struct(), ref[-1])
    if not CONFIGS[config][1]:
        assert np.array_equal(wa['S'], _State(list_name, config, seed=1).words()['S'])         # no EMA: the shadow's buffer is not touched


# ---------------------------------------------------------------------------------------------- 2. a planted non-finite element
PLACES = {'first': ('small', 0, 0), 'last': ('small', 6, -1), 'tail': ('small', 4, 2048), 'second_launch': ('list161', 160, 0)}
PLANTED = [(v, p) for v in ('nan', 'inf', '-inf') for p in sorted(PLACES)]


@pytest.mark.parametrize('value,place', PLANTED, ids=['%s_%s' % vp for vp in PLANTED])
def test_planted_non_finite_element_skips_the_call_and_the_next_one_counts_without_it(value, place):
    from deepphysinet_amd import guard as G
    list_name, ti, e = PLACES[place]
    config = sorted(CONFIGS)[PLANTED.index((value, place)) % 4]
    a = _State(list_name, config, seed=2, step=6)
    a.set_gradients(seed=0, plant=(ti, e, float(value)))
    before = a.words()
    assert a.guarded() == 0
    after = a.words()
    _same(before, after, STATE + ('G', 'base'), (value, place, config))                        # every byte of p, m, v and the shadow as it was
    assert after['step'] == before['step'] + 1 and not np.isfinite(a.norm())
    st = a.struct()
    verdicts, ref = G.guard_reference([a.norm()], 0.0, 0.99, 1, 1)
    assert verdicts == [1] and all(st[k] == ref[0][k] for k in G.INT_FIELDS) and st['skipped_nonfinite'] == 1 and st['verdict'] == 1
    assert np.isnan(st['last']) == np.isnan(a.norm()) and (np.isnan(st['last']) or st['last'] == np.float64(a.norm()))
    # the next call, finite: the unguarded entry from the same state with its step counter one lower (te = t + base follows: the same ema_base)
    a.set_gradients(seed=1)
    b = a.clone(step_delta=-1)
    assert a.guarded() == 0 and b.unguarded() == 0
    wa, wb = a.words(), b.words()
    _same(wa, wb, STATE + ('norm',), (value, place, config, 'next'))
    assert wa['step'] == wb['step'] + 1 == before['step'] + 2
    assert not np.array_equal(wa['P'], after['P']) and a.struct()['verdict'] == 0 and a.struct()['seen'] == 1
    if CONFIGS[config][1]:
        assert not np.array_equal(wa['S'], after['S'])


# ---------------------------------------------------------------------------------------------- 3. finite overflow
def test_a_finite_gradient_whose_square_overflows_is_skipped_as_non_finite():
    a = _State('small', 'ema', seed=3)
    a.set_gradients(plant=(3, 100, GC.FINITE_OVERFLOW))
    before = a.words()
    assert a.guarded() == 0
    _same(before, a.words(), STATE, 'overflow')
    assert np.isposinf(a.norm()) and a.struct()['verdict'] == 1 and a.struct()['skipped_nonfinite'] == 1 and a.words()['step'] == 1


# ---------------------------------------------------------------------------------------------- 4. the scripted scale sequence
def test_scripted_scale_sequence_follows_guard_reference_bit_for_bit():
    from deepphysinet_amd import guard as G
    a = _State('small', 'groups_ema', seed=4)
    s = GC.SCRIPT
    ref_state, skipped = G.zero_state(), 0
    got_verdicts = []
    for k, scale in enumerate(GC.SCRIPT_SCALES):
        a.set_gradients(scale=scale)
        b = a.clone(step_delta=-skipped)
        before = a.words()
        assert a.guarded(s['spike_factor'], s['spike_decay'], s['spike_warmup'], s['spike_patience']) == 0
        wa = a.words()
        verdict, ref_state = G.guard_step(ref_state, a.norm(), s['spike_factor'], s['spike_decay'], s['spike_warmup'], s['spike_patience'])
        st = a.struct()
        assert G.state_equal(st, ref_state), (k, st, ref_state)
        got_verdicts.append(st['verdict'])
        assert wa['step'] == k + 1 and G.effective_step(k + 1, st) == k + 1 - st['skipped_spike']
        if verdict == 0:
            assert b.unguarded() == 0
            _same(wa, b.words(), STATE + ('norm',), ('applied', k))
        else:
            _same(wa, before, STATE, ('skipped', k))
            skipped += 1
    assert tuple(got_verdicts) == GC.SCRIPT_VERDICTS


# ---------------------------------------------------------------------------------------------- 8. rejected arguments
@pytest.mark.parametrize('why', REFUSALS)
def test_refusal_returns_minus_one_and_writes_nothing(why):
    a = _State('list161', 'groups_ema', seed=5, step=9)
    before = a.words()
    scratch = a.d['scratch'].clone()
    args = dict(a.args(), factor=10.0, decay=0.99, warmup=3, patience=2)
    rc = _lib().dpn_clip_adam_flat_guard(*guard_call_args(why, args)[:-1], torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    after = a.words()
    _same(before, after, STATE + ('G', 'norm', 'base'), why)
    assert after['step'] == 9 and torch.equal(scratch, a.d['scratch']) and not a.d['guard'].any()


# ---------------------------------------------------------------------------------------------- FusedClipAdam
SHAPES = [(3,), (2049,), (16, 17), (1,), (4100,)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(_dev()).requires_grad_(True) for s in SHAPES]


def _grads(k):
    g = torch.Generator().manual_seed(100 + k)
    return [(torch.randn(*s, generator=g) * 0.1).to(_dev()) for s in SHAPES]


def _opt(params, grouped=False, **kw):
    from deepphysinet_amd.optim import FusedClipAdam
    groups = [dict(params=params[0::2], lr=1e-2), dict(params=params[1::2], lr=1e-3, weight_decay=0.0)] if grouped else params
    return FusedClipAdam(groups, lr=1e-2, weight_decay=1e-4, max_norm=1.0, **kw)


def _equal_state(a, b, ema=True):
    ok = all(torch.equal(x, y) for x, y in zip(a.params, b.params))
    ok = ok and all(torch.equal(x, y) for x, y in zip(a.exp_avg, b.exp_avg)) and all(torch.equal(x, y) for x, y in zip(a.exp_avg_sq, b.exp_avg_sq))
    return ok and (not ema or all(torch.equal(x, y) for x, y in zip(a.ema, b.ema)))


# ---------------------------------------------------------------------------------------------- 5. graph capture
@pytest.mark.parametrize('grouped', [False, True], ids=['one_group', 'two_groups'])
def test_captured_step_skips_and_applies_between_replays(grouped):
    """One capture, a linear chain of three launches.  Replays: finite, NaN planted in the flat gradients, NaN taken out, finite again."""
    from deepphysinet_amd import grad_arena
    pa, pb = _params(1), _params(1)
    a = _opt(pa, grouped, ema_decay=0.9, skip_nonfinite=True)
    b = _opt(pb, grouped, ema_decay=0.9)
    for p, q, g in zip(pa, pb, _grads(0)):
        p.grad = g.clone(); q.grad = g.clone()
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
        flat = a.flat_gradients()
        graph.replay(); b.step()
        torch.cuda.synchronize()
        assert _equal_state(a, b)
        kept = flat[1].clone()
        flat[1] = float('nan')                                 # (an element of the first tensor; the padding behind it is never read)
        held = [x.clone() for x in list(a.params) + list(a.exp_avg) + list(a.exp_avg_sq) + list(a.ema)]
        graph.replay()                                         # skipped: b takes no step
        torch.cuda.synchronize()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(held, list(a.params) + list(a.exp_avg) + list(a.exp_avg_sq) + list(a.ema)))
        assert a.guard_stats()['verdict'] == 1 and not np.isfinite(float(a.grad_norm))
        flat[1] = kept
        graph.replay(); b.step()
        graph.replay(); b.step()
        torch.cuda.synchronize()
    finally:
        grad_arena.captured_step[0] = was
    assert _equal_state(a, b)
    st = a.guard_stats()
    assert st['skipped_nonfinite'] == 1 and st['skipped_spike'] == 0 and st['verdict'] == 0 and st['seen'] == 4
    assert int(a.step_count) == 5 and int(b.step_count) == 4 and a.effective_step() == 4 and a.ema_updates() == b.ema_updates() == 4
    assert torch.equal(a.grad_norm, b.grad_norm) and a.state[pa[0]]['step'] is a.step_count


# ---------------------------------------------------------------------------------------------- 7. state dict round trip
def test_state_dict_round_trip_in_mid_sequence_and_old_state_dicts():
    s = GC.SCRIPT
    pa = _params(2)
    a = _opt(pa, True, ema_decay=0.9, **s)
    for k, scale in enumerate(GC.SCRIPT_SCALES[:7]):           # ends on a spike: consecutive = 1, two calls skipped so far
        for p, g in zip(pa, _grads(0)):
            p.grad = g * scale
        a.step()
    st = a.guard_stats()
    assert st['skipped_spike'] == 2 and st['consecutive'] == 1 and st['verdict'] == 2 and a.effective_step() == 5 and int(a.step_count) == 7
    sd = a.state_dict()
    assert sd['step_guard'] == dict(s, state=st) and sd['ema_updates'] == 5
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    b = _opt(pb, True, ema_decay=0.9, **s)
    b.load_state_dict(sd)
    assert b.guard_stats() == st and int(b.step_count) == 7 and b.effective_step() == 5 and b.ema_updates() == 5
    for k, scale in enumerate(GC.SCRIPT_SCALES[7:]):           # both go on: a spike, the overruling call, an applied one
        for p, q, g in zip(pa, pb, _grads(0)):
            p.grad = g * scale; q.grad = g * scale
        a.step(); b.step()
    assert _equal_state(a, b) and a.guard_stats() == b.guard_stats() and a.guard_stats()['skipped_spike'] == 3
    # a state dict from before the guard: a zeroed guard, every call so far counts as applied
    old = {k: v for k, v in sd.items() if k != 'step_guard'}
    pc = [p.detach().clone().requires_grad_(True) for p in pa]
    c = _opt(pc, True, ema_decay=0.9, **s)
    c._load_guard(st)
    c.load_state_dict(old)
    zero = c.guard_stats()
    assert all(v == 0 for v in zero.values()) and int(c.step_count) == 7 and c.effective_step() == 7
    # a state dict with the guard into an optimiser built without: ignored, with a warning
    pd = [p.detach().clone().requires_grad_(True) for p in pa]
    d = _opt(pd, True, ema_decay=0.9)
    with pytest.warns(UserWarning, match='step guard'):
        d.load_state_dict(sd)
    assert d.step_guard is None and int(d.step_count) == 7 and d.ema_updates() == 5 and all(torch.equal(x, y) for x, y in zip(d.exp_avg, c.exp_avg))
    with pytest.raises(RuntimeError, match='skip_nonfinite'):
        d.guard_stats()


# ---------------------------------------------------------------------------------------------- 9. without the option
ENTRIES = ('dpn_clip_adam_flat_dev', 'dpn_clip_adam_flat_ema', 'dpn_clip_adam_flat_groups', 'dpn_clip_adam_flat_guard')


class _Spy:
    def __init__(self):
        self.lib = _lib()
        self.inner = {k: getattr(self.lib, k) for k in ENTRIES}
        self.calls = []

    def __enter__(self):
        for k in ENTRIES:
            setattr(self.lib, k, (lambda name: lambda *a: (self.calls.append(name), self.inner[name](*a))[1])(k))
        return self

    def __exit__(self, *exc):
        for k in ENTRIES:
            setattr(self.lib, k, self.inner[k])


def test_without_the_option_the_new_entry_is_never_called():
    want = {(False, None): 'dpn_clip_adam_flat_dev', (False, 0.9): 'dpn_clip_adam_flat_ema', (True, None): 'dpn_clip_adam_flat_groups',
            (True, 0.9): 'dpn_clip_adam_flat_groups'}
    for (grouped, ema), entry in want.items():
        for kw in ({}, dict(skip_nonfinite=False, spike_factor=None), dict(spike_factor=0.0)):
            ps = _params(3)
            opt = _opt(ps, grouped, ema_decay=ema, **kw)
            assert opt.step_guard is None and opt._guard is None
            with _Spy() as spy:
                for k in range(2):
                    for p, g in zip(ps, _grads(k)):
                        p.grad = g
                    opt.step()
            assert spy.calls == [entry] * 2, (grouped, ema, kw, spy.calls)
            assert opt.effective_step() == 2 and 'step_guard' not in opt.state_dict()
    ps = _params(3)
    opt = _opt(ps, False, skip_nonfinite=True)
    with _Spy() as spy:
        for p, g in zip(ps, _grads(0)):
            p.grad = g
        opt.step()
    assert spy.calls == ['dpn_clip_adam_flat_guard']
    assert _opt(_params(3), spike_factor=10.0).step_guard.as_dict() == dict(spike_factor=10.0, spike_decay=0.99, spike_warmup=100, spike_patience=5)
    with pytest.raises(ValueError, match='step guard'):
        _opt(_params(3), spike_factor=10.0, spike_patience=0)


# ---------------------------------------------------------------------------------------------- 6. a poisoned sample leaves no trace
def _model():
    from test_gpu_adaptive import _model as make
    return make()


_SAMPLES = {}


def _samples():
    """Fixed batches (dicts of tensors, no sampler): the tile unit, 128 interior + 256 margin points.  bad = sample 0 with one NaN label."""
    if not _SAMPLES:
        from deepphysinet_amd.sampler import SyntheticSamples
        src = SyntheticSamples(_dev(), n_margin=256, n_inter=128, leads=5, seed=3)
        good = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in src[i].items()} for i in range(5)]
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in good[0].items()}
        bad['margin_data'].view(-1)[7] = float('nan')
        _SAMPLES.update(good=good, bad=bad)
    return _SAMPLES['good'], _SAMPLES['bad']


def _train(samples, **kw):
    m = _model()
    out = m.run_train_interface(samples=samples, num_epoch=1, device=str(_dev()), ema_weights=0.9, **kw)
    opt = out['optimizer']
    torch.cuda.synchronize()
    return m, opt


@pytest.mark.parametrize('mode', ['data_loss', 'pde_from_step_0', 'lead_batch'])
def test_a_poisoned_sample_leaves_no_trace(mode):
    good, bad = _samples()
    kw = dict(data_loss={}, pde_from_step_0=dict(pde_start_step=0), lead_batch=dict(pde_start_step=0, lead_batch=2))[mode]
    if mode == 'lead_batch':                                    # one poisoned sample in a group of two: the whole step is skipped
        with_bad, without = [good[0], good[1], bad, good[3], good[2], good[4]], [good[0], good[1], good[2], good[4]]
    else:
        with_bad, without = [good[0], bad, good[2]], [good[0], good[2]]
    ma, a = _train(with_bad, step_guard=True, **kw)
    mb, b = _train(without, **kw)
    st = a.guard_stats()
    assert st['skipped_nonfinite'] == 1 and st['skipped_spike'] == 0 and int(a.step_count) == 3 and int(b.step_count) == 2
    assert a.effective_step() == 2 and a.ema_updates() == b.ema_updates() == 2
    assert _equal_state(a, b), mode
    for (k, x), (_, y) in zip(ma.physics_net.named_parameters(), mb.physics_net.named_parameters()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and bool(torch.isfinite(x).all()), k
    if mode == 'data_loss':
        # the behaviour being replaced: the same three samples without the guard end with non-finite parameters (passes before and after)
        from deepphysinet_amd import encoder_ops
        mc = _model()
        try:
            mc.run_train_interface(samples=with_bad, num_epoch=1, device=str(_dev()), ema_weights=0.9, **kw)
        except RuntimeError as err:                             # the epoch's encoder status check may notice the damage: too late, it is done
            assert 'non-finite' in str(err)
        finally:
            torch.cuda.synchronize()
            encoder_ops.reset_enc_status()                      # (the status word is sticky and shared: the tests behind this one start clean)
        assert not all(bool(torch.isfinite(p).all()) for p in mc.physics_net.parameters())


def test_loop_logs_the_counters_and_raises_when_every_step_is_skipped(tmp_path):
    import json
    from deepphysinet_amd.sampler import SyntheticSamples
    good, bad = _samples()
    val = SyntheticSamples(_dev(), n_margin=256, n_inter=128, leads=1, seed=1)
    m = _model()
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    out = m.run_train_interface(samples=[good[0], bad, good[2]], valid_samples=val, log_path=str(tmp_path), num_epoch=1, device=str(_dev()),
                                step_guard=dict(spike_factor=1e3, spike_warmup=1))
    rows = [json.loads(l) for l in open(tmp_path / 'metrics.jsonl')]
    train = [r for r in rows if r['event'] == 'training']
    assert [(r['skipped_nonfinite'], r['skipped_spike']) for r in train] == [(0, 0), (1, 0)] and all(r['running_norm'] > 0 for r in train)
    assert out['optimizer'].step_guard.spike_factor == 1e3
    m2 = _model()
    m2.train_cfg.setdefault('log', {})['log_step'] = 2
    with pytest.raises(RuntimeError, match=r'all 2 optimiser steps.*skipped_nonfinite 2'):
        m2.run_train_interface(samples=[good[0], bad, bad, good[2]], num_epoch=1, device=str(_dev()), step_guard=True)
