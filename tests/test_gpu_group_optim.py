"""GPU (MI355X): clip + Adam with parameter groups -- dpn_clip_adam_flat_groups through the C ABI and FusedClipAdam over several groups.

Kernel level: every case of tests/group_optim_cases.py runs once through the new entry point and, on copies of the same inputs, once per group
through dpn_clip_adam_flat_dev (with EMA: dpn_clip_adam_flat_ema) with that group's row as hyper_dev.  Pass conditions: p, m, v and out_norm
inside the derived bounds of optim_cases.py taken per tensor with its group's row, the shadow inside ema_cases.py's (nothing measured); every
tensor bit-identical to its group's one-group run, out_norm and the step counter too; every buffer inside guards of a sentinel bit pattern (NaN
around the read-only g), the padding of the flat buffers included.  Rows past 0 of hyper_dev carry poison where the kernel must read row 0.
"""
import ctypes

import numpy as np
import pytest
import torch

import group_optim_cases as G
import optim_cases as O
from test_gpu_ema import _EmaRun
from test_gpu_optim import _assert_guards

pytestmark = pytest.mark.gpu

_RATIOS = {}


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    print('\ngrouped optim bound ratios (largest error / bound): ' + ', '.join('%s %.3f' % (k, v) for k, v in sorted(_RATIOS.items())))


class _GroupRun(_EmaRun):
    """test_gpu_ema._EmaRun (the _dev form's guarded buffers plus a guarded shadow and ema_base) with a group per tensor and hyper_dev
    [n_groups][8].  A case without EMA passes no shadow: its buffer then has to come back untouched."""

    def __init__(self, case, inp, s0):
        shifts, sshift = G.shifts_of(case)
        decay, base, warm = case.ema if case.ema is not None else (0.0, 0, False)
        super().__init__(inp, shifts, s0 if s0 is not None else [p.copy() for p in inp.p], sshift, O.f32(decay), base)
        self.case, self.warm = case, int(warm)
        self.rows = G.hyper_rows(case)
        self.d['rows'] = torch.from_numpy(self.rows).to(_dev())
        self.group_of = (ctypes.c_uint8 * self.n)(*case.groups)
        self.args.update(rows=ctypes.c_void_p(self.d['rows'].data_ptr()), group_of=self.group_of)

    def launch_groups(self, n_tensors=None, n_groups=None, **override):
        from deepphysinet_amd import _lib
        a = dict(self.args, **override)
        ema = self.case.ema is not None
        return _lib.load().dpn_clip_adam_flat_groups(
            self.n if n_tensors is None else n_tensors, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], a['group_of'],
            self.case.n_groups if n_groups is None else n_groups, a['rows'], a['norm'], a['s'] if ema else None, a['base'] if ema else None,
            self.warm, torch.cuda.current_stream().cuda_stream)

    def launch_one_group(self, k):
        """dpn_clip_adam_flat_dev / _ema with group k's row (and row 0's max_norm, grad_scale, decay) as the one hyper_dev."""
        from deepphysinet_amd import _lib
        row = np.concatenate([self.rows[k, :5], self.rows[0, 5:]]).astype(np.float32)
        self.d['row'] = torch.from_numpy(row).to(_dev())
        a, lib, stream = self.args, _lib.load(), torch.cuda.current_stream().cuda_stream
        hyper = ctypes.c_void_p(self.d['row'].data_ptr())
        if self.case.ema is None:
            return lib.dpn_clip_adam_flat_dev(self.n, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], hyper, a['norm'], stream)
        return lib.dpn_clip_adam_flat_ema(self.n, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], hyper, a['norm'], a['s'],
                                          a['base'], self.warm, stream)


_RESULTS = {}


def _result(name):
    """(rc, state after the grouped call, {group: (rc, state after its one-group call)}): every launch made once and shared."""
    if name not in _RESULTS:
        case = G.case_by_name(name)
        inp, s0 = G.built(name)
        run = _GroupRun(case, inp, s0)
        rc = run.launch_groups()
        per = {}
        for k in sorted(set(case.groups)):
            one = _GroupRun(case, inp, s0)
            per[k] = (one.launch_one_group(k), one.fetch())
        _RESULTS[name] = (rc, run.fetch(), per)
    return _RESULTS[name]


# ---------------------------------------------------------------------------------------------- the table against fp64
@pytest.mark.parametrize('name', G.CASE_IDS)
def test_grouped_entry_point_is_inside_the_fp64_bounds(name):
    case = G.case_by_name(name)
    inp, s0 = G.built(name)
    rc, got, _ = _result(name)
    assert rc == 0 and got['step'] == case.t
    _assert_guards(got, name)
    assert all(np.isfinite(x).all() for k in 'pmv' for x in got[k]) and np.isfinite(got['norm'])      # the NaN guards and the poison reach no result
    r = G.ratios(case, got)
    if case.ema is not None:
        r['s'] = G.shadow_ratio(case, s0, got)
    else:
        assert got['untouched']['s'] and got['untouched']['base'], name
    print('%s: %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(r.items()))))
    for k, x in r.items():
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), x)
    for k in r:
        assert r[k] <= 1.0, (name, k, r)
    for i, k in enumerate(case.groups):                       # lr = 0: that group's parameters stay, its moments move
        if G.rows_of(case)[k]['lr'] == 0.0:
            assert O.bits_equal(got['p'][i], inp.p[i]) and not O.bits_equal(got['m'][i], inp.m[i])


# ---------------------------------------------------------------------------------------------- bit for bit against one group at a time
@pytest.mark.parametrize('name', G.CASE_IDS)
def test_every_tensor_equals_its_groups_one_group_run_bit_for_bit(name):
    case = G.case_by_name(name)
    rc, got, per = _result(name)
    assert rc == 0
    for k, (rc_k, one) in per.items():
        assert rc_k == 0 and one['step'] == got['step'] == case.t
        assert O.bits_equal(one['norm_bits'], got['norm_bits']), (name, k, one['norm'], got['norm'])
    for i, k in enumerate(case.groups):
        one = per[k][1]
        for q in 'pmvs' if case.ema is not None else 'pmv':
            assert O.bits_equal(got[q][i], one[q][i]), (name, q, 'tensor', i, 'group', k)


@pytest.mark.parametrize('name', [c.name for c in G.CASES if c.n_groups == 1])
def test_one_group_equals_the_entry_point_without_groups_on_every_output(name):
    rc, got, per = _result(name)
    one = per[0][1]
    assert rc == 0 and per[0][0] == 0
    for q in ('p', 'm', 'v', 's'):
        assert all(O.bits_equal(a, b) for a, b in zip(got[q], one[q])), (name, q)
    assert O.bits_equal(got['norm_bits'], one['norm_bits']) and got['step'] == one['step']
    assert got['guards'] == one['guards'] and all(got['guards'].values())


def test_two_calls_on_equal_inputs_agree_bitwise():
    name = 'list321_mixed'
    case = G.case_by_name(name)
    inp, s0 = G.built(name)
    again = _GroupRun(case, inp, s0)
    assert again.launch_groups() == 0
    a, b = _result(name)[1], again.fetch()
    for q in 'pmvs' if case.ema is not None else 'pmv':
        assert all(O.bits_equal(x, y) for x, y in zip(a[q], b[q])), q
    assert O.bits_equal(a['norm_bits'], b['norm_bits']) and a['step'] == b['step']


# ---------------------------------------------------------------------------------------------- refusals
REFUSALS = (['null_' + a for a in ('params', 'grads', 'numel', 'scratch', 'step', 'm', 'v', 'rows', 'group_of')]
            + ['n_tensors_0', 'numel_0_first', 'numel_0_last_table', 'numel_2^31_first', 'numel_2^31_last_table',
               'n_groups_0', 'n_groups_17', 'n_groups_-1', 'group_too_large_first', 'group_too_large_last_table', 'group_255'])


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('why', REFUSALS)
def test_refusal_returns_minus_one_and_writes_nothing(why, ema):
    name = 'list161_shifted' if ema else 'list161_aligned'
    case = G.case_by_name(name)
    assert (case.ema is not None) == ema and len(O.table_starts(len(case.numels), O.FLAT_TABLE)) == 2
    inp, s0 = G.built(name)
    run = _GroupRun(case, inp, s0)
    if why.startswith('null_'):
        rc = run.launch_groups(**{why[5:]: None})
    elif why == 'n_tensors_0':
        rc = run.launch_groups(n_tensors=0)
    elif why.startswith('numel'):
        numel = list(case.numels)
        numel[0 if why.endswith('first') else -1] = 0 if why.startswith('numel_0') else 2 ** 31        # a host-side value only: nothing is launched
        rc = run.launch_groups(numel=(ctypes.c_int64 * len(numel))(*numel))
    elif why.startswith('n_groups'):
        rc = run.launch_groups(n_groups=int(why.split('_')[-1]))
    else:
        groups = list(case.groups)
        groups[0 if why.endswith('first') else -1] = 255 if why == 'group_255' else case.n_groups
        rc = run.launch_groups(group_of=(ctypes.c_uint8 * len(groups))(*groups))
    got = run.fetch()
    assert rc == -1
    assert all(got['untouched'].values()) and got['guards']['g'], (why, got['untouched'])
    assert got['step'] == case.t - 1


# ---------------------------------------------------------------------------------------------- FusedClipAdam over several groups
SHAPES = [(256, 193), (7,), (1, 128, 256), (300, 17), (1,)] * 20            # test_fused_clip_adam_equals_torch's: 100 tensors
GROUP_KW = (dict(lr=1e-3, weight_decay=1e-2), dict(lr=1e-4, weight_decay=0.0, betas=(0.8, 0.99)), dict(lr=3e-3, weight_decay=1e-3, eps=1e-6))


def _grouped(params, kws=GROUP_KW):
    k = len(kws)
    return [dict(params=params[i::k], **kw) for i, kw in enumerate(kws)]


@pytest.mark.parametrize('max_norm', [1e9, 0.5], ids=['inactive', 'active'])
def test_three_groups_equal_clip_grad_norm_and_torch_adam_with_the_same_groups(max_norm):
    from deepphysinet_amd.optim import FusedClipAdam
    dev = _dev()
    torch.manual_seed(0)
    a = [torch.randn(s, device=dev).requires_grad_(True) for s in SHAPES]
    b = [t.detach().clone().requires_grad_(True) for t in a]
    ref = torch.optim.Adam(_grouped(a), lr=1e-3, weight_decay=1e-2)
    mine = FusedClipAdam(_grouped(b), lr=1e-3, weight_decay=1e-2, max_norm=max_norm)
    assert len(mine.param_groups) == 3 and tuple(mine._hyper.shape) == (3, 8)
    state = {id(p): (m, v) for p, m, v in zip(mine.params, mine.exp_avg, mine.exp_avg_sq)}
    for it in range(3):
        gs = [torch.randn_like(t) * (1 + it) for t in a]
        for t, u, g in zip(a, b, gs):
            t.grad = g.clone(); u.grad = g.clone()
        n_ref = torch.nn.utils.clip_grad_norm_(a, max_norm=max_norm)           # one norm over ALL parameters
        ref.step()
        n_mine = mine.step()
        assert abs(float(n_mine) - float(n_ref)) <= 1e-5 * float(n_ref)
        for t, u in zip(a, b):
            m, v = state[id(u)]
            assert torch.allclose(t, u, rtol=2e-5, atol=2e-7)
            assert torch.allclose(ref.state[t]['exp_avg'], m, rtol=2e-5, atol=2e-7)
            assert torch.allclose(ref.state[t]['exp_avg_sq'], v, rtol=2e-5, atol=2e-7)
    assert int(mine.step_count) == 3


def test_constructor_takes_what_it_is_given_and_refuses_the_rest():
    from deepphysinet_amd.optim import FusedClipAdam
    dev = _dev()
    ps = [torch.randn(s, device=dev).requires_grad_(True) for s in ((5,), (2049,), (16, 17), (3,))]
    opt = FusedClipAdam([dict(params=ps[:1], lr=1e-2), dict(params=ps[2:3], weight_decay=0.5)], lr=1e-3, max_norm=2.0)
    assert [id(p) for p in opt.params] == [id(ps[0]), id(ps[2])] and len(opt._slots) == 2          # ps[1], ps[3]: no slot, no moments
    assert opt.param_groups[0]['lr'] == 1e-2 and opt.param_groups[1]['lr'] == 1e-3 and opt.max_norm == 2.0
    assert ps[1] not in opt.state and ps[3] not in opt.state
    with pytest.raises(NotImplementedError, match='load_state_dict'):
        opt.add_param_group(dict(params=[ps[1]]))
    with pytest.raises(ValueError, match='max_norm'):
        FusedClipAdam([dict(params=ps[:1]), dict(params=ps[1:2], max_norm=1.0)], max_norm=2.0)
    with pytest.raises(ValueError, match='partition'):
        FusedClipAdam([dict(params=ps[:2])], layout=[ps[:3]])
    opt.max_norm = 3.0
    assert all(g['max_norm'] == 3.0 for g in opt.param_groups)
    # place_gradients: a parameter without a slot is skipped, nothing raises
    opt.place_gradients([ps[0], ps[1]], [torch.ones(5, device=dev), torch.ones(2049, device=dev)])
    assert ps[1].grad is None and torch.equal(ps[0].grad, torch.ones(5, device=dev))
    # a layout with an empty bucket: a zero-length range
    ps = [p.detach().clone().requires_grad_(True) for p in ps]                  # (fresh tensors: the arena slots of the first optimiser stay its own)
    lay = FusedClipAdam([dict(params=ps[:2], lr=1e-2), dict(params=ps[2:])], layout=[ps[:2], [], ps[2:], []])
    assert [b - a for a, b in lay.bucket_bounds] == [2048 + 4096, 0, 2 * 2048, 0] and lay.bucket_bounds[1][0] == lay.bucket_bounds[1][1] == 6144


def _params(seed=0):
    from test_gpu_ema import SHAPES as S
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(_dev()).requires_grad_(True) for s in S]


def _grads(k):
    from test_gpu_ema import SHAPES as S
    g = torch.Generator().manual_seed(100 + k)
    return [(torch.randn(*s, generator=g) * 0.1).to(_dev()) for s in S]


def _two_groups(params, **kw):
    from deepphysinet_amd.optim import FusedClipAdam
    return FusedClipAdam([dict(params=params[0::2], lr=1e-2), dict(params=params[1::2], lr=1e-3, weight_decay=0.0)], weight_decay=1e-4, max_norm=1.0, **kw)


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('sched', ['StepLR', 'CosineAnnealingLR'])
def test_scheduled_two_groups_captured_and_replayed_three_times_equal_three_eager_steps(sched, ema):
    """test_gpu_ema's capture recipe.  The scheduler scales every group's lr from its initial_lr between the replays; sync_hyper uploads all rows."""
    from deepphysinet_amd import grad_arena
    kw = dict(ema_decay=0.9999, ema_warmup=True) if ema else {}
    pa, pb = _params(1), _params(1)
    a, b = _two_groups(pa, **kw), _two_groups(pb, **kw)
    make = lambda o: (torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) if sched == 'StepLR'
                      else torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=5))
    sa, sb = make(a), make(b)
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
    lrs = []
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            a.step()
        for _ in range(3):
            sa.step(); a.sync_hyper()
            sb.step()
            lrs.append([g['lr'] for g in a.param_groups])
            graph.replay()
            b.step()
        torch.cuda.synchronize()
    finally:
        grad_arena.captured_step[0] = was
    assert len({tuple(l) for l in lrs}) == 3 and all(abs(l[0] / l[1] - 10.0) < 1e-9 for l in lrs)       # both groups moved, each from its own initial_lr
    assert torch.equal(a._hyper, b._hyper) and tuple(a._hyper.shape) == (2, 8)
    assert int(a.step_count) == int(b.step_count) == 4             # the eager step and three replays (the capture itself runs nothing)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(torch.equal(x, y) for x, y in zip(a.exp_avg, b.exp_avg)) and all(torch.equal(x, y) for x, y in zip(a.exp_avg_sq, b.exp_avg_sq))
    if ema:
        assert all(torch.equal(x, y) for x, y in zip(a.ema, b.ema)) and not any(torch.equal(s_, p) for s_, p in zip(a.ema, pa))


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
def test_state_dicts_round_trip_grouped_to_grouped_and_with_torch_adam(ema):
    kw = dict(ema_decay=0.9) if ema else {}
    pa = _params(2)
    a = _two_groups(pa, **kw)
    for k in range(2):
        for p, g in zip(pa, _grads(k)):
            p.grad = g.clone()
        a.step()
    sd = a.state_dict()
    assert len(sd['param_groups']) == 2 and [g['lr'] for g in sd['param_groups']] == [1e-2, 1e-3]
    given = [p for g in a.param_groups for p in g['params']]
    if ema:
        shadow = {id(p): s for p, s in zip(a.params, a.ema)}
        assert sd['ema_updates'] == 2 and all(torch.equal(sd['state'][i]['ema'], shadow[id(p)]) for i, p in enumerate(given))
    # grouped -> grouped
    pb = _params(3)
    b = _two_groups(pb, **kw)
    b.param_groups[0]['lr'] = 5.0
    b.load_state_dict(sd)
    assert [g['lr'] for g in b.param_groups] == [1e-2, 1e-3] and int(b.step_count) == 2 and b.max_norm == 1.0
    assert all(torch.equal(x, y) for x, y in zip(a.exp_avg, b.exp_avg)) and all(torch.equal(x, y) for x, y in zip(a.exp_avg_sq, b.exp_avg_sq))
    assert torch.equal(a._hyper, b._hyper)
    if ema:
        assert all(torch.equal(x, y) for x, y in zip(a.ema, b.ema)) and b.ema_updates() == 2
    # grouped -> torch.optim.Adam of the same groups
    pc = [p.detach().clone().requires_grad_(True) for p in pa]
    ref = torch.optim.Adam([dict(params=pc[0::2], lr=1e-2), dict(params=pc[1::2], lr=1e-3, weight_decay=0.0)], weight_decay=1e-4)
    ref.load_state_dict(sd)
    ref_given = [p for g in ref.param_groups for p in g['params']]
    assert all(torch.equal(ref.state[q]['exp_avg'], a.state[p]['exp_avg']) for p, q in zip(given, ref_given))
    assert all(float(ref.state[q]['step']) == 2.0 for q in ref_given)
    # ... one more step on both sides from the same state: the fused step follows torch's
    for p, q, g in zip(pa, pc, _grads(2)):
        p.grad = g.clone(); q.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(pc, max_norm=1.0)
    ref.step(); a.step()
    assert all(torch.allclose(p, q, rtol=2e-5, atol=2e-7) for p, q in zip(pa, pc))
    # torch.optim.Adam -> grouped: the moments arrive, max_norm comes from the defaults, the shadow restarts from the parameters
    pd = [p.detach().clone().requires_grad_(True) for p in pc]
    d = _two_groups(pd, **kw)
    plain = ref.state_dict()
    for g in plain['param_groups']:
        g.pop('max_norm', None)                                  # as a torch.optim.Adam that never saw this optimiser writes it
    d.load_state_dict(plain)
    d_given = [p for g in d.param_groups for p in g['params']]
    assert int(d.step_count) == 3 and d.max_norm == 1.0 and all(g['max_norm'] == 1.0 for g in d.param_groups)
    assert all(torch.equal(d.state[p]['exp_avg_sq'], ref.state[q]['exp_avg_sq']) for p, q in zip(d_given, ref_given))
    if ema:
        assert all(torch.equal(s, p) for s, p in zip(d.ema, d.params)) and int(d.ema_base) == 0
