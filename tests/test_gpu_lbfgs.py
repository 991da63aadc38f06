"""GPU (MI355X): L-BFGS on the flat buffers -- the kernels of csrc/dpn_lbfgs.inc through the C ABI against their numpy restatements
(deepphysinet_amd/lbfgs.py) bit for bit on the case table of tests/lbfgs_cases.py, FusedLBFGS.step in lockstep with lbfgs_reference,
InterfacePhysics.loss_and_gradients against the training steps, and the loops' `lbfgs` option.

Yardsticks: the restatements (whole buffers as 32-bit words, guards and flat padding included; fp64 results by their bits), and for the Gram pass
also math.fsum of the fp64 products with the bound 2 N 2^-53 sum |a_i| |b_i| (fp64 accumulation of exact products, N the vector length)."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import lbfgs_cases as LC
from test_lbfgs_cpu import refusal_calls

pytestmark = pytest.mark.gpu

GUARD = 64                      # sentinel floats on either side of every window
SENTINEL = np.float32(-7.25e11)
PAD = np.float32(3.5e-7)        # what the flat padding holds before a kernel runs


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def LB():
    from deepphysinet_amd import lbfgs
    return lbfgs


def words(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


class Rig:
    """The buffers of one tensor list on the device, every window between sentinel guards, and their numpy twins."""

    def __init__(self, tl, m):
        lb = LB()
        self.tl, self.m, self.lay = tl, m, lb.Layout(tl.numels)
        self.n, total = len(tl.numels), self.lay.total
        # the parameters: one arena, tensor i in a window of its own; the misaligned one starts one float past a 16-byte boundary
        self.p_off, off = [], GUARD
        for i, n in enumerate(tl.numels):
            off = -(-off // 4) * 4 + (1 if i == tl.misaligned else 0)
            self.p_off.append(off)
            off += n + GUARD
        self.arena = torch.full((off,), float(SENTINEL), dtype=torch.float32, device=_dev())
        assert self.arena.data_ptr() % 16 == 0
        self.params = [self.arena[o:o + n] for o, n in zip(self.p_off, tl.numels)]
        if tl.misaligned is not None:
            assert self.params[tl.misaligned].data_ptr() % 16 == 4
        self.flat = {}
        for name, count, dtype in (('x0', total, torch.float32), ('d', total, torch.float32), ('g', total, torch.float32), ('gp', total, torch.float32),
                                   ('S', m * total, torch.float32), ('Y', m * total, torch.float32),
                                   ('scratch', (3 * (2 * m + 1) + 2) * self.lay.chunks, torch.float64), ('G', (2 * m + 1) ** 2, torch.float64),
                                   ('delta', 2 * m + 1, torch.float64), ('out', 1, torch.float64), ('state', 9, torch.int64)):
            fill = {torch.float32: float(PAD), torch.float64: -1.5, torch.int64: 0}[dtype]
            full = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=_dev())
            full[:GUARD] = full[-GUARD:] = 77
            self.flat[name] = (full, full[GUARD:GUARD + count])
        self.numel = (ctypes.c_int64 * self.n)(*tl.numels)
        self.pp = (ctypes.c_void_p * self.n)(*[p.data_ptr() for p in self.params])

    def __getitem__(self, k):
        return self.flat[k][1]

    def ptr(self, k):
        return ctypes.c_void_p(self[k].data_ptr())

    def args(self):
        """The dict test_lbfgs_cpu.refusal_calls builds its argument lists from."""
        return dict(n=self.n, params=self.pp, numel=self.numel, m=self.m, **{k: self.ptr(k) for k in self.flat})

    def call(self, entry, *names, **scalars):
        from deepphysinet_amd import _lib
        a = dict(self.args(), **scalars)
        code = getattr(_lib.load(), entry)(a['n'], a['params'], a['numel'], *[a[k] for k in names], torch.cuda.current_stream().cuda_stream)
        assert code == 0, entry

    def upload(self, k, tensors):
        """A tensor list into the flat buffer k: the padding keeps what it held."""
        for o, n, t in zip(self.lay.offsets, self.lay.numels, tensors):
            self[k][o:o + n] = torch.from_numpy(np.ascontiguousarray(t)).to(_dev())

    def set_params(self, tensors):
        for p, t in zip(self.params, tensors):
            p.copy_(torch.from_numpy(np.ascontiguousarray(t)).to(_dev()))

    def host(self, k):
        return self[k].cpu().numpy().copy()

    def state(self):
        raw = self['state'].cpu().numpy()
        lb = LB()
        out = {k: int(raw.view(np.int32)[i]) for i, k in enumerate(lb.INT_FIELDS)}
        out.update({k: float(raw.view(np.float64)[3 + i]) for i, k in enumerate(lb.FIELDS[6:])})
        return out

    def snapshot(self):
        torch.cuda.synchronize()
        return [words(self.arena).copy()] + [words(full).copy() for full, _ in self.flat.values()]

    def guards_intact(self):
        a = self.arena.cpu().numpy()
        inside = np.zeros(a.size, bool)
        for o, n in zip(self.p_off, self.tl.numels):
            inside[o:o + n] = True
        assert np.all(a[~inside] == SENTINEL)
        for name, (full, _) in self.flat.items():
            f = full.cpu().numpy()
            assert np.all(f[:GUARD] == 77) and np.all(f[-GUARD:] == 77), name


def same_state(a, b, keys):
    for k in keys:
        if k in LB().INT_FIELDS:
            assert int(a[k]) == int(b[k]), (k, a[k], b[k])
        else:
            assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), (k, a[k], b[k])


# ---------------------------------------------------------------------------------------------- every push sequence of the table
@pytest.mark.parametrize('name,m,pairs,bad', LC.SEQUENCES, ids=LC.SEQUENCE_IDS)
def test_kernels_follow_their_restatements_bit_for_bit(name, m, pairs, bad):
    lb = LB()
    tl = LC.tensor_list(name)
    rig = Rig(tl, m)
    lay, B = rig.lay, 2 * m + 1
    seq = LC.push_sequence(tl.numels, m, pairs, 100 * m + pairs, bad)
    x_start = LC.vectors(tl.numels, 7, 1)[0]
    rig.set_params(x_start)
    rig.upload('g', seq[0].g)
    rig['gp'].copy_(rig['g'])
    # numpy twins, the padding holding what the device's holds
    S, Y = rig.host('S').reshape(m, -1), rig.host('Y').reshape(m, -1)
    g_prev, d_np, st, G = rig.host('gp'), rig.host('d'), lb.zero_state(), np.zeros((B, B))
    fsum_checked = 0
    for k in range(pairs + 1):
        p = seq[k]
        if k > 0:
            # ---- save, move, move(0), push
            rig.call('dpn_lbfgs_save', 'x0')
            x0 = lay.pack(x_start, fill=PAD)
            assert np.array_equal(words(rig['x0']), words(x0))
            rig.upload('d', p.d)
            rig.upload('g', p.g)
            d_np, g = rig.host('d'), rig.host('g')
            rig.call('dpn_lbfgs_move', 'x0', 'd', 't', t=ctypes.c_float(p.t))
            moved = lay.unpack(lb.move(x0, d_np, np.float32(p.t)))
            for got, want in zip(rig.params, moved):
                assert np.array_equal(words(got), words(want))
            if k % 2 == 0:                              # the restore after a trial: every parameter word
                rig.call('dpn_lbfgs_move', 'x0', 'd', 't', t=ctypes.c_float(0.0))
                for got, want in zip(rig.params, x_start):
                    assert np.array_equal(words(got), words(want))
            else:
                x_start = moved
            rig.call('dpn_lbfgs_push', 'g', 'gp', 'd', 't', 'S', 'Y', 'm', 'state', t=ctypes.c_float(p.t))
            st = lb.push(g, g_prev, d_np, np.float32(p.t), S, Y, st, m, lay.mask)
            assert np.array_equal(words(rig['S']), words(S.reshape(-1))) and np.array_equal(words(rig['Y']), words(Y.reshape(-1)))
            assert np.array_equal(words(rig['gp']), words(g_prev))
            same_state(rig.state(), st, ('count', 'newest', 'pending', 'skipped'))
        else:
            g = rig.host('g')
        # ---- the Gram pass and its reduce
        rig['scratch'].fill_(-1.5)
        rig.call('dpn_lbfgs_gram', 'S', 'Y', 'g', 'm', 'state', 'scratch', 'G')
        part = lb.gram_partials(S, Y, g, lay, m, st)
        got_part = rig.host('scratch').reshape(3 * B + 2, lay.chunks)
        written = ~np.isnan(part)
        assert np.array_equal(words(got_part[written]), words(part[written]))
        assert np.all(got_part[~written] == -1.5)                        # a slot without a pair: nothing written
        G, st = lb.gram_reduce(part, G, m, st)
        G_dev = rig.host('G').reshape(B, B)
        order = lb.basis_order(st, m)
        for a in order:
            for b in order:
                assert G_dev[a, b].view(np.uint64) == G[a, b].view(np.uint64), (k, a, b)
        same_state(rig.state(), st, ('g_l1', 'g_inf', 'gg'))
        if k in (0, pairs):                             # the exact reference, on the rows this pass wrote
            vec = lambda b_: g if b_ == 2 * m else (S[b_] if b_ < m else Y[b_ - m])
            N = sum(tl.numels)
            rows = (st['newest'], m + st['newest'], 2 * m) if st['count'] else (2 * m,)
            for a in rows:
                for b in order:
                    x, y = vec(a)[lay.mask].astype(np.float64), vec(b)[lay.mask].astype(np.float64)
                    exact = math.fsum((x * y).tolist())
                    assert abs(G_dev[a, b] - exact) <= 2 * N * 2.0 ** -53 * math.fsum(np.abs(x * y).tolist()), (k, a, b)
                    fsum_checked += 1
        # ---- the coefficient launch fed the device's own G, the direction pass fed the device's delta
        before = rig.state()
        rig.call('dpn_lbfgs_direction', 'S', 'Y', 'g', 'm', 'state', 'G', 'delta', 'd')
        delta, st = lb.coefficients(G_dev, before, m)
        same_state(rig.state(), st, lb.FIELDS)
        delta_dev = rig.host('delta')
        order = lb.basis_order(st, m)
        assert np.array_equal(words(delta_dev[order]), words(delta[order]))
        vecs = [g if b == 2 * m else (S[b] if b < m else Y[b - m]) for b in order]
        d_np = np.where(lay.mask, lb.direction(vecs, delta_dev[order]), d_np)
        assert np.array_equal(words(rig['d']), words(d_np))
        if st['count'] == 0:
            assert np.array_equal(words(d_np[lay.mask]), words(-g[lay.mask]))
        # ---- the line search's inner product
        rig.call('dpn_lbfgs_gtd', 'g', 'd', 'scratch', 'out')
        assert np.float64(rig.host('out')[0]).view(np.uint64) == np.float64(lb.gtd_reference(g, d_np, lay)).view(np.uint64)
        # (the one-element list: a pair of magnitude 1e-6 has s.y under the threshold by itself, so its skips are the restatement's to say)
        if bad is not None and k == bad + 1:            # the refused pair: the ring pointer stepped back (in a full ring the overwritten slot is lost)
            assert st['skipped'] == 1 and st['count'] == min(k, m) - 1
        elif bad is None and name != 'one':
            assert st['count'] == min(k, m)
    assert st['iters'] == pairs + 1 and fsum_checked > 0 and (name == 'one' or st['skipped'] == (0 if bad is None else 1))
    rig.guards_intact()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_return_minus_one_and_touch_nothing():
    from deepphysinet_amd import _lib
    rig = Rig(LC.tensor_list('small'), 3)
    rig.set_params(LC.vectors(rig.tl.numels, 3, 1)[0])
    before = rig.snapshot()
    calls = refusal_calls(rig.args())
    assert len(calls) > 60
    for why, (entry, args) in calls.items():
        assert getattr(_lib.load(), entry)(*args[:-1], torch.cuda.current_stream().cuda_stream) == -1, why
    after = rig.snapshot()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---------------------------------------------------------------------------------------------- FusedLBFGS in lockstep with the reference
def _small_params(scale=1.0, seed=5):
    tl = LC.tensor_list('small')
    rng = np.random.default_rng(seed)
    x0 = [(scale * rng.standard_normal(n)).astype(np.float32) for n in tl.numels]
    curv = [np.exp(rng.uniform(0.0, math.log(100.0), n)).astype(np.float32) for n in tl.numels]      # a diagonal quadratic, cond 100
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(_dev())) for x in x0]
    return x0, curv, params


def test_step_runs_in_lockstep_with_the_fp32_reference():
    """The closure is eager torch: f = 0.5 sum a x^2, whose autograd gradient is fl(a x) exactly (0.5 fl(a x) + 0.5 fl(x a)).  The reference is fed the
    recorded losses and the numpy gradient fl(a x): parameters at every evaluation, and the `last` dict, must be identical."""
    lb = LB()
    x0, curv, params = _small_params()
    a_dev = [torch.from_numpy(c).to(_dev()) for c in curv]
    opt = lb.FusedLBFGS(params, history_size=3, max_iter=10, max_eval=1000)
    seen = []

    def closure():
        opt.zero_grad()
        loss = sum(0.5 * ((a * p) * p).sum() for a, p in zip(a_dev, params))
        loss.backward()
        seen.append(([p.detach().cpu().numpy().copy() for p in params], float(loss.detach())))
        return loss
    count0 = int(opt.step_count)
    first = opt.step(closure)
    assert int(opt.step_count) == count0 + 1 and first == seen[0][1] == opt.last['f0']
    ref_seen = []

    def fun(x):
        k = len(ref_seen)
        ref_seen.append([t.copy() for t in x])
        assert k < len(seen), 'the reference evaluates more often than the device run did'
        return seen[k][1], [c * t for c, t in zip(curv, x)]
    x, last = lb.lbfgs_reference(fun, x0, history_size=3, max_iter=10, max_eval=1000, dtype=np.float32)
    assert len(ref_seen) == len(seen) and last == opt.last, (last, opt.last)
    for k, (mine, theirs) in enumerate(zip(ref_seen, seen)):
        for a, b in zip(mine, theirs[0]):
            assert np.array_equal(words(a), words(b)), k
    for a, p in zip(x, params):
        assert np.array_equal(words(a), words(p))
    assert last['iters'] == 10 and last['f'] < last['f0'] and opt.lbfgs_state()['count'] == 3         # the ring has wrapped
    # state_dict carries the options and counters, not the history; a loaded optimiser starts with an empty ring
    sd = opt.state_dict()
    assert sd['lbfgs']['step_count'] == 1 and sd['param_groups'][0]['history_size'] == 3 and not sd['state']
    from deepphysinet_amd import grad_arena
    grad_arena.unregister(opt)
    opt2 = lb.FusedLBFGS(params, history_size=3, max_iter=2)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]['max_iter'] == 10 and int(opt2.step_count) == 1 and opt2.lbfgs_state()['count'] == 0


def test_closure_that_is_infinite_beyond_a_radius_and_a_forced_failure():
    lb = LB()
    x0, curv, params = _small_params(scale=0.05)
    a_dev = [torch.from_numpy(c).to(_dev()) for c in curv]
    radius = 1.05 * math.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in x0))

    def make(always_inf_after_first):
        calls = [0]

        def closure():
            opt.zero_grad()
            loss = sum(0.5 * ((a * (p - 1.0)) * (p - 1.0)).sum() for a, p in zip(a_dev, params))      # the minimum lies outside the radius
            loss.backward()
            calls[0] += 1
            r = math.sqrt(sum(float((p.detach().double() ** 2).sum()) for p in params))
            if r > radius or (always_inf_after_first and calls[0] > 1):
                return loss.detach() * float('inf')
            return loss
        return closure
    opt = lb.FusedLBFGS(params, history_size=3, max_iter=4, history='keep')
    opt.step(make(False))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert opt.last['status'] != 'ls_failed' and opt.last['f'] < opt.last['f0'] and math.isfinite(opt.last['f'])
    assert math.sqrt(sum(float((p.detach().double() ** 2).sum()) for p in params)) <= radius
    # every trial infinite: the parameters come back word for word, the history is empty
    start = [words(p).copy() for p in params]
    assert opt.lbfgs_state()['count'] > 0
    opt.step(make(True))
    assert opt.last['status'] == 'ls_failed' and opt.last['t'] == 0.0 and opt.last['iters'] == 0
    assert all(np.array_equal(words(p), s) for p, s in zip(params, start))
    assert opt.lbfgs_state()['count'] == 0
    with pytest.raises(RuntimeError, match='closure'):
        opt.step()


def test_a_fused_lbfgs_replaces_an_unregistered_adam_without_a_warning():
    import warnings
    from deepphysinet_amd import grad_arena
    from deepphysinet_amd.optim import FusedClipAdam
    _, _, params = _small_params()
    adam = FusedClipAdam(params)
    grad_arena.unregister(adam)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        opt = LB().FusedLBFGS(params)
    assert grad_arena.slot_of(params[0]).data_ptr() == opt.flat_gradients().data_ptr()
    opt.zero_grad()


# ---------------------------------------------------------------------------------------------- the real net
def _model():
    from test_gpu_adaptive import _model as make
    return make('scaled')


def _samples(leads, seed=3):
    from deepphysinet_amd.sampler import SyntheticSamples
    return SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=leads, seed=seed)


def test_loss_and_gradients_leaves_what_the_training_steps_leave():
    src = _samples(2)
    for batch, step in ((src[0], 'training_step'), ([src[0], src[1]], 'training_step_batch')):
        a, b = _model(), _model()
        opt_a, opt_b = a.build_optimizer(), b.build_optimizer()
        loss_a = getattr(a, step)(batch, opt_a, with_pde=True)[0]
        loss_b, parts = b.loss_and_gradients(batch, opt_b, with_pde=True)
        assert torch.equal(loss_a, loss_b) and set(parts) == {'margin_loss', 'inter_pde_loss', 'margin_pde_loss'}
        assert np.array_equal(words(opt_a.flat_gradients()), words(opt_b.flat_gradients())), step
        assert float(opt_b.flat_gradients().abs().max()) > 0.0 and int(opt_b.step_count) == 0
        # the same into a FusedLBFGS's arena, once Adam has let go of it
        from deepphysinet_amd import grad_arena
        grad_arena.unregister(opt_b)
        opt_b.zero_grad()
        lb = LB().FusedLBFGS(list(b.physics_net.parameters()))
        loss_c, _ = b.loss_and_gradients(batch, lb, with_pde=True)
        assert torch.equal(loss_c, loss_b)
        by_param = {id(p): s for p, s in zip(opt_b.params, opt_b._slots)}
        lb.gather_gradients()
        assert all(torch.equal(p.grad, by_param[id(p)]) for p in lb.params)


def test_three_iterations_on_the_real_net_with_a_frozen_encoder():
    m = _model()
    frozen = m.freeze(['meta_net.*'])
    start = {k: v.detach().clone() for k, v in m.physics_net.state_dict().items()}
    batch = _samples(1)[0]
    opt = LB().FusedLBFGS([p for p in m.physics_net.parameters() if p.requires_grad], max_iter=3, max_eval=40, history_size=3)
    opt.step(lambda: m.loss_and_gradients(batch, opt, with_pde=True)[0])
    last = opt.last
    print('real net: %s' % (last,))
    assert last['f'] <= last['f0'] and math.isfinite(last['f']) and 1 <= last['evals']
    assert last['iters'] == 3 or last['status'] not in ('max_iter', 'max_eval')
    assert int(opt.step_count) == 1
    now = m.physics_net.state_dict()
    assert all(np.array_equal(words(now[k]), words(start[k])) for k in frozen)
    assert all(bool(torch.isfinite(p).all()) for p in m.physics_net.parameters())
    if last['iters'] > 0:
        assert any(not torch.equal(now[k], start[k]) for k in now if k not in frozen)


def test_loop_switches_to_lbfgs_at_the_configured_epoch(tmp_path):
    from deepphysinet_amd.lbfgs import FusedLBFGS
    m = _model()
    src, val = _samples(2, seed=0), _samples(1, seed=1)
    out = m.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path / 'log'), checkpoint_path=str(tmp_path / 'ck'), num_epoch=2,
                                pde_start_step=1, lbfgs=dict(start_epoch=1, max_iter=2))
    assert out['global_step'] == 4 and isinstance(out['optimizer'], FusedLBFGS) and int(out['optimizer'].step_count) == 2
    events = [json.loads(l) for l in open(tmp_path / 'log' / 'metrics.jsonl')]
    training = [e for e in events if e['event'] == 'training']
    # log_step 100: the loop logs at global_step 1 (Adam); the L-BFGS row is asked for below
    assert training and all('lbfgs_iters' not in e for e in training if e['global_step'] <= 2)
    ck = torch.load(tmp_path / 'ck' / 'physics_latest.pth', map_location='cpu')
    m2 = _model()
    m2.physics_net.load_state_dict(ck['model'], strict=True)
    # a second run resumes INTO the phase (epoch 2 >= start_epoch), on a lead batch, and logs its step
    m2.train_cfg.setdefault('log', {})['log_step'] = 2              # (a log step is global_step % log_step == 1: step 5)
    out2 = m2.run_train_interface(samples=src, valid_samples=val, log_path=str(tmp_path / 'log2'), checkpoint_path=str(tmp_path / 'ck'), num_epoch=3,
                                  pde_start_step=1, lead_batch=2, lbfgs=dict(start_epoch=1, max_iter=2, history_size=2))
    assert isinstance(out2['optimizer'], FusedLBFGS) and out2['global_step'] == 5
    rows = [e for e in (json.loads(l) for l in open(tmp_path / 'log2' / 'metrics.jsonl')) if e['event'] == 'training']
    assert rows and all({'lbfgs_iters', 'lbfgs_evals', 'lbfgs_t', 'lbfgs_status'} <= set(e) for e in rows)
    assert all(e['lbfgs_iters'] <= 2 and e['lbfgs_evals'] >= 1 and isinstance(e['lbfgs_status'], str) for e in rows)
    assert m2.last_lbfgs['lbfgs_status'] == out2['optimizer'].last['status']
    for bad in (dict(ema_weights=0.9), dict(step_guard=True), dict(balance_losses=True), dict(causal_weights=dict(eps=1.0)), dict(adaptive_interior=True)):
        with pytest.raises(ValueError, match='lbfgs together with'):
            m2.run_train_interface(samples=src, num_epoch=4, lbfgs=dict(start_epoch=0), **bad)
