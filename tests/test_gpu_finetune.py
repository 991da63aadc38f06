"""GPU (MI355X): fine-tuning -- the training steps with frozen parameters and the configured parameter groups, on a closed-form-filled
PhysicsNet at precision 'bf16x2', all PDE losses on, (n_inter, n_margin) = (256, 256) and (300, 200).

What a frozen part must give: its tensors bit-identical after the steps, its backward not run (the encoder's: counters on the two encoder
nodes' backward stay 0), and the gradients of everything trainable equal to those of the same batch's all-trainable backward.  The optimiser
then holds the trainable parameters only; its step is held against clip_grad_norm_ over the trainable set + torch.optim.Adam fed the same
gradients, at the bounds of test_fused_clip_adam_equals_torch (rtol 2e-5, atol 2e-7).
"""
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_step import ROOT, _dev, _free_port, _gpu, _loss, _model, _RecordingReducer
from oracle.fill import synthetic_inputs

pytestmark = pytest.mark.gpu

SIZES = [(256, 256), (300, 200)]
ENCODER = ['meta_net.*']
HEADS = ['*_net.coord_*_fc.*', '*_net.fore_h_fc.*']
SUBSETS = {
    'encoder': ENCODER,
    'encoder+heads': ENCODER + HEADS,
    'only_T_net': ENCODER + ['U_net.*', 'V_net.*', 'P_net.*', 'rio_net.*', 'q_net.*'],
}

# The heads' weight gradients come out of ONE dpn_sgemm_batch launch, which picks its kernel by the launch's size: more than 512 output tiles run the
# pipelined 64-k form, fewer the single-stage 256-k form (csrc/dpn_gemm.hip: kSingleStageMaxOutTiles), and the two add the K products in different
# orders.  All twelve heads are 1056 tiles (with the g_meta problems 1440), so freezing the encoder keeps the kernel and the bits; one net's
# heads alone are 176 tiles and take the other kernel.  Those tensors are held to the gradient bound of the step parity tests
# (tests/test_gpu_parity.py TOL['bf16x2']['grad']: every element within 1e-3 of its tensor's maximum) -- DESIGN.md section 6d.
SMALL_HEADS_LAUNCH = ('only_T_net',)
PARITY_GRAD = 1e-3


def _batch(n_inter, n_margin, k=0):
    from deepphysinet_amd.sampler import SyntheticSamples
    return SyntheticSamples(_dev(), n_margin=n_margin, n_inter=n_inter, leads=k + 1, seed=3)[k]


class _BackwardCounter:
    """Counts the calls of the encoder stack's and the data embedding's backward."""

    def __init__(self, monkeypatch):
        from deepphysinet_amd import encoder_ops
        self.n = 0
        for cls in (encoder_ops._EncoderStackFn, encoder_ops._DataEmbeddingFn):
            inner = cls.backward

            def counted(ctx, *g, _inner=inner):
                self.n += 1
                return _inner(ctx, *g)
            monkeypatch.setattr(cls, 'backward', staticmethod(counted))


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.physics_net.named_parameters() if p.grad is not None}


_REFERENCE = {}


def _all_trainable_gradients(n_inter, n_margin):
    """{name: gradient} of one all-trainable training_step backward on the batch of this size: computed once, shared, never written to."""
    if (n_inter, n_margin) not in _REFERENCE:
        m = _model()
        opt = m.build_optimizer()
        m.training_step(_batch(n_inter, n_margin), opt, with_pde=True)       # (the gradients stay in their slots until the next zero_grad)
        assert len(opt.params) == 155
        _REFERENCE[(n_inter, n_margin)] = _grads(m)
    return _REFERENCE[(n_inter, n_margin)]


@pytest.mark.parametrize('n_inter,n_margin', SIZES)
@pytest.mark.parametrize('subset', list(SUBSETS))
def test_training_step_with_a_frozen_subset(subset, n_inter, n_margin, monkeypatch):
    ref = _all_trainable_gradients(n_inter, n_margin)
    counter = _BackwardCounter(monkeypatch)
    m = _model()
    frozen = m.freeze(SUBSETS[subset])
    start = {k: v.detach().clone() for k, v in m.physics_net.state_dict().items()}
    trainable = [k for k, p in m.physics_net.named_parameters() if p.requires_grad]
    assert set(frozen) | set(trainable) == set(dict(m.physics_net.named_parameters())) and not set(frozen) & set(trainable)
    opt = m.build_optimizer(lr=1e-3, weight_decay=1e-2)
    assert len(opt.params) == len(trainable) and len(opt.bucket_bounds) == 4
    b = _batch(n_inter, n_margin)
    assert not m.physics_net.encode_field(b['field_data'], b['forecast_h']).requires_grad
    m.physics_net.clear_field_cache()
    # the reference optimiser: clip_grad_norm_ over the trainable set + torch.optim.Adam, fed this model's gradients
    params = dict(m.physics_net.named_parameters())
    shadow = {k: params[k].detach().clone().requires_grad_(True) for k in trainable}
    ref_opt = torch.optim.Adam(list(shadow.values()), lr=1e-3, weight_decay=1e-2)
    max_norm = None
    for step in range(3):
        loss, _, gnorm = m.training_step(_batch(n_inter, n_margin, step), opt, with_pde=True, max_norm=1e30 if max_norm is None else max_norm)
        assert counter.n == 0 and torch.isfinite(loss)
        got = _grads(m)
        assert set(got) == set(trainable)                      # nothing was written for a frozen parameter
        if step == 0:
            worst = max(float((got[k] - ref[k]).abs().max() / (ref[k].abs().max() + 1e-30)) for k in trainable)
            print('%s (%d, %d): worst |g - g_all_trainable| / max |g| = %.3e' % (subset, n_inter, n_margin, worst))
            for k in trainable:
                if subset in SMALL_HEADS_LAUNCH and ('.coord_' in k or '.fore_h_fc.' in k):
                    assert float((got[k] - ref[k]).abs().max()) <= PARITY_GRAD * float(ref[k].abs().max()), (subset, k)
                else:
                    assert torch.equal(got[k], ref[k]), (subset, k)
            max_norm = 0.5 * float(gnorm)                      # steps 2 and 3 run with an active clip (asserted below)
        for k in trainable:
            shadow[k].grad = got[k].clone()
        n_ref = torch.nn.utils.clip_grad_norm_(list(shadow.values()), max_norm=1e30 if step == 0 else max_norm)       # the norm over the trainable set only
        ref_opt.step()
        assert abs(float(gnorm) - float(n_ref)) <= 1e-5 * float(n_ref)
        if step > 0:
            assert float(gnorm) > max_norm
        for k in trainable:
            assert torch.allclose(params[k].detach(), shadow[k].detach(), rtol=2e-5, atol=2e-7), (subset, step, k)
    now = m.physics_net.state_dict()
    for k in frozen:
        assert torch.equal(now[k].view(torch.int32), start[k].view(torch.int32)), k
    assert any(not torch.equal(now[k], start[k]) for k in trainable)
    # validation and the balance refresh run on the frozen model too
    v = m.validation_step(_batch(n_inter, n_margin))
    assert torch.isfinite(v['valid_loss'])
    from deepphysinet_amd.balance import LossBalance
    loss, _, _ = m.training_step(_batch(n_inter, n_margin), opt, with_pde=True, balance=LossBalance(every=1))
    assert torch.isfinite(loss) and counter.n == 0


@pytest.mark.parametrize('n_inter,n_margin', SIZES)
def test_training_step_batch_with_the_encoder_frozen(n_inter, n_margin, monkeypatch):
    batches = [_batch(n_inter, n_margin, k) for k in range(2)]
    m0 = _model()
    opt0 = m0.build_optimizer()
    m0.training_step_batch(batches, opt0, with_pde=True)
    ref = _grads(m0)
    counter = _BackwardCounter(monkeypatch)
    m = _model()
    frozen = m.freeze(ENCODER)
    start = {k: v.detach().clone() for k, v in m.physics_net.state_dict().items()}
    opt = m.build_optimizer()
    loss, parts, gnorm, per = m.training_step_batch(batches, opt, with_pde=True)
    got = _grads(m)
    assert torch.isfinite(loss) and torch.isfinite(gnorm) and counter.n == 0 and len(got) == 84
    for k, g in got.items():
        assert torch.equal(g, ref[k]), k
    now = m.physics_net.state_dict()
    assert all(torch.equal(now[k].view(torch.int32), start[k].view(torch.int32)) for k in frozen)


def test_staged_step_with_the_encoder_frozen_is_one_stage_and_equals_the_plain_backward(monkeypatch):
    """StagedPdeStep differentiates place_one_batch's loss: its eager stage gives the gradients of that loss's plain backward, which are the
    all-trainable model's for every trainable tensor.  training_step's own staged form (a reducer bound to the optimiser) hands reduce_bucket the
    ranges (0, 2), (2, 4), the second empty, and leaves the plain step's gradients and parameters."""
    from deepphysinet_amd.interface.interface_physics import StagedPdeStep
    g = _gpu(synthetic_inputs(300, tag='inter'))
    m0 = _model()
    _loss(m0, g).backward()
    full = _grads(m0)
    counter = _BackwardCounter(monkeypatch)
    m = _model()
    m.freeze(ENCODER)
    opt = m.build_optimizer()
    _loss(m, g).backward()
    plain = _grads(m)
    st = StagedPdeStep(m, opt, g)
    assert st.stages == (st.stage_points_and_heads,) and st.stage_buckets == ((0, 2),)
    st.stages[0]()
    got = _grads(m)
    assert counter.n == 0 and set(got) == set(plain) and len(got) == 84
    assert all(getattr(st.back, k) is None for k in st.back.HELD)
    for k in got:
        assert torch.equal(got[k], plain[k]) and torch.equal(got[k], full[k]), k
    opt.step()
    assert torch.isfinite(opt.grad_norm).all()
    # training_step: the staged form against the plain one
    res = []
    for staged in (False, True):
        mm = _model()
        mm.freeze(ENCODER)
        oo = mm.build_optimizer()
        rec = _RecordingReducer(oo) if staged else None
        if staged:
            assert [len(b) for b in mm._can_stage(oo, rec, True)] == [48, 36, 0, 0]
        loss, _, gnorm = mm.training_step(_batch(256, 256), oo, with_pde=True, grad_sync=rec)
        res.append((loss, gnorm.clone(), _grads(mm), [p.detach().clone() for p in mm.physics_net.parameters()]))
    assert rec.calls == [(0, 2), (2, 4)] and oo.bucket_bounds[2][0] == oo.bucket_bounds[3][1]        # the second range is empty
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(res[0][2][k], res[1][2][k]) for k in res[0][2]) and all(torch.equal(a, b) for a, b in zip(res[0][3], res[1][3]))
    assert counter.n == 0


def test_captured_staged_step_with_the_encoder_frozen_replayed_three_times_equals_three_eager_steps():
    from deepphysinet_amd import grad_arena
    from deepphysinet_amd.interface.interface_physics import StagedPdeStep
    g = _gpu(synthetic_inputs(300, tag='inter'))
    runs = []
    for _ in range(2):
        m = _model()
        m.freeze(ENCODER)
        opt = m.build_optimizer(lr=1e-3)
        st = StagedPdeStep(m, opt, g)

        def step(st=st, opt=opt):
            for stage in st.stages:
                stage()
            opt.step()
        runs.append((m, opt, step))
    (ma, oa, step_a), (mb, ob, step_b) = runs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step_a(); step_a()                                     # eager steps in front of the capture
    torch.cuda.current_stream().wait_stream(s)
    step_b(); step_b()
    torch.cuda.synchronize()
    was = grad_arena.captured_step[0]
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step_a()
        for _ in range(3):
            graph.replay()
            step_b()
        torch.cuda.synchronize()
    finally:
        grad_arena.captured_step[0] = was
    assert int(oa.step_count) == int(ob.step_count) == 5
    for (k, a), b in zip(ma.physics_net.named_parameters(), mb.physics_net.parameters()):
        assert torch.equal(a, b), k


_DIST_SCRIPT = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, 'tests'))
import torch
from deepphysinet_amd import distributed as D
from deepphysinet_amd.sampler import SyntheticSamples
from test_gpu_step import _model
rank, world, local = D.init_from_env('nccl', force=True)
dev = torch.device('cuda:0')
batch = SyntheticSamples(dev, n_margin=256, n_inter=256, leads=1, seed=3)[0]
res = {{}}
for mode in ('plain', 'staged'):
    m = _model()
    m.freeze(['meta_net.*'])
    opt = m.build_optimizer()
    sync = D.GradientAllReduce(opt, single_rank_too=True) if mode == 'staged' else None
    if sync is not None:
        buckets = m._can_stage(opt, sync, True)
        assert buckets is not None and [len(b) for b in buckets] == [48, 36, 0, 0], buckets
        sync.reduce_bucket(2, 4)                                  # an empty range: no collective, nothing queued
        assert sync._work == [] and sync.last_queued is None
    loss, parts, gnorm = m.training_step(batch, opt, with_pde=True, grad_sync=sync)
    torch.cuda.synchronize()
    if sync is not None:
        assert sync.last_queued == (0, 2), sync.last_queued
        sync(m.physics_net.parameters())                          # the unstaged route on the same optimiser: frozen parameters have no gradient to gather
        assert all(p.grad is None for p in m.physics_net.meta_net.parameters())
    res[mode] = (float(loss), float(gnorm), [p.detach().clone() for p in m.physics_net.parameters()])
assert res['plain'][0] == res['staged'][0] and res['plain'][1] == res['staged'][1], (res['plain'][:2], res['staged'][:2])
assert all(torch.equal(a, b) for a, b in zip(res['plain'][2], res['staged'][2]))
# the generic path (no optimiser): frozen parameters are skipped, not given zero gradients
generic = D.GradientAllReduce(None, single_rank_too=True)
generic(m.physics_net.parameters())
assert all(p.grad is None for p in m.physics_net.meta_net.parameters())
print('FINETUNE_DIST_OK')
torch.distributed.destroy_process_group()
'''


def test_one_rank_all_reduce_with_a_frozen_encoder_takes_the_staged_path(tmp_path):
    script = tmp_path / 'finetune_dist.py'
    script.write_text(_DIST_SCRIPT.format(root=ROOT))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'FINETUNE_DIST_OK' in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------- configured groups, the loop
TUNE = dict(freeze=['meta_net.*'], param_groups=[dict(match=HEADS, lr=1e-5), dict(match=['*.bias'], weight_decay=0.0)])


def _configured():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['train_cfg']['optimizer'].update(TUNE)
    cfg['train_cfg']['train_data'].update(label_batch_size=256, batch_size_inter=256)
    torch.manual_seed(11)
    return builder_models(**cfg, precision='bf16x2').to(_dev())


def test_build_optimizer_from_a_config_with_freeze_and_two_groups():
    m = _configured()
    opt = m.build_optimizer()
    names = {id(p): k for k, p in m.physics_net.named_parameters()}
    member = [[names[id(p)] for p in g['params']] for g in opt.param_groups]
    assert [len(x) for x in member] == [36, 24, 24] and member == [g['names'] for g in opt.param_groups]
    assert all('.coord_' in k or '.fore_h_fc.' in k for k in member[0])
    assert all(k.endswith('.bias') for k in member[1]) and not any(k.endswith('.bias') for k in member[2])
    assert not any(k.startswith('meta_net.') for x in member for k in x)
    assert [(g['lr'], g['initial_lr'], g['weight_decay']) for g in opt.param_groups] == [(1e-5, 1e-5, 1e-4), (1e-4, 1e-4, 0.0), (1e-4, 1e-4, 1e-4)]
    assert tuple(opt._hyper.shape) == (3, 8) and len(opt.params) == 84 and [len(b) for b in opt.layout_ids] == [48, 36, 0, 0]
    assert all(not p.requires_grad for p in m.physics_net.meta_net.parameters())
    hyper = opt._hyper.cpu()
    assert [round(float(x), 12) for x in hyper[:, 0]] == [round(float(torch.tensor(v, dtype=torch.float32)), 12) for v in (1e-5, 1e-4, 1e-4)]
    with pytest.raises(NotImplementedError):
        opt.add_param_group(dict(params=list(m.physics_net.meta_net.parameters())[:1]))


def test_loop_with_configured_groups_writes_a_full_checkpoint_and_a_complete_ema(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.model.physics_net import PhysicsNet
    m = _configured()
    start = {k: v.detach().cpu().clone() for k, v in m.physics_net.state_dict().items()}
    out = m.run_train_interface(samples='synthetic', samples_per_epoch=3, max_steps=3, num_epoch=1, pde_start_step=1, checkpoint_path=str(tmp_path / 'ck'),
                                ema_weights=0.9)
    assert out['global_step'] == 3 and isinstance(out['lr'], list) and len(out['lr']) == 3
    ck = torch.load(tmp_path / 'ck' / 'physics_latest.pth', map_location='cpu')
    assert len(ck['model']) == 156 and list(ck['model']) == list(start) == list(ck['model_ema'])
    frozen = [k for k in start if k.startswith('meta_net.')]
    assert len(frozen) >= 71
    for k in frozen:
        assert torch.equal(ck['model'][k], start[k]) and torch.equal(ck['model_ema'][k], start[k]), k
    moved = [k for k in start if not k.startswith('meta_net.') and not torch.equal(ck['model'][k], start[k])]
    assert moved
    assert any(not torch.equal(ck['model_ema'][k], ck['model'][k]) for k in moved)
    cfg = ncep_config()
    fresh = PhysicsNet(cfg['meta_cfg'], cfg['net_cfg'])
    fresh.load_state_dict(ck['model_ema'], strict=True)
    fresh.load_state_dict(ck['model'], strict=True)
    assert ck['ema']['updates'] == 3
    # the fine-tuning run proper: a second run resumes from this checkpoint with the keywords instead of the config
    m2 = _configured()
    m2.train_cfg['optimizer'] = {k: v for k, v in m2.train_cfg['optimizer'].items() if k not in TUNE}
    out2 = m2.run_train_interface(samples=[], checkpoint_path=str(tmp_path / 'ck'), num_epoch=1, ema_weights=0.9, freeze=['meta_net.*', 'U_net.*'])
    opt2 = out2['optimizer']
    assert len(opt2.param_groups) == 1 and len(opt2.params) == 70 and opt2.ema_updates() == 3
    again = opt2.ema_state_dict(m2.physics_net)              # owned: the saved average; not owned (now frozen): the module's own, loaded, value
    assert all(torch.equal(again[k].cpu(), ck['model' if k.startswith('U_net.') else 'model_ema'][k]) for k in again)
