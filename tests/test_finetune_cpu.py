"""No GPU: the fine-tuning surface up to the point where a device is needed -- optim.resolve_param_groups (patterns -> groups), the train.py
flags, InterfacePhysics.freeze / unfreeze and build_optimizer's config path (what it freezes and which groups, layout and keywords it hands to
the fused optimiser), the staged backward's cuts on tensors that do not require grad."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _P:
    def __init__(self, requires_grad=True):
        self.requires_grad = requires_grad


NAMES = ['meta_net.enc.weight', 'meta_net.enc.bias', 'meta_net.norm.weight', 'U_net.coord_input_fc.weight', 'U_net.coord_input_fc.bias',
         'U_net.out_fc.weight', 'U_net.out_fc.bias', 'T_net.coord_hidden_fc.weight', 'T_net.norm.weight']


def _named(frozen=()):
    return [(k, _P(k not in frozen)) for k in NAMES]


# ---------------------------------------------------------------------------------------------- resolve_param_groups
def test_earlier_groups_win_and_the_rest_forms_the_last_group_with_the_defaults():
    from deepphysinet_amd.optim import resolve_param_groups
    named = _named()
    frozen, groups = resolve_param_groups(named, ['meta_net.*'], [dict(match=['*.bias', '*norm*'], weight_decay=0.0),
                                                                  dict(match=['*_net.coord_*_fc.*'], lr=1e-5, betas=[0.8, 0.99])],
                                          dict(lr=1e-4, weight_decay=1e-4))
    assert frozen == NAMES[:3]
    assert [g['names'] for g in groups] == [['U_net.coord_input_fc.bias', 'U_net.out_fc.bias', 'T_net.norm.weight'],       # '*.bias' claimed coord_input_fc.bias first
                                            ['U_net.coord_input_fc.weight', 'T_net.coord_hidden_fc.weight'],
                                            ['U_net.out_fc.weight']]
    by_name = dict(named)
    assert all(g['params'] == [by_name[k] for k in g['names']] for g in groups)
    assert groups[0]['weight_decay'] == 0.0 and groups[0]['lr'] == 1e-4                       # missing keys come from the defaults
    assert groups[1]['lr'] == 1e-5 and groups[1]['weight_decay'] == 1e-4 and groups[1]['betas'] == (0.8, 0.99)
    assert {k: v for k, v in groups[2].items() if k not in ('names', 'params')} == dict(lr=1e-4, weight_decay=1e-4)
    # nothing configured: one group of everything, nothing frozen; a parameter frozen beforehand counts as frozen
    assert resolve_param_groups(_named())[0] == [] and [g['names'] for g in resolve_param_groups(_named())[1]] == [NAMES]
    frozen, groups = resolve_param_groups(_named(frozen=NAMES[:3]), None, None, {})
    assert frozen == NAMES[:3] and [g['names'] for g in groups] == [NAMES[3:]]
    # groups that claim everything: no remainder group; a single pattern string is a list of one
    _, groups = resolve_param_groups(_named(), None, [dict(match='meta_net.*', lr=1.0), dict(match=['*'])], {})
    assert [len(g['names']) for g in groups] == [3, 6]


def test_resolution_errors_are_value_errors():
    from deepphysinet_amd.optim import resolve_param_groups
    with pytest.raises(ValueError, match='matches no parameter'):
        resolve_param_groups(_named(), ['metanet.*'])
    with pytest.raises(ValueError, match='matches no parameter'):
        resolve_param_groups(_named(), None, [dict(match=['*.bias', 'nothing.*'])])
    with pytest.raises(ValueError, match='no trainable parameter'):
        resolve_param_groups(_named(), ['*'])
    with pytest.raises(ValueError, match='no trainable parameter'):
        resolve_param_groups(_named(frozen=NAMES[3:]), ['meta_net.*'])
    with pytest.raises(ValueError, match='not an Adam hyper-parameter'):
        resolve_param_groups(_named(), None, [dict(match=['*.bias'], momentum=0.9)])
    with pytest.raises(ValueError, match='not an Adam hyper-parameter'):
        resolve_param_groups(_named(), None, [dict(match=['*.bias'], max_norm=1.0)])         # the clip is global
    with pytest.raises(ValueError, match='not an Adam hyper-parameter'):
        resolve_param_groups(_named(), None, None, dict(max_norm=1.0))
    with pytest.raises(ValueError, match='match'):
        resolve_param_groups(_named(), None, [dict(lr=1e-3)])
    with pytest.raises(ValueError, match='frozen or belongs to an earlier group'):
        resolve_param_groups(_named(), ['meta_net.*'], [dict(match=['meta_net.norm.*'])])
    with pytest.raises(ValueError, match='at most 16'):
        resolve_param_groups([('p%d' % i, _P()) for i in range(17)], None, [dict(match=['p%d' % i]) for i in range(17)])


# ---------------------------------------------------------------------------------------------- train.py
def _train_cli():
    spec = importlib.util.spec_from_file_location('train_cli_under_test', os.path.join(ROOT, 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                  # (the launcher's body runs under __main__ only)
    return mod


def test_train_py_parses_freeze_and_param_group_flags(capsys):
    cli = _train_cli()
    a = cli.parse.parse_args(['--freeze', 'meta_net.*', '--freeze', '*.out_fc.*', '--param_group', '*.bias,*norm*:weight_decay=0,betas=0.5/0.9',
                              '--param_group', '*_net.coord_*_fc.*:lr=1e-5,eps=1e-6'])
    assert a.freeze == ['meta_net.*', '*.out_fc.*']
    assert a.param_group == [dict(match=['*.bias', '*norm*'], weight_decay=0.0, betas=(0.5, 0.9)), dict(match=['*_net.coord_*_fc.*'], lr=1e-5, eps=1e-6)]
    none = cli.parse.parse_args([])
    assert none.freeze is None and none.param_group is None
    for bad in ('no_colon', ':lr=1', 'x:momentum=0.9', 'x:lr', 'x:lr=abc', 'x:betas=0.9', 'x:max_norm=1'):
        with pytest.raises(SystemExit):
            cli.parse.parse_args(['--param_group', bad])
    capsys.readouterr()
    # what the parser gives is what resolve_param_groups takes
    from deepphysinet_amd.optim import resolve_param_groups
    frozen, groups = resolve_param_groups(_named(), a.freeze, a.param_group, {})
    assert 'U_net.out_fc.weight' in frozen and [len(g['names']) for g in groups] == [2, 2]


# ---------------------------------------------------------------------------------------------- the interface, on the host
def _interface(optimizer=None):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config(), precision='bf16x2')
    if optimizer:
        m.train_cfg['optimizer'] = dict(m.train_cfg['optimizer'], **optimizer)
    return m


def test_freeze_and_unfreeze_return_the_names_they_changed():
    m = _interface()
    names = [k for k, _ in m.physics_net.named_parameters()]
    enc = [k for k in names if k.startswith('meta_net.')]
    assert m.freeze(['meta_net.*']) == enc and m.freeze('meta_net.*') == []
    assert all(p.requires_grad == (not k.startswith('meta_net.')) for k, p in m.physics_net.named_parameters())
    assert [len(b) for b in m.physics_net.trainable_buckets()] == [48, 36, 0, 0]
    heads = m.freeze(['*_net.coord_*_fc.*', '*_net.fore_h_fc.*'])
    assert len(heads) == 36 and [len(b) for b in m.physics_net.trainable_buckets()] == [48, 0, 0, 0]
    assert m.unfreeze(['meta_net.model.learnable_token', '*_net.fore_h_fc.bias']) == ['meta_net.model.learnable_token'] + [k for k in names if k.endswith('fore_h_fc.bias')]
    assert [len(b) for b in m.physics_net.trainable_buckets()] == [48, 6, 0, 1]
    with pytest.raises(ValueError, match='matches no parameter'):
        m.freeze(['encoder.*'])
    with pytest.raises(ValueError, match='no trainable parameter'):
        m.freeze(['*'])
    assert sum(p.requires_grad for p in m.physics_net.parameters()) == 55                  # the refused freeze changed nothing
    assert len(m.unfreeze('*')) == 100 and all(p.requires_grad for p in m.physics_net.parameters())


class _Recorder:
    def __init__(self, params, **kw):
        self.params_arg, self.kw = params, kw
        self.param_groups = [dict(g) for g in params] if isinstance(params, list) and params and isinstance(params[0], dict) else [dict(params=list(params), lr=kw['lr'])]
        self.ema_decay = kw.get('ema_decay')


def test_build_optimizer_config_path_freezes_and_groups_before_it_needs_a_device(monkeypatch):
    from deepphysinet_amd.interface import interface_physics
    cfg = dict(freeze=['meta_net.*'], param_groups=[dict(match=['*_net.coord_*_fc.*', '*_net.fore_h_fc.*'], lr=1e-5),
                                                    dict(match=['*.bias'], weight_decay=0.0, betas=(0.8, 0.99))])
    # the real optimiser: the freeze is applied, then the fused optimiser refuses host parameters (there is no CPU fallback)
    m = _interface(cfg)
    with pytest.raises(RuntimeError, match='HIP parameters'):
        m.build_optimizer()
    assert all(p.requires_grad == (not k.startswith('meta_net.')) for k, p in m.physics_net.named_parameters())
    # what it hands over
    monkeypatch.setattr(interface_physics, 'FusedClipAdam', _Recorder)
    m = _interface(cfg)
    opt = m.build_optimizer(max_norm=3.0)
    names = {id(p): k for k, p in m.physics_net.named_parameters()}
    groups = opt.params_arg
    assert [len(g['params']) for g in groups] == [36, 24, 24] and sum(len(g['params']) for g in groups) == 84
    assert all(names[id(p)] == k for g in groups for p, k in zip(g['params'], g['names']))
    assert all('.coord_' in k or '.fore_h_fc.' in k for k in groups[0]['names'])
    assert all(k.endswith('.bias') and '.coord_' not in k for k in groups[1]['names'])
    assert not any(k.endswith('.bias') or k.startswith('meta_net.') for k in groups[2]['names'])
    assert (groups[0]['lr'], groups[0]['weight_decay']) == (1e-5, 1e-4) and (groups[1]['lr'], groups[1]['weight_decay'], groups[1]['betas']) == (1e-4, 0.0, (0.8, 0.99))
    assert (groups[2]['lr'], groups[2]['weight_decay']) == (1e-4, 1e-4) and 'betas' not in groups[2]
    assert [g['initial_lr'] for g in opt.param_groups] == [1e-5, 1e-4, 1e-4]
    assert opt.kw['max_norm'] == 3.0 and 'freeze' not in opt.kw and 'param_groups' not in opt.kw and opt.kw['lr'] == 1e-4
    layout = opt.kw['layout']
    assert [len(b) for b in layout] == [48, 36, 0, 0] and {id(p) for b in layout for p in b} == {id(p) for g in groups for p in g['params']}
    # keywords win over the config; without either key and nothing frozen: the call of before
    m = _interface(cfg)
    opt = m.build_optimizer(freeze=['*_net.out_fc.*'], param_groups=None)
    assert len(opt.params_arg) == 1 and len(opt.params_arg[0]['params']) == 155 - 12 and [len(b) for b in opt.kw['layout']] == [36, 36, 68, 3]
    m = _interface()
    opt = m.build_optimizer()
    assert not isinstance(opt.params_arg, list) and len(list(opt.param_groups[0]['params'])) == 155 and [len(b) for b in opt.kw['layout']] == [48, 36, 68, 3]
    assert opt.param_groups[0]['initial_lr'] == 1e-4
    with pytest.raises(ValueError, match='not an Adam hyper-parameter'):
        _interface(dict(param_groups=[dict(match=['*.bias'], momentum=0.9)])).build_optimizer()


# ---------------------------------------------------------------------------------------------- the staged backward's cuts
class _Placer:
    def __init__(self):
        self.placed = {}

    def place_gradients(self, params, grads):
        assert len(params) == len(grads)
        for p, g in zip(params, grads):
            self.placed[id(p)] = g


@pytest.mark.parametrize('frozen', ['encoder', 'encoder+heads', 'a static', 'nothing'])
def test_staged_backward_differentiates_only_what_requires_grad(frozen):
    """A four-bucket toy graph in plain torch: statics | heads | encoder | embedding.  Whatever is frozen, the trainable gradients equal those
    of loss.backward(), the frozen ones are never asked for, and the cuts behind a frozen part launch nothing."""
    from deepphysinet_amd.staged_backward import StagedBackward
    torch.manual_seed(0)
    leaf = lambda *s: torch.randn(*s, dtype=torch.float64, requires_grad=True)
    statics, heads_p, enc_p, emb_p = [leaf(3), leaf(3)], [leaf(4, 3)], [leaf(4, 4)], [leaf(4)]
    off = {'encoder': enc_p + emb_p, 'encoder+heads': enc_p + emb_p + heads_p, 'a static': statics[:1], 'nothing': []}[frozen]
    for p in off:
        p.requires_grad_(False)
    field = torch.randn(4, dtype=torch.float64)

    def forward():
        x0 = field * emb_p[0]
        meta = torch.tanh(enc_p[0] @ x0)
        heads = meta @ heads_p[0]
        evec = torch.sin(meta) @ heads_p[0]                      # a sibling of heads, as in _HeadsFn: neither lies on the other's path
        loss = (heads * statics[0]).sum() + (evec * statics[1]).sum() ** 2
        return loss, heads, evec, meta, x0
    loss, *_ = forward()
    loss.backward()
    everything = statics + heads_p + enc_p + emb_p
    plain = {id(p): (p.grad.clone() if p.grad is not None else None) for p in everything}
    buckets = [[p for p in b if p.requires_grad] for b in (statics, heads_p, enc_p, emb_p)]
    placer = _Placer()
    back = StagedBackward(buckets, placer)
    loss, heads, evec, meta, x0 = forward()
    back.points(loss, heads, evec, statics, meta, x0, torch.ones((), dtype=torch.float64))
    back.heads_cut()
    if frozen in ('encoder', 'encoder+heads'):
        assert back.g_meta is None and back.meta_out is None and back.x0 is None
    back.encoder()
    back.embedding()
    assert all(getattr(back, k) is None for k in StagedBackward.HELD)
    assert set(placer.placed) == {id(p) for p in everything if p.requires_grad}
    for p in everything:
        if p.requires_grad:
            assert torch.equal(placer.placed[id(p)], plain[id(p)])
        else:
            assert plain[id(p)] is None
