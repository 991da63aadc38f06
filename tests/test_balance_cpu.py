"""CPU: loss balancing by gradient norms -- the option's value type, the host references of deepphysinet_amd.balance on
hand-worked cases, the groups' maps, the loops' option parsing, and the binding of the new entry points."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (('dpn_balance_scratch_doubles', 2), ('dpn_balance_sumsq', 6), ('dpn_balance_update', 8), ('dpn_balance_combine', 8))


def test_loss_balance_checks_its_arguments():
    from deepphysinet_amd.balance import LossBalance
    b = LossBalance()
    assert (b.every, b.momentum, b.groups, b.lam_min, b.lam_max) == (100, 0.9, 'equations', 1e-3, 1e3)
    assert b.n_terms == 7 and b.names == ('data', 'motion_u', 'motion_v', 'continuous', 'energy', 'vapor', 'gas')
    p = LossBalance(every=1, momentum=0, groups='parts', lam_min=1, lam_max=1)
    assert p.n_terms == 3 and p.names == ('data', 'inter', 'margin') and isinstance(p.momentum, float) and (p.lam_min, p.lam_max) == (1.0, 1.0)
    assert LossBalance(momentum=1).momentum == 1.0
    for bad in (dict(every=0), dict(every=-3), dict(every=2.5), dict(every=True), dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=float('nan')),
                dict(groups='terms'), dict(lam_min=0.0), dict(lam_min=-1.0), dict(lam_min=2.0), dict(lam_max=0.5), dict(lam_max=float('inf')),
                dict(lam_min=float('nan'))):
        with pytest.raises(ValueError):
            LossBalance(**bad)
    with pytest.raises(Exception):
        b.every = 3                                                       # a value type: frozen


def test_the_groups_maps():
    from deepphysinet_amd.balance import STEP_TERMS, LossBalance, group_map
    eq, parts = group_map('equations'), group_map('parts')
    assert len(eq) == len(parts) == STEP_TERMS == 13
    assert eq == (1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 0)                 # interior e and margin e share equation e; the data loss is term 0
    assert parts == (1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 0)
    assert LossBalance(groups='parts').term_map() == parts and LossBalance().term_map() == eq
    assert max(eq) == LossBalance().n_terms - 1 and max(parts) == LossBalance(groups='parts').n_terms - 1
    with pytest.raises(ValueError):
        group_map('points')


def test_sumsq_reference_adds_squares_in_fp64_and_skips_none():
    from deepphysinet_amd.balance import sumsq_reference
    assert sumsq_reference([np.array([3.0, 4.0], dtype=np.float32)]) == 25.0
    assert sumsq_reference([np.array([1.0], dtype=np.float32), None, np.array([[2.0], [2.0]], dtype=np.float32)]) == 9.0
    # fp64 keeps what an fp32 sum loses: 1e15^2 + 1 - 1e15^2
    big = np.float32(1e15)
    assert sumsq_reference([np.array([1e-18], dtype=np.float32)]) == float(np.float32(1e-18)) ** 2 > 0.0
    assert sumsq_reference([np.array([big, 3e7], dtype=np.float32)]) == float(big) ** 2 + float(np.float32(3e7)) ** 2


def test_update_reference_on_hand_worked_cases():
    from deepphysinet_amd.balance import update_reference
    ones = np.ones(3, dtype=np.float32)
    # equal norms: the mean over each norm is 1, lambda stays exactly 1 (the mean form)
    lam, flag = update_reference([4.0, 4.0, 4.0], ones, 0.9, 1e-3, 1e3)
    assert flag == 0 and lam.dtype == np.float32 and (lam == 1.0).all()
    # norms 1, 3: mean 2 -> targets 2 and 2/3; momentum 0.5 from lambda = 1: 1.5 and 5/6
    lam, flag, diag = update_reference([1.0, 9.0], [1.0, 1.0], 0.5, 1e-3, 1e3, with_diag=True)
    assert flag == 0 and lam[0] == np.float32(1.5) and lam[1] == np.float32(0.5 + 0.5 * (2.0 / 3.0))
    assert diag.shape == (8,) and list(diag[:2]) == [1.0, 3.0] and list(diag[2:4]) == [2.0, 2.0 / 3.0] and diag[6] == 2.0 and diag[7] == 0.0
    assert list(diag[4:6]) == [float(lam[0]), float(lam[1])]
    # one zero norm: that term is inactive, keeps its lambda, and does not count in the mean
    lam, flag, diag = update_reference([1.0, 0.0, 9.0], [1.0, 7.0, 1.0], 0.0, 1e-3, 1e3, with_diag=True)
    assert flag == 0 and list(lam) == [np.float32(2.0), np.float32(7.0), np.float32(2.0 / 3.0)] and diag[3 + 1] == 0.0 and diag[9] == 2.0
    # one active term only: nothing to balance against
    lam, flag = update_reference([0.0, 5.0, 0.0], [2.0, 3.0, 4.0], 0.0, 1e-3, 1e3)
    assert flag == 1 and list(lam) == [2.0, 3.0, 4.0]
    # a NaN, an infinity: flagged, lambda unchanged
    for bad in (float('nan'), float('inf')):
        lam, flag, diag = update_reference([1.0, bad, 9.0], [2.0, 3.0, 4.0], 0.0, 1e-3, 1e3, with_diag=True)
        assert flag == 1 and list(lam) == [2.0, 3.0, 4.0] and diag[-1] == 1.0 and diag[-2] == 0.0 and (diag[3:6] == 0.0).all()
    # both clamps: norms 1e-4 and 1e4, mean ~ 5e3 -> targets 5e7 and 0.5 under [0.75, 100]: 100 and 0.75
    lam, flag = update_reference([1e-8, 1e8], [1.0, 1.0], 0.0, 0.75, 100.0)
    assert flag == 0 and list(lam) == [np.float32(100.0), np.float32(0.75)]
    # momentum 0: the target at once; momentum 1: lambda never moves
    lam0, _ = update_reference([1.0, 9.0], [5.0, 5.0], 0.0, 1e-3, 1e3)
    lam1, flag = update_reference([1.0, 9.0], [5.0, 0.25], 1.0, 1e-3, 1e3)
    assert list(lam0) == [np.float32(2.0), np.float32(2.0 / 3.0)] and flag == 0 and list(lam1) == [5.0, 0.25]
    for bad in (dict(momentum=1.5), dict(lam_min=0.0), dict(lam_max=0.5)):
        kw = dict(dict(momentum=0.5, lam_min=1e-3, lam_max=1e3), **bad)
        with pytest.raises(ValueError):
            update_reference([1.0, 2.0], [1.0, 1.0], **kw)
    with pytest.raises(ValueError):
        update_reference(np.ones(17), np.ones(17), 0.5, 1e-3, 1e3)


def test_the_loops_parse_the_option():
    from deepphysinet_amd.balance import LossBalance
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    assert m._balance_option({}) is None and m._balance_option({'balance_losses': None}) is None and m._balance_option({'balance_losses': False}) is None
    assert m.loss_balance_state is None
    opt = m._balance_option({'balance_losses': {'every': 2}})
    assert opt == LossBalance(every=2)
    assert m._balance_option({'balance_losses': True}) == LossBalance()
    given = LossBalance(every=7, groups='parts')
    assert m._balance_option({'balance_losses': given}) is given
    with pytest.raises(ValueError, match='unknown keys'):
        m._balance_option({'balance_losses': {'every': 2, 'group': 'parts'}})
    with pytest.raises(ValueError, match='every'):
        m._balance_option({'balance_losses': {'every': 0}})
    m.train_cfg['losses']['balance_losses'] = dict(every=5, momentum=0.5, groups='parts', lam_min=0.1, lam_max=10.0)          # the configuration's route
    opt = m._balance_option({})
    assert (opt.every, opt.momentum, opt.groups, opt.lam_min, opt.lam_max) == (5, 0.5, 'parts', 0.1, 10.0)
    assert m._balance_option({'balance_losses': None}) is None                                                           # the keyword wins
    m.train_cfg['losses']['balance_losses'] = LossBalance(every=9)
    assert m._balance_option({}).every == 9


def test_the_step_refuses_the_option_where_it_is_not_implemented():
    import torch
    from deepphysinet_amd.balance import LossBalance
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.interface.interface_physics import StagedPdeStep
    m = builder_models(**ncep_config())
    with pytest.raises(ValueError, match='device tensors'):
        m.training_step({'field_data': torch.zeros(1, 159, 2405)}, None, with_pde=True, balance=LossBalance())
    with pytest.raises(TypeError):
        m.training_step({'field_data': torch.zeros(1, 159, 2405)}, None, with_pde=True, balance={'every': 2})
    with pytest.raises(TypeError, match='GradientAllReduce'):                       # a plain callable could not keep lambda equal on the ranks
        m.training_step({'field_data': torch.zeros(1, 159, 2405)}, None, with_pde=True, grad_sync=lambda params: None, balance=LossBalance())
    with pytest.raises(NotImplementedError, match='balanc'):
        StagedPdeStep(m, None, {}, balance=LossBalance())


def test_a_checkpoint_carries_the_weights_and_one_without_them_loads_as_before(tmp_path):
    import torch
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    m.save_model(str(tmp_path), 0, 5, prefix='physics')
    assert 'loss_balance' not in torch.load(tmp_path / 'physics_0.pth')
    m.loss_balance_state = {'groups': 'parts', 'lam': torch.tensor([1.0, 0.3, 7.5]), 'step': 4, 'diag': None}
    m.save_model(str(tmp_path), 1, 9, prefix='physics')
    m2 = builder_models(**ncep_config())
    sd, epoch, step = m2.load_model(str(tmp_path / 'physics_0.pth'))
    assert m2.loss_balance_state is None and (epoch, step) == (1, 5)
    sd, epoch, step = m2.load_model(str(tmp_path), prefix='physics')
    st = m2.loss_balance_state
    assert (epoch, step) == (2, 9) and st['groups'] == 'parts' and st['step'] == 4 and st['lam'].dtype == torch.float32
    assert torch.equal(st['lam'], torch.tensor([1.0, 0.3, 7.5]))


def test_balance_entry_points_are_declared_exported_and_match_the_binding():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.build import EXP_UNITS, UNITS, build_library
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    unit = [u for u in UNITS if os.path.basename(u[0]) == 'dpn_balance.hip']
    assert len(unit) == 1 and unit[0][2] == 'dpn_balance.o' and unit[0][1] == []
    assert EXP_UNITS == (4,) and os.path.basename(UNITS[4][0]) == 'dpn_fp8.hip'                # the experiment unit keeps its index
    assert [os.path.basename(u[0]) for u in UNITS[:11]] == ['dpn_point.hip', 'dpn_wgrad.hip', 'dpn_encoder.hip', 'dpn_sampler.hip', 'dpn_fp8.hip',
                                                           'dpn_encoder_chain.hip', 'dpn_eval.hip', 'dpn_adaptive.hip', 'dpn_residual.hip',
                                                           'dpn_gemm.hip', 'dpn_optim.hip']
    lib = build_library()
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name, n_args in NEW:
        assert re.search(r' T %s$' % name, syms, re.M), name
        assert name in L.EXPORTS and len(L.EXPORTS[name][1]) == n_args
        decl = re.search(r'^int(?:64_t)? %s\((.*?)\);' % name, header, re.M | re.S).group(1)
        assert len(decl.split(',')) == n_args, name
    assert L.BALANCE_MAX_TERMS == 16 and '#define DPN_BALANCE_MAX_TERMS 16' in header
    assert L.BALANCE_STEP_TERMS == 13 and '#define DPN_BALANCE_STEP_TERMS 13' in header and '#define DPN_BALANCE_MAX_TENSORS 4096' in header
    # every balance symbol the header declares is bound
    assert sorted(set(re.findall(r'\b(dpn_balance_\w+)\(', header))) == sorted(n for n, _ in NEW)


def test_balance_unit_cross_compiles_without_atomics_or_spills(tmp_path):
    from deepphysinet_amd.build import COMMON, UNITS
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src, flags, obj = [u for u in UNITS if u[2] == 'dpn_balance.o'][0]
    asm = str(tmp_path / 'dpn_balance.s')
    subprocess.run([hipcc, *[f for f in COMMON if f != '-fPIC'], *flags, '--cuda-device-only', '-S', '-I' + os.path.join(ROOT, 'include'), src, '-o', asm],
                   check=True, capture_output=True)
    text = open(asm).read()
    names = re.findall(r'\.name:\s+(\S*dpn_balance_\w+_kernel\S*)', text)
    assert len(names) == 4, names
    for name in names:
        at = text.index('.name:           ' + name)
        end = text.find('- .agpr_count', at)
        block = text[text.rindex('- .agpr_count', 0, at):end if end > 0 else len(text)]
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.wavefront_size:\s+(\d+)', block).group(1)) == 64, name
    code = '\n'.join(re.sub(r';.*', '', ln) for ln in text.splitlines())
    assert not re.search(r'\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_', code), 'the unit must not use atomics'
    # one rounding per operation in fp32 (dpn_balance_combine): no fused fp32 multiply-add in the unit (fp64 ones remain: the division's and the
    # square root's own expansions)
    assert not re.search(r'\bv_(fma|fmac|mad|mac)_f32\b', code)
