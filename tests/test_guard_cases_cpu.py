"""No GPU: the step guard's host restatement (deepphysinet_amd/guard.py) against the hand-written sequences of tests/guard_cases.py, the seeded
mistakes the table has to catch, the struct's layout against gcc, the new symbol, the refusals of dpn_clip_adam_flat_guard (nothing is launched), and
the option's way from train.py's flags and the configuration to FusedClipAdam's keywords."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import guard_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(seq, mistake=None):
    from deepphysinet_amd import guard as G
    verdicts, states = G.guard_reference(seq.totals, seq.factor, seq.decay, seq.warmup, seq.patience, mistake=mistake)
    ts = [G.effective_step(i + 1, st, mistake=mistake) for i, st in enumerate(states)]
    return verdicts, states, ts


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize('name', GC.SEQUENCE_IDS)
def test_guard_reference_follows_the_hand_written_sequence(name):
    seq = GC.sequence_by_name(name)
    assert GC.mismatches(seq, *_run(seq)) == []


def test_every_seeded_mistake_is_caught_by_the_table():
    from deepphysinet_amd import guard as G
    assert set(GC.CAUGHT_BY) == set(G.MISTAKES)
    assert {'running_on_skip', 'patience_off_by_one', 't_not_reduced', 'inf_passes'} <= set(G.MISTAKES)
    for mistake, name in GC.CAUGHT_BY.items():
        seq = GC.sequence_by_name(name)
        assert GC.mismatches(seq, *_run(seq, mistake)) != [], mistake
        assert any(GC.mismatches(s, *_run(s, mistake)) for s in GC.SEQUENCES)


def test_scripted_sequence_of_the_gpu_test_has_the_expected_verdicts():
    from deepphysinet_amd import guard as G
    for norm in (1.0, 3.7e-3, 2.5e4):
        totals = [np.float32(norm * s) for s in GC.SCRIPT_SCALES]
        verdicts, states = G.guard_reference(totals, GC.SCRIPT['spike_factor'], GC.SCRIPT['spike_decay'], GC.SCRIPT['spike_warmup'], GC.SCRIPT['spike_patience'])
        assert tuple(verdicts) == GC.SCRIPT_VERDICTS
        assert states[-1]['skipped_spike'] == 3 and states[-1]['skipped_nonfinite'] == 0 and states[-1]['seen'] == 2


def test_reference_continues_from_a_given_state_and_saturates_seen():
    from deepphysinet_amd import guard as G
    seq = GC.sequence_by_name('nonfinite')
    _, states = G.guard_reference(seq.totals, seq.factor, seq.decay, seq.warmup, seq.patience)
    _, first = G.guard_reference(seq.totals[:6], seq.factor, seq.decay, seq.warmup, seq.patience)
    _, rest = G.guard_reference(seq.totals[6:], seq.factor, seq.decay, seq.warmup, seq.patience, state=first[-1])
    assert all(G.state_equal(a, b) for a, b in zip(states[6:], rest))
    full = dict(G.zero_state(), seen=2 ** 31 - 1, running=np.float64(1.0))
    v, st = G.guard_step(full, 1.0, 0.0, 0.5, 1, 1)
    assert v == 0 and st['seen'] == 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------- the option
def test_step_guard_option_validates_with_the_abi_rules():
    from deepphysinet_amd.guard import StepGuard
    assert StepGuard().as_dict() == dict(spike_factor=0.0, spike_decay=0.99, spike_warmup=100, spike_patience=5)
    assert StepGuard(spike_factor=None).spike_factor == 0.0 and StepGuard(spike_factor=7, spike_decay=0).spike_decay == 0.0
    for kw in (dict(spike_factor=-1.0), dict(spike_factor=float('nan')), dict(spike_factor=float('inf')), dict(spike_decay=1.0), dict(spike_decay=-0.1),
               dict(spike_decay=float('nan')), dict(spike_warmup=0), dict(spike_patience=0), dict(spike_warmup=1.5), dict(spike_patience=True)):
        with pytest.raises(ValueError, match='step guard'):
            StepGuard(**kw)
    assert StepGuard.from_option(None) is None and StepGuard.from_option(False) is None
    assert StepGuard.from_option(True) == StepGuard()
    assert StepGuard.from_option(dict(spike_factor=10, spike_warmup=3)).as_dict() == dict(spike_factor=10.0, spike_decay=0.99, spike_warmup=3, spike_patience=5)
    with pytest.raises(ValueError, match='unknown keys'):
        StepGuard.from_option(dict(factor=10))


def _interface():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    return builder_models(**ncep_config(), precision='bf16x2')


def test_loop_option_and_build_optimizer_forward_the_guard(monkeypatch):
    from deepphysinet_amd.guard import StepGuard
    from deepphysinet_amd.interface import interface_physics as IP
    m = _interface()
    assert m._step_guard_option({}) is None and m._step_guard_option({'step_guard': False}) is None
    assert m._step_guard_option({'step_guard': True}) == StepGuard()
    assert m._step_guard_option({'step_guard': {'spike_factor': 8.0}}) == StepGuard(spike_factor=8.0)
    with pytest.raises(ValueError, match='unknown keys'):
        m._step_guard_option({'step_guard': {'spike': 8.0}})
    with pytest.raises(ValueError, match='spike_patience'):
        m._step_guard_option({'step_guard': {'spike_factor': 8.0, 'spike_patience': 0}})
    seen = []

    class Recorder:
        ema_decay = None

        def __init__(self, params, **kw):
            seen.append(kw)
            self.param_groups = [{'lr': kw.get('lr', 1e-4)}]
    monkeypatch.setattr(IP, 'FusedClipAdam', Recorder)
    m.build_optimizer()
    assert not any(k.startswith('spike') or k in ('skip_nonfinite', 'step_guard') for k in seen[-1])      # unset: the keywords of before
    m.build_optimizer(step_guard=True)
    assert seen[-1]['skip_nonfinite'] is True and seen[-1]['spike_factor'] == 0.0 and 'step_guard' not in seen[-1]
    m.train_cfg['optimizer']['step_guard'] = {'spike_factor': 10.0, 'spike_warmup': 7}                   # the configuration's path
    m.build_optimizer()
    assert {k: seen[-1][k] for k in StepGuard.KEYS} == dict(spike_factor=10.0, spike_decay=0.99, spike_warmup=7, spike_patience=5)
    assert seen[-1]['skip_nonfinite'] is True
    assert m._step_guard_option({}) == StepGuard(spike_factor=10.0, spike_warmup=7)
    m.build_optimizer(step_guard=None)                                                                     # an override switches it off
    assert 'skip_nonfinite' not in seen[-1]


def test_loop_refuses_the_option_with_another_optimiser(monkeypatch):
    from test_adaptive_cpu import _stub_loop
    m = _interface()
    calls = []
    _stub_loop(m, monkeypatch, calls)                                  # build_optimizer -> torch.optim.SGD
    batches = [{'forecast_h': torch.zeros(1, 1, 1)}] * 2
    with pytest.raises(ValueError, match='FusedClipAdam'):
        m.run_train_interface(samples=batches, device='cpu', num_epoch=1, step_guard=True)
    assert calls == []
    out = m.run_train_interface(samples=batches, device='cpu', num_epoch=1)
    assert out['global_step'] == 2


def test_the_log_step_check_raises_when_every_step_was_skipped():
    m = _interface()

    class Opt:
        def __init__(self, calls, sn, ss):
            self.step_count, self.st = calls, dict(skipped_nonfinite=sn, skipped_spike=ss, running=2.0, last=float('nan'))

        def guard_stats(self):
            return self.st
    row, prev = m._step_guard_log(Opt(1, 0, 0), (0, 0))
    assert row == dict(skipped_nonfinite=0, skipped_spike=0, running_norm=2.0) and prev == (1, 0)
    row, prev = m._step_guard_log(Opt(101, 60, 39), prev)             # 99 of 100 skipped: still moving
    assert prev == (101, 99)
    with pytest.raises(RuntimeError, match=r'all 100 optimiser steps.*skipped_nonfinite 120.*skipped_spike 79'):
        m._step_guard_log(Opt(201, 120, 79), prev)
    assert m._step_guard_log(Opt(201, 120, 79), (201, 199))[1] == (201, 199)      # no call since: nothing to judge


def test_train_py_flags_become_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_launcher', os.path.join(ROOT, 'train.py'))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    arg = lambda *a: train.step_guard_arg(train.parse.parse_args(list(a)))
    assert arg() is None and arg('--skip_nonfinite') is True
    assert arg('--spike_factor', '10') == dict(spike_factor=10.0)
    assert arg('--skip_nonfinite', '--spike_factor', '6', '--spike_warmup', '50', '--spike_patience', '3') == dict(spike_factor=6.0, spike_warmup=50,
                                                                                                                   spike_patience=3)
    with pytest.raises(SystemExit):
        arg('--spike_warmup', '5')


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU
def test_struct_has_the_c_compilers_layout(tmp_path):
    from deepphysinet_amd import _lib
    from deepphysinet_amd.guard import FIELDS
    st = _lib.DpnStepGuard
    assert tuple(f[0] for f in st._fields_) == FIELDS and ctypes.sizeof(st) == 40
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(DpnStepGuard));']
    lines += ['  printf("%s %%zu\\n", offsetof(DpnStepGuard, %s));' % (f[0], f[0]) for f in st._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'guard_layout.c', tmp_path / 'guard_layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    want = dict({f[0]: getattr(st, f[0]).offset for f in st._fields_}, size=ctypes.sizeof(st))
    assert got == want
    assert want['running'] == 24 and want['last'] == 32                # what FusedClipAdam.guard_stats reads as fp64 words 3 and 4


def test_symbol_is_declared_exported_and_bound():
    from deepphysinet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    assert re.search(r'^int\s+dpn_clip_adam_flat_guard\s*\(', header, flags=re.M) and 'typedef struct DpnStepGuard' in header
    assert 'dpn_clip_adam_flat_guard' in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, 'dpn_clip_adam_flat_guard') and lib.dpn_clip_adam_flat_guard.argtypes[16:20] == [ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                                                                           ctypes.c_int]


REFUSALS = ('guard_null', 'factor_negative', 'factor_nan', 'factor_inf', 'decay_1', 'decay_negative', 'decay_nan', 'warmup_0', 'patience_0',
            'n_tensors_0', 'null_params', 'null_grads', 'null_numel', 'null_m', 'null_v', 'null_scratch', 'null_step', 'null_hyper', 'numel_0',
            'numel_2^31', 'n_groups_0', 'n_groups_17', 'group_too_large')


def guard_call_args(why, a):
    """The argument list of dpn_clip_adam_flat_guard for the refusal `why`, from a dict `a` of valid arguments (n, params, grads, numel [list], m, v,
    scratch, step, group_of [list or None], n_groups, hyper, norm, s, base, warm, guard, factor, decay, warmup, patience)."""
    a = dict(a)
    nan, inf = float('nan'), float('inf')
    simple = {'guard_null': ('guard', None), 'factor_negative': ('factor', -1.0), 'factor_nan': ('factor', nan), 'factor_inf': ('factor', inf),
              'decay_1': ('decay', 1.0), 'decay_negative': ('decay', -0.5), 'decay_nan': ('decay', nan), 'warmup_0': ('warmup', 0),
              'patience_0': ('patience', 0), 'n_tensors_0': ('n', 0), 'n_groups_0': ('n_groups', 0), 'n_groups_17': ('n_groups', 17)}
    if why in simple:
        k, v = simple[why]
        a[k] = v
    elif why.startswith('null_'):
        a[why[5:]] = None
    elif why.startswith('numel'):
        a['numel'] = list(a['numel'])
        a['numel'][-1] = 0 if why == 'numel_0' else 2 ** 31
    elif why == 'group_too_large':
        a['group_of'] = list(a['group_of'])
        a['group_of'][-1] = a['n_groups']
    else:
        raise KeyError(why)
    if why in ('n_groups_0', 'n_groups_17', 'group_too_large'):
        assert a['group_of'] is not None
    numel = None if a['numel'] is None else (ctypes.c_int64 * len(a['numel']))(*a['numel'])
    group_of = None if a['group_of'] is None else (ctypes.c_uint8 * len(a['group_of']))(*a['group_of'])
    return (a['n'], a['params'], a['grads'], numel, a['m'], a['v'], a['scratch'], a['step'], group_of, a['n_groups'], a['hyper'], a['norm'], a['s'],
            a['base'], a['warm'], a['guard'], a['factor'], a['decay'], a['warmup'], a['patience'], None)


@pytest.mark.parametrize('why', REFUSALS)
def test_refusals_return_minus_one_before_anything_is_launched(why):
    """Made-up addresses: a refusal launches nothing and dereferences no device pointer, so it is safe without a GPU (as test_ema_cases_cpu does)."""
    from deepphysinet_amd import _lib
    fake = ctypes.c_void_p(4096)
    ptrs = (ctypes.c_void_p * 2)(4096, 8192)
    valid = dict(n=2, params=ptrs, grads=ptrs, numel=[5, 7], m=fake, v=fake, scratch=fake, step=fake, group_of=[0, 1], n_groups=2, hyper=fake, norm=fake,
                 s=None, base=None, warm=0, guard=fake, factor=10.0, decay=0.99, warmup=3, patience=2)
    assert _lib.load().dpn_clip_adam_flat_guard(*guard_call_args(why, valid)) == -1
