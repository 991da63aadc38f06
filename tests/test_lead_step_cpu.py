"""CPU: the host side of the trained lead-batch step -- the fp64 restatement of dpn_step_finish_batch (deepphysinet_amd.lead_step), the size function
of the block rows, the loops' grouping, the refusals of training_step_batch and of the loops, train.py --lead_batch, and the build of the unit that
holds the kernels: it cross-compiles for gfx950 and neither kernel spills or uses scratch."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _interface():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    return builder_models(**ncep_config())


def _sample(n_inter=4, n_margin=6, **extra):
    z = torch.zeros
    b = {'field_data': z(1, 159, 2405), 'forecast_h': z(1, 1, 1), 'margin_data': z(n_margin, 6), 'margin_input_data': z(n_margin, 6),
         'inter_data': z(n_inter, 6)}
    b.update({'margin_' + k: z(n_margin, 1) for k in 'xytf'})
    b.update({'inter_' + k: z(n_inter, 1) for k in 'xytf'})
    b.update(extra)
    return b


# ------------------------------------------------------------------------------------------------ the finish kernel's restatement
def test_finish_reference_on_hand_made_rows_layout_and_order_of_the_total():
    from deepphysinet_amd.lead_step import LOSSES, finish_reference
    # n_inter = 300 (2 blocks), n_m = 513 (3 blocks): 5 rows of 7
    rows = np.zeros((5, 7))
    rows[0, :6] = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    rows[1, :6] = [0.5, 0.25, 1.0, 2.0, 4.0, 8.0]
    rows[2:, :6] = np.arange(18, dtype=np.float64).reshape(3, 6) + 1.0
    rows[2:, 6] = [10.0, 20.0, 0.78]
    factors = [2.0, 4.0, 0.5, 8.0, 1.0, 16.0]
    out = finish_reference(rows, 300, 813, factors, 3.0)
    assert LOSSES == 16 and out.shape == (16,) and out.dtype == np.float32
    f32 = np.float32
    inter = [f32(f32(s / 300.0) * fac) for s, fac in zip([1.5, 2.25, 4.0, 6.0, 9.0, 14.0], factors)]
    margin = [f32(f32((1.0 + e + 7.0 + e + 13.0 + e) / 513.0) * fac) for e, fac in zip(range(6), factors)]
    np.testing.assert_array_equal(out[0:6], inter)
    np.testing.assert_array_equal(out[7:13], margin)
    for base, t in ((0, inter), (7, margin)):                       # the reference's order: u + v + energy + continuity + vapour + gas
        assert out[base + 6] == ((((t[0] + t[1]) + t[3]) + t[2]) + t[4]) + t[5]
    assert out[14] == f32(30.78 / (6.0 * 513.0)) * f32(3.0)
    assert out[15] == (out[14] + out[6]) + out[13]
    # an order that matters: in fp32, (data + interior) + margin differs from data + (interior + margin) here
    big = np.zeros((2, 7))
    big[0, 0], big[1, 0], big[1, 6] = 2.0 ** 24, 1.0, 6.0
    o = finish_reference(big, 1, 2, [1.0] * 6, 1.0)
    assert o[6] == f32(2.0 ** 24) and o[13] == 1.0 and o[14] == 1.0
    assert o[15] == f32(2.0 ** 24) and (o[14] + o[13]) + o[6] == f32(2.0 ** 24 + 2.0)
    # reduction 'sum': no division by the group's point count
    s = finish_reference(rows, 300, 813, factors, 3.0, reduce_sum=True)
    np.testing.assert_array_equal(s[0:6], [f32(f32(v) * fac) for v, fac in zip([1.5, 2.25, 4.0, 6.0, 9.0, 14.0], factors)])
    assert s[14] == out[14]
    # more than 64 rows: lane l adds rows l, l + 64, ... before the tree -- exact on integers, whatever the order
    many = np.zeros((1 + 130, 7))
    many[0, :6] = 1.0
    many[1:, 2] = np.arange(130)
    many[1:, 6] = 1.0
    m = finish_reference(many, 256, 256 + 130 * 256, [1.0] * 6, 1.0)
    assert m[9] == f32(f32(130 * 129 / 2 / (130 * 256.0))) and m[14] == f32(130.0 / (6.0 * 130 * 256))
    with pytest.raises(ValueError):
        finish_reference(rows[:4], 300, 813, factors, 3.0)
    with pytest.raises(ValueError):
        finish_reference(rows, 0, 813, factors, 3.0)


def test_step_rows_doubles():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.build import build_library
    from deepphysinet_amd.lead_step import rows_doubles
    if not os.path.exists(shutil.which('hipcc') or '/opt/rocm/bin/hipcc'):
        pytest.skip('hipcc not available')
    build_library()
    lib = L.load()
    for (n_inter, n), want in (((1, 2), 14), ((255, 512), 21), ((256, 512), 14), ((300, 813), 35), ((0, 5), 0), ((-1, 5), 0), ((5, 5), 0), ((6, 5), 0)):
        assert lib.dpn_step_rows_doubles(n_inter, n) == want == rows_doubles(n_inter, n), (n_inter, n)
    assert L.STEP_LOSSES == 16
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name, n_args in (('dpn_step_rows_doubles', 2), ('dpn_step_residual', 15), ('dpn_step_finish_batch', 8)):
        assert len(L.EXPORTS[name][1]) == n_args
        decl = re.search(r'^int(?:64_t)? %s\((.*?)\);' % name, header, re.M | re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', decl).split(',')) == n_args, name


# ------------------------------------------------------------------------------------------------ grouping
def test_lead_groups():
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics
    groups = InterfacePhysics._lead_groups
    five = [_sample(tag=i) for i in range(5)]
    assert [[b['tag'] for b in g] for g in groups(five, 2)] == [[0, 1], [2, 3], [4]]
    assert [[b['tag'] for b in g] for g in groups(five, 1)] == [[0], [1], [2], [3], [4]]
    assert [[b['tag'] for b in g] for g in groups(five, 8)] == [[0, 1, 2, 3, 4]]
    # a change of the point counts (interior or margin) cuts a group
    mixed = [_sample(tag=0), _sample(tag=1), _sample(tag=2), _sample(n_inter=5, tag=3), _sample(n_inter=5, tag=4), _sample(n_inter=5, n_margin=7, tag=5)]
    assert [[b['tag'] for b in g] for g in groups(mixed, 3)] == [[0, 1, 2], [3, 4], [5]]
    assert [[b['tag'] for b in g] for g in groups(mixed, 2)] == [[0, 1], [2], [3, 4], [5]]
    assert list(groups([], 4)) == []
    assert [len(g) for g in groups(iter(five), 2)] == [2, 2, 1]              # any iterable, consumed lazily
    with pytest.raises(ValueError):
        list(groups(five, 0))


# ------------------------------------------------------------------------------------------------ refusals
def test_training_step_batch_refuses_host_tensors_unequal_point_counts_and_point_weights():
    m = _interface()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.training_step_batch([_sample(), _sample()], None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.training_step_batch([_sample()], None, with_pde=False)
    with pytest.raises(ValueError, match='equal point counts'):
        m.training_step_batch([_sample(), _sample(n_inter=5)], None)
    with pytest.raises(ValueError, match='equal point counts'):
        m.training_step_batch([_sample(), _sample(n_margin=7)], None, with_pde=False)
    with pytest.raises(NotImplementedError, match='inter_w'):
        m.training_step_batch([_sample(), _sample(inter_w=torch.ones(4))], None)
    with pytest.raises(ValueError, match='no samples'):
        m.training_step_batch([], None)


def test_step_losses_batch_checks_before_any_launch():
    from deepphysinet_amd.point_path import PointConfig, step_losses_batch
    z = torch.zeros
    B, n, n_inter = 2, 10, 4
    args = lambda lab_rows: (z(B, n), z(B, n), z(B, n), z(B, n), z(B, n, 6), z(B, lab_rows, 6), z(B, 256, 2700), z(B, 6, 256), [])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        step_losses_batch(PointConfig(), n_inter, *args(n - n_inter))
    with pytest.raises(TypeError):                                        # no such argument: weights are for one field at a time
        step_losses_batch(PointConfig(), n_inter, *args(n - n_inter), causal=None)


@pytest.mark.parametrize('dist', (False, True))
def test_the_loops_refuse_lead_batch_with_causal_weights_or_balancing_before_any_step(dist):
    m = _interface()
    run = m.run_train_interface_dist if dist else m.run_train_interface

    def no_samples(epoch):
        raise AssertionError('the loop asked for samples')
    m.training_step = m.training_step_batch = m.build_optimizer = no_samples
    for bad in (dict(causal_weights=dict(eps=1.0)), dict(balance_losses=True), dict(causal_weights=dict(eps=1.0), balance_losses=dict(every=2))):
        with pytest.raises(NotImplementedError, match='lead_batch=2'):
            run(samples=no_samples, lead_batch=2, device='cpu', **bad)
    m.train_cfg['train_data']['lead_batch'] = 3                           # the config's own entry
    with pytest.raises(NotImplementedError, match='lead_batch=3'):
        run(samples=no_samples, device='cpu', balance_losses=True)
    with pytest.raises(ValueError, match='lead_batch'):
        run(samples=no_samples, device='cpu', lead_batch=0)
    assert m._lead_batch_option({}) == 3 and m._lead_batch_option({'lead_batch': 1, 'causal_weights': dict(eps=1.0), 'balance_losses': True}) == 1
    assert m._lead_batch_option({'causal_weights': None, 'balance_losses': False}) == 3              # options that are off do not count
    del m.train_cfg['train_data']['lead_batch']
    assert m._lead_batch_option({'balance_losses': True}) == 1


def test_train_py_lead_batch_parses():
    code = ("import sys, runpy; sys.argv = ['train.py'] + sys.argv[1:]; ns = runpy.run_path(%r, run_name='launcher'); "
            "a = ns['parse'].parse_args(); print('lead_batch', a.lead_batch)" % os.path.join(ROOT, 'train.py'))
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-c', code, '--synthetic', '--lead_batch', '4'], check=True, capture_output=True, text=True, env=env).stdout
    assert 'lead_batch 4' in out
    out = subprocess.run([sys.executable, '-c', code, '--synthetic'], check=True, capture_output=True, text=True, env=env).stdout
    assert 'lead_batch None' in out


# ------------------------------------------------------------------------------------------------ build
def test_the_step_kernels_cross_compile_without_spills_or_scratch(tmp_path):
    from deepphysinet_amd.build import COMMON, UNITS
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    unit = [u for u in UNITS if os.path.basename(u[0]) == 'dpn_residual.hip']         # the step kernel is an instantiation of dpn_residual_kernel
    assert len(unit) == 1 and os.path.basename(UNITS[-1][0]) == 'dpn_causal.hip'
    src, flags, obj = unit[0]
    asm = str(tmp_path / (obj + '.s'))
    subprocess.run([hipcc, *[f for f in COMMON if f != '-fPIC'], *flags, '--cuda-device-only', '-S', '-I' + os.path.join(ROOT, 'include'), src, '-o', asm],
                   check=True, capture_output=True)
    text = open(asm).read()
    names = re.findall(r'\.name:\s+(\S*dpn_residual_kernel\S*ResStepArgs\S*|\S*dpn_step_finish_kernel\S*)', text)
    assert len(names) == 2, names
    for name in names:
        at = text.index('.name:           ' + name)
        end = text.find('- .agpr_count', at)
        block = text[text.rindex('- .agpr_count', 0, at):end if end > 0 else len(text)]
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.wavefront_size:\s+(\d+)', block).group(1)) == 64, name
    assert 's_swappc_b64' not in text and 'scratch_' not in text
    assert not re.search(r'\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_', text), 'the unit must not use atomics'
