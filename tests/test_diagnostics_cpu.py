"""CPU: the host side of the derived diagnostics (dpn_diagnostics_out) -- the C ABI addition, the product table and its numpy restatement
(deepphysinet_amd.diagnostics) on analytic flows, the seeded mistakes against the GPU tests' bars, the loop's new key and the launcher's flag.
Nothing here touches a GPU (the kernel itself: tests/test_gpu_diagnostics.py)."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import diagnostics_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _physics(**over):
    """A physics table with DpnPhysics' fields (denorm_reference reads attributes only): the identity for every variable unless overridden."""
    ph = types.SimpleNamespace(mean=[0.0] * 6, std=[1.0] * 6, clip_lo=[-1e30] * 6, clip_hi=[1e30] * 6, clip_on=[0] * 6, sq_on=[0] * 6, sq_add=[0.0] * 6)
    for k, v in over.items():
        getattr(ph, k)[v[0]] = v[1]
    return ph


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbol_is_declared_bound_and_exported_and_the_unit_sits_in_front_of_the_causal_one():
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib, build
    from deepphysinet_amd.diagnostics import PRODUCTS
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    assert 'dpn_diagnostics_out' in declared and 'dpn_diagnostics_out' in _lib.EXPORTS and hasattr(_lib.load(), 'dpn_diagnostics_out')
    n_products = int(re.search(r'^#define DPN_DIAG_PRODUCTS (\d+)', header, flags=re.M).group(1))
    assert n_products == len(PRODUCTS) == _lib.DIAG_PRODUCTS == 28 and len(set(PRODUCTS)) == 28
    names = [os.path.basename(u[0]) for u in build.UNITS]
    assert names[12] == 'dpn_diag.hip' and names[-1] == 'dpn_causal.hip' and len(names) == 14 and build.EXP_UNITS == (4,)
    # every product is stated in the header, in id order
    for i, name in enumerate(PRODUCTS[18:], start=18):
        assert re.search(r'^ \*\s+%d\s+%s\s' % (i, name), header, flags=re.M), name


# ------------------------------------------------------------------------------------------------ 2. analytic flows, fp64
def _flow(J_uv, val=None, n=5):
    """val [n, 6] and J [n, 6, 3] with the 2 x 2 block d(u, v) / d(x, y) = J_uv at every point."""
    J = np.zeros((n, 6, 3))
    J[:, :2, :2] = np.asarray(J_uv, dtype=np.float64)
    v = np.zeros((n, 6)) if val is None else np.asarray(val, dtype=np.float64)
    return v, J


def test_reference_on_analytic_flows():
    from deepphysinet_amd.diagnostics import PRODUCTS, diagnostics_reference
    names = ('vorticity', 'abs_vorticity', 'divergence', 'deformation')
    om, a = 3.5e-5, -2.25e-5
    f = np.linspace(4e-5, 1.2e-4, 5).astype(np.float32).astype(np.float64)        # f is an fp32 input of the kernel
    # solid-body rotation u = -om y, v = om x
    d = diagnostics_reference(*_flow([[0.0, -om], [om, 0.0]]), f, names, np.float64)
    assert np.array_equal(d[:, 0], np.full(5, 2 * om)) and np.array_equal(d[:, 1], 2 * om + f) and np.all(d[:, 2] == 0) and np.all(d[:, 3] == 0)
    # pure strain u = a x, v = -a y
    d = diagnostics_reference(*_flow([[a, 0.0], [0.0, -a]]), f, names, np.float64)
    assert np.all(d[:, 0] == 0) and np.array_equal(d[:, 1], f) and np.all(d[:, 2] == 0) and np.array_equal(d[:, 3], np.full(5, 2 * abs(a)))
    # the 18 derivative columns are J itself; omega, the advections and the flux divergence on one hand-computed point
    g = np.random.default_rng(1)
    val, J = g.standard_normal((7, 6)), g.standard_normal((7, 6, 3))
    d = diagnostics_reference(val, J, np.zeros(7), PRODUCTS, np.float64)
    assert d.shape == (7, 28) and np.array_equal(d[:, :18], J.reshape(7, 18))
    u, v, q = val[:, 0], val[:, 1], val[:, 4]
    assert np.array_equal(d[:, 21], J[:, 2, 2] + u * J[:, 2, 0] + v * J[:, 2, 1])
    assert np.array_equal(d[:, 22], -(u * J[:, 3, 0] + v * J[:, 3, 1])) and np.array_equal(d[:, 23], -(u * J[:, 4, 0] + v * J[:, 4, 1]))
    assert np.array_equal(d[:, 24], q * (J[:, 0, 0] + J[:, 1, 1]) + (u * J[:, 4, 0] + v * J[:, 4, 1]))
    assert np.array_equal(d[:, 25], np.sqrt(u * u + v * v))
    # rel_humidity at (p, T, q) = (100 000 Pa, 293.15 K, 0.01): tc = 20, e_s = 611.2 exp(17.67 * 20 / 263.5) = 2 336.947.. Pa,
    # q_s = 0.622 e_s / (p - 0.378 e_s) = 0.01466536.., rh = 0.6818789..
    val = np.array([[0.0, 0.0, 1.0e5, 293.15, 0.01, 1.2]])
    rh = diagnostics_reference(val, np.zeros((1, 6, 3)), [0.0], ['rel_humidity'], np.float64)[0, 0]
    e_s = 611.2 * np.exp(353.4 / 263.5)
    assert abs(e_s - 2336.947) < 0.001 and abs(rh - 0.01 / (0.622 * e_s / (1.0e5 - 0.378 * e_s))) < 1e-12 and abs(rh - 0.6818789) < 1e-7
    # the floor of q_s (1e-6) and a NaN passing through it
    val = np.array([[0.0, 0.0, 1.0e5, 150.0, 0.01, 1.2], [0.0, 0.0, 1.0e5, np.nan, 0.01, 1.2]])
    rh = diagnostics_reference(val, np.zeros((2, 6, 3)), [0.0, 0.0], ['rel_humidity'], np.float64)[:, 0]
    assert rh[0] == 0.01 / 1e-6 and np.isnan(rh[1])


# ------------------------------------------------------------------------------------------------ 3. fp32 against fp64
def test_fp32_and_fp64_restatements_agree_to_fp32_rounding():
    """Random inputs of the shipped normalisation's size.  A product is a chain of at most 8 fp32 operations on intermediates no larger than the
    column's maximum here, each rounding 2^-24 relative: 16 * 2^-24 of the column's maximum covers it.  rel_humidity is the exception: T - 273.15
    cancels a 283 K value to ~10 K (x 30), and that error enters an exponent of order 1 (a relative error of the same size in e_s), then q_s's
    denominator: 256 * 2^-24 = 1.5e-5.  The restatement's deviation on the network's own fields is what the GPU test measures (and prints)."""
    from oracle import dpn_oracle as O
    from deepphysinet_amd.diagnostics import PRODUCTS, denorm_reference, diagnostics_reference
    g = np.random.default_rng(5)
    n = 4000
    out_n = g.standard_normal((n, 6)).astype(np.float32)
    out_n[:, 2] = np.abs(out_n[:, 2]) * 0.25                  # pressures of 0.9 .. 1.0 bar: far above 0.378 e_s, a well-conditioned q_s
    out_n[:, 3] = out_n[:, 3] * 0.5 + 0.5                     # 276 .. 307 K
    jac_n = (g.standard_normal((n, 6, 3)) * 1e-5).astype(np.float32)
    f = (g.random(n) * 1e-4).astype(np.float32)
    ph = _physics()
    ph.mean, ph.std = list(O.OBS_MEAN), list(O.OBS_STD)
    d32 = diagnostics_reference(*denorm_reference(out_n, jac_n, ph, False, np.float32)[::2], f, PRODUCTS, np.float32)
    d64 = diagnostics_reference(*denorm_reference(out_n, jac_n, ph, False, np.float64)[::2], f, PRODUCTS, np.float64)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    err = np.abs(d32.astype(np.float64) - d64).max(axis=0) / np.abs(d64).max(axis=0)
    bound = np.full(28, 16 * 2.0 ** -24)
    bound[26] = 256 * 2.0 ** -24
    print('fp32 restatement against fp64, of the column maximum: %s' % err)
    assert np.all(err <= bound), (err, bound)
    assert np.all(err[18:] > 0)                               # and the two are different arithmetics


# ------------------------------------------------------------------------------------------------ 4. denorm_reference
def test_denorm_reference_forms_and_clip_mask():
    from deepphysinet_amd.diagnostics import denorm_reference
    out_n = np.array([[0.5, -1.0, 2.0, 0.25, 3.0, -0.5], [1.5, 2.0, -3.0, 4.0, 0.5, 0.0]], dtype=np.float32)
    jac_n = np.arange(36, dtype=np.float32).reshape(2, 6, 3) + 1
    # affine: val = out * std + mean, msk = std, J = jac * std
    ph = _physics(std=(0, 2.0), mean=(0, 10.0))
    val, msk, J = denorm_reference(out_n, jac_n, ph, False, np.float64)
    assert np.array_equal(val[:, 0], [11.0, 13.0]) and np.array_equal(msk[:, 0], [2.0, 2.0]) and np.array_equal(J[:, 0], jac_n[:, 0] * 2.0)
    assert np.array_equal(val[:, 1:], out_n[:, 1:]) and np.array_equal(J[:, 1:], jac_n[:, 1:])
    # the squared min_max form: v = out * std + mean, val = v * v + add, d val / d out = (2 v) std
    ph = _physics(std=(4, 0.5), mean=(4, 1.0), sq_on=(4, 1), sq_add=(4, 0.25))
    val, msk, J = denorm_reference(out_n, jac_n, ph, False, np.float64)
    assert np.array_equal(val[:, 4], [2.5 * 2.5 + 0.25, 1.25 * 1.25 + 0.25]) and np.array_equal(msk[:, 4], [2 * 2.5 * 0.5, 2 * 1.25 * 0.5])
    assert np.array_equal(J[:, 4], jac_n[:, 4] * msk[:, 4, None])
    # the clip: on only with with_clip AND clip_on; the mask is 0 outside [lo, hi] and the value clamped, a NaN goes to lo with a zero mask
    ph = _physics(std=(3, 10.0), clip_on=(3, 1), clip_lo=(3, 0.0), clip_hi=(3, 30.0))
    val, msk, J = denorm_reference(out_n, jac_n, ph, True, np.float64)
    assert np.array_equal(val[:, 3], [2.5, 30.0]) and np.array_equal(msk[:, 3], [10.0, 0.0]) and np.all(J[1, 3] == 0) and np.array_equal(J[0, 3], jac_n[0, 3] * 10)
    val, msk, J = denorm_reference(out_n, jac_n, ph, False, np.float64)
    assert np.array_equal(val[:, 3], [2.5, 40.0]) and np.array_equal(msk[:, 3], [10.0, 10.0])
    ph.clip_on[3] = 0
    assert np.array_equal(denorm_reference(out_n, jac_n, ph, True, np.float64)[0][:, 3], [2.5, 40.0])
    ph.clip_on[3] = 1
    bad = out_n.copy()
    bad[0, 3] = np.nan
    val, msk, J = denorm_reference(bad, jac_n, ph, True, np.float32)
    assert val.dtype == np.float32 and val[0, 3] == 0.0 and msk[0, 3] == 0.0 and np.isnan(denorm_reference(bad, jac_n, ph, False)[0][0, 3])
    # fp32: one rounding per operation (the product is rounded before the mean is added)
    ph = _physics(std=(0, 3.0050219), mean=(0, 0.14507187))
    o = np.float32(0.7183)
    want = np.float32(np.float32(o * np.float32(3.0050219)) + np.float32(0.14507187))
    assert denorm_reference(np.full((1, 6), o, np.float32), np.zeros((1, 6, 3), np.float32), ph, False, np.float32)[0][0, 0] == want


# ------------------------------------------------------------------------------------------------ 5. seeded mistakes
_bars_tool = []


def _tool():
    if not _bars_tool:
        spec = importlib.util.spec_from_file_location('diagnostics_bars', os.path.join(ROOT, 'tools', 'diagnostics_bars.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _bars_tool.append(mod)
    return _bars_tool[0]


def test_seeded_mistakes_exceed_the_gpu_tests_bars():
    """The GPU tests' inputs, as the CPU has them: the fp32 oracle's normalised fields and Jacobian at the 1 037 stations of seed 0 (what the kernels
    compute to fp32 rounding).  A restatement with one mistake plays the kernel; it must miss the end-to-end bar of its product (and, for
    rel_humidity, the bar of the kernel test) by a wide margin, while the unmistaken fp32 restatement passes both."""
    from oracle import dpn_oracle as O
    from deepphysinet_amd.diagnostics import PRODUCTS, denorm_reference, diagnostics_reference, product_ids
    c, _, out_n, jac_n, _, _ = _tool().oracle_run(torch.float32)
    ph = _physics()
    ph.mean, ph.std = list(O.OBS_MEAN), list(O.OBS_STD)
    f = c['f'].numpy().reshape(-1)
    v32, _, J32 = denorm_reference(out_n.numpy(), jac_n.numpy(), ph, False, np.float32)
    v64, _, J64 = denorm_reference(out_n.numpy(), jac_n.numpy(), ph, False, np.float64)
    truth = diagnostics_reference(v64, J64, f, PRODUCTS, np.float64)
    good = diagnostics_reference(v32, J32, f, PRODUCTS, np.float32).astype(np.float64)
    bars = DC.oracle_bars()
    scale = np.abs(truth).max(axis=0)
    assert np.all(np.abs(good - truth).max(axis=0) / scale <= bars)
    rh_bar, rh_dev = DC.rel_humidity_bar(good[:, 26].astype(np.float32), truth[:, 26])
    assert 0 < rh_dev < bars[26]
    for name, wrong in DC.seeded_mistakes(v32, J32, f).items():
        i = product_ids([name])[0]
        err = np.abs(wrong.astype(np.float64) - truth[:, i]).max() / scale[i]
        print('%s with its mistake: %.3e of the maximum (bar %.3e)' % (name, err, bars[i]))
        assert err > 100 * bars[i], (name, err, bars[i])
        if name == 'rel_humidity':
            assert err > 100 * rh_bar


# ------------------------------------------------------------------------------------------------ 6. names
def test_product_ids_keep_order_and_repeats_and_refuse_unknown_names():
    from deepphysinet_amd.diagnostics import PRODUCTS, product_ids
    assert PRODUCTS[:18] == tuple('d%s_d%s' % (k, c) for k in ('u', 'v', 'p', 'T', 'q', 'rho') for c in 'xyt')
    assert PRODUCTS[18:] == ('vorticity', 'abs_vorticity', 'divergence', 'omega', 't_advection', 'q_advection', 'q_flux_divergence', 'speed',
                             'rel_humidity', 'deformation')
    assert product_ids(PRODUCTS) == list(range(28))
    assert product_ids(['vorticity', 'dT_dt', 'vorticity', 'du_dx']) == [18, 11, 18, 0]
    for bad in (['vorticity', 'curl'], ['dT_dz'], ['Vorticity'], []):
        with pytest.raises(KeyError):
            product_ids(bad)


# ------------------------------------------------------------------------------------------------ 7. the loop's key
def test_run_inference_interface_checks_export_diagnostic_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False, export_diagnostic=['vorticity', 'curl'])
    torch.manual_seed(0)
    m = builder_models(**cfg)
    with pytest.raises(KeyError, match='curl'):                          # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    m.inference_cfg['log']['export_diagnostic'] = ['vorticity', 'dT_dt']
    with pytest.raises(NotImplementedError):
        m.run_inference_interface(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_diagnostics is None
    m.inference_cfg['log']['export_variable'] = ['T', 'vorticity']       # export_variable keeps its own names and its KeyError
    with pytest.raises(KeyError, match='export_variable'):
        m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[])


# ------------------------------------------------------------------------------------------------ 8. the launcher
def test_infer_launcher_parses_the_diagnostics_flag():
    import infer
    assert infer.parse.parse_args([]).diagnostics is None
    assert infer.parse.parse_args(['--diagnostics', 'vorticity']).diagnostics == ['vorticity']
    assert infer.parse.parse_args(['--diagnostics', 'vorticity,dT_dt,vorticity', '--synthetic']).diagnostics == ['vorticity', 'dT_dt', 'vorticity']


# ------------------------------------------------------------------------------------------------ 9. no CPU fallback
def test_entry_points_refuse_cpu_tensors():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics as IP
    from tests.test_inference_cpu import _HostSampler
    m = builder_models(**ncep_config())
    s = _HostSampler()
    field, fh = torch.zeros(1, 159, 2405), torch.zeros(1, 1, 1)
    lat = s.lattice(hours=0)
    for call in (lambda: m.diagnostics_at(field, s, [1.5], [2.5], [3.5], fh, ['vorticity']),
                 lambda: m.diagnostic_lattice(field, s, lat, fh, ['vorticity', 'speed'])):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(KeyError):                                        # an unknown name is refused before anything else
        m.diagnostics_at(field, s, [1.5], [2.5], [3.5], fh, ['curl'])
    with pytest.raises(KeyError):
        m.diagnostic_lattice(field, s, lat, fh, ['curl'])
    assert IP.DIAG_POINT_BYTES == 4 * (4 + 6 + 6 + 18)
    d = IP.chunk_size(15_000_000, None, IP.DIAG_POINT_BYTES)
    assert d % 128 == 0 and d * IP.DIAG_POINT_BYTES <= IP.INFER_BUDGET_BYTES < (d + 128) * IP.DIAG_POINT_BYTES
