"""No GPU: the host side of the window extremes -- deepphysinet_amd/extremes.py, the numpy restatement of dpn_extreme_scan / _begin / _refine and the
driver that runs it over any evaluator.  Analytic evaluators with known extremes (tests/extremes_cases.py), seven seeded mistakes, each of which must
make one of those checks fail, the host refusals, the column names, the launcher's flags, the configuration key, the build lists, and the condition
of the dense-route comparison of tests/test_gpu_extremes.py on the fp64 oracle of the network."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deepphysinet_amd import extremes as X
from tests import extremes_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the driver on analytic evaluators
@pytest.mark.parametrize('check', EC.CHECKS, ids=lambda c: c.__name__)
def test_driver(check):
    check(X.extremes_reference)


@pytest.mark.parametrize('kind', X.MISTAKES)
def test_seeded_mistakes_are_caught(kind):
    """min compared like max; a tie that takes the later node; a bracket that leaves out the step before the best node; the best value overwritten by
    every probe; the speed's slope without its v term; the trapezoid's end nodes at full weight; a closed bracket that is not reported.  Each makes the
    check named in extremes_cases.CAUGHT_BY fail (and that check passes on the code as it is: test_driver)."""
    assert set(EC.CAUGHT_BY) == set(X.MISTAKES)
    with pytest.raises(AssertionError):
        EC.CAUGHT_BY[kind](EC.mistaken(kind))


def test_pieces_compose_to_the_driver_and_leave_their_inputs_alone():
    """scan_reference, begin_reference and refine_reference called by hand on one column give the driver's result; none modifies the state it is
    given; a state's fill never reaches a result."""
    ev = EC.evaluator(lambda h, p: {EC.T: (np.sin(h / 2.0 + p), 0.5 * np.cos(h / 2.0 + p))})
    n, K, R, t0, dt = 5, 6, 3, 1.0, 0.5
    want = X.extremes_reference(ev, n, ['T:min', 'T:mean', 'T:max'], (t0, t0 + K * dt), dt, R)
    ids, senses = X.parse_columns('T:min,T:mean,T:max')[1:]
    state = X.new_state(3, n, fill=-7)
    for k in range(K + 1):
        x, _ = X.products_reference(ev(np.full(n, X.node_hour(t0, dt, k)), np.arange(n))[0], None, X.IDENTITY, False, ids, n)
        before = {key: a.copy() for key, a in state.items()}
        new = X.scan_reference(x, state, senses, k, K)
        assert all(np.array_equal(state[key], before[key]) for key in state)
        state = new
    state, m = X.begin_reference(state, senses, K, t0, dt)
    assert m.shape == (2, n)
    for rnd in range(R + 1):
        out_n, jac_n = ev(m.reshape(-1), np.tile(np.arange(n), 2))
        g, s = X.products_reference(out_n, jac_n, X.IDENTITY, False, [ids[0], ids[2]], n)
        state, (m_next, moved) = X.refine_reference(g, s, state, senses, rnd, t0, dt)
        m = np.where(moved, m_next, m)
    got = X.results_of(state, want['names'])
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert EC.bitwise(got[key], want[key]), key
    assert not (got['value'] == -7).any() and not (got['hour'] == -7).any()


def test_products_follow_the_ensemble_table():
    """The seven products against diagnostics' restatement of the residual body: ids 28..33 are val, 25 the speed; a clipped variable's slope is 0 where
    it is clipped; a row with a NaN among its six fields is NaN in every product, clip or not."""
    from deepphysinet_amd import diagnostics as D
    g = np.random.default_rng(5)
    out_n, jac_n = g.normal(size=(9, 6)).astype(np.float32), g.normal(size=(9, 6, 3)).astype(np.float32)
    out_n[4, 2] = np.nan
    ph = X.Identity((1.0, -2.0, 0.5, 0.0, 0.25, 3.0), (2.0, 0.5, 1.5, 1.0, 0.75, 1.25), (0.0,) * 6, (1.0,) * 6, (0, 0, 1, 1, 1, 1), (0, 0, 0, 0, 1, 0),
                    (0.0, 0.0, 0.0, 0.0, 0.125, 0.0))
    ids = X.parse_columns('u:max,v:max,p:max,T:max,q:max,rho:max,speed:max')[1]
    assert ids == [28, 29, 30, 31, 32, 33, 25]
    for clip in (False, True):
        x, s = X.products_reference(out_n, jac_n, ph, clip, ids, 9)
        val, _, J = D.denorm_reference(out_n, jac_n, ph, clip)
        ok = ~np.isnan(out_n).any(axis=1)
        for k in range(6):
            assert EC.bitwise(x[k][ok], val[ok, k]) and EC.bitwise(s[k], J[:, k, 2])
        assert EC.bitwise(x[6][ok], np.sqrt(val[ok, 0] * val[ok, 0] + val[ok, 1] * val[ok, 1]))
        assert EC.bitwise(s[6], val[:, 0] * J[:, 0, 2] + val[:, 1] * J[:, 1, 2])
        assert np.isnan(x[:, 4]).all() and np.isfinite(x[:, ok]).all()
        if clip:
            out = (val[:, 3] <= 0.0) | (val[:, 3] >= 1.0)
            assert out.any() and (s[3][out] == 0).all() and (x[3][ok] >= 0).all() and (x[3][ok] <= 1).all()


# ------------------------------------------------------------------------------------------------ 2. names and host refusals
def test_column_names():
    assert X.parse_columns('T:max,T:min,speed:max') == (['T:max', 'T:min', 'speed:max'], [31, 31, 25], [X.MAX, X.MIN, X.MAX])
    assert X.parse_columns(['rho:mean', 'u:min', 'rho:mean'])[1:] == ([33, 28, 33], [X.MEAN, X.MIN, X.MEAN])
    assert X.refined_columns([X.MEAN, X.MIN, X.MAX, X.MEAN]) == [1, 2]
    for bad in ('gust:max', 'T', 'T:median', 'vorticity:max', ':max', 'T:', [], ''):
        with pytest.raises(KeyError):
            X.parse_columns(bad)
    assert len(X.parse_columns(['T:max'] * 32)[0]) == 32
    with pytest.raises(ValueError):
        X.parse_columns(['T:max'] * 33)


def test_host_refusals_and_the_clock():
    ok = dict(columns='T:max', window=(0.0, 24.0), scan_hours=1.0, refine=10, hours_top=24)
    r = X.check_request(**ok)
    assert (r.t0, r.dt, r.K, r.R) == (0.0, 1.0, 24, 10) and r.names == ['T:max']
    for kw in (dict(window=(0.0, 24.5)), dict(window=(-1.0, 3.0)), dict(window=(5.0, 5.0)), dict(window=(6.0, 5.0)), dict(window=(0.0, float('nan'))),
               dict(window=(0.0,)), dict(window=3.0), dict(scan_hours=0.0), dict(scan_hours=-1.0), dict(scan_hours=float('inf')), dict(scan_hours=2.0 ** -11),
               dict(scan_hours=100.0), dict(window=(0.0, 24.0), scan_hours=2.0 ** -10), dict(refine=-1), dict(refine=33), dict(refine=2.5), dict(refine=True)):
        with pytest.raises(ValueError):
            X.check_request(**{**ok, **kw})
    with pytest.raises(KeyError):
        X.check_request(**{**ok, 'columns': 'gust:max'})
    assert X.check_request(**{**ok, 'refine': 0}).R == 0 and X.check_request(**{**ok, 'refine': 32}).R == 32
    assert X.check_request(**{**ok, 'window': (3.0, 4.0)}).K == 1 and X.check_request(**{**ok, 'scan_hours': 24.0}).K == 1
    # a step that does not divide the window in fp64: K steps of (t1 - t0) / K, and node K never passes t1 (it would leave the coarse cube)
    for window, step in (((0.0, 24.0), 0.1), ((0.3, 23.9), 0.7), ((1.0, 2.0), 1.0 / 3.0), ((0.0, 24.0), 5.0)):
        r = X.check_request('T:max', window, step, 3, 24)
        assert r.K == int(round((window[1] - window[0]) / step)) and X.node_hour(r.t0, r.dt, r.K) <= window[1]
        assert window[1] - X.node_hour(r.t0, r.dt, r.K) <= 4 * np.spacing(window[1]) and abs(r.dt - (window[1] - window[0]) / r.K) <= 1e-12
    assert X.node_hour(0.1, 0.7, 3) == np.float64(0.1) + np.float64(3.0) * np.float64(0.7)


def test_spells_refuse_a_bad_clock_in_the_extremes_words():
    """One clock check serves both products: for the sixteen bad clocks of tests/test_spells_cpu.py the message of spells.check_request is the
    message of extremes.check_request with its first 'extremes:' replaced by 'spells:', and it names the offending value."""
    from deepphysinet_amd import spells as S
    ok = dict(window=(0.0, 24.0), scan_hours=1.0, refine=10, hours_top=24)
    bad = (dict(window=(0.0, 24.5)), dict(window=(-1.0, 3.0)), dict(window=(5.0, 5.0)), dict(window=(6.0, 5.0)), dict(window=(0.0, float('nan'))),
           dict(window=(0.0,)), dict(window=3.0), dict(scan_hours=0.0), dict(scan_hours=-1.0), dict(scan_hours=float('inf')), dict(scan_hours=2.0 ** -11),
           dict(scan_hours=100.0), dict(refine=-1), dict(refine=33), dict(refine=2.5), dict(refine=True))
    assert len(bad) == 16
    for kw in bad:
        with pytest.raises(ValueError) as of_extremes:
            X.check_request('T:max', **{**ok, **kw})
        with pytest.raises(ValueError) as of_spells:
            S.check_request('T:below:273.15', **{**ok, **kw})
        text = str(of_extremes.value)
        assert text.startswith('extremes: ') and text.count('extremes:') == 1 and repr(next(iter(kw.values()))) in text
        assert str(of_spells.value) == text.replace('extremes:', 'spells:', 1)


# ------------------------------------------------------------------------------------------------ 3. the loop's key and the launcher
def test_run_inference_interface_checks_the_extremes_key_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    cfg['inference_cfg']['extremes'] = dict(columns=['T:max', 'gust:max'], window=(0.0, 24.0))
    torch.manual_seed(0)
    m = builder_models(**cfg)
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(KeyError, match='gust'):                          # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(**nothing)
    for bad in (dict(window=(5.0, 5.0)), dict(window=(0.0, 24.0), scan_hours=0.0), dict(window=(0.0, 24.0), refine=40), dict(window=(0.0, 24.0), lonlat=[])):
        m.inference_cfg['extremes'] = dict(columns=['T:max'], **bad)
        with pytest.raises(ValueError):
            m.run_inference_interface(**nothing)
    m.inference_cfg['extremes'] = dict(columns=['T:max', 'speed:max'], window=(0.0, 24.0), lonlat=[(100.5, 30.25)])
    with pytest.raises(NotImplementedError):                             # now the missing checkpoint is what stops it
        m.run_inference_interface(**nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_extremes is None


def test_interface_refuses_a_bad_request_before_anything_runs():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import Lattice
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    field = torch.zeros(1, 159, 2405)
    with pytest.raises(RuntimeError, match='HIP device'):                # a host tensor never reaches a kernel
        m.extremes_at(field, None, [1.0], [1.0], (0.0, 24.0), None, ['T:max'])
    with pytest.raises(RuntimeError, match='HIP device'):
        m.extreme_lattice(field, None, Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 3, 1), (0.0, 24.0), None, ['T:max'])


def test_infer_launcher_flags_reach_the_extremes_key():
    import infer
    args = infer.parse.parse_args([])
    assert args.extremes is None and args.extreme_window is None and infer.extremes_option(args) is None
    args = infer.parse.parse_args(['--extremes', 'T:max,T:min,speed:max', '--extreme_window', '0,24', '--synthetic'])
    assert infer.extremes_option(args) == dict(columns=['T:max', 'T:min', 'speed:max'], window=(0.0, 24.0), scan_hours=1.0, refine=10)
    args = infer.parse.parse_args(['--extremes', 'q:mean', '--extreme_window', '6,18.5', '--extreme_scan', '0.5', '--extreme_refine', '4'])
    assert infer.extremes_option(args) == dict(columns=['q:mean'], window=(6.0, 18.5), scan_hours=0.5, refine=4)
    for bad in (['--extreme_window', '0,24'], ['--extremes', 'T:max'], ['--extremes', 'T:max', '--extreme_window', '0,12,24']):
        with pytest.raises(SystemExit):
            infer.extremes_option(infer.parse.parse_args(bad))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "['extremes'] = extremes_option(args)" in src                  # ... and the launcher puts it into inference_cfg


# ------------------------------------------------------------------------------------------------ 4. the build lists and the binding
def test_kernels_ride_in_the_diagnostics_unit_and_are_bound():
    """No translation unit is added: build.ALL_UNITS is what it was, the new include file is a dependency of the library, dpn_diag.hip includes it,
    and the three entry points are declared, bound and linked."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import build as B
    assert [os.path.basename(u[0]) for u in B.ALL_UNITS] == [
        'dpn_point.hip', 'dpn_wgrad.hip', 'dpn_encoder.hip', 'dpn_sampler.hip', 'dpn_fp8.hip', 'dpn_encoder_chain.hip', 'dpn_eval.hip', 'dpn_adaptive.hip',
        'dpn_residual.hip', 'dpn_gemm.hip', 'dpn_optim.hip', 'dpn_balance.hip', 'dpn_diag.hip', 'dpn_causal.hip', 'dpn_traj.hip']
    csrc = os.path.join(B.HERE, 'csrc')
    assert os.path.join(csrc, 'dpn_extreme.inc') in B.DEPS and not os.path.exists(os.path.join(csrc, 'dpn_extreme.hip'))
    diag = open(os.path.join(csrc, 'dpn_diag.hip')).read()
    assert '#include "dpn_extreme.inc"' in diag and '#include "dpn_sample_point.h"' in diag
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    lib = ctypes.CDLL(B.build_library())                                  # linked in (no GPU needed to load the library)
    for name, n_args in (('dpn_extreme_scan', 22), ('dpn_extreme_begin', 18), ('dpn_extreme_refine', 23)):
        assert 'int %s(' % name in header and len(L.EXPORTS[name][1]) == n_args and hasattr(lib, name)
    assert 'typedef struct DpnExtremeState' in header and ctypes.sizeof(L.DpnExtremeState) == 7 * 8
    for name, value in (('DPN_EXT_MAX_COLUMNS', L.EXT_MAX_COLUMNS), ('DPN_EXT_MEAN', L.EXT_MEAN), ('DPN_EXT_BAD_SCAN', L.EXT_BAD_SCAN),
                        ('DPN_EXT_STOPPED', L.EXT_STOPPED), ('DPN_EXT_AT_START', L.EXT_AT_START), ('DPN_EXT_AT_END', L.EXT_AT_END)):
        assert '#define %s' % name in header and int(header.split('#define %s' % name)[1].split()[0]) == value
    assert (X.MAX, X.MIN, X.MEAN) == (L.EXT_MAX, L.EXT_MIN, L.EXT_MEAN) and X.MAX_COLUMNS == L.EXT_MAX_COLUMNS
    assert (X.OK, X.BAD_SCAN, X.STOPPED, X.AT_START, X.AT_END) == (L.EXT_OK, L.EXT_BAD_SCAN, L.EXT_STOPPED, L.EXT_AT_START, L.EXT_AT_END)


# ------------------------------------------------------------------------------------------------ 5. the condition of the dense-route comparison
def test_sampler_restatement_is_trilinear():
    """extremes_cases.sample_reference at the cube's own nodes returns the cube, between two of them their mean, outside it NaN."""
    cube = EC.host_world(EC.DENSE_SEED)[0]
    x, y, t, cd = EC.sample_reference(cube, [8.0, 10.0, 8.0, 300.0], [12.0, 12.0, 14.0, 12.0], [6.0, 6.0, 9.0, 6.0])
    assert np.array_equal(cd[0], cube[:, 3, 2, 1]) and np.isnan(cd[3]).all()
    assert np.allclose(cd[1], 0.5 * (cube[:, 3, 2, 1] + cube[:, 3, 3, 1]), rtol=0, atol=1e-6)
    assert np.allclose(cd[2], 0.25 * (cube[:, 3, 2, 1] + cube[:, 3, 2, 2] + cube[:, 4, 2, 1] + cube[:, 4, 2, 2]), rtol=0, atol=1e-6)
    assert (x[0], y[2], t[2]) == (216000.0, 378000.0, 32400.0)


def test_dense_route_condition_holds_on_the_fp64_oracle():
    """Seed extremes_cases.DENSE_SEED, stations DENSE_STATIONS: with the fp64 oracle of the network as the evaluator, extremes_reference (hourly scan,
    R = 10, everything in fp64) equals or exceeds the one-minute dense extreme of T:max, T:min and speed:max at EVERY station -- the condition under
    which tests/test_gpu_extremes.py compares the two routes on the device.  The stations are chosen for it: the slope the bisection reads is the
    network's d/dt at fixed interpolated input, not the slope of a station's series, whose coarse-cube part changes with the hour too."""
    n = len(EC.DENSE_STATIONS)
    assert n == 8 and len(set(EC.DENSE_STATIONS)) == 8
    ev, ph = EC.oracle_evaluator(EC.DENSE_SEED, EC.DENSE_STATIONS), EC.OraclePhysics()
    minutes = np.arange(1441) / 60.0
    out_n, _ = ev(np.repeat(minutes, n), np.tile(np.arange(n), minutes.size), want_jac=False)
    values, _ = X.products_reference(out_n, None, ph, False, [28, 29, 30, 31, 32, 33], out_n.shape[0], np.float64)
    dense = np.stack(EC.dense_extremes(values.T.reshape(minutes.size, n, 6)), axis=1)
    r = X.extremes_reference(ev, n, list(EC.DENSE_COLUMNS), (0.0, 24.0), 1.0, 10, physics=ph, dtype=np.float64)
    print('refined', r['value'].tolist(), 'dense', dense.tolist(), 'hours', r['hour'].tolist(), 'status', r['status'].tolist())
    assert np.isfinite(dense).all() and (r['status'] != X.BAD_SCAN).all() and (r['status'] != X.STOPPED).all()
    # Where both routes evaluate the same hour (an extreme on a scan node) they do so in batches of different sizes, and a BLAS may sum a row of a
    # larger batch in another order: the oracle's own fp64 evaluation noise, 1e-12 of the value (a few thousand fp64 steps; the gains, where the
    # refinement beats the lattice, are 1e-5 of it), is not a shortfall.
    noise = 1e-12 * np.abs(dense)
    short = (dense - r['value']) * np.array([1.0, -1.0, 1.0])
    assert (short <= noise).all(), short.max(axis=0)
    assert (short < -1e-4).any()                                         # and somewhere the refinement does better than the one-minute lattice
