"""CPU: the host side of the ensemble statistics (dpn_ensemble_accumulate, dpn_ensemble_finish) -- the C ABI additions, the product table, the
threshold table and the numpy restatement (deepphysinet_amd.ensemble) on hand-written member sequences, against numpy on random members, the
seeded mistakes, the loop's new key and the launcher's flags.  Nothing here touches a GPU (the kernels: tests/test_gpu_ensemble.py)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_are_declared_bound_and_exported_and_the_tables_keep_their_sizes():
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib, build
    from deepphysinet_amd.diagnostics import PRODUCTS, VARIABLES
    from deepphysinet_amd.ensemble import ENSEMBLE_PRODUCTS, MAX_THRESHOLDS
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    for name in ('dpn_ensemble_accumulate', 'dpn_ensemble_finish'):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    define = lambda what: int(re.search(r'^#define %s (\d+)' % what, header, flags=re.M).group(1))
    assert define('DPN_ENS_PRODUCTS') == len(ENSEMBLE_PRODUCTS) == _lib.ENS_PRODUCTS == 34 and len(set(ENSEMBLE_PRODUCTS)) == 34
    assert define('DPN_ENS_MAX_THRESHOLDS') == MAX_THRESHOLDS == _lib.ENS_MAX_THRESHOLDS == 16
    assert define('DPN_DIAG_PRODUCTS') == len(PRODUCTS) == 28                        # the diagnostics' table is as it was
    assert ENSEMBLE_PRODUCTS[:28] == PRODUCTS and ENSEMBLE_PRODUCTS[28:] == VARIABLES == ('u', 'v', 'p', 'T', 'q', 'rho')
    # the kernels live in dpn_diag.hip: the unit lists are as they were
    assert [os.path.basename(u[0]) for u in build.MORE_UNITS] == ['dpn_traj.hip'] and len(build.UNITS) == 14
    assert '#include "dpn_ensemble.inc"' in open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_diag.hip')).read()
    assert os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_ensemble.inc') in build.DEPS       # a change of it rebuilds the library


# ------------------------------------------------------------------------------------------------ 2. names and thresholds
def test_ensemble_ids_and_the_forward_they_choose():
    from deepphysinet_amd.ensemble import ENSEMBLE_PRODUCTS, ensemble_ids, reads_coriolis, reads_jacobian
    assert ensemble_ids(ENSEMBLE_PRODUCTS) == list(range(34))
    assert ensemble_ids(['T', 'vorticity', 'T', 'speed', 'rho']) == [31, 18, 31, 25, 33]
    for bad in (['speed', 'gust'], ['t'], ['RHO'], []):
        with pytest.raises(KeyError):
            ensemble_ids(bad)
    no_j = ensemble_ids(['speed', 'rel_humidity', 'u', 'v', 'p', 'T', 'q', 'rho'])
    assert not reads_jacobian(no_j) and not reads_coriolis(no_j)
    for i in list(range(25)) + [27]:
        assert reads_jacobian(no_j + [i]), i
    assert reads_coriolis([19]) and not reads_coriolis([18, 20])


def test_check_thresholds_orders_and_refuses():
    from deepphysinet_amd.ensemble import check_thresholds
    products = ['T', 'speed', 'rel_humidity', 'speed']
    assert check_thresholds(products, None) == ([], []) and check_thresholds(products, {}) == ([], [])
    # the products' order, then the listed order; a repeated name is thresholded in its first column; a scalar is a list of one
    col, val = check_thresholds(products, {'speed': [15.0, 10.0], 'rel_humidity': 0.9, 'T': [273.15]})
    assert col == [0, 1, 1, 2] and val == [float(np.float32(273.15)), 15.0, 10.0, float(np.float32(0.9))]
    with pytest.raises(ValueError, match='vorticity'):
        check_thresholds(products, {'vorticity': [1e-4]})                            # not in the request
    for bad in (float('nan'), float('inf'), -float('inf'), 1e39):                      # (1e39 is not a finite float32)
        with pytest.raises(ValueError, match='finite'):
            check_thresholds(products, {'speed': [1.0, bad]})
    assert len(check_thresholds(products, {'speed': list(range(10)), 'T': list(range(6))})[0]) == 16
    with pytest.raises(ValueError, match='17'):
        check_thresholds(products, {'speed': list(range(10)), 'T': list(range(7))})


# ------------------------------------------------------------------------------------------------ 3. the restatement on hand-written sequences
@pytest.mark.parametrize('name', sorted(EC.hand_cases()))
def test_reference_on_hand_written_sequences(name):
    from deepphysinet_amd.ensemble import ensemble_reference
    values, thr_col, thr_val, expected = EC.hand_cases()[name]
    got = ensemble_reference(values, thr_col, thr_val)
    for key in ('mean', 'spread', 'min', 'max', 'count', 'prob'):
        assert got[key].dtype == (np.int32 if key == 'count' else np.float32), key
        if key in expected:
            assert EC.same(got[key], expected[key]), (key, got[key], expected[key])
    assert got['prob'].shape == (1, len(thr_col))
    assert EC.matches(EC.loop_statistics(values, thr_col, thr_val), expected)          # and so does the plain loop the mistakes are seeded in


@pytest.mark.parametrize('mistake', EC.MISTAKES)
def test_every_seeded_mistake_is_caught_by_a_hand_written_case(mistake):
    caught = [name for name, (values, thr_col, thr_val, expected) in EC.hand_cases().items()
              if not EC.matches(EC.loop_statistics(values, thr_col, thr_val, mistake=mistake), expected)]
    print('%s: caught by %s' % (mistake, caught))
    assert caught, mistake


def test_members_arrive_in_order_and_columns_do_not_mix():
    """The statistics of a column depend on that column's members alone, and on their order only through rounding: a permutation of the members keeps
    count, min, max and prob bit for bit."""
    from deepphysinet_amd.ensemble import ensemble_reference
    g = np.random.default_rng(3)
    v = g.normal(size=(7, 11, 5)).astype(np.float32)
    v[2, 3, 1] = np.nan
    a = ensemble_reference(v, [1, 4], [0.0, 0.5])
    b = ensemble_reference(v[::-1], [1, 4], [0.0, 0.5])
    for key in ('count', 'min', 'max', 'prob'):
        assert EC.same(a[key], b[key]), key
    alone = ensemble_reference(v[:, :, 1:2], [0], [0.0])
    for key in ('mean', 'spread', 'min', 'max', 'count'):
        assert EC.same(alone[key][:, 0], a[key][:, 1]), key
    assert EC.same(alone['prob'][:, 0], a['prob'][:, 0]) and a['count'][3, 1] == 6 and a['count'].sum() == 7 * 11 * 5 - 1


# ------------------------------------------------------------------------------------------------ 4. against numpy
@pytest.mark.parametrize('M', [2, 8, 61])
def test_reference_against_numpy_on_random_members(M):
    """ensemble_reference against numpy's own fp64 two-pass mean and std(ddof=1) on seeded random [M, 257, 6] members with the magnitudes of the
    products (a temperature near 280 with a spread of 3, a vorticity of 1e-4, a humidity, a wind), count / min / max / prob against numpy exactly.
    The bar is the float32 rounding of the two-pass result, times 4 (tests/ensemble_cases.against_numpy); it is computed here on the CPU, not taken
    from the kernel.  The deviation of the float32-rounded two-pass result from the Welford result cannot serve as that bar: it is 0 wherever both
    round to the same float32 (measured: 0 for five of the six figures below, 1.1e-07, one float32 step, for the mean at M = 8), and a float32 result
    cannot be within 0 of an fp64 number.
    Measured (error / bar; mean, then spread): M = 2: 5.873e-08 / 2.349e-07, 4.335e-08 / 1.734e-07; M = 8: 5.396e-08 / 2.158e-07, 4.934e-08 /
    1.973e-07; M = 61: 5.500e-08 / 2.200e-07, 4.620e-08 / 1.848e-07 (the float32 rounding itself: Welford's fp64 error does not show)."""
    from deepphysinet_amd.ensemble import ensemble_reference
    g = np.random.default_rng(100 + M)
    scale = np.array([3.0, 1e-4, 2e-3, 5.0, 1.0, 40.0])
    shift = np.array([280.0, 0.0, 8e-3, 0.0, 1e5, -3.0])
    v = (g.normal(size=(M, 257, 6)) * scale + shift).astype(np.float32)
    thr_col, thr_val = [0, 3, 3], np.array([281.0, 0.0, 5.0], dtype=np.float32)
    ref = ensemble_reference(v, thr_col, thr_val)
    for key, (err, bar, rounded) in EC.against_numpy(v, ref).items():
        print('M = %d, %s: error %.3e, bar %.3e (Welford against the float32-rounded two-pass result: %.3e)' % (M, key, err, bar, rounded))
        assert 0 < bar and err <= bar, (key, err, bar)
    assert EC.same(ref['min'], v.min(axis=0)) and EC.same(ref['max'], v.max(axis=0)) and bool((ref['count'] == M).all())
    want = np.stack([(v[:, :, c] > t).sum(axis=0) / np.float64(M) for c, t in zip(thr_col, thr_val)], axis=1).astype(np.float32)
    assert EC.same(ref['prob'], want)


# ------------------------------------------------------------------------------------------------ 5. the loop's key and the launcher
def test_run_inference_interface_checks_the_ensemble_key_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    cfg['inference_cfg']['ensemble'] = dict(products=['speed', 'gust'])
    torch.manual_seed(0)
    m = builder_models(**cfg)
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(KeyError, match='gust'):                          # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(**nothing)
    for bad in ({'T': [280.0]}, {'speed': [float('nan')]}, {'speed': list(range(17))}):
        m.inference_cfg['ensemble'] = dict(products=['speed', 'rel_humidity'], thresholds=bad)
        with pytest.raises(ValueError):
            m.run_inference_interface(**nothing)
    m.inference_cfg['ensemble'] = dict(products=['speed', 'rel_humidity'], thresholds={'speed': [15.0]})
    with pytest.raises(NotImplementedError):                             # now the missing checkpoint is what stops it
        m.run_inference_interface(**nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_ensemble is None


def test_interface_refuses_a_bad_request_before_anything_runs():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import Lattice
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    lat = Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 3, 2)
    with pytest.raises(ValueError, match='no members'):
        m.ensemble_lattice([], lat, ['speed'])
    with pytest.raises(KeyError, match='gust'):
        m.ensemble_lattice([], lat, ['gust'])
    with pytest.raises(ValueError, match='vorticity'):
        m.ensemble_at([], [1.0], [1.0], [1.0], ['speed'], thresholds={'vorticity': [0.0]})


def test_infer_launcher_flags_reach_the_ensemble_key():
    import infer
    args = infer.parse.parse_args([])
    assert args.ensemble is None and args.ensemble_threshold == [] and infer.ensemble_option(args) is None
    args = infer.parse.parse_args(['--ensemble', 'speed,T', '--synthetic'])
    assert infer.ensemble_option(args) == dict(products=['speed', 'T'], thresholds={})
    args = infer.parse.parse_args(['--ensemble', 'speed,T,rel_humidity', '--ensemble_threshold', 'speed:10,15', '--ensemble_threshold', 'rel_humidity:0.9',
                                   '--ensemble_threshold', 'speed:20.5'])
    assert infer.ensemble_option(args) == dict(products=['speed', 'T', 'rel_humidity'], thresholds={'speed': [10.0, 15.0, 20.5], 'rel_humidity': [0.9]})
    for bad in (['--ensemble_threshold', 'speed:10'], ['--ensemble', 'speed', '--ensemble_threshold', 'speed'],
                ['--ensemble', 'speed', '--ensemble_threshold', ':3']):
        with pytest.raises(SystemExit):
            infer.ensemble_option(infer.parse.parse_args(bad))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "['ensemble'] = ensemble_option(args)" in src                  # ... and the launcher puts it into inference_cfg
