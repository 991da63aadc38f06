"""No GPU: the host side of the verification against observations (dpn_verify_accumulate, dpn_verify_pool, dpn_verify_finish) -- the C ABI additions
and struct layouts, the product table, the threshold parser, the pooling plan, the numpy restatement (deepphysinet_amd/verification.py) against the
exact tables of tests/verify_cases.py, pooling against accumulating the pooled pairs, chunking, the seeded mistakes, every host refusal, the loop's
new key, the report reader and the launcher's flags.  The kernels: tests/test_gpu_verify.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import verify_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(case, groups=None, chunks=None):
    """The restatement over a case: accumulate date by date (in `chunks` of points), pool when groups are given, finish."""
    from deepphysinet_amd import verification as VF
    x, b, o = case['x'], case['b'], case['o']
    thr_col, thr_val, thr_side = case['thr']
    M, n, P = x.shape
    st = VF.verify_state_zeros(n, P, len(thr_col))
    for m in range(M):
        for first, stop in chunks or [(0, n)]:
            VF.verify_accumulate_reference(st, x[m, first:stop], b[m, first:stop], o[m, first:stop], thr_col, thr_val, thr_side, first)
    if groups is not None:
        st = VF.verify_pool_reference(st, *VF.pool_plan(groups), thr_col)
    return VF.verify_finish_reference(st, thr_col), st


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_are_declared_bound_and_exported_and_the_structs_follow_the_header():
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib, build, verification as VF
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    for name in ('dpn_verify_accumulate', 'dpn_verify_pool', 'dpn_verify_finish'):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    define = lambda what: int(re.search(r'^#define %s (\d+)' % what, header, flags=re.M).group(1))
    assert define('DPN_VERIFY_MAX_COLUMNS') == VF.MAX_COLUMNS == _lib.VERIFY_MAX_COLUMNS == 16
    assert define('DPN_VERIFY_MAX_THRESHOLDS') == VF.MAX_THRESHOLDS == _lib.VERIFY_MAX_THRESHOLDS == 16
    assert (define('DPN_VERIFY_ABOVE'), define('DPN_VERIFY_BELOW')) == (VF.ABOVE, VF.BELOW) == (_lib.VERIFY_ABOVE, _lib.VERIFY_BELOW) == (0, 1)
    for struct in (VF.DpnVerifyState, VF.DpnVerifyOut):                  # the members of the typedef, in its order, every one a pointer
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct.__name__, struct.__name__), header, flags=re.S).group(1)
        members = [n for decl in body.split(';') for n in re.findall(r'\*\s*(\w+)', decl)]
        assert members == [n for n, _ in struct._fields_], struct.__name__
        assert ctypes.sizeof(struct) == 8 * len(members) and all(t is ctypes.c_void_p for _, t in struct._fields_)
        assert [getattr(struct, n).offset for n in members] == [8 * i for i in range(len(members))]
    assert len(VF.DpnVerifyState._fields_) == 14 and len(VF.DpnVerifyOut._fields_) == 20
    assert _lib.DpnVerifyState is VF.DpnVerifyState and _lib.DpnVerifyOut is VF.DpnVerifyOut
    res, args = _lib.EXPORTS['dpn_verify_accumulate']
    assert res is ctypes.c_int and len(args) == 16 and len(_lib.EXPORTS['dpn_verify_pool'][1]) == 11 and len(_lib.EXPORTS['dpn_verify_finish'][1]) == 9
    assert '#include "dpn_verify.inc"' in open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_diag.hip')).read()
    assert os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_verify.inc') in build.DEPS       # a change of it rebuilds the library
    text = open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_verify.inc')).read()
    assert 'atomic' not in text.replace('No atomics', '').replace('no atomics', '') and '__shared__' not in text


# ------------------------------------------------------------------------------------------------ 2. names, thresholds, plan
def test_verify_ids_are_the_value_products_of_the_ensemble_table():
    from deepphysinet_amd.ensemble import ensemble_ids
    from deepphysinet_amd.verification import VERIFY_PRODUCTS, verify_ids
    assert VERIFY_PRODUCTS == ('u', 'v', 'p', 'T', 'q', 'rho', 'speed', 'rel_humidity')
    assert verify_ids(VERIFY_PRODUCTS) == [28, 29, 30, 31, 32, 33, 25, 26] == ensemble_ids(VERIFY_PRODUCTS)
    assert verify_ids(['T', 'speed', 'T']) == [31, 25, 31]
    for bad in (['vorticity'], ['dT_dt'], ['T', 'gust'], []):
        with pytest.raises(KeyError):
            verify_ids(bad)


def test_threshold_parser():
    from deepphysinet_amd.verification import ABOVE, BELOW, check_thresholds
    assert check_thresholds(['T'], None) == ([], [], [])
    assert check_thresholds(['T', 'speed'], {'speed': 10, 'T': ('below', 273.15)}) == ([0, 1], [float(np.float32(273.15)), 10.0], [BELOW, ABOVE])
    assert check_thresholds(['speed', 'T', 'speed'], {'speed': [10, 15.5], 'T': [('below', [270, 273]), 300.0, ('above', 305)]}) == \
        ([0, 0, 1, 1, 1, 1], [10.0, 15.5, 270.0, 273.0, 300.0, 305.0], [ABOVE, ABOVE, BELOW, BELOW, ABOVE, ABOVE])
    assert check_thresholds(['T'], {'T': np.arange(16.0)})[0] == [0] * 16
    for bad in ({'q': 1.0}, {'T': float('nan')}, {'T': [1.0, float('inf')]}, {'T': 1e39}, {'T': ('sideways', 1.0)}, {'T': ('below',)},
                {'T': ('below', 1.0, 2.0)}, {'T': np.arange(17.0)}, {'T': ('below', 'cold')}, {'T': [('below', float('nan'))]}):
        with pytest.raises(ValueError):
            check_thresholds(['T'], bad)


def test_pool_plan():
    from deepphysinet_amd.verification import pool_plan
    order, seg = pool_plan([2, 0, 2, 1, 0, 4])
    assert order.tolist() == [1, 4, 3, 0, 2, 5] and order.dtype == np.int32                 # stable: ascending inside a group
    assert seg.tolist() == [0, 2, 3, 5, 5, 6] and seg.dtype == np.int64                     # group 3 is empty
    assert pool_plan([0, 0], n_groups=3)[1].tolist() == [0, 2, 2, 2]
    assert pool_plan(torch.tensor([1, 0]).numpy())[0].tolist() == [1, 0] and pool_plan(np.array([1.0, 0.0]))[0].tolist() == [1, 0]
    g = VC.layout_groups()
    order, seg = pool_plan(g)
    assert np.diff(seg).tolist() == list(VC.SEGMENTS) and (np.diff(order[seg[6]:seg[7]]) > 0).all() and not (np.diff(g) >= 0).all()
    for bad in ([], [[0, 1]], [0, -1], [0.5, 1.0], [float('nan')], ['a']):
        with pytest.raises(ValueError):
            pool_plan(bad)
    with pytest.raises(ValueError):
        pool_plan([0, 3], n_groups=3)


# ------------------------------------------------------------------------------------------------ 3. the restatement against the exact tables
def test_restatement_meets_the_exact_tables():
    """Every score of every point and of every pooled group of the hand-written cases, against fractions.Fraction.  Prints the worst relative
    deviation: the number MEASURED of tests/verify_cases.py was read here."""
    worst = {}
    for name, case in VC.exact_cases().items():
        got, _ = _run(case)
        worst[name, 'point'] = VC.deviation(got, VC.exact_of(name, False))
        got, _ = _run(case, case['groups'])
        worst[name, 'pooled'] = VC.deviation(got, VC.exact_of(name, True))
    print('worst relative deviation from the exact value: %s; bound %.3e' % ({k: '%.3e' % v for k, v in worst.items()}, VC.BOUND))
    assert max(worst.values()) <= VC.BOUND, worst


def test_the_basic_table_says_what_its_points_are_there_for():
    case = VC.basic_case()
    got, st = _run(case)
    want = VC.exact_of('basic', False)
    assert got['count'].tolist() == [[0, 0], [1, 5], [5, 5], [5, 5], [5, 5], [5, 5], [5, 5], [2, 5]] == want['count'].tolist()
    for key in VC.SCORES:
        assert np.isnan(got[key][0]).all(), key                            # no report ever: everything NaN
    assert np.isnan(got['pod'][0]).all() and np.isnan(got['base_ets'][0]).all()
    assert got['bias'][1, 0] == 1.25 and np.isnan(got['corr'][1, 0]) and got['max_abs_error'][1, 0] == 1.25           # one pair
    assert st['m2_o'][0, 2] == 0 and np.isnan(got['corr'][2, 0]) and not np.isnan(got['skill'][2, 0])                  # constant reports
    assert st['sum_d2'][0, 3] == 0 and got['skill'][3, 0] == 1 and got['rmse'][3, 0] == 0 and got['corr'][3, 0] == 1   # forecast = report
    assert st['sum_e2'][0, 4] == 0 and np.isnan(got['skill'][4, 0]) and got['base_rmse'][4, 0] == 0                    # baseline = report
    assert got['bias'][5, 0] == 0 and got['max_abs_error'][5, 0] == 0 and np.isnan(got['corr'][5, 0]) and np.isnan(got['skill'][5, 0])     # +0 / -0
    # strict on both sides: 300.0 is not above 300, 273.15f is not below 273.15f (point 3: reports 271, 273.15f, 275.5, 300, 300.25)
    cont = st['cont'][:, :, 3]
    assert cont[0].tolist() == [1, 0, 0, 0, 1, 1] and cont[1].tolist() == [1, 0, 0, 1, 0, 0]
    assert st['cont'][2, :, 2].tolist() == [0, 2, 2, 1, 1, 1]                # the wind: 10.0 is not above 10, neither as forecast nor as report


def test_the_vector_restatement_is_the_plain_loop_bit_for_bit():
    for name, case in list(VC.exact_cases().items()) + list(VC.order_cases().items()):
        for groups in (None, case['groups']):
            got, _ = _run(case, groups)
            loop = VC.loop_scores(case, groups)
            for key in loop:
                assert _same_bits(got[key], loop[key]), (name, groups is not None, key)


def test_the_fold_order_is_the_one_the_header_states():
    for name, case in VC.order_cases().items():
        got, _ = _run(case, case['groups'])
        assert VC.meets(got, case['expect']), (name, got['bias'], got['count'])


# ------------------------------------------------------------------------------------------------ 4. pooling
def test_pooling_equals_accumulating_the_pooled_pairs_directly():
    """A group's pooled state against ONE point that received all the group's pairs in the pooled order, date after date: the same scores within the
    bound (Chan's merge and Welford's update round differently), the same counts and contingency tables exactly."""
    from deepphysinet_amd import verification as VF
    for name, case in VC.exact_cases().items():
        pooled, _ = _run(case, case['groups'])
        thr_col, thr_val, thr_side = case['thr']
        M, n, P = case['x'].shape
        G = int(case['groups'].max()) + 1
        st = VF.verify_state_zeros(G, P, len(thr_col))
        for g in range(G):
            for i in np.nonzero(case['groups'] == g)[0]:
                for m in range(M):
                    VF.verify_accumulate_reference(st, case['x'][m, i:i + 1], case['b'][m, i:i + 1], case['o'][m, i:i + 1], thr_col, thr_val, thr_side, g)
        direct = VF.verify_finish_reference(st, thr_col)
        assert np.array_equal(direct['count'], pooled['count'])
        for key in VF.THRESHOLD_SCORES:
            assert _same_bits(direct[key], pooled[key]), (name, key)
        dev = VC.deviation(pooled, {k: direct[k].astype(np.float64) for k in VF.SCORES})
        print('%s: pooled against direct %.3e' % (name, dev))
        assert dev <= VC.BOUND, (name, dev)


def test_chunking_of_the_accumulate_calls_does_not_change_a_bit():
    from deepphysinet_amd import verification as VF
    case = VC.layout_case()
    n = case['x'].shape[1]
    whole, st = _run(case, case['groups'])
    for size in (1000, 257, 4418):
        chunks = [(f, min(f + size, n)) for f in range(0, n, size)]
        again, st2 = _run(case, case['groups'], chunks)
        for key in whole:
            assert _same_bits(whole[key], again[key]), (size, key)
        for key in VF.STATE_FIELDS:
            assert _same_bits(st[key], st2[key]), (size, key)


# ------------------------------------------------------------------------------------------------ 5. the seeded mistakes
@pytest.mark.parametrize('mistake', VC.MISTAKES)
def test_every_seeded_mistake_is_caught_by_the_tables(mistake):
    """The plain loop, which equals the restatement bit for bit, with one mistake seeded: a table must refuse it."""
    caught = []
    for name, case in VC.exact_cases().items():
        for groups in (None, case['groups']):
            if VC.deviation(VC.loop_scores(case, groups, mistake), VC.exact_of(name, groups is not None)) > VC.BOUND:
                caught.append((name, 'pooled' if groups is not None else 'point'))
    for name, case in VC.order_cases().items():
        if not VC.meets(VC.loop_scores(case, case['groups'], mistake), case['expect']):
            caught.append((name, 'pooled'))
    print('%s: caught by %s' % (mistake, caught))
    assert caught, mistake


def test_the_tables_pass_the_loop_without_a_mistake():
    for name, case in VC.exact_cases().items():
        for groups in (None, case['groups']):
            assert VC.deviation(VC.loop_scores(case, groups), VC.exact_of(name, groups is not None)) <= VC.BOUND, name


# ------------------------------------------------------------------------------------------------ 6. host refusals
def test_host_refusals():
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics
    from deepphysinet_amd.point_path import VerifyState
    with pytest.raises(ValueError, match='17 products'):
        InterfacePhysics._verify_request(['T'] * 17, None)
    with pytest.raises(KeyError, match='vorticity'):
        InterfacePhysics._verify_request(['T', 'vorticity'], None)
    with pytest.raises(ValueError, match='not among'):
        InterfacePhysics._verify_request(['T'], {'speed': 1.0})
    with pytest.raises(ValueError, match='point'):
        InterfacePhysics._verify_request(['T'], None, ['station', 'point'])
    names, ids, thr = InterfacePhysics._verify_request(['T', 'speed'], {'T': ('below', 273.15)}, ['station'])
    assert (names, ids, thr) == (['T', 'speed'], [31, 25], ([0], [float(np.float32(273.15))], [1]))
    for args in ((0, [31], [], [], []), (4, [], [], [], []), (4, [31] * 17, [], [], []), (4, [31], [0] * 17, [1.0] * 17, [0] * 17),
                 (4, [31], [0], [], [0]), (4, [31], [0], [1.0], [])):
        with pytest.raises(ValueError, match='VerifyState'):
            VerifyState(*args, device='cpu')                               # (refused before anything is allocated)
    st = VF.verify_state_zeros(4, 2, 0)
    z = np.zeros((2, 2), np.float32)
    for bad in (lambda: VF.verify_accumulate_reference(st, z, z, z[:1]), lambda: VF.verify_accumulate_reference(st, z, z, z, first=3),
                lambda: VF.verify_accumulate_reference(st, z[:, :1], z[:, :1], z[:, :1]), lambda: VF.verify_pool_reference(st, [0, 1, 2, 3], [0, 3]),
                lambda: VF.verify_pool_reference(st, [0, 1, 2, 3], [0, 3, 2, 4]), lambda: VF.verify_pool_reference(st, [0, 1, 2], [0, 4])):
        with pytest.raises(ValueError):
            bad()


def test_verify_at_refuses_before_the_first_launch():
    """On the CPU nothing can launch: every refusal below comes from the checks in front."""
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    stub = lambda cfg: type('S', (), dict(cfg=cfg, cube=torch.zeros(1), check_positions=CollocationSampler.check_positions,
                                          lonlat_to_index=CollocationSampler.lonlat_to_index))()       # nothing below reaches a kernel
    s = stub(SamplerConfig())
    obs = torch.zeros((3, 1), dtype=torch.float32)
    case = dict(field_data=None, forecast_h=None, sampler=s, obs=obs)
    xi, yi, hr = [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0, 2.0]
    with pytest.raises(KeyError, match='gust'):
        m.verify_at([case], xi, yi, hr, ['gust'])
    with pytest.raises(ValueError, match='not finite'):
        m.verify_at([case], xi, yi, hr, ['T'], thresholds={'T': float('inf')})
    with pytest.raises(ValueError, match='no cases'):
        m.verify_at([], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='17 products'):
        m.verify_at([case], xi, yi, hr, ['T'] * 17)
    other = stub(SamplerConfig(input_time_step_nums=3))
    with pytest.raises(ValueError, match='verification case 1: input_time_step_nums'):
        m.verify_at([case, dict(case, sampler=other)], xi, yi, hr, ['T'])
    with pytest.raises(IndexError):
        m.verify_at([case], [1.0, 2.0, 300.0], yi, hr, ['T'])
    for bad in (obs[:2], obs.double(), obs.numpy(), None, torch.zeros((3, 2))):
        with pytest.raises(ValueError, match='obs must be'):
            m.verify_at([dict(case, obs=bad)], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='verification case 1: obs'):
        m.verify_at([case, dict(case, obs=None)], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='negative'):
        m.verify_at([case], xi, yi, hr, ['T'], by={'station': [0, -1, 1]})
    with pytest.raises(ValueError, match=r'by\[\'hour\'\]'):
        m.verify_at([case], xi, yi, hr, ['T'], by={'hour': [0, 1]})
    with pytest.raises(ValueError, match='may not be called'):
        m.verify_at([case], xi, yi, hr, ['T'], by={'names': [0, 0, 0]})


# ------------------------------------------------------------------------------------------------ 7. the report file, the loop's key, the flags
def _reports(path=None, M=2, H=3, S=4, names=('speed', 'T', 'q')):
    g = np.random.default_rng(5)
    d = dict(lon=80.0 + np.arange(S) * 1.5, lat=20.0 + np.arange(S) * 2.0, hours=np.arange(H) * 6.0, names=np.array(names),
             obs=g.normal(size=(M, H, S, len(names))).astype(np.float32))
    d['obs'][0, 1, 2, :] = np.nan
    if path is not None:
        np.savez(path, **d)
    return d


def test_report_reader_and_point_list(tmp_path):
    from deepphysinet_amd.verification import GROUPINGS, read_observations, report_points
    d = _reports(tmp_path / 'r.npz')
    r = read_observations(str(tmp_path / 'r.npz'), ['T', 'speed'])
    assert r['obs'].shape == (2, 3, 4, 2) and r['obs'].dtype == np.float32 and r['obs'].flags['C_CONTIGUOUS']
    assert np.array_equal(r['obs'], d['obs'][..., [1, 0]], equal_nan=True) and np.array_equal(r['lon'], d['lon']) and r['hours'].dtype == np.float64
    assert np.array_equal(read_observations(d, ['q'])['obs'][..., 0], d['obs'][..., 2], equal_nan=True)
    lon, lat, hrs, groups = report_points(r)
    assert GROUPINGS == ('station', 'hour', 'all') and list(groups) == list(GROUPINGS)
    i = 2 * 4 + 3                                                          # point i = h * S + s
    assert (lon[i], lat[i], hrs[i]) == (d['lon'][3], d['lat'][3], 12.0) and (groups['station'][i], groups['hour'][i], groups['all'][i]) == (3, 2, 0)
    assert np.array_equal(r['obs'][1].reshape(12, 2)[i], r['obs'][1, 2, 3])
    assert list(report_points(r, ['hour'])[3]) == ['hour']
    with pytest.raises(ValueError, match='decade'):
        report_points(r, ['decade'])
    with pytest.raises(KeyError, match='rho'):
        read_observations(d, ['T', 'rho'])
    for bad in (dict(d, obs=d['obs'][:, :2]), dict(d, lat=d['lat'][:3]), dict(d, obs=np.zeros(d['obs'].shape, dtype=np.int32)), dict(d, obs=d['obs'][:0]),
                {k: v for k, v in d.items() if k != 'hours'}, dict(d, names=d['names'][:2])):
        with pytest.raises(ValueError):
            read_observations(bad, ['T'])


def test_run_inference_interface_checks_the_verify_key_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    _reports(tmp_path / 'r.npz')
    torch.manual_seed(0)
    m = builder_models(**cfg)
    assert m.last_verification is None
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(KeyError, match='gust'):                            # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(verify=dict(products=['gust'], obs=str(tmp_path / 'r.npz')), **nothing)
    with pytest.raises(ValueError, match='no reports to verify against'):  # what --synthetic without a file comes to
        m.run_inference_interface(verify=dict(products=['T']), samples='synthetic', checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu')
    for bad in (dict(obs=str(tmp_path / 'r.npz')), dict(products=['T'], obs=str(tmp_path / 'r.npz'), colour='red'),
                dict(products=['T'], obs=str(tmp_path / 'r.npz'), thresholds={'T': float('nan')}),
                dict(products=['T'], obs=str(tmp_path / 'r.npz'), by=['decade']), dict(products=['T'], obs=dict(lon=[1.0]))):
        with pytest.raises(ValueError):
            m.run_inference_interface(verify=bad, **nothing)
    with pytest.raises(KeyError, match='rho'):                             # a product the file does not hold
        m.run_inference_interface(verify=dict(products=['rho'], obs=str(tmp_path / 'r.npz')), **nothing)
    m.inference_cfg['verify'] = dict(products=['T', 'speed'], obs=str(tmp_path / 'r.npz'), thresholds={'T': ('below', 273.15)}, by=['station', 'all'])
    with pytest.raises(NotImplementedError):                               # now the missing checkpoint is what stops it
        m.run_inference_interface(**nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_verification is None


def test_infer_launcher_flags_reach_the_verify_key():
    import infer
    args = infer.parse.parse_args([])
    assert args.verify is None and args.verify_obs is None and args.verify_threshold == [] and infer.verify_option(args) is None
    args = infer.parse.parse_args(['--verify', 'T,speed', '--verify_obs', 'r.npz', '--synthetic'])
    assert infer.verify_option(args) == dict(products=['T', 'speed'], obs='r.npz', thresholds={}, by=['station', 'hour', 'all'])
    args = infer.parse.parse_args(['--verify', 'T,speed', '--verify_obs', 'r.npz', '--verify_threshold', 'T:below:273.15', '--verify_threshold', 'speed:10,15',
                                   '--verify_threshold', 'T:above:300', '--verify_by', 'hour'])
    opt = infer.verify_option(args)
    assert opt == dict(products=['T', 'speed'], obs='r.npz', by=['hour'],
                       thresholds={'T': [('below', 273.15), ('above', 300.0)], 'speed': [('above', 10.0), ('above', 15.0)]})
    from deepphysinet_amd.verification import check_thresholds
    assert check_thresholds(opt['products'], opt['thresholds']) == ([0, 0, 1, 1], [float(np.float32(273.15)), 300.0, 10.0, 15.0], [1, 0, 0, 0])
    for bad in (['--verify', 'T'], ['--verify', 'T', '--synthetic'], ['--verify_obs', 'r.npz'], ['--verify_threshold', 'T:1'],
                ['--verify', 'T', '--verify_obs', 'r.npz', '--verify_threshold', 'T'], ['--verify', 'T', '--verify_obs', 'r.npz', '--verify_threshold', 'T:near:1'],
                ['--verify', 'T', '--verify_obs', 'r.npz', '--verify_threshold', ':below:1']):
        with pytest.raises(SystemExit):
            infer.verify_option(infer.parse.parse_args(bad))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "['verify'] = verify_option(args)" in src                      # ... and the launcher puts it into inference_cfg
