"""No GPU: the host side of the probabilistic verification of ensembles (dpn_pverify_stage, dpn_pverify_case, dpn_pverify_pool, dpn_pverify_finish)
-- the C ABI additions and struct layouts, the numpy restatement (deepphysinet_amd/prob_verification.py) against the exact tables of
tests/prob_verify_cases.py, the identities the scores obey, pooling against folding the pooled pairs into one state, chunking, the seeded mistakes,
every host refusal, the loop's new key and the launcher's flag.  The kernels: tests/test_gpu_prob_verify.py."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import prob_verify_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(case, groups=None, chunks=None):
    """The restatement over a table: per case stage member by member and fold (both in `chunks` of points), pool when groups are given, finish."""
    from deepphysinet_amd import prob_verification as PV
    x, b, o = case['x'], case['b'], case['o']
    thr = case['thr']
    C, M, n, P = x.shape
    chunks = chunks or [(0, n)]
    st = PV.prob_verify_state_zeros(n, P, len(thr[0]), M)
    pf, pb = PV.planes_zeros(n, P, M)
    for c in range(C):
        for m in range(M):
            for first, stop in chunks:
                PV.pverify_stage_reference(pf, pb, x[c, m, first:stop], b[c, m, first:stop], m, first)
        for first, stop in chunks:
            PV.pverify_case_reference(st, pf, pb, o[c, first:stop], *thr, first)
    if groups is not None:
        st = PV.pverify_pool_reference(st, *PV.pool_plan(groups, PC.n_groups(case)), thr[0])
    return PV.pverify_finish_reference(st, thr[0]), st


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_are_declared_bound_and_exported_and_the_structs_follow_the_header():
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib, build, prob_verification as PV
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    for name in ('dpn_pverify_stage', 'dpn_pverify_case', 'dpn_pverify_pool', 'dpn_pverify_finish'):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    define = lambda what: int(re.search(r'^#define %s (\d+)' % what, header, flags=re.M).group(1))
    assert define('DPN_PV_MAX_MEMBERS') == PV.MAX_MEMBERS == _lib.PV_MAX_MEMBERS == 64
    assert (PV.MAX_COLUMNS, PV.MAX_THRESHOLDS) == (define('DPN_VERIFY_MAX_COLUMNS'), define('DPN_VERIFY_MAX_THRESHOLDS'))
    for struct in (PV.DpnPVerifyState, PV.DpnPVerifyOut):                # the members of the typedef, in its order, every one a pointer
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct.__name__, struct.__name__), header, flags=re.S).group(1)
        members = [n for decl in body.split(';') for n in re.findall(r'\*\s*(\w+)', decl)]
        assert members == [n for n, _ in struct._fields_], struct.__name__
        assert ctypes.sizeof(struct) == 8 * len(members) and all(t is ctypes.c_void_p for _, t in struct._fields_)
        assert [getattr(struct, n).offset for n in members] == [8 * i for i in range(len(members))]
    assert len(PV.DpnPVerifyState._fields_) == 8 and len(PV.DpnPVerifyOut._fields_) == 32
    assert _lib.DpnPVerifyState is PV.DpnPVerifyState and _lib.DpnPVerifyOut is PV.DpnPVerifyOut
    sizes = {k: len(_lib.EXPORTS['dpn_pverify_' + k][1]) for k in ('stage', 'case', 'pool', 'finish')}
    assert sizes == dict(stage=14, case=14, pool=12, finish=10) and all(_lib.EXPORTS['dpn_pverify_' + k][0] is ctypes.c_int for k in sizes)
    assert '#include "dpn_pverify.inc"' in open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_diag.hip')).read()
    assert os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_pverify.inc') in build.DEPS     # a change of it rebuilds the library
    text = open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_pverify.inc')).read()
    assert 'atomic' not in text.replace('No atomics', '').replace('no atomics', '') and '__syncthreads' not in text
    assert set(PC.SCORES) == set(PV.SCORES) and set(PC.THRESHOLD_SCORES) == set(PV.THRESHOLD_SCORES)
    assert set(PC.INT_KEYS) == {'count'} | set(PV.HISTS) | set(PV.DIAGRAMS)


# ------------------------------------------------------------------------------------------------ 2. the restatement against the exact tables
def test_restatement_meets_the_exact_tables():
    """The integer outputs exactly, the float scores within BOUND of the exact rationals; prints the deviation that MEASURED records."""
    worst = 0.0
    for name, case in PC.tables().items():
        for pooled in (False, True):
            rows, _ = _run(case, case['groups'] if pooled else None)
            dev = PC.deviation(rows, PC.exact_of(name, pooled))
            print('%s, %s: worst relative deviation %.3e' % (name, 'pooled' if pooled else 'points', dev))
            assert dev <= PC.BOUND, (name, pooled, dev)
            worst = max(worst, dev)
    print('worst over the tables %.3e; MEASURED %.3e, BOUND %.3e' % (worst, PC.MEASURED, PC.BOUND))
    assert worst <= PC.MEASURED                                            # the recorded figure is the measured one, rounded up


def test_the_tables_say_what_their_points_are_there_for():
    three, two, eight, one = (_run(PC.tables()[k])[0] for k in ('three', 'two', 'eight', 'one'))
    assert three['count'][:, 0].tolist() == [3, 3, 3, 2, 2, 1, 0, 3] and three['count'][6].tolist() == [0, 0]
    assert three['rank_hist'][0, 0].tolist() == [1, 0, 1, 1]              # below, inside (two members under the report), above
    assert three['rank_hist'][1, 0].tolist() == [0, 2, 1, 0]              # ties of 1, 3 and 2 members: lt + eq // 2 = 1 + 0, 0 + 1, 1 + 1
    assert three['base_rank_hist'][1, 0].tolist() == [0, 3, 0, 0]         # ties of 2, 1 and 2: 0 + 1, 1 + 0, 0 + 1
    assert np.isnan(three['crps'][6]).all() and not three['rank_hist'][6].any()
    assert three['crps'][7, 0] == 0 and three['rmse'][7, 0] == 0 and np.isnan(three['spread_skill'][7, 0]) and three['base_crps'][7, 0] > 0
    assert three['rel_n'][1, 0].tolist() == [2, 1, 0, 0]                  # `above 300`: a member AT 300 is no event, 301 is the only one
    assert three['rel_n'][2, 1].tolist() == [1, 1, 0, 1] and three['rel_o'][2, 1].tolist() == [0, 1, 0, 0]       # `below 273.15f`: T0 itself is none
    assert eight['rank_hist'][0, 0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]          # under all eight; two under and three equal: 2 + 3 // 2
    assert one['crps'][0, 0] == one['fair_crps'][0, 0] == np.float32(1.125) and one['spread'][0, 0] == 0 and np.isnan(one['spread_skill'][0, 0])
    assert one['rel_n'][1, 0].tolist() == [1, 1] and one['rel_o'][1, 0].tolist() == [0, 1]
    for e in (1, 2):                                                       # never and always: no uncertainty, no skill score, no ROC
        assert (two['uncertainty'][[0, 1, 2], e] == 0).all() and np.isnan(two['bss'][:, e]).all() and np.isnan(two['roc_area'][:, e]).all()
    assert two['brier'][0, 1] == 0 and two['brier'][0, 2] == 0 and two['count'][3, 0] == 0
    pooled = _run(PC.tables()['two'], PC.tables()['two']['groups'])[0]
    assert pooled['count'][:, 0].tolist() == [2, 0, 4] and np.isnan(pooled['crps'][1, 0]) and not pooled['rel_n'][1].any()


def test_brier_is_reliability_minus_resolution_plus_uncertainty_exactly():
    seen = 0
    for name in PC.tables():
        for pooled in (False, True):
            ex = PC.exact_of(name, pooled)
            for pre in ('', 'base_'):
                for idx in np.ndindex(ex['brier'].shape):
                    if ex[pre + 'brier'][idx] is not None:
                        assert ex[pre + 'brier'][idx] == ex[pre + 'reliability'][idx] - ex[pre + 'resolution'][idx] + ex['uncertainty'][idx], (name, idx)
                        seen += 1
    assert seen > 100


def test_crps_pair_form_is_the_sorted_closed_form_and_the_integral():
    """a / M - g / M^2 against the sorted form of g and against the integral of (F - H)^2 over the real line, F the ensemble's step function, H
    the report's -- piecewise constant, so summed exactly."""
    rng = np.random.default_rng(3)
    for M in (1, 2, 3, 8, 17):
        for trial in range(6):
            xs = [Fraction(float(v)) for v in np.round(rng.normal(size=M) * 4) / 4]       # quarters: ties happen
            o = Fraction(float(np.round(rng.normal() * 4) / 4)) if trial else xs[0]
            a = sum(abs(v - o) for v in xs)
            g = sum(abs(xs[i] - xs[k]) for i in range(M) for k in range(i + 1, M))
            crps = a / M - g / (M * M)
            srt = sorted(xs)
            assert g == sum((2 * i - M + 1) * v for i, v in enumerate(srt))
            cuts = sorted(set(xs) | {o})
            integral = Fraction(0)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                F = Fraction(sum(v <= lo for v in xs), M)
                integral += (F - (1 if lo >= o else 0)) ** 2 * (hi - lo)
            assert crps == integral, (M, trial)


# ------------------------------------------------------------------------------------------------ 3. one order, one result
def test_the_vector_restatement_is_the_plain_loop_bit_for_bit():
    for name, case in PC.tables().items():
        for groups in (None, case['groups']):
            rows, _ = _run(case, groups)
            loop = PC.loop_scores(case, groups)
            for key, v in rows.items():
                assert _same_bits(v, loop[key]), (name, groups is not None, key)


def test_pooling_equals_folding_the_pooled_pairs_into_one_state():
    """A group's pooled state against ONE point that receives every (point, case) pair of the group as a case of its own: the integer outputs
    exactly, the sums (added in another order) within the bound."""
    from deepphysinet_amd import prob_verification as PV
    for name, case in PC.tables().items():
        x, b, o, thr = case['x'], case['b'], case['o'], case['thr']
        C, M, n, P = x.shape
        pooled, _ = _run(case, case['groups'])
        for g in range(PC.n_groups(case)):
            st = PV.prob_verify_state_zeros(1, P, len(thr[0]), M)
            for i in np.nonzero(case['groups'] == g)[0]:
                for c in range(C):
                    PV.pverify_case_reference(st, np.ascontiguousarray(x[c, :, i:i + 1].transpose(0, 2, 1)),
                                              np.ascontiguousarray(b[c, :, i:i + 1].transpose(0, 2, 1)), o[c, i:i + 1], *thr)
            direct = PV.pverify_finish_reference(st, thr[0])
            for key, v in direct.items():
                got = pooled[key][g:g + 1]
                if key in PC.INT_KEYS:
                    assert np.array_equal(got, v), (name, g, key)
                    continue
                assert np.array_equal(np.isnan(got), np.isnan(v)), (name, g, key)
                ok = ~np.isnan(v)
                assert np.all(np.abs(got[ok].astype(np.float64) - v[ok]) <= PC.BOUND * np.abs(v[ok])), (name, g, key)


def test_chunking_of_the_stage_and_case_calls_does_not_change_a_bit():
    for name in ('three', 'layout'):
        case = PC.tables()[name]
        n = case['x'].shape[2]
        whole, st = _run(case, case['groups'])
        for size in (1, 3, 64):
            chunks = [(first, min(first + size, n)) for first in range(0, n, size)]
            rows, st2 = _run(case, case['groups'], chunks)
            assert all(_same_bits(rows[k], whole[k]) for k in whole) and all(_same_bits(st[k], st2[k]) for k in st), (name, size)


# ------------------------------------------------------------------------------------------------ 4. the seeded mistakes
@pytest.mark.parametrize('mistake', PC.MISTAKES)
def test_every_seeded_mistake_is_caught_by_the_tables(mistake):
    caught = []
    for name, case in PC.tables().items():
        for pooled in (False, True):
            with np.errstate(invalid='ignore'):
                rows = PC.loop_scores(case, case['groups'] if pooled else None, mistake)
            if PC.deviation(rows, PC.exact_of(name, pooled)) > PC.BOUND:
                caught.append((name, pooled))
    print('%s: caught by %s' % (mistake, caught))
    assert caught, mistake


def test_the_tables_pass_the_loop_without_a_mistake():
    for name, case in PC.tables().items():
        for pooled in (False, True):
            assert PC.deviation(PC.loop_scores(case, case['groups'] if pooled else None), PC.exact_of(name, pooled)) <= PC.BOUND, (name, pooled)


# ------------------------------------------------------------------------------------------------ 5. refusals on the host
def test_host_refusals():
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics
    from deepphysinet_amd.point_path import ProbVerifyState
    request = lambda *args: InterfacePhysics._verify_request(*args, word='verify_ensemble')
    with pytest.raises(ValueError, match='17 products'):
        request(['T'] * 17, None)
    with pytest.raises(KeyError, match='vorticity'):
        request(['T', 'vorticity'], None)
    with pytest.raises(ValueError, match='not among'):
        request(['T'], {'speed': 1.0})
    for word in ('point', 'members', 'names', 'thresholds'):
        with pytest.raises(ValueError, match='may not be called'):
            request(['T'], None, ['station', word])
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match='members per case'):
            request(['T'], None, None, bad)
    names, ids, thr = request(['T', 'speed'], {'T': ('below', 273.15)}, ['station'], 64)
    assert (names, ids, thr) == (['T', 'speed'], [31, 25], ([0], [float(np.float32(273.15))], [1]))
    assert PV.VF.verify_ids(['u', 'rel_humidity', 'u']) == [28, 26, 28]
    for args in ((0, [31], [], [], [], 3), (4, [], [], [], [], 3), (4, [31] * 17, [], [], [], 3), (4, [31], [0] * 17, [1.0] * 17, [0] * 17, 3),
                 (4, [31], [0], [], [0], 3), (4, [31], [0], [1.0], [], 3), (4, [31], [], [], [], 0), (4, [31], [], [], [], 65)):
        with pytest.raises(ValueError):
            ProbVerifyState(*args, device='cpu')                           # (refused before anything is allocated)
    # a state past 2^31 - 1 elements in any array: the rank histogram, the reliability table, a plane
    assert PV.state_elements(6400, 4, 3, 61) == dict(n=25600, sums=51200, rank=3174400, rel=4761600, plane=1561600)
    for args, word in (((2 ** 22, 16, 0, 64), 'rank'), ((2 ** 24, 1, 16, 1), 'rel'), ((2 ** 26, 1, 0, 64), 'rank'), ((2 ** 31, 1, 0, 1), 'n')):
        with pytest.raises(ValueError, match=word + ' would hold'):
            PV.check_state_size(*args)
        with pytest.raises(ValueError, match='2\\^31 - 1'):
            ProbVerifyState(args[0], [31] * args[1], [0] * args[2], [1.0] * args[2], [0] * args[2], args[3], device='cpu')
    PV.check_state_size(2 ** 23, 1, 0, 64)                                 # 2 * 65 * 2^23 < 2^31
    st = PV.prob_verify_state_zeros(4, 2, 0, 3)
    pf, pb = PV.planes_zeros(4, 2, 3)
    z = np.zeros((2, 2), np.float32)
    for bad in (lambda: PV.pverify_stage_reference(pf, pb, z, z[:1], 0), lambda: PV.pverify_stage_reference(pf, pb, z, z, 3),
                lambda: PV.pverify_stage_reference(pf, pb, z, z, -1), lambda: PV.pverify_stage_reference(pf, pb, z, z, 0, first=3),
                lambda: PV.pverify_stage_reference(pf, pb, z[:, :1], z[:, :1], 0), lambda: PV.pverify_case_reference(st, pf, pb, z[:, :1]),
                lambda: PV.pverify_case_reference(st, pf, pb, z, first=3), lambda: PV.pverify_case_reference(st, pf[:2], pb[:2], z),
                lambda: PV.pverify_pool_reference(st, [0, 1, 2, 3], [0, 3]), lambda: PV.pverify_pool_reference(st, [0, 1, 2, 3], [0, 3, 2, 4]),
                lambda: PV.pverify_pool_reference(st, [0, 1, 2], [0, 4])):
        with pytest.raises(ValueError):
            bad()


def test_verify_ensemble_at_refuses_before_the_first_launch():
    """On the CPU nothing can launch: every refusal below comes from the checks in front."""
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    stub = lambda cfg: type('S', (), dict(cfg=cfg, cube=torch.zeros(1), check_positions=CollocationSampler.check_positions,
                                          lonlat_to_index=CollocationSampler.lonlat_to_index))()       # nothing below reaches a kernel
    mem = dict(field_data=None, forecast_h=None, sampler=stub(SamplerConfig()))
    obs = torch.zeros((3, 1), dtype=torch.float32)
    case = dict(members=[mem, mem], obs=obs)
    xi, yi, hr = [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0, 2.0]
    with pytest.raises(KeyError, match='gust'):
        m.verify_ensemble_at([case], xi, yi, hr, ['gust'])
    with pytest.raises(ValueError, match='not finite'):
        m.verify_ensemble_at([case], xi, yi, hr, ['T'], thresholds={'T': float('inf')})
    with pytest.raises(ValueError, match='no cases'):
        m.verify_ensemble_at([], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='17 products'):
        m.verify_ensemble_at([case], xi, yi, hr, ['T'] * 17)
    with pytest.raises(ValueError, match='case 1 has 3 members, case 0 has 2'):
        m.verify_ensemble_at([case, dict(case, members=[mem] * 3)], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='no members'):
        m.verify_ensemble_at([dict(case, members=[])], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='65 members per case'):
        m.verify_ensemble_at([dict(case, members=[mem] * 65)], xi, yi, hr, ['T'])
    other = dict(mem, sampler=stub(SamplerConfig(input_time_step_nums=3)))
    with pytest.raises(ValueError, match='ensemble member 3: input_time_step_nums'):
        m.verify_ensemble_at([case, dict(case, members=[mem, other])], xi, yi, hr, ['T'])
    with pytest.raises(IndexError):
        m.verify_ensemble_at([case], [1.0, 2.0, 300.0], yi, hr, ['T'])
    for bad in (obs[:2], obs.double(), obs.numpy(), None, torch.zeros((3, 2))):
        with pytest.raises(ValueError, match='obs must be'):
            m.verify_ensemble_at([dict(case, obs=bad)], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='verification case 1: obs'):
        m.verify_ensemble_at([case, dict(case, obs=None)], xi, yi, hr, ['T'])
    with pytest.raises(ValueError, match='negative'):
        m.verify_ensemble_at([case], xi, yi, hr, ['T'], by={'station': [0, -1, 1]})
    with pytest.raises(ValueError, match=r'by\[\'hour\'\]'):
        m.verify_ensemble_at([case], xi, yi, hr, ['T'], by={'hour': [0, 1]})
    with pytest.raises(ValueError, match='may not be called'):
        m.verify_ensemble_at([case], xi, yi, hr, ['T'], by={'members': [0, 0, 0]})


# ------------------------------------------------------------------------------------------------ 6. the loop's key, the flag
def _reports(path, M=2, H=3, S=4, names=('speed', 'T', 'q')):
    g = np.random.default_rng(5)
    d = dict(lon=80.0 + np.arange(S) * 1.5, lat=20.0 + np.arange(S) * 2.0, hours=np.arange(H) * 6.0, names=np.array(names),
             obs=g.normal(size=(M, H, S, len(names))).astype(np.float32))
    np.savez(path, **d)
    return d


def test_run_inference_interface_checks_the_members_key(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    _reports(tmp_path / 'r.npz')
    torch.manual_seed(0)
    m = builder_models(**cfg)
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    option = dict(products=['T', 'speed'], obs=str(tmp_path / 'r.npz'), by=['station', 'all'])
    for bad in (0, 65, -2):                                                # no checkpoint exists at that path: the count is refused first
        with pytest.raises(ValueError, match='members per case'):
            m.run_inference_interface(verify=dict(option, members=bad), **nothing)
    with pytest.raises(KeyError, match='gust'):
        m.run_inference_interface(verify=dict(option, products=['gust'], members=3), **nothing)
    with pytest.raises(ValueError, match='may not be called|grouping'):
        m.run_inference_interface(verify=dict(option, by=['decade'], members=3), **nothing)
    with pytest.raises(NotImplementedError):                               # now the missing checkpoint is what stops it
        m.run_inference_interface(verify=dict(option, members=3), **nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    with pytest.raises(ValueError, match='the reports hold 2 cases, the sample source 0 of 3 members'):
        m.run_inference_interface(verify=dict(option, members=3), checkpoint_path=str(tmp_path), device='cpu', samples=[])
    with pytest.raises(ValueError, match='2 samples are not a multiple of members = 3'):
        m.run_inference_interface(verify=dict(option, members=3), checkpoint_path=str(tmp_path), device='cpu', samples=iter([{}, {}]))
    # members = 1 is today's route: an empty source runs through it untouched
    assert m.run_inference_interface(verify=dict(option, members=1), checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None
    assert m.last_verification is None


def test_infer_launcher_flag_reaches_the_verify_key():
    import infer
    args = infer.parse.parse_args(['--verify', 'T,speed', '--verify_obs', 'r.npz'])
    assert args.verify_members == 1 and 'members' not in infer.verify_option(args)            # the default leaves the key as it was
    args = infer.parse.parse_args(['--verify', 'T,speed', '--verify_obs', 'r.npz', '--verify_members', '5', '--synthetic', '--synthetic_samples', '10'])
    assert infer.verify_option(args) == dict(products=['T', 'speed'], obs='r.npz', thresholds={}, by=['station', 'hour', 'all'], members=5)
    assert args.synthetic_samples == 10
    with pytest.raises(SystemExit):
        infer.verify_option(infer.parse.parse_args(['--verify_members', '5']))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "kwargs['samples_per_epoch'] = args.synthetic_samples" in src
