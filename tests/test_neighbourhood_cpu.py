"""CPU: the neighbourhood verification's host side -- deepphysinet_amd.neighbourhood (the scales of a request, the analysis reader, the numpy
restatement of dpn_nbhd_stage / dpn_nbhd_fold / dpn_nbhd_finish) against exact tables by brute force in fractions.Fraction, known answers, a plain
scalar loop with seeded mistakes (tests/neighbourhood_cases.py), and the header, the binding table, the include line and infer.py's option."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import neighbourhood_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restate(case, planes_per_fold=None, cases=None):
    """(state, tables) of the restatement over the M cases of `case` (or the listed ones), folded planes_per_fold planes at a time."""
    from deepphysinet_amd import neighbourhood as NB
    M, nt = case['x'].shape[:2]
    E, K = len(case['thr'][0]), len(case['radius'])
    st = NB.nbhd_state_zeros(nt, E, K)
    for m in range(M) if cases is None else cases:
        mask = NB.nbhd_stage_reference(case['x'][m], case['b'][m], case['o'][m], case['thr'])
        step = nt * E if planes_per_fold is None else planes_per_fold
        for p0 in range(0, nt * E, step):
            NB.nbhd_fold_reference(st, mask, case['radius'], p0, min(step, nt * E - p0))
    return st, NB.nbhd_finish_reference(st)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_tables(a, b):
    return all(_same(a[g][k], b[g][k]) for g in ('hour', 'all') for k in a[g])


def _random_case(nx, ny, seed, nt=1, M=1, radius=(0, 1, 3)):
    g = np.random.default_rng(seed)
    x, b, o = (g.random((M, nt, 1, ny, nx)).astype(np.float32) for _ in range(3))
    o[g.random(o.shape) < 0.1] = np.nan
    return dict(x=x, b=b, o=o, thr=([0, 0], [0.5, 0.3], [0, 1]), radius=list(radius))


# ------------------------------------------------------------------------------------------------ 1. exact tables
def test_restatement_meets_the_exact_tables():
    """Integers exactly, float scores within the derived bound (tests/neighbourhood_cases.py: 2^-23, absolute for scores and frequencies, relative
    for the frequency biases).  Measured: point pair 2.384e-08, blob 2.908e-08, gaps 3.142e-08, tall 5.189e-08."""
    for name, case in NC.exact_cases().items():
        _, tab = _restate(case)
        exact = NC.exact_tables(case)
        nt, E = tab['hour']['count'].shape
        worst = max([NC.deviation(tab['hour'], exact['hour'][it][e], (it, e)) for it in range(nt) for e in range(E)]
                    + [NC.deviation(tab['all'], exact['all'][e], (e,)) for e in range(E)])
        print('%s: worst deviation from the exact table %.3e (bound %.3e)' % (name, worst, NC.BOUND))
        assert worst <= NC.BOUND, (name, worst)


# ------------------------------------------------------------------------------------------------ 2. known answers
def _planes(f, b, o, valid=None):
    """A one-case, one-hour, one-column case from event planes [ny, nx] (bool): values 1 where the event holds, NaN analysis where not valid."""
    x, bb, oo = (np.asarray(v, dtype=np.float32)[None, None, None] for v in (f, b, o))
    if valid is not None:
        oo = np.where(np.asarray(valid, dtype=bool)[None, None, None], oo, np.float32(np.nan)).astype(np.float32)
    return dict(x=x, b=bb, o=oo, thr=([0], [0.5], [0]))


def test_known_answers():
    g = np.random.default_rng(2)
    ny, nx = 9, 21
    f = g.random((ny, nx)) < 0.3
    # forecast == analysis: fss = 1 at every scale
    _, tab = _restate(dict(_planes(f, ~f, f), radius=[0, 1, 2, 5, 30]))
    assert tab['all']['fss'].tolist() == [[1.0] * 5] and tab['all']['skilful_scale'].tolist() == [0] and bool((tab['all']['base_fss'] < 1).all())
    # one event node at (5, 4) against one at (11, 4): nothing shared up to r = 2, a shared window from r = 3 on
    pair = NC.exact_cases()['point pair']
    _, tab = _restate(pair)
    fss = tab['all']['fss'][0]
    assert pair['radius'][:5] == [0, 1, 2, 3, 4] and bool((np.abs(fss[:3]) <= NC.BOUND).all()) and bool((fss[3:] > NC.BOUND).all()), fss
    assert bool((np.diff(fss[2:]) > 0).all()) and fss[5] == 1.0
    # r >= max(nx, ny) - 1: every window is the plane, the asymptotic value from the plane totals
    o = g.random((ny, nx)) < 0.2
    _, tab = _restate(dict(_planes(f, f, o), radius=[20, 21, 1000]))
    nf, no = int(f.sum()), int(o.sum())
    want = np.float32(2.0 * nf * no / (nf * nf + no * no))
    assert bool((np.abs(tab['all']['fss'][0] - want) <= NC.BOUND).all()) and tab['all']['windows'].tolist() == [[ny * nx] * 3]
    # an invalid node changes counts and windows only through V: the same tables as with the node's events cleared and V counted without it
    valid = np.ones((ny, nx), dtype=bool)
    valid[4, 5], valid[0, 0] = False, False
    st, tab = _restate(dict(_planes(f, f, o, valid), radius=[0, 1, 4]))
    assert int(st['n_valid'][0, 0]) == ny * nx - 2 and int(st['n_f'][0, 0]) == int((f & valid).sum()) and int(st['n_o'][0, 0]) == int((o & valid).sum())
    assert st['windows'][0, 0].tolist() == [ny * nx - 2, ny * nx, ny * nx]             # r = 0: the two nodes' own windows are empty
    exact = NC.exact_tables(dict(_planes(f, f, o, valid), radius=[0, 1, 4]))
    assert NC.deviation(tab['all'], exact['all'][0], (0,)) <= NC.BOUND
    # a plane with no valid node: NaN scores, no windows, no skilful scale
    st, tab = _restate(dict(_planes(f, f, o, np.zeros((ny, nx), dtype=bool)), radius=[0, 3]))
    assert st['windows'].tolist() == [[[0, 0]]] and bool(np.isnan(tab['hour']['fss']).all()) and bool(np.isnan(tab['hour']['useful']).all())
    assert tab['hour']['count'].tolist() == [[0]] and tab['hour']['skilful_scale'].tolist() == [[-1]] and bool(np.isnan(tab['all']['fbias']).all())


# ------------------------------------------------------------------------------------------------ 3. bit for bit against a plain loop
@pytest.mark.parametrize('nx,ny', [(63, 2), (64, 3), (65, 2), (130, 1), (3, 64), (2, 65), (1, 70), (66, 66)])
def test_restatement_is_the_plain_loop_bit_for_bit(nx, ny):
    case = _random_case(nx, ny, seed=nx * 100 + ny, nt=2, M=2, radius=(0, 2, max(nx, ny)))
    st, tab = _restate(case)
    loop_st, loop_tab = NC.loop_tables(case)
    for key in st:
        assert _same(st[key], loop_st[key]), key
    assert _same_tables(tab, loop_tab)
    # any plane batching; cases one by one against the sum of their totals in order
    for step in (1, 3):
        other, _ = _restate(case, planes_per_fold=step)
        assert all(_same(st[k], other[k]) for k in st), step
    first, second = _restate(case, cases=[0])[0], _restate(case, cases=[1])[0]
    assert all(_same(st[k], first[k] + second[k]) for k in st)


def test_hand_written_cases_are_the_plain_loop_and_the_stage_chunks_freely():
    from deepphysinet_amd import neighbourhood as NB
    for name, case in NC.exact_cases().items():
        st, tab = _restate(case)
        loop_st, loop_tab = NC.loop_tables(case)
        assert all(_same(st[k], loop_st[k]) for k in st) and _same_tables(tab, loop_tab), name
        whole = NB.nbhd_stage_reference(case['x'][0], case['b'][0], case['o'][0], case['thr'])
        cut = case['x'].shape[3] // 2
        parts = [NB.nbhd_stage_reference(case['x'][0][:, :, s], case['b'][0][:, :, s], case['o'][0][:, :, s], case['thr']) for s in (slice(0, cut), slice(cut, None))]
        assert _same(whole, np.concatenate(parts, axis=2)) and whole.dtype == np.uint8 and int(whole.max()) <= 15, name
        assert bool(((whole & 8) != 0)[(whole & 7) != 0].all()), name             # an event bit only on a valid node


def test_table_is_exclusive_and_interleaved():
    from deepphysinet_amd import neighbourhood as NB
    g = np.random.default_rng(1)
    mask = g.integers(0, 16, size=(3, 7, 11)).astype(np.uint8)
    S = NB.nbhd_table_reference(mask)
    assert S.shape == (3, 8, 12, 4) and S.dtype == np.int32 and not S[:, 0].any() and not S[:, :, 0].any()
    for q in range(4):
        assert int(S[1, 5, 9, q]) == int(((mask[1, :5, :9] >> q) & 1).sum())


# ------------------------------------------------------------------------------------------------ 4. seeded mistakes
@pytest.mark.parametrize('mistake', NC.MISTAKES)
def test_every_seeded_mistake_is_caught(mistake):
    """The plain loop with the mistake leaves the restatement's bits on at least one hand-written case (the row order: on `tall`, ny = 70 > 64),
    and where the mistake changes the mathematics it leaves the exact table's bound too."""
    caught, beyond = [], []
    for name, case in NC.exact_cases().items():
        st, tab = _restate(case)
        bad_st, bad_tab = NC.loop_tables(case, mistake)
        if not (all(_same(st[k], bad_st[k]) for k in st) and _same_tables(tab, bad_tab)):
            caught.append(name)
            exact = NC.exact_tables(case)
            try:
                nt, E = bad_tab['hour']['count'].shape
                if max(NC.deviation(bad_tab['hour'], exact['hour'][it][e], (it, e)) for it in range(nt) for e in range(E)) > NC.BOUND:
                    beyond.append(name)
            except AssertionError:
                beyond.append(name)
    assert caught, mistake
    if mistake == 'rows folded in plain order':
        assert caught == ['tall']                                          # a rounding-level difference: only the bits show it
    else:
        assert beyond, mistake


# ------------------------------------------------------------------------------------------------ 5. header, bindings, include line
def test_struct_layouts_match_the_header(tmp_path):
    from deepphysinet_amd import _lib, neighbourhood as NB
    assert _lib.DpnNbhdState is NB.DpnNbhdState and _lib.DpnNbhdOut is NB.DpnNbhdOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {', '  printf("scales %d\\n", DPN_NBHD_MAX_SCALES);']
    want = {'scales': NB.MAX_SCALES}
    for st in (NB.DpnNbhdState, NB.DpnNbhdOut):
        n = st.__name__
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (n, n))
        want[n] = ctypes.sizeof(st)
        for f in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (n, f[0], n, f[0]))
            want['%s.%s' % (n, f[0])] = getattr(st, f[0]).offset
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines + ['  return 0;', '}']))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()} == want
    assert _lib.NBHD_MAX_SCALES == NB.MAX_SCALES == 8 and len(NB.STATE_FIELDS) == 10 and len(NB.OUT_FIELDS) == 12


def test_exports_have_the_headers_arities_and_the_unit_includes_the_file():
    from deepphysinet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name in ('dpn_nbhd_stage', 'dpn_nbhd_fold', 'dpn_nbhd_finish'):
        decl = re.search(r'^int %s\((.*?)\);' % name, header, flags=re.M | re.S).group(1)
        n_args = len(re.sub(r'/\*.*?\*/', '', decl, flags=re.S).split(','))
        assert _lib.EXPORTS[name][0] is ctypes.c_int and len(_lib.EXPORTS[name][1]) == n_args, name
    unit = open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_diag.hip')).read()
    includes = re.findall(r'^#include "(dpn_\w+\.inc)"', unit, flags=re.M)
    assert includes[-2:] == ['dpn_pverify.inc', 'dpn_nbhd.inc']
    inc = open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_nbhd.inc')).read()
    assert 'atomic' not in inc.replace('No atomics', '') and inc.count('#pragma clang fp contract(off)') >= 4


# ------------------------------------------------------------------------------------------------ 6. host refusals
def test_check_scales_takes_odd_ascending_widths():
    from deepphysinet_amd.neighbourhood import check_scales
    assert check_scales((1, 3, 5, 9, 17, 33)) == [0, 1, 2, 4, 8, 16] and check_scales(7) == [3] and check_scales([1.0, 2 ** 31 - 1]) == [0, 2 ** 30 - 1]
    for bad in ((), None, [2], [1, 4], [0], [-1], [3, 3], [5, 3], [1.5], [float('nan')], [float('inf')], list(range(1, 19, 2)), 'wide', [2 ** 31 + 1]):
        with pytest.raises(ValueError):
            check_scales(bad)


def test_read_analysis_checks_the_file(tmp_path):
    from deepphysinet_amd.neighbourhood import read_analysis
    g = np.random.default_rng(0)
    d = dict(names=np.array(['T', 'speed', 'q']), hours=np.array([0.0, 6.0]), analysis=g.random((3, 2, 3, 4, 5)))
    np.savez(tmp_path / 'a.npz', **d)
    got = read_analysis(str(tmp_path / 'a.npz'), ['speed', 'T'])
    assert got['analysis'].shape == (3, 2, 2, 4, 5) and got['analysis'].dtype == np.float32 and got['hours'].tolist() == [0.0, 6.0]
    assert np.array_equal(got['analysis'][:, :, 0], d['analysis'][:, :, 1].astype(np.float32)) and got['analysis'].flags['C_CONTIGUOUS']
    with pytest.raises(KeyError, match="not 'u'"):
        read_analysis(d, ['u'])
    for bad in (dict(d, analysis=d['analysis'][0]), dict(d, hours=np.zeros(3)), dict(d, analysis=d['analysis'].astype(np.int32)),
                {k: v for k, v in d.items() if k != 'names'}, dict(d, hours=np.zeros((2, 1))), dict(d, analysis=d['analysis'][:0])):
        with pytest.raises(ValueError):
            read_analysis(bad, ['T'])


def test_references_and_the_state_refuse_bad_requests():
    import torch
    from deepphysinet_amd import neighbourhood as NB
    from deepphysinet_amd.point_path import NbhdState
    from deepphysinet_amd.sampler import Lattice
    z = np.zeros((1, 1, 2, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        NB.nbhd_stage_reference(z, z, z, ([], [], []))
    with pytest.raises(ValueError):
        NB.nbhd_stage_reference(z, z[0], z, ([0], [0.5], [0]))
    with pytest.raises(ValueError):
        NB.nbhd_fold_reference(NB.nbhd_state_zeros(1, 1, 1), np.zeros((1, 1, 2, 3), np.uint8), [0], p0=1)
    lat = Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 5, 4, 3)
    ok = dict(lattice=lat, ids=[31], thr_col=[0], thr_val=[273.0], thr_side=[1], radius=[0, 2], device='cpu', budget_bytes=1 << 20)
    st = NbhdState(**ok)
    assert st.mask.shape == (3, 1, 4, 5) and st.sum_fo2.shape == (3, 1, 2) and st.n_o.shape == (3, 1) and st.planes_per_fold == 3
    assert st.buffer.numel() == 8 * (6 * 3 * 2 + 4 * 3) and st.plane_bytes == 16 * 5 * 6 + 44 * 2 * 4 and NbhdState(**dict(ok, budget_bytes=0)).planes_per_fold == 1
    for bad in (dict(ids=[]), dict(ids=[31] * 17), dict(thr_col=[], thr_val=[], thr_side=[]), dict(thr_val=[1.0, 2.0]), dict(radius=[]),
                dict(radius=list(range(9))), dict(lattice=Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 2 ** 16, 2 ** 15, 1))):
        with pytest.raises(ValueError):
            NbhdState(**dict(ok, **bad))
    with pytest.raises(ValueError):
        st.fold(planes_per_fold=4)
    with pytest.raises(ValueError):
        st.stage(torch.zeros(5, 6), torch.zeros(5, 6), torch.zeros(3, 1, 4, 4), None)


def test_verify_lattice_refuses_before_it_touches_a_case():
    """Names (KeyError), thresholds, scales and an empty case list (ValueError) are refused by the request checks alone."""
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import Lattice
    m = builder_models(**ncep_config())
    lat = Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 5, 4, 3)
    with pytest.raises(KeyError):
        m.verify_lattice([], lat, ['vorticity'], {'vorticity': 1.0}, [1, 3])
    for thresholds, scales in (({}, [1, 3]), (None, [1]), ({'T': float('nan')}, [1]), ({'u': 1.0}, [1]), ({'T': 280.0}, [2]), ({'T': 280.0}, [3, 1]),
                               ({'T': 280.0}, []), ({'T': list(range(17))}, [1]), ({'T': 280.0}, [1, 3])):
        with pytest.raises(ValueError):
            m.verify_lattice([], lat, ['T'], thresholds, scales)


# ------------------------------------------------------------------------------------------------ 7. the launcher's option
def test_infer_option_path(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    args = infer.parse.parse_args(['--verify_grid', 'T,speed', '--verify_analysis', 'a.npz', '--verify_grid_threshold', 'T:below:273.15',
                                   '--verify_grid_threshold', 'speed:10,15', '--verify_scales', '1,3,9'])
    assert infer.verify_grid_option(args) == dict(products=['T', 'speed'], analysis='a.npz', scales=[1, 3, 9],
                                                  thresholds={'T': [('below', 273.15)], 'speed': [('above', 10.0), ('above', 15.0)]})
    assert infer.verify_option(args) is None
    assert 'scales' not in infer.verify_grid_option(infer.parse.parse_args(['--verify_grid', 'T', '--verify_analysis', 'a.npz', '--verify_grid_threshold', 'T:1']))
    for argv, word in ((['--verify_grid', 'T'], 'nothing to verify against'), (['--verify_analysis', 'a.npz'], 'need --verify_grid'),
                       (['--verify_grid', 'T', '--verify_analysis', 'a.npz'], 'at least one --verify_grid_threshold'),
                       (['--verify_grid', 'T', '--verify_analysis', 'a.npz', '--verify_grid_threshold', 'T:beside:1'], '--verify_grid_threshold takes'),
                       (['--verify', 'T'], 'nothing to verify against')):
        child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--synthetic'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert child.returncode == 2 and word in child.stderr, (argv, child.stderr[-500:])
    # the loop refuses a bad option before it reads a checkpoint
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    g = np.random.default_rng(0)
    held = dict(names=np.array(['T']), hours=np.array([0.0, 6.0]), analysis=g.random((1, 2, 1, 4, 5)).astype(np.float32))
    for option, err in ((dict(products=['T'], analysis=held, thresholds={}), ValueError), (dict(products=['T'], thresholds={'T': 1.0}), ValueError),
                        (dict(products=['vorticity'], analysis=held, thresholds={'vorticity': 1.0}), KeyError),
                        (dict(products=['T'], analysis=held, thresholds={'T': 1.0}, scales=[2]), ValueError),
                        (dict(products=['u'], analysis=held, thresholds={'u': 1.0}), KeyError),
                        (dict(products=['T'], analysis=held, thresholds={'T': 1.0}, by=['all']), ValueError)):
        with pytest.raises(err):
            m.run_inference_interface(checkpoint_path=str(tmp_path / 'none'), samples='synthetic', verify_grid=option)
