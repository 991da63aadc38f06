"""No GPU: the host side of the threshold spells -- deepphysinet_amd/spells.py, the numpy restatement of dpn_spell_scan / _begin / _refine / _finish and
the driver that runs it over any evaluator.  Analytic series with known crossings (tests/spells_cases.py), eight seeded mistakes, each of which must
make one of those checks fail, the host refusals, the column names, the launcher's flags, the configuration key, the build lists, and the conditions
of the dense-route comparison of tests/test_gpu_spells.py on the fp64 oracle of the network."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deepphysinet_amd import extremes as X
from deepphysinet_amd import spells as S
from tests import extremes_cases as EC
from tests import spells_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the driver on analytic series
@pytest.mark.parametrize('check', SC.CHECKS, ids=lambda c: c.__name__)
def test_driver(check):
    check(S.spells_reference)


@pytest.mark.parametrize('kind', S.MISTAKES)
def test_seeded_mistakes_are_caught(kind):
    """A compare that is not strict; the entry's share of its step swapped with the exit's; part_first overwritten by a later entry; k_last and
    part_last not reset by a re-entry; the below margin not negated; k_last moved by an exit; the refinement's sides swapped; the scan's interpolated
    ends left in `hours`.  Each makes the check named in spells_cases.CAUGHT_BY fail (and that check passes on the code as it is: test_driver)."""
    assert set(SC.CAUGHT_BY) == set(S.MISTAKES) and len(S.MISTAKES) >= 6
    with pytest.raises(AssertionError):
        SC.CAUGHT_BY[kind](SC.mistaken(kind))


def test_pieces_compose_to_the_driver_and_leave_their_inputs_alone():
    """scan_reference, begin_reference, refine_reference and finish_reference called by hand give the driver's result; none modifies the state it is
    given; a state's fill never reaches a result."""
    ev = SC.fields(lambda h, p: {EC.T: np.sin(h / 2.0 + p)})
    n, K, R, t0, dt = 5, 12, 3, 1.0, 0.5
    cols = 'T:above:0.25,T:below:-0.5,T:above:2'
    want = S.spells_reference(ev, n, cols, (t0, t0 + K * dt), dt, R)
    _, ids, sides, thr = S.parse_columns(cols)
    state = S.new_state(3, n, fill=-7)

    def step(fn, *args):
        before = {key: a.copy() for key, a in state.items()}
        new = fn(*args)
        assert all(np.array_equal(state[key], before[key], equal_nan=True) for key in state)
        return new
    for k in range(K + 1):
        x = S.products_reference(ev(np.full(n, S.node_hour(t0, dt, k)), np.arange(n))[0], S.IDENTITY, False, ids, n)
        state = step(S.scan_reference, x, state, sides, thr, k, dt)
    state, m = step(S.begin_reference, state, K, t0, dt)
    assert m.shape == (6, n) and (m[4:] == t0).all()                     # the column that is never in probes t0
    for _ in range(R):
        g = S.products_reference(ev(m.reshape(-1), np.tile(np.arange(n), 6))[0], S.IDENTITY, False, [i for i in ids for _ in range(2)], n)
        state, (m_next, moved) = step(S.refine_reference, g, state, sides, thr, K)
        assert not moved[4:].any()
        m = np.where(moved, m_next, m)
    state = step(S.finish_reference, state, K, t0, dt)
    got = S.results_of(state, want['names'])
    for key in ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess', 'crossings', 'status'):
        assert EC.bitwise(got[key], want[key]), key
        assert not (got[key] == -7).any(), key
    assert got['hours'].dtype == np.float64 and got['crossings'].dtype == np.int32 and got['status'].dtype == np.int32 and got['hours'].shape == (n, 3)
    assert (got['status'][:, 2] == S.NEVER).all()


def test_compare_is_in_float32_and_the_margin_in_fp64():
    """The threshold is rounded to float32 once and the compare is a float32 compare: a value one float32 step above the rounded threshold is in, the
    rounded threshold itself is not, although 273.15 as a double lies above both."""
    req = S.check_request('T:above:273.15', (0.0, 1.0), 1.0, 0)
    thr = np.float32(273.15)
    assert req.thr == [float(thr)] and float(thr) < 273.15
    x = np.array([[thr, np.nextafter(thr, np.float32(np.inf))]], dtype=np.float32)
    st = S.scan_reference(x, S.new_state(1, 2), req.sides, req.thr, 0, 1.0)
    assert st['k_first'].tolist() == [[-1, 0]]
    st = S.scan_reference(x[:, ::-1].copy(), st, req.sides, req.thr, 1, 1.0)
    assert st['crossings'].tolist() == [[1, 1]] and st['hours'].tolist() == [[1.0, 1.0]]     # the out end's margin is 0: the whole step counts


# ------------------------------------------------------------------------------------------------ 2. names and host refusals
def test_column_names():
    assert S.parse_columns('T:below:273.15,speed:above:15') == (['T:below:273.15', 'speed:above:15'], [31, 25], [S.BELOW, S.ABOVE],
                                                                 [float(np.float32(273.15)), 15.0])
    assert S.parse_columns(['rho:above:1.2', 'u:below:-3', 'rho:above:1.2'])[1:3] == ([33, 28, 33], [S.ABOVE, S.BELOW, S.ABOVE])
    for bad in ('gust:above:3', 'T', 'T:above', 'T:max', 'T:over:3', 'vorticity:above:0', ':above:3', 'T:above:', 'T:above:3:4', [], ''):
        with pytest.raises(KeyError):
            S.parse_columns(bad)
    for bad in ('T:above:warm', 'T:above:nan', 'T:above:inf', 'T:above:1e39'):
        with pytest.raises(ValueError):
            S.parse_columns(bad)
    assert len(S.parse_columns(['T:above:1'] * 16)[0]) == 16
    with pytest.raises(ValueError):
        S.parse_columns(['T:above:1'] * 17)


def test_host_refusals_and_the_clock():
    """The window, the scan step and the rounds follow extremes.check_request: the same refusals, the same clock."""
    ok = dict(columns='T:below:273.15', window=(0.0, 24.0), scan_hours=1.0, refine=10, hours_top=24)
    r = S.check_request(**ok)
    assert (r.t0, r.dt, r.K, r.R) == (0.0, 1.0, 24, 10) and r.names == ['T:below:273.15'] and r.sides == [S.BELOW]
    for kw in (dict(window=(0.0, 24.5)), dict(window=(-1.0, 3.0)), dict(window=(5.0, 5.0)), dict(window=(6.0, 5.0)), dict(window=(0.0, float('nan'))),
               dict(window=(0.0,)), dict(window=3.0), dict(scan_hours=0.0), dict(scan_hours=-1.0), dict(scan_hours=float('inf')), dict(scan_hours=2.0 ** -11),
               dict(scan_hours=100.0), dict(refine=-1), dict(refine=33), dict(refine=2.5), dict(refine=True)):
        with pytest.raises(ValueError, match='spells'):
            S.check_request(**{**ok, **kw})
    with pytest.raises(KeyError):
        S.check_request(**{**ok, 'columns': 'gust:above:3'})
    for window, step in (((0.0, 24.0), 0.1), ((0.3, 23.9), 0.7), ((1.0, 2.0), 1.0 / 3.0), ((3.0, 4.0), 1.0)):
        a, b = S.check_request('T:above:0', window, step, 3, 24), X.check_request('T:max', window, step, 3, 24)
        assert (a.t0, a.dt, a.K, a.R) == (b.t0, b.dt, b.K, b.R)
    assert S.node_hour(0.1, 0.7, 3) == np.float64(0.1) + np.float64(3.0) * np.float64(0.7)


# ------------------------------------------------------------------------------------------------ 3. the loop's key and the launcher
def test_run_inference_interface_checks_the_spells_key_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    cfg['inference_cfg']['spells'] = dict(columns=['T:below:273.15', 'gust:above:20'], window=(0.0, 24.0))
    torch.manual_seed(0)
    m = builder_models(**cfg)
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(KeyError, match='gust'):                          # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(**nothing)
    for bad in (dict(window=(5.0, 5.0)), dict(window=(0.0, 24.0), scan_hours=0.0), dict(window=(0.0, 24.0), refine=40), dict(window=(0.0, 24.0), lonlat=[]),
                dict(window=(0.0, 24.0), columns=['T:below:cold'])):
        m.inference_cfg['spells'] = dict(dict(columns=['T:below:273.15']), **bad)
        with pytest.raises(ValueError):
            m.run_inference_interface(**nothing)
    m.inference_cfg['spells'] = dict(columns=['T:below:273.15', 'speed:above:15'], window=(0.0, 24.0), lonlat=[(100.5, 30.25)])
    with pytest.raises(NotImplementedError):                             # now the missing checkpoint is what stops it
        m.run_inference_interface(**nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_spells is None


def test_interface_refuses_a_bad_request_before_anything_runs():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import Lattice
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    field = torch.zeros(1, 159, 2405)
    with pytest.raises(RuntimeError, match='HIP device'):                # a host tensor never reaches a kernel
        m.spells_at(field, None, [1.0], [1.0], (0.0, 24.0), None, ['T:below:273.15'])
    with pytest.raises(RuntimeError, match='HIP device'):
        m.spell_lattice(field, None, Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 3, 1), (0.0, 24.0), None, ['T:below:273.15'])


def test_infer_launcher_flags_reach_the_spells_key():
    import infer
    args = infer.parse.parse_args([])
    assert args.spells is None and args.spell_window is None and infer.spells_option(args) is None
    args = infer.parse.parse_args(['--spells', 'T:below:273.15,speed:above:15', '--spell_window', '0,24', '--synthetic'])
    assert infer.spells_option(args) == dict(columns=['T:below:273.15', 'speed:above:15'], window=(0.0, 24.0), scan_hours=1.0, refine=10)
    args = infer.parse.parse_args(['--spells', 'q:above:0.01', '--spell_window', '6,18.5', '--spell_scan', '0.5', '--spell_refine', '4'])
    assert infer.spells_option(args) == dict(columns=['q:above:0.01'], window=(6.0, 18.5), scan_hours=0.5, refine=4)
    for bad in (['--spell_window', '0,24'], ['--spells', 'T:below:273.15'], ['--spells', 'T:below:273.15', '--spell_window', '0,12,24']):
        with pytest.raises(SystemExit):
            infer.spells_option(infer.parse.parse_args(bad))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "['spells'] = spells_option(args)" in src                      # ... and the launcher puts it into inference_cfg
    assert infer.extremes_option(infer.parse.parse_args(['--spells', 'T:below:273.15', '--spell_window', '0,24'])) is None


# ------------------------------------------------------------------------------------------------ 4. the build lists and the binding
def test_kernels_ride_in_the_diagnostics_unit_and_are_bound():
    """No translation unit is added: the new include file is a dependency of the library, dpn_diag.hip includes it behind dpn_extreme.inc, and the
    four entry points are declared, bound and linked; the constants agree between the header, the binding and the host module."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import build as B
    from deepphysinet_amd import point_path as PP
    assert len(B.ALL_UNITS) == 15
    csrc = os.path.join(B.HERE, 'csrc')
    assert os.path.join(csrc, 'dpn_spell.inc') in B.DEPS and not os.path.exists(os.path.join(csrc, 'dpn_spell.hip'))
    diag = open(os.path.join(csrc, 'dpn_diag.hip')).read()
    assert diag.index('#include "dpn_extreme.inc"') < diag.index('#include "dpn_spell.inc"')
    spell = open(os.path.join(csrc, 'dpn_spell.inc')).read()
    assert spell.count('#pragma clang fp contract(off)') >= 6 and 'atomic' not in spell.replace('No atomics', '') and '__shared__' not in spell
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    lib = ctypes.CDLL(B.build_library())                                  # linked in (no GPU needed to load the library)
    for name, n_args in (('dpn_spell_scan', 23), ('dpn_spell_begin', 19), ('dpn_spell_refine', 23), ('dpn_spell_finish', 7)):
        assert 'int %s(' % name in header and len(L.EXPORTS[name][1]) == n_args and hasattr(lib, name)
    assert 'typedef struct DpnSpellState' in header and ctypes.sizeof(L.DpnSpellState) == 13 * 8
    assert tuple(f[0] for f in L.DpnSpellState._fields_) == S.STATE_KEYS == PP.SpellState.KEYS
    for name, value in (('DPN_SPELL_MAX_COLUMNS', L.SPELL_MAX_COLUMNS), ('DPN_SPELL_ABOVE', L.SPELL_ABOVE), ('DPN_SPELL_BELOW', L.SPELL_BELOW),
                        ('DPN_SPELL_BAD_SCAN', L.SPELL_BAD_SCAN), ('DPN_SPELL_STOPPED', L.SPELL_STOPPED), ('DPN_SPELL_NEVER', L.SPELL_NEVER),
                        ('DPN_SPELL_HOLDS_AT_START', L.SPELL_HOLDS_AT_START), ('DPN_SPELL_HOLDS_AT_END', L.SPELL_HOLDS_AT_END)):
        assert '#define %s' % name in header and int(header.split('#define %s' % name)[1].split()[0]) == value
    assert (S.ABOVE, S.BELOW, S.MAX_COLUMNS) == (L.SPELL_ABOVE, L.SPELL_BELOW, L.SPELL_MAX_COLUMNS) == (0, 1, 16)
    assert (S.BAD_SCAN, S.STOPPED, S.NEVER, S.HOLDS_AT_START, S.HOLDS_AT_END) == (1, 2, 4, 8, 16) == \
        (L.SPELL_BAD_SCAN, L.SPELL_STOPPED, L.SPELL_NEVER, L.SPELL_HOLDS_AT_START, L.SPELL_HOLDS_AT_END)


def test_state_struct_has_the_c_compilers_layout(tmp_path):
    """DpnSpellState as gcc lays it out against the ctypes mirror: size and the offset of every field."""
    import subprocess
    from deepphysinet_amd import _lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(DpnSpellState));']
    lines += ['  printf("%%zu\\n", offsetof(DpnSpellState, %s));' % f[0] for f in L.DpnSpellState._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(L.DpnSpellState)] + [getattr(L.DpnSpellState, f[0]).offset for f in L.DpnSpellState._fields_]


# ------------------------------------------------------------------------------------------------ 5. the conditions of the dense-route comparison
def test_dense_route_conditions_hold_on_the_fp64_oracle():
    """Seed extremes_cases.DENSE_SEED, its eight stations, the five columns spells_cases.DENSE_COLUMNS, 24 h: on the fp64 oracle's one-minute series
    alone at least half of the 40 station-columns have a crossing, at most a quarter show another crossing count on the hourly nodes than on the
    minutes (a spell hidden inside a scan step), and no compared station-column with two crossings is in at both ends of the window (a gap, which the
    refinement does not touch).  With the oracle as the evaluator, spells_reference (hourly scan, R = 10, fp64) then meets the bars of
    tests/test_gpu_spells.py's comparison on every compared station-column (spells_cases.check_against_dense)."""
    n = len(EC.DENSE_STATIONS)
    ev, ph = EC.oracle_evaluator(EC.DENSE_SEED, EC.DENSE_STATIONS), EC.OraclePhysics()
    req = S.check_request(list(SC.DENSE_COLUMNS), SC.DENSE_WINDOW, SC.DENSE_SCAN, SC.DENSE_ROUNDS)
    out_n, _ = ev(np.repeat(SC.MINUTES, n), np.tile(np.arange(n), SC.MINUTES.size), want_jac=False)
    values = S.products_reference(out_n, ph, False, [28, 29, 30, 31, 32, 33], out_n.shape[0], np.float64).T.reshape(SC.MINUTES.size, n, 6)
    d = SC.dense_spells(SC.dense_series(values, req.names), req)
    compared, crossing, left_out, gaps = SC.dense_conditions(d)
    print('station-columns with a crossing %d, left out %d, gaps among the compared %d; crossings %s' % (crossing, left_out, gaps, d['crossings'].tolist()))
    assert compared.shape == (8, 5) and crossing >= 20 and left_out <= 10 and gaps == 0
    r = S.spells_reference(ev, n, list(SC.DENSE_COLUMNS), SC.DENSE_WINDOW, SC.DENSE_SCAN, SC.DENSE_ROUNDS, physics=ph, dtype=np.float64)
    assert not (r['status'] & (S.BAD_SCAN | S.STOPPED)).any()
    n_hours = SC.check_against_dense(r, d, SC.DENSE_SCAN / 2 ** SC.DENSE_ROUNDS)
    assert n_hours >= 20 and int(((d['crossings'] > 0) & (d['crossings'] <= 2) & compared).sum()) >= 10
    assert np.array_equal(r['crossings'], d['hourly'])                   # the scan counts what the hourly nodes show
