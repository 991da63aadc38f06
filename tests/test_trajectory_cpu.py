"""No GPU: the host side of the parcel trajectories -- deepphysinet_amd/trajectory.py, the numpy fp64 restatement of dpn_traj_stage and the integrator
that drives it with a Python wind.  Closed forms (uniform wind), convergence orders (solid-body rotation, an accelerating rotation forward and back),
parcels that leave, the host refusals, the case table of tests/trajectory_cases.py, and six seeded mistakes, each of which must make one of the checks
here fail."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

from deepphysinet_amd import trajectory as T
from tests import trajectory_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = {m: len(rows) for m, rows in T.METHODS.items()}
ORDER = {'euler': 1, 'midpoint': 2, 'rk4': 4}
CENTRE = (128.0, 72.0)
OMEGA = 2.0 * np.pi / 24.0            # one revolution per 24 h window
DOMAIN = T.Domain(257, 145, 24, 27000.0, 13500.0)          # dy != dx: an axis mix-up shows


def _rotation(x, y, hour, dom=DOMAIN, pulse=0.0):
    """Solid-body rotation about CENTRE in index units, as a wind in m/s; pulse: its rate rises linearly over the window, from that fraction below the
    mean to that fraction above (not periodically: a sum over the steps' start hours would integrate a periodic rate exactly and hide a wrong hour)."""
    rate = OMEGA * (1.0 + pulse * (hour / 12.0 - 1.0))
    return -rate * (y - CENTRE[1]) * dom.dx / 3600.0, rate * (x - CENTRE[0]) * dom.dy / 3600.0


# ------------------------------------------------------------------------------------------------ the checks (each takes the integrator)
def check_uniform_wind(integrate):
    """A uniform wind carries every parcel along a straight line: x_K = x_0 + K h u 3600 / dx exactly (rationals below).
    Bound, per axis, in ulps of the travelled distance D = K |h kx|.  The parcels start within D of the origin side they leave from, so |x_k| <= 2 D
    all the way and the one rounding of each step's x0 + d is at most ulp(2 D) / 2 = ulp(D): K ulp(D) over K steps.  The displacement d itself is a
    product chain: kx two roundings, every stage a multiplication and an addition into the sum, h * inv_wsum two, the product with the sum one -- a
    relative error of at most (5 + 2 stages) 2^-53 on every d, so at most (5 + 2 stages) ulp(D) on their total, D 2^-53 being below ulp(D).  Together
    (K + 5 + 2 stages) ulp(D), which is below K * stages * 4 ulp(D), the bound asserted, for every K >= 3."""
    u, v = 61.0, -19.0
    x0, y0 = np.array([1.0, 2.5, 7.25, 3.0]), np.array([143.0, 140.5, 144.0, 139.25])
    for method in T.METHODS:
        for K, step in ((96, 0.25), (24, 1.0)):
            r = integrate(lambda x, y, t: (np.full_like(x, u), np.full_like(x, v)), x0, y0, 0.0, K * step, step, method, DOMAIN)
            assert r['status'].tolist() == [0] * 4 and r['steps_done'].tolist() == [K] * 4
            for axis, (start, wind, cell) in enumerate(((x0, u, DOMAIN.dx), (y0, v, DOMAIN.dy))):
                travelled = Fraction(K) * Fraction(step) * Fraction(wind) * 3600 / Fraction(cell)
                bound = K * STAGES[method] * 4 * np.spacing(abs(float(travelled)))
                for i in range(4):
                    exact = Fraction(float(start[i])) + travelled
                    err = abs(float(Fraction(float(r['positions'][K, i, axis])) - exact))
                    assert err <= bound, (method, K, axis, i, err, bound)
            # a straight line: every row lies on it to the same bound
            assert np.allclose(np.diff(r['positions'][:, :, 0], axis=0), step * u * 3600.0 / DOMAIN.dx, rtol=0, atol=1e-9)


def _closing_error(integrate, method, K, pulse=0.0, there_and_back=False):
    x0, y0 = np.array([158.0, 128.0, 100.0]), np.array([72.0, 100.0, 60.0])
    wind = functools.partial(_rotation, pulse=pulse)
    step = 24.0 / K
    r = integrate(wind, x0, y0, 0.0, 24.0, step, method, DOMAIN)
    assert r['status'].tolist() == [0, 0, 0] and r['steps_done'].tolist() == [K] * 3, (method, K, r['status'], r['steps_done'])
    end = r['positions'][K]
    if there_and_back:
        back = integrate(wind, end[:, 0], end[:, 1], 24.0, -24.0, step, method, DOMAIN)
        assert back['status'].tolist() == [0, 0, 0] and back['hours'][-1] == 0.0
        end = back['positions'][K]
    return float(np.hypot(end[:, 0] - x0, end[:, 1] - y0).max())


# (K, 2 K) per method: steps at which the restatement is in its asymptotic range and far above rounding
ROTATION_STEPS = {'euler': 512, 'midpoint': 96, 'rk4': 48}


def check_rotation_order(integrate):
    """One revolution about the domain centre closes on itself; what is left is the method's error, and halving h divides it by 2^p, p within 0.5 of the
    method's order.  The same with a rate that rises from half to one and a half times the steady one over the window (its mean is the steady rate, so the revolution still closes): there
    the hours of the stage points matter."""
    for pulse in (0.0, 0.5):
        for method, K in ROTATION_STEPS.items():
            e1, e2 = _closing_error(integrate, method, K, pulse), _closing_error(integrate, method, 2 * K, pulse)
            p = np.log2(e1 / e2)
            print('%-8s pulse %.1f closing error after one revolution: K = %4d %.3e, K = %4d %.3e, order %.2f' % (method, pulse, K, e1, 2 * K, e2, p))
            assert abs(p - ORDER[method]) <= 0.5, (method, pulse, e1, e2, p)


def check_there_and_back(integrate):
    """Forward over the window and backward over the same steps, through the rotation whose rate changes with the hour: the parcels return to their
    start to the method's order of accuracy, or one better.  One better because the way back is the way out with h negated: the leading error term
    of a method of even order p is even in h over a step pair and cancels on the round trip (midpoint returns to third order, RK4 to fifth), that of
    Euler's first order does not.  So halving h divides the miss by 2^q with order - 0.5 <= q <= order + 1.5."""
    for method, K in ROTATION_STEPS.items():
        e1 = _closing_error(integrate, method, K, pulse=0.5, there_and_back=True)
        e2 = _closing_error(integrate, method, 2 * K, pulse=0.5, there_and_back=True)
        q = np.log2(e1 / e2)
        print('%-8s there and back: K = %4d %.3e, K = %4d %.3e, order %.2f' % (method, K, e1, 2 * K, e2, q))
        assert ORDER[method] - 0.5 <= q <= ORDER[method] + 1.5, (method, e1, e2, q)
        assert e1 <= 4.0 * _closing_error(integrate, method, K, pulse=0.5), method           # and no worse than the way out alone, by more than a few


def check_parcels_that_leave(integrate):
    """A 6.75 m/s westerly is 0.9 cells an hour: at one-hour steps the parcel 2 cells from the east side completes two steps (254.9, 255.8) and leaves
    in the third, the one in the middle never.  The one that left keeps its last position, NaN rows from then on, status 1; a NaN wind stops a
    parcel with status 3; the window's end with 2."""
    wind = lambda x, y, t: (np.where(y > 100.0, np.nan, 6.75), np.zeros_like(x))
    r = integrate(wind, [254.0, 100.0, 50.0], [10.0, 20.0, 120.0], 0.0, 8.0, 1.0, 'rk4', T.Domain(257, 145, 24, 27000.0, 27000.0))
    assert r['status'].tolist() == [T.LEFT_GRID, T.ALIVE, T.BAD_WIND] and r['steps_done'].tolist() == [2, 8, 0]
    assert np.allclose(r['positions'][:3, 0], [[254.0, 10.0], [254.9, 10.0], [255.8, 10.0]], rtol=0, atol=1e-12)
    assert np.isnan(r['positions'][3:, 0]).all() and np.isfinite(r['positions'][:3, 0]).all()
    assert np.array_equal(r['last_positions'][0], r['positions'][2, 0])
    assert np.isfinite(r['positions'][:, 1]).all() and np.isnan(r['positions'][1:, 2]).all() and np.isfinite(r['positions'][0, 2]).all()
    # the clock leaves the window after 4 of 8 steps: everything still alive stops there
    r = integrate(lambda x, y, t: (np.zeros_like(x), np.zeros_like(x)), [10.0], [10.0], 20.0, 8.0, 1.0, 'euler', T.Domain(257, 145, 24, 27000.0, 27000.0))
    assert r['status'].tolist() == [T.LEFT_WINDOW] and r['steps_done'].tolist() == [4] and np.isnan(r['positions'][5:]).all()
    assert np.array_equal(r['positions'][4, 0], [10.0, 10.0])


CHECKS = (check_uniform_wind, check_rotation_order, check_there_and_back, check_parcels_that_leave)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('check', CHECKS, ids=lambda c: c.__name__)
def test_integrator(check):
    check(T.integrate_reference)


def test_host_refusals():
    wind = lambda x, y, t: (np.zeros_like(x), np.zeros_like(x))
    run = lambda **kw: T.integrate_reference(wind, **{**dict(x_idx=[10.0, 20.0], y_idx=[10.0, 20.0], hours=0.0, duration_hours=6.0, step_hours=0.25), **kw})
    assert run()['steps_done'].tolist() == [24, 24]
    with pytest.raises(ValueError, match='predict_points'):
        run(hours=[0.0, 1.0])
    with pytest.raises(ValueError, match='predict_points'):
        run(hours=np.array([0.0]))
    for kw in (dict(x_idx=[10.0, 256.5]), dict(y_idx=[-0.1, 20.0]), dict(x_idx=[10.0, np.nan]), dict(hours=24.5), dict(hours=-1.0)):
        with pytest.raises(IndexError):
            run(**kw)
    for kw in (dict(step_hours=0.0), dict(step_hours=np.nan), dict(duration_hours=0.0), dict(method='rk5'), dict(x_idx=[1.0]), dict(x_idx=[], y_idx=[])):
        with pytest.raises(ValueError):
            run(**kw)
    # direction and count: sign(duration) x |step|, round(|duration| / |step|)
    r = run(hours=12.0, duration_hours=-6.0, step_hours=0.25)
    assert r['hours'][0] == 12.0 and r['hours'][-1] == 6.0 and r['hours'].size == 25
    assert run(hours=12.0, duration_hours=-6.0, step_hours=-0.25)['hours'][-1] == 6.0


def _mistaken(kind):
    """The integrator with one seeded mistake."""
    tables = {'rk4_weight': ((1.0, 0.5, 0.5), (1.0, 0.5, 0.5), (2.0, 1.0, 1.0), (1.0, 0.0, 0.0)),
              'rk4_a_next': ((1.0, 0.5, 0.5), (2.0, 0.5, 0.5), (2.0, 0.5, 1.0), (1.0, 0.0, 0.0))}

    def run(wind, x, y, hours, duration, step, method='rk4', domain=T.Domain(257, 145, 24, 27000.0, 27000.0)):
        if kind in tables:
            return T.integrate_reference(wind, x, y, hours, duration, step, tables[kind] if method == 'rk4' else method, domain)
        return T.integrate_reference(wind, x, y, hours, duration, step, method, domain, _mistakes=(kind,))
    return run


@pytest.mark.parametrize('kind, caught_by', [('rk4_weight', check_rotation_order), ('rk4_a_next', check_rotation_order),
                                             ('c_frozen', check_there_and_back), ('no_3600', check_uniform_wind), ('dx_for_y', check_uniform_wind),
                                             ('dead_moves', check_parcels_that_leave)])
def test_seeded_mistakes_are_caught(kind, caught_by):
    """RK4 weight 2 -> 1; a_next of RK4's third stage 1 -> 1/2; the hour not advanced in the intermediate stages; the factor 3600 dropped; dx used
    for y; a dead parcel that keeps moving.  Each makes the named check fail (and that check passes on the code as it is: test_integrator)."""
    with pytest.raises(AssertionError):
        caught_by(_mistaken(kind))


def test_case_table_gives_the_statuses_it_is_built_for():
    """Every case of tests/trajectory_cases.py through traj_stage_reference: the parcels built to land exactly on a face do and stay alive, those built
    just beyond die with status 1, a NaN or an infinity in either wind column gives 3, the clock beyond the window 2 (after 3 and 1), dead parcels keep
    their status and every bit of their state, and a NaN among columns 2..5 changes nothing.  All roles occur at every size but 1, and at n = 1 over the
    cases."""
    seen, seen_single = set(), set()
    for name, case in TC.cases():
        c = TC.build(case)
        st, (xe, ye, te, moved), path = T.traj_stage_reference(c.out_n, c.state, c.domain, c.physics, c.t0, c.h, c.stage, c.inv_wsum)
        assert np.array_equal(st['status'], c.expect), name
        assert np.array_equal(moved, (c.state['status'] == 0) & (c.expect == 0)), name
        assert (path is not None) == c.stage.last
        faces = {'on_x_lo': (xe, 0.0), 'on_x_hi': (xe, 256.0), 'on_y_lo': (ye, 0.0), 'on_y_hi': (ye, 144.0)}
        for i, r in enumerate(c.roles):
            if r in faces:
                assert faces[r][0][i] == faces[r][1], (name, i, r)
            if r.startswith('beyond_'):
                off = (xe[i] if '_x_' in r else ye[i]) - (0.0 if r.endswith('lo') else (256.0 if '_x_' in r else 144.0))
                assert 0 < abs(off) < 1e-12, (name, i, r, off)
            if not moved[i]:                                  # dead before or dying now: the last completed step's state stays, bit for bit
                for key in ('x0', 'y0', 'accx', 'accy', 'steps_done'):
                    assert st[key][i] == c.state[key][i], (name, i, key)
                assert path is None or np.isnan(path[i]).all()
            elif c.stage.last:
                assert st['steps_done'][i] == c.state['steps_done'][i] + 1 and st['accx'][i] == 0.0 and np.array_equal(path[i], [xe[i], ye[i]])
        if case['t_face'] == 'on':
            assert te[0] == (24.0 if c.h > 0 else 0.0), name
        clean = np.where(np.isnan(c.out_n[:, 2:]), np.float32(0), c.out_n[:, 2:])
        st2, ev2, path2 = T.traj_stage_reference(np.concatenate([c.out_n[:, :2], clean], axis=1), c.state, c.domain, c.physics, c.t0, c.h, c.stage, c.inv_wsum)
        assert all(np.array_equal(st[k], st2[k], equal_nan=True) for k in st) and np.array_equal(ev2[3], moved)
        (seen_single if case['n'] == 1 else seen).update(c.roles)
        if case['n'] > 1:
            assert set(c.roles) == set(TC.ROLES), name
    assert seen == set(TC.ROLES) and len(seen_single) >= 12
    sizes = {case['n'] for _, case in TC.cases()}
    assert sizes == {1, 255, 256, 257}
    assert {(case['method'], case['stage']) for _, case in TC.cases()} == {(m, j) for m in T.METHODS for j in range(STAGES[m])}


def test_stage_tables():
    """Weights, nodes and the closing row of the three methods; consistency (the weights sum to 1 / inv_wsum, a_next = c_next: the stage point's hour is
    the hour its position was extrapolated to)."""
    for m, rows in T.METHODS.items():
        stages, inv_wsum = T.stage_table(m)
        assert [s.first for s in stages] == [True] + [False] * (len(rows) - 1) and [s.last for s in stages] == [False] * (len(rows) - 1) + [True]
        assert inv_wsum == 1.0 / sum(r[0] for r in rows)
        assert all(s.a_next == s.c_next for s in stages)
    assert [s.w for s in T.stage_table('rk4')[0]] == [1.0, 2.0, 2.0, 1.0] and [s.a_next for s in T.stage_table('rk4')[0]][:3] == [0.5, 0.5, 1.0]
    with pytest.raises(ValueError):
        T.stage_table('heun')


def test_unit_is_built_with_the_library_and_bound():
    """UNITS keeps its fourteen entries and their indices (other tests and tools address them); the new unit is compiled and linked through
    MORE_UNITS, into the product library and the experiment library alike."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import build as B
    names = [os.path.basename(u[0]) for u in B.UNITS]
    assert names == ['dpn_point.hip', 'dpn_wgrad.hip', 'dpn_encoder.hip', 'dpn_sampler.hip', 'dpn_fp8.hip', 'dpn_encoder_chain.hip', 'dpn_eval.hip',
                     'dpn_adaptive.hip', 'dpn_residual.hip', 'dpn_gemm.hip', 'dpn_optim.hip', 'dpn_balance.hip', 'dpn_diag.hip', 'dpn_causal.hip']
    assert [(os.path.basename(u[0]), u[1], u[2]) for u in B.MORE_UNITS] == [('dpn_traj.hip', [], 'dpn_traj.o')]
    assert B.ALL_UNITS == B.UNITS + B.MORE_UNITS and B.SRCS == [u[0] for u in B.ALL_UNITS] and len({u[2] for u in B.ALL_UNITS}) == 15
    assert os.path.join(B.HERE, 'csrc', 'dpn_traj.hip') in B.DEPS and os.path.join(B.HERE, 'csrc', 'dpn_sample_point.h') in B.DEPS
    # sample_point and denorm live in the shared header now, once
    csrc = os.path.join(ROOT, 'deepphysinet_amd', 'csrc')
    shared, sampler, traj = (open(os.path.join(csrc, f)).read() for f in ('dpn_sample_point.h', 'dpn_sampler.hip', 'dpn_traj.hip'))
    for fn in ('void sample_point(', 'float denorm('):
        assert shared.count(fn) == 1 and fn not in sampler and fn not in traj
    assert '#include "dpn_sample_point.h"' in sampler and '#include "dpn_sample_point.h"' in traj
    assert 'dpn_traj_stage' in L.EXPORTS and len(L.EXPORTS['dpn_traj_stage'][1]) == 21
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    assert 'int dpn_traj_stage(' in header and 'typedef struct DpnTrajStage' in header
    import ctypes
    assert ctypes.sizeof(L.DpnTrajStage) == 6 * 8 + 8 + 4 * 4
    assert hasattr(ctypes.CDLL(B.build_library()), 'dpn_traj_stage')             # linked in (no GPU needed to load the library)
