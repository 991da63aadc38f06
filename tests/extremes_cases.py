"""Cases of the window extremes (deepphysinet_amd/extremes.py), shared by tests/test_extremes_cpu.py and tests/test_gpu_extremes.py: analytic evaluators
with known extremes, the checks that drive any implementation of the driver over them (the seeded mistakes go through the same checks), and the
world of the dense-route comparison -- SyntheticSamples' cube and first field sample restated on the host, the sampler in numpy, and the fp64 oracle
of the network as an evaluator."""
import functools

import numpy as np
import torch

from deepphysinet_amd import extremes as X

U, V, P, T, Q, RHO = range(6)


def evaluator(fn):
    """evaluate(hours, points) of extremes_reference from fn(hours, points) -> {column of out_n: (value, d value / dt)}; the other columns are 0."""
    def evaluate(hours, points):
        hours = np.asarray(hours, dtype=np.float64)
        out_n, jac_n = np.zeros((hours.size, 6)), np.zeros((hours.size, 6, 3))
        for k, (v, d) in fn(hours, np.asarray(points)).items():
            out_n[:, k], jac_n[:, k, 2] = v, d
        return out_n, jac_n
    return evaluate


def bitwise(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(view)[~na], b.view(view)[~nb]))


# ------------------------------------------------------------------------------------------------ the checks (each takes the driver)
PEAKS = np.array([13.3, 12.7, 13.5, 6.02, 20.96])             # right of, left of and between scan nodes, and next to one


def check_sine(run):
    """T = 280 + 5 cos((t - a) pi / 12): the maximum at a, the minimum at a - 12 (mod 24), both inside (0, 24).  In fp64 the hour lies within
    dt / 2**R of the truth for every R (R = 0: the best scan node, half a step), the final bracket holds the truth and is dt / 2**R wide (R >= 1;
    after round 0 alone it is the one step the side's choice leaves), the value is no worse than any scan node, the status 0.  In float32 the
    values near the top tie (5 (1 - cos) falls below one float32 step of 285 within 0.013 h), so there the bracket is held to the same width and the
    hour to the bracket plus that flat stretch."""
    a = PEAKS
    w = np.pi / 12.0
    ev = evaluator(lambda h, p: {T: (280.0 + 5.0 * np.cos((h - a[p]) * w), -5.0 * w * np.sin((h - a[p]) * w))})
    low = np.where(a >= 12.0, a - 12.0, a + 12.0)
    for dtype, flat in ((np.float64, 0.0), (np.float32, 0.013)):
        for R in (0, 1, 4, 10):
            r = run(ev, a.size, ['T:max', 'T:min'], (0.0, 24.0), 1.0, R, dtype=dtype)
            assert r['status'].tolist() == [[0, 0]] * a.size, (R, r['status'])
            width = 1.0 / 2 ** R
            for j, truth in enumerate((a, low)):
                assert np.all(np.abs(r['hour'][:, j] - truth) <= max(width, 0.5 if R == 0 else 0.0) + flat), (dtype, R, j, r['hour'][:, j])
                assert np.all(r['lo'][:, j] <= truth) and np.all(truth <= r['hi'][:, j]), (dtype, R, j)
                assert np.all(r['hi'][:, j] - r['lo'][:, j] == width), (dtype, R, j, r['hi'][:, j] - r['lo'][:, j])
            assert np.all(r['value'][:, 0] >= r['scan'][:, :, 0].max(axis=0)) and np.all(r['value'][:, 1] <= r['scan'][:, :, 1].min(axis=0))
            assert np.all(np.abs(r['value'][:, 0] - 285.0) <= 5.0 * (1.0 - np.cos(width * w)) + 1e-4), (dtype, R)
            assert np.all(np.abs(r['value'][:, 1] - 275.0) <= 5.0 * (1.0 - np.cos(width * w)) + 1e-4), (dtype, R)


def check_kink(run):
    """T = -|t - a|: the slope jumps from +1 to -1 at the kink, which the bisection must find to dt / 2**R; next to a scan node (a = 13.001) the
    node itself stays the answer until a probe beats it: the result is never worse than the best scan node."""
    a = np.array([7.37, 13.001, 2.5, 22.9])
    ev = evaluator(lambda h, p: {T: (-np.abs(h - a[p]), -np.sign(h - a[p]))})
    for R in (1, 4, 10):
        r = run(ev, a.size, ['T:max'], (0.0, 24.0), 1.0, R, dtype=np.float64)
        assert r['status'][:, 0].tolist() == [0] * a.size
        assert np.all(np.abs(r['hour'][:, 0] - a) <= 1.0 / 2 ** R), (R, r['hour'][:, 0])
        assert np.all(r['value'][:, 0] >= r['scan'][:, :, 0].max(axis=0)), (R, r['value'][:, 0])
        assert np.all(r['value'][:, 0] == -np.abs(r['hour'][:, 0] - a))                       # the pair comes from one evaluation
    assert r['hour'][1, 0] != 13.0 and run(ev, a.size, ['T:max'], (0.0, 24.0), 1.0, 4, dtype=np.float64)['hour'][1, 0] == 13.0


def check_monotone(run):
    """u rises, v falls over the window (2, 20): the maximum of u and the minimum of v sit on the window's end with the slope pointing outward
    (AT_END, hour 20), the minimum of u and the maximum of v on its start (AT_START, hour 2); lo = hi = the face."""
    ev = evaluator(lambda h, p: {U: (0.5 * h + p, np.full_like(h, 0.5)), V: (-0.25 * h, np.full_like(h, -0.25))})
    for R in (0, 3):
        r = run(ev, 2, ['u:max', 'u:min', 'v:max', 'v:min'], (2.0, 20.0), 1.5, R, dtype=np.float32)
        assert r['status'].tolist() == [[X.AT_END, X.AT_START, X.AT_START, X.AT_END]] * 2, r['status']
        assert r['hour'].tolist() == [[20.0, 2.0, 2.0, 20.0]] * 2 and np.array_equal(r['lo'], r['hour']) and np.array_equal(r['hi'], r['hour'])
        assert r['value'].tolist() == [[10.0, 1.0, -0.5, -5.0], [11.0, 2.0, -0.5, -5.0]]


def check_constant(run):
    """A constant: every node ties, the first keeps the place -- node 0, hour t0 --, and with a zero slope the bracket closes on the window's start."""
    ev = evaluator(lambda h, p: {T: (np.full_like(h, 3.0), np.zeros_like(h))})
    r = run(ev, 3, ['T:max', 'T:min', 'T:mean'], (4.0, 10.0), 1.0, 5)
    assert r['value'].tolist() == [[3.0, 3.0, 3.0]] * 3 and r['hour'][:, :2].tolist() == [[4.0, 4.0]] * 3 and np.isnan(r['hour'][:, 2]).all()
    assert r['status'].tolist() == [[X.AT_START, X.AT_START, 0]] * 3


def check_two_humps(run):
    """Two humps, the later one higher: the later scan node wins and the refinement climbs that one."""
    ev = evaluator(lambda h, p: {T: (np.exp(-((h - 5.0) / 2.0) ** 2) + 1.5 * np.exp(-((h - 17.4) / 2.0) ** 2),
                                     -(h - 5.0) / 2.0 * np.exp(-((h - 5.0) / 2.0) ** 2) - 1.5 * (h - 17.4) / 2.0 * np.exp(-((h - 17.4) / 2.0) ** 2))})
    r = run(ev, 1, ['T:max'], (0.0, 24.0), 2.0, 10, dtype=np.float64)
    assert abs(r['hour'][0, 0] - 17.4) <= 2.0 / 2 ** 10 + 1e-6 and abs(r['value'][0, 0] - 1.5) < 1e-6 and r['status'][0, 0] == 0


def _speed_fields(h, p):
    eu, ev_ = 5.0 * np.exp(-((h - 9.0) / 4.0) ** 2), 6.0 * np.exp(-((h - 14.0) / 4.0) ** 2)
    return {U: (eu, -2.0 * (h - 9.0) / 16.0 * eu), V: (ev_, -2.0 * (h - 14.0) / 16.0 * ev_)}


def check_speed(run):
    """u peaks at hour 9, v, larger, at hour 14: the speed's maximum lies near 14 where u is falling and v still rising, so the sign of
    u du/dt + v dv/dt is not the sign of either term alone.  The truth is the dense fp64 maximum on a 1e-4 h lattice."""
    h = np.arange(0.0, 24.0, 1e-4)
    f = _speed_fields(h, 0)
    speed = np.hypot(f[U][0], f[V][0])
    truth = h[np.argmax(speed)]
    r = run(evaluator(_speed_fields), 1, ['speed:max', 'u:max'], (0.0, 24.0), 1.0, 10, dtype=np.float64)
    assert abs(r['hour'][0, 0] - truth) <= 1.0 / 2 ** 10 + 1e-4, (r['hour'][0, 0], truth)
    assert abs(r['value'][0, 0] - speed.max()) <= 1e-6 and abs(r['hour'][0, 1] - 9.0) <= 1.0 / 2 ** 10


def check_nan_in_scan(run):
    """A NaN at one scan node of one point: that point's columns end with BAD_SCAN and NaN everywhere, the other point is untouched."""
    def fn(h, p):
        v = 280.0 + np.sin(h / 1.5)
        return {T: (np.where((p == 1) & (h == 7.0), np.nan, v), np.cos(h / 1.5) / 1.5)}
    r = run(evaluator(fn), 2, ['T:max', 'T:min', 'T:mean'], (0.0, 12.0), 1.0, 3)
    assert r['status'].tolist() == [[0, 0, 0], [X.BAD_SCAN] * 3]
    for key in ('value', 'hour', 'lo', 'hi'):
        assert np.isnan(r[key][1]).all(), key
    assert np.isfinite(r['value'][0]).all() and np.isfinite(r['hour'][0, :2]).all()


def check_nan_in_refinement(run):
    """Point 0's slope is NaN away from the whole hours: round 0 (at the node) passes, round 1 stops the column with STOPPED and the scan's best
    stands, value and hour; point 1 goes on."""
    def fn(h, p):
        d = np.cos((h - 1.3) / 3.0) / 3.0
        return {T: (280.0 + np.sin((h - 1.3) / 3.0), np.where((p == 0) & (h != np.round(h)), np.nan, d))}
    r = run(evaluator(fn), 2, ['T:max'], (0.0, 12.0), 1.0, 6, dtype=np.float64)
    assert r['status'][:, 0].tolist() == [X.STOPPED, 0]
    k = int(np.argmax(r['scan'][:, 0, 0]))
    assert r['value'][0, 0] == r['scan'][k, 0, 0] and r['hour'][0, 0] == float(k)
    assert abs(r['hour'][1, 0] - (1.3 + 1.5 * np.pi)) <= 1.0 / 2 ** 6


def check_small(run):
    """K = 1 with R = 0 and R = 1: two nodes, the bracket is the window; a maximum inside it is approached from the better node."""
    ev = evaluator(lambda h, p: {T: (-(h - 3.3) ** 2, -2.0 * (h - 3.3))})
    r0 = run(ev, 1, ['T:max', 'T:min'], (3.0, 4.0), 1.0, 0, dtype=np.float64)
    assert r0['scan'].shape == (2, 1, 2) and r0['hour'].tolist() == [[3.0, 4.0]] and r0['status'].tolist() == [[0, X.AT_END]]
    assert r0['lo'][0, 0] == 3.0 and r0['hi'][0, 0] == 4.0
    r1 = run(ev, 1, ['T:max', 'T:min'], (3.0, 4.0), 1.0, 1, dtype=np.float64)
    assert r1['hour'].tolist() == [[3.5, 4.0]] and r1['lo'][0, 0] == 3.0 and r1['hi'][0, 0] == 3.5 and r1['value'][0, 0] == -(3.5 - 3.3) ** 2


def check_mean(run):
    """The window mean against numpy's trapezoid of the same nodes over (t1 - t0), in fp64: to 4 fp64 steps with fp64 values, and with float32
    values to one float32 rounding of the result."""
    fn = lambda h, p: {T: (280.0 + 5.0 * np.sin(h / 2.0 + p), 2.5 * np.cos(h / 2.0 + p)), Q: (1e-3 * h * h, 2e-3 * h)}
    for (t0, t1, dt) in ((0.0, 24.0, 1.0), (1.5, 19.5, 0.75), (3.0, 4.0, 1.0)):
        for dtype in (np.float64, np.float32):
            r = run(evaluator(fn), 3, ['T:mean', 'q:mean'], (t0, t1), dt, 0, dtype=dtype)
            nodes = r['scan'].astype(np.float64)                                            # [K + 1, n, C]
            trapz = getattr(np, 'trapezoid', None) or np.trapz
            want = trapz(nodes, dx=dt, axis=0) / (t1 - t0)
            if dtype == np.float64:
                assert np.all(np.abs(r['value'] - want) <= 4 * np.spacing(np.abs(want))), (t0, t1, r['value'], want)
            else:
                assert r['value'].dtype == np.float32 and np.all(np.abs(r['value'].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))
            assert np.isnan(r['hour']).all() and (r['status'] == 0).all()


CHECKS = (check_sine, check_kink, check_monotone, check_constant, check_two_humps, check_speed, check_nan_in_scan, check_nan_in_refinement, check_small,
          check_mean)
# the check that catches each seeded mistake of deepphysinet_amd.extremes.MISTAKES
CAUGHT_BY = {'min_sign': check_sine, 'tie_takes_later': check_constant, 'bracket_off_by_one': check_sine, 'best_not_kept': check_kink,
             'speed_slope_drops_v': check_speed, 'mean_end_weights': check_mean, 'face_not_detected': check_monotone}


def mistaken(kind):
    return functools.partial(X.extremes_reference, _mistakes=(kind,))


# ------------------------------------------------------------------------------------------------ the dense-route comparison
# Seed of SyntheticSamples and the 8 stations (fine-grid index units) of the comparison with the one-minute dense route.  The slope the bisection reads
# is the network's d/dt at fixed interpolated input; chosen so that on the fp64 oracle of the network the refined T:max, T:min and speed:max equal or
# exceed the dense extreme at every station (tests/test_extremes_cpu.py checks it).
DENSE_SEED = 0
DENSE_STATIONS = ((173.33, 38.03), (71.64, 49.48), (63.92, 104.59), (31.95, 48.89), (169.22, 136.51), (94.16, 138.1), (241.1, 39.22), (33.29, 63.43))
DENSE_COLUMNS = ('T:max', 'T:min', 'speed:max')


def host_world(seed):
    """SyntheticSamples(seed=seed) restated on the host: the coarse cube [6, 37, 65, 5], its first field sample [1, 159, 2405] and forecast_h."""
    g = torch.Generator().manual_seed(seed)
    cube = torch.randn(6, 37, 65, 5, generator=g)
    g = torch.Generator().manual_seed(seed * 1000 + 17)
    field = torch.randn(1, 159, 2405, generator=g)
    field[:, 155:, :] = torch.rand(1, 4, 2405, generator=g)
    return cube.numpy(), field, torch.full((1, 1, 1), 0.0)


def sample_reference(cube, xr, yr, tr, cells=0.25, t_step=6.0, dx=27000.0, dy=27000.0):
    """dpn_sample_at in numpy (csrc/dpn_sample_point.h): x, y (m), t (s) and coord_data [n, 6], each cast to float32 once; NaN outside the cube."""
    xr, yr, tr = (np.asarray(v, dtype=np.float64) for v in (xr, yr, tr))
    _, ny, nx, nt = cube.shape
    fx, fy, ft = xr * cells, yr * cells, tr / t_step
    ix, iy, it = (np.clip(np.floor(f).astype(np.int64), 0, top - 2) for f, top in ((fx, nx), (fy, ny), (ft, nt)))
    wx, wy, wt = fx - ix, fy - iy, ft - it
    inside = (wx >= 0) & (wx <= 1) & (wy >= 0) & (wy <= 1) & (wt >= 0) & (wt <= 1)
    c = cube.astype(np.float64)
    g = lambda dy_, dx_, dt_: c[:, iy + dy_, ix + dx_, it + dt_]                              # [6, n]
    lo = (g(0, 0, 0) * (1 - wt) + g(0, 0, 1) * wt) * (1 - wx) + (g(0, 1, 0) * (1 - wt) + g(0, 1, 1) * wt) * wx
    hi = (g(1, 0, 0) * (1 - wt) + g(1, 0, 1) * wt) * (1 - wx) + (g(1, 1, 0) * (1 - wt) + g(1, 1, 1) * wt) * wx
    cd = np.where(inside, lo * (1 - wy) + hi * wy, np.nan).T.astype(np.float32)
    return (xr * dx).astype(np.float32), (yr * dy).astype(np.float32), (tr * 3600.0).astype(np.float32), cd


class OraclePhysics:
    """The shipped de-normalisation (oracle/dpn_oracle.py) as a physics table of extremes_reference; nothing is clipped."""

    def __init__(self):
        from oracle import dpn_oracle as O
        self.mean, self.std = tuple(O.OBS_MEAN), tuple(O.OBS_STD)
        self.clip_lo = self.clip_hi = self.sq_add = (0.0,) * 6
        self.clip_on = self.sq_on = (0,) * 6


def oracle_evaluator(seed, stations):
    """evaluate(hours, points) over the fp64 oracle of the network (oracle/dpn_oracle.py) with the seeded weights of the parity tests, the field sample
    of host_world(seed) and the inputs the device sampler would hand the forward (float32, taken as they are): out_n [m, 6] and jac_n [m, 6, 3]
    of which only d/dt is filled."""
    from oracle import dpn_oracle as O
    cube, field, fh = host_world(seed)
    state = O.make_state(dtype=torch.float64)
    field, fh = field.double(), fh.double()
    with torch.no_grad():
        meta = O.meta_net_forward(state, field, fh)
    xs, ys = (np.array([s[j] for s in stations], dtype=np.float64) for j in (0, 1))
    geo = O.Geometry()

    def evaluate(hours, points, want_jac=True):
        x, y, t, cd = sample_reference(cube, xs[points], ys[points], hours)
        col = lambda v: torch.from_numpy(v.astype(np.float64)).reshape(-1, 1)
        tt = col(t).requires_grad_(want_jac)
        with torch.set_grad_enabled(want_jac):
            fields = O.physics_net_forward(state, field, O.encoding_coord(col(x), col(y), tt, geo), torch.from_numpy(cd.astype(np.float64)), fh, meta_out=meta)
        out_n = torch.cat(fields, dim=1).detach().numpy()
        jac_n = np.zeros((out_n.shape[0], 6, 3))
        if want_jac:
            for k in range(6):
                jac_n[:, k, 2] = torch.autograd.grad(fields[k].sum(), tt, retain_graph=k < 5)[0].reshape(-1).numpy()
        return out_n, jac_n
    return evaluate


def dense_extremes(values):
    """(T:max, T:min, speed:max) [n] of de-normalised rows values [nt, n, 6]."""
    speed = np.sqrt(values[..., 0] * values[..., 0] + values[..., 1] * values[..., 1])
    return values[..., 3].max(axis=0), values[..., 3].min(axis=0), speed.max(axis=0)
