"""Parcel trajectories through the learned wind field (csrc/dpn_traj.hip): the stage tables of the integrators, the host checks
of a request, and the numpy fp64 restatement of what dpn_traj_stage defines.

A parcel at (x, y) in fine-grid index units moves with dx/dt = u * 3600 / dx_metres, dy/dt = v * 3600 / dy_metres index units per hour, u and v the
network's de-normalised wind at the parcel.  One explicit Runge-Kutta step is a sequence of stages, each of which needs only the step's start point and
the previous stage's slope; on the device one stage is one fields-only forward and one dpn_traj_stage launch (InterfacePhysics.trajectories).
`traj_stage_reference` restates that launch operation by operation -- the kernel is compiled without contraction, so state, path and status agree bit
for bit --, and `integrate_reference` drives the same stage with a Python wind callback instead of the network: for tests without a GPU, and for
users without one.  Nothing here runs in the device path except METHODS, stage_table and check_request.
"""
from collections import namedtuple

import numpy as np

ALIVE, LEFT_GRID, LEFT_WINDOW, BAD_WIND = 0, 1, 2, 3      # DPN_TRAJ_* (include/dpn_hip.h)

# Rows (w, a_next, c_next), one per stage: the weight of the stage's slope in the step's sum, and where the NEXT stage evaluates the wind -- a_next * h
# along this slope from the step's start point, at hour t0 + c_next * h.  The last row closes the step (its a_next, c_next are not read).
METHODS = {
    'euler': ((1.0, 0.0, 0.0),),
    'midpoint': ((0.0, 0.5, 0.5), (1.0, 0.0, 0.0)),
    'rk4': ((1.0, 0.5, 0.5), (2.0, 0.5, 0.5), (2.0, 1.0, 1.0), (1.0, 0.0, 0.0)),
}

Stage = namedtuple('Stage', 'w a_next c_next first last')
# The box a parcel lives in: 0 <= x <= lon_size - 1, 0 <= y <= lat_size - 1, 0 <= hour <= hours; dx, dy: metres per fine cell (DpnSampler's fp32 values).
Domain = namedtuple('Domain', 'lon_size lat_size hours dx dy')


def domain_of(sampler_struct):
    """The Domain of a DpnSampler (CollocationSampler._s)."""
    s = sampler_struct
    return Domain(int(s.lon), int(s.lat), int(s.t_hours), float(s.dx), float(s.dy))


def stage_table(method):
    """([Stage, ...], inv_wsum) of a method name of METHODS, or of a table of (w, a_next, c_next) rows.  ValueError on an unknown name."""
    if isinstance(method, str):
        if method not in METHODS:
            raise ValueError('trajectories: unknown method %r; one of %s' % (method, ', '.join(sorted(METHODS))))
        rows = METHODS[method]
    else:
        rows = tuple(tuple(float(v) for v in r) for r in method)
    wsum = float(sum(r[0] for r in rows))
    if not rows or not np.isfinite(wsum) or wsum == 0.0:
        raise ValueError('trajectories: a stage table needs at least one row and a non-zero weight sum')
    n = len(rows)
    return [Stage(float(w), float(a), float(c), j == 0, j == n - 1) for j, (w, a, c) in enumerate(rows)], 1.0 / wsum


def check_request(x_idx, y_idx, hours, duration_hours, step_hours, method, domain):
    """The host checks of a trajectory request, once, before anything is launched: -> (x [N] fp64, y [N] fp64, t0, h, K, stages, inv_wsum).
    ValueError: a start hour that is not one scalar (parcels of one call share the clock: evaluate other sets with predict_points), x_idx and y_idx of
    different or zero length, a zero or non-finite step or duration, an unknown method.  IndexError: a start position or hour outside the domain
    (a NaN is outside).  h = sign(duration_hours) * |step_hours|, K = round(|duration_hours| / |step_hours|) steps (at least one)."""
    stages, inv_wsum = stage_table(method)
    if np.ndim(hours) != 0:
        raise ValueError('trajectories: all parcels of a call start at the same hour, so `hours` is one scalar (got shape %r); evaluate fields at '
                         'arbitrary (position, hour) sets with predict_points' % (np.shape(hours),))
    t0 = float(hours)
    x, y = (np.ascontiguousarray(np.atleast_1d(np.asarray(v)), dtype=np.float64).reshape(-1) for v in (x_idx, y_idx))
    if x.size == 0 or x.size != y.size:
        raise ValueError('trajectories: x_idx and y_idx must have the same, non-zero length')
    step, duration = float(step_hours), float(duration_hours)
    if not (np.isfinite(step) and step != 0.0):
        raise ValueError('trajectories: step_hours must be finite and non-zero, got %r' % (step_hours,))
    if not (np.isfinite(duration) and duration != 0.0):
        raise ValueError('trajectories: duration_hours must be finite and non-zero (its sign is the direction), got %r' % (duration_hours,))
    for v, top in ((x, domain.lon_size - 1), (y, domain.lat_size - 1), (np.array([t0]), domain.hours)):
        if not (np.all(v >= 0.0) and np.all(v <= top)):                  # (NaN fails both)
            raise IndexError('trajectories: start position / hour outside the domain')
    h = abs(step) if duration > 0 else -abs(step)
    K = max(1, int(round(abs(duration) / abs(step))))
    return x, y, t0, h, K, stages, inv_wsum


def new_state(x, y):
    """The state of n parcels at the start points x, y: x0, y0, accx, accy [n] fp64, status, steps_done [n] int32."""
    x, y = np.array(x, dtype=np.float64).reshape(-1), np.array(y, dtype=np.float64).reshape(-1)
    n = x.size
    return {'x0': x, 'y0': y, 'accx': np.zeros(n), 'accy': np.zeros(n), 'status': np.zeros(n, np.int32), 'steps_done': np.zeros(n, np.int32)}


def denorm_wind(out_n, physics):
    """u, v [n] fp64 = (double) of dpn_fields_out's fp32 de-normalisation of columns 0 and 1 of out_n [n, 6]: out * std, + mean, the squared min_max
    form v * v, + sq_add, each one fp32 operation; never clipped."""
    return tuple(denorm_column(out_n, k, physics, False).astype(np.float64) for k in (0, 1))


def denorm_column(out_n, k, physics, with_clip):
    """Column k of out_n [n, 6] de-normalised in fp32 as dpn_fields_out does it (the clip of P, T, q, rho lets a NaN through)."""
    f32 = np.float32
    o = np.asarray(out_n, dtype=f32)[:, k]
    with np.errstate(invalid='ignore', over='ignore'):
        v = o * f32(physics.std[k])
        v = v + f32(physics.mean[k])
        if physics.sq_on[k]:
            v = v * v
            v = v + f32(physics.sq_add[k])
        if with_clip and k >= 2:
            v = np.where(np.isnan(v), v, np.fmin(np.fmax(v, f32(physics.clip_lo[k])), f32(physics.clip_hi[k]))).astype(f32)
    return v


def fields_row_reference(out_n, status, physics, with_clip):
    """The fields row [n, 6] fp32 that a first or record_only launch writes: the de-normalised fields of parcels with status 0, NaN for the others."""
    row = np.stack([denorm_column(out_n, k, physics, with_clip) for k in range(6)], axis=1)
    row[np.asarray(status) != ALIVE] = np.nan
    return row


def _stage(u, v, state, domain, t0, h, stage, inv_wsum, mistakes=()):
    """dpn_traj_stage's arithmetic for winds u, v [n] fp64 (m/s): -> (state', (xe, ye, te, moved), path row [n, 2] or None).  Every line is one fp64
    operation per parcel, in the order include/dpn_hip.h writes them.  moved [n] bool: the parcels whose evaluation point was written (alive before
    and after); xe, ye, te are NaN-free only there.  mistakes: names of seeded errors (tests/test_trajectory_cpu.py)."""
    f64 = np.float64
    u, v = np.asarray(u, dtype=f64), np.asarray(v, dtype=f64)
    t0, h, w, a_next, c_next, inv_wsum = (f64(s) for s in (t0, h, stage.w, stage.a_next, stage.c_next, inv_wsum))
    sec = f64(1.0 if 'no_3600' in mistakes else 3600.0)
    dx, dy = f64(np.float32(domain.dx)), f64(np.float32(domain.dx if 'dx_for_y' in mistakes else domain.dy))
    st = {k: a.copy() for k, a in state.items()}
    alive = state['status'] == ALIVE
    with np.errstate(invalid='ignore', over='ignore'):
        kx = (u * sec) / dx
        ky = (v * sec) / dy
        ax = state['accx'] + w * kx
        ay = state['accy'] + w * ky
        if stage.last:
            hw = h * inv_wsum
            xe = state['x0'] + hw * ax
            ye = state['y0'] + hw * ay
            te = t0 + h
        else:
            ah = a_next * h
            xe = state['x0'] + ah * kx
            ye = state['y0'] + ah * ky
            te = t0 + c_next * h
        in_grid = (xe >= 0.0) & (xe <= f64(domain.lon_size - 1)) & (ye >= 0.0) & (ye <= f64(domain.lat_size - 1))
        in_window = bool(te >= 0.0 and te <= f64(domain.hours))
    status = np.where(~(np.isfinite(u) & np.isfinite(v)), BAD_WIND, np.where(~in_grid, LEFT_GRID, ALIVE if in_window else LEFT_WINDOW)).astype(np.int32)
    st['status'] = np.where(alive, status, state['status']).astype(np.int32)
    moved = alive & (status == ALIVE)
    if 'dead_moves' in mistakes:                              # a parcel that has left goes on as if nothing had happened
        moved = np.ones_like(moved)
    path = None
    if stage.last:
        st['x0'] = np.where(moved, xe, state['x0'])
        st['y0'] = np.where(moved, ye, state['y0'])
        st['accx'] = np.where(moved, 0.0, state['accx'])
        st['accy'] = np.where(moved, 0.0, state['accy'])
        st['steps_done'] = (state['steps_done'] + moved).astype(np.int32)
        path = np.where(moved[:, None], np.stack([xe, ye], axis=1), np.nan)
    else:
        st['accx'] = np.where(moved, ax, state['accx'])
        st['accy'] = np.where(moved, ay, state['accy'])
    return st, (xe, ye, np.full(xe.shape, te), moved), path


def traj_stage_reference(out_n, state, domain, physics, t0, h, stage, inv_wsum):
    """One dpn_traj_stage launch (not record_only) restated in numpy fp64: out_n [n, 6] fp32 (the forward at the current evaluation points), state (a
    dict as new_state gives it; not modified), domain (Domain), physics (a DpnPhysics or anything with its mean, std, sq_on, sq_add), the step's
    start hour t0, the step h, stage (a Stage), inv_wsum.  -> (state', (xe, ye, te, moved), path row [n, 2] or None): the new state; the next
    evaluation points with moved [n] bool marking the parcels whose x, y, t, f, coord_data the kernel wrote (the others keep what they had); the path
    row step + 1 when the stage closes the step.  The fields row of a first stage is fields_row_reference(out_n, state['status'], ...)."""
    u, v = denorm_wind(out_n, physics)
    return _stage(u, v, state, domain, t0, h, stage, inv_wsum)


def integrate_reference(wind, x_idx, y_idx, hours, duration_hours, step_hours, method='rk4', domain=Domain(257, 145, 24, 27000.0, 27000.0),
                        _mistakes=()):
    """InterfacePhysics.trajectories with a Python wind in place of the network: wind(x, y, hour) -> (u, v) in m/s, arrays [N] of fp64, x and y in
    fine-grid index units.  Same host checks (check_request), same stages (the arithmetic of traj_stage_reference), same outputs:
    {'positions' [K + 1, N, 2] fp64 (NaN from the step a parcel left in), 'hours' [K + 1], 'status' [N], 'steps_done' [N]}.  A parcel that leaves
    keeps its last completed step's position in 'last_positions' [N, 2]; its wind is still asked for, at its last valid evaluation point, and
    ignored.  method: a name of METHODS or a table of (w, a_next, c_next) rows."""
    x, y, t0, h, K, stages, inv_wsum = check_request(x_idx, y_idx, hours, duration_hours, step_hours, method, domain)
    if 'c_frozen' in _mistakes:                               # the hour is not advanced in the intermediate stages
        stages = [s._replace(c_next=0.0) for s in stages]
    state = new_state(x, y)
    xe, ye, te = x.copy(), y.copy(), np.full(x.shape, t0)
    positions = np.full((K + 1, x.size, 2), np.nan)
    positions[0, :, 0], positions[0, :, 1] = x, y
    hrs = np.empty(K + 1)
    hrs[0] = t0
    for k in range(K):
        for stage in stages:
            u, v = wind(xe.copy(), ye.copy(), te.copy())
            state, (nx, ny, nt, moved), row = _stage(u, v, state, domain, t0, h, stage, inv_wsum, _mistakes)
            xe, ye, te = np.where(moved, nx, xe), np.where(moved, ny, ye), np.where(moved, nt, te)
        positions[k + 1] = row
        t0 = t0 + h
        hrs[k + 1] = t0
    return {'positions': positions, 'hours': hrs, 'status': state['status'], 'steps_done': state['steps_done'],
            'last_positions': np.stack([state['x0'], state['y0']], axis=1)}
