"""The case table of dpn_traj_stage (csrc/dpn_traj.hip): launches built in numpy, shared by tests/test_trajectory_cpu.py (the restatement gives the
status every case is built to give) and tests/test_gpu_trajectory.py (the kernel equals the restatement bit for bit on every case).

A case is one launch: n parcels (either side of the 256-thread block edge), one stage of one method, h > 0 or h < 0, the shipped physics table or u in
the squared min_max form, dy equal to dx or half of it, and optionally the shared clock placed on or just beyond the end of the hour window that this h
can reach.  Inside a launch the parcels take the ROLES in turn, starting at the case's own offset (so the single parcel of n = 1 plays another role in
every case): parcels in the interior, parcels whose next point lands exactly on each of the four side faces (alive) or on the nearest fp64 position
beyond it that a start coordinate can produce (status 1), a NaN and an infinity in either wind column (status 3), a NaN in the other four columns (no
effect on the motion), and parcels that come in dead with each status.  out_n is random; only the sign of a face parcel's wind is chosen (redrawn
until it points at the face)."""
import itertools
import types

import numpy as np

from deepphysinet_amd import trajectory as T

ROLES = ('interior', 'on_x_lo', 'on_x_hi', 'on_y_lo', 'on_y_hi', 'beyond_x_lo', 'beyond_x_hi', 'beyond_y_lo', 'beyond_y_hi', 'nan_u', 'inf_u', 'nan_v',
         'neg_inf_v', 'nan_others', 'dead_1', 'dead_2', 'dead_3', 'interior')
SIZES = (1, 255, 256, 257)
STEPS = (0.25, -0.25)
T_FACES = (None, 'on', 'beyond')
LON, LAT, HOURS, DX = 257, 145, 24, 27000.0


def physics(sq_u=False):
    """The shipped normalisation table as a plain namespace (the fields of DpnPhysics that the stage reads); sq_u: u in the squared min_max form."""
    from deepphysinet_amd.point_path import PointConfig
    ph = PointConfig().physics()
    out = types.SimpleNamespace(**{k: [getattr(ph, k)[i] for i in range(6)] for k in ('mean', 'std', 'clip_lo', 'clip_hi', 'sq_on', 'sq_add')})
    if sq_u:
        out.sq_on[0], out.sq_add[0] = 1, -4.0
    return out


def cases():
    """[(name, dict)]: every size x method x stage position x direction, the other options cycling through so that each occurs with each size."""
    out = []
    stage_ids = [(m, j) for m in ('euler', 'midpoint', 'rk4') for j in range(len(T.METHODS[m]))]
    for c, (n, (method, j), h) in enumerate(itertools.product(SIZES, stage_ids, STEPS)):
        case = dict(n=n, method=method, stage=j, h=h, offset=c, sq_u=c % 3 == 1, dy=DX / 2 if c % 4 == 2 else DX, t_face=T_FACES[(c // 2) % 3], seed=c)
        out.append(('n=%d %s[%d] h=%+g %s%s t:%s' % (n, method, j, h, 'sq_u ' if case['sq_u'] else '', 'dy=dx/2' if case['dy'] != DX else '', case['t_face']),
                    case))
    return out


def _place(face, d, outward):
    """(on, beyond): start coordinates with fl(on + d) == face and fl(beyond + d) the nearest value strictly beyond face (in direction `outward`) that
    a start coordinate reaches."""
    on = face - d
    for _ in range(8):
        if on + d == face:
            break
        on = np.nextafter(on, on + (face - (on + d)))
    assert on + d == face, (face, d)
    beyond = on
    for _ in range(8):
        beyond = np.nextafter(beyond, beyond + outward)
        if (beyond + d - face) * outward > 0:
            break
    assert (beyond + d - face) * outward > 0, (face, d)
    return on, beyond


def build(case):
    """One launch: -> namespace(out_n [n, 6] fp32, state, t0, h, stage, inv_wsum, domain, physics, roles [n], expect [n] int32 (the status after)."""
    rng = np.random.default_rng(1000 + case['seed'])
    n, h = case['n'], case['h']
    stages, inv_wsum = T.stage_table(case['method'])
    stage = stages[case['stage']]
    ph = physics(case['sq_u'])
    dom = T.Domain(LON, LAT, HOURS, DX, case['dy'])
    roles = [ROLES[(i + case['offset']) % len(ROLES)] for i in range(n)]
    # the displacement's sign per axis: toward the face of the role; interior parcels take what comes
    want = np.zeros((n, 2))
    for i, r in enumerate(roles):
        if r.endswith(('_x_lo', '_x_hi', '_y_lo', '_y_hi')):
            want[i, 0 if '_x_' in r else 1] = -1.0 if r.endswith('lo') else 1.0
    # the accumulators of a later stage: sums of earlier slopes, of the sign of this one (so that a closing stage moves toward the face as well)
    out_n = rng.standard_normal((n, 6)).astype(np.float32)
    move = np.sign(h) * want                       # the sign the slope needs
    for _ in range(200):
        uv = np.stack(T.denorm_wind(out_n, ph), axis=1)
        bad = (move != 0) & (np.sign(uv) != move)
        if not bad.any():
            break
        out_n[:, :2] = np.where(bad, rng.standard_normal((n, 2)).astype(np.float32), out_n[:, :2])
    assert not bad.any()
    u, v = T.denorm_wind(out_n, ph)
    kx, ky = (u * 3600.0) / np.float64(np.float32(dom.dx)), (v * 3600.0) / np.float64(np.float32(dom.dy))
    acc = np.zeros((n, 2))
    if case['stage'] > 0:
        acc = np.abs(rng.standard_normal((n, 2))) * 0.3 * np.sign(np.stack([kx, ky], axis=1))
    if stage.last:
        hw = np.float64(h) * np.float64(inv_wsum)
        d = np.stack([hw * (acc[:, 0] + np.float64(stage.w) * kx), hw * (acc[:, 1] + np.float64(stage.w) * ky)], axis=1)
        c_h = np.float64(h)
    else:
        ah = np.float64(stage.a_next) * np.float64(h)
        d = np.stack([ah * kx, ah * ky], axis=1)
        c_h = np.float64(stage.c_next) * np.float64(h)
    # the clock: in the middle of the window, or the end this h runs toward
    t_face = float(HOURS) if h > 0 else 0.0
    t_on, t_beyond = _place(t_face, c_h, 1.0 if h > 0 else -1.0)
    t0 = {None: 12.0, 'on': t_on, 'beyond': t_beyond}[case['t_face']]
    late = case['t_face'] == 'beyond'
    pos = np.stack([rng.uniform(20.0, LON - 21.0, n), rng.uniform(20.0, LAT - 21.0, n)], axis=1)
    status = np.zeros(n, np.int32)
    expect = np.full(n, T.LEFT_WINDOW if late else T.ALIVE, np.int32)
    for i, r in enumerate(roles):
        if r.startswith(('on_', 'beyond_')):
            ax = 0 if '_x_' in r else 1
            face = 0.0 if r.endswith('lo') else float((LON, LAT)[ax] - 1)
            on, beyond = _place(face, d[i, ax], -1.0 if r.endswith('lo') else 1.0)
            pos[i, ax] = on if r.startswith('on_') else beyond
            if r.startswith('beyond_'):
                expect[i] = T.LEFT_GRID
        elif r in ('nan_u', 'inf_u', 'nan_v', 'neg_inf_v'):
            out_n[i, 0 if r.endswith('u') else 1] = {'nan': np.nan, 'inf': np.inf, 'neg': -np.inf}[r[:3]]
            expect[i] = T.BAD_WIND
        elif r == 'nan_others':
            out_n[i, 2:] = np.nan
        elif r.startswith('dead_'):
            status[i] = expect[i] = int(r[-1])
    state = T.new_state(pos[:, 0], pos[:, 1])
    state['accx'], state['accy'], state['status'] = acc[:, 0].copy(), acc[:, 1].copy(), status
    state['steps_done'] = rng.integers(0, 5, n).astype(np.int32)
    return types.SimpleNamespace(out_n=out_n, state=state, t0=float(t0), h=float(h), stage=stage, inv_wsum=inv_wsum, domain=dom, physics=ph, roles=roles,
                                 expect=expect)
