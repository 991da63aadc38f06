"""GPU (MI355X): parcel trajectories -- dpn_traj_stage against its numpy restatement on the case table of tests/trajectory_cases.py, its refusals,
InterfacePhysics.trajectories against a loop of the entry points that existed before it, the fields along the path, parcel chunks, degrees, and
infer.py --trajectories.

Yardsticks: deepphysinet_amd.trajectory.traj_stage_reference (fp64, bit for bit: the kernel is compiled without contraction), dpn_sample_at at the same
fp64 positions (bit for bit: the same device function), and for the end-to-end run the composed route sample_at -> fields-only forward ->
traj_stage_reference on the host, which evaluates the same forward on the same bits."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deepphysinet_amd import trajectory as T
from tests import trajectory_cases as TC
from tests.test_gpu_parity import _dev, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7.0
_cache = {}


def _world():
    """Model, sampler and field sample, once: the seeded hi+lo model of the parity tests and SyntheticSamples' cube and first sample."""
    if not _cache:
        from deepphysinet_amd.sampler import SyntheticSamples
        syn = SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=1)
        b = syn[0]
        _cache.update(m=_model('bf16x2'), s=syn.sampler, field=b['field_data'].to(_dev()), fh=b['forecast_h'].to(_dev()))
    return _cache


def _same(got, want):
    """Bit for bit, a NaN matching any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan_g, nan_w = (np.isnan(a) if a.dtype.kind == 'f' else np.zeros(a.shape, bool) for a in (got, want))
    return np.array_equal(nan_g, nan_w) and np.array_equal(got.view(view)[~nan_g], want.view(view)[~nan_w])


def _dev_physics(ph):
    from deepphysinet_amd.point_path import PointConfig
    out = PointConfig().physics()
    for k in range(6):
        out.sq_on[k], out.sq_add[k] = int(ph.sq_on[k]), float(ph.sq_add[k])
    return out


class _Launch:
    """The device side of one launch: state, path, fields and sampler outputs, all holding FILL where the case has no value of its own."""

    def __init__(self, c, s, rows=3, step=1, fields=True, with_clip=False, record_only=False):
        from deepphysinet_amd import _lib as L
        dev, n = _dev(), c.out_n.shape[0]
        self.n, self.rows, self.L = n, rows, L
        self.sampler = L.DpnSampler.from_buffer_copy(s._s)
        self.sampler.dy = c.domain.dy
        self.cube = s.cube
        self.ph = _dev_physics(c.physics)
        self.out_n = torch.from_numpy(c.out_n).to(dev)
        self.state = {k: torch.from_numpy(v.copy()).to(dev) for k, v in c.state.items()}
        self.path = torch.full((rows, n, 2), FILL, dtype=torch.float64, device=dev)
        self.fields = torch.full((rows, n, 6), FILL, dtype=torch.float32, device=dev) if fields else None
        self.points = [torch.full((n,), FILL, dtype=torch.float32, device=dev) for _ in range(4)] + [torch.full((n, 6), FILL, dtype=torch.float32, device=dev)]
        self.st = L.DpnTrajStage(c.t0, c.h, c.stage.w, c.stage.a_next, c.stage.c_next, c.inv_wsum, step, int(c.stage.first), int(c.stage.last),
                                 int(record_only), int(with_clip))

    def args(self, **over):
        from deepphysinet_amd.point_path import _ptr, _stream
        by, s = ctypes.byref, self.state
        a = dict(s=by(self.sampler), cube=_ptr(self.cube), phys=by(self.ph), out_n=_ptr(self.out_n), n=self.n, st=by(self.st), x0=_ptr(s['x0']),
                 y0=_ptr(s['y0']), accx=_ptr(s['accx']), accy=_ptr(s['accy']), status=_ptr(s['status']), steps_done=_ptr(s['steps_done']),
                 path=_ptr(self.path), path_rows=self.rows, fields=_ptr(self.fields), x=_ptr(self.points[0]), y=_ptr(self.points[1]),
                 t=_ptr(self.points[2]), f=_ptr(self.points[3]), coord_data=_ptr(self.points[4]))
        a.update(over)
        return list(a.values()) + [_stream()]

    def run(self, **over):
        return self.L.load().dpn_traj_stage(*self.args(**over))

    def sample_at(self, xe, ye, te):
        """dpn_sample_at with this launch's sampler struct at fp64 positions."""
        from deepphysinet_amd.point_path import _ptr, _stream
        dev, n = _dev(), self.n
        pos = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in (xe, ye, te)]
        out = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)] + [torch.empty((n, 6), dtype=torch.float32, device=dev)]
        assert self.L.load().dpn_sample_at(ctypes.byref(self.sampler), _ptr(self.cube), _ptr(pos[0]), _ptr(pos[1]), _ptr(pos[2]), None, 0, n,
                                           *[_ptr(v) for v in out], _stream()) == 0
        return [v.cpu().numpy() for v in out]


# ------------------------------------------------------------------------------------------------ 1. the kernel against its restatement
@pytest.mark.parametrize('n', TC.SIZES)
def test_kernel_is_the_restatement_bit_for_bit(n):
    """Every case of the table with this n (all stage positions of the three methods, both directions, u in the affine and the squared form, dy = dx
    and dx / 2, the clock inside, on and beyond the window's end): x0, y0, accx, accy, status, steps_done and the path row equal
    traj_stage_reference bit for bit; x, y, t, f, coord_data of the parcels that moved equal dpn_sample_at at the restatement's fp64 evaluation points
    bit for bit, those of the others still hold what they held (finite); a first stage's fields row equals fields_row_reference, without and with
    the clip; rows that the launch does not own keep their fill."""
    s = _world()['s']
    ran = 0
    for ci, (name, case) in enumerate(TC.cases()):
        if case['n'] != n:
            continue
        c = TC.build(case)
        clip = ci % 2 == 1
        run = _Launch(c, s, fields=c.stage.first, with_clip=clip)
        assert run.run() == 0, name
        torch.cuda.synchronize()
        want, (xe, ye, te, moved), row = T.traj_stage_reference(c.out_n, c.state, c.domain, c.physics, c.t0, c.h, c.stage, c.inv_wsum)
        assert np.array_equal(want['status'], c.expect), name
        for key in want:
            assert _same(run.state[key].cpu().numpy(), want[key]), (name, key)
        path = run.path.cpu().numpy()
        assert (path[[0, 1]] == FILL).all(), name
        assert _same(path[2], row) if c.stage.last else (path[2] == FILL).all(), name
        got = [v.cpu().numpy() for v in run.points]
        assert all(np.isfinite(g).all() for g in got), name                     # nothing dead, dying or alive ever holds a NaN for the forward
        safe = [np.where(moved, v, 1.0) for v in (xe, ye, te)]
        ref = run.sample_at(*safe)
        for g, r_, what in zip(got, ref, ('x', 'y', 't', 'f', 'coord_data')):
            assert _same(g[moved], r_[moved]), (name, what)
            assert (g[~moved] == FILL).all(), (name, what)
        if c.stage.first:
            fields = run.fields.cpu().numpy()
            assert _same(fields[1], T.fields_row_reference(c.out_n, c.state['status'], c.physics, clip)), name
            assert (fields[[0, 2]] == FILL).all(), name
        ran += 1
    assert ran == 14


def test_record_only_writes_the_fields_row_and_nothing_else():
    s = _world()['s']
    c = TC.build(dict(TC.cases()[-1][1], n=257))
    for clip in (False, True):
        run = _Launch(c, s, step=2, with_clip=clip, record_only=True)
        assert run.run() == 0
        torch.cuda.synchronize()
        fields = run.fields.cpu().numpy()
        assert _same(fields[2], T.fields_row_reference(c.out_n, c.state['status'], c.physics, clip)) and (fields[:2] == FILL).all()
        for key, v in c.state.items():
            assert _same(run.state[key].cpu().numpy(), v), key
        assert bool((run.path == FILL).all()) and all(bool((p == FILL).all()) for p in run.points)
    assert np.isnan(fields[2][c.state['status'] != 0]).all() and (c.state['status'] != 0).any()


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_entry_point_refuses_bad_arguments_and_writes_nothing():
    s = _world()['s']
    name, case = next((nm, cs) for nm, cs in TC.cases() if cs['n'] == 257 and cs['method'] == 'rk4' and cs['stage'] == 0)
    c = TC.build(case)
    run = _Launch(c, s)
    L = run.L
    before = {k: v.clone() for k, v in run.state.items()}

    def stage(**kw):
        st = L.DpnTrajStage.from_buffer_copy(run.st)
        for k, v in kw.items():
            setattr(st, k, v)
        return dict(st=ctypes.byref(st))
    bad_sampler = L.DpnSampler.from_buffer_copy(run.sampler)
    bad_sampler.t_in = 1
    nan, inf = float('nan'), float('inf')
    cases = [{k: None} for k in ('s', 'cube', 'phys', 'out_n', 'st', 'x0', 'y0', 'accx', 'accy', 'status', 'steps_done', 'path', 'x', 'y', 't', 'f',
                                 'coord_data')]
    cases += [dict(n=0), dict(n=-3), dict(s=ctypes.byref(bad_sampler)), stage(h=0.0), stage(h=nan), stage(h=inf), stage(h=-inf), stage(w=nan),
              stage(a_next=inf), stage(c_next=nan), stage(inv_wsum=inf), stage(t0=nan), stage(step=-1), stage(step=2), stage(step=3), dict(path_rows=2),
              stage(first=0), stage(record_only=1, step=3), stage(first=0, last=1), dict(fields=None, **stage(record_only=1))]
    for over in cases:
        assert run.run(**over) == -1, sorted(over)
    torch.cuda.synchronize()
    assert bool((run.path == FILL).all()) and bool((run.fields == FILL).all()) and all(bool((p == FILL).all()) for p in run.points)
    for k, v in before.items():
        assert torch.equal(run.state[k], v), k
    assert run.run() == 0 and run.run(**stage(record_only=1, step=2)) == 0 and run.run(fields=None, **stage(first=0)) == 0      # and the same arguments, accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. end to end
N_PARCELS, K_STEPS = 200, 8


def _starts():
    """200 parcels: 160 anywhere at least 12 cells inside, 40 within one cell of a side (ten per side), some of which the wind carries out."""
    g = np.random.default_rng(3)
    x, y = 12.0 + g.random(N_PARCELS) * 232.0, 12.0 + g.random(N_PARCELS) * 120.0
    near = g.random(40) * 0.999 + 0.001
    x[160:170], x[170:180] = near[:10], 256.0 - near[10:20]
    y[180:190], y[190:200] = near[20:30], 144.0 - near[30:40]
    return x, y


def _composed(W, xs, ys, t0, h, K, method, with_clip):
    """The route a user could compose before: per stage dpn_sample_at at host positions, the fields-only forward of PackedField (the call that
    PackedField.fields makes, which hands out only de-normalised rows: the normalised ones are taken from the same forward), the stage on the host
    (traj_stage_reference), the fields along the path from PackedField.fields."""
    from deepphysinet_amd import point_path as PP
    m, s = W['m'], W['s']
    n, dev = xs.size, _dev()
    pf = m._inference_weights(W['field'], W['fh'], n)
    dom, ph = T.domain_of(s._s), pf.cfg.physics()
    stages, inv_wsum = T.stage_table(method)
    state = T.new_state(xs, ys)
    xe, ye, te = xs.copy(), ys.copy(), np.full(n, t0)
    positions, fields, hours = np.full((K + 1, n, 2), np.nan), np.full((K + 1, n, 6), np.nan, np.float32), [t0]
    positions[0, :, 0], positions[0, :, 1] = xs, ys

    def forward(record):
        x, y, t, f, cd = s.sample_at(n, *[torch.from_numpy(v).to(dev) for v in (xe, ye, te)])
        out_n, _ = PP._forward_points(pf.cfg, pf.ws, pf.nets, x, y, t, None, cd, want_jac=False, want_saved=False)
        if record is not None:
            rows = torch.empty((n, 6), dtype=torch.float32, device=dev)
            pf.fields(x, y, t, cd, with_clip, rows=rows)
            fields[record] = np.where((state['status'] == 0)[:, None], rows.cpu().numpy(), np.float32(np.nan))
        return out_n.cpu().numpy()
    for k in range(K):
        for stage in stages:
            out_n = forward(k if stage.first else None)
            state, (nx, ny, nt, moved), row = T.traj_stage_reference(out_n, state, dom, ph, hours[k], h, stage, inv_wsum)
            xe, ye, te = np.where(moved, nx, xe), np.where(moved, ny, ye), np.where(moved, nt, te)
        positions[k + 1] = row
        hours.append(hours[k] + h)
    forward(K)
    return dict(positions=positions, hours=np.array(hours), status=state['status'], steps_done=state['steps_done'], fields=fields)


def _run(W, key, **kw):
    if key not in W:
        x, y = _starts()
        args = dict(x_idx=x, y_idx=y, hours=2.0, duration_hours=8.0, step_hours=1.0, method='rk4', with_fields=True)
        args.update(kw)
        r = W['m'].trajectories(W['field'], W['s'], args.pop('x_idx'), args.pop('y_idx'), args.pop('hours'), W['fh'], **args)
        W[key] = {k: v.cpu().numpy() for k, v in r.items()}
    return W[key]


@pytest.mark.parametrize('direction', ['forward', 'backward'])
def test_trajectories_equal_the_composed_route_bit_for_bit(direction):
    """200 parcels, 8 RK4 steps of one hour forward from hour 2 and backward from hour 20, without and with the clip of the recorded fields: positions,
    status, steps_done, hours and fields equal the composed route's bit for bit; some of the parcels near a side leave (NaN rows from then on), most
    do not."""
    W = _world()
    kw = dict(hours=2.0, duration_hours=8.0) if direction == 'forward' else dict(hours=20.0, duration_hours=-8.0, with_clip=True)
    got = _run(W, direction, **kw)
    x, y = _starts()
    want = _composed(W, x, y, kw['hours'], 1.0 if direction == 'forward' else -1.0, K_STEPS, 'rk4', bool(kw.get('with_clip')))
    for key in ('positions', 'hours', 'status', 'steps_done', 'fields'):
        assert _same(got[key], want[key]), key
    left = got['status'] != 0
    print('%s: %d of %d parcels left (status %s), steps done %s' % (direction, left.sum(), N_PARCELS, sorted(set(got['status'].tolist())),
                                                                   sorted(set(got['steps_done'].tolist()))))
    assert 0 < left.sum() < 40 and not left[:160].any() and set(got['status'][left].tolist()) == {T.LEFT_GRID}
    assert got['positions'].shape == (K_STEPS + 1, N_PARCELS, 2) and got['fields'].shape == (K_STEPS + 1, N_PARCELS, 6)
    assert (got['steps_done'][~left] == K_STEPS).all() and (got['steps_done'][left] < K_STEPS).all()
    for i in np.flatnonzero(left):
        done = got['steps_done'][i]
        assert np.isfinite(got['positions'][:done + 1, i]).all() and np.isnan(got['positions'][done + 1:, i]).all()
        assert np.isfinite(got['fields'][:done + 1, i]).all() and np.isnan(got['fields'][done + 1:, i]).all()
    assert got['hours'].tolist() == [kw['hours'] + k * (1.0 if direction == 'forward' else -1.0) for k in range(K_STEPS + 1)]
    assert np.abs(got['positions'][K_STEPS, :160] - got['positions'][0, :160]).max() > 0.05             # the wind does carry them


def test_fields_rows_are_predict_points_at_the_returned_positions():
    """with_fields: row k of the parcels alive there equals predict_points at positions[k], hours[k] bit for bit (parcels that have left stand in with
    their start point, so that every parcel keeps its place in the forward's tiles)."""
    W = _world()
    got = _run(W, 'forward')
    x0, y0 = _starts()
    for k in (0, 3, K_STEPS):
        alive = np.isfinite(got['positions'][k, :, 0])
        px, py = np.where(alive, got['positions'][k, :, 0], x0), np.where(alive, got['positions'][k, :, 1], y0)
        rows = W['m'].predict_points(W['field'], W['s'], px, py, np.full(N_PARCELS, got['hours'][k]), W['fh']).cpu().numpy()
        assert alive.sum() > 160 and _same(got['fields'][k][alive], rows[alive]), k


def test_parcel_chunks_and_methods():
    """A run forced into parcel chunks of 128 (128 + 72 parcels) equals the unchunked one bit for bit; without with_fields the same positions and no
    fields; Euler and midpoint run and differ from RK4."""
    W = _world()
    whole = _run(W, 'forward')
    chunked = _run(W, 'chunked', chunk_points=128)
    for key in whole:
        assert _same(chunked[key], whole[key]), key
    plain = _run(W, 'plain', with_fields=False)
    assert 'fields' not in plain and _same(plain['positions'], whole['positions']) and _same(plain['status'], whole['status'])
    for method in ('euler', 'midpoint'):
        other = _run(W, method, method=method, with_fields=False)
        both = np.isfinite(other['positions'][-1, :, 0]) & np.isfinite(whole['positions'][-1, :, 0])
        assert both.sum() > 160 and np.abs(other['positions'][-1][both] - whole['positions'][-1][both]).max() > 0, method
    # Euler's first step is the start point plus h times the wind recorded there: the stage's arithmetic on row 0 of the RK4 run's fields
    euler, (x0, y0) = W['euler'], _starts()
    kx, ky = (whole['fields'][0][:, 0].astype(np.float64) * 3600.0) / 27000.0, (whole['fields'][0][:, 1].astype(np.float64) * 3600.0) / 27000.0
    step1 = np.stack([x0 + (1.0 * 1.0) * (0.0 + 1.0 * kx), y0 + (1.0 * 1.0) * (0.0 + 1.0 * ky)], axis=1)
    ok = np.isfinite(euler['positions'][1, :, 0])
    assert ok.sum() > 160 and _same(euler['positions'][1][ok], step1[ok])
    m, x, y = W['m'], *_starts()
    with pytest.raises(ValueError, match='predict_points'):
        m.trajectories(W['field'], W['s'], x, y, np.full(N_PARCELS, 2.0), W['fh'], 8.0, 1.0)
    with pytest.raises(IndexError):
        m.trajectories(W['field'], W['s'], x + 100.0, y, 2.0, W['fh'], 8.0, 1.0)
    with pytest.raises(ValueError):
        m.trajectories(W['field'], W['s'], x, y, 2.0, W['fh'], 8.0, 0.0)
    with pytest.raises(ValueError):
        m.trajectories(W['field'], W['s'], x, y, 2.0, W['fh'], 8.0, 1.0, method='rk5')


def test_lonlat_round_trips():
    """Starts given in degrees that are exact in index units: the same integration; the returned degrees go back through lonlat_to_index to the index
    positions (two roundings each way: 1e-10 of a cell)."""
    W = _world()
    s = W['s']
    xi, yi = np.array([100.0, 30.125, 200.5, 230.875]), np.array([70.0, 100.25, 20.5, 10.0])
    lon, lat = s.cfg.begin_lon + xi * s.cfg.out_res_deg, s.cfg.begin_lat + yi * s.cfg.out_res_deg
    assert np.array_equal(s.lonlat_to_index(lon, lat)[0], xi) and np.array_equal(s.lonlat_to_index(lon, lat)[1], yi)
    a = W['m'].trajectories(W['field'], s, xi, yi, 12.0, W['fh'], -4.0, 0.5, 'midpoint')
    b = W['m'].trajectories(W['field'], s, lon, lat, 12.0, W['fh'], -4.0, 0.5, 'midpoint', lonlat=True)
    assert torch.equal(a['status'], b['status']) and torch.equal(a['steps_done'], b['steps_done']) and torch.equal(a['hours'], b['hours'])
    deg = b['positions'].cpu().numpy()
    bx, by = s.lonlat_to_index(deg[..., 0], deg[..., 1])
    idx = a['positions'].cpu().numpy()
    assert a['positions'].shape == (9, 4, 2) and np.isfinite(idx).all()
    assert np.abs(bx - idx[..., 0]).max() <= 1e-10 and np.abs(by - idx[..., 1]).max() <= 1e-10
    assert np.array_equal(deg[0, :, 0], lon) and np.array_equal(deg[0, :, 1], lat)


# ------------------------------------------------------------------------------------------------ 4. the launcher
def test_infer_launcher_writes_the_trajectories(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(4)
    m = builder_models(**ncep_config())
    (tmp_path / 'ckpt').mkdir()
    m.save_model(str(tmp_path / 'ckpt'), epoch=0, global_step=1, prefix='physics')
    cfg = tmp_path / 'cfg.py'
    cfg.write_text("from deepphysinet_amd.configs import ncep_config\nconfig = ncep_config()\nconfig['inference_cfg'].update(img_size=(145, 257), dt=21600)\n"
                   "config['inference_cfg']['log'].update(write_source=True, export_variable=['T'])\n")
    out = tmp_path / 'out'
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--config_file', str(cfg), '--checkpoint_path', str(tmp_path / 'ckpt'),
                            '--log_path', str(out), '--synthetic', '--trajectories', '100.5,30.25;110,35;72.01,18.01', '--traj_start', '24',
                            '--traj_hours', '-2', '--traj_step', '0.25'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert 'trajectories: positions (9, 3, 2)' in child.stdout
    files = {fn.split('_traj_')[1]: np.load(os.path.join(out, fn)) for fn in os.listdir(out) if '_traj_' in fn}
    assert sorted(files) == ['fields.npy', 'hours.npy', 'positions.npy', 'status.npy', 'steps.npy']
    assert files['positions.npy'].shape == (9, 3, 2) and files['positions.npy'].dtype == np.float64 and files['fields.npy'].shape == (9, 3, 6)
    assert files['hours.npy'].tolist() == [24.0 - 0.25 * k for k in range(9)]
    assert files['status.npy'].shape == (3,) and files['steps.npy'].shape == (3,) and files['steps.npy'][0] == 8
    assert np.allclose(files['positions.npy'][0], [[100.5, 30.25], [110.0, 35.0], [72.01, 18.01]], rtol=0, atol=1e-12)
    assert np.isfinite(files['positions.npy'][:, :2]).all() and np.isfinite(files['fields.npy'][:, :2]).all()
    assert len([fn for fn in os.listdir(out) if fn.endswith('_T.npy')]) == 5
