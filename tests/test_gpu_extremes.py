"""GPU (MI355X): window extremes and means in time -- dpn_extreme_scan / _begin / _refine against their numpy restatement, fed with the device forwards'
own out_n / jac_n; the sampler outputs they write against dpn_sample_at; their refusals; InterfacePhysics.extremes_at / extreme_lattice against the
same loop composed from sampler.sample_at, the PackedField forwards and the restatement; chunks, maps, degrees; the scan nodes and the mean against
predict_points; the one-minute dense route; the inference loop's key and infer.py --extremes.

Yardsticks: deepphysinet_amd.extremes (bit for bit: the kernels are compiled without contraction), dpn_sample_at at the same fp64 positions and hours
(bit for bit: the same device function), predict_points (exactly, for the scan nodes), and for the dense route the bar of tests/test_gpu_parity.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deepphysinet_amd import extremes as X
from tests import extremes_cases as EC
from tests.test_gpu_parity import TOL, _dev
from tests.test_gpu_trajectory import _world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7
ALL_COLUMNS = ['%s:%s' % (p, s) for p in X.PRODUCTS for s in X.SENSES]            # 7 products x 3 senses = 21 columns
STATE_KEYS = ('best_v', 'best_t', 'best_k', 'acc', 'status', 'lo', 'hi')
_runs = {}


def _points(n, outside=True):
    """n points inside the fine grid; with `outside`, every 16th (and the first) lies beyond the coarse cube's east side, where the sampler gives NaN."""
    g = np.random.default_rng(11 + n)
    x, y = 2.0 + g.random(n) * 252.0, 2.0 + g.random(n) * 140.0
    if outside:
        x[::16] = 261.0 + g.random(x[::16].size) * 20.0
    return x, y


def _composed(W, xs, ys, req, with_clip):
    """The route a user could compose before, checked step by step against the device: per scan node dpn_sample_at at the node's hour, the
    fields-only forward of PackedField and the scan on the host (scan_reference); the scan's close (begin_reference); per round dpn_sample_at at the
    probes' hours, the forward with the Jacobian and the round on the host (refine_reference).  The kernels run beside it on the same out_n / jac_n:
    after every launch the device state equals the restatement's bit for bit, and the inputs the kernels wrote for the next forward equal
    dpn_sample_at's.  -> the final state (numpy, [C, n])."""
    from deepphysinet_amd import point_path as PP
    m, s, dev = W['m'], W['s'], _dev()
    n, C = xs.size, len(req.ids)
    cols = X.refined_columns(req.senses)
    pf = m._inference_weights(W['field'], W['fh'], n * max(len(cols), 1))
    ph = pf._clip_physics(with_clip)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    st = PP.ExtremeState(s, xd, yd, req)
    ref = X.new_state(C, n, fill=FILL)                         # both sides start from the same fill: what a launch must not touch is compared too
    for key in STATE_KEYS:
        getattr(st, key).fill_(FILL)

    def same_state(where):
        for key in STATE_KEYS:
            assert EC.bitwise(getattr(st, key).cpu().numpy(), ref[key]), (where, key)

    def same_inputs(bufs, px, py, hours, where):
        want = s.sample_at(hours.size, torch.from_numpy(px).to(dev), torch.from_numpy(py).to(dev), torch.from_numpy(hours).to(dev))
        for got, w, what in zip(bufs, want, ('x', 'y', 't', 'f', 'coord_data')):
            assert EC.bitwise(got.cpu().numpy(), w.cpu().numpy()), (where, what)

    for k in range(req.K + 1):
        same_inputs(st.points, xs, ys, np.full(n, X.node_hour(req.t0, req.dt, k)), 'node %d' % k)
        x, y, t, _, cd = st.points
        out_n, _ = PP._forward_points(pf.cfg, pf.ws, pf.nets, x, y, t, None, cd, want_jac=False, want_saved=False)
        st.scan(s, ph, with_clip, out_n, k)
        xv, _ = X.products_reference(out_n.cpu().numpy(), None, ph, with_clip, req.ids, n)
        ref = X.scan_reference(xv, ref, req.senses, k, req.K)
        same_state('scan %d' % k)
    st.begin(s)
    ref, hours = X.begin_reference(ref, req.senses, req.K, req.t0, req.dt)
    same_state('begin')
    if cols:
        px, py = np.tile(xs, len(cols)), np.tile(ys, len(cols))
        ids_r = [req.ids[c] for c in cols]
        for rnd in range(req.R + 1):
            same_inputs(st.probes, px, py, hours.reshape(-1), 'round %d' % rnd)
            x, y, t, _, cd = st.probes
            out_n, jac_n = PP._forward_points(pf.cfg, pf.ws, pf.nets, x, y, t, None, cd, want_jac=True, want_saved=False)
            st.refine(s, ph, with_clip, out_n, jac_n, rnd)
            g, sl = X.products_reference(out_n.cpu().numpy(), jac_n.cpu().numpy(), ph, with_clip, ids_r, n)
            ref, (nxt, moved) = X.refine_reference(g, sl, ref, req.senses, rnd, req.t0, req.dt)
            hours = np.where(moved, nxt, hours)
            same_state('round %d' % rnd)
        same_inputs(st.probes, px, py, hours.reshape(-1), 'after the last round')
    return ref


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n, columns, K, R, clip', [(1, ['T:max'], 1, 0, False), (1, ['speed:min'], 3, 4, True), (255, ALL_COLUMNS, 3, 1, True),
                                                    (257, ALL_COLUMNS, 3, 4, False), (257, ['q:mean'], 1, 1, True), (257, ['rho:min'], 1, 0, False)])
def test_kernels_are_the_restatement_bit_for_bit(n, columns, K, R, clip):
    """One block and less, two blocks and a point (n = 1, 255, 257), one column and all 21, K = 1 and 3, R = 0, 1 and 4, without and with the clip,
    points beyond the coarse cube among them: after every launch best_v, best_t, best_k, acc, status, lo and hi equal the restatement bit for bit
    (both start from the same fill, so what a launch must not touch is compared too), and x, y, t, f, coord_data the kernels wrote equal dpn_sample_at
    at the same positions and hours bit for bit (_composed asserts both).  The points outside end with BAD_SCAN and NaN, the others do not."""
    W = _world()
    xs, ys = _points(n, outside=n > 1)
    req = X.check_request(columns, (5.0, 5.0 + 1.5 * K), 1.5, R, 24)
    ref = _composed(W, xs, ys, req, clip)
    outside = xs > 256.0
    assert (ref['status'][:, outside] == X.BAD_SCAN).all() and (ref['status'][:, ~outside] != X.BAD_SCAN).all()
    assert np.isnan(ref['best_v'][:, outside]).all() and np.isfinite(ref['best_v'][:, ~outside]).all()
    if n > 1:
        assert outside.sum() >= 16
        print('n = %d, C = %d, K = %d, R = %d: statuses %s' % (n, len(columns), K, R, np.unique(ref['status'], return_counts=True)))


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as PP
    W = _world()
    s, dev, n = W['s'], _dev(), 257
    xs, ys = _points(n, outside=False)
    req = X.check_request(['T:max', 'T:mean', 'speed:min'], (0.0, 3.0), 1.0, 2, 24)
    st = PP.ExtremeState(s, torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev), req)
    for key in STATE_KEYS:
        getattr(st, key).fill_(FILL)
    for buf in st.points + st.probes:
        buf.fill_(FILL)
    out_n, jac_n = torch.zeros((2 * n, 6), device=dev), torch.zeros((2 * n, 6, 3), device=dev)
    ph = PP.PointConfig().physics()
    lib, by, ptr, stream = L.load(), ctypes.byref, PP._ptr, PP._stream()
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    nan, inf = float('nan'), float('inf')

    def call(which, **over):
        a = dict(s=by(s._s), cube=ptr(s.cube), phys=by(ph), with_clip=0, out_n=ptr(out_n), jac_n=ptr(jac_n), n=n, products=st.c_ids, senses=st.c_senses,
                 C=3, k=1, round=0, K=3, t0=0.0, dt=1.0, xr=ptr(st.xr), yr=ptr(st.yr), st=by(st.c_struct()))
        a.update(dict(zip(('x', 'y', 't', 'f', 'coord_data'), (ptr(v) for v in (st.points if which == 'scan' else st.probes)))))
        a.update(over)
        order = {'scan': 's cube phys with_clip out_n n products senses C k K t0 dt xr yr st x y t f coord_data',
                 'begin': 's cube n products senses C K t0 dt xr yr st x y t f coord_data',
                 'refine': 's cube phys with_clip out_n jac_n n products senses C round K t0 dt xr yr st x y t f coord_data'}[which]
        return getattr(lib, 'dpn_extreme_' + which)(*[a[key] for key in order.split()], stream)

    def hollow(field):
        c = st.c_struct()
        setattr(c, field, None)
        return dict(st=by(c))
    bad_sampler = L.DpnSampler.from_buffer_copy(s._s)
    bad_sampler.t_in = 1
    shared = [{key: None} for key in ('s', 'cube', 'products', 'senses', 'xr', 'yr', 'st', 'x', 'y', 't', 'f', 'coord_data')] + [hollow(f) for f in STATE_KEYS]
    shared += [dict(n=0), dict(n=-5), dict(K=0), dict(K=-1), dict(t0=nan), dict(t0=inf), dict(dt=nan), dict(dt=inf), dict(dt=0.0), dict(dt=-1.0), dict(C=0),
               dict(C=33), dict(products=i32([31, 27, 25])), dict(products=i32([31, 34, 25])), dict(products=i32([0, 31, 25])), dict(senses=i32([0, 3, 1])),
               dict(senses=i32([-1, 2, 1])), dict(s=by(bad_sampler))]
    cases = {'scan': shared + [dict(phys=None), dict(out_n=None), dict(k=-1), dict(k=4)], 'begin': shared,
             'refine': shared + [dict(phys=None), dict(out_n=None), dict(jac_n=None), dict(round=-1), dict(senses=i32([2, 2, 2]))]}
    for which, overs in cases.items():
        for over in overs:
            assert call(which, **over) == -1, (which, sorted(over))
    torch.cuda.synchronize()
    assert all(bool((getattr(st, key) == FILL).all()) for key in STATE_KEYS) and all(bool((b == FILL).all()) for b in st.points + st.probes)
    assert call('scan', k=0) == 0 and call('scan') == 0 and call('scan', k=3) == 0 and call('begin') == 0 and call('refine') == 0      # the same arguments, accepted
    torch.cuda.synchronize()
    assert not bool((st.status == FILL).any()) and not bool((st.best_v == FILL).any()) and not bool((st.lo == FILL).any())


# ------------------------------------------------------------------------------------------------ 3. end to end
N_STATIONS, WINDOW, SCAN, ROUNDS = 257, (3.0, 9.0), 2.0, 4
LATTICE = dict(x_range=(40.0, 56.0), y_range=(30.0, 45.0))              # 17 x 16 = 272 positions


def _run(W, key, **kw):
    if key not in _runs:
        x, y = _points(N_STATIONS, outside=False)
        args = dict(x_idx=x, y_idx=y, window=WINDOW, columns=ALL_COLUMNS, scan_hours=SCAN, refine=ROUNDS)
        args.update(kw)
        r = W['m'].extremes_at(W['field'], W['s'], args.pop('x_idx'), args.pop('y_idx'), args.pop('window'), W['fh'], args.pop('columns'), **args)
        _runs[key] = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
    return _runs[key]


@pytest.mark.parametrize('clip', [False, True])
def test_extremes_at_equals_the_composed_route_bit_for_bit(clip):
    """257 stations, all 21 columns, hours 3..9 in steps of 2, four rounds: value, hour, lo, hi and status equal the composed route's bit for bit,
    without and with the clip."""
    W = _world()
    got = _run(W, 'clip%d' % clip, with_clip=clip)
    x, y = _points(N_STATIONS, outside=False)
    want = X.results_of(_composed(W, x, y, X.check_request(ALL_COLUMNS, WINDOW, SCAN, ROUNDS, 24), clip), ALL_COLUMNS)
    assert got['names'] == ALL_COLUMNS and got['value'].shape == (N_STATIONS, 21) and got['status'].dtype == np.int32
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert EC.bitwise(got[key], want[key]), key
    mean = np.array([n.endswith(':mean') for n in ALL_COLUMNS])
    assert np.isnan(got['hour'][:, mean]).all() and np.isfinite(got['hour'][:, ~mean]).all() and np.isfinite(got['value']).all()
    assert (got['lo'][:, ~mean] <= got['hi'][:, ~mean]).all() and (got['lo'][:, ~mean] >= WINDOW[0]).all() and (got['hi'][:, ~mean] <= WINDOW[1]).all()
    print('clip %d: statuses %s' % (clip, dict(zip(*np.unique(got['status'], return_counts=True)))))


def test_chunks_maps_and_degrees():
    """A run forced into chunks of 128 stations (128 + 128 + 1) equals the unchunked one bit for bit; extreme_lattice's maps [C, ny, nx] are
    extremes_at at the lattice's positions, chunked (128 + 128 + 16) or not; stations given in degrees that are exact in index units give the same
    result as in index units; a lattice with nt != 1 and positions outside the grid are refused."""
    W = _world()
    m, s = W['m'], W['s']
    whole, chunked = _run(W, 'clip0', with_clip=False), _run(W, 'chunked', chunk_points=128)
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert EC.bitwise(chunked[key], whole[key]), key
    cols = ['T:max', 'speed:max', 'p:mean', 'q:min']
    lattice = s.lattice(refine=1, hours=0.0, **LATTICE)
    assert (lattice.nx, lattice.ny, lattice.nt) == (17, 16, 1)
    maps = m.extreme_lattice(W['field'], s, lattice, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    maps_c = m.extreme_lattice(W['field'], s, lattice, WINDOW, W['fh'], cols, SCAN, ROUNDS, chunk_points=128)
    px, py, _ = lattice.positions()
    rows = m.extremes_at(W['field'], s, px, py, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    assert maps['names'] == rows['names'] == ['T:max', 'speed:max', 'p:mean', 'q:min']
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert tuple(maps[key].shape) == (4, 16, 17)
        assert EC.bitwise(maps[key].reshape(4, -1).t().contiguous().cpu().numpy(), rows[key].cpu().numpy()), key
        assert EC.bitwise(maps_c[key].cpu().numpy(), maps[key].cpu().numpy()), key
    xi, yi = np.array([100.0, 30.125, 200.5, 230.875]), np.array([70.0, 100.25, 20.5, 10.0])
    lon, lat = s.cfg.begin_lon + xi * s.cfg.out_res_deg, s.cfg.begin_lat + yi * s.cfg.out_res_deg
    a = m.extremes_at(W['field'], s, xi, yi, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    b = m.extremes_at(W['field'], s, lon, lat, WINDOW, W['fh'], cols, SCAN, ROUNDS, lonlat=True)
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert EC.bitwise(a[key].cpu().numpy(), b[key].cpu().numpy()), key
    with pytest.raises(ValueError, match='nt == 1'):
        m.extreme_lattice(W['field'], s, s.lattice(hours=(0.0, 1.0, 2), **LATTICE), WINDOW, W['fh'], cols)
    with pytest.raises(IndexError):
        m.extremes_at(W['field'], s, xi + 100.0, yi, WINDOW, W['fh'], cols)
    with pytest.raises(ValueError):
        m.extremes_at(W['field'], s, xi, yi, (3.0, 25.0), W['fh'], cols)
    with pytest.raises(KeyError):
        m.extremes_at(W['field'], s, xi, yi, WINDOW, W['fh'], ['gust:max'])


@pytest.mark.parametrize('clip', [False, True])
def test_scan_nodes_bound_the_extremes_and_the_mean_is_their_trapezoid(clip):
    """For every column, the value is >= (max) or <= (min) predict_points' value at every scan node, exactly; a mean equals the fp64 trapezoid of
    those rows over the window to one float32 rounding of the result."""
    W = _world()
    got = _run(W, 'clip%d' % clip, with_clip=clip)
    x, y = _points(N_STATIONS, outside=False)
    K = int(round((WINDOW[1] - WINDOW[0]) / SCAN))
    nodes = np.stack([W['m'].predict_points(W['field'], W['s'], x, y, np.full(N_STATIONS, WINDOW[0] + k * SCAN), W['fh'], with_clip=clip).cpu().numpy()
                      for k in range(K + 1)])                                                 # [K + 1, N, 6]
    speed = np.sqrt(nodes[..., 0] * nodes[..., 0] + nodes[..., 1] * nodes[..., 1])
    series = {name: nodes[..., k] for k, name in enumerate(X.PRODUCTS[:6])}
    series['speed'] = speed
    trapz = getattr(np, 'trapezoid', None) or np.trapz
    for c, name in enumerate(ALL_COLUMNS):
        product, sense = name.split(':')
        v = series[product]
        if sense == 'max':
            assert (got['value'][:, c] >= v.max(axis=0)).all(), name
        elif sense == 'min':
            assert (got['value'][:, c] <= v.min(axis=0)).all(), name
        else:
            want = trapz(v.astype(np.float64), dx=SCAN, axis=0) / (WINDOW[1] - WINDOW[0])
            err = np.abs(got['value'][:, c].astype(np.float64) - want)
            assert (err <= np.spacing(np.abs(want).astype(np.float32))).all(), (name, err.max())
    better = sum(int((got['value'][:, c] != (series[n.split(':')[0]].max(axis=0) if n.endswith('max') else series[n.split(':')[0]].min(axis=0))).sum())
                 for c, n in enumerate(ALL_COLUMNS) if not n.endswith('mean'))
    print('clip %d: %d of %d (station, column) extremes were improved by the refinement' % (clip, better, N_STATIONS * 14))
    assert better > 0


# ------------------------------------------------------------------------------------------------ 4. against the dense route
def test_refined_extremes_against_the_one_minute_dense_route():
    """Seed extremes_cases.DENSE_SEED (SyntheticSamples' default, the world of these tests) and the 8 stations DENSE_STATIONS, 24 h, T:max, T:min,
    speed:max, hourly scan, R = 10, against predict_points on the one-minute lattice of the same window plus a max / min: the stations are those at
    which the fp64 oracle of the network meets the condition (tests/test_extremes_cpu.py::test_dense_route_condition_holds_on_the_fp64_oracle).
    The refined value may fall short of the dense extreme by at most twice the bar tests/test_gpu_parity.py grants one value against the fp64 oracle:
    line 86 there holds the normalised fields to TOL['bf16x2']['field'] = 5e-5 (line 22) of the largest normalised field, which de-normalises to
    5e-5 * max |out_n| * std[k] for variable k; both sides here are GPU forwards and each carries one such error.  The speed's bar is the sum of u's
    and v's (|d sqrt(u^2 + v^2)| <= |du| + |dv|).  max |out_n| is taken over the dense rows."""
    W = _world()
    m, s = W['m'], W['s']
    assert EC.DENSE_SEED == 0                                             # SyntheticSamples' default seed: _world()'s cube and field sample
    xs, ys = (np.array([p[j] for p in EC.DENSE_STATIONS]) for j in (0, 1))
    n = xs.size
    got = m.extremes_at(W['field'], s, xs, ys, (0.0, 24.0), W['fh'], list(EC.DENSE_COLUMNS), 1.0, 10)
    minutes = np.arange(1441) / 60.0
    dense = m.predict_points(W['field'], s, np.tile(xs, minutes.size), np.tile(ys, minutes.size), np.repeat(minutes, n), W['fh']).cpu().numpy()
    dense = dense.reshape(minutes.size, n, 6)
    ph = m.point_config().physics()
    mean, std = np.array(ph.mean[:], dtype=np.float64), np.array(ph.std[:], dtype=np.float64)
    assert not any(ph.sq_on[:])
    top = np.abs((dense.astype(np.float64) - mean) / std).max()
    bar = 2.0 * TOL['bf16x2']['field'] * top * std
    bars = np.array([bar[3], bar[3], bar[0] + bar[1]])
    want = np.stack(EC.dense_extremes(dense), axis=1).astype(np.float64)
    value = got['value'].cpu().numpy().astype(np.float64)
    shortfall = (want - value) * np.array([1.0, -1.0, 1.0])              # > 0: the refined value is worse than the dense one
    print('dense route: largest normalised field %.3f, bars %s, shortfall per column %s, gain per column %s; hours %s; status %s'
          % (top, bars.tolist(), shortfall.max(axis=0).tolist(), (-shortfall).max(axis=0).tolist(), got['hour'].cpu().numpy().tolist(),
             got['status'].cpu().numpy().tolist()))
    assert np.isfinite(value).all() and (shortfall <= bars).all(), (shortfall.max(axis=0), bars)


# ------------------------------------------------------------------------------------------------ 5. the inference loop and the launcher
def test_run_inference_interface_takes_the_extremes_key(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg'].update(img_size=(145, 257), dt=21600)
    cfg['inference_cfg']['log'].update(write_source=True, result_path=str(tmp_path / 'out'), export_variable=['T'])
    cfg['inference_cfg']['extremes'] = dict(columns=['T:max', 'speed:mean'], window=(6.0, 12.0), scan_hours=2.0, refine=2,
                                            lonlat=[(100.5, 30.25), (110.0, 35.0), (72.5, 18.25)])
    torch.manual_seed(4)
    m = builder_models(**cfg)
    (tmp_path / 'ckpt').mkdir()
    m.save_model(str(tmp_path / 'ckpt'), epoch=0, global_step=1, prefix='physics')
    maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', device='cuda:0')
    e = m.last_extremes
    assert maps is not None and e['names'] == ['T:max', 'speed:mean'] and tuple(e['value'].shape) == (3, 2) and e['hour'].dtype == torch.float64
    files = {fn.split('_extreme_')[1]: np.load(os.path.join(tmp_path / 'out', fn)) for fn in os.listdir(tmp_path / 'out') if '_extreme_' in fn}
    assert sorted(files) == ['hi.npy', 'hour.npy', 'lo.npy', 'status.npy', 'value.npy']
    for key in ('value', 'hour', 'lo', 'hi', 'status'):
        assert EC.bitwise(files[key + '.npy'], e[key].cpu().numpy()), key
    assert np.isfinite(files['value.npy']).all() and np.isnan(files['hour.npy'][:, 1]).all() and (6.0 <= files['hour.npy'][:, 0]).all()


def test_infer_launcher_writes_the_extreme_maps(tmp_path):
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
                            '--log_path', str(out), '--synthetic', '--extremes', 'T:max,T:min,speed:max', '--extreme_window', '0,24', '--extreme_scan', '6',
                            '--extreme_refine', '3'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert 'extremes T:max,T:min,speed:max: value (3, 145, 257)' in child.stdout
    names = sorted(fn.split('_extreme_')[1] for fn in os.listdir(out) if '_extreme_' in fn)
    assert names == sorted('%s_%s.npy' % (k, c) for k in ('value', 'hour', 'lo', 'hi', 'status') for c in ('T_max', 'T_min', 'speed_max'))
    files = {fn.split('_extreme_')[1]: np.load(os.path.join(out, fn)) for fn in os.listdir(out) if '_extreme_' in fn}
    assert all(a.shape == (145, 257) for a in files.values()) and files['hour_T_max.npy'].dtype == np.float64 and files['status_T_min.npy'].dtype == np.int32
    assert np.isfinite(files['value_T_max.npy']).all() and (files['value_T_max.npy'] >= files['value_T_min.npy']).all()
    assert (files['hour_speed_max.npy'] >= 0.0).all() and (files['hour_speed_max.npy'] <= 24.0).all()
    assert len([fn for fn in os.listdir(out) if fn.endswith('_T.npy')]) == 5
