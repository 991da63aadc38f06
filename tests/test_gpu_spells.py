"""GPU (MI355X): threshold spells in time -- dpn_spell_scan / _begin / _refine / _finish against their numpy restatement, fed with the device forwards'
own out_n; the sampler outputs they write against dpn_sample_at; their refusals; InterfacePhysics.spells_at / spell_lattice against the same loop
composed from sampler.sample_at, the PackedField forward and the restatement; chunks, maps, degrees, points outside the cube; the one-minute dense
route; the inference loop's key and infer.py --spells.

Yardsticks: deepphysinet_amd.spells (bit for bit: the kernels are compiled without contraction), dpn_sample_at at the same fp64 positions and hours
(bit for bit: the same device function), and for the dense route predict_points at one-minute steps, counted on the host (spells_cases.dense_spells),
under the bars spells_cases.check_against_dense derives."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deepphysinet_amd import spells as S
from tests import extremes_cases as EC
from tests import spells_cases as SC
from tests.test_gpu_parity import _dev
from tests.test_gpu_trajectory import _world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7
# 16 columns: every product on both sides of a threshold near the middle of what the seeded network gives, two repeats, one threshold rarely reached
COLUMNS16 = ['T:above:221', 'T:below:221', 'speed:above:10', 'speed:below:10', 'u:above:-5', 'u:below:-5', 'v:above:-7.6', 'v:below:-7.6',
             'p:above:113767', 'p:below:113767', 'q:above:0.034', 'q:below:0.034', 'rho:above:1.33', 'rho:below:1.33', 'T:above:221', 'T:above:285']
RESULT_KEYS = ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess', 'crossings', 'status')
_runs = {}


def _points(n, outside=True):
    """n points inside the fine grid; with `outside`, every 16th (and the first) lies beyond the coarse cube's east side, where the sampler gives NaN."""
    g = np.random.default_rng(23 + n)
    x, y = 2.0 + g.random(n) * 252.0, 2.0 + g.random(n) * 140.0
    if outside:
        x[::16] = 261.0 + g.random(x[::16].size) * 20.0
    return x, y


def _composed(W, xs, ys, req, with_clip):
    """The route a user could compose before, checked step by step against the device: per scan node dpn_sample_at at the node's hour, the
    fields-only forward of PackedField and the scan on the host (scan_reference); the scan's close (begin_reference); per round dpn_sample_at at the
    probes' hours, the same forward and the round on the host (refine_reference); finish_reference.  The kernels run beside it on the same out_n:
    after every launch the device state equals the restatement's bit for bit, and the inputs the kernels wrote for the next forward equal
    dpn_sample_at's.  -> the final state (numpy, [C, n])."""
    from deepphysinet_amd import point_path as PP
    m, s, dev = W['m'], W['s'], _dev()
    n, C = xs.size, len(req.ids)
    pf = m._inference_weights(W['field'], W['fh'], n * 2 * C)
    ph = pf._clip_physics(with_clip)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    st = PP.SpellState(s, xd, yd, req)
    ref = S.new_state(C, n, fill=FILL)                         # both sides start from the same fill: what a launch must not touch is compared too
    for key in S.STATE_KEYS:
        getattr(st, key).fill_(FILL)

    def same_state(where):
        for key in S.STATE_KEYS:
            assert EC.bitwise(getattr(st, key).cpu().numpy(), ref[key]), (where, key)

    def same_inputs(bufs, px, py, hours, where):
        want = s.sample_at(hours.size, torch.from_numpy(px).to(dev), torch.from_numpy(py).to(dev), torch.from_numpy(hours).to(dev))
        for got, w, what in zip(bufs, want, ('x', 'y', 't', 'f', 'coord_data')):
            assert EC.bitwise(got.cpu().numpy(), w.cpu().numpy()), (where, what)

    def forward(bufs):
        x, y, t, _, cd = bufs
        return PP._forward_points(pf.cfg, pf.ws, pf.nets, x, y, t, None, cd, want_jac=False, want_saved=False)[0]

    for k in range(req.K + 1):
        same_inputs(st.points, xs, ys, np.full(n, S.node_hour(req.t0, req.dt, k)), 'node %d' % k)
        out_n = forward(st.points)
        st.scan(s, ph, with_clip, out_n, k)
        ref = S.scan_reference(S.products_reference(out_n.cpu().numpy(), ph, with_clip, req.ids, n), ref, req.sides, req.thr, k, req.dt)
        same_state('scan %d' % k)
    st.begin(s)
    ref, hours = S.begin_reference(ref, req.K, req.t0, req.dt)
    same_state('begin')
    has_entry, has_exit = S.brackets_of(ref, req.K)
    unbracketed = ~np.stack([has_entry, has_exit], axis=1).reshape(2 * C, n)
    assert (hours[unbracketed] == req.t0).all()                # probes without a bracket sit at t0
    px, py = np.tile(xs, 2 * C), np.tile(ys, 2 * C)
    ids2 = [i for i in req.ids for _ in range(2)]
    for rnd in range(req.R):
        same_inputs(st.probes, px, py, hours.reshape(-1), 'round %d' % rnd)
        out_n = forward(st.probes)
        st.refine(s, ph, with_clip, out_n, None, rnd)
        ref, (nxt, moved) = S.refine_reference(S.products_reference(out_n.cpu().numpy(), ph, with_clip, ids2, n), ref, req.sides, req.thr, req.K)
        assert not moved[unbracketed].any()
        hours = np.where(moved, nxt, hours)
        same_state('round %d' % rnd)
    same_inputs(st.probes, px, py, hours.reshape(-1), 'after the last round')
    st.finish()
    ref = S.finish_reference(ref, req.K, req.t0, req.dt)
    same_state('finish')
    return ref


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n, columns, K, R, clip', [(1, ['T:below:221'], 1, 0, False), (1, COLUMNS16, 24, 3, True), (255, COLUMNS16, 1, 3, False),
                                                    (257, COLUMNS16, 24, 3, False), (257, ['speed:above:10'], 24, 0, True),
                                                    (255, ['q:below:0.034'], 1, 0, True)])
def test_kernels_are_the_restatement_bit_for_bit(n, columns, K, R, clip):
    """One block and less, two blocks and a point (n = 1, 255, 257), one column and 16 (repeated products, both sides), K = 1 and 24, R = 0 and 3,
    without and with the clip, points beyond the coarse cube among them: after every launch the thirteen arrays of the state equal the restatement
    bit for bit (both start from the same fill, so what a launch must not touch is compared too), and x, y, t, f, coord_data the kernels wrote
    equal dpn_sample_at at the same positions and hours bit for bit, probes without a bracket at t0 (_composed asserts all of it).  The points
    outside end with BAD_SCAN and NaN, the others do not."""
    W = _world()
    xs, ys = _points(n, outside=n > 1)
    req = S.check_request(columns, (0.0, float(K)), 1.0, R, 24)
    assert (req.K, req.R) == (K, R)
    ref = _composed(W, xs, ys, req, clip)
    outside = xs > 256.0
    assert (ref['status'][:, outside] == S.BAD_SCAN).all() and not (ref['status'][:, ~outside] & (S.BAD_SCAN | S.STOPPED)).any()
    for key in ('hours', 'excess', 'f_lo', 'f_hi', 'l_lo', 'l_hi'):
        assert np.isnan(ref[key][:, outside]).all(), key
    inside = ref['status'][:, ~outside]
    hours = ref['hours'][:, ~outside]                          # sums of at most 28 terms of at most 24 h: their rounding stays far below 1e-12
    assert np.isfinite(hours).all() and (hours >= -1e-12).all() and (hours <= K + 1e-12).all()
    never = (inside & S.NEVER) != 0
    assert np.isnan(ref['f_hi'][:, ~outside][never]).all() and np.isfinite(ref['f_hi'][:, ~outside][~never]).all()
    if n > 1:
        assert outside.sum() >= 16
        print('n = %d, C = %d, K = %d, R = %d: statuses %s, crossings up to %d' % (n, len(columns), K, R, np.unique(ref['status'], return_counts=True),
                                                                                   ref['crossings'][:, ~outside].max()))
    if len(columns) == 16 and K == 24 and n > 1:               # the request exercises every branch
        assert {0, S.NEVER, S.HOLDS_AT_START, S.HOLDS_AT_END, S.HOLDS_AT_START | S.HOLDS_AT_END} <= set(np.unique(inside).tolist())
        assert ref['crossings'][:, ~outside].max() >= 3


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as PP
    W = _world()
    s, dev, n = W['s'], _dev(), 257
    xs, ys = _points(n, outside=False)
    req = S.check_request(['T:above:221', 'speed:below:10', 'q:above:0.034'], (0.0, 3.0), 1.0, 2, 24)
    st = PP.SpellState(s, torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev), req)
    for key in S.STATE_KEYS:
        getattr(st, key).fill_(FILL)
    for buf in st.points + st.probes:
        buf.fill_(FILL)
    out_n = torch.zeros((6 * n, 6), device=dev)
    ph = PP.PointConfig().physics()
    lib, by, ptr, stream = L.load(), ctypes.byref, PP._ptr, PP._stream()
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    f32 = lambda v: (ctypes.c_float * len(v))(*v)
    nan, inf = float('nan'), float('inf')

    def call(which, **over):
        a = dict(s=by(s._s), cube=ptr(s.cube), phys=by(ph), with_clip=0, out_n=ptr(out_n), n=n, products=st.c_ids, sides=st.c_sides, thr=st.c_thr, C=3,
                 k=1, round=0, K=3, t0=0.0, dt=1.0, xr=ptr(st.xr), yr=ptr(st.yr), st=by(st.c_struct()))
        a.update(dict(zip(('x', 'y', 't', 'f', 'coord_data'), (ptr(v) for v in (st.points if which == 'scan' else st.probes)))))
        a.update(over)
        order = {'scan': 's cube phys with_clip out_n n products sides thr C k K t0 dt xr yr st x y t f coord_data',
                 'begin': 's cube n products sides thr C K t0 dt xr yr st x y t f coord_data',
                 'refine': 's cube phys with_clip out_n n products sides thr C round K t0 dt xr yr st x y t f coord_data',
                 'finish': 'n C K t0 dt st'}[which]
        return getattr(lib, 'dpn_spell_' + which)(*[a[key] for key in order.split()], stream)

    def hollow(field):
        c = st.c_struct()
        setattr(c, field, None)
        return dict(st=by(c))
    bad_sampler = L.DpnSampler.from_buffer_copy(s._s)
    bad_sampler.t_in = 1
    clock = [dict(st=None)] + [hollow(f) for f in S.STATE_KEYS] + [dict(n=0), dict(n=-5), dict(K=0), dict(K=-1), dict(t0=nan), dict(t0=inf), dict(dt=nan),
                                                                   dict(dt=inf), dict(dt=0.0), dict(dt=-1.0), dict(C=0), dict(C=17)]
    shared = clock + [{key: None} for key in ('s', 'cube', 'products', 'sides', 'thr', 'xr', 'yr', 'x', 'y', 't', 'f', 'coord_data')]
    shared += [dict(products=i32([31, 27, 25])), dict(products=i32([31, 34, 25])), dict(products=i32([0, 31, 25])), dict(sides=i32([0, 2, 1])),
               dict(sides=i32([-1, 0, 1])), dict(thr=f32([221.0, nan, 0.5])), dict(thr=f32([221.0, 10.0, inf])), dict(thr=f32([-inf, 10.0, 0.5])),
               dict(s=by(bad_sampler))]
    cases = {'scan': shared + [dict(phys=None), dict(out_n=None), dict(k=-1), dict(k=4)], 'begin': shared,
             'refine': shared + [dict(phys=None), dict(out_n=None), dict(round=-1)], 'finish': clock}
    for which, overs in cases.items():
        for over in overs:
            assert call(which, **over) == -1, (which, sorted(over))
    torch.cuda.synchronize()
    assert all(bool((getattr(st, key) == FILL).all()) for key in S.STATE_KEYS) and all(bool((b == FILL).all()) for b in st.points + st.probes)
    for which, over in (('scan', dict(k=0)), ('scan', {}), ('scan', dict(k=2)), ('scan', dict(k=3)), ('begin', {}), ('refine', {}), ('finish', {})):
        assert call(which, **over) == 0, (which, over)                   # the same arguments, accepted
    torch.cuda.synchronize()
    assert not any(bool((getattr(st, key) == FILL).any()) for key in ('status', 'hours', 'k_first', 'crossings', 'prev_x'))


# ------------------------------------------------------------------------------------------------ 3. end to end
N_STATIONS, WINDOW, SCAN, ROUNDS = 257, (3.0, 15.0), 2.0, 4
LATTICE = dict(x_range=(40.0, 56.0), y_range=(30.0, 45.0))              # 17 x 16 = 272 positions


def _run(W, key, **kw):
    if key not in _runs:
        x, y = _points(N_STATIONS, outside=False)
        args = dict(x_idx=x, y_idx=y, window=WINDOW, columns=COLUMNS16, scan_hours=SCAN, refine=ROUNDS)
        args.update(kw)
        r = W['m'].spells_at(W['field'], W['s'], args.pop('x_idx'), args.pop('y_idx'), args.pop('window'), W['fh'], args.pop('columns'), **args)
        _runs[key] = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
    return _runs[key]


@pytest.mark.parametrize('clip', [False, True])
def test_spells_at_equals_the_composed_route_bit_for_bit(clip):
    """257 stations, 16 columns, hours 3..15 in steps of 2, four rounds: every result equals the composed route's bit for bit, without and with the
    clip; first and last lie inside the window, in that order, and hours never exceeds the span between them."""
    W = _world()
    got = _run(W, 'clip%d' % clip, with_clip=clip)
    x, y = _points(N_STATIONS, outside=False)
    want = S.results_of(_composed(W, x, y, S.check_request(COLUMNS16, WINDOW, SCAN, ROUNDS, 24), clip), COLUMNS16)
    assert got['names'] == COLUMNS16 and got['hours'].shape == (N_STATIONS, 16) and got['status'].dtype == np.int32 and got['hours'].dtype == np.float64
    for key in RESULT_KEYS:
        assert EC.bitwise(got[key], want[key]), key
    some = (got['status'] & S.NEVER) == 0
    assert not (got['status'] & (S.BAD_SCAN | S.STOPPED)).any() and some.any() and (~some).any()
    assert (got['first'][some] >= WINDOW[0]).all() and (got['last'][some] <= WINDOW[1]).all() and (got['first'][some] <= got['last'][some]).all()
    assert (got['hours'][some] <= (got['last'] - got['first'])[some] + 1e-12).all() and (got['hours'][~some] == 0.0).all() and np.isnan(got['first'][~some]).all()
    assert (got['excess'] >= 0.0).all()
    print('clip %d: statuses %s' % (clip, dict(zip(*np.unique(got['status'], return_counts=True)))))


def test_chunks_maps_degrees_and_points_outside_the_cube():
    """A run forced into chunks of 128 stations (128 + 128 + 1) equals the unchunked one bit for bit; spell_lattice's maps [C, ny, nx] are spells_at
    at the lattice's positions, chunked (128 + 128 + 16) or not; stations given in degrees that are exact in index units give the same result as in
    index units; a lattice that reaches beyond the coarse cube has BAD_SCAN and NaN there and nowhere else; a lattice with nt != 1, positions outside
    the grid, a window outside the sample's and a malformed column are refused."""
    from deepphysinet_amd.sampler import Lattice
    W = _world()
    m, s = W['m'], W['s']
    whole, chunked = _run(W, 'clip0', with_clip=False), _run(W, 'chunked', chunk_points=128)
    for key in RESULT_KEYS:
        assert EC.bitwise(chunked[key], whole[key]), key
    cols = ['T:above:221', 'speed:below:10', 'p:above:113767', 'q:below:0.034']
    lattice = s.lattice(refine=1, hours=0.0, **LATTICE)
    assert (lattice.nx, lattice.ny, lattice.nt) == (17, 16, 1)
    maps = m.spell_lattice(W['field'], s, lattice, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    maps_c = m.spell_lattice(W['field'], s, lattice, WINDOW, W['fh'], cols, SCAN, ROUNDS, chunk_points=128)
    px, py, _ = lattice.positions()
    rows = m.spells_at(W['field'], s, px, py, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    assert maps['names'] == rows['names'] == cols
    for key in RESULT_KEYS:
        assert tuple(maps[key].shape) == (4, 16, 17)
        assert EC.bitwise(maps[key].reshape(4, -1).t().contiguous().cpu().numpy(), rows[key].cpu().numpy()), key
        assert EC.bitwise(maps_c[key].cpu().numpy(), maps[key].cpu().numpy()), key
    xi, yi = np.array([100.0, 30.125, 200.5, 230.875]), np.array([70.0, 100.25, 20.5, 10.0])
    lon, lat = s.cfg.begin_lon + xi * s.cfg.out_res_deg, s.cfg.begin_lat + yi * s.cfg.out_res_deg
    a = m.spells_at(W['field'], s, xi, yi, WINDOW, W['fh'], cols, SCAN, ROUNDS)
    b = m.spells_at(W['field'], s, lon, lat, WINDOW, W['fh'], cols, SCAN, ROUNDS, lonlat=True)
    for key in RESULT_KEYS:
        assert EC.bitwise(a[key].cpu().numpy(), b[key].cpu().numpy()), key
    east = m.spell_lattice(W['field'], s, Lattice(250.0, 1.0, 60.0, 1.0, 0.0, 1.0, 12, 3, 1), WINDOW, W['fh'], cols, SCAN, ROUNDS)       # x = 250 .. 261
    out = np.zeros((4, 3, 12), dtype=bool)
    out[:, :, 7:] = True                                                  # x > 256: beyond the coarse cube
    status = east['status'].cpu().numpy()
    assert (status[out] == S.BAD_SCAN).all() and not (status[~out] & S.BAD_SCAN).any()
    for key in ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess'):
        v = east[key].cpu().numpy()
        assert np.isnan(v[out]).all() and np.isfinite(v[~out & ((status & S.NEVER) == 0)]).all(), key
    with pytest.raises(ValueError, match='nt == 1'):
        m.spell_lattice(W['field'], s, s.lattice(hours=(0.0, 1.0, 2), **LATTICE), WINDOW, W['fh'], cols)
    with pytest.raises(IndexError):
        m.spells_at(W['field'], s, xi + 100.0, yi, WINDOW, W['fh'], cols)
    with pytest.raises(ValueError):
        m.spells_at(W['field'], s, xi, yi, (3.0, 25.0), W['fh'], cols)
    with pytest.raises(KeyError):
        m.spells_at(W['field'], s, xi, yi, WINDOW, W['fh'], ['gust:above:20'])


# ------------------------------------------------------------------------------------------------ 4. against the dense route
def test_refined_spells_against_the_one_minute_dense_route():
    """Seed extremes_cases.DENSE_SEED (SyntheticSamples' default, the world of these tests), its 8 stations, the five columns and thresholds
    spells_cases.DENSE_COLUMNS fixed on the fp64 oracle (tests/test_spells_cpu.py::test_dense_route_conditions_hold_on_the_fp64_oracle), 24 h, hourly
    scan, R = 10, against predict_points on the one-minute lattice of the same window counted on the host.  On the device's own one-minute series the
    conditions still hold: at least half of the station-columns have a crossing, at most a quarter are left out for another crossing count on the
    hourly nodes than on the minutes -- left out by that count alone, never by how their hours compare --, none of the compared ones is a gap between
    two spells that reach the window's ends.  On every compared station-column: the same crossings, |first - dense first| and |last - dense last|
    <= 1/60 h + dt / 2**R, and with at most two crossings |hours - dense hours| <= crossings / 60 h + 2 dt / 2**R."""
    W = _world()
    m, s = W['m'], W['s']
    assert EC.DENSE_SEED == 0                                             # SyntheticSamples' default seed: _world()'s cube and field sample
    xs, ys = (np.array([p[j] for p in EC.DENSE_STATIONS]) for j in (0, 1))
    n = xs.size
    req = S.check_request(list(SC.DENSE_COLUMNS), SC.DENSE_WINDOW, SC.DENSE_SCAN, SC.DENSE_ROUNDS)
    got = m.spells_at(W['field'], s, xs, ys, SC.DENSE_WINDOW, W['fh'], list(SC.DENSE_COLUMNS), SC.DENSE_SCAN, SC.DENSE_ROUNDS)
    r = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    dense = m.predict_points(W['field'], s, np.tile(xs, SC.MINUTES.size), np.tile(ys, SC.MINUTES.size), np.repeat(SC.MINUTES, n), W['fh']).cpu().numpy()
    d = SC.dense_spells(SC.dense_series(dense.reshape(SC.MINUTES.size, n, 6), req.names), req)
    compared, crossing, left_out, gaps = SC.dense_conditions(d)
    print('dense route: %d station-columns with a crossing, %d left out, %d gaps; crossings dense %s, refined %s; hours dense %s, refined %s; first dense '
          '%s, refined %s; last dense %s, refined %s; status %s' % (crossing, left_out, gaps, d['crossings'].tolist(), r['crossings'].tolist(),
                                                                    d['hours'].tolist(), r['hours'].tolist(), d['first'].tolist(), r['first'].tolist(),
                                                                    d['last'].tolist(), r['last'].tolist(), r['status'].tolist()))
    assert not (r['status'] & (S.BAD_SCAN | S.STOPPED)).any()
    assert crossing >= 20 and left_out <= 10 and gaps == 0
    assert SC.check_against_dense(r, d, SC.DENSE_SCAN / 2 ** SC.DENSE_ROUNDS) >= 20


# ------------------------------------------------------------------------------------------------ 5. the inference loop and the launcher
def test_run_inference_interface_takes_the_spells_key(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg'].update(img_size=(145, 257), dt=21600)
    cfg['inference_cfg']['log'].update(write_source=True, result_path=str(tmp_path / 'out'), export_variable=['T'])
    cfg['inference_cfg']['spells'] = dict(columns=['T:below:221', 'speed:above:10'], window=(6.0, 12.0), scan_hours=2.0, refine=2,
                                          lonlat=[(100.5, 30.25), (110.0, 35.0), (72.5, 18.25)])
    torch.manual_seed(4)
    m = builder_models(**cfg)
    (tmp_path / 'ckpt').mkdir()
    m.save_model(str(tmp_path / 'ckpt'), epoch=0, global_step=1, prefix='physics')
    maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', device='cuda:0')
    e = m.last_spells
    assert maps is not None and e['names'] == ['T:below:221', 'speed:above:10'] and tuple(e['hours'].shape) == (3, 2) and e['first'].dtype == torch.float64
    files = {fn.split('_spell_')[1]: np.load(os.path.join(tmp_path / 'out', fn)) for fn in os.listdir(tmp_path / 'out') if '_spell_' in fn}
    assert sorted(files) == sorted(k + '.npy' for k in RESULT_KEYS)
    for key in RESULT_KEYS:
        assert EC.bitwise(files[key + '.npy'], e[key].cpu().numpy()), key
    assert np.isfinite(files['hours.npy']).all() and (files['hours.npy'] >= -1e-12).all() and (files['hours.npy'] <= 6.0 + 1e-12).all()


def test_infer_launcher_writes_the_spell_maps(tmp_path):
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
                            '--log_path', str(out), '--synthetic', '--spells', 'T:below:221,speed:above:10', '--spell_window', '0,24', '--spell_scan', '6',
                            '--spell_refine', '3'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert 'spells T:below:221,speed:above:10: hours (2, 145, 257)' in child.stdout
    names = sorted(fn.split('_spell_')[1] for fn in os.listdir(out) if '_spell_' in fn)
    assert names == sorted('%s_%s.npy' % (k, c) for k in RESULT_KEYS for c in ('T_below_221', 'speed_above_10'))
    files = {fn.split('_spell_')[1]: np.load(os.path.join(out, fn)) for fn in os.listdir(out) if '_spell_' in fn}
    assert all(a.shape == (145, 257) for a in files.values()) and files['hours_T_below_221.npy'].dtype == np.float64
    assert files['status_speed_above_10.npy'].dtype == np.int32 and files['crossings_T_below_221.npy'].dtype == np.int32
    hours = files['hours_T_below_221.npy']
    assert np.isfinite(hours).all() and (hours >= -1e-12).all() and (hours <= 24.0 + 1e-12).all() and hours.max() > 0.0
    assert len([fn for fn in os.listdir(out) if fn.endswith('_T.npy')]) == 5
