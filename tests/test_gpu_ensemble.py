"""GPU (MI355X): ensemble statistics over field samples -- dpn_ensemble_accumulate / dpn_ensemble_finish through PackedField.ensemble_accumulate,
EnsembleState, InterfacePhysics.ensemble_at / ensemble_lattice, run_inference_interface's inference_cfg.ensemble and infer.py --ensemble (hi+lo mode).

Yardsticks: deepphysinet_amd.ensemble.ensemble_reference, the numpy restatement of the two kernels (bit for bit: both are compiled without
contraction), fed with what dpn_diagnostics_out and dpn_fields_out write for the same inputs; the rows / maps / chunking identities of the inference
surface; the single-sample entry points.  Model, field, sampler and stations are those of tests/test_gpu_inference.py; the members are that model
on M different seeded fields and coarse cubes (member 0: the field and cube of that file)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_diagnostics import N, _inputs, _launch as _diag_launch, _loop_model, _physics_cases
from tests.test_gpu_inference import _stations
from tests.test_gpu_parity import _dev
from tests.test_sampler import _cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_MAX = 5
_cache = {}


def _members(M):
    """The first M of five members: dicts of field_data, forecast_h and sampler, as _inference_samples yields them."""
    if 'members' not in _cache:
        from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
        I = _inputs()
        out = [dict(field_data=I['field'], forecast_h=I['fh'], sampler=I['s'])]
        for m in range(1, M_MAX):
            g = torch.Generator().manual_seed(100 + m)
            field = I['field'].cpu().clone()
            field[:, :155] += 0.25 * torch.randn(field[:, :155].shape, generator=g)
            cube = torch.from_numpy(_cube(seed=3 + m)).to(_dev())
            out.append(dict(field_data=field.to(_dev()), forecast_h=I['fh'], sampler=CollocationSampler(SamplerConfig(), cube)))
        _cache['members'] = out
    return _cache['members'][:M]


def _kernel_inputs():
    """Per member the kernel's inputs at the 1 037 stations of seed 0 (out_n, jac_n, f), computed once."""
    if 'inputs' not in _cache:
        import deepphysinet_amd as dpn
        I = _inputs()
        xi, yi, hr = I['stations']
        rows = []
        for mem in _members(M_MAX):
            x, y, t, cd, f = mem['sampler'].at_positions(xi, yi, hr)
            with torch.no_grad():
                heads, evec, statics = I['m'].physics_net.field_weights(mem['field_data'], mem['forecast_h'])
                out_n, jac_n = dpn.pde_fields_and_jacobian(I['cfg'], x, y, t, cd, heads, evec, statics)
            rows.append((out_n.contiguous(), jac_n.contiguous(), f.reshape(-1).contiguous()))
        _cache['inputs'] = rows
    return _cache['inputs']


def _single_rows(out_n, jac_n, f, ph, clip):
    """[n, 34] float32: what dpn_diagnostics_out (ids 0..27) and dpn_fields_out (ids 28..33) write for one member's inputs, a point with a NaN among
    its six out_n NaN in every column (the rule of the diagnostics, which the ensemble calls extend to the six variables)."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.diagnostics import nan_rows
    from deepphysinet_amd.point_path import _ptr, _stream
    n = out_n.shape[0]
    diag = torch.empty((n, 28), dtype=torch.float32, device=_dev())
    fields = torch.empty((n, 6), dtype=torch.float32, device=_dev())
    assert _diag_launch(out_n, jac_n, f, n, ph, clip, list(range(28)), rows=diag) == 0
    assert L.load().dpn_fields_out(_ptr(out_n), n, ctypes.byref(ph), clip, _ptr(fields), None, None, 0, _stream()) == 0
    rows = torch.cat([diag, fields], dim=1).cpu().numpy()
    rows[nan_rows(out_n.cpu().numpy())] = np.nan
    return rows


def _values(case):
    """values [5, 1 037, 34] of a physics case of tests/test_gpu_diagnostics._physics_cases, computed once."""
    key = ('values', case)
    if key not in _cache:
        name, ph, clip = _physics_cases(_inputs())[case]
        _cache[key] = (name, ph, clip, np.stack([_single_rows(o, j, f, ph, clip) for o, j, f in _kernel_inputs()]))
    return _cache[key]


def _accumulate(state, out_n, jac_n, f, n, ph, clip, first=0, n_total=None, ids=-1, thr_col=-1, thr_val=-1, n_thr=None):
    """dpn_ensemble_accumulate on the tensors of `state` (a dict of count, mean, m2, vmin, vmax, exceed, ids, thr_col, thr_val); the keyword
    arguments override single arguments for the refusal cases."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    ids = state['ids'] if ids == -1 else ids
    thr_col = state['thr_col'] if thr_col == -1 else thr_col
    thr_val = state['thr_val'] if thr_val == -1 else thr_val
    arr = lambda v, t: None if v is None else (t * max(len(v), 1))(*v)
    return L.load().dpn_ensemble_accumulate(
        _ptr(out_n), _ptr(jac_n), _ptr(f), n, None if ph is None else ctypes.byref(ph), clip, arr(ids, ctypes.c_int32), 0 if ids is None else len(ids),
        arr(thr_col, ctypes.c_int32), arr(thr_val, ctypes.c_float), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, first,
        state['n_total'] if n_total is None else n_total, _ptr(state['count']), _ptr(state['mean']), _ptr(state['m2']), _ptr(state['vmin']),
        _ptr(state['vmax']), _ptr(state['exceed']), _stream())


def _new_state(n_total, ids, thr_col=(), thr_val=()):
    P, E, dev = len(ids), len(thr_col), _dev()
    return dict(n_total=n_total, ids=list(ids), thr_col=list(thr_col), thr_val=[float(v) for v in thr_val],
                count=torch.zeros((P, n_total), dtype=torch.int32, device=dev), mean=torch.zeros((P, n_total), dtype=torch.float64, device=dev),
                m2=torch.zeros((P, n_total), dtype=torch.float64, device=dev), vmin=torch.full((P, n_total), -7.0, dtype=torch.float32, device=dev),
                vmax=torch.full((P, n_total), -7.0, dtype=torch.float32, device=dev),               # not infinities: the kernel must not need them
                exceed=torch.zeros((max(E, 1), n_total), dtype=torch.int32, device=dev))


def _out(shape_of, P, E, fill=-7.0):
    dev = _dev()
    out = {k: torch.full(shape_of(P), fill, dtype=torch.float32, device=dev) for k in ('mean', 'spread', 'min', 'max')}
    out['count'] = torch.full(shape_of(P), -7, dtype=torch.int32, device=dev)
    out['prob'] = torch.full(shape_of(max(E, 1)), fill, dtype=torch.float32, device=dev)
    return out


def _finish(state, first, n, rows=None, maps=None, lattice=None, n_total=None, n_products=None, thr_col=-1, n_thr=None, drop=()):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    thr_col = state['thr_col'] if thr_col == -1 else thr_col
    table = lambda d: None if d is None else ctypes.byref(L.DpnEnsembleOut(*[None if k in drop else _ptr(d[k])
                                                                              for k in ('mean', 'spread', 'min', 'max', 'count', 'prob')]))
    get = lambda k: None if k in drop else _ptr(state[k])
    return L.load().dpn_ensemble_finish(get('count'), get('mean'), get('m2'), get('vmin'), get('vmax'), get('exceed'),
                                        state['n_total'] if n_total is None else n_total, len(state['ids']) if n_products is None else n_products,
                                        None if thr_col is None else (ctypes.c_int32 * max(len(thr_col), 1))(*thr_col),
                                        (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, first, n, table(rows), table(maps), lattice,
                                        _stream())


def _bit_equal(got, want):
    """NaN in the same places, and the same bits everywhere else (a -0 is not a +0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def _assert_equals_reference(got, values, thr_col, thr_val, what):
    from deepphysinet_amd.ensemble import ensemble_reference
    want = ensemble_reference(values, thr_col, thr_val)
    for key in ('count', 'mean', 'spread', 'min', 'max') + (('prob',) if len(thr_col) else ()):
        g = got[key].cpu().numpy()
        if key == 'prob':
            g = g[:, :len(thr_col)]
        if not _bit_equal(g, want[key]):
            bad = np.argwhere(~((g == want[key]) & (np.signbit(g) == np.signbit(want[key])) | (np.isnan(g) & np.isnan(want[key]))))
            raise AssertionError((what, key, len(bad), [(tuple(i), g[tuple(i)], want[key][tuple(i)]) for i in bad[:5]]))
    return want


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n', [1, 255, 256, 257, N])
def test_kernels_are_the_restatement_bit_for_bit(n):
    """accumulate per member, then finish in row form: every output equals ensemble_reference fed with dpn_diagnostics_out's rows (ids 0..27) and
    dpn_fields_out's rows (ids 28..33) of the same inputs, bit for bit -- rel_humidity too: the same kernel arithmetic produced the values on both
    sides.  One point, either side of the 256-thread block edge, a ragged multi-block size; M = 1, 2, 5 members; all 34 products with 16 thresholds
    spread over three columns, one product alone with two thresholds on it, the list reversed without thresholds, a list with a repeat and a
    threshold set to a value that occurs; the physics tables of the diagnostics test (without the clip, with it, a squared-form variable and a variable
    clipped on part of the points)."""
    all_ids = list(range(34))
    for case in range(3):
        name, ph, clip, values = _values(case)
        assert np.isfinite(values).all()
        v25, v31, v18 = (values[:, :, c] for c in (25, 31, 18))
        q = lambda v, k: [float(x) for x in np.quantile(v, np.linspace(0.1, 0.9, k)).astype(np.float32)]
        occurs = float(values[0, 0, 20])                                             # member 0's divergence at point 0: equal is not above
        requests = [(all_ids, [25] * 6 + [31] * 5 + [18] * 5, q(v25, 6) + q(v31, 5) + q(v18, 5)),
                    ([26], [0, 0], q(values[:, :, 26], 2)),
                    (all_ids[::-1], [], []),
                    ([20, 3, 26, 20, 18, 3, 31], [0, 3, 6], [occurs, occurs, q(v31, 1)[0]])]
        for M in (1, 2, 5):
            for ids, thr_col, thr_val in requests:
                st = _new_state(n, ids, thr_col, thr_val)
                for o, j, f in _kernel_inputs()[:M]:
                    assert _accumulate(st, o[:n], j[:n], f[:n], n, ph, clip) == 0
                got = _out(lambda c: (n, c), len(ids), len(thr_col))
                assert _finish(st, 0, n, rows=got) == 0
                want = _assert_equals_reference(got, values[:M, :n][:, :, ids], thr_col, thr_val, (name, M, ids))
                assert bool((want['count'] == M).all())
                if not thr_col:
                    assert bool((got['prob'] == -7.0).all())                         # no threshold: prob is not written
        # the threshold on a value that occurs: member 0 does not count at point 0, whatever the others do
        assert values[0, 0, 20] == np.float32(occurs)


# ------------------------------------------------------------------------------------------------ 2. the forward the request chooses
def test_request_chooses_the_forward_and_a_missing_jacobian_is_refused():
    """A request without a product that reads the Jacobian runs the fields-only forward: its statistics equal the reference fed with predict_points'
    rows (speed: diagnostics_reference on those rows).  The same columns inside a request that also holds vorticity come from the Jacobian forward
    and equal the reference fed with diagnostics_at's rows."""
    from deepphysinet_amd.diagnostics import diagnostics_reference
    I = _inputs()
    m = I['m']
    xi, yi, hr = _stations(300, seed=5)
    members = _members(3)
    names = ['speed', 'u', 'v', 'p', 'T', 'q', 'rho']
    calls = []
    import deepphysinet_amd.point_path as PP
    inner = PP._forward_points
    PP._forward_points = lambda *a, **k: (calls.append(k['want_jac']), inner(*a, **k))[1]
    try:
        got = m.ensemble_at(members, xi, yi, hr, names, thresholds={'speed': [0.5], 'T': [280.0]})
        assert calls == [False] * 3
        rows = [m.predict_points(mem['field_data'], mem['sampler'], xi, yi, hr, mem['forecast_h']).cpu().numpy() for mem in members]
        speed = [diagnostics_reference(r, np.zeros((300, 6, 3), np.float32), np.zeros(300, np.float32), ['speed'], np.float32) for r in rows]
        values = np.stack([np.concatenate([s, r], axis=1) for s, r in zip(speed, rows)])
        _assert_equals_reference(got, values, [0, 4], [0.5, 280.0], 'fields-only')
        assert got['names'] == names and got['thresholds'] == [('speed', 0.5), ('T', 280.0)]
        del calls[:]
        mixed = ['vorticity', 'speed', 'rel_humidity']
        got = m.ensemble_at(members, xi, yi, hr, mixed, thresholds={'rel_humidity': [0.9, 0.5]})
        assert calls == [True] * 3
    finally:
        PP._forward_points = inner
    values = np.stack([m.diagnostics_at(mem['field_data'], mem['sampler'], xi, yi, hr, mem['forecast_h'], mixed).cpu().numpy() for mem in members])
    _assert_equals_reference(got, values, [2, 2], [0.9, 0.5], 'with the Jacobian')
    # at the entry point: a product that reads J without jac_n, abs_vorticity without f
    o, j, f = (v[:300] for v in _kernel_inputs()[0])
    ph = I['cfg'].physics()
    for ids, jac, cor in (([18], None, f), ([25, 0], None, f), ([27], None, f), ([19], j, None), ([24], None, None)):
        assert _accumulate(_new_state(300, ids), o, jac, cor, 300, ph, 0) == -1, ids
    st = _new_state(300, [25, 26, 28, 33])
    assert _accumulate(st, o, None, None, 300, ph, 0) == 0                           # ... and without them where nothing reads them
    st18 = _new_state(300, [18, 20])
    assert _accumulate(st18, o, j, None, 300, ph, 0) == 0
    torch.cuda.synchronize()
    assert bool((st['count'] == 1).all()) and bool((st18['count'] == 1).all())


# ------------------------------------------------------------------------------------------------ 3. NaN
def test_a_poisoned_member_is_skipped_at_its_point_and_nowhere_else():
    I = _inputs()
    n, M = 300, 3
    ph = I['cfg'].physics()
    hit = [0, 63, 64, 255, 256, 299]
    ins = [(o[:n].clone(), j[:n], f[:n]) for o, j, f in _kernel_inputs()[:M]]
    for r, k in zip(hit, range(6)):
        ins[k % M][0][r, k] = float('nan')                                           # one entry of one member
    ids = list(range(34))
    st = _new_state(n, ids, [25, 31], [0.4, 280.0])
    for o, j, f in ins:
        assert _accumulate(st, o, j, f, n, ph, 1) == 0
    got = _out(lambda c: (n, c), 34, 2)
    assert _finish(st, 0, n, rows=got) == 0
    count = got['count'].cpu().numpy()
    want_count = np.full((n, 34), M, dtype=np.int32)
    want_count[hit] = M - 1
    assert np.array_equal(count, want_count)                                         # one less in every column of exactly those rows
    values = np.stack([_single_rows(o, j, f, ph, 1) for o, j, f in ins])
    assert int(np.isnan(values).sum()) == len(hit) * 34
    _assert_equals_reference(got, values, [25, 31], [0.4, 280.0], 'poisoned')


def test_lattice_points_outside_every_cube_have_count_zero_and_nan():
    from deepphysinet_amd.sampler import Lattice
    m = _inputs()['m']
    out = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    px, py, pt = out.positions()
    outside = ((px > 256) | (py > 144) | (pt > 24)).reshape(out.nt, 1, out.ny, out.nx)
    assert 0 < outside.sum() < outside.size
    names = ['vorticity', 'speed', 'T', 'rel_humidity']
    for clip in (False, True):
        e = m.ensemble_lattice(_members(2), out, names, thresholds={'speed': [0.5]}, with_clip=clip)
        where = np.repeat(outside, 4, axis=1)
        assert np.array_equal(e['count'].cpu().numpy(), np.where(where, 0, 2).astype(np.int32))
        for key in ('mean', 'spread', 'min', 'max'):
            a = e[key].cpu().numpy()
            assert np.array_equal(np.isnan(a), where) and np.all(np.isfinite(a[~where])), (key, clip)
        p = e['prob'].cpu().numpy()
        assert np.array_equal(np.isnan(p), outside) and np.all((p[~outside] >= 0) & (p[~outside] <= 1))


# ------------------------------------------------------------------------------------------------ 4. rows, maps, chunks
def _same_dict(a, b, nan_aware=False):
    for key in ('mean', 'spread', 'min', 'max', 'count', 'prob'):
        x, y = a[key], b[key]
        if nan_aware and x.dtype.is_floating_point:
            assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), key
        else:
            assert torch.equal(x, y), key


def test_lattice_maps_are_the_station_rows_chunked_or_not():
    from deepphysinet_amd.sampler import Lattice
    I = _inputs()
    s, m = I['s'], I['m']
    members = _members(3)
    names = ['dT_dt', 'abs_vorticity', 'speed', 'T', 'dT_dt']
    thr = {'speed': [0.3, 0.6], 'T': [280.0]}
    lat = s.lattice(refine=2, hours=(4.0, 0.5, 3), x_range=(10, 40), y_range=(20, 35.5))      # 61 x 32 x 3
    assert (lat.nx, lat.ny, lat.nt) == (61, 32, 3)
    px, py, pt = lat.positions()
    for clip in (False, True):
        rows = m.ensemble_at(members, px, py, pt, names, thresholds=thr, with_clip=clip)
        whole = m.ensemble_lattice(members, lat, names, thresholds=thr, with_clip=clip)
        for key, C in (('mean', 5), ('spread', 5), ('min', 5), ('max', 5), ('count', 5), ('prob', 3)):
            assert rows[key].shape == (lat.n_points, C) and whole[key].shape == (lat.nt, C, lat.ny, lat.nx), key
            assert torch.equal(whole[key], rows[key].view(lat.nt, lat.ny, lat.nx, C).permute(0, 3, 1, 2)), key
        assert bool((whole['count'] == 3).all()) and bool(torch.isfinite(whole['spread']).all()) and bool((whole['spread'][:, 2] > 0).all())
        assert torch.equal(whole['mean'][:, 0], whole['mean'][:, 4])                       # a repeated name is the same column
        for chunk in (128, 256, 640):
            _same_dict(m.ensemble_lattice(members, lat, names, thresholds=thr, with_clip=clip, chunk_points=chunk), whole)
    lon, la = 72.0 + px[:200] * 0.25, 18.0 + py[:200] * 0.25
    deg = m.ensemble_at(members, lon, la, pt[:200], names, thresholds=thr, with_clip=True, lonlat=True)
    for key in ('mean', 'spread', 'min', 'max', 'count', 'prob'):
        assert torch.equal(deg[key], rows[key][:200]), key
    # a chunk edge mid-row (20 x 15 x 4 points in chunks of 128: 6 rows + 8 points), on a lattice that leaves the cube
    out = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    a = m.ensemble_lattice(members, out, names, thresholds=thr)
    b = m.ensemble_lattice(members, out, names, thresholds=thr, chunk_points=128)
    assert 0 < int(torch.isnan(a['mean']).sum()) < a['mean'].numel()
    _same_dict(a, b, nan_aware=True)


# ------------------------------------------------------------------------------------------------ 5. the interface
def test_one_member_is_the_single_sample_call_and_equal_members_have_no_spread():
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    one = _members(1)
    lat = s.lattice(refine=1, hours=(3.0, 6.0, 2), x_range=(0, 70), y_range=(0, 40))          # 71 x 41 x 2
    diag = ['vorticity', 'dq_dt', 'speed', 'rel_humidity', 'deformation']
    var = ['u', 'v', 'p', 'T', 'q', 'rho']
    for clip in (False, True):
        for names, single in ((diag, m.diagnostic_lattice(field, s, lat, fh, diag, with_clip=clip)), (var, m.predict_lattice(field, s, lat, fh, with_clip=clip))):
            e = m.ensemble_lattice(one, lat, names, with_clip=clip)
            for key in ('mean', 'min', 'max'):
                assert torch.equal(e[key], single), (key, names, clip)
            assert bool((e['count'] == 1).all()) and bool(torch.isnan(e['spread']).all()) and e['prob'] is None and e['thresholds'] == []
    e = m.ensemble_lattice(one * 3, lat, diag + var, thresholds={'T': [0.0, 1e9]})
    assert bool((e['spread'] == 0).all()) and bool((e['count'] == 3).all()) and torch.equal(e['min'], e['max']) and torch.equal(e['mean'], e['min'])
    assert bool((e['prob'][:, 0] == 1).all()) and bool((e['prob'][:, 1] == 0).all())
    # refusals, all before anything is launched
    from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
    xi, yi, hr = _stations(10, seed=1)
    with pytest.raises(ValueError, match='no members'):
        m.ensemble_at([], xi, yi, hr, ['speed'])
    for over, field_name in ((dict(dx=25000.0), 'dx'), (dict(input_time_step=3), 'input_time_step')):
        other = dict(one[0], sampler=CollocationSampler(SamplerConfig(**over), s.cube))
        with pytest.raises(ValueError, match='member 1: %s' % field_name):
            m.ensemble_lattice([one[0], other], lat, ['speed'])
    shifted = dict(one[0], sampler=CollocationSampler(SamplerConfig(begin_lon=73.0), s.cube))
    m.ensemble_at([one[0], shifted], xi, yi, hr, ['speed'])                                   # index units: the origin does not matter
    with pytest.raises(ValueError, match='member 1: begin_lon'):
        m.ensemble_at([one[0], shifted], 80.0 + xi * 0.1, 20.0 + yi * 0.1, hr, ['speed'], lonlat=True)
    with pytest.raises(KeyError, match='gust'):
        m.ensemble_at(one, xi, yi, hr, ['speed', 'gust'])
    with pytest.raises(ValueError, match='17'):
        m.ensemble_at(one, xi, yi, hr, ['speed'], thresholds={'speed': list(range(17))})
    with pytest.raises(IndexError):
        m.ensemble_at(one, xi + 300.0, yi, hr, ['speed'])


# ------------------------------------------------------------------------------------------------ 6. entry-point refusals
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import _lib as L
    I = _inputs()
    n = 300
    o, j, f = (v[:n] for v in _kernel_inputs()[0])
    ph = I['cfg'].physics()
    ids, thr_col, thr_val = [18, 19, 25], [0, 2], [1e-5, 0.5]
    st = _new_state(n, ids, thr_col, thr_val)
    for key in ('count', 'exceed'):
        st[key].fill_(-7)
    for key in ('mean', 'm2'):
        st[key].fill_(-7.0)
    ok = dict(out_n=o, jac_n=j, f=f, n=n, ph=ph, clip=0)
    nan, inf = float('nan'), float('inf')
    cases = [dict(out_n=None), dict(jac_n=None), dict(f=None), dict(ph=None), dict(ids=None), dict(n=0), dict(n=-5), dict(first=-1), dict(first=1),
             dict(n_total=n - 1), dict(n_total=0), dict(ids=[]), dict(ids=list(range(34)) + [0]), dict(ids=[18, 34, 25]), dict(ids=[-1, 19, 25]),
             dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 3]), dict(thr_col=[-1, 2]), dict(thr_val=[1e-5, nan]), dict(thr_val=[inf, 0.5]),
             dict(thr_val=[1e-5, -inf]), dict(thr_col=None, n_thr=2), dict(thr_val=None, n_thr=2)]
    for case in cases:
        assert _accumulate(st, **{**ok, **case}) == -1, sorted(case)
    for key in ('count', 'mean', 'm2', 'vmin', 'vmax', 'exceed'):
        st2 = dict(st)
        st2[key] = None
        assert _accumulate(st2, **ok) == -1, key
    torch.cuda.synchronize()
    for key in ('count', 'mean', 'm2', 'vmin', 'vmax', 'exceed'):
        assert bool((st[key] == -7).all()), key
    # finish
    rows = _out(lambda c: (n, c), 3, 2)
    maps = _out(lambda c: (3, c, 10, 10), 3, 2)
    lat = L.DpnLattice(0, 1, 0, 1, 0, 1, 10, 10, 3)
    by = ctypes.byref
    good = dict(first=0, n=n, rows=rows)
    cases = [dict(rows=None), dict(rows=rows, maps=maps, lattice=by(lat)), dict(rows=rows, lattice=by(lat)), dict(rows=None, maps=maps),
             dict(n=0), dict(n=-1), dict(first=-1), dict(first=1), dict(n_total=n - 1), dict(n_products=0), dict(n_products=35), dict(n_thr=17), dict(n_thr=-1),
             dict(thr_col=[0, 3]), dict(thr_col=[-1, 0]), dict(thr_col=None, n_thr=2)] + \
            [dict(drop=(k,)) for k in ('count', 'mean', 'm2', 'vmin', 'vmax', 'exceed', 'spread', 'min', 'max', 'prob')] + \
            [dict(rows=None, maps=maps, lattice=by(L.DpnLattice(0, 1, 0, 1, 0, 1, *dims))) for dims in ((0, 10, 3), (10, 0, 3), (10, 10, 0), (10, 10, 2))]
    for case in cases:
        assert _finish(st, **{**good, **case}) == -1, sorted(case)
    torch.cuda.synchronize()
    for d in (rows, maps):
        for key, v in d.items():
            assert bool((v == -7).all()), key
    # and the same arguments, accepted: 300 points fill a 10 x 10 x 3 lattice exactly; rows and maps hold the same numbers
    st = _new_state(n, ids, thr_col, thr_val)
    assert _accumulate(st, **ok) == 0 and _finish(st, **good) == 0 and _finish(st, 0, n, maps=maps, lattice=by(lat)) == 0
    torch.cuda.synchronize()
    for key in ('mean', 'min', 'max', 'count', 'prob'):
        C = rows[key].shape[1]
        assert bool((rows[key] != -7).all()) and torch.equal(maps[key].permute(0, 2, 3, 1).reshape(n, C), rows[key]), key
    assert bool(torch.isnan(rows['spread']).all()) and bool(torch.isnan(maps['spread']).all())


# ------------------------------------------------------------------------------------------------ 7. loop and launcher
class _Spy:
    """Counts calls of the two new entry points on the loaded library (the spy of tests/test_gpu_diagnostics.py)."""
    NAMES = ('dpn_ensemble_accumulate', 'dpn_ensemble_finish')

    def __init__(self):
        from deepphysinet_amd import _lib as L
        self.lib, self.calls = L.load(), []
        self.inner = {name: getattr(self.lib, name) for name in self.NAMES}

    def __enter__(self):
        for name, fn in self.inner.items():
            setattr(self.lib, name, lambda *a, _n=name, _f=fn: (self.calls.append(_n), _f(*a))[1])
        return self

    def __exit__(self, *exc):
        for name, fn in self.inner.items():
            setattr(self.lib, name, fn)


def test_loop_writes_the_statistics_and_leaves_the_rest_alone(tmp_path):
    plain, with_key = tmp_path / 'plain', tmp_path / 'ens'
    m = _loop_model(tmp_path, write_source=True, result_path=str(plain), export_variable=['T'])
    ref = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
    assert m.last_ensemble is None
    m = _loop_model(tmp_path, write_source=True, result_path=str(with_key), export_variable=['T'])
    m.inference_cfg['ensemble'] = dict(products=['speed', 'T'], thresholds={'speed': [0.5, 1.5]})
    with _Spy() as spy:
        maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
        assert spy.calls == ['dpn_ensemble_accumulate'] * 2 + ['dpn_ensemble_finish']        # two members, one chunk
    nt = 13
    assert maps.shape == (nt, 6, 145, 257) and torch.equal(maps, ref)                        # the return value is unchanged
    for fn in sorted(os.listdir(plain)):                                                     # ... and so are the per-sample files
        assert np.array_equal(np.load(plain / fn), np.load(with_key / fn)), fn
    assert len(os.listdir(plain)) == 2 * nt - 1                                              # (the samples' windows share one stamp)
    e = m.last_ensemble
    assert e['names'] == ['speed', 'T'] and e['thresholds'] == [('speed', 0.5), ('speed', 1.5)]
    assert e['mean'].shape == (nt, 2, 145, 257) and e['prob'].shape == (nt, 2, 145, 257) and bool((e['count'] == 2).all())
    assert bool(torch.isfinite(e['spread']).all()) and bool((e['spread'][:, 0] > 0).any()) and bool((e['prob'][:, 1] <= e['prob'][:, 0]).all())
    new = sorted(fn for fn in os.listdir(with_key) if '_ens_' in fn)
    assert len(new) == nt * (2 * 5 + 2) and len(os.listdir(with_key)) == 2 * nt - 1 + len(new)
    stamps = sorted({fn.split('_ens_')[0] for fn in new})
    assert stamps == sorted(fn[:-len('_T.npy')] for fn in os.listdir(plain))[:nt]            # the first sample's stamps (they sort in time order)
    for it, stamp in enumerate(stamps):
        for j, name in enumerate(e['names']):
            for key in ('mean', 'spread', 'min', 'max', 'count'):
                a = np.load(with_key / ('%s_ens_%s_%s.npy' % (stamp, key, name)))
                assert a.shape == (145, 257) and a.dtype == (np.int32 if key == 'count' else np.float32)
                assert np.array_equal(a, e[key][it, j].cpu().numpy()), (stamp, key, name)
        for j, value in enumerate(('0.5', '1.5')):
            assert np.array_equal(np.load(with_key / ('%s_ens_prob_speed_gt_%s.npy' % (stamp, value))), e['prob'][it, j].cpu().numpy())


def test_nothing_calls_the_new_kernels_without_the_key(tmp_path):
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    xi, yi, hr = _stations(300, seed=5)
    lat = s.lattice(hours=3, x_range=(0, 40), y_range=(0, 30))
    loop = _loop_model(tmp_path, write_source=False, export_diagnostic=['vorticity'])
    with _Spy() as spy:
        m.predict_points(field, s, xi, yi, hr, fh)
        m.predict_lattice(field, s, lat, fh)
        m.residuals_at(field, s, xi, yi, hr, fh)
        m.diagnostics_at(field, s, xi, yi, hr, fh, ['speed'])
        m.diagnostic_lattice(field, s, lat, fh, ['speed', 'vorticity'])
        assert loop.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic') is not None
        assert spy.calls == [] and loop.last_ensemble is None
        m.ensemble_at(_members(2), xi, yi, hr, ['speed'])                                # the spy does see the kernels when they are asked for
        assert spy.calls == ['dpn_ensemble_accumulate'] * 2 + ['dpn_ensemble_finish']


def test_the_launcher_runs_with_the_ensemble_flags(tmp_path):
    _loop_model(tmp_path)
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--ensemble', 'speed,T', '--ensemble_threshold', 'speed:0.5'], cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert "ensemble speed,T: mean (49, 2, 145, 257), members counted 1..1, thresholds [('speed', 0.5)]" in child.stdout
    assert len([fn for fn in os.listdir(tmp_path / 'cli') if '_ens_' in fn]) == 49 * (2 * 5 + 1)
