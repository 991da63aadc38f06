"""GPU (MI355X): regional statistics in space -- dpn_region_accumulate / dpn_region_finish through RegionState, PackedField.region_accumulate,
InterfacePhysics.regional_lattice / regional_at, run_inference_interface's inference_cfg.regions and infer.py --regions (hi+lo mode).

Yardsticks: deepphysinet_amd.regions.regions_reference, the numpy restatement of the two kernels, partials included (bit for bit: both are compiled
without contraction), fed with what dpn_diagnostics_out and dpn_fields_out write for the same inputs; diagnostic_lattice / predict_lattice + fp64
numpy masked reductions (count, min, max and where exactly; mean, total and frac within the bound of sequential fp64 summation); the chunking and
station / lattice identities of the inference surface.  Model, field, sampler and stations are those of tests/test_gpu_diagnostics.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import regions_cases as RC
from tests.test_gpu_diagnostics import N, _inputs, _loop_model, _physics_cases
from tests.test_gpu_ensemble import _single_rows
from tests.test_gpu_parity import _dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT_MAX = 3
IDS16 = [18, 19, 25, 31, 0, 17, 20, 21, 24, 26, 27, 28, 33, 22, 30, 19]      # ids that read J, f (19) and neither (25, 26, 28..33); one repeat
THR_COL16 = [0] * 4 + [2] * 4 + [3] * 4 + [9] * 4
PARTIALS = ('w', 'wx', 'count', 'vmin', 'vmax', 'imin', 'imax', 'wexc')
_cache = {}


def _pool():
    """3 x 1 037 rows of kernel inputs (out_n, jac_n, f): the stations of tests/test_gpu_diagnostics.py in three orders, five rows poisoned (a NaN
    in one of their six out_n)."""
    if 'pool' not in _cache:
        I = _inputs()
        o, j, f = I['out_n'], I['jac_n'], I['f']
        o = torch.cat([o, o.flip(0), o.roll(517, 0)]).clone()
        for row, k in ((1, 3), (2, 0), (130, 5), (N + 1, 1), (2 * N + 7, 4)):
            o[row, k] = float('nan')
        _cache['pool'] = (o.contiguous(), torch.cat([j, j.flip(0), j.roll(517, 0)]).contiguous(), torch.cat([f, f.flip(0), f.roll(517, 0)]).contiguous())
    return _cache['pool']


def _values(case):
    """[3 111, 34] float32: what dpn_diagnostics_out (ids 0..27) and dpn_fields_out (ids 28..33) write for the pool under a physics case of
    tests/test_gpu_diagnostics._physics_cases (NaN in every column of a poisoned row), computed once."""
    key = ('values', case)
    if key not in _cache:
        name, ph, clip = _physics_cases(_inputs())[case]
        _cache[key] = (ph, clip, _single_rows(*_pool(), ph, clip))
    return _cache[key]


def _plan(n_sel, R, seed=0):
    """n_sel stations in R groups (some empty where n_sel is small), weights in [0.5, 1) with zeros."""
    from deepphysinet_amd.regions import region_plan
    g = np.random.default_rng(1000 * R + n_sel + seed)
    groups = g.integers(0, R, size=n_sel)
    w = g.uniform(0.5, 1.0, size=n_sel).astype(np.float32)
    w[g.integers(0, n_sel, size=max(1, n_sel // 8))] = 0
    if n_sel == 1:
        w[:] = 0.75
    return region_plan(groups=groups, weights=w, n_regions=R)


def _flat_rows(plan, nt):
    """Pool rows of the flat point list: entry j of time plane it is pool row it * 1 037 + order[j]."""
    return torch.from_numpy(np.concatenate([it * N + plan.order for it in range(nt)])).to(_dev())


def _assert_state_and_outputs(state, out, want, what):
    for key in PARTIALS:
        got = getattr(state, key)
        if got is None:
            assert want['partials'][key].shape[0] == 0
            continue
        assert RC.same(got.cpu().numpy(), want['partials'][key]), (what, 'partial', key)
    for key in RC.KEYS:
        if out[key] is None:
            assert key == 'frac' and want['frac'].shape[-1] == 0
            continue
        assert RC.same(out[key].cpu().numpy(), want[key]), (what, key)


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n_sel', [1, 63, 64, 65, 255, 256, 257, N])
def test_kernels_are_the_restatement_bit_for_bit(n_sel):
    """One accumulate launch over the whole flat list, then finish: all eight partial arrays and all nine outputs equal regions_reference fed with
    dpn_diagnostics_out's and dpn_fields_out's rows of the same inputs, bit for bit.  One point, either side of the 64-point group and of the
    256-thread block, a ragged multi-block size; R = 1, 3, 40 regions; nt = 1, 3 time nodes (groups then straddle the time planes); one product that
    reads neither the Jacobian nor f (both pointers NULL) without thresholds, and 16 products that read J, f and neither with 16 thresholds on four
    columns; weights with zeros; poisoned rows."""
    from deepphysinet_amd.point_path import RegionState
    from deepphysinet_amd.regions import regions_reference
    o, j, f = _pool()
    requests = []
    ph, clip, values = _values(0)
    requests.append((ph, clip, values, [31], [], []))
    ph, clip, values = _values(2)
    quant = [float(x) for c in (0, 2, 3, 9) for x in np.nanquantile(values[:, IDS16[c]], [0.2, 0.4, 0.6, 0.8]).astype(np.float32)]
    quant[5] = float(values[N + 5, 25])                                       # a value that occurs: equal is not above
    requests.append((ph, clip, values, IDS16, THR_COL16, quant))
    for R in (1, 3, 40):
        plan = _plan(n_sel, R)
        for nt in (1, NT_MAX):
            rows = _flat_rows(plan, nt)
            on, jn, fn = o[rows].contiguous(), j[rows].contiguous(), f[rows].contiguous()
            for ph, clip, values, ids, thr_col, thr_val in requests:
                state = RegionState(plan, nt, ids, thr_col, thr_val, _dev())
                need_j, need_f = any(i <= 24 or i == 27 for i in ids), 19 in ids
                state.accumulate(on, jn if need_j else None, fn if need_f else None, ph, 0, clip)
                out = state.finish()
                want = regions_reference(values[rows.cpu().numpy()][:, ids], plan, nt, thr_col, thr_val)
                _assert_state_and_outputs(state, out, want, (n_sel, R, nt, len(ids)))
                assert int(want['count'].sum()) > 0
    if n_sel >= 255:
        assert np.isnan(values[rows.cpu().numpy()]).any() and (plan.wgt == 0).any()       # poisoned rows and zero weights took part


# ------------------------------------------------------------------------------------------------ 2. chunks, two runs
def test_chunking_and_a_second_run_change_no_bit():
    """The flat list of 3 x 1 037 points in chunks of 128, 256, 640 points and in one: identical partials and outputs; two runs alike.  Then the
    interface on a lattice: chunk_points 128, 256, 640 and one chunk, and a second run, give identical dicts."""
    from deepphysinet_amd.point_path import RegionState
    o, j, f = _pool()
    ph, clip, values = _values(1)
    plan = _plan(N, 40, seed=1)
    rows = _flat_rows(plan, NT_MAX)
    on, jn, fn = o[rows].contiguous(), j[rows].contiguous(), f[rows].contiguous()
    thr_val = [float(x) for x in np.linspace(0.1, 0.9, 16)]

    def run(chunk):
        state = RegionState(plan, NT_MAX, IDS16, THR_COL16, thr_val, _dev())
        for first in range(0, on.shape[0], chunk):
            state.accumulate(on[first:first + chunk], jn[first:first + chunk], fn[first:first + chunk], ph, first, clip)
        return state, state.finish()
    whole = run(on.shape[0])
    for chunk in (128, 256, 640, on.shape[0]):
        state, out = run(chunk)
        for key in PARTIALS:
            assert RC.same(getattr(state, key).cpu().numpy(), getattr(whole[0], key).cpu().numpy()), (chunk, key)
        for key in RC.KEYS:
            assert RC.same(out[key].cpu().numpy(), whole[1][key].cpu().numpy()), (chunk, key)
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    lat = s.lattice(refine=2, hours=(4.0, 0.5, 3), x_range=(10, 40), y_range=(20, 35.5))      # 61 x 32 x 3
    lab = _labels(lat.ny, lat.nx)
    names, thr = ['dT_dt', 'abs_vorticity', 'speed', 'T'], {'speed': [0.25, 0.75], 'T': [280.0]}
    one = m.regional_lattice(field, s, lat, fh, lab, names, weights='area', thresholds=thr, with_clip=True)
    assert one['mean'].shape == (3, 5, 4) and one['frac'].shape == (3, 5, 3) and one['where_max'].shape == (3, 5, 4, 2)
    assert one['names'] == names and one['thresholds'] == [('speed', 0.25), ('speed', 0.75), ('T', 280.0)]
    for chunk in (128, 256, 640, None):
        again = m.regional_lattice(field, s, lat, fh, lab, names, weights='area', thresholds=thr, with_clip=True, chunk_points=chunk)
        for key in RC.KEYS:
            assert torch.equal(again[key], one[key]), (chunk, key)


def _labels(ny, nx):
    """A label plane of 5 regions over about 60 % of the plane, the rest -1: vertical bands of different widths, cut by a diagonal."""
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    lab = (ix * 5 // nx).astype(np.int64)
    lab[(ix + 2 * iy) % 5 < 2] = -1
    return lab


# ------------------------------------------------------------------------------------------------ 3. the composed route
def test_regional_lattice_against_the_maps_and_numpy_reductions():
    """diagnostic_lattice / predict_lattice build the maps, fp64 numpy reduces them region by region; the lattice leaves the coarse cube (NaN there)
    and the area weights differ row by row.  count, min, max and where are equal exactly (the station route gives the lattice maps' bits).  mean,
    total and frac stay within 2^-24 |v| + 2 N 2^-52 S / W, N the points of the cell: the bound of N sequential fp64 additions of exact products, with
    S = sum |w x| for the mean, S = W sum |w x| for the total (nothing is divided) and S = W for frac (x is 0 or 1).
    Measured (MI355X): the largest error is 0.827 of its bound, with and without the clip (the float32 rounding of the result is nearly all of it)."""
    from deepphysinet_amd.sampler import Lattice
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    lat = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    lab = _labels(lat.ny, lat.nx)
    names = ['vorticity', 'speed', 'T', 'dq_dt']
    thr = {'speed': [0.5], 'T': [281.0, 283.0]}
    thr_list = [(1, np.float32(0.5)), (2, np.float32(281.0)), (2, np.float32(283.0))]
    for clip in (False, True):
        got = m.regional_lattice(field, s, lat, fh, lab, names, weights='area', thresholds=thr, with_clip=clip)
        diag = m.diagnostic_lattice(field, s, lat, fh, ['vorticity', 'speed', 'dq_dt'], with_clip=clip).cpu().numpy()
        var = m.predict_lattice(field, s, lat, fh, with_clip=clip).cpu().numpy()
        maps = np.stack([diag[:, 0], diag[:, 1], var[:, 3], diag[:, 2]], axis=1)              # [nt, P, ny, nx]
        assert 0 < int(np.isnan(maps).sum()) < maps.size
        wrow = np.cos(np.deg2rad(18.0 + (140.0 + 0.5 * np.arange(lat.ny)) * 0.25)).astype(np.float32)
        w = np.repeat(wrow[:, None], lat.nx, axis=1).astype(np.float64)
        g = {k: got[k].cpu().numpy() for k in RC.KEYS}
        worst = 0.0
        for it in range(lat.nt):
            for r in range(5):
                for p in range(4):
                    x = maps[it, p]
                    sel = (lab == r) & np.isfinite(x)
                    n = int(sel.sum())
                    assert g['count'][it, r, p] == n
                    if n == 0:
                        assert g['weight'][it, r, p] == 0 and np.isnan(g['mean'][it, r, p]) and (g['where_min'][it, r, p] == -1).all()
                        continue
                    xs, ws = x[sel].astype(np.float64), w[sel]
                    iy, ix = np.nonzero(sel)                                                  # ascending plane order: argmin is the first minimum
                    lo, hi = int(np.argmin(xs)), int(np.argmax(xs))
                    assert g['min'][it, r, p] == x[sel][lo] and g['max'][it, r, p] == x[sel][hi]
                    assert g['where_min'][it, r, p].tolist() == [ix[lo], iy[lo]] and g['where_max'][it, r, p].tolist() == [ix[hi], iy[hi]]
                    W, S = ws.sum(), np.abs(ws * xs).sum()
                    eps = 2 * n * 2.0 ** -52
                    checks = [('mean', g['mean'][it, r, p], (ws * xs).sum() / W, eps * S / W), ('total', g['total'][it, r, p], (ws * xs).sum(), eps * S),
                              ('weight', g['weight'][it, r, p], W, eps * W)]
                    for e, (col, t) in enumerate(thr_list):
                        if col == p:
                            checks.append(('frac', g['frac'][it, r, e], ws[x[sel] > t].sum() / W, eps))
                    for key, a, b, slack in checks:
                        bound = 2.0 ** -24 * abs(b) + slack
                        worst = max(worst, abs(float(a) - b) / bound)
                        assert abs(float(a) - b) <= bound, (key, it, r, p, a, b, bound)
        print('clip %s: largest error / bound %.3f' % (clip, worst))
        assert np.isnan(g['frac'][g['count'][:, :, [1, 2, 2]] == 0]).all()


# ------------------------------------------------------------------------------------------------ 4. the forward the request chooses
def test_request_chooses_the_forward_and_a_missing_jacobian_is_refused():
    """A request without a product that reads the Jacobian runs the fields-only forward: with every station a group of its own, min = max = mean are
    predict_points' rows, bit for bit.  At the entry point a product that reads J without jac_n, or f without f, is refused."""
    from deepphysinet_amd.point_path import RegionState
    from tests.test_gpu_inference import _stations
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    xi, yi, _ = _stations(300, seed=5)
    names = ['u', 'v', 'p', 'T', 'q', 'rho']
    calls = []
    import deepphysinet_amd.point_path as PP
    inner = PP._forward_points
    PP._forward_points = lambda *a, **k: (calls.append(k['want_jac']), inner(*a, **k))[1]
    try:
        got = m.regional_at(field, s, xi, yi, [3.0, 7.5], fh, np.arange(300), names)
        assert calls == [False]
        del calls[:]
        m.regional_at(field, s, xi, yi, [3.0, 7.5], fh, np.arange(300), names + ['vorticity'])
        assert calls == [True]
    finally:
        PP._forward_points = inner
    for it, hour in enumerate((3.0, 7.5)):
        rows = m.predict_points(field, s, xi, yi, np.full(300, hour), fh)
        for key in ('min', 'max', 'mean', 'total'):
            assert torch.equal(got[key][it], rows), (key, hour)
    assert bool((got['count'] == 1).all()) and bool((got['weight'] == 1).all()) and got['frac'] is None
    assert torch.equal(got['where_min'][0, :, 0], torch.arange(300, device=_dev()))
    o, j, f = (v[:256] for v in _pool())
    ph = I['cfg'].physics()
    plan = _plan(256, 3)
    for ids, jac, cor in (([18], None, f), ([25, 0], None, f), ([27], None, f), ([19], j, None), ([24], None, None)):
        st = RegionState(plan, 1, ids, [], [], _dev())
        with pytest.raises(RuntimeError, match='code -1'):
            st.accumulate(o, jac, cor, ph, 0)
        torch.cuda.synchronize()
        assert not bool(st.count.any())
    st = RegionState(plan, 1, [25, 26, 28, 33], [], [], _dev())
    st.accumulate(o, None, None, ph, 0)                                                       # ... and without them where nothing reads them
    assert int(st.finish()['count'].sum()) > 0


# ------------------------------------------------------------------------------------------------ 5. stations and lattices
def test_regional_at_is_regional_lattice_on_the_same_positions():
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    lat = s.lattice(refine=2, hours=(4.0, 0.5, 3), x_range=(10, 40), y_range=(20, 35.5))      # 61 x 32 x 3
    plane = lat.ny * lat.nx
    px, py, pt = lat.positions()
    lab = _labels(lat.ny, lat.nx)
    w = np.random.default_rng(3).uniform(0.0, 2.0, size=lab.shape).astype(np.float32)
    w[::7, ::3] = 0
    names, thr = ['vorticity', 'speed', 'T'], {'speed': [0.4], 'T': [280.0, 285.0]}
    on_lattice = m.regional_lattice(field, s, lat, fh, lab, names, weights=w, thresholds=thr)
    at = m.regional_at(field, s, px[:plane], py[:plane], pt[::plane], fh, lab.reshape(-1), names, weights=w.reshape(-1), thresholds=thr)
    deg = m.regional_at(field, s, 72.0 + px[:plane] * 0.25, 18.0 + py[:plane] * 0.25, pt[::plane], fh, lab.reshape(-1), names, weights=w.reshape(-1),
                        thresholds=thr, lonlat=True)
    for other in (at, deg):
        for key in ('mean', 'total', 'weight', 'min', 'max', 'count', 'frac'):
            assert torch.equal(other[key], on_lattice[key]), key
        for key in ('where_min', 'where_max'):
            ixy = on_lattice[key]
            assert torch.equal(other[key], ixy[..., 1] * lat.nx + ixy[..., 0]), key          # the station index of a plane is iy * nx + ix
    assert bool((on_lattice['count'] > 0).all()) and bool(torch.isfinite(on_lattice['mean']).all())
    lab_at = torch.from_numpy(lab).to(_dev())[on_lattice['where_max'][..., 1], on_lattice['where_max'][..., 0]]
    assert torch.equal(lab_at, torch.arange(5, device=_dev()).view(1, 5, 1).expand(3, 5, 3))  # the maximum of region r sits inside region r
    area = m.regional_at(field, s, px[:plane], py[:plane], [4.0], fh, lab.reshape(-1), ['T'], weights='area')
    area_lat = m.regional_lattice(field, s, s.lattice(refine=2, hours=4.0, x_range=(10, 40), y_range=(20, 35.5)), fh, lab, ['T'], weights='area')
    assert torch.equal(area['mean'], area_lat['mean']) and torch.equal(area['weight'], area_lat['weight'])
    with pytest.raises(IndexError):
        m.regional_at(field, s, px[:plane] + 300.0, py[:plane], [4.0], fh, lab.reshape(-1), ['T'])
    with pytest.raises(IndexError):
        m.regional_at(field, s, px[:plane], py[:plane], [4.0, 25.0], fh, lab.reshape(-1), ['T'])


# ------------------------------------------------------------------------------------------------ 6. entry-point refusals
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import RegionState, _ptr, _stream
    lib = L.load()
    o, j, f = (v[:200].contiguous() for v in _pool())
    ph = _inputs()['cfg'].physics()
    plan = _plan(100, 3)
    st = RegionState(plan, 2, [18, 19, 25], [0, 2], [1e-5, 0.5], _dev())
    tensors = [getattr(st, k) for k in PARTIALS]
    for t in tensors:
        t.fill_(-7)
    by = ctypes.byref
    i32, f32 = (lambda *v: (ctypes.c_int32 * len(v))(*v)), (lambda *v: (ctypes.c_float * len(v))(*v))
    p = lambda seg=st.seg, wgt=st.wgt, offs=st.offs, n_sel=100, R=3, nt=2: by(L.DpnRegionPlan(_ptr(seg), _ptr(wgt), _ptr(offs), n_sel, R, nt))
    state = lambda drop=None: by(L.DpnRegionState(*[None if k == drop else _ptr(getattr(st, k)) for k in PARTIALS]))
    acc_ok = dict(out_n=_ptr(o), jac_n=_ptr(j), f=_ptr(f), n=136, ph=by(ph), clip=0, ids=i32(18, 19, 25), P=3, col=i32(0, 2), val=f32(1e-5, 0.5), E=2, first=64,
                  plan=p(), st=state(), stream=_stream())
    acc = lambda **k: lib.dpn_region_accumulate(*{**acc_ok, **k}.values())
    nan, inf = float('nan'), float('inf')
    cases = [dict(out_n=None), dict(jac_n=None), dict(f=None), dict(ph=None), dict(ids=None), dict(plan=None), dict(st=None), dict(n=0), dict(n=-3),
             dict(first=-64), dict(first=1), dict(first=63), dict(first=128, n=73), dict(first=0, n=201), dict(P=0), dict(P=17), dict(E=17), dict(E=-1),
             dict(ids=i32(18, 34, 25)), dict(ids=i32(-1, 19, 25)), dict(col=i32(0, 3)), dict(col=i32(-1, 2)), dict(val=f32(1e-5, nan)), dict(val=f32(inf, 0.5)),
             dict(val=f32(1e-5, -inf)), dict(col=None), dict(val=None), dict(plan=p(seg=None)), dict(plan=p(wgt=None)), dict(plan=p(n_sel=0)),
             dict(plan=p(R=0)), dict(plan=p(nt=0)), dict(plan=p(n_sel=2 ** 30)), dict(plan=p(n_sel=2 ** 31, nt=1))] + [dict(st=state(k)) for k in PARTIALS]
    for case in cases:
        assert acc(**case) == -1, sorted(case)
    out = {k: torch.full((2, 3, 3), -7, dtype=torch.float32 if k in ('mean', 'total', 'weight', 'min', 'max') else torch.int32, device=_dev())
           for k in RC.KEYS[:-1]}
    out['frac'] = torch.full((2, 3, 2), -7.0, dtype=torch.float32, device=_dev())
    table = lambda drop=None: by(L.DpnRegionOut(*[None if k == drop else _ptr(out[k]) for k in RC.KEYS]))
    fin_ok = dict(plan=p(), st=state(), P=3, col=i32(0, 2), E=2, out=table(), stream=_stream())
    fin = lambda **k: lib.dpn_region_finish(*{**fin_ok, **k}.values())
    cases = [dict(plan=None), dict(st=None), dict(out=None), dict(P=0), dict(P=17), dict(E=17), dict(E=-1), dict(col=i32(0, 3)), dict(col=i32(-1, 0)),
             dict(col=None), dict(plan=p(offs=None)), dict(plan=p(n_sel=0)), dict(plan=p(R=0)), dict(plan=p(nt=0)), dict(plan=p(n_sel=2 ** 30))] + \
            [dict(st=state(k)) for k in PARTIALS] + [dict(out=table(k)) for k in RC.KEYS]
    for case in cases:
        assert fin(**case) == -1, sorted(case)
    torch.cuda.synchronize()
    for key, t in list(zip(PARTIALS, tensors)) + list(out.items()):
        assert bool((t == -7).all()), key
    # and the same arguments, accepted
    for t in tensors:
        t.zero_()
    assert acc(first=0, n=200) == 0 and fin() == 0
    torch.cuda.synchronize()
    assert int(out['count'].sum()) > 0 and bool((out['frac'] != -7).all())


# ------------------------------------------------------------------------------------------------ 7. loop and launcher
class _Spy:
    """Counts calls of the two new entry points on the loaded library (the spy of tests/test_gpu_diagnostics.py)."""
    NAMES = ('dpn_region_accumulate', 'dpn_region_finish')

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


def test_loop_writes_the_tables_and_leaves_the_rest_alone(tmp_path):
    plain, with_key = tmp_path / 'plain', tmp_path / 'regions'
    m = _loop_model(tmp_path, write_source=True, result_path=str(plain), export_variable=['T'])
    with _Spy() as spy:
        ref = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
        assert spy.calls == [] and m.last_regions is None                                     # without the key nothing new is called
    lab = _labels(145, 257)
    np.save(tmp_path / 'labels.npy', lab)
    m = _loop_model(tmp_path, write_source=True, result_path=str(with_key), export_variable=['T'])
    m.inference_cfg['regions'] = dict(products=['speed', 'T'], labels=str(tmp_path / 'labels.npy'), weights='area', thresholds={'speed': [0.5, 1.5]})
    with _Spy() as spy:
        maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
        assert spy.calls == ['dpn_region_accumulate', 'dpn_region_finish'] * 2                # two samples, one chunk each
    nt = 13
    assert maps.shape == (nt, 6, 145, 257) and torch.equal(maps, ref)                        # the return value is unchanged
    for fn in sorted(os.listdir(plain)):                                                     # ... and so are the per-sample files
        assert np.array_equal(np.load(plain / fn), np.load(with_key / fn)), fn
    r = m.last_regions
    assert r['names'] == ['speed', 'T'] and r['thresholds'] == [('speed', 0.5), ('speed', 1.5)] and r['mean'].shape == (nt, 5, 2)
    assert int(r['count'].min()) > 0 and bool((r['frac'][..., 1] <= r['frac'][..., 0]).all())
    new = sorted(fn for fn in os.listdir(with_key) if '_region_' in fn)
    assert len(new) == 2 * (8 * 2 + 2) and len(os.listdir(with_key)) == len(os.listdir(plain)) + len(new)
    stamp = new[-1].split('_region_')[0]                                                      # the last sample's first time step
    for j, name in enumerate(r['names']):
        for key in RC.KEYS[:-1]:
            a = np.load(with_key / ('%s_region_%s_%s.npy' % (stamp, key, name)))
            assert a.shape == ((nt, 5, 2) if key.startswith('where') else (nt, 5)) and np.array_equal(a, r[key][:, :, j].cpu().numpy(), equal_nan=True), key
    for j, value in enumerate(('0.5', '1.5')):
        assert np.array_equal(np.load(with_key / ('%s_region_frac_speed_gt_%s.npy' % (stamp, value))), r['frac'][:, :, j].cpu().numpy())
    # against the maps the loop returns: the last sample's mean T of region 0 at the first time step, area-weighted
    x = maps[0, 3].cpu().numpy().astype(np.float64)
    w = np.repeat(np.cos(np.deg2rad(18.0 + 0.25 * np.arange(145)))[:, None].astype(np.float32), 257, axis=1).astype(np.float64)
    sel = lab == 0
    assert abs(float(r['mean'][0, 0, 1]) - (w[sel] * x[sel]).sum() / w[sel].sum()) <= 2.0 ** -23 * 300.0


def test_the_launcher_runs_with_the_region_flags(tmp_path):
    _loop_model(tmp_path)
    np.save(tmp_path / 'labels.npy', _labels(145, 257))
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--regions', 'speed,T', '--region_labels', str(tmp_path / 'labels.npy'), '--region_weights', 'area',
                            '--region_threshold', 'T:280'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert "regions speed,T: mean (49, 5, 2), points counted" in child.stdout and "thresholds [('T', 280.0)]" in child.stdout
    assert len([fn for fn in os.listdir(tmp_path / 'cli') if '_region_' in fn]) == 8 * 2 + 1
