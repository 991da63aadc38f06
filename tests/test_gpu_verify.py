"""GPU (MI355X): forecast verification against observations -- dpn_verify_accumulate / dpn_verify_pool / dpn_verify_finish through VerifyState,
PackedField.verify_accumulate, InterfacePhysics.verify_at, run_inference_interface's `verify` key and infer.py --verify (hi+lo mode).

Yardsticks: deepphysinet_amd.verification's numpy restatement of the three kernels (bit for bit: all are compiled without contraction), fed with what
dpn_fields_out and dpn_diagnostics_out write for the same out_n (the forecast) and for coord_data in its place (the baseline); the exact tables and
the bound of tests/verify_cases.py; predict_points per case plus fp64 numpy on the stacked values.  Model, field, sampler, stations and the five
members (here: cases) are those of tests/test_gpu_ensemble.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import verify_cases as VC
from tests.test_gpu_diagnostics import _inputs, _loop_model, _physics_cases
from tests.test_gpu_ensemble import _kernel_inputs, _members, _single_rows
from tests.test_gpu_inference import _stations
from tests.test_gpu_parity import _dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [28, 29, 30, 31, 32, 33, 25, 26]                          # u v p T q rho speed rel_humidity
M_MAX = 5
_cache = {}


def _coord_data():
    """Per case the sampler's coord_data [1 037, 6] at the stations of seed 0: the baseline's input."""
    if 'cd' not in _cache:
        xi, yi, hr = _inputs()['stations']
        _cache['cd'] = [mem['sampler'].at_positions(xi, yi, hr)[3].contiguous() for mem in _members(M_MAX)]
    return _cache['cd']


def _sides(case):
    """(name, ph, clip, out_n list, coord_data list, x [5, 1 037, 8], b [5, 1 037, 8]) of a physics case: the kernel's inputs with their NaN points, and
    the forecast and baseline values in the order of IDS -- dpn_fields_out's and dpn_diagnostics_out's own rows of out_n, and of coord_data in its
    place with J = 0.  The last station lies outside the coarse cube in every case (out_n and coord_data NaN), station 1 031 in case 1 only, and
    the baseline of station 1 027 is missing in case 0."""
    key = ('sides', case)
    if key not in _cache:
        name, ph, clip = _physics_cases(_inputs())[case]
        outs, cds, xs, bs = [], [], [], []
        for m, ((o, j, f), cd) in enumerate(zip(_kernel_inputs(), _coord_data())):
            o, cd = o.clone(), cd.clone()
            o[-1], cd[-1] = float('nan'), float('nan')
            if m == 1:
                o[1031], cd[1031] = float('nan'), float('nan')
            if m == 0:
                cd[1027, 2] = float('nan')
            zero = torch.zeros_like(j)
            xs.append(_single_rows(o, zero, f, ph, clip)[:, IDS])
            bs.append(_single_rows(cd, zero, f, ph, clip)[:, IDS])
            outs.append(o)
            cds.append(cd)
        _cache[key] = (name, ph, clip, outs, cds, np.stack(xs), np.stack(bs))
    return _cache[key]


def _reports(x, seed=0):
    """Reports for forecast values x [M, n, P]: the forecast plus a biased noise of the column's own spread, a tenth of them missing, one infinite."""
    g = np.random.default_rng(seed)
    scale = np.nanstd(np.where(np.isfinite(x), x, np.nan).astype(np.float64), axis=(0, 1), keepdims=True) + 1e-30
    o = (x.astype(np.float64) + scale * (0.5 * g.standard_normal(x.shape) + 0.125)).astype(np.float32)
    o[g.random(x.shape) < 0.1] = np.nan
    o[0, 0, 0] = np.inf
    return o


def _thresholds(cols, x):
    """Two thresholds (above the column's median, below its lower quartile) on each of `cols`, one of them a value that occurs."""
    thr_col, thr_val, thr_side = [], [], []
    for c in cols:
        v = x[..., c][np.isfinite(x[..., c])]
        thr_col += [c, c]
        thr_val += [float(v[0]), float(np.float32(np.quantile(v, 0.25)))]
        thr_side += [0, 1]
    return thr_col, thr_val, thr_side


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _host(state):
    """The arrays of a VerifyState on the host, by the restatement's names (cont [E, 6, N]; an empty array without thresholds)."""
    P, N = state.n.shape
    out = {k: v.cpu().numpy() for k, v in state.arrays().items() if v is not None}
    out.setdefault('cont', np.zeros((0, 6, N), dtype=np.int32))
    return out


def _assert_state(state, want, what):
    got = _host(state)
    for key in want:
        assert _same(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())


def _assert_rows(rows, want, what):
    for key, w in want.items():
        if rows.get(key) is None:
            assert w.shape[1] == 0, (what, key)
            continue
        assert _same(rows[key].cpu().numpy(), w), (what, key)


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 300])
def test_kernels_are_the_restatement_bit_for_bit(n):
    """After every launch -- accumulate per case, pool, finish of points and of groups -- the state and the scores equal the restatement bit for bit.
    M = 1, 2, 5 cases; all eight products with six thresholds, and a short list with a repeat; reports with NaN and an infinity; a station outside
    the coarse cube in every case (count 0, all NaN) when n > 1, one outside in one case, a baseline that is missing once."""
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.point_path import VerifyState
    groups = {'thirds': np.arange(n) % 3 if n >= 3 else np.zeros(n, dtype=np.int64), 'all': np.zeros(n, dtype=np.int64),
              'own, reversed': np.arange(n)[::-1].copy(), 'gaps': (np.arange(n) % 2) * 4}
    for case in range(3):
        name, ph, clip, outs, cds, x_all, b_all = _sides(case)
        lo = 0 if n == 1 else 1037 - n                                     # n > 1: the last n stations, the one outside the cube among them
        for cols in (list(range(8)), [3, 6, 3]):
            ids = [IDS[c] for c in cols]
            x, b = x_all[:, lo:lo + n][:, :, cols], b_all[:, lo:lo + n][:, :, cols]
            o = _reports(x, seed=n + case)
            thr = _thresholds([0, 1, 2] if len(cols) > 3 else [0, 2], x) if n > 1 else ([], [], [])
            if n > 1:
                o[0, 0, thr[0][0]] = np.float32(thr[1][0])                 # a report that hits a threshold exactly
            for M in (1, 2, 5):
                st = VerifyState(n, ids, *thr, _dev())
                want = VF.verify_state_zeros(n, len(ids), len(thr[0]))
                for m in range(M):
                    st.accumulate(outs[m][lo:lo + n].contiguous(), cds[m][lo:lo + n].contiguous(), torch.from_numpy(np.ascontiguousarray(o[m])).to(_dev()),
                                  ph, 0, clip)
                    VF.verify_accumulate_reference(want, x[m], b[m], o[m], *thr)
                    _assert_state(st, want, (name, cols, M, m))
                _assert_rows(st.finish(), VF.verify_finish_reference(want, thr[0]), (name, cols, M, 'points'))
                if n > 1:
                    assert bool((st.n[:, -1] == 0).all()) and bool(torch.isnan(st.finish()['bias'][-1]).all())        # outside the cube
                for gname, g in groups.items():
                    plan = VF.pool_plan(g)
                    pooled = st.pool(*plan)
                    want_pool = VF.verify_pool_reference(want, *plan, thr[0])
                    _assert_state(pooled, want_pool, (name, cols, M, gname))
                    _assert_rows(pooled.finish(), VF.verify_finish_reference(want_pool, thr[0]), (name, cols, M, gname))


def _upload(case):
    """The restatement's point state of a hand-written case of tests/verify_cases.py, and the same numbers in a VerifyState on the device."""
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.point_path import VerifyState
    M, n, P = case['x'].shape
    thr = case['thr']
    host = VF.verify_state_zeros(n, P, len(thr[0]))
    for m in range(M):
        VF.verify_accumulate_reference(host, case['x'][m], case['b'][m], case['o'][m], *thr)
    st = VerifyState(n, [31] * P, *thr, _dev())
    for key, v in st.arrays().items():
        if v is not None:
            v.copy_(torch.from_numpy(host[key]))
    return host, st


def test_pool_and_finish_on_the_hand_written_tables():
    """The states of the exact tables, uploaded: segments of 1, 0, 63, 64, 65, 129 and 4 097 points in an interleaved order pool to the restatement's
    bits, the pooled scores meet the exact values within the bound, and the two order cases give the bias the header's fold order gives."""
    from deepphysinet_amd import verification as VF
    for name, case in VC.exact_cases().items():
        host, st = _upload(case)
        thr_col = case['thr'][0]
        _assert_rows(st.finish(), VF.verify_finish_reference(host, thr_col), (name, 'points'))
        plan = VF.pool_plan(case['groups'])
        pooled = st.pool(*plan)
        want = VF.verify_pool_reference(host, *plan, thr_col)
        _assert_state(pooled, want, (name, 'pooled'))
        rows = pooled.finish()
        _assert_rows(rows, VF.verify_finish_reference(want, thr_col), (name, 'pooled'))
        dev = VC.deviation({k: v.cpu().numpy() for k, v in rows.items() if v is not None}, VC.exact_of(name, True))
        print('%s: pooled on the device against the exact table %.3e (bound %.3e)' % (name, dev, VC.BOUND))
        assert dev <= VC.BOUND, (name, dev)
    assert np.diff(VF.pool_plan(VC.exact_cases()['layout']['groups'])[1]).tolist() == [1, 0, 63, 64, 65, 129, 4097]
    for name, case in VC.order_cases().items():
        host, st = _upload(case)
        rows = st.pool(*VF.pool_plan(case['groups'])).finish()
        assert VC.meets({k: v.cpu().numpy() for k, v in rows.items() if v is not None}, case['expect']), (name, rows['bias'], rows['count'])


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_two_runs_and_two_chunkings_give_the_same_bits():
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.point_path import VerifyState
    name, ph, clip, outs, cds, x, b = _sides(1)
    n, ids = 1037, IDS
    o = _reports(x, seed=9)
    thr = _thresholds([3, 6], x)
    obs = [torch.from_numpy(np.ascontiguousarray(o[m])).to(_dev()) for m in range(M_MAX)]
    plan = VF.pool_plan(np.arange(n) % 7)
    results = []
    for chunk in (n, n, 256, 100):
        st = VerifyState(n, ids, *thr, _dev())
        for m in range(M_MAX):
            for first in range(0, n, chunk):
                k = min(chunk, n - first)
                st.accumulate(outs[m][first:first + k], cds[m][first:first + k], obs[m][first:first + k], ph, first, clip)
        pooled = st.pool(*plan)
        results.append((_host(st), _host(pooled), {k: v.cpu().numpy() for k, v in pooled.finish().items()}))
    for other in results[1:]:
        for a, c in zip(results[0], other):
            for key in a:
                assert _same(a[key], c[key]), key
    st.clear()
    assert not bool(st.buffer.any())                                       # one memset clears the whole state


# ------------------------------------------------------------------------------------------------ 3. refusals
CANARY = 0xA5


def _raw_state(n_total, P, E):
    """A canary-filled state as plain tensors by DpnVerifyState's names."""
    from deepphysinet_amd import verification as VF
    dev = _dev()
    fill = lambda shape, dt: torch.full(shape, CANARY, dtype=torch.uint8, device=dev).repeat_interleave(torch.empty((), dtype=dt).element_size()) \
        .view(dt).view(shape)
    st = {'n': fill((P, n_total), torch.int32), 'max_ad': fill((P, n_total), torch.float32), 'cont': fill((max(E, 1), 6, n_total), torch.int32)}
    st.update({k: fill((P, n_total), torch.float64) for k in VF.STATE_F64})
    return st


def _c_state(st, drop=()):
    from deepphysinet_amd import verification as VF
    from deepphysinet_amd.point_path import _ptr
    return VF.DpnVerifyState(*[None if k in drop else _ptr(st[k]) for k in VF.STATE_FIELDS])


def _arr(v, t):
    return None if v is None else (t * max(len(v), 1))(*v)


def _accumulate(st, out_n, cd, obs, n, ph, clip=0, ids=(31, 25), thr_col=(0, 1), thr_val=(280.0, 0.5), thr_side=(1, 0), n_thr=None, first=0,
                n_total=None, drop=(), no_state=False):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    return L.load().dpn_verify_accumulate(_ptr(out_n), _ptr(cd), _ptr(obs), n, None if ph is None else ctypes.byref(ph), clip, _arr(ids, ctypes.c_int32),
                                          0 if ids is None else len(ids), _arr(thr_col, ctypes.c_int32), _arr(thr_val, ctypes.c_float),
                                          _arr(thr_side, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, first,
                                          st['n'].shape[1] if n_total is None else n_total, None if no_state else ctypes.byref(_c_state(st, drop)),
                                          _stream())


def _finish(st, rows, first=0, n=None, n_total=None, n_products=2, thr_col=(0, 1), n_thr=None, drop=(), no_state=False, no_rows=False):
    from deepphysinet_amd import _lib as L, verification as VF
    from deepphysinet_amd.point_path import _ptr, _stream
    table = L.DpnVerifyOut(*[None if k in drop else _ptr(rows[k]) for k in VF.OUT_FIELDS])
    N = st['n'].shape[1]
    return L.load().dpn_verify_finish(None if no_state else ctypes.byref(_c_state(st, drop)), N if n_total is None else n_total, n_products,
                                      _arr(thr_col, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, first,
                                      N if n is None else n, None if no_rows else ctypes.byref(table), _stream())


def _pool(src, dst, order, seg_dev, seg_host, n_points=None, n_groups=None, n_products=2, thr_col=(0, 1), n_thr=None, drop_src=(), drop_dst=(),
          no_src=False, no_dst=False):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    host = None if seg_host is None else (ctypes.c_int64 * len(seg_host))(*seg_host)
    return L.load().dpn_verify_pool(None if no_src else ctypes.byref(_c_state(src, drop_src)), src['n'].shape[1] if n_points is None else n_points,
                                    _ptr(order), _ptr(seg_dev), host, dst['n'].shape[1] if n_groups is None else n_groups, n_products,
                                    _arr(thr_col, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr,
                                    None if no_dst else ctypes.byref(_c_state(dst, drop_dst)), _stream())


def _untouched(tensors):
    return all(bool((v.contiguous().view(torch.uint8) == CANARY).all()) for v in tensors.values() if v is not None)


def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import verification as VF
    I = _inputs()
    n = 300
    ph = I['cfg'].physics()
    out_n, cd = _kernel_inputs()[0][0][:n].contiguous(), _coord_data()[0][:n].contiguous()
    obs = torch.zeros((n, 2), dtype=torch.float32, device=_dev())
    st = _raw_state(n, 2, 2)
    ok = dict(out_n=out_n, cd=cd, obs=obs, n=n, ph=ph)
    nan, inf = float('nan'), float('inf')
    cases = [dict(out_n=None), dict(cd=None), dict(obs=None), dict(ph=None), dict(ids=None), dict(no_state=True), dict(n=0), dict(n=-3), dict(first=-1),
             dict(first=1), dict(n_total=n - 1), dict(n_total=0), dict(ids=[]), dict(ids=[31] * 17), dict(ids=[31, 18]), dict(ids=[27, 25]),
             dict(ids=[31, 34]), dict(ids=[-1, 25]), dict(ids=[0, 25]), dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=[-1, 1]),
             dict(thr_side=[1, 2]), dict(thr_side=[-1, 0]), dict(thr_val=[280.0, nan]), dict(thr_val=[inf, 0.5]), dict(thr_val=[280.0, -inf]),
             dict(thr_col=None, n_thr=2), dict(thr_val=None, n_thr=2), dict(thr_side=None, n_thr=2)] + [dict(drop=(k,)) for k in VF.STATE_FIELDS]
    for case in cases:
        assert _accumulate(st, **{**ok, **case}) == -1, sorted(case)
    rows = {'count': torch.full((n, 2), CANARY, dtype=torch.uint8, device=_dev()).repeat_interleave(4).view(torch.int32).view(n, 2)}
    rows.update({k: torch.full((n, 2), CANARY, dtype=torch.uint8, device=_dev()).repeat_interleave(4).view(torch.float32).view(n, 2)
                 for k in VF.SCORES + VF.THRESHOLD_SCORES})
    cases = [dict(no_state=True), dict(no_rows=True), dict(n=0), dict(n=-1), dict(first=-1), dict(first=1), dict(n_total=n - 1), dict(n_total=0),
             dict(n_products=0), dict(n_products=17), dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=[-1, 0]), dict(thr_col=None, n_thr=2)] + \
            [dict(drop=(k,)) for k in VF.STATE_FIELDS + VF.OUT_FIELDS]
    for case in cases:
        assert _finish(st, rows, **case) == -1, sorted(case)
    G = 3
    dst = _raw_state(G, 2, 2)
    order = torch.arange(n, dtype=torch.int32, device=_dev())
    seg = [0, 100, 100, n]
    seg_dev = torch.tensor(seg, dtype=torch.int64, device=_dev())
    good = dict(order=order, seg_dev=seg_dev, seg_host=seg)
    cases = [dict(order=None), dict(seg_dev=None), dict(seg_host=None), dict(no_src=True), dict(no_dst=True), dict(n_points=0), dict(n_points=-1),
             dict(n_groups=0), dict(n_groups=-2), dict(seg_host=[1, 100, 100, n]), dict(seg_host=[0, 100, 99, n]), dict(seg_host=[0, 100, 100, n - 1]),
             dict(seg_host=[0, 100, 100, n + 1]), dict(seg_host=[0, n + 5, 100, n]), dict(n_products=0), dict(n_products=17), dict(n_thr=17),
             dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=None, n_thr=2)] + \
            [dict(drop_src=(k,)) for k in VF.STATE_FIELDS] + [dict(drop_dst=(k,)) for k in VF.STATE_FIELDS]
    for case in cases:
        assert _pool(st, dst, **{**good, **case}) == -1, sorted(case)
    torch.cuda.synchronize()
    assert _untouched(st) and _untouched(dst) and _untouched(rows)
    # and the same arguments, accepted (without thresholds cont and the threshold destinations may be NULL)
    for key in st:
        st[key].zero_()
    assert _accumulate(st, **ok) == 0 and _finish(st, rows) == 0 and _pool(st, dst, **good) == 0
    assert _accumulate(st, **ok, thr_col=[], thr_val=[], thr_side=[], drop=('cont',)) == 0
    assert _finish(st, rows, thr_col=[], drop=('cont',) + VF.THRESHOLD_SCORES) == 0
    assert _pool(st, dst, **good, thr_col=[], drop_src=('cont',), drop_dst=('cont',)) == 0
    torch.cuda.synchronize()
    assert bool((st['n'] == 2).all()) and dst['n'][:, 1].tolist() == [0, 0] and dst['n'][:, 2].tolist() == [400, 400]
    assert bool((rows['count'] == 2).all())


# ------------------------------------------------------------------------------------------------ 4. the composed route
def _numpy_scores(x, b, o, thr, groups=None):
    """fp64 numpy on stacked values x, b, o [M, N, P]: the scores per point (or per group, the pairs pooled), two-pass."""
    M, N, P = x.shape
    groups = np.arange(N) if groups is None else np.asarray(groups)
    G, E = int(groups.max()) + 1, len(thr[0])
    out = {k: np.full((G, P), np.nan) for k in VC.SCORES}
    out['count'] = np.zeros((G, P), dtype=np.int32)
    out.update({pre + k: np.full((G, E), np.nan, dtype=np.float32) for pre in ('', 'base_') for k in VC.TABLE})
    ok = np.isfinite(x) & np.isfinite(b) & np.isfinite(o)
    for g in range(G):
        pts = groups == g
        for j in range(P):
            sel = ok[:, pts, j]
            X, B, O = (v[:, pts, j][sel].astype(np.float64) for v in (x, b, o))
            c = X.size
            out['count'][g, j] = c
            for e in range(E):
                if thr[0][e] != j:
                    continue
                ev = (lambda z: z > np.float32(thr[1][e])) if thr[2][e] == 0 else (lambda z: z < np.float32(thr[1][e]))
                eo = ev(o[:, pts, j][sel])
                for pre, side in (('', x), ('base_', b)):
                    ef = ev(side[:, pts, j][sel])
                    h, f, m_ = float((ef & eo).sum()), float((ef & ~eo).sum()), float((~ef & eo).sum())
                    with np.errstate(divide='ignore', invalid='ignore'):
                        hr = np.float64((h + f) * (h + m_)) / np.float64(c)
                        vals = [np.float64(h) / (h + m_), np.float64(f) / (h + f), np.float64(h) / ((h + f) + m_), np.float64(h + f) / (h + m_),
                                (h - hr) / (((h + f) + m_) - hr)]
                    for key, v in zip(VC.TABLE, vals):
                        out[pre + key][g, e] = np.float32(v) if np.isfinite(v) else np.nan
            if c == 0:
                continue
            d, e_ = X - O, B - O
            out['bias'][g, j], out['mae'][g, j], out['rmse'][g, j] = d.mean(), np.abs(d).mean(), np.sqrt((d * d).mean())
            out['max_abs_error'][g, j] = np.abs(d).max()
            out['base_bias'][g, j], out['base_mae'][g, j], out['base_rmse'][g, j] = e_.mean(), np.abs(e_).mean(), np.sqrt((e_ * e_).mean())
            if (e_ * e_).sum() != 0:
                out['skill'][g, j] = 1.0 - (d * d).sum() / (e_ * e_).sum()
            if c > 1 and X.std() != 0 and O.std() != 0:
                out['corr'][g, j] = ((X - X.mean()) * (O - O.mean())).sum() / np.sqrt(((X - X.mean()) ** 2).sum() * ((O - O.mean()) ** 2).sum())
    return out


def _baseline_rows(sampler, xi, yi, hr, ph, clip):
    """[N, 6]: the interpolated coarse forecast at the stations, de-normalised by dpn_fields_out."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    cd = sampler.at_positions(xi, yi, hr)[3].contiguous()
    rows = torch.empty_like(cd)
    assert L.load().dpn_fields_out(_ptr(cd), cd.shape[0], ctypes.byref(ph), int(clip), _ptr(rows), None, None, 0, _stream()) == 0
    return rows.cpu().numpy()


def _with_speed(rows):
    from deepphysinet_amd.diagnostics import diagnostics_reference
    n = rows.shape[0]
    speed = diagnostics_reference(rows, np.zeros((n, 6, 3), np.float32), np.zeros(n, np.float32), ['speed'], np.float32)
    return np.concatenate([rows[:, [3, 0, 2]], speed], axis=1)                                   # T, u, p, speed


def test_verify_at_against_predict_points_and_numpy():
    """verify_at against predict_points per case (the baseline: dpn_fields_out on the sampler's coord_data) + fp64 numpy on the stacked values: the
    scores within the CPU test's bound, counts and contingency scores exactly; with and without the clip, five cases and one, three groupings,
    positions in degrees, a chunked walk."""
    I = _inputs()
    m = I['m']
    N = 300
    xi, yi, hr = _stations(N, seed=5)
    names = ['T', 'u', 'p', 'speed']
    by = {'station': np.arange(N) % 37, 'hour': np.floor(hr / 6.0).astype(np.int64), 'all': np.zeros(N, dtype=np.int64)}
    ph = I['cfg'].physics()
    for clip, M in ((False, 5), (True, 2), (False, 1)):
        cases = _members(M)
        x = np.stack([_with_speed(m.predict_points(c['field_data'], c['sampler'], xi, yi, hr, c['forecast_h'], with_clip=clip).cpu().numpy()) for c in cases])
        b = np.stack([_with_speed(_baseline_rows(c['sampler'], xi, yi, hr, ph, clip)) for c in cases])
        o = _reports(x, seed=31 + M)
        thresholds = {'T': [('below', float(np.nanmedian(x[..., 0]))), float(np.nanquantile(x[..., 0], 0.75))], 'speed': float(np.nanmedian(x[..., 3]))}
        thr = ([0, 0, 3], [float(np.float32(thresholds['T'][0][1])), float(np.float32(thresholds['T'][1])), float(np.float32(thresholds['speed']))], [1, 0, 0])
        with_obs = [dict(c, obs=torch.from_numpy(np.ascontiguousarray(o[k])).to(_dev())) for k, c in enumerate(cases)]
        got = m.verify_at(with_obs, xi, yi, hr, names, thresholds=thresholds, by=by, with_clip=clip)
        assert got['names'] == names and got['thresholds'] == [('T', 'below', thr[1][0]), ('T', 'above', thr[1][1]), ('speed', 'above', thr[1][2])]
        assert sorted(got) == sorted(['names', 'thresholds', 'point', 'station', 'hour', 'all'])
        for key, groups in [('point', None)] + list(by.items()):
            want = _numpy_scores(x, b, o, thr, groups)
            table = {k: v.cpu().numpy() for k, v in got[key].items()}
            assert np.array_equal(table['count'], want['count']), (clip, M, key)
            for k in VC.TABLE:
                for pre in ('', 'base_'):
                    assert np.array_equal(table[pre + k], want[pre + k], equal_nan=True), (clip, M, key, pre + k)
            dev = VC.deviation(table, {k: want[k] for k in VC.SCORES})
            print('clip %s, %d cases, %s: worst relative deviation %.3e (bound %.3e)' % (clip, M, key, dev, VC.BOUND))
            assert dev <= VC.BOUND, (clip, M, key, dev)
        assert got['point']['count'].shape == (N, 4) and got['station']['bias'].shape == (37, 4) and got['hour']['pod'].shape == (4, 3)
        assert got['all']['count'].shape == (1, 4) and int(got['all']['count'][0, 0]) == int(got['point']['count'][:, 0].sum())
    # one case, no thresholds, no grouping
    alone = m.verify_at([dict(c, obs=c['obs'][:, :1].contiguous()) for c in with_obs], xi, yi, hr, ['T'])
    assert sorted(alone) == ['names', 'point', 'thresholds'] and alone['thresholds'] == [] and alone['point']['pod'] is None
    assert torch.equal(alone['point']['count'][:, 0], got['point']['count'][:, 0]) and bool(torch.isnan(alone['point']['corr']).all())
    # degrees: the same bits as the index units they convert to; a chunked walk: the same bits as the whole
    cfg = cases[0]['sampler'].cfg
    lon, lat = cfg.begin_lon + xi * cfg.out_res_deg, cfg.begin_lat + yi * cfg.out_res_deg
    index = m.verify_at(with_obs, *cases[0]['sampler'].lonlat_to_index(lon, lat), hr, names, thresholds=thresholds, by=by)
    degrees = m.verify_at(with_obs, lon, lat, hr, names, thresholds=thresholds, by=by, lonlat=True)
    m.chunk_size = lambda *a, **k: 128
    try:
        chunked = m.verify_at(with_obs, *cases[0]['sampler'].lonlat_to_index(lon, lat), hr, names, thresholds=thresholds, by=by)
    finally:
        del m.chunk_size
    for other in (degrees, chunked):
        for key in ('point', 'station', 'hour', 'all'):
            for k, v in index[key].items():
                assert _same(v.cpu().numpy(), other[key][k].cpu().numpy()), (key, k)


# ------------------------------------------------------------------------------------------------ 5. loop and launcher
def _report_file(path, M, names=('T', 'speed', 'q')):
    g = np.random.default_rng(17)
    S, H = 5, 4
    d = dict(lon=74.0 + g.random(S) * 60.0, lat=19.0 + g.random(S) * 34.0, hours=np.array([0.0, 6.0, 13.5, 24.0]), names=np.array(names),
             obs=(g.standard_normal((M, H, S, len(names))) * np.array([5.0, 2.0, 1e-3]) + np.array([280.0, 3.0, 5e-3])).astype(np.float32))
    d['obs'][0, 1, 2, :] = np.nan
    np.savez(path, **d)
    return d


def test_loop_writes_the_tables_and_leaves_the_rest_alone(tmp_path):
    from deepphysinet_amd.verification import OUT_FIELDS
    plain, with_key = tmp_path / 'plain', tmp_path / 'verify'
    _report_file(tmp_path / 'reports.npz', M=2)
    m = _loop_model(tmp_path, write_source=True, result_path=str(plain), export_variable=['T'])
    ref = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
    assert m.last_verification is None
    m = _loop_model(tmp_path, write_source=True, result_path=str(with_key), export_variable=['T'])
    option = dict(products=['speed', 'T'], obs=str(tmp_path / 'reports.npz'), thresholds={'T': ('below', 280.0), 'speed': [3.0]}, by=['station', 'hour', 'all'])
    maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2, verify=option)
    assert torch.equal(maps, ref)                                          # the return value is unchanged
    for fn in sorted(os.listdir(plain)):                                   # ... and so are the per-sample files
        assert np.array_equal(np.load(plain / fn), np.load(with_key / fn)), fn
    v = m.last_verification
    assert v['names'] == ['speed', 'T'] and v['thresholds'] == [('speed', 'above', 3.0), ('T', 'below', 280.0)]
    assert v['point']['bias'].shape == (20, 2) and v['station']['bias'].shape == (5, 2) and v['hour']['pod'].shape == (4, 2) and v['all']['count'].shape == (1, 2)
    count = v['point']['count'].cpu().numpy().reshape(4, 5, 2)             # point i = h * S + s
    assert count[1, 2].tolist() == [1, 1] and int(count.sum()) == 2 * 20 * 2 - 2 and bool(torch.isfinite(v['all']['skill']).all())
    assert v['hour']['count'].cpu().numpy().tolist() == count.sum(axis=1).tolist() and v['station']['count'].cpu().numpy().tolist() == count.sum(axis=0).tolist()
    new = sorted(fn for fn in os.listdir(with_key) if '_verify_' in fn)
    assert len(new) == 4 * len(OUT_FIELDS) and len(os.listdir(with_key)) == len(os.listdir(plain)) + len(new)
    stamp = sorted(os.listdir(plain))[0][:-len('_T.npy')]                  # the first sample's first time step
    for group in ('point', 'station', 'hour', 'all'):
        for key in OUT_FIELDS:
            assert np.array_equal(np.load(with_key / ('%s_verify_%s_%s.npy' % (stamp, group, key))), v[group][key].cpu().numpy(), equal_nan=True), (group, key)
    with pytest.raises(ValueError, match='hold 2 cases, the sample source 1'):
        m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', verify=option)


def test_the_launcher_runs_with_the_verify_flags(tmp_path):
    _loop_model(tmp_path)
    _report_file(tmp_path / 'reports.npz', M=1)
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--verify', 'T,speed', '--verify_obs', str(tmp_path / 'reports.npz'), '--verify_threshold', 'T:below:280',
                            '--verify_by', 'station,all'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert "verification T,speed: point (20, 2), pairs counted 0..1, groupings ['station', 'all'], thresholds [('T', 'below', 280.0)]" in child.stdout
    refused = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--synthetic', '--verify', 'T'], cwd=ROOT, capture_output=True, text=True,
                             timeout=600)
    assert refused.returncode == 2 and 'nothing to verify against' in refused.stderr
