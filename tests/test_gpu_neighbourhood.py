"""GPU (MI355X): neighbourhood verification on lattices -- dpn_nbhd_stage / dpn_nbhd_fold / dpn_nbhd_finish through NbhdState,
PackedField.nbhd_stage, InterfacePhysics.verify_lattice, run_inference_interface's `verify_grid` key and infer.py --verify_grid (hi+lo mode).

Yardsticks: deepphysinet_amd.neighbourhood's numpy restatement of the kernels (bit for bit: all are compiled without contraction), fed with what
dpn_fields_out and dpn_diagnostics_out write for the same out_n (the forecast) and for coord_data in its place (the baseline); predict_lattice per
case plus fp64 numpy brute force over the windows, with the bound of tests/neighbourhood_cases.py; verify_at on the same nodes.  Model, field,
sampler and cases are those of tests/test_gpu_verify.py; a lattice's nodes take their rows from the 1 037 stations of seed 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import neighbourhood_cases as NC
from tests.test_gpu_diagnostics import _inputs, _loop_model
from tests.test_gpu_ensemble import _members
from tests.test_gpu_parity import _dev
from tests.test_gpu_verify import IDS, _sides, _with_speed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lattice(nx, ny, nt):
    from deepphysinet_amd.sampler import Lattice
    return Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, nx, ny, nt)


def _node_rows(n):
    """The station row of every lattice node: from station 1 027 (its baseline is missing in case 0) in steps of 9, so station 1 036 (outside the
    coarse cube in every case: forecast and baseline NaN) is node 1 and every station comes up on a lattice of 1 037 nodes or more."""
    return (1027 + 9 * np.arange(n)) % 1037


def _case_inputs(lat, cols, m, physics=0, seed=0):
    """(out_n, coord_data [n, 6] on the device, ph, clip, x, b, o [nt, P, ny, nx] float32) of case m on `lat`: the kernel's inputs and the values
    dpn_fields_out / dpn_diagnostics_out write for them, the analysis x plus noise with a tenth of the nodes missing and one infinite."""
    _, ph, clip, outs, cds, x_all, b_all = _sides(physics)
    idx = _node_rows(lat.n_points)
    planes = lambda v: np.ascontiguousarray(v[m][idx][:, cols].reshape(lat.nt, lat.ny, lat.nx, len(cols)).transpose(0, 3, 1, 2))
    x, b = planes(x_all), planes(b_all)
    g = np.random.default_rng(1000 * seed + m)
    scale = np.nanstd(np.where(np.isfinite(x), x, np.nan).astype(np.float64), axis=(0, 2, 3), keepdims=True) + 1e-30
    o = (np.nan_to_num(x).astype(np.float64) + scale * (0.7 * g.standard_normal(x.shape) + 0.1)).astype(np.float32)
    o[g.random(o.shape) < 0.1] = np.nan
    o.reshape(-1)[o.size // 2] = np.inf
    t = torch.from_numpy(idx).to(_dev())
    return outs[m][t].contiguous(), cds[m][t].contiguous(), ph, clip, x, b, o


def _thresholds(E, x, P):
    """E thresholds spread over the P columns, sides alternating, at quantiles of the column's values; the first is a value that occurs."""
    thr_col, thr_val, thr_side = [], [], []
    for e in range(E):
        j = e % P
        v = x[:, j][np.isfinite(x[:, j])]
        thr_col.append(j)
        thr_val.append(float(v[0]) if e == 0 else float(np.float32(np.quantile(v, 0.2 + 0.6 * ((e * 7) % 16) / 16.0))))
        thr_side.append(e % 2)
    order = np.argsort(thr_col, kind='stable')                            # (check_thresholds' order: by column)
    return [thr_col[i] for i in order], [thr_val[i] for i in order], [thr_side[i] for i in order]


def _new_state(lat, ids, thr, radius, budget=64 << 20):
    from deepphysinet_amd.point_path import NbhdState
    return NbhdState(lat, ids, *thr, radius, _dev(), budget)


def _host(state):
    return {k: v.cpu().numpy() for k, v in state.arrays().items()}


def _stage(state, out_n, cd, o_dev, ph, clip, chunk):
    n = out_n.shape[0]
    for first in range(0, n, chunk):
        state.stage(out_n[first:first + chunk], cd[first:first + chunk], o_dev, ph, first, clip)


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
SHAPES = [(1, 1), (5, 3), (63, 64), (64, 65), (65, 70), (130, 3), (130, 70), (1, 70), (64, 1), (5, 65)]


@pytest.mark.parametrize('nx,ny', SHAPES)
def test_kernels_are_the_restatement_bit_for_bit(nx, ny):
    """After every launch -- stage (three chunkings, two of them beginning and ending inside a row), fold, finish -- the mask bytes, the table S and
    the row partials read back from the scratch, the state after every case and the tables equal the restatement bit for bit.  nt = 1 with E = 1,
    K = 1 and nt = 3 with E = 16, K = 8; r out of 0, 1, 2, 7, max(nx, ny) and beyond; NaN analysis nodes, a node outside the coarse cube, a missing
    baseline, and in the second case an hour whose first column has no valid node."""
    from deepphysinet_amd import neighbourhood as NB
    big = max(nx, ny)
    which = SHAPES.index((nx, ny))
    for nt, E, radius, cols, physics in ((1, 1, [[0], [1], [2], [7], [big]][which % 5], [3], which % 3),
                                         (3, 16, [0, 1, 2, 3, 7, big + 7, big + 8, 2 * big + 50], [0, 3, 6, 7, 3], (which + 1) % 3)):
        lat = _lattice(nx, ny, nt)
        ids = [IDS[c] for c in cols]
        n, K = lat.n_points, len(radius)
        x0 = _case_inputs(lat, cols, 0, physics, seed=which)[4]
        thr = _thresholds(E, x0, len(cols))
        st = _new_state(lat, ids, thr, radius)
        assert st.planes_per_fold == nt * E
        want = NB.nbhd_state_zeros(nt, E, K)
        for m in range(2):
            out_n, cd, ph, clip, x, b, o = _case_inputs(lat, cols, m, physics, seed=which)
            if m == 1 and nt == 3:
                o[0, 0] = np.nan
            o_dev = torch.from_numpy(o).to(_dev())
            mask = NB.nbhd_stage_reference(x, b, o, thr)
            for chunk in (n, max(1, (n * 2) // 5 + 1), 37):
                st.mask.fill_(CANARY)
                _stage(st, out_n, cd, o_dev, ph, clip, chunk)
                assert _same(st.mask.cpu().numpy(), mask), (nt, m, chunk)
            st.fold()
            S, part, rows = NB.nbhd_fold_reference(want, mask, radius)
            got = [v.cpu().numpy() for v in st.scratch_views(nt * E)]
            assert _same(got[0], S), (nt, m, 'S', np.argwhere(got[0] != S)[:4].tolist())
            assert _same(got[1], part) and _same(got[2], rows), (nt, m, 'row partials')
            for key, v in _host(st).items():
                assert _same(v, want[key]), (nt, m, key)
            if m == 0:
                after_first = want['n_valid'].copy()
            elif nt == 3:                                                  # no valid node in this case: the plane's totals are the first case's
                assert int(mask[0, 0].max()) == 0 and int(want['n_valid'][0, 0]) == int(after_first[0, 0])
        tables = st.finish()
        ref = NB.nbhd_finish_reference(want)
        for group in ('hour', 'all'):
            for key in NB.OUT_FIELDS:
                assert _same(tables[group][key].cpu().numpy(), ref[group][key]), (nt, group, key)


def test_a_plane_without_a_valid_node_scores_nan():
    from deepphysinet_amd import neighbourhood as NB
    lat = _lattice(9, 7, 2)
    out_n, cd, ph, clip, x, b, o = _case_inputs(lat, [3], 0)
    o[1] = np.nan
    thr = ([0], [float(np.nanmedian(x))], [0])
    st = _new_state(lat, [31], thr, [0, 2])
    _stage(st, out_n, cd, torch.from_numpy(o).to(_dev()), ph, clip, lat.n_points)
    st.fold()
    t = {g: {k: v.cpu().numpy() for k, v in tab.items()} for g, tab in st.finish().items()}
    assert t['hour']['count'][1, 0] == 0 and t['hour']['windows'][1].tolist() == [[0, 0]] and t['hour']['skilful_scale'][1, 0] == -1
    for key in ('fss', 'base_fss', 'freq_f', 'freq_o', 'fbias', 'useful'):
        assert bool(np.isnan(t['hour'][key][1]).all()) and bool(np.isfinite(t['hour'][key][0]).all()), key
    for key in NB.OUT_FIELDS:                                              # the hour without nodes adds nothing to the table over all hours
        assert _same(t['all'][key][0], t['hour'][key][0, 0]), key


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_plane_batches_chunkings_and_a_second_run_give_the_same_bits():
    lat = _lattice(65, 33, 3)
    cols, radius = [3, 6], [0, 1, 4, 40]
    ids = [IDS[c] for c in cols]
    inputs = [_case_inputs(lat, cols, m, 1) for m in range(2)]
    thr = _thresholds(4, inputs[0][4], 2)
    results = []
    for planes, chunk in ((None, lat.n_points), (None, lat.n_points), (1, 1000), (2, 100), (5, 129)):
        st = _new_state(lat, ids, thr, radius)
        for out_n, cd, ph, clip, x, b, o in inputs:
            _stage(st, out_n, cd, torch.from_numpy(o).to(_dev()), ph, clip, chunk)
            st.fold(planes)
        tables = st.finish()
        results.append((st.buffer.cpu().numpy(), {g + k: v.cpu().numpy() for g, t in tables.items() for k, v in t.items()}))
    for buf, tables in results[1:]:
        assert _same(buf, results[0][0])
        for key, v in tables.items():
            assert _same(v, results[0][1][key]), key
    assert bool(st.buffer.any())
    st.clear()
    assert not bool(st.buffer.any())                                       # one memset clears the whole state


# ------------------------------------------------------------------------------------------------ 3. refusals
def _fill(shape, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((int(np.prod(shape)) * size,), CANARY, dtype=torch.uint8, device=_dev()).view(dtype).view(shape)


def _untouched(tensors):
    return all(bool((v.contiguous().view(-1).view(torch.uint8) == CANARY).all()) for v in tensors)


def _arr(v, t):
    return None if v is None else (t * max(len(v), 1))(*v)


def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import _lib as L, neighbourhood as NB
    from deepphysinet_amd.point_path import NbhdState, _ptr, _stream
    lib = L.load()
    nx, ny, nt, P, E, K = 7, 5, 2, 2, 2, 2
    lat = _lattice(nx, ny, nt)
    n = lat.n_points
    out_n, cd, ph, clip, x, b, o = _case_inputs(lat, [3, 6], 0)
    an = torch.from_numpy(o).to(_dev())
    state = {k: _fill((nt, E, K) if k in NB.SUMS + ('windows',) else (nt, E), torch.float64 if k in NB.SUMS else torch.int64) for k in NB.STATE_FIELDS}
    mask = _fill((nt, E, ny, nx), torch.uint8)
    scratch = _fill((NbhdState.scratch_bytes(nx, ny, K, nt * E),), torch.uint8)
    hour = {k: _fill((nt, E, K) if k in NB.SCALE_FIELDS else (nt, E), getattr(torch, np.dtype(NB.OUT_DTYPES[k]).name)) for k in NB.OUT_FIELDS}
    every = {k: _fill((E, K) if k in NB.SCALE_FIELDS else (E,), getattr(torch, np.dtype(NB.OUT_DTYPES[k]).name)) for k in NB.OUT_FIELDS}
    c_lat = lambda **kw: lat.c_struct() if not kw else L.DpnLattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, kw.get('nx', nx), kw.get('ny', ny), kw.get('nt', nt))
    c_state = lambda drop=(): NB.DpnNbhdState(*[None if k in drop else _ptr(state[k]) for k in NB.STATE_FIELDS])
    c_out = lambda t, drop=(): NB.DpnNbhdOut(*[None if k in drop else _ptr(t[k]) for k in NB.OUT_FIELDS])

    def stage(out_n=out_n, cd=cd, an=an, n=n, ph=ph, ids=(31, 25), thr_col=(0, 1), thr_val=(280.0, 0.5), thr_side=(1, 0), n_thr=None, lattice=True,
              first=0, mask=mask, **dims):
        return lib.dpn_nbhd_stage(_ptr(out_n), _ptr(cd), _ptr(an), n, None if ph is None else ctypes.byref(ph), 0, _arr(ids, ctypes.c_int32),
                                  0 if ids is None else len(ids), _arr(thr_col, ctypes.c_int32), _arr(thr_val, ctypes.c_float),
                                  _arr(thr_side, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr,
                                  ctypes.byref(c_lat(**dims)) if lattice else None, first, _ptr(mask), _stream())

    def fold(mask=mask, lattice=True, n_thr=E, radius=(0, 2), n_scales=None, p0=0, planes=nt * E, scratch=scratch, drop=(), no_state=False, **dims):
        return lib.dpn_nbhd_fold(_ptr(mask), ctypes.byref(c_lat(**dims)) if lattice else None, n_thr, _arr(radius, ctypes.c_int32),
                                 (0 if radius is None else len(radius)) if n_scales is None else n_scales, p0, planes, _ptr(scratch),
                                 None if no_state else ctypes.byref(c_state(drop)), _stream())

    def finish(nt_=nt, n_thr=E, n_scales=K, drop=(), drop_hour=(), drop_all=(), no_state=False, no_hour=False, no_all=False):
        return lib.dpn_nbhd_finish(None if no_state else ctypes.byref(c_state(drop)), nt_, n_thr, n_scales,
                                   None if no_hour else ctypes.byref(c_out(hour, drop_hour)), None if no_all else ctypes.byref(c_out(every, drop_all)),
                                   _stream())

    nan, inf = float('nan'), float('inf')
    for case in [dict(out_n=None), dict(cd=None), dict(an=None), dict(ph=None), dict(ids=None), dict(mask=None), dict(lattice=False), dict(n=0), dict(n=-3),
                 dict(first=-1), dict(first=1), dict(n=n + 1), dict(ids=[]), dict(ids=[31] * 17), dict(ids=[31, 18]), dict(ids=[27, 25]), dict(ids=[31, 34]),
                 dict(thr_col=[], thr_val=[], thr_side=[]), dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=[-1, 1]),
                 dict(thr_side=[1, 2]), dict(thr_side=[-1, 0]), dict(thr_val=[280.0, nan]), dict(thr_val=[inf, 0.5]), dict(thr_col=None, n_thr=2),
                 dict(thr_val=None, n_thr=2), dict(thr_side=None, n_thr=2), dict(nx=0), dict(ny=0), dict(nt=0), dict(nx=2 ** 16, ny=2 ** 15, nt=1),
                 dict(nx=2 ** 11, ny=2 ** 10, nt=2 ** 10)]:
        assert stage(**case) == -1, sorted(case)
    for case in [dict(mask=None), dict(scratch=None), dict(lattice=False), dict(no_state=True), dict(n_thr=0), dict(n_thr=17), dict(radius=None, n_scales=2),
                 dict(radius=[]), dict(radius=list(range(9))), dict(radius=[-1, 2]), dict(radius=[2, 2]), dict(radius=[3, 1]), dict(nx=0), dict(ny=0),
                 dict(nt=0), dict(nx=2 ** 16, ny=2 ** 15, nt=1), dict(p0=-1), dict(planes=0), dict(planes=-1), dict(p0=1), dict(planes=nt * E + 1),
                 dict(p0=nt * E, planes=1)] + [dict(drop=(k,)) for k in NB.STATE_FIELDS]:
        assert fold(**case) == -1, sorted(case)
    for case in [dict(no_state=True), dict(no_hour=True), dict(no_all=True), dict(nt_=0), dict(n_thr=0), dict(n_thr=17), dict(n_scales=0), dict(n_scales=9)] \
            + [dict(drop=(k,)) for k in NB.STATE_FIELDS] + [dict(drop_hour=(k,)) for k in NB.OUT_FIELDS] + [dict(drop_all=(k,)) for k in NB.OUT_FIELDS]:
        assert finish(**case) == -1, sorted(case)
    torch.cuda.synchronize()
    assert _untouched(list(state.values()) + [mask, scratch] + list(hour.values()) + list(every.values()))
    # and the same arguments, accepted
    for v in state.values():
        v.zero_()
    assert stage() == 0 and fold() == 0 and fold(p0=1, planes=2) == 0 and finish() == 0
    torch.cuda.synchronize()
    want = NB.nbhd_state_zeros(nt, E, K)
    m = NB.nbhd_stage_reference(x, b, o, ([0, 1], [280.0, 0.5], [1, 0]))
    NB.nbhd_fold_reference(want, m, [0, 2])
    NB.nbhd_fold_reference(want, m, [0, 2], 1, 2)
    assert _same(mask.cpu().numpy(), m) and all(_same(state[k].cpu().numpy(), want[k]) for k in want)
    assert _same(hour['fss'].cpu().numpy(), NB.nbhd_finish_reference(want)['hour']['fss'])


# ------------------------------------------------------------------------------------------------ 4. the composed route
def _brute_force(x, b, o, thr, radius):
    """fp64 numpy on values [M, nt, P, ny, nx]: per (hour, threshold, scale) the sums over every clamped window, the windows summed node by node
    (shifted planes, no summed-area table), two-pass.  -> ints (n_valid, n_f, n_b, n_o [nt, E], windows [nt, E, K]) and the fss tables."""
    M, nt, _, ny, nx = x.shape
    E, K = len(thr[0]), len(radius)
    ints = {k: np.zeros((nt, E), dtype=np.int64) for k in ('n_valid', 'n_f', 'n_b', 'n_o')}
    ints['windows'] = np.zeros((nt, E, K), dtype=np.int64)
    sums = np.zeros((5, nt, E, K))
    for m in range(M):
        for e, (j, v, side) in enumerate(zip(*thr)):
            ev = (lambda z: z > np.float32(v)) if side == 0 else (lambda z: z < np.float32(v))
            with np.errstate(invalid='ignore'):
                valid = np.isfinite(x[m, :, j]) & np.isfinite(b[m, :, j]) & np.isfinite(o[m, :, j])
                planes = [(ev(z[m, :, j]) & valid).astype(np.int64) for z in (x, b, o)] + [valid.astype(np.int64)]
            for key, p in zip(('n_f', 'n_b', 'n_o', 'n_valid'), planes):
                ints[key][:, e] += p.sum(axis=(1, 2))
            for k, r in enumerate(radius):
                ry, rx = min(r, ny - 1), min(r, nx - 1)
                counts = []
                for p in planes:
                    if r >= max(nx, ny) - 1:                              # every window is the whole plane
                        counts.append(np.broadcast_to(p.sum(axis=(1, 2), keepdims=True), p.shape))
                        continue
                    pad = np.zeros((nt, ny + 2 * ry, nx + 2 * rx), dtype=np.int64)
                    pad[:, ry:ry + ny, rx:rx + nx] = p
                    counts.append(sum(pad[:, dy:dy + ny, dx:dx + nx] for dy in range(2 * ry + 1) for dx in range(2 * rx + 1)))
                cf, cb, co, cv = counts
                on = cv > 0
                V = np.where(on, cv, 1).astype(np.float64)
                Pf, Pb, Po = (np.where(on, c / V, 0.0) for c in (cf, cb, co))
                ints['windows'][:, e, k] += on.sum(axis=(1, 2))
                for q, term in enumerate(((Pf - Po) ** 2, Pf ** 2, Po ** 2, (Pb - Po) ** 2, Pb ** 2)):
                    sums[q, :, e, k] += np.sort(term.reshape(nt, -1), axis=1).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return ints, {'fss': 1.0 - sums[0] / (sums[1] + sums[2]), 'base_fss': 1.0 - sums[3] / (sums[4] + sums[2]),
                      'all_fss': 1.0 - sums[0].sum(0) / (sums[1].sum(0) + sums[2].sum(0)), 'all_base_fss': 1.0 - sums[3].sum(0) / (sums[4].sum(0) + sums[2].sum(0))}


def _lattice_values(m, case, lat, clip, ph):
    """(x, b) [nt, 4, ny, nx] (T, u, p, speed) of one case on `lat`: predict_lattice, and dpn_fields_out on the sampler's coord_data."""
    maps = m.predict_lattice(case['field_data'], case['sampler'], lat, case['forecast_h'], with_clip=clip)
    speed = m.diagnostic_lattice(case['field_data'], case['sampler'], lat, case['forecast_h'], ['speed'], with_clip=clip)
    x = torch.cat([maps[:, [3, 0, 2]], speed], dim=1).cpu().numpy()
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    cd = case['sampler'].sample_at(lat.n_points, lattice=lat)[4].contiguous()
    rows = torch.empty_like(cd)
    assert L.load().dpn_fields_out(_ptr(cd), cd.shape[0], ctypes.byref(ph), int(clip), _ptr(rows), None, None, 0, _stream()) == 0
    b = _with_speed(rows.cpu().numpy())
    return x, np.ascontiguousarray(b.reshape(lat.nt, lat.ny, lat.nx, 4).transpose(0, 3, 1, 2))


def test_verify_lattice_against_predict_lattice_and_numpy():
    """verify_lattice against predict_lattice / diagnostic_lattice per case + fp64 numpy brute force: the de-normalisation is the same code, so the
    counts and windows are equal exactly; the scores within the bound of tests/neighbourhood_cases.py (|fss| <= 1: 2^-23 absolute).  65 x 33 x 3
    nodes that leave the coarse cube on two faces, 2 cases, with and without the clip, a chunked walk, every refusal before the first launch."""
    from deepphysinet_amd.sampler import Lattice
    I = _inputs()
    m, ph = I['m'], I['cfg'].physics()
    lat = Lattice(200.0, 1.0, 120.0, 1.0, 12.0, 6.0, 65, 33, 3)          # x to 264 > 256 and y to 152 > 144: outside there
    names, scales = ['T', 'u', 'p', 'speed'], (1, 3, 5, 17, 131)
    radius = [0, 1, 2, 8, 65]
    cases = _members(2)
    for clip in (False, True):
        vals = [_lattice_values(m, c, lat, clip, ph) for c in cases]
        x, b = np.stack([v[0] for v in vals]), np.stack([v[1] for v in vals])
        assert 0 < int(np.isnan(b[0, 0, 0]).sum()) < b[0, 0, 0].size and np.array_equal(np.isnan(x), np.isnan(b))
        g = np.random.default_rng(11)
        scale = np.nanstd(x.astype(np.float64), axis=(0, 1, 3, 4), keepdims=True)
        o = (np.nan_to_num(x).astype(np.float64) + scale * (0.6 * g.standard_normal(x.shape) + 0.1)).astype(np.float32)
        o[g.random(o.shape) < 0.05] = np.nan
        thresholds = {'T': [('below', float(np.nanmedian(x[:, :, 0]))), float(np.nanquantile(x[:, :, 0], 0.8))], 'speed': float(np.nanquantile(x[:, :, 3], 0.7))}
        thr = ([0, 0, 3], [float(np.float32(thresholds['T'][0][1])), float(np.float32(thresholds['T'][1])), float(np.float32(thresholds['speed']))], [1, 0, 0])
        with_an = [dict(c, analysis=torch.from_numpy(o[k]).to(_dev())) for k, c in enumerate(cases)]
        got = m.verify_lattice(with_an, lat, names, thresholds, scales, with_clip=clip)
        assert sorted(got) == sorted(['names', 'thresholds', 'scales', 'hour', 'all']) and got['names'] == names and got['scales'] == list(scales)
        assert got['thresholds'] == [('T', 'below', thr[1][0]), ('T', 'above', thr[1][1]), ('speed', 'above', thr[1][2])]
        ints, scores = _brute_force(x, b, o, thr, radius)
        hour = {k: v.cpu().numpy() for k, v in got['hour'].items()}
        every = {k: v.cpu().numpy() for k, v in got['all'].items()}
        assert np.array_equal(hour['count'], ints['n_valid']) and np.array_equal(hour['windows'], ints['windows'])
        assert np.array_equal(every['count'], ints['n_valid'].sum(0)) and np.array_equal(every['windows'], ints['windows'].sum(0))
        with np.errstate(divide='ignore', invalid='ignore'):
            for key, num, den in (('freq_f', 'n_f', 'n_valid'), ('freq_b', 'n_b', 'n_valid'), ('freq_o', 'n_o', 'n_valid'), ('fbias', 'n_f', 'n_o'),
                                  ('base_fbias', 'n_b', 'n_o')):
                assert np.array_equal(hour[key], (ints[num] / ints[den]).astype(np.float32), equal_nan=True), key        # (one correctly rounded quotient)
        for key, table, want in (('fss', hour, scores['fss']), ('base_fss', hour, scores['base_fss']), ('fss', every, scores['all_fss']),
                                 ('base_fss', every, scores['all_base_fss'])):
            assert np.array_equal(np.isnan(table[key]), np.isnan(want)) and bool(np.isfinite(want).any())
            dev = float(np.nanmax(np.abs(table[key].astype(np.float64) - want)))
            print('clip %s, %s %s: worst deviation from fp64 brute force %.3e (bound %.3e)' % (clip, key, table[key].shape, dev, NC.BOUND))
            assert dev <= NC.BOUND and float(np.nanmax(np.abs(want))) <= 1.0, (clip, key, dev)
        assert hour['skilful_scale'].min() >= -1 and hour['skilful_scale'].max() < 5
        m.chunk_size = lambda *a, **k: 640                                 # a chunked walk: 9 rows + 55 nodes per chunk
        try:
            chunked = m.verify_lattice(with_an, lat, names, thresholds, scales, with_clip=clip)
        finally:
            del m.chunk_size
        for group in ('hour', 'all'):
            for key, v in got[group].items():
                assert _same(v.cpu().numpy(), chunked[group][key].cpu().numpy()), (group, key)
    # every refusal comes before the first launch
    for bad, err in ((dict(products=['vorticity']), KeyError), (dict(thresholds={}), ValueError), (dict(thresholds={'q': 1.0}), ValueError),
                     (dict(scales=[2]), ValueError), (dict(scales=[3, 1]), ValueError), (dict(cases=[]), ValueError),
                     (dict(cases=[dict(with_an[0], analysis=with_an[0]['analysis'][:, :3])]), ValueError),
                     (dict(cases=[dict(with_an[0], analysis=with_an[0]['analysis'].double())]), ValueError),
                     (dict(cases=[dict(with_an[0], analysis=with_an[0]['analysis'].cpu())]), ValueError),
                     (dict(cases=[{k: v for k, v in with_an[0].items() if k != 'analysis'}]), ValueError)):
        ok = dict(cases=with_an, lattice=lat, products=names, thresholds=thresholds, scales=scales)
        with pytest.raises(err):
            m.verify_lattice(**{**ok, **bad})


def test_width_one_agrees_with_verify_at_on_the_same_nodes():
    """r = 0 on a fully valid lattice: the fractions are 0 or 1, so n_f, n_o and the hits (n_f + n_o - sum_fo2) / 2 are the contingency counts of
    verify_at at the same nodes, and its pod, fbias and csi follow from them."""
    I = _inputs()
    m, s = I['m'], I['s']
    lat = s.lattice(refine=1, hours=(3.0, 9.0, 2), x_range=(30, 70), y_range=(50, 62))      # 41 x 13 x 2, inside the cube
    cases = _members(2)
    names = ['T', 'speed']
    vals = [_lattice_values(m, c, lat, False, I['cfg'].physics())[0][:, [0, 3]] for c in cases]
    g = np.random.default_rng(3)
    o = [(v.astype(np.float64) + np.nanstd(v, axis=(0, 2, 3), keepdims=True) * 0.5 * g.standard_normal(v.shape)).astype(np.float32) for v in vals]
    thresholds = {'T': ('below', float(np.median(vals[0][:, 0]))), 'speed': float(np.median(vals[0][:, 1]))}
    grid = m.verify_lattice([dict(c, analysis=torch.from_numpy(a).to(_dev())) for c, a in zip(cases, o)], lat, names, thresholds, [1])
    px, py, pt = lat.positions()
    obs = [torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(lat.n_points, 2))).to(_dev()) for a in o]
    point = m.verify_at([dict(c, obs=ob) for c, ob in zip(cases, obs)], px, py, pt, names, thresholds=thresholds, by={'all': np.zeros(lat.n_points, dtype=np.int64)})
    every = {k: v.cpu().numpy() for k, v in grid['all'].items()}
    table = {k: v.cpu().numpy() for k, v in point['all'].items()}
    assert every['count'].tolist() == [2 * lat.n_points] * 2 == table['count'][0].tolist() and every['windows'][:, 0].tolist() == every['count'].tolist()
    assert _same(every['fbias'], table['fbias'][0]) and _same(every['base_fbias'], table['base_fbias'][0])
    st_fo2 = (1.0 - every['fss'][:, 0].astype(np.float64))                 # r = 0: sum_fo2 / (n_f + n_o)
    n_f, n_o = (np.rint(every[k].astype(np.float64) * every['count']) for k in ('freq_f', 'freq_o'))
    hits = np.rint((n_f + n_o - st_fo2 * (n_f + n_o)) / 2.0)
    assert bool((hits > 0).all()) and bool((hits < np.minimum(n_f, n_o)).all())
    assert _same(table['pod'][0], (hits / n_o).astype(np.float32)) and _same(table['csi'][0], (hits / (n_f + n_o - hits)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 5. loop and launcher
def _analysis_file(path, M, names=('speed', 'T', 'q')):
    g = np.random.default_rng(23)
    d = dict(names=np.array(names), hours=np.array([0.0, 12.0]),
             analysis=(g.standard_normal((M, 2, len(names), 145, 257)) * np.array([2.0, 5.0, 1e-3]).reshape(1, 1, -1, 1, 1)
                       + np.array([3.0, 280.0, 5e-3]).reshape(1, 1, -1, 1, 1)).astype(np.float32))
    d['analysis'][0, 1, :, :10] = np.nan
    np.savez(path, **d)
    return d


def test_loop_writes_the_tables_and_leaves_the_rest_alone(tmp_path):
    from deepphysinet_amd.neighbourhood import OUT_FIELDS
    plain, with_key = tmp_path / 'plain', tmp_path / 'grid'
    _analysis_file(tmp_path / 'analysis.npz', M=2)
    m = _loop_model(tmp_path, write_source=True, result_path=str(plain), export_variable=['T'])
    ref = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)
    assert m.last_grid_verification is None
    m = _loop_model(tmp_path, write_source=True, result_path=str(with_key), export_variable=['T'])
    option = dict(products=['T', 'speed'], analysis=str(tmp_path / 'analysis.npz'), thresholds={'T': ('below', 280.0), 'speed': [3.0]}, scales=[1, 5, 33])
    maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2, verify_grid=option)
    assert torch.equal(maps, ref)                                          # the return value is unchanged
    for fn in sorted(os.listdir(plain)):                                   # ... and so are the per-sample files
        assert np.array_equal(np.load(plain / fn), np.load(with_key / fn)), fn
    v = m.last_grid_verification
    assert v['names'] == ['T', 'speed'] and v['thresholds'] == [('T', 'below', 280.0), ('speed', 'above', 3.0)] and v['scales'] == [1, 5, 33]
    assert v['hour']['fss'].shape == (2, 2, 3) and v['all']['fss'].shape == (2, 3) and v['hour']['count'].shape == (2, 2)
    assert v['hour']['count'].cpu().numpy().tolist() == [[2 * 145 * 257] * 2, [2 * 145 * 257 - 10 * 257] * 2]
    assert bool(torch.isfinite(v['all']['fss']).all()) and bool(torch.isfinite(v['all']['base_fss']).all())
    new = sorted(fn for fn in os.listdir(with_key) if '_nbhd_' in fn)
    assert len(new) == 2 * len(OUT_FIELDS) and len(os.listdir(with_key)) == len(os.listdir(plain)) + len(new)
    stamp = sorted(os.listdir(plain))[0][:-len('_T.npy')]                  # the first sample's first time step
    for group in ('hour', 'all'):
        for key in OUT_FIELDS:
            assert np.array_equal(np.load(with_key / ('%s_nbhd_%s_%s.npy' % (stamp, group, key))), v[group][key].cpu().numpy(), equal_nan=True), (group, key)
    with pytest.raises(ValueError, match='holds 2 cases, the sample source 1'):
        m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', verify_grid=option)


def test_the_launcher_runs_with_the_verify_grid_flags(tmp_path):
    _loop_model(tmp_path)
    _analysis_file(tmp_path / 'analysis.npz', M=1)
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--verify_grid', 'T,speed', '--verify_analysis', str(tmp_path / 'analysis.npz'), '--verify_grid_threshold',
                            'T:below:280', '--verify_scales', '1,9'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert "neighbourhood verification T,speed: fss (2, 1, 2), scales [1, 9], nodes counted 34695..37265, thresholds [('T', 'below', 280.0)]" in child.stdout
