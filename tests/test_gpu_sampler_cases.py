"""GPU (MI355X): the sampler family of csrc/dpn_sampler.hip across its C ABI against tests/sampler_cases.py.
  bit-exact
      * raw of dpn_sample_points / dpn_sample_points_replay against the host Philox-4x32-10 (`draws`): both drawing modes, four seeds, offsets whose
        carry into the high counter word falls inside the batch, a device step counter against the same counters as a host offset;
      * the u column of dpn_adaptive_select against `select_uniforms` (stream 2);
      * x, y, t of every point against the scipy oracle; chunks of a lattice against slices of the whole; the label gather; dpn_grid_maps and
        dpn_fields_out against `denorm_model`; every refused call: -1 and every output buffer untouched.
  derived bars (sampler_cases' docstring), no element left out
      * f within one fp32 ulp, coord_data within ulp32 + (W + 16 u) max|corner| of the oracle, on eight geometries x two cubes, through EXPLICIT
        node indices, stations and lattices; NaN exactly where the oracle is NaN; every fine node finite.
Every output lives inside a larger owned buffer whose rows before and after hold a sentinel bit pattern (map mode: every place outside the chunk as
well); the cube and the labels lie between NaN guards.  The last test prints the largest error / bar seen per case."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import sampler_cases as C

pytestmark = pytest.mark.gpu

RATIOS = {}
G = C.GUARD_ROWS
N = 600                                  # two full blocks of 256 and a ragged one


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _lib():
    from deepphysinet_amd import _lib as L
    return L, L.load()


class Out:
    """rows x cols outputs inside an owned buffer with G sentinel rows before and after."""

    def __init__(self, rows, cols=1, dtype=np.float32):
        self.rows, self.cols, self.dtype = rows, cols, np.dtype(dtype)
        self.fill = C.SENTINEL if self.dtype == np.float32 else C.SENTINEL64
        self.full = torch.from_numpy(np.full((rows + 2 * G) * cols, self.fill, self.dtype)).to(_dev())
        self.ptr = self.full.data_ptr() + G * cols * self.dtype.itemsize

    def _bits(self):
        return self.full.cpu().numpy().view(np.uint32 if self.dtype == np.float32 else np.uint64)

    def get(self):
        v = self.full.cpu().numpy()[G * self.cols:(G + self.rows) * self.cols]
        return v.reshape(self.rows, self.cols) if self.cols > 1 else v

    def guards_kept(self, written=None):
        """The rows outside the first `written` (default: all) rows of the window still hold the sentinel."""
        b, w = self._bits(), self.rows if written is None else written
        want = C.SENTINEL_BITS if self.dtype == np.float32 else C.SENTINEL64_BITS
        return bool((b[:G * self.cols] == want).all() and (b[(G + w) * self.cols:] == want).all())

    def untouched(self):
        return self.guards_kept(0)


def _input(values, dtype=np.float32):
    """An input between NaN guards (integers: between -2^30) -> (owned tensor, pointer to the values)."""
    values = np.ascontiguousarray(values, dtype).reshape(-1)
    pad = 64
    host = np.full(values.size + 2 * pad, np.nan if np.dtype(dtype).kind == 'f' else -2 ** 30, dtype)
    host[pad:pad + values.size] = values
    t = torch.from_numpy(host).to(_dev())
    return t, t.data_ptr() + pad * np.dtype(dtype).itemsize


@lru_cache(maxsize=None)
def _cube_dev(name, kind):
    return _input(C.cube(name, kind))


@lru_cache(maxsize=None)
def _labels_dev(name):
    return _input(C.labels(name))


@lru_cache(maxsize=None)
def _oracle(name, kind, what):
    geo = C.GEO[name]
    pts = {'nodes': lambda: C.node_points(geo), 'stations': lambda: C.station_points(geo)[:3],
           'lattice': lambda: C.lattice_positions(C.lattice_of(geo))}[what]()
    return pts, C.oracle_points(geo, C.cube(name, kind), *pts)


class Outs:
    def __init__(self, n, rows=None, lab=False, raw=False):
        rows = n if rows is None else rows
        self.n = n
        self.x, self.y, self.t, self.f = (Out(rows) for _ in range(4))
        self.cd = Out(rows, 6)
        self.lab = Out(rows, 6) if lab else None
        self.raw = Out(rows, 3, np.float64) if raw else None

    def all(self):
        return [b for b in (self.x, self.y, self.t, self.f, self.cd, self.lab, self.raw) if b is not None]

    def guards_kept(self):
        return all(b.guards_kept(self.n) for b in self.all())

    def untouched(self):
        return all(b.untouched() for b in self.all())

    def values(self):
        return tuple(b.get()[:self.n] for b in (self.x, self.y, self.t, self.f, self.cd))


def _sample_points(s, cube_ptr, mode, o, seed=0, offset=0, idx=(None, None, None), labels_ptr=None, step=None, stride=0, replay=False, n=None):
    """One launch of dpn_sample_points (or _replay) into the buffers `o` -> the return code (synchronised)."""
    L, lib = _lib()
    p = lambda b: None if b is None else b.ptr
    n = o.n if n is None else n
    if replay:
        rc = lib.dpn_sample_points_replay(ctypes.byref(s), cube_ptr, labels_ptr, mode, idx[0], idx[1], idx[2], n, seed, offset,
                                          None if step is None else step.data_ptr(), stride, o.x.ptr, o.y.ptr, o.t.ptr, o.f.ptr, o.cd.ptr, p(o.lab),
                                          p(o.raw), None)
    else:
        rc = lib.dpn_sample_points(ctypes.byref(s), cube_ptr, labels_ptr, mode, idx[0], idx[1], idx[2], n, seed, offset, o.x.ptr, o.y.ptr, o.t.ptr,
                                   o.f.ptr, o.cd.ptr, p(o.lab), p(o.raw), None)
    torch.cuda.synchronize()
    return rc


def _sample_at(s, cube_ptr, o, pos=None, lattice=None, first=0, n=None):
    L, lib = _lib()
    n = o.n if n is None else n
    ptrs = (None, None, None) if pos is None else pos
    lat = None if lattice is None else ctypes.byref(L.DpnLattice(*lattice))
    rc = lib.dpn_sample_at(ctypes.byref(s), cube_ptr, ptrs[0], ptrs[1], ptrs[2], lat, first, n, o.x.ptr, o.y.ptr, o.t.ptr, o.f.ptr, o.cd.ptr, None)
    torch.cuda.synchronize()
    return rc


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize('mode', (C.INTERIOR, C.MARGIN), ids=('interior', 'margin'))
def test_draws_equal_the_host_philox(mode):
    geo = C.GEO['default']
    s, (_, cube) = geo.struct(), _cube_dev('default', 'normal')
    for seed in (0, 1, 2 ** 32 + 5, 2 ** 64 - 1):
        for offset in (0, 2 ** 32 - 300, 2 ** 40 + 7):
            o = Outs(N, raw=True)
            assert _sample_points(s, cube, mode, o, seed, offset) == 0
            want = C.draws(mode, seed, offset, 0, 0, N, s)
            assert np.array_equal(_bits64(o.raw.get()), _bits64(want)), (seed, offset)
            assert o.guards_kept()
            x, y, t, _, _ = o.values()
            assert np.array_equal(x, (want[:, 0] * 27000.0).astype(np.float32)) and np.array_equal(t, (want[:, 2] * 3600.0).astype(np.float32))
    if mode == C.INTERIOR:                       # point 0 of seed 0, offset 0: the first Random123 known answer
        o = Outs(N, raw=True)
        assert _sample_points(s, cube, mode, o, 0, 0) == 0
        assert o.raw.get()[0, 0] == C.u53(0x6627e8d5, 0xe169c58d) * (s.lon - 1)


def test_replay_counter_equals_the_host_offset():
    """A device step counter of 3 with stride 2^31 (the product passes 2^32) against the model and against the same counters as a host offset."""
    geo = C.GEO['default']
    s, (_, cube) = geo.struct(), _cube_dev('default', 'normal')
    step = torch.tensor([3], dtype=torch.int32, device=_dev())
    for mode in (C.INTERIOR, C.MARGIN):
        a, b = Outs(N, raw=True), Outs(N, raw=True)
        assert _sample_points(s, cube, mode, a, 9, 11, step=step, stride=2 ** 31, replay=True) == 0
        assert _sample_points(s, cube, mode, b, 9, 11 + 3 * 2 ** 31) == 0
        want = C.draws(mode, 9, 11, 3, 2 ** 31, N, s)
        assert np.array_equal(_bits64(a.raw.get()), _bits64(want)) and np.array_equal(_bits64(b.raw.get()), _bits64(want))
        assert all(np.array_equal(_bits32(u), _bits32(v)) for u, v in zip(a.values(), b.values()))
        assert a.guards_kept() and b.guards_kept()


def test_margin_draws_of_a_small_geometry_and_their_labels():
    """4096 MARGIN draws on the 10 x 16 geometry equal the model (the CPU test shows that these reach both end nodes and every hour); the labels
    gathered at them are exact on a geometry with lon != lat."""
    geo = C.GEO['r01_03']
    s, (_, cube), (_, lab) = geo.struct(), _cube_dev('r01_03', 'normal'), _labels_dev('r01_03')
    n = 4096
    o = Outs(n, lab=True, raw=True)
    assert _sample_points(s, cube, C.MARGIN, o, 1, 0, labels_ptr=lab) == 0
    want = C.draws(C.MARGIN, 1, 0, 0, 0, n, s)
    raw = o.raw.get()
    assert np.array_equal(_bits64(raw), _bits64(want)) and o.guards_kept()
    assert raw[:, 0].max() == geo.lon - 1 and raw[:, 1].max() == geo.lat - 1 and raw[:, 2].max() == geo.t_hours and raw.min() == 0
    assert np.array_equal(o.lab.get(), C.SO.labels_at(C.labels('r01_03'), raw[:, 0], raw[:, 1], raw[:, 2]))
    res = C.check_points(geo, C.cube('r01_03', 'normal'), raw[:, 0], raw[:, 1], raw[:, 2], o.values())
    assert C.passes(res) and res['n_nan'] == 0, res
    RATIOS['r01_03 normal margin draws'] = (res['cd_ratio'], res['f_ratio'], res['n_differ'], res['n_compared'])


def test_selection_uniforms_equal_stream_two():
    from deepphysinet_amd.sampler import CollocationSampler
    geo = C.GEO['r02_10']
    dev = _dev()
    m, n, seed = 5, 300, 2 ** 32 + 5
    smp = CollocationSampler(geo.cfg, torch.from_numpy(np.array(C.cube('r02_10', 'normal'))).to(dev), seed=seed)
    score = torch.tensor([1.0, 0.5, 2.0, 0.0, 3.0], dtype=torch.float64, device=dev)
    pool = tuple(torch.arange(m, dtype=torch.float32, device=dev) + k for k in range(4)) + (torch.arange(6 * m, dtype=torch.float32, device=dev).reshape(m, 6),)
    for offset in (0, 2 ** 32 - 100):
        out = smp.select_weighted(score, pool, n, offset=offset, with_details=True)
        torch.cuda.synchronize()
        assert np.array_equal(_bits64(out[6].cpu().numpy()), _bits64(C.select_uniforms(seed, offset, 0, 0, n))), offset
        idx = out[5].cpu().numpy()
        assert idx.min() >= 0 and idx.max() < m
    smp.bind_step_counter(torch.tensor([3], dtype=torch.int32, device=dev), 2 ** 31)
    out = smp.select_weighted(score, pool, n, offset=7, with_details=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits64(out[6].cpu().numpy()), _bits64(C.select_uniforms(seed, 7, 3, 2 ** 31, n)))


# ---------------------------------------------------------------------------------------------- values
def _check(geo, kind, what, got, tag):
    pts, ref = _oracle(geo.name, kind, what)
    res = C.check_points(geo, C.cube(geo.name, kind), *pts, got, ref=ref)
    assert C.passes(res), (geo.name, kind, tag, res)
    RATIOS['%s %s %s' % (geo.name, kind, what)] = (res['cd_ratio'], res['f_ratio'], res['n_differ'], res['n_compared'])
    return res


@pytest.mark.parametrize('kind', C.CUBES)
@pytest.mark.parametrize('geo', C.GEOMETRIES, ids=lambda g: g.name)
def test_values_through_all_three_sources(geo, kind):
    s, (_, cube) = geo.struct(), _cube_dev(geo.name, kind)
    # EXPLICIT over every node (small geometries: with the label gather)
    xi, yi, ti = C.node_points(geo)
    n = xi.size
    with_lab = geo.name != 'default'
    keep = [_input(v, np.int32) for v in (xi, yi, ti)]
    o = Outs(n, lab=with_lab)
    assert _sample_points(s, cube, C.EXPLICIT, o, idx=tuple(k[1] for k in keep), labels_ptr=_labels_dev(geo.name)[1] if with_lab else None) == 0
    assert o.guards_kept()
    res = _check(geo, kind, 'nodes', o.values(), 'explicit')
    assert res['n_nan'] == 0 and np.isfinite(o.cd.get()).all()                     # every fine node is inside, the last row and column too
    if with_lab:
        assert np.array_equal(o.lab.get(), C.SO.labels_at(C.labels(geo.name), xi, yi, ti))
    # stations: random, on coarse cell faces, first and last node, and (the last rows) outside the cube
    xr, yr, tr, n_out = C.station_points(geo)
    keep = [_input(v, np.float64) for v in (xr, yr, tr)]
    o = Outs(xr.size)
    assert _sample_at(s, cube, o, pos=tuple(k[1] for k in keep)) == 0
    assert o.guards_kept()
    res = _check(geo, kind, 'stations', o.values(), 'stations')
    cd = o.cd.get()
    assert res['n_nan'] == 6 * n_out and np.isnan(cd[-n_out:]).all() and np.isfinite(cd[:-n_out]).all()
    # the two sides of the inside rule: 1e-10 of a cell beyond a face is taken as on the face, 1e-8 beyond is NaN
    pts = C.tolerance_points(geo)[0]
    keep = [_input(v, np.float64) for v in pts]
    o = Outs(pts[0].size)
    assert _sample_at(s, cube, o, pos=tuple(k[1] for k in keep)) == 0
    assert o.guards_kept()
    pattern, ratio, differ = C.check_tolerance_points(geo, C.cube(geo.name, kind), o.cd.get())
    assert pattern and ratio <= 1.0, (geo.name, kind, pattern, ratio)
    RATIOS['%s %s tolerance' % (geo.name, kind)] = (ratio, 0.0, differ, 6 * int(C.tolerance_points(geo)[1].sum()))
    # a lattice: the whole, then chunks that begin and end mid-row and cross the time plane, in buffers that are longer than the chunk
    lat = C.lattice_of(geo)
    total = lat[6] * lat[7] * lat[8]
    o = Outs(total)
    assert _sample_at(s, cube, o, lattice=lat, first=0) == 0
    assert o.guards_kept()
    res = _check(geo, kind, 'lattice', o.values(), 'lattice')
    assert res['n_nan'] == 0
    whole = o.values()
    for first, cnt in C.LATTICE_CHUNKS:
        c = Outs(cnt, rows=cnt + 5)
        assert _sample_at(s, cube, c, lattice=lat, first=first) == 0
        assert c.guards_kept()
        assert all(np.array_equal(_bits32(u), _bits32(v[first:first + cnt])) for u, v in zip(c.values(), whole)), (first, cnt)


# ---------------------------------------------------------------------------------------------- de-normalisation and scatter
@pytest.mark.parametrize('table', sorted(C.PHYS_TABLES))
def test_grid_maps_and_fields_out_equal_the_fp32_model(table):
    L, lib = _lib()
    ph = C.phys_struct(table)
    for clip in (0, 1):
        # dpn_grid_maps on a 5 x 3 grid
        out = C.denorm_inputs(15, clip)
        keep = _input(out)
        maps = Out(6 * 3, 5)
        assert lib.dpn_grid_maps(keep[1], 5, 3, ctypes.byref(ph), clip, maps.ptr, None) == 0
        torch.cuda.synchronize()
        assert maps.guards_kept()
        assert np.array_equal(_bits32(maps.get().reshape(6, 3, 5)), _bits32(C.grid_maps_model(out, 5, 3, table, bool(clip))))
        # dpn_fields_out, rows mode
        out = C.denorm_inputs(N, 2 + clip)
        keep = _input(out)
        rows = Out(N, 6)
        assert lib.dpn_fields_out(keep[1], N, ctypes.byref(ph), clip, rows.ptr, None, None, 0, None) == 0
        torch.cuda.synchronize()
        assert rows.guards_kept()
        want = C.fields_out_model(out, table, bool(clip))
        assert np.array_equal(_bits32(rows.get()), _bits32(want))
        assert np.array_equal(np.isnan(rows.get()), np.isnan(out))
        # dpn_fields_out, map mode: the whole lattice, then chunks; every place outside the chunk keeps the sentinel
        lat = C.lattice_of(C.GEO['r01_03'])
        nx, ny, nt = lat[6:]
        out = C.denorm_inputs(nx * ny * nt, 4 + clip)
        keep = _input(out)
        for first, cnt in ((0, nx * ny * nt),) + C.LATTICE_CHUNKS:
            m = Out(nt * 6 * ny, nx)
            lt = L.DpnLattice(*lat)
            assert lib.dpn_fields_out(keep[1] + first * 24, cnt, ctypes.byref(ph), clip, None, m.ptr, ctypes.byref(lt), first, None) == 0
            torch.cuda.synchronize()
            assert m.guards_kept()
            want = C.fields_out_model(out[first:first + cnt], table, bool(clip), lat, first, np.full((nt, 6, ny, nx), C.SENTINEL, np.float32))
            assert np.array_equal(_bits32(m.get().reshape(nt, 6, ny, nx)), _bits32(want)), (clip, first, cnt)


# ---------------------------------------------------------------------------------------------- refusals
def test_refused_calls_write_nothing():
    L, lib = _lib()
    geo = C.GEO['r01_03']
    s, (_, cube), (_, lab) = geo.struct(), _cube_dev('r01_03', 'normal'), _labels_dev('r01_03')
    xi, yi, ti = C.node_points(geo)
    keep = [_input(v[:N], np.int32) for v in (xi, yi, ti)]
    idx = tuple(k[1] for k in keep)

    def refused(o, rc):
        assert rc == -1 and o.untouched()

    plain, pos = Outs(N, raw=True), [_input(v[:N].astype(np.float64), np.float64) for v in (xi, yi, ti)]
    refused(plain, _sample_points(s, cube, 3, plain, replay=True))                                     # no such mode
    refused(plain, _sample_points(s, cube, 3, plain, idx=idx, replay=True))
    refused(plain, _sample_points(s, cube, -1, plain, replay=True))
    for missing in range(3):                                                                           # EXPLICIT without an index array
        part = tuple(None if k == missing else v for k, v in enumerate(idx))
        refused(plain, _sample_points(s, cube, C.EXPLICIT, plain, idx=part))
    refused(plain, _sample_points(s, cube, C.EXPLICIT, plain))
    o = Outs(N, lab=True, raw=True)
    refused(o, _sample_points(s, cube, C.INTERIOR, o, labels_ptr=lab))                                 # labels exist at nodes only
    refused(o, _sample_points(s, cube, C.MARGIN, o))                                                   # label_out without labels
    refused(o, _sample_points(s, cube, C.EXPLICIT, o, idx=idx))
    assert _sample_points(s, cube, C.EXPLICIT, o, idx=idx, labels_ptr=lab) == 0 and o.guards_kept() and not o.lab.untouched()
    for field in ('lon_in', 'lat_in', 't_in', 'lon', 'lat'):
        for value in (1, 0):
            bad = geo.struct()
            setattr(bad, field, value)
            refused(plain, _sample_points(bad, cube, C.MARGIN, plain))
            refused(plain, _sample_points(bad, cube, C.EXPLICIT, plain, idx=idx, replay=True))
            refused(plain, _sample_at(bad, cube, plain, pos=tuple(k[1] for k in pos)))
    lat = C.lattice_of(geo)
    refused(plain, _sample_at(s, cube, plain, lattice=lat, first=0))                                   # more points than the lattice has
    refused(plain, _sample_at(s, cube, plain, lattice=lat, first=40, n=3))
    refused(plain, _sample_at(s, cube, plain, pos=tuple(k[1] for k in pos), lattice=lat, n=10))        # both sources
    refused(plain, _sample_at(s, cube, plain))                                                         # neither
    assert _sample_points(s, cube, C.MARGIN, plain) == 0 and plain.guards_kept() and not plain.untouched()       # (the buffers were live)
    ph = C.phys_struct('affine')
    out = _input(C.denorm_inputs(15))
    maps = Out(18, 5)
    for lon, la in ((0, 3), (5, 0), (-1, 3)):
        assert lib.dpn_grid_maps(out[1], lon, la, ctypes.byref(ph), 1, maps.ptr, None) == -1
    torch.cuda.synchronize()
    assert maps.untouched()
    rows, maps, lt = Out(15, 6), Out(2 * 6 * 3, 7), L.DpnLattice(*lat)
    assert lib.dpn_fields_out(out[1], 15, ctypes.byref(ph), 1, rows.ptr, maps.ptr, ctypes.byref(lt), 0, None) == -1      # both destinations
    assert lib.dpn_fields_out(out[1], 15, ctypes.byref(ph), 1, None, None, None, 0, None) == -1                            # neither
    assert lib.dpn_fields_out(out[1], 15, ctypes.byref(ph), 1, rows.ptr, None, ctypes.byref(lt), 0, None) == -1            # rows with a lattice
    assert lib.dpn_fields_out(out[1], 15, ctypes.byref(ph), 1, None, maps.ptr, ctypes.byref(lt), 30, None) == -1           # past the lattice's end
    torch.cuda.synchronize()
    assert maps.untouched() and rows.untouched()


def test_zz_summary_of_error_to_bar_ratios():
    """Printed for the reviewer: the largest error / bar per case against the scipy oracle (of the tests above that ran in this process), and how
    many of the compared coord_data elements differ from the oracle at all.  A ratio of 1.0000 is one fp32 ulp: both sides cast an fp64 value
    once, and at the nodes of a grid whose weights are short binary fractions that value often lies on an fp32 tie."""
    print()
    for k in sorted(RATIOS):
        r = RATIOS[k]
        print('largest error / bar   %-30s coord_data %.4f   f %.4f   differing %d of %d' % (k, r[0], r[1], r[2], r[3]))
        assert max(r[:2]) <= 1.0
