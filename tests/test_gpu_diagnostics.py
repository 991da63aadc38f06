"""GPU (MI355X): derived diagnostics from the Jacobian -- dpn_diagnostics_out through PackedField.diagnostics, InterfacePhysics.diagnostics_at /
diagnostic_lattice, run_inference_interface's log.export_diagnostic and infer.py --diagnostics (hi+lo mode).

Yardsticks: deepphysinet_amd.diagnostics, the numpy restatement of the kernel (fp32: bit for bit, the kernel is compiled without contraction; fp64: the
truth for rel_humidity, which goes through expf), the rows / maps / chunking identities of the inference surface, and oracle/dpn_oracle.py in fp64 with
bars from the reference's own arithmetic (tests/diagnostics_cases.py, tools/diagnostics_bars.py).  Model, field, sampler and stations are those of
tests/test_gpu_inference.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from tests import diagnostics_cases as DC
from tests.test_gpu_inference import _field, _stations
from tests.test_gpu_parity import GEO, TOL, _clip_and_delta, _dev, _model, _oracle_masks
from tests.test_sampler import _sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1037
_cache = {}


def _inputs():
    """The kernel's inputs at the 1 037 stations of seed 0, computed once: normalised fields and Jacobian of the forward kernel, f of the sampler."""
    if not _cache:
        import deepphysinet_amd as dpn
        s, _, _ = _sampler(with_labels=False)
        m = _model('bf16x2')
        field, fh = _field()
        xi, yi, hr = _stations(N, seed=0)
        x, y, t, cd, f = s.at_positions(xi, yi, hr)
        cfg = m.point_config()
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(field, fh)
            out_n, jac_n = dpn.pde_fields_and_jacobian(cfg, x, y, t, cd, heads, evec, statics)
        _cache.update(s=s, m=m, field=field, fh=fh, stations=(xi, yi, hr), points=(x, y, t, cd, f), cfg=cfg, weights=(heads, evec, statics),
                      out_n=out_n.contiguous(), jac_n=jac_n.contiguous(), f=f.reshape(-1).contiguous())
    return _cache


def _launch(out_n, jac_n, f, n, ph, with_clip, ids, rows=None, maps=None, lattice=None, first=0):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    arr = None if ids is None else (ctypes.c_int32 * len(ids))(*ids)
    return L.load().dpn_diagnostics_out(_ptr(out_n), _ptr(jac_n), _ptr(f), n, None if ph is None else ctypes.byref(ph), with_clip, arr,
                                        0 if ids is None else len(ids), _ptr(rows), _ptr(maps), lattice, first, _stream())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _physics_cases(I):
    """(name, DpnPhysics, with_clip): the shipped table without and with its clip, and one with q in the squared min_max form and T clipped at the
    median of its values (a part of the points on either side)."""
    from deepphysinet_amd.diagnostics import denorm_reference
    shipped = I['cfg'].physics()
    assert [shipped.clip_on[k] for k in range(6)] == [0, 0, 1, 1, 1, 1]
    odd = I['cfg'].physics()
    odd.mean[4], odd.std[4], odd.sq_on[4], odd.sq_add[4] = 0.08, 0.03, 1, 0.001
    T = denorm_reference(I['out_n'].cpu().numpy(), I['jac_n'].cpu().numpy(), shipped, False, np.float32)[0][:, 3]
    odd.clip_lo[3] = float(np.float32(np.median(T)))
    return [('shipped, no clip', shipped, 0), ('shipped, clip', shipped, 1), ('q squared, T clipped at its median', odd, 1)]


# ------------------------------------------------------------------------------------------------ 1. the kernel against its restatement
@pytest.mark.parametrize('n', [1, 255, 256, 257, N])
def test_kernel_is_the_fp32_restatement_bit_for_bit(n):
    """Every product but rel_humidity equals diagnostics_reference(denorm_reference(float32), float32) bit for bit: one point, either side of the
    256-thread block edge, a ragged multi-block size; all 28 products, one alone, the list reversed, a list with a repeat; without and with the
    clip, and a table with a squared-form variable and a variable clipped on part of the points.  rel_humidity (expf and two divisions) is held to the
    fp64 restatement on the same inputs, within 4 x the fp32 restatement's own deviation, both of max |rh| over the 1 037 points; a smaller n writes
    the first n rows of that run, bit for bit.
    Measured (MI355X), rel_humidity against the fp64 restatement, of max |rh|: kernel 1.239e-06, numpy float32 1.239e-06, bar 4.957e-06 (the shipped
    table, without and with the clip); 1.498e-06, 1.498e-06, 5.991e-06 (q in the squared form)."""
    from deepphysinet_amd.diagnostics import PRODUCTS, denorm_reference, diagnostics_reference, product_ids
    I = _inputs()
    out_n, jac_n, f = I['out_n'][:n], I['jac_n'][:n], I['f'][:n]
    ho, hj, hf = I['out_n'].cpu().numpy(), I['jac_n'].cpu().numpy(), I['f'].cpu().numpy()
    all_ids = list(range(28))
    selections = [all_ids, [18], [26], all_ids[::-1], [20, 3, 26, 20, 18, 3]]
    exact = np.array([i != 26 for i in all_ids])
    for name, ph, clip in _physics_cases(I):
        v32, m32, J32 = denorm_reference(ho, hj, ph, clip, np.float32)
        v64, _, J64 = denorm_reference(ho, hj, ph, clip, np.float64)
        want = diagnostics_reference(v32, J32, hf, PRODUCTS, np.float32)
        rh64 = diagnostics_reference(v64, J64, hf, ['rel_humidity'], np.float64)[:, 0]
        if clip and n >= 255:
            assert 0 < int((m32[:n, 3] == 0).sum()) < n or 'median' not in name           # T is clipped on a part of these points
        full = torch.full((N, 28), -7.0, dtype=torch.float32, device=_dev())
        assert _launch(I['out_n'], I['jac_n'], I['f'], N, ph, clip, all_ids, rows=full) == 0
        full = full.cpu().numpy()
        bar, dev = DC.rel_humidity_bar(want[:, 26], rh64)
        err = np.abs(full[:, 26].astype(np.float64) - rh64).max() / np.abs(rh64).max()
        print('%s: rel_humidity against the fp64 restatement, of max |rh|: kernel %.3e, fp32 restatement %.3e, bar %.3e' % (name, err, dev, bar))
        assert np.all(np.isfinite(want)) and np.isfinite(rh64).all()
        assert err <= bar, (name, err, bar)
        assert np.array_equal(_bits(full[:, exact]), _bits(want[:, exact])), name
        for ids in selections:
            rows = torch.full((n, len(ids)), -7.0, dtype=torch.float32, device=_dev())
            assert _launch(out_n, jac_n, f, n, ph, clip, ids, rows=rows) == 0
            got = rows.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(full[:n][:, ids])), (name, ids)            # a column is the same column of the full run
    assert product_ids(PRODUCTS) == all_ids


# ------------------------------------------------------------------------------------------------ 2. NaN
def test_points_outside_the_coarse_cube_are_nan_in_every_product_and_no_other_row_is():
    """Stations are range-checked on the host, so positions outside the cube reach the kernel through a lattice: its points, sampled (NaN coord_data
    outside), go through PackedField.diagnostics in ROW mode.  Every product of exactly those rows is NaN -- the 18 derivatives included, although the
    forward kernel's Jacobian is finite there --, without and with the clip."""
    from deepphysinet_amd.diagnostics import PRODUCTS, product_ids
    from deepphysinet_amd.sampler import Lattice
    I = _inputs()
    s, m = I['s'], I['m']
    out = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    px, py, pt = out.positions()
    nan = (px > 256) | (py > 144) | (pt > 24)
    assert 0 < nan.sum() < nan.size
    x, y, t, f, cd = s.sample_at(out.n_points, lattice=out)
    field = m._inference_weights(I['field'], I['fh'], out.n_points)
    for clip in (False, True):
        rows = torch.full((out.n_points, 28), -7.0, dtype=torch.float32, device=_dev())
        field.diagnostics(x, y, t, f, cd, product_ids(PRODUCTS), clip, rows=rows)
        got = rows.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.repeat(nan[:, None], 28, axis=1)), clip
        assert np.all(np.isfinite(got[~nan]))
    # at the kernel: one NaN among a point's six fields poisons the point's whole row and no other
    out_n = I['out_n'][:300].clone()
    hit = [0, 63, 64, 255, 256, 299]
    for r, k in zip(hit, range(6)):
        out_n[r, k] = float('nan')
    rows = torch.full((300, 28), -7.0, dtype=torch.float32, device=_dev())
    assert _launch(out_n, I['jac_n'][:300], I['f'][:300], 300, I['cfg'].physics(), 1, list(range(28)), rows=rows) == 0
    bad = np.zeros(300, dtype=bool)
    bad[hit] = True
    assert np.array_equal(np.isnan(rows.cpu().numpy()), np.repeat(bad[:, None], 28, axis=1))


# ------------------------------------------------------------------------------------------------ 3. rows and maps
def test_lattice_maps_are_the_station_rows_chunked_or_not():
    from deepphysinet_amd.diagnostics import PRODUCTS
    from deepphysinet_amd.sampler import Lattice
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    names = list(PRODUCTS)
    lat = s.lattice(refine=2, hours=(4.0, 0.5, 3), x_range=(10, 40), y_range=(20, 35.5))      # the lattice of the residual_lattice test: 61 x 32 x 3
    px, py, pt = lat.positions()
    for clip in (False, True):
        rows = m.diagnostics_at(field, s, px, py, pt, fh, names, with_clip=clip)
        assert rows.shape == (lat.n_points, 28) and bool(torch.isfinite(rows).all())
        want = rows.view(lat.nt, lat.ny, lat.nx, 28).permute(0, 3, 1, 2)
        whole = m.diagnostic_lattice(field, s, lat, fh, names, with_clip=clip)
        assert whole.shape == (lat.nt, 28, lat.ny, lat.nx) and torch.equal(whole, want)
        assert torch.equal(m.diagnostic_lattice(field, s, lat, fh, names, with_clip=clip, chunk_points=128), whole)
        assert torch.equal(m.diagnostic_lattice(field, s, lat, fh, names, with_clip=clip, chunk_points=256), whole)
    few = ['dT_dt', 'vorticity', 'dT_dt']                                                    # a selection is the same columns
    assert torch.equal(m.diagnostic_lattice(field, s, lat, fh, few, with_clip=True, chunk_points=640), whole[:, [11, 18, 11]])
    lon, la = 72.0 + px[:200] * 0.25, 18.0 + py[:200] * 0.25
    assert torch.equal(m.diagnostics_at(field, s, lon, la, pt[:200], fh, few, with_clip=True, lonlat=True), rows[:200][:, [11, 18, 11]])
    # a chunk boundary mid-row (20 x 15 x 4 points in chunks of 128: 6 rows + 8 points), on a lattice that leaves the cube: NaN exactly there
    out = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    px, py, pt = out.positions()
    nan = ((px > 256) | (py > 144) | (pt > 24)).reshape(out.nt, 1, out.ny, out.nx).repeat(3, axis=1)
    a = m.diagnostic_lattice(field, s, out, fh, few)
    b = m.diagnostic_lattice(field, s, out, fh, few, chunk_points=128)
    assert np.array_equal(torch.isnan(a).cpu().numpy(), nan) and 0 < nan.sum() < nan.size
    assert torch.equal(torch.isnan(b), torch.isnan(a)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert bool(torch.isfinite(a[~torch.isnan(a)]).all())


# ------------------------------------------------------------------------------------------------ 4. end to end against the fp64 oracle
def test_diagnostics_match_the_fp64_oracle():
    """diagnostics_at (all 28 products, no clip) at the 1 037 stations of seed 0 against the fp64 oracle: oracle.dpn_oracle's forward, inverse_norm and
    jacobian_fields, then diagnostics_reference(float64).  The points and the rule for points left out are those of
    test_per_point_residuals_match_the_fp64_oracle (a ReLU, clip or vapour switch that differs from the fp64 oracle's; at most n // 100 = 10).

    Bars (tests/diagnostics_cases.py), from the reference's own arithmetic alone: `python tools/diagnostics_bars.py` (CPU) printed
    e32_J = 2.697e-06 (the constant of that test, reproduced), e32_field = 1.729e-06, 2 of 1 037 points left out, and e32_d =
    1.160e-06 1.056e-06 1.604e-06 9.115e-07 5.130e-07 3.959e-07 1.710e-06 1.780e-06 1.697e-06 1.227e-06 2.215e-06 2.923e-06 6.603e-07 9.124e-07
    1.051e-06 1.394e-06 9.673e-07 2.611e-06 | 1.086e-06 4.137e-07 6.498e-07 2.182e-06 3.703e-06 8.201e-07 6.212e-07 1.389e-06 9.998e-06 5.638e-07.
    Products linear in the Jacobian: bar_i = (2e-4 / e32_J) * e32_d[i] (2.9e-05 .. 2.7e-04); speed and rel_humidity: (5e-5 / e32_field) * e32_d[i] =
    4.0e-05, 2.9e-04.
    Measured on an MI355X (error / bar, of max |product|; 8 points left out: 203, 440, 591, 608, 622, 785, 857, 899): the derivatives 7.1e-06 /
    8.6e-05, 6.2e-06 / 7.8e-05, 1.1e-05 / 1.2e-04 (u); 6.0e-06 / 6.8e-05, 3.2e-06 / 3.8e-05, 3.5e-06 / 2.9e-05 (v); 9.4e-06 / 1.3e-04, 6.3e-06 /
    1.3e-04, 5.2e-06 / 1.3e-04 (p); 6.6e-06 / 9.1e-05, 8.9e-06 / 1.6e-04, 9.1e-06 / 2.2e-04 (T); 5.8e-06 / 4.9e-05, 4.6e-06 / 6.8e-05, 5.1e-06 /
    7.8e-05 (q); 8.0e-06 / 1.0e-04, 5.8e-06 / 7.2e-05, 1.7e-05 / 1.9e-04 (rho); vorticity 6.4e-06 / 8.1e-05, abs_vorticity 2.4e-06 / 3.1e-05,
    divergence 3.0e-06 / 4.8e-05, omega 4.9e-06 / 1.6e-04, t_advection 1.6e-05 / 2.7e-04, q_advection 7.3e-06 / 6.1e-05, q_flux_divergence
    3.4e-06 / 4.6e-05, speed 6.3e-06 / 4.0e-05, rel_humidity 3.3e-05 / 2.9e-04, deformation 3.3e-06 / 4.2e-05."""
    from deepphysinet_amd.diagnostics import PRODUCTS, diagnostics_reference
    from deepphysinet_amd.point_path import relu_masks
    assert (TOL['bf16x2']['jac'], TOL['bf16x2']['field']) == (DC.TOL_JAC, DC.TOL_FIELD) and DC.E32_J == 2.697e-06
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    xi, yi, hr = I['stations']
    got = m.diagnostics_at(field, s, xi, yi, hr, fh, PRODUCTS).double().cpu().numpy()
    x, y, t, cd, f = I['points']
    heads, evec, statics = I['weights']
    with torch.no_grad():
        m1, m2 = relu_masks(I['cfg'], x, y, t, cd, heads, evec, statics)
    clip, delta = _clip_and_delta(I['out_n'], I['jac_n'], True)
    st = O.make_state(dtype=torch.float64)
    c = dict(x=x.cpu().double().reshape(-1, 1), y=y.cpu().double().reshape(-1, 1), t=t.cpu().double().reshape(-1, 1), f=f.cpu().double().reshape(-1, 1),
             coord_data=cd.cpu().double(), field_data=field.cpu().double(), forecast_h=fh.cpu().double())
    X, Y, T_ = (c[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    fields = O.inverse_norm(O.physics_net_forward(st, c['field_data'], O.encoding_coord(X, Y, T_, GEO), c['coord_data'], c['forecast_h']),
                            with_clip=False)
    J = O.jacobian_fields(X, Y, T_, fields).detach().numpy()
    want = diagnostics_reference(torch.cat(fields, 1).detach().numpy(), J, f.cpu().numpy().reshape(-1), PRODUCTS, np.float64)
    o1, o2, oclip, odelta = _oracle_masks(c, st=st)
    flipped = ((m1.cpu() != o1) | (m2.cpu() != o2)).any(dim=2).any(dim=0) | (clip != oclip).any(dim=1) | (delta != odelta)
    idx = torch.nonzero(flipped).flatten().tolist()
    print('points left out (a switch differs from the fp64 oracle): %s' % idx)
    assert len(idx) <= N // 100, idx
    keep = (~flipped).numpy()
    err = np.abs(got[keep] - want[keep]).max(axis=0) / np.abs(want[keep]).max(axis=0)
    bars = DC.oracle_bars()
    for i, name in enumerate(PRODUCTS):
        print('%-18s error / max %.3e   bar %.3e' % (name, err[i], bars[i]))
    assert np.all(err <= bars), (err, bars)


# ------------------------------------------------------------------------------------------------ 5, 6. loop, launcher, and the option off
class _Spy:
    """Counts calls of the new entry point on the loaded library (the spy of tests/test_gpu_causal.py)."""

    def __init__(self):
        from deepphysinet_amd import _lib as L
        self.lib, self.calls = L.load(), []
        self.inner = self.lib.dpn_diagnostics_out

    def __enter__(self):
        self.lib.dpn_diagnostics_out = lambda *a: (self.calls.append('dpn_diagnostics_out'), self.inner(*a))[1]
        return self

    def __exit__(self, *exc):
        self.lib.dpn_diagnostics_out = self.inner


def _loop_model(tmp_path, **log):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg'].update(img_size=(145, 257), dt=7200)
    cfg['inference_cfg']['log'].update(log)
    torch.manual_seed(4)
    m = builder_models(**cfg)
    m.with_clip = True
    if not (tmp_path / 'ckpt' / 'physics_latest.pth').exists():
        (tmp_path / 'ckpt').mkdir()
        m.save_model(str(tmp_path / 'ckpt'), epoch=0, global_step=1, prefix='physics')
    return m


def test_loop_writes_the_products_and_the_launcher_runs(tmp_path):
    from deepphysinet_amd.sampler import SyntheticSamples
    results = tmp_path / 'results'
    m = _loop_model(tmp_path, write_source=True, result_path=str(results), export_variable=['T'], export_diagnostic=['vorticity', 'dT_dt'])
    with _Spy() as spy:
        maps = m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic')
        assert spy.calls == ['dpn_diagnostics_out']                      # one sample, one chunk: one launch
    nt = 13
    assert maps.shape == (nt, 6, 145, 257)
    d = m.last_diagnostics
    assert d['names'] == ['vorticity', 'dT_dt'] and d['maps'].shape == (nt, 2, 145, 257) and bool(torch.isfinite(d['maps']).all())
    syn = SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    lattice = syn.sampler.lattice(refine=1, hours=(0.0, 2.0, nt))
    assert torch.equal(m.predict_lattice(b['field_data'], syn.sampler, lattice, b['forecast_h'], with_clip=True), maps)      # the return value is unchanged
    direct = m.diagnostic_lattice(b['field_data'], syn.sampler, lattice, b['forecast_h'], ['vorticity', 'dT_dt'], with_clip=True)
    assert torch.equal(direct, d['maps'])
    for j, name in enumerate(d['names']):
        files = sorted(fn for fn in os.listdir(results) if fn.endswith('_%s.npy' % name))
        assert len(files) == nt, files
        for it, fn in enumerate(files):
            a = np.load(os.path.join(results, fn))
            assert a.shape == (145, 257) and a.dtype == np.float32 and np.array_equal(a, direct[it, j].cpu().numpy()), fn
    assert len(os.listdir(results)) == 3 * nt
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--diagnostics', 'vorticity'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert 'diagnostics vorticity: maps (49, 1, 145, 257), finite True' in child.stdout          # the configuration's dt: half-hourly
    assert len([fn for fn in os.listdir(tmp_path / 'cli') if fn.endswith('_vorticity.npy')]) == 49


def test_nothing_calls_the_new_kernel_without_the_option(tmp_path):
    I = _inputs()
    s, m, field, fh = I['s'], I['m'], I['field'], I['fh']
    xi, yi, hr = _stations(300, seed=5)
    lat = s.lattice(hours=3, x_range=(0, 40), y_range=(0, 30))
    loop = _loop_model(tmp_path, write_source=False)
    with _Spy() as spy:
        m.predict_points(field, s, xi, yi, hr, fh)
        m.predict_lattice(field, s, lat, fh)
        m.residuals_at(field, s, xi, yi, hr, fh)
        m.residual_lattice(field, s, lat, fh)
        assert loop.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic') is not None
        assert spy.calls == [] and loop.last_diagnostics is None
        m.diagnostics_at(field, s, xi, yi, hr, fh, ['speed'])            # the spy does see the kernel when it is asked for
        assert spy.calls == ['dpn_diagnostics_out']


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_entry_point_refuses_bad_arguments_and_writes_nothing():
    from deepphysinet_amd import _lib as L
    I = _inputs()
    n = 300
    o, j, f, ph = I['out_n'][:n], I['jac_n'][:n], I['f'][:n], I['cfg'].physics()
    rows = torch.full((n, 28), -7.0, dtype=torch.float32, device=_dev())
    maps = torch.full((3, 28, 10, 10), -7.0, dtype=torch.float32, device=_dev())
    lat = L.DpnLattice(0, 1, 0, 1, 0, 1, 10, 10, 3)
    by = ctypes.byref
    ids = [18, 20]
    ok = dict(out_n=o, jac_n=j, f=f, n=n, ph=ph, with_clip=0, ids=ids, rows=rows)
    cases = [dict(out_n=None), dict(jac_n=None), dict(f=None), dict(ph=None), dict(ids=None), dict(n=0), dict(n=-5),
             dict(ids=[]), dict(ids=list(range(28)) + [0]), dict(ids=[18, 28]), dict(ids=[-1]),
             dict(rows=rows, maps=maps, lattice=by(lat)), dict(rows=None), dict(rows=None, maps=maps),
             dict(rows=None, maps=maps, lattice=by(L.DpnLattice(0, 1, 0, 1, 0, 1, 0, 10, 3))),
             dict(rows=None, maps=maps, lattice=by(L.DpnLattice(0, 1, 0, 1, 0, 1, 10, 0, 3))),
             dict(rows=None, maps=maps, lattice=by(L.DpnLattice(0, 1, 0, 1, 0, 1, 10, 10, 0))),
             dict(rows=None, maps=maps, lattice=by(lat), first=1), dict(rows=None, maps=maps, lattice=by(lat), n=n, first=-1)]
    for case in cases:
        assert _launch(**{**ok, **case}) == -1, sorted(case)
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((maps == -7.0).all())
    # and the same arguments, accepted: 300 points fill a 10 x 10 x 3 lattice exactly
    maps2 = torch.full((3, 2, 10, 10), -7.0, dtype=torch.float32, device=_dev())
    rows2 = torch.full((n, 2), -7.0, dtype=torch.float32, device=_dev())
    assert _launch(**{**ok, **dict(rows=None, maps=maps2, lattice=by(lat))}) == 0 and _launch(**{**ok, **dict(rows=rows2)}) == 0
    torch.cuda.synchronize()
    assert bool((rows2 != -7.0).all()) and torch.equal(maps2.permute(0, 2, 3, 1).reshape(n, 2), rows2)
