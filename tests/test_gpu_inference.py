"""GPU (MI355X): inference at stations and on lattices -- dpn_sample_at, dpn_fields_out, dpn_residual_points through CollocationSampler.at_positions /
lattice and InterfacePhysics.predict_points / predict_lattice / residuals_at / residual_lattice / run_inference_interface (hi+lo mode).

Yardsticks: the existing integer-node path (bitwise), oracle/sampler_oracle.py (the sampler's bars: coordinates bit-exact, coord_data rtol 2e-7 /
atol 1e-7, f rtol 2e-7), oracle/dpn_oracle.py (fields: TOL['bf16x2']['field'] of the maximum; residuals: see the residual tests), and the training
step itself (bitwise before / after an inference call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dpn_oracle as O
from oracle import sampler_oracle as SO
from oracle.fill import synthetic_inputs
from tests.test_gpu_parity import GEO, TOL, _clip_and_delta, _dev, _gpu, _model, _oracle_masks
from tests.test_sampler import IN_LAT, IN_LON, _cube, _sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _field():
    inp = synthetic_inputs(8)
    return inp['field_data'].to(_dev()), inp['forecast_h'].to(_dev())


def _stations(n, seed):
    g = np.random.default_rng(seed)
    return g.random(n) * 256.0, g.random(n) * 144.0, g.random(n) * 24.0


def _oracle_points(cube, xi, yi, hr):
    return SO.points_from_draws(cube, xi, yi, hr, 72.0, 18.0, IN_LON, IN_LAT, 6, 27000.0, 27000.0)


def _check_sampler_bars(got, want):
    x, y, t, cd, f = (v.cpu().numpy() for v in got)
    ox, oy, ot, od, of = want
    np.testing.assert_array_equal(x, ox)
    np.testing.assert_array_equal(y, oy)
    np.testing.assert_array_equal(t, ot)
    np.testing.assert_allclose(cd, od, rtol=2e-7, atol=1e-7)
    np.testing.assert_allclose(f, of, rtol=2e-7, atol=0)


# ------------------------------------------------------------------------------------------------ 1, 2: the sampler at given positions
def test_integer_positions_are_the_explicit_node_path_bitwise():
    s, _, _ = _sampler(with_labels=False)
    g = np.random.default_rng(2)
    xi, yi, ti = g.integers(0, 257, 5000), g.integers(0, 145, 5000), g.integers(0, 25, 5000)
    old = s.get_margin_grid(xi, yi, ti)
    new = s.at_positions(xi, yi, ti)
    for a, b in zip(old, new):
        assert a.shape == b.shape and torch.equal(a, b)
    # a refine-1 lattice of one hour = full_grid(h) after the (x outer, y inner) -> (y, x) reorder
    lat = s.lattice(refine=1, hours=7)
    assert (lat.nx, lat.ny, lat.nt) == (257, 145, 1)
    x, y, t, f, cd = s.sample_at(lat.n_points, lattice=lat)
    fx, fy, ft, fcd, ff = s.full_grid(7)
    reorder = lambda v: v.reshape(257, 145, *v.shape[1:]).transpose(0, 1).reshape(v.shape)
    for a, b in ((x, fx), (y, fy), (t, ft), (cd, fcd), (f, ff.reshape(-1))):
        assert torch.equal(a, reorder(b))
    # the entry point validates its arguments as its neighbours do
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    lib, c = L.load(), lat.c_struct()
    args = lambda **k: (ctypes.byref(s._s), _ptr(s.cube), k.get('xr'), None, None, k.get('lat', ctypes.byref(c)), k.get('first', 0), k.get('n', 10),
                        _ptr(x), _ptr(y), _ptr(t), _ptr(f), _ptr(cd), _stream())
    assert lib.dpn_sample_at(*args(n=0)) == -1
    assert lib.dpn_sample_at(*args(first=lat.n_points - 5)) == -1                      # first + n > nx * ny * nt
    assert lib.dpn_sample_at(*args(lat=None)) == -1                                    # neither source
    assert lib.dpn_sample_at(*args(xr=_ptr(x))) == -1                                  # one station array, and a lattice beside it
    bad = L.DpnLattice(0, 1, 0, 1, 0, 1, 257, 0, 1)
    assert lib.dpn_sample_at(*args(lat=ctypes.byref(bad))) == -1
    assert lib.dpn_fields_out(_ptr(cd), 10, ctypes.byref(L.DpnPhysics()), 0, None, None, None, 0, _stream()) == -1
    assert lib.dpn_fields_out(_ptr(cd), 10, ctypes.byref(L.DpnPhysics()), 0, _ptr(cd), _ptr(cd), ctypes.byref(c), 0, _stream()) == -1
    assert lib.dpn_residual_points(_ptr(cd), None, _ptr(f), 10, None, None, _ptr(cd), _stream()) == -1
    torch.cuda.synchronize()


def test_fractional_stations_and_a_refined_lattice_match_the_sampler_oracle():
    s, cube, _ = _sampler(with_labels=False)
    xi, yi, hr = _stations(4096, seed=7)
    x, y, t, cd, f = s.at_positions(xi, yi, hr)
    _check_sampler_bars((x, y, t, cd, f), _oracle_points(cube, xi, yi, hr))
    assert not torch.isnan(cd).any()
    # stations in degrees: the same positions after the host's fp64 conversion
    lon, la = 72.0 + xi[:512] * 0.25, 18.0 + yi[:512] * 0.25
    got = s.at_lonlat(lon, la, hr[:512])
    _check_sampler_bars(got, _oracle_points(cube, (lon - 72.0) / 0.25, (la - 18.0) / 0.25, hr[:512]))
    # refine 3, 20-minute steps, on a window (the oracle is a Python loop over scipy calls: 7 x 31 x 37 points keep it short)
    lat = s.lattice(refine=3, hours=(5.0, 1.0 / 3.0, 7), x_range=(100, 112), y_range=(40, 50))
    assert (lat.nx, lat.ny, lat.nt) == (37, 31, 7)
    px, py, pt = lat.positions()
    x, y, t, f, cd = s.sample_at(lat.n_points, lattice=lat)
    _check_sampler_bars((x, y, t, cd, f.unsqueeze(1)), _oracle_points(cube, px, py, pt))
    # chunks of the lattice (any first / n) are slices of the whole
    x2, y2, t2, f2, cd2 = s.sample_at(1000, lattice=lat, first=777)
    for a, b in ((x, x2), (y, y2), (t, t2), (f, f2), (cd, cd2)):
        assert torch.equal(a[777:1777], b)
    # outside the cube: NaN, as the oracle (the range checks of at_positions sit in front of the kernel for stations; a lattice may leave the domain)
    from deepphysinet_amd.sampler import Lattice
    out = Lattice(254.0, 0.75, 142.5, 0.75, 23.0, 0.5, 6, 5, 4)
    px, py, pt = out.positions()
    x, y, t, f, cd = s.sample_at(out.n_points, lattice=out)
    want = _oracle_points(cube, px, py, pt)
    nan = np.isnan(want[3]).any(axis=1)
    assert nan.sum() > 0 and (~nan).sum() > 0 and np.array_equal(nan, (px > 256) | (py > 144) | (pt > 24))
    assert np.array_equal(np.isnan(cd.cpu().numpy()), np.isnan(want[3]))
    np.testing.assert_allclose(cd.cpu().numpy()[~nan], want[3][~nan], rtol=2e-7, atol=1e-7)
    np.testing.assert_array_equal(x.cpu().numpy(), want[0])


# ------------------------------------------------------------------------------------------------ 3: fields
def test_station_fields_match_the_oracle():
    n = 1037
    s, cube, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    xi, yi, hr = _stations(n, seed=11)
    for clip in (False, True):
        got = m.predict_points(field, s, xi, yi, hr, fh, with_clip=clip).cpu()
        ox, oy, ot, od, _ = _oracle_points(cube, xi, yi, hr)
        tt = lambda a: torch.from_numpy(a)
        st = O.make_state()
        with torch.no_grad():
            pe = O.encoding_coord(tt(ox).reshape(-1, 1), tt(oy).reshape(-1, 1), tt(ot).reshape(-1, 1), GEO)
            want = torch.cat(O.inverse_norm(O.physics_net_forward(st, field.cpu(), pe, tt(od), fh.cpu()), with_clip=clip), dim=1)
        assert got.shape == (n, 6)
        err = ((got - want).abs().max(dim=0).values / want.abs().max(dim=0).values).numpy()
        print('predict_points vs oracle (clip %s): per-field error / maximum %s' % (clip, err))
        assert np.all(err <= TOL['bf16x2']['field']), err
    lon, la = 72.0 + xi * 0.25, 18.0 + yi * 0.25
    assert torch.equal(m.predict_points(field, s, lon, la, hr, fh, with_clip=True, lonlat=True),
                       m.predict_points(field, s, (lon - 72.0) / 0.25, (la - 18.0) / 0.25, hr, fh, with_clip=True))


# ------------------------------------------------------------------------------------------------ 4, 5: maps
def test_lattice_maps_are_the_point_fields():
    s, cube, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    x, y, t, cd, _ = s.full_grid(7)
    lat1 = s.lattice(refine=1, hours=7)
    for clip in (False, True):
        old = m.predict_grid(field, x, y, t, cd, fh, with_clip=clip)
        new = m.predict_lattice(field, s, lat1, fh, with_clip=clip)
        assert new.shape == (1, 6, 145, 257)
        assert torch.equal(new[0], old)                       # every output element of the point kernels is its own dot product: point order is immaterial
    # refine 2, 3 hours: the maps are forward_xyt on the lattice's points, de-normalised and scattered (the f3 check)
    lat = s.lattice(refine=2, hours=(3.0, 1.0, 3))
    px, py, pt, pf, pcd = s.sample_at(lat.n_points, lattice=lat)
    with torch.no_grad():
        fields = torch.cat(m.physics_net.forward_xyt(field, px, py, pt, pcd, fh), dim=1).cpu().numpy()
    cfg = m.point_config()
    for clip in (False, True):
        maps = m.predict_lattice(field, s, lat, fh, with_clip=clip).cpu().numpy()
        v = fields.astype(np.float32) * np.asarray(cfg.std, np.float32)[None] + np.asarray(cfg.mean, np.float32)[None]
        if clip:
            for k in range(2, 6):
                v[:, k] = np.clip(v[:, k], np.float32(cfg.clip_lo[k]), np.float32(cfg.clip_hi[k]))
        want = np.ascontiguousarray(v.reshape(lat.nt, lat.ny, lat.nx, 6).transpose(0, 3, 1, 2))
        np.testing.assert_array_equal(maps, want)


def test_chunking_changes_nothing_and_nan_stays_where_the_lattice_leaves_the_cube():
    from deepphysinet_amd.sampler import Lattice
    s, cube, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    lat = s.lattice(refine=2, hours=(2.0, 1.5, 5))
    whole = m.predict_lattice(field, s, lat, fh, with_clip=True)
    assert whole.shape == (5, 6, 289, 513) and bool(torch.isfinite(whole).all())
    for chunk in (4096, 513 * 100 + 300):                    # (the second splits planes mid-row: 51 600 -> 51 584 = 100 rows + 284 points)
        assert torch.equal(m.predict_lattice(field, s, lat, fh, with_clip=True, chunk_points=chunk), whole), chunk
    small = s.lattice(refine=2, hours=(2.0, 1.5, 5), x_range=(30, 60), y_range=(100, 112.5))       # 61 x 26 x 5 points in 62 chunks of 128
    ws = m.predict_lattice(field, s, small, fh, with_clip=True)
    assert torch.equal(m.predict_lattice(field, s, small, fh, with_clip=True, chunk_points=128), ws)
    assert torch.equal(ws, whole[:, :, 200:226, 60:121])    # a window of the lattice is a window of its maps
    # a lattice that leaves the cube: NaN exactly there, chunked or not
    out = Lattice(250.0, 0.5, 140.0, 0.5, 22.0, 1.0, 20, 15, 4)
    px, py, pt = out.positions()
    nan = ((px > 256) | (py > 144) | (pt > 24)).reshape(out.nt, 1, out.ny, out.nx).repeat(6, axis=1)
    a = m.predict_lattice(field, s, out, fh, with_clip=True)
    b = m.predict_lattice(field, s, out, fh, with_clip=True, chunk_points=128)
    assert np.array_equal(torch.isnan(a).cpu().numpy(), nan) and 0 < nan.sum() < nan.size
    assert torch.equal(torch.isnan(b), torch.isnan(a)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert bool(torch.isfinite(a[~torch.isnan(a)]).all())


# ------------------------------------------------------------------------------------------------ 6: residuals
@pytest.mark.parametrize('n', [1037, 5197])
def test_mean_squared_residuals_are_the_loss_terms(n):
    """loss_factor_i * mean(res_i ** 2) over residuals_at's rows = pde_loss_terms on the same points, within 2e-5 relative: the project's bar for a
    change of summation order (test_full_grid_properties) -- the residual values are the same instructions, the sums are not."""
    s, _, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    xi, yi, hr = _stations(n, seed=13)
    res = m.residuals_at(field, s, xi, yi, hr, fh)
    assert res.shape == (n, 6) and bool(torch.isfinite(res).all())
    x, y, t, cd, f = s.at_positions(xi, yi, hr)
    terms = m.pde_loss_terms(x, y, t, f, field, cd, fh).detach().double().cpu().numpy()
    lf = m.train_cfg['losses']['loss_factor']
    from deepphysinet_amd.point_path import LOSS_ORDER
    fac = np.array([lf[k] for k in LOSS_ORDER], dtype=np.float64)
    mine = fac * (res.double().cpu().numpy() ** 2).mean(axis=0)
    rel = np.abs(mine - terms) / np.abs(terms)
    print('n = %d: factor * mean(res^2) vs pde_loss_terms, relative: %s' % (n, rel))
    assert np.all(rel <= 2e-5), (rel, mine, terms)
    scaled = m.residuals_at(field, s, xi, yi, hr, fh, residual_factors=True)
    assert torch.equal(scaled, res * torch.tensor(fac, dtype=torch.float64).float().to(res.device))


# e32_J, e32_r[i] and the bars derived from them (see the docstring below); measured on the CPU on this test's own points
E32_J = 2.697e-06
E32_R = (1.937e-06, 1.971e-06, 7.232e-07, 1.129e-06, 9.151e-07, 1.381e-06)
RESIDUAL_BARS = tuple(TOL['bf16x2']['jac'] / E32_J * e for e in E32_R)


def test_per_point_residuals_match_the_fp64_oracle():
    """Every residual of residuals_at against the fp64 oracle: oracle.dpn_oracle.residual_losses called with crit = a - b returns the signed per-point
    residual times its factor (nothing is restated here).  1 037 stations at fractional positions and hours (numpy default_rng(0)).

    Bars, from the reference's own arithmetic alone (CPU): the fp32 oracle's deviation from the fp64 oracle on these points is e32_J = 2.697e-06 for
    the Jacobian (worst field, of that field's maximum) and e32_r = 1.937e-06, 1.971e-06, 7.232e-07, 1.129e-06, 9.151e-07, 1.381e-06 for the six
    residuals (of max |res_i|).  The project accepts 2e-4 for the Jacobian (TOL['bf16x2']['jac']), which these residuals are linear in, so term i
    gets the same allowance over fp32 noise: (2e-4 / e32_J) * e32_r[i] = 1.436e-04, 1.461e-04, 5.362e-05, 8.368e-05, 6.785e-05, 1.024e-04 --
    cancellation inside a term widens its bar exactly as it widens fp32's.  Points whose ReLU / clip / vapour switch differs from the fp64 oracle's
    are left out, at most 1 % of them (the cap of the parity tests; the fp32 oracle differs from the fp64 one at 2 of the 1 037)."""
    import deepphysinet_amd as dpn
    from deepphysinet_amd.point_path import LOSS_ORDER, relu_masks
    n = 1037
    s, _, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    xi, yi, hr = _stations(n, seed=0)
    res = m.residuals_at(field, s, xi, yi, hr, fh).double().cpu()
    x, y, t, cd, f = s.at_positions(xi, yi, hr)
    cfg = m.point_config()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(field, fh)
        m1, m2 = relu_masks(cfg, x, y, t, cd, heads, evec, statics)
        out_n, jac_n = dpn.pde_fields_and_jacobian(cfg, x, y, t, cd, heads, evec, statics)
    clip, delta = _clip_and_delta(out_n, jac_n, True)
    # the fp64 oracle on the device sampler's own outputs
    st = O.make_state(dtype=torch.float64)
    c = dict(x=x.cpu().double().reshape(-1, 1), y=y.cpu().double().reshape(-1, 1), t=t.cpu().double().reshape(-1, 1), f=f.cpu().double().reshape(-1, 1),
             coord_data=cd.cpu().double(), field_data=field.cpu().double(), forecast_h=fh.cpu().double())
    X, Y, T_ = (c[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    _, parts, _, _ = O.place_one_batch(st, X, Y, T_, c['f'], c['field_data'], c['coord_data'], c['forecast_h'], GEO, return_parts=True,
                                       crit=lambda a, b: a - b)
    fac = torch.tensor([O.LOSS_FACTOR[k] for k in LOSS_ORDER], dtype=torch.float64)
    want = torch.cat([p.detach() for p in parts], dim=1) / fac
    o1, o2, oclip, odelta = _oracle_masks(c, st=st)
    flipped = ((m1.cpu() != o1) | (m2.cpu() != o2)).any(dim=2).any(dim=0) | (clip != oclip).any(dim=1) | (delta != odelta)
    idx = torch.nonzero(flipped).flatten().tolist()
    print('points left out (a switch differs from the fp64 oracle): %s' % idx)
    assert len(idx) <= n // 100, idx
    keep = ~flipped
    err = ((res[keep] - want[keep]).abs().max(dim=0).values / want[keep].abs().max(dim=0).values).numpy()
    print('residuals_at vs fp64 oracle, error / max |res_i|: %s\nbars: %s' % (err, np.array(RESIDUAL_BARS)))
    assert np.all(err <= np.array(RESIDUAL_BARS)), (err, RESIDUAL_BARS)


def test_residual_lattice_is_residuals_at_on_the_lattice_points():
    s, _, _ = _sampler(with_labels=False)
    m = _model('bf16x2')
    field, fh = _field()
    lat = s.lattice(refine=2, hours=(4.0, 0.5, 3), x_range=(10, 40), y_range=(20, 35.5))
    px, py, pt = lat.positions()
    rows = m.residuals_at(field, s, px, py, pt, fh)
    want = rows.view(lat.nt, lat.ny, lat.nx, 6).permute(0, 3, 1, 2)
    assert torch.equal(m.residual_lattice(field, s, lat, fh), want)
    assert torch.equal(m.residual_lattice(field, s, lat, fh, chunk_points=256), want)


# ------------------------------------------------------------------------------------------------ 7: training is untouched
def test_inference_calls_leave_the_training_step_bitwise_alone():
    """The fused step's losses and every gradient on a fixed batch, before and after inference calls on the same model: bitwise equal.  An inference call
    between a training forward and its backward neither clears the field cache nor disturbs the state that forward saved."""
    s, _, _ = _sampler(with_labels=True)
    m = _model('bf16x2')
    field, fh = _field()
    batch = s.training_batch(field, fh, n_margin=2048, n_inter=1037)
    lf = m.train_cfg['losses']['loss_factor']
    lat = s.lattice(refine=1, hours=(0.0, 6.0, 2))
    xi, yi, hr = _stations(300, seed=5)

    def infer():
        return (m.predict_lattice(field, s, lat, fh, chunk_points=8192), m.predict_points(field, s, xi, yi, hr, fh),
                m.residuals_at(field, s, xi, yi, hr, fh), m.residual_lattice(field, s, s.lattice(hours=3, x_range=(0, 40), y_range=(0, 30)), fh))

    def step(between=None):
        from deepphysinet_amd.point_path import step_losses
        m.physics_net.zero_grad(set_to_none=True)
        b = batch
        cfg = m.point_config(lf)
        heads, evec, statics = m.physics_net.field_weights(b['field_data'], b['forecast_h'], use_cache=True)
        cat = lambda a_, b_: torch.cat([a_.reshape(a_.shape[0], -1), b_.reshape(b_.shape[0], -1)], dim=0)
        out = step_losses(cfg, b['inter_x'].shape[0], cat(b['inter_x'], b['margin_x']), cat(b['inter_y'], b['margin_y']), cat(b['inter_t'], b['margin_t']),
                          cat(b['inter_f'], b['margin_f']), cat(b['inter_data'], b['margin_input_data']), b['margin_data'], heads, evec, statics,
                          beta=0.1, margin_factor=lf['margin_factor'])
        cache = m.physics_net._meta_cache
        assert cache is not None
        if between is not None:
            between()
            assert m.physics_net._meta_cache is cache                     # the field cache is as the call found it
        (out[1] + out[3] + out[4]).backward()
        m.physics_net.clear_field_cache()
        torch.cuda.synchronize()
        return [v.detach().clone() for v in out] + [p.grad.detach().clone() for p in m.physics_net.parameters() if p.grad is not None]

    before = step()
    first = infer()
    after = step()
    mid = step(between=infer)                                             # the saved workspace of a pending backward survives an inference call
    assert len(before) == len(after) == len(mid) > 100
    for i, (a_, b_, c_) in enumerate(zip(before, after, mid)):
        assert torch.equal(a_, b_) and torch.equal(a_, c_), i
    for a_, b_ in zip(first, infer()):                                    # and inference is unmoved by the training steps in between (no optimiser ran)
        assert torch.equal(a_, b_)
    assert m.physics_net._meta_cache is None


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_train_save_and_run_inference_interface(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    ckpt, results = tmp_path / 'ckpt', tmp_path / 'results'
    cfg = ncep_config()
    cfg['train_cfg']['train_data'].update(label_batch_size=2048, batch_size_inter=1024)
    torch.manual_seed(3)
    trainer = builder_models(**cfg)
    out = trainer.run_train_interface(checkpoint_path=str(ckpt), samples='synthetic', max_steps=2, pde_start_step=0, samples_per_epoch=2, num_epoch=1)
    assert out['global_step'] == 2 and (ckpt / 'physics_latest.pth').exists()
    cfg = ncep_config()
    cfg['inference_cfg'].update(img_size=(145, 257), dt=1800)
    cfg['inference_cfg']['log'].update(write_source=True, result_path=str(results), export_variable=['T', 'u'])
    torch.manual_seed(4)
    m = builder_models(**cfg)
    m.with_clip = True
    maps = m.run_inference_interface(checkpoint_path=str(ckpt), samples='synthetic')
    nt = 49
    assert maps.shape == (nt, 6, 145, 257) and bool(torch.isfinite(maps).all())
    for (k, a), (_, b) in zip(m.physics_net.state_dict().items(), trainer.physics_net.state_dict().items()):
        assert torch.equal(a, b.to(a.device)), k
    # the files: nt per exported variable, [lat, lon], finite, T inside its clip bounds, and bitwise a direct predict_lattice call on the loaded weights
    syn = SyntheticSamples(_dev(), n_margin=128, n_inter=128, leads=1)
    b = syn[0]
    direct = m.predict_lattice(b['field_data'], syn.sampler, syn.sampler.lattice(refine=1, hours=(0.0, 0.5, nt)), b['forecast_h'], with_clip=True)
    assert torch.equal(direct, maps)
    lo, hi = m.obs_norm_cfg['t2']['bound']
    for var, col in (('T', 3), ('u', 0)):
        files = sorted(f for f in os.listdir(results) if f.endswith('_%s.npy' % var))
        assert len(files) == nt, files
        for it, fn in enumerate(files):                                  # (time stamps sort in time order)
            a = np.load(os.path.join(results, fn))
            assert a.shape == (145, 257) and a.dtype == np.float32 and np.all(np.isfinite(a))
            assert np.array_equal(a, direct[it, col].cpu().numpy()), fn
            if var == 'T':
                assert a.min() >= lo and a.max() <= hi
    assert len(os.listdir(results)) == 2 * nt
    # the launcher, in a child process of its own
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(ckpt), '--log_path', str(tmp_path / 'cli'), '--synthetic'],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert 'maps (49, 6, 145, 257), finite True' in child.stdout
    assert len(os.listdir(tmp_path / 'cli')) == nt                       # the configuration's export_variable: T
