"""CPU: the host side of inference at stations and on lattices -- the C ABI additions (dpn_sample_at, dpn_fields_out, dpn_residual_points, DpnLattice),
Lattice / refine arithmetic and point order, the degrees -> index conversion, the range checks, chunk rounding, and run_inference_interface's
reading of a checkpoint.  Nothing here touches a GPU (the kernels themselves: tests/test_gpu_inference.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dpn_sample_at', 'dpn_fields_out', 'dpn_residual_points')


class _HostSampler:
    """CollocationSampler's host-side methods on a sampler that owns no device cube (its constructor refuses host tensors)."""

    def __new__(cls, cfg=None):
        from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
        s = object.__new__(CollocationSampler)
        s.cfg = cfg or SamplerConfig()
        s._s = s.cfg.c_struct()
        s.cube = torch.zeros(1)
        return s


def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert 'typedef struct DpnLattice' in header


def test_lattice_struct_has_the_c_compilers_layout(tmp_path):
    from deepphysinet_amd import _lib
    st = _lib.DpnLattice
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(DpnLattice));']
    want = {'size': ctypes.sizeof(st)}
    for f in st._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(DpnLattice, %s));' % (f[0], f[0]))
        want[f[0]] = getattr(st, f[0]).offset
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'lattice.c', tmp_path / 'lattice'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert got == want and got['size'] == 64 and got['nx'] == 48


def test_sampler_config_gains_begin_lon_as_its_last_field():
    import dataclasses
    from deepphysinet_amd.sampler import SamplerConfig
    fields = [f.name for f in dataclasses.fields(SamplerConfig)]
    assert fields[-1] == 'begin_lon' and SamplerConfig().begin_lon == 72.0
    assert SamplerConfig(257, 145, 65, 37, 6, 4, 0.25, 1.0, 18.0, 27000.0, 27000.0).begin_lon == 72.0      # positional callers keep working
    assert ctypes.sizeof(SamplerConfig().c_struct()) == 6 * 4 + 5 * 8 + 2 * 4                             # the C struct did not grow


def test_lattice_refine_arithmetic_and_point_order():
    from deepphysinet_amd.sampler import Lattice
    s = _HostSampler()
    for r in (1, 2, 3, 4):
        lat = s.lattice(refine=r, hours=(0.0, 1.0 / 3.0, 7))
        assert (lat.nx, lat.ny, lat.nt) == (256 * r + 1, 144 * r + 1, 7)
        assert lat.xstep == 1.0 / r and lat.ystep == 1.0 / r and lat.x0 == 0.0 and lat.y0 == 0.0
        assert lat.n_points == lat.nx * lat.ny * 7
        assert lat.x0 + (lat.nx - 1) * lat.xstep == 256.0 and lat.y0 + (lat.ny - 1) * lat.ystep == 144.0
    lat = s.lattice(refine=3, hours=(2.0, 1.0 / 3.0, 4), x_range=(10, 12), y_range=(5.0, 5.5))
    assert (lat.x0, lat.nx, lat.y0, lat.ny) == (10.0, 7, 5.0, 2)
    # point order (it, iy, ix), ix fastest: numpy's meshgrid with indexing='ij' over (t, y, x)
    x, y, t = lat.positions()
    T, Y, X = np.meshgrid(2.0 + np.arange(4) * (1.0 / 3.0), 5.0 + np.arange(2) * (1.0 / 3.0), 10.0 + np.arange(7) * (1.0 / 3.0), indexing='ij')
    assert np.array_equal(x, X.reshape(-1)) and np.array_equal(y, Y.reshape(-1)) and np.array_equal(t, T.reshape(-1))
    g = (3 * lat.ny + 1) * lat.nx + 5
    assert (x[g], y[g], t[g]) == (10.0 + 5 * (1.0 / 3.0), 5.0 + 1.0 / 3.0, 2.0 + 3 * (1.0 / 3.0))
    # hours as a sequence / one hour / a tuple
    assert (s.lattice(hours=[3, 6, 9]).t0, s.lattice(hours=[3, 6, 9]).tstep, s.lattice(hours=[3, 6, 9]).nt) == (3.0, 3.0, 3)
    assert (s.lattice(hours=range(25)).tstep, s.lattice(hours=range(25)).nt) == (1.0, 25)
    assert (s.lattice(hours=7).t0, s.lattice(hours=7).nt) == (7.0, 1)
    with pytest.raises(ValueError):
        s.lattice(hours=[0, 1, 3])
    with pytest.raises(ValueError):
        s.lattice(refine=0)
    with pytest.raises(ValueError):
        Lattice(0, 1, 0, 1, 0, 1, 4, 0, 1)
    c = lat.c_struct()
    assert (c.x0, c.xstep, c.y0, c.ystep, c.t0, c.tstep, c.nx, c.ny, c.nt) == (10.0, 1.0 / 3.0, 5.0, 1.0 / 3.0, 2.0, 1.0 / 3.0, 7, 2, 4)


def test_lonlat_conversion_is_fp64_on_the_host():
    from deepphysinet_amd.sampler import SamplerConfig
    s = _HostSampler()
    lon, lat = np.array([72.0, 72.25, 100.1, 136.0]), np.array([18.0, 18.25, 33.3, 54.0])
    xi, yi = s.lonlat_to_index(lon, lat)
    assert xi.dtype == np.float64 and np.array_equal(xi, (lon - 72.0) / 0.25) and np.array_equal(yi, (lat - 18.0) / 0.25)
    assert xi[0] == 0.0 and xi[1] == 1.0 and xi[3] == 256.0 and yi[3] == 144.0
    s2 = _HostSampler(SamplerConfig(begin_lon=-10.0, begin_lat=35.0, out_res_deg=0.5, in_res_deg=2.0))
    xi, yi = s2.lonlat_to_index([-9.0], [36.25])
    assert xi[0] == 2.0 and yi[0] == 2.5


@pytest.mark.parametrize('x,y,h', [([257.0], [0.0], [0.0]), ([256.0001], [0.0], [0.0]), ([-0.5], [0.0], [0.0]), ([0.0], [144.5], [0.0]), ([0.0], [-1e-9], [0.0]),
                                   ([0.0], [0.0], [24.01]), ([0.0], [0.0], [-1.0]), ([float('nan')], [0.0], [0.0])])
def test_positions_outside_the_domain_raise_index_error(x, y, h):
    s = _HostSampler()
    with pytest.raises(IndexError):
        s.at_positions(x, y, h)
    with pytest.raises(IndexError):
        s.at_lonlat(72.0 + 0.25 * np.asarray(x), 18.0 + 0.25 * np.asarray(y), h)


def test_positions_inside_the_domain_pass_the_checks_and_need_a_device():
    s = _HostSampler()
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # range checks passed: the next thing is the kernel, which refuses host tensors
        s.at_positions([0.0, 256.0, 13.7], [144.0, 0.0, 99.9], [24.0, 0.0, 5.25])
    with pytest.raises(ValueError):
        s.at_positions([0.0, 1.0], [0.0], [0.0])


def test_chunks_are_multiples_of_the_kernels_padding_unit():
    from deepphysinet_amd import _lib
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics as IP
    sizes = _lib.DpnSizes()
    assert _lib.load().dpn_sizes(1, 2, ctypes.byref(sizes)) == 0 and sizes.n_pad == 128
    n = 15_000_000
    assert IP.chunk_size(n, 128) == 128 and IP.chunk_size(n, 255) == 128 and IP.chunk_size(n, 4096) == 4096
    assert IP.chunk_size(n, 513 * 289 + 77) == (513 * 289 + 77) // 128 * 128
    assert IP.chunk_size(n, 5) == 128                                    # never below one unit
    assert IP.chunk_size(1000, 4096) == 1000 and IP.chunk_size(1000, None) == 1000      # a lattice smaller than a chunk is one chunk
    with pytest.raises(ValueError):
        IP.chunk_size(n, 0)
    # the default: what the stated budget of per-point buffers holds -- far below a 15 M-point lattice, and a multiple of the unit
    d = IP.chunk_size(n)
    assert d % 128 == 0 and d * IP.FIELD_POINT_BYTES <= IP.INFER_BUDGET_BYTES < (d + 128) * IP.FIELD_POINT_BYTES and d < n // 3
    dr = IP.chunk_size(n, None, IP.RESIDUAL_POINT_BYTES)
    assert dr % 128 == 0 and dr * IP.RESIDUAL_POINT_BYTES <= IP.INFER_BUDGET_BYTES and dr < d


def test_inference_config_carries_the_reference_keys():
    from deepphysinet_amd.configs import ncep_config
    ic = ncep_config()['inference_cfg']
    for k in ('batch_size', 'device', 'num_epoch', 'num_workers', 'dt', 'img_size', 'pred_t_span', 'start_time', 'end_time', 'checkpoints', 'log'):
        assert k in ic, k
    for k in ('with_vis', 'vis_path', 'result_path', 'write_source', 'export_variable', 'vis_downscale_cfg'):
        assert k in ic['log'], k
    assert ic['checkpoints']['checkpoints_path'] and ic['log']['result_path'] and '\\' not in ic['checkpoints']['checkpoints_path']
    assert ncep_config(img_size=(37, 65))['inference_cfg']['img_size'] == (37, 65)


def test_run_inference_interface_reads_the_checkpoints_own_normalisation_and_span(tmp_path, capsys):
    """A checkpoint written by save_model with obs_norm_cfg / pred_t_span of its own: run_inference_interface takes both from it (:1450-1452), loads
    the weights strictly, and -- given no samples -- returns None without touching a GPU."""
    import copy
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(0)
    trained = builder_models(**ncep_config())
    norm = copy.deepcopy(trained.obs_norm_cfg)
    norm['t2']['norm_factor'] = [280.0, 11.0]
    norm['t2']['bound'] = [200, 330]
    trained.save_model(str(tmp_path), epoch=4, global_step=99, prefix='physics', pred_t_span=43200.0, obs_norm_cfg=norm, dx=27000.0)
    torch.manual_seed(1)
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False, with_vis=True)
    m = builder_models(**cfg)
    assert m.pred_t_span == 86400.0 and m.obs_norm_cfg['t2']['norm_factor'] != [280.0, 11.0]
    out = m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[])
    assert out is None
    assert m.pred_t_span == 43200.0 and m.obs_norm_cfg == norm
    pc = m.point_config()
    assert pc.pred_t_span == 43200.0 and pc.mean[3] == 280.0 and pc.std[3] == 11.0 and (pc.clip_lo[3], pc.clip_hi[3]) == (200.0, 330.0)
    for (k, a), (_, b) in zip(m.physics_net.state_dict().items(), trained.physics_net.state_dict().items()):
        assert torch.equal(a, b), k
    assert 'not built' in capsys.readouterr().out                        # with_vis: one line, and the run continues
    # a checkpoint without the keys leaves the configuration's values; a missing checkpoint raises like the reference (:1453-1454)
    bare = tmp_path / 'bare'
    bare.mkdir()
    trained.save_model(str(bare), epoch=0, global_step=1, prefix='physics')
    m2 = builder_models(**cfg)
    m2.run_inference_interface(checkpoint_path=str(bare), device='cpu', samples=[])
    assert m2.pred_t_span == 86400.0 and m2.obs_norm_cfg == cfg['obs_norm_cfg']
    with pytest.raises(NotImplementedError):
        m2.run_inference_interface(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(RuntimeError, match='samples'):
        m2.run_inference_interface(checkpoint_path=str(bare), device='cpu')


def test_inference_entry_points_refuse_cpu_tensors():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    s = _HostSampler()
    field, fh = torch.zeros(1, 159, 2405), torch.zeros(1, 1, 1)
    lat = s.lattice(hours=0)
    for call in (lambda: m.predict_points(field, s, [1.5], [2.5], [3.5], fh), lambda: m.residuals_at(field, s, [1.5], [2.5], [3.5], fh),
                 lambda: m.predict_lattice(field, s, lat, fh), lambda: m.residual_lattice(field, s, lat, fh)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
