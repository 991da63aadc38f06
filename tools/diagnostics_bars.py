"""The constants behind the bars of tests/test_gpu_diagnostics.py::test_diagnostics_match_the_fp64_oracle, from the reference's own arithmetic alone
(CPU only; the only file of the diagnostics feature that imports oracle/ besides the tests).

At the 1 037 fractional stations of numpy default_rng(0) (the points of test_per_point_residuals_match_the_fp64_oracle; positions through
oracle/sampler_oracle.py) the oracle runs twice, in fp32 and in fp64: forward, inverse_norm without the clip, jacobian_fields, then
deepphysinet_amd.diagnostics.diagnostics_reference in the same precision.  Points whose ReLU, clip or vapour switch differs between the two are left out
(the rule of that test).  Printed:
  e32_J      the fp32 oracle's Jacobian of the normalised fields against the fp64 one, worst field, of that field's maximum (the test of the residuals
             states 2.697e-06: a check that this tool measures the way that constant was measured);
  e32_field  the same for the six de-normalised fields;
  e32_d[i]   the same for product i, of max |product i|.

usage: python tools/diagnostics_bars.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SEED = 1037, 0


def stations(n=N, seed=SEED):
    g = np.random.default_rng(seed)
    return g.random(n) * 256.0, g.random(n) * 144.0, g.random(n) * 24.0


def oracle_inputs(dtype):
    from oracle import sampler_oracle as SO
    from oracle.fill import synthetic_inputs
    from tests.test_sampler import IN_LAT, IN_LON, _cube
    xi, yi, hr = stations()
    ox, oy, ot, od, of = SO.points_from_draws(_cube(), xi, yi, hr, 72.0, 18.0, IN_LON, IN_LAT, 6, 27000.0, 27000.0)
    inp = synthetic_inputs(8)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return dict(x=tt(ox).reshape(-1, 1), y=tt(oy).reshape(-1, 1), t=tt(ot).reshape(-1, 1), f=tt(of).reshape(-1, 1), coord_data=tt(od),
                field_data=inp['field_data'].to(dtype), forecast_h=inp['forecast_h'].to(dtype))


def oracle_run(dtype):
    """(inputs, out_n [n, 6], jac_n [n, 6, 3], val [n, 6], J [n, 6, 3]) of the oracle in `dtype`, without the clip."""
    from oracle import dpn_oracle as O
    from tests.test_gpu_parity import GEO
    c = oracle_inputs(dtype)
    st = O.make_state(dtype=dtype)
    x, y, t = (c[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
    fields_n = O.physics_net_forward(st, c['field_data'], O.encoding_coord(x, y, t, GEO), c['coord_data'], c['forecast_h'])
    fields = O.inverse_norm(fields_n, with_clip=False)
    jac_n = O.jacobian_fields(x, y, t, fields_n).detach()
    J = O.jacobian_fields(x, y, t, fields).detach()
    return c, st, torch.cat(fields_n, 1).detach(), jac_n, torch.cat(fields, 1).detach(), J


def rel_max(a, b, axis=0):
    """max |a - b| / max |b| along `axis`."""
    return np.abs(a - b).max(axis=axis) / np.abs(b).max(axis=axis)


def main():
    from deepphysinet_amd.diagnostics import PRODUCTS, diagnostics_reference
    from tests.test_gpu_parity import _oracle_masks
    c32, _, on32, jn32, v32, J32 = oracle_run(torch.float32)
    c64, st64, on64, jn64, v64, J64 = oracle_run(torch.float64)
    a = _oracle_masks(c32)
    b = _oracle_masks(c64, st=st64)
    flipped = ((a[0] != b[0]) | (a[1] != b[1])).any(dim=2).any(dim=0) | (a[2] != b[2]).any(dim=1) | (a[3] != b[3])
    keep = (~flipped).numpy()
    print('points where a switch of the fp32 oracle differs from the fp64 oracle: %s (%d of %d; cap %d)'
          % (torch.nonzero(flipped).flatten().tolist(), int(flipped.sum()), N, N // 100))
    e_j = rel_max(jn32.double().numpy()[keep].reshape(-1, 6, 3), jn64.numpy()[keep].reshape(-1, 6, 3), axis=(0, 2))
    e_f = rel_max(v32.double().numpy()[keep], v64.numpy()[keep])
    print('e32_J     = %.3e   (per field: %s)' % (e_j.max(), ' '.join('%.3e' % e for e in e_j)))
    print('e32_field = %.3e   (per field: %s)' % (e_f.max(), ' '.join('%.3e' % e for e in e_f)))
    f = c32['f'].numpy().reshape(-1)
    d32 = diagnostics_reference(v32.numpy(), J32.numpy(), f, PRODUCTS, np.float32).astype(np.float64)
    d64 = diagnostics_reference(v64.numpy(), J64.numpy(), f, PRODUCTS, np.float64)
    e_d = rel_max(d32[keep], d64[keep])
    for i, name in enumerate(PRODUCTS):
        print('e32_d[%2d] %-18s %.3e   (max |product| %.3e)' % (i, name, e_d[i], np.abs(d64[keep, i]).max()))
    print('E32_D = (%s)' % ', '.join('%.3e' % e for e in e_d))


if __name__ == '__main__':
    main()
