"""Shared by tests/test_diagnostics_cpu.py and tests/test_gpu_diagnostics.py: the constants behind the end-to-end bars of the derived diagnostics
(dpn_diagnostics_out), the bars themselves, and the seeded mistakes.

Constants -- printed by `python tools/diagnostics_bars.py` (CPU; the fp32 oracle against the fp64 oracle at the 1 037 fractional stations of numpy
default_rng(0), the 2 points whose switches differ left out; each relative to the column's maximum):
  E32_J      the Jacobian of the normalised fields, worst field: the value tests/test_gpu_inference.py already uses;
  E32_FIELD  the six de-normalised fields, worst field;
  E32_D[i]   product i of deepphysinet_amd.diagnostics.PRODUCTS.
Bars: the project accepts TOL['bf16x2']['jac'] = 2e-4 for the Jacobian and TOL['bf16x2']['field'] = 5e-5 for the fields.  A product linear in the
Jacobian (ids 0-24 and 27) gets the Jacobian's allowance over fp32 noise, (2e-4 / E32_J) * E32_D[i]; speed and rel_humidity depend on the fields
alone and get the fields', (5e-5 / E32_FIELD) * E32_D[i].  Cancellation inside a product widens its bar exactly as it widens fp32's."""
import numpy as np

E32_J = 2.697e-06
E32_FIELD = 1.729e-06
E32_D = (1.160e-06, 1.056e-06, 1.604e-06, 9.115e-07, 5.130e-07, 3.959e-07, 1.710e-06, 1.780e-06, 1.697e-06, 1.227e-06, 2.215e-06, 2.923e-06, 6.603e-07,
         9.124e-07, 1.051e-06, 1.394e-06, 9.673e-07, 2.611e-06, 1.086e-06, 4.137e-07, 6.498e-07, 2.182e-06, 3.703e-06, 8.201e-07, 6.212e-07, 1.389e-06,
         9.998e-06, 5.638e-07)
TOL_JAC, TOL_FIELD = 2e-4, 5e-5                     # tests/test_gpu_parity.py TOL['bf16x2'] (the GPU test asserts that they are these)
FIELD_ONLY_IDS = (25, 26)                           # speed, rel_humidity


def oracle_bars():
    """bar[i], of max |product i|, for the 28 products."""
    return np.array([(TOL_FIELD / E32_FIELD if i in FIELD_ONLY_IDS else TOL_JAC / E32_J) * e for i, e in enumerate(E32_D)])


def rel_humidity_bar(rh32, rh64):
    """The bar of the kernel's rel_humidity against the fp64 restatement on the same inputs (it goes through expf and two divisions, so it is not
    compared bitwise): 4 x the fp32 restatement's own deviation, both relative to max |rh|.  The factor allows the device expf a few ulp where numpy's
    has one; a wrong constant or unit is orders of magnitude above it.  -> (bar, the fp32 restatement's deviation)."""
    fin = np.isfinite(rh64)
    dev = np.abs(rh32.astype(np.float64)[fin] - rh64[fin]).max() / np.abs(rh64[fin]).max()
    return 4.0 * dev, dev


def seeded_mistakes(val, J, f, dtype=np.float32):
    """{product name: a wrong column [n]}: what a kernel with one plausible mistake would write, in `dtype`."""
    from deepphysinet_amd.diagnostics import saturation_humidity
    dt = np.dtype(dtype).type
    val, J = np.asarray(val).astype(dt), np.asarray(J).astype(dt)
    with np.errstate(all='ignore'):
        return {'vorticity': J[:, 0, 1] - J[:, 1, 0],                                # the sign swapped
                'divergence': J[:, 0, 1] + J[:, 1, 0],                               # x and y exchanged
                'abs_vorticity': J[:, 1, 0] - J[:, 0, 1],                            # without f
                'rel_humidity': val[:, 4] / saturation_humidity(val[:, 2], val[:, 3], dt, e_s_unit=1.0)}      # e_s left in hPa
