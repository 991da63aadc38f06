"""Derived diagnostics from the fields and their coordinate Jacobian (csrc/dpn_diag.hip): the product names and the host
restatement of what the kernel defines, in numpy.

The forward kernel gives, at any point, the six normalised fields and their 6 x 3 Jacobian with respect to x (m), y (m), t (s).  dpn_diagnostics_out
de-normalises both with the residual body (`denorm_reference`) and forms the products of the table in include/dpn_hip.h (`diagnostics_reference`):
the 18 derivatives themselves, relative and absolute vorticity, divergence, Dp/Dt, temperature and moisture advection, moisture-flux divergence, wind
speed, relative humidity and total deformation.  With dtype=np.float32 the two functions follow the kernel's order of operations, one rounding per
operation -- the kernel is compiled without contraction, so every product that does not go through expf agrees bit for bit --; with np.float64 they
are the truth the GPU tests measure against.  Nothing here runs in inference.
"""
import numpy as np

VARIABLES = ('u', 'v', 'p', 'T', 'q', 'rho')          # k = 0..5, the order of the network's outputs
COORDINATES = ('x', 'y', 't')                         # c = 0..2
PRODUCTS = tuple('d%s_d%s' % (k, c) for k in VARIABLES for c in COORDINATES) + (
    'vorticity', 'abs_vorticity', 'divergence', 'omega', 't_advection', 'q_advection', 'q_flux_divergence', 'speed', 'rel_humidity', 'deformation')
_IDS = {name: i for i, name in enumerate(PRODUCTS)}


def product_ids(names):
    """The ids (column selectors of dpn_diagnostics_out) of a sequence of product names, repeats and order kept; KeyError on an unknown name."""
    ids = []
    for n in names:
        if n not in _IDS:
            raise KeyError('diagnostic product %r: one of %s' % (n, ', '.join(PRODUCTS)))
        ids.append(_IDS[n])
    if not ids:
        raise KeyError('no diagnostic product named; known: %s' % ', '.join(PRODUCTS))
    return ids


def denorm_reference(out_n, jac_n, physics, with_clip=False, dtype=np.float32):
    """The residual body's val [n, 6], msk [n, 6] and J [n, 6, 3] (csrc/dpn_residual_body.inc) from normalised fields out_n [n, 6] and their Jacobian
    jac_n [n, 6, 3]: val = out * std + mean; the squared min_max form val = val * val + sq_add with d val / d out = (2 * val) * std; with_clip, where
    physics.clip_on[k]: the mask 1 inside [lo, hi], 0 outside (and for a NaN), val clamped (a NaN goes to lo, as fminf(fmaxf(.)) sends it);
    msk = mask * d val / d out; J = jac_n * msk.  physics: a DpnPhysics (or anything with its mean, std, clip_lo, clip_hi, clip_on, sq_on, sq_add);
    its fp32 constants are taken as they are.  Every operation is one operation of `dtype`."""
    dt = np.dtype(dtype).type
    o = np.asarray(out_n, dtype=np.float32).astype(dt)
    jn = np.asarray(jac_n, dtype=np.float32).astype(dt).reshape(o.shape[0], 6, 3)
    val, msk = np.empty_like(o), np.empty_like(o)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(6):
            std, mean = dt(np.float32(physics.std[k])), dt(np.float32(physics.mean[k]))
            v = o[:, k] * std + mean
            dv = np.full_like(v, std)
            if physics.sq_on[k]:
                dv = dt(2.0) * v * std
                v = v * v + dt(np.float32(physics.sq_add[k]))
            m = np.ones_like(v)
            if with_clip and physics.clip_on[k]:
                lo, hi = dt(np.float32(physics.clip_lo[k])), dt(np.float32(physics.clip_hi[k]))
                m = ((v >= lo) & (v <= hi)).astype(dt)
                v = np.fmin(np.fmax(v, lo), hi)
            val[:, k], msk[:, k] = v, m * dv
        J = jn * msk[:, :, None]
    return val, msk, J


def nan_rows(out_n):
    """bool [n]: the points with a NaN among their six normalised fields, which dpn_diagnostics_out writes as NaN in every product (a lattice point
    outside the coarse cube: the forward kernel's Jacobian is finite there, and the clip sends a NaN value to its lower bound)."""
    return np.isnan(np.asarray(out_n, dtype=np.float32)).any(axis=1)


def diagnostics_reference(val, J, f, names, dtype=np.float32, nan_rows=None):
    """The products `names` [n, P] from val [n, 6], J [n, 6, 3] (denorm_reference) and the Coriolis parameter f [n]: the table of include/dpn_hip.h, each
    line one operation of `dtype`, left to right as written there.  nan_rows (bool [n], the function of that name on out_n): those rows are NaN in
    every product, as the kernel writes them."""
    dt = np.dtype(dtype).type
    ids = product_ids(names)
    val, J = np.asarray(val).astype(dt), np.asarray(J).astype(dt)
    fc = np.asarray(f, dtype=np.float32).reshape(-1).astype(dt)
    u, v, p, T, q = (val[:, k] for k in range(5))
    out = np.empty((val.shape[0], len(ids)), dtype=dt)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        zeta = J[:, 1, 0] - J[:, 0, 1]
        div = J[:, 0, 0] + J[:, 1, 1]
        adv_T = u * J[:, 3, 0] + v * J[:, 3, 1]
        adv_q = u * J[:, 4, 0] + v * J[:, 4, 1]
        stretch, shear = J[:, 0, 0] - J[:, 1, 1], J[:, 1, 0] + J[:, 0, 1]
        for j, i in enumerate(ids):
            if i < 18:
                o = J[:, i // 3, i % 3]
            elif i == 18:
                o = zeta
            elif i == 19:
                o = zeta + fc
            elif i == 20:
                o = div
            elif i == 21:
                o = (J[:, 2, 2] + u * J[:, 2, 0]) + v * J[:, 2, 1]
            elif i == 22:
                o = -adv_T
            elif i == 23:
                o = -adv_q
            elif i == 24:
                o = q * div + adv_q
            elif i == 25:
                o = np.sqrt(u * u + v * v)
            elif i == 26:
                o = q / saturation_humidity(p, T, dt)
            else:
                o = np.sqrt(stretch * stretch + shear * shear)
            out[:, j] = o
    if nan_rows is not None:
        out[np.asarray(nan_rows, dtype=bool)] = np.nan
    return out


def saturation_humidity(p, T, dtype=np.float32, e_s_unit=100.0):
    """q_s of the residual body (the reference's get_qs, interface_physics.py:181-185): e_s = 6.112 exp(17.67 tc / (tc + 243.5)) hPa, times 100 -> Pa;
    q_s = max(0.622 e_s / (p - 0.378 e_s), 1e-6), a NaN passing through.  e_s_unit is the hPa -> Pa factor (the tests seed a mistake through it)."""
    dt = np.dtype(dtype).type
    p, T = np.asarray(p).astype(dt), np.asarray(T).astype(dt)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        tc = T - dt(273.15)
        e_s = dt(6.112) * np.exp(dt(17.67) * tc / (tc + dt(243.5))) * dt(e_s_unit)
        qs_raw = dt(0.622) * e_s / (p - dt(0.378) * e_s)
        return np.maximum(qs_raw, dt(1e-6))                  # np.maximum propagates NaN, as the body does
