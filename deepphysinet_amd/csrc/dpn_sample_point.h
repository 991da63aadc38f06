// One point of the collocation sampler (sample_point) and the de-normalisation of one network output (denorm), shared by the sampler unit
// (dpn_sampler.hip), the trajectory unit (dpn_traj.hip) and the window extremes of the diagnostics unit (dpn_extreme.inc in dpn_diag.hip).  Both are
// inlined into their kernels; each unit has its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dpn_hip.h"

namespace {

// One point of the sampler at position (xr, yr) in fine-grid index units and tr in hours: fp64 weights in the clamped coarse cell, NaN outside the
// cube (more than 1e-9 of a cell beyond a face), the Coriolis term, one cast to fp32.  The drawn points (dpn_sample_kernel) and the given ones (dpn_sample_at_kernel) share it.
__device__ __forceinline__ void sample_point(const DpnSampler& s, const float* cube, const double xr, const double yr, const double tr, const int64_t i,
                                             float* x, float* y, float* t, float* f, float* coord_data) {
    // trilinear interpolation of the coarse cube [6][lat_in][lon_in][t_in] at (lat, lon, hour)               (:405-411)
    const double fx = xr * s.cells_x, fy = yr * s.cells_y, ft = tr / s.t_step_hours;
    int ix = (int)floor(fx), iy = (int)floor(fy), it = (int)floor(ft);
    ix = ix < 0 ? 0 : (ix > s.lon_in - 2 ? s.lon_in - 2 : ix);
    iy = iy < 0 ? 0 : (iy > s.lat_in - 2 ? s.lat_in - 2 : iy);
    it = it < 0 ? 0 : (it > s.t_in - 2 ? s.t_in - 2 : it);
    double wx = fx - ix, wy = fy - iy, wt = ft - it;
    // Inside: every weight within 1e-9 of [0, 1], then clamped to [0, 1]; anything further out -> NaN (xarray).  A position on the cube's last face
    // can come out an ulp or two of fx beyond it when cells_x is no binary fraction (0.1 / 0.3); that excess is below 5e-10 up to 2^20 cells, and
    // 1e-9 of a cell moves the result by 1e-9 of the corner spread.  The clamp is the identity on weights already in [0, 1].
    const double tol = 1e-9;
    const bool inside = wx >= -tol && wx <= 1.0 + tol && wy >= -tol && wy <= 1.0 + tol && wt >= -tol && wt <= 1.0 + tol;   // (a NaN fails)
    wx = fmin(fmax(wx, 0.0), 1.0); wy = fmin(fmax(wy, 0.0), 1.0); wt = fmin(fmax(wt, 0.0), 1.0);
    const int64_t sy = (int64_t)s.lon_in * s.t_in, sx = s.t_in, sk = (int64_t)s.lat_in * sy;
    const float* c0 = cube + (int64_t)iy * sy + (int64_t)ix * sx + it;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float* c = c0 + k * sk;
        const double v000 = c[0], v001 = c[1], v010 = c[sx], v011 = c[sx + 1];
        const double v100 = c[sy], v101 = c[sy + 1], v110 = c[sy + sx], v111 = c[sy + sx + 1];
        const double lo = (v000 * (1 - wt) + v001 * wt) * (1 - wx) + (v010 * (1 - wt) + v011 * wt) * wx;
        const double hi = (v100 * (1 - wt) + v101 * wt) * (1 - wx) + (v110 * (1 - wt) + v111 * wt) * wx;
        coord_data[i * 6 + k] = inside ? (float)(lo * (1 - wy) + hi * wy) : __builtin_nanf("");
    }
    const double lat_deg = s.begin_lat + yr * s.dlat;
    x[i] = (float)(xr * (double)s.dx);
    y[i] = (float)(yr * (double)s.dy);
    t[i] = (float)(tr * 3600.0);
    f[i] = (float)(2.0 * 7.29e-5 * sin(lat_deg / 180.0 * 3.141592653589793));                           // get_coriolis (:521-526)
}

// inverse_norm (:232-262) of one normalised value of variable k: two roundings (mul, then add) like the reference's `v * std + mean` in torch -- not
// contracted into one fma --, the three-factor min_max form, and the clip of P, T, q, rho.
__device__ __forceinline__ float denorm(const float out, const int k, const DpnPhysics& ph, const int with_clip) {
    float v;
    {
#pragma clang fp contract(off)
        const float prod = out * ph.std[k];
        v = prod + ph.mean[k];
        if (ph.sq_on[k]) { const float sq = v * v; v = sq + ph.sq_add[k]; }       // three-factor min_max (interface_physics.py:244-247)
    }
    if (with_clip && k >= 2) v = v != v ? v : fminf(fmaxf(v, ph.clip_lo[k]), ph.clip_hi[k]);      // NaN passes through like torch.clip
    return v;
}

}  // namespace
