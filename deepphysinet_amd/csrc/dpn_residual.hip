// MI355X (gfx950 / CDNA4) point path, the losses on the point kernels' outputs.  A unit of its own.
//
// Reference behaviour restated here (paths relative to the reference's DeepPhysiNet tree):
//   interface/interface_physics.py:97-185   six residual losses
//   interface/interface_physics.py:232-262  inverse_norm (+clip)
//
// Kernel inventory
//   dpn_contract_gpe_kernel     cotangent of caller-encoded coordinates
//   dpn_residual_kernel<Args>   de-norm, clip, six residuals, wave-shuffle loss reduction, analytic cotangents; instantiated for ResArgs
//                               (dpn_residual), for ResWArgs (dpn_residual_weighted: a weight per point in the sums and the cotangents) and for
//                               ResStepArgs (dpn_step_residual: the [interior | margin] rows of a step in one launch, + the data loss)
//   dpn_residual_points_kernel  the same residual body, written out per point (inference diagnostics)
//   dpn_residual_finish_kernel  block rows -> the six scaled losses and their sum
//   dpn_step_finish_kernel      dpn_step_residual's block rows of B fields -> per field both groups' losses, the data loss, the step's total
//   dpn_smooth_l1_kernel        the data loss and its cotangent
// No kernel in this file uses atomics: every reduction is fixed-order, the whole step is bitwise reproducible.
#include "dpn_device.h"
#include "dpn_criterion.h"

// g_pe[n][c] = sum_k g_out[n][k] * gpe[n][k][c]: the cotangent of caller-encoded coordinates (PhysicsNet.forward backward w.r.t. coord_x)
__global__ __launch_bounds__(192) void dpn_contract_gpe_kernel(const float* g_out, const float* gpe, int64_t n, float* g_pe) {
    const int64_t pt = blockIdx.x;
    const int c = threadIdx.x;
    float s_ = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) s_ = fmaf(g_out[pt * 6 + k], gpe[(pt * 6 + k) * kPe + c], s_);
    g_pe[pt * kPe + c] = s_;
}

// ------------------------------------------------------------------------------------------------ residuals
struct ResArgs {
    const float *out_n, *jac_n, *f;
    int64_t n;
    DpnGeometry geo;
    DpnPhysics ph;
    const float *gl, *gtot;
    double* loss_sums;
    float *g_out, *g_jxi;
    static constexpr bool weighted = false, step = false;
};
// + the point weight wt_i = w[i] * bin_w[bin[i]]; either source may be absent (1.0f)
struct ResWArgs : ResArgs {
    const float* w;
    const int32_t* bin;
    const float* bin_w;
    static constexpr bool weighted = true;
};

// The step body of one field (dpn_step_residual): n = all rows, the first n_inter interior, the rest margin points with labels [n - n_inter][6].
// Blocks 0 .. nb_inter - 1 hold the interior points, the others the margin points from row n_inter on: no block straddles the boundary.
struct ResStepArgs : ResArgs {
    const float* labels;
    int64_t n_inter, nb_inter;
    float data_beta, data_scale;
    static constexpr bool step = true;
};

DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One kernel, three instantiations.  The weighted one differs in `wt` alone: in the fp64 block sums and in inv_n, the last factor of g[e], the head of
// the cotangent chain (everything behind g[e] is linear in it); with every weight 1.0f its block rows and cotangents are bitwise the unweighted
// one's.  The template is on the __global__ function itself: through a shared device function the compiler loads the argument struct wholesale
// and both instruction streams change.
// The step one (ResStepArgs) differs in where a block's points lie (first, n_grp: the rows of the block's own group, whose 1 / n the cotangent takes),
// in a seventh column of the block row (the fp64 sum of SmoothL1(data_beta) over the block's margin points x 6 variables against the labels:
// elements of a point in order, shuffle tree, waves in order; 0.0 from an interior block), and on margin rows in the data cotangent
// data_scale * gtot[0] * slope added behind the finished PDE cotangent -- dpn_smooth_l1_kernel's expressions, its accumulate form's one addition.  The
// six criterion sums and the PDE cotangents are bitwise what dpn_residual writes for each group's slice.
template <class Args> __global__ __launch_bounds__(256) void dpn_residual_kernel(Args a) {
    constexpr int ROW = Args::step ? 7 : 6;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t n_grp = a.n, end = a.n;                 // the group's point count; one past the group's last row
    [[maybe_unused]] bool margin = false;
    if constexpr (Args::step) {
        margin = (int64_t)blockIdx.x >= a.nb_inter;
        if (margin) { i = a.n_inter + (((int64_t)blockIdx.x - a.nb_inter) * 256 + threadIdx.x); n_grp = a.n - a.n_inter; }
        else n_grp = end = a.n_inter;
    }
    const bool valid = i < end;
    const int64_t ic = valid ? i : end - 1;
#include "dpn_residual_body.inc"
    float wt = 1.f;
    if constexpr (Args::weighted) wt = (a.w ? a.w[ic] : 1.f) * (a.bin ? a.bin_w[a.bin[ic]] : 1.f);
    if (a.loss_sums) {
        // fp64 partial sums (residual^2 spans 1e-20..1e+20 across equations): wave shuffle tree, then the four waves of the block
        // in a fixed order -> one [6] row per block.  No atomics: dpn_residual_finish adds the rows in a fixed order, so the
        // losses are run-to-run deterministic (and 3.5k serialised fp64 atomics are gone from the step).
        __shared__ double wsum[4][ROW];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
#pragma clang fp contract(off)
            double s = 0.0;
            if (valid) {
                s = rho64(r[e], a.ph.criterion, a.ph.beta);
                if constexpr (Args::weighted) s = (double)wt * s;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][e] = s;
        }
        if constexpr (Args::step) {
#pragma clang fp contract(off)
            double s = 0.0;
            if (valid && margin) {
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const float d = a.out_n[i * 6 + k] - a.labels[(i - a.n_inter) * 6 + k];
                    const float ad = fabsf(d);
                    s = s + (double)((ad < a.data_beta) ? 0.5f * d * d / a.data_beta : ad - 0.5f * a.data_beta);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][6] = s;
        }
        __syncthreads();
        if (threadIdx.x < ROW) {
#pragma clang fp contract(off)
            a.loss_sums[(int64_t)blockIdx.x * ROW + threadIdx.x] =
                ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
        }
    }
    if (!a.g_out || !valid) return;
    float g[6];
    float inv_n = a.ph.reduce_sum ? 1.0f : 1.0f / (float)n_grp;           // reduction "sum": the criterion does not divide by the number of points
    // The weight rides on 1 / n (the division is by n, not by the sum of the weights): g[e] keeps its shape, last factor included -- the compiler
    // contracts that multiply into the sums that read g[e], so a factor appended behind it would move a rounding.
    if constexpr (Args::weighted) inv_n = inv_n * wt;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        // upstream weight of loss e: cotangent of losses[e] plus cotangent of the in-kernel total (1 when neither is given)
        const float w = (a.gl || a.gtot) ? ((a.gl ? a.gl[e] : 0.f) + (a.gtot ? a.gtot[0] : 0.f)) : 1.f;
        g[e] = a.ph.factor[e] * w * crit_slope(r[e], a.ph.criterion, a.ph.beta) * inv_n;     // d(factor*mean(rho(r)))/dr ; MSE: 2 r
    }
    const float ir = 1.f / rho, ire = 1.f / (rho + EPS);
    float gv[6], gJ[6][3];
    gv[0] = g[0] * J[0][0] + g[1] * (J[1][0] + fc) + g[2] * J[5][0] + g[3] * (C_P * J[3][0] - J[2][0] * ire + L_V * J[4][0]) + g[4] * (-J[2][0] * K + J[4][0]);
    gv[1] = g[0] * (J[0][1] - fc) + g[1] * J[1][1] + g[2] * J[5][1] + g[3] * (C_P * J[3][1] - J[2][1] * ire + L_V * J[4][1]) + g[4] * (-J[2][1] * K + J[4][1]);
    gv[2] = g[4] * omega * delta * Fv / ((p + EPS) * (p + EPS)) + g[5];
    gv[3] = -g[5] * rho * (1.f + 0.608f * q) * R_D;
    gv[4] = -g[5] * rho * 0.608f * R_D * T;
    gv[5] = -g[0] * J[2][0] * ir * ir - g[1] * J[2][1] * ir * ir + g[2] * (J[0][0] + J[1][1]) + g[3] * omega * ire * ire - g[5] * (1.f + 0.608f * q) * R_D * T;
    gJ[0][0] = g[0] * u + g[2] * rho; gJ[0][1] = g[0] * v;             gJ[0][2] = g[0];
    gJ[1][0] = g[1] * u;              gJ[1][1] = g[1] * v + g[2] * rho; gJ[1][2] = g[1];
    gJ[2][0] = g[0] * ir - g[3] * u * ire - g[4] * u * K;
    gJ[2][1] = g[1] * ir - g[3] * v * ire - g[4] * v * K;
    gJ[2][2] = -g[3] * ire - g[4] * K;
    gJ[3][0] = g[3] * C_P * u; gJ[3][1] = g[3] * C_P * v; gJ[3][2] = g[3] * C_P;
    const float gq = g[3] * L_V + g[4];
    gJ[4][0] = gq * u; gJ[4][1] = gq * v; gJ[4][2] = gq;
    gJ[5][0] = g[2] * u; gJ[5][1] = g[2] * v; gJ[5][2] = g[2];
    const float sc[3] = {1.f / a.geo.lon_m1 / a.geo.dx, 1.f / a.geo.lat_m1 / a.geo.dy, 1.f / a.geo.pred_t_span};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float go = gv[k] * msk[k];
        if (a.ph.sq_on[k] && msk[k] != 0.f) {
            // the squared form is not affine: J = jac * d val / d out depends on `out` as well -- d J / d out = jac * 2 std^2 (inside the clip bounds)
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) t = fmaf(gJ[k][c], a.jac_n[(i * 6 + k) * 3 + c], t);
            go = fmaf(t, 2.f * a.ph.std[k] * a.ph.std[k], go);
        }
        if constexpr (Args::step) {
            if (margin) {                                                // + d (data loss) / d out, one rounded addition behind the PDE cotangent
#pragma clang fp contract(off)
                const float d = a.out_n[i * 6 + k] - a.labels[(i - a.n_inter) * 6 + k];
                const float ad = fabsf(d);
                const float gd = a.data_scale * a.gtot[0] * ((ad < a.data_beta) ? d / a.data_beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : d)));   // (NaN stays NaN: dpn_smooth_l1_kernel)
                go = go + gd;
            }
        }
        a.g_out[i * 6 + k] = go;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.g_jxi[(i * 6 + k) * 3 + c] = gJ[k][c] * msk[k] * sc[c];
    }
}

// The six signed residuals of every point, res[n][6] = lhs - rhs (motion-u, motion-v, continuity, energy, vapour, gas), unscaled: the same body as
// dpn_residual_kernel (dpn_residual_body.inc), no reduction and no cotangents -- where a trained field violates its equations.  One thread per point.
struct ResPointArgs {
    const float *out_n, *jac_n, *f;
    int64_t n;
    DpnPhysics ph;
    float* res;
};
__global__ __launch_bounds__(256) void dpn_residual_points_kernel(ResPointArgs a) {
    const int64_t ic = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ic >= a.n) return;
#include "dpn_residual_body.inc"
    float2* dst = reinterpret_cast<float2*>(a.res + ic * 6);               // rows of 24 bytes: 8-byte aligned
    dst[0] = make_float2(r[0], r[1]); dst[1] = make_float2(r[2], r[3]); dst[2] = make_float2(r[4], r[5]);
}

__global__ __launch_bounds__(384) void dpn_residual_finish_kernel(const double* partials, int64_t n, DpnPhysics ph, float* losses) {
    // (a batch of fields: one workgroup per field, its block rows and its seven outputs side by side)
    partials += (int64_t)blockIdx.x * ((n + 255) / 256) * 6;
    losses += (int64_t)blockIdx.x * 7;
    // partials: [ceil(n/256)][6] block rows of dpn_residual.  Wave e adds equation e (lane l takes rows l, l+64, ... in order, then a
    // fixed shuffle tree).  losses[0..5]: the six scaled terms; losses[6]: their sum in the reference's order of additions (:301)
    __shared__ float l[6];
    const int e = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nblk = (n + 255) / 256;
    double s = 0.0;
    for (int64_t b = lane; b < nblk; b += 64) s += partials[b * 6 + e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) { l[e] = (float)((double)(float)(ph.reduce_sum ? s : s / (double)n) * (double)ph.factor[e]); losses[e] = l[e]; }   // .float() * factor (:104)
    __syncthreads();
    if (threadIdx.x == 0) losses[6] = ((((l[0] + l[1]) + l[3]) + l[2]) + l[4]) + l[5];   // montion_u + montion_v + energy + continous + vapor + gas
}

// dpn_step_residual's rows of B fields side by side (per field blocks(n_inter) + blocks(n - n_inter) rows of 7) -> losses[field][16]: [0:6] the interior
// terms, [6] their total, [7:13] the margin terms, [13] their total -- each group as dpn_residual_finish_kernel forms it from that group's rows --,
// [14] the data loss (float)(S / (6 n_m)) * margin_factor, S = column 6 of the margin rows (wave 6: lane l takes rows l, l + 64, ..., the same tree),
// [15] the step's total (data + interior) + margin in fp32.  One workgroup per field, wave e < 6 adds equation e of the interior, then of the margin group.
__global__ __launch_bounds__(448) void dpn_step_finish_kernel(const double* rows, int64_t n_inter, int64_t n, DpnPhysics ph, float margin_factor,
                                                              float* losses) {
#pragma clang fp contract(off)
    const int64_t n_m = n - n_inter, nb_i = (n_inter + 255) / 256, nb_m = (n_m + 255) / 256;
    rows += (int64_t)blockIdx.x * (nb_i + nb_m) * 7;
    losses += (int64_t)blockIdx.x * 16;
    __shared__ float l[2][6];
    __shared__ float data;
    const int e = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = 0; g < (e < 6 ? 2 : 1); ++g) {
        // wave 6 takes column 6 of the margin rows; the others column e of group g
        const bool mrg = g == 1 || e == 6;
        const double* part = mrg ? rows + nb_i * 7 : rows;
        const int64_t nblk = mrg ? nb_m : nb_i, ng = mrg ? n_m : n_inter;
        double s = 0.0;
        for (int64_t b = lane; b < nblk; b += 64) s += part[b * 7 + e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane != 0) continue;
        if (e == 6) {
            data = (float)(s / (6.0 * (double)n_m)) * margin_factor;
            losses[14] = data;
        } else {
            l[g][e] = (float)((double)(float)(ph.reduce_sum ? s : s / (double)ng) * (double)ph.factor[e]);                       // .float() * factor (:104)
            losses[g * 7 + e] = l[g][e];
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float tot[2];
    for (int g = 0; g < 2; ++g) tot[g] = ((((l[g][0] + l[g][1]) + l[g][3]) + l[g][2]) + l[g][4]) + l[g][5];
    losses[6] = tot[0]; losses[13] = tot[1];
    losses[15] = (data + tot[0]) + tot[1];                              // the order in which training_step adds its parts
}

__global__ __launch_bounds__(256) void dpn_smooth_l1_kernel(const float* out_n, const float* labels, int64_t n, float beta, float scale,
                                                            double* loss_sum, float* g_out, int accumulate, const float* scale_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // one element of [N][6]
    const bool valid = i < n * 6;
    float l = 0.f;
    if (valid) {
        const float d = out_n[i] - labels[i];
        const float ad = fabsf(d);
        l = (ad < beta) ? 0.5f * d * d / beta : ad - 0.5f * beta;    // nn.SmoothL1Loss(beta), weights_loss.py:15-19
        if (g_out) {
            const float gv = scale * (scale_dev ? scale_dev[0] : 1.f) * ((ad < beta) ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : d)));   // (a NaN residual
            // gives a NaN slope, as torch's backward does -- not -1: the optimiser's step guard sees a poisoned label through the gradient norm)
            g_out[i] = accumulate ? g_out[i] + gv : gv;             // accumulate: joins the PDE cotangent of the same points
        }
    }
    if (!loss_sum) return;
    double s = (double)l;                          // one fp64 partial per block, fixed order, no atomics: the caller adds the blocks up
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss_sum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int dpn_contract_gpe(const float* g_out, const float* gpe, int64_t n, float* g_pe, void* stream) {
    if (!g_out || !gpe || !g_pe || n <= 0) return -1;
    hipLaunchKernelGGL(dpn_contract_gpe_kernel, dim3((unsigned)n), dim3(192), 0, reinterpret_cast<hipStream_t>(stream), g_out, gpe, n, g_pe);
    return ck(hipGetLastError());
}

int dpn_residual(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys,
                 const float* gl, const float* gtot, double* loss_sums, float* g_out, float* g_jxi, void* stream) {
    if (!out_n || !jac_n || !f || !geo || !phys || n <= 0 || (g_out && !g_jxi)) return -1;
    if (!criterion_ok(phys)) return -1;
    ResArgs a{out_n, jac_n, f, n, *geo, *phys, gl, gtot, loss_sums, g_out, g_jxi};
    hipLaunchKernelGGL(dpn_residual_kernel<ResArgs>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return ck(hipGetLastError());
}

int dpn_residual_weighted(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys,
                          const float* gl, const float* gtot, double* loss_sums, float* g_out, float* g_jxi, const float* w, const int32_t* bin,
                          const float* bin_w, void* stream) {
    if (!out_n || !jac_n || !f || !geo || !phys || n <= 0 || (g_out && !g_jxi) || !criterion_ok(phys)) return -1;
    if ((!w && !bin) || (!bin != !bin_w)) return -1;                       // a weight source is required; bin and bin_w come together
    ResWArgs a{{out_n, jac_n, f, n, *geo, *phys, gl, gtot, loss_sums, g_out, g_jxi}, w, bin, bin_w};
    hipLaunchKernelGGL(dpn_residual_kernel<ResWArgs>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_residual_points(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys, float* res,
                        void* stream) {
    if (!out_n || !jac_n || !f || !geo || !phys || !res || n <= 0) return -1;
    ResPointArgs a{out_n, jac_n, f, n, *phys, res};
    hipLaunchKernelGGL(dpn_residual_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return ck(hipGetLastError());
}

int dpn_residual_finish_batch(const double* loss_sums, int64_t n, int n_fields, const DpnPhysics* phys, float* losses, void* stream) {
    if (!loss_sums || !phys || !losses || n <= 0 || n_fields < 1) return -1;
    hipLaunchKernelGGL(dpn_residual_finish_kernel, dim3(n_fields), dim3(384), 0, reinterpret_cast<hipStream_t>(stream), loss_sums, n, *phys, losses);
    return ck(hipGetLastError());
}
int dpn_residual_finish(const double* loss_sums, int64_t n, const DpnPhysics* phys, float* losses, void* stream) {
    return dpn_residual_finish_batch(loss_sums, n, 1, phys, losses, stream);
}

int64_t dpn_step_rows_doubles(int64_t n_inter, int64_t n) {
    if (n_inter < 1 || n_inter >= n) return 0;
    return 7 * ((n_inter + 255) / 256 + (n - n_inter + 255) / 256);
}

int dpn_step_residual(const float* out_n, const float* jac_n, const float* f, const float* labels, int64_t n_inter, int64_t n, const DpnGeometry* geo,
                      const DpnPhysics* phys, float beta, float data_scale, const float* gtot, double* rows, float* g_out, float* g_jxi, void* stream) {
    if (!out_n || !jac_n || !f || !labels || !geo || !phys || !gtot || !rows || (g_out && !g_jxi)) return -1;
    if (n_inter < 1 || n_inter >= n || !criterion_ok(phys) || !(beta > 0.f)) return -1;
    const int64_t nb_inter = (n_inter + 255) / 256, nb = nb_inter + (n - n_inter + 255) / 256;
    if (nb > 0x7fffffff) return -1;
    ResStepArgs a{{out_n, jac_n, f, n, *geo, *phys, nullptr, gtot, rows, g_out, g_jxi}, labels, n_inter, nb_inter, beta, data_scale};
    hipLaunchKernelGGL(dpn_residual_kernel<ResStepArgs>, dim3((unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_step_finish_batch(const double* rows, int64_t n_inter, int64_t n, int n_fields, const DpnPhysics* phys, float margin_factor, float* losses,
                          void* stream) {
    if (!rows || !phys || !losses || n_inter < 1 || n_inter >= n || n_fields < 1) return -1;
    hipLaunchKernelGGL(dpn_step_finish_kernel, dim3(n_fields), dim3(448), 0, reinterpret_cast<hipStream_t>(stream), rows, n_inter, n, *phys, margin_factor,
                       losses);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_smooth_l1(const float* out_n, const float* labels, int64_t n, float beta, float scale, double* loss_sum, float* g_out, int accumulate,
                  const float* scale_dev, void* stream) {
    if (!out_n || !labels || n <= 0) return -1;
    hipLaunchKernelGGL(dpn_smooth_l1_kernel, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       out_n, labels, n, beta, scale, loss_sum, g_out, accumulate, scale_dev);
    return ck(hipGetLastError());
}

}  // extern "C"
