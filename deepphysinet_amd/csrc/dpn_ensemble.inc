// Ensemble statistics over field samples (DESIGN.md section 6b, item f3 continued), included by dpn_diag.hip behind dpn_diagnostics_kernel: the member
// axis of the product table.  include/dpn_hip.h states the state's layout and every operation's order.
//   dpn_ensemble_accumulate : ONE member's products at points first .. first + n folded into a resident state (count, Welford mean and M2 in fp64, min,
//                             max, exceedance counts), the residual body per point and dpn_diagnostics_kernel's product expressions, one thread per point.
//   dpn_ensemble_finish     : the state of points first .. first + n -> mean, spread, min, max, count and exceedance probabilities, as rows or as maps.
// Both kernels are compiled without contraction: every fp32 and fp64 operation is rounded on its own, so the numpy restatement
// (deepphysinet_amd/ensemble.py) reproduces them bit for bit.  The state is product-major ([column][point]): lane l of a wave reads and writes place
// first + r + l of a column.  No atomics (a point belongs to one thread, members arrive launch after launch on one stream), no LDS, plain per-lane stores.

namespace {

struct EnsArgs {
    const float *out_n, *jac_n, *f;
    int64_t n, first, n_total;
    DpnPhysics ph;
    int32_t n_products, n_thr;
    int32_t id[DPN_ENS_PRODUCTS];                       // the column selector, in output order
    int32_t thr_col[DPN_ENS_MAX_THRESHOLDS];            // the column a threshold applies to
    float thr_val[DPN_ENS_MAX_THRESHOLDS];
    int32_t* count;
    double *mean, *m2;
    float *vmin, *vmax;
    int32_t* exceed;
};

// What the residual body reads as a.jac_n[.] and a.f[.]: the array, or, in the instantiations for requests that do not read it, a zero that touches no
// memory (the pointer may be NULL there).
template <bool WITH> struct EnsSrc {
    const float* p;
    __device__ __forceinline__ explicit EnsSrc(const float* q) : p(q) {}
    __device__ __forceinline__ float operator[](const int64_t i) const { return p[i]; }
};
template <> struct EnsSrc<false> {
    __device__ __forceinline__ explicit EnsSrc(const float*) {}
    __device__ __forceinline__ float operator[](const int64_t) const { return 0.f; }
};
template <bool WITH_J, bool WITH_F> struct EnsBody {
    const float* out_n;
    EnsSrc<WITH_J> jac_n;
    EnsSrc<WITH_F> f;
    const DpnPhysics& ph;
};

template <bool WITH_J, bool WITH_F>
__global__ __launch_bounds__(THREADS) void dpn_ensemble_accumulate_kernel(EnsArgs e) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= e.n) return;
    const EnsBody<WITH_J, WITH_F> a{e.out_n, EnsSrc<WITH_J>(e.jac_n), EnsSrc<WITH_F>(e.f), e.ph};
#include "dpn_residual_body.inc"
    const float zeta = J[1][0] - J[0][1];                     // the expressions of dpn_diagnostics_kernel, in its order
    const float div = J[0][0] + J[1][1];
    const float adv_T = u * J[3][0] + v * J[3][1];
    const float adv_q = u * J[4][0] + v * J[4][1];
    const float stretch = J[0][0] - J[1][1], shear = J[1][0] + J[0][1];
    bool poisoned = false;                                    // its NaN rule: a NaN among the six normalised fields is a NaN in every product
#pragma unroll
    for (int k = 0; k < 6; ++k) { const float o_n = a.out_n[ic * 6 + k]; poisoned |= o_n != o_n; }
    if (poisoned) return;                                     // ... and a NaN changes nothing of a column
    const int64_t g = e.first + ic;
    for (int j = 0; j < e.n_products; ++j) {                  // the selector is uniform: a scalar branch per product
        float x;
        switch (e.id[j]) {
#define DPN_ENS_J(k) case 3 * k: x = J[k][0]; break; case 3 * k + 1: x = J[k][1]; break; case 3 * k + 2: x = J[k][2]; break;
            DPN_ENS_J(0) DPN_ENS_J(1) DPN_ENS_J(2) DPN_ENS_J(3) DPN_ENS_J(4) DPN_ENS_J(5)
#undef DPN_ENS_J
            case 18: x = zeta; break;
            case 19: x = zeta + fc; break;
            case 20: x = div; break;
            case 21: x = omega; break;
            case 22: x = -adv_T; break;
            case 23: x = -adv_q; break;
            case 24: x = q * div + adv_q; break;
            case 25: x = sqrtf(u * u + v * v); break;
            case 26: x = q / q_s; break;
            case 27: x = sqrtf(stretch * stretch + shear * shear); break;
            case 28: x = u; break;
            case 29: x = v; break;
            case 30: x = p; break;
            case 31: x = T; break;
            case 32: x = q; break;
            default: x = rho; break;                          // 33 (the entry point admits 0..33 only)
        }
        if (!__builtin_isfinite(x)) continue;
        const int64_t s = (int64_t)j * e.n_total + g;
        const int32_t c = e.count[s] + 1;
        const double xd = (double)x;
        double mean = e.mean[s];
        const double d = xd - mean;
        mean = mean + d / (double)c;
        e.m2[s] = e.m2[s] + d * (xd - mean);
        e.mean[s] = mean;
        e.count[s] = c;
        if (c == 1) {                                         // min and max are not read before they are set
            e.vmin[s] = x;
            e.vmax[s] = x;
        } else {                                              // fminf / fmaxf of two finite numbers, written as a comparison: between +0 and -0
            const float lo = e.vmin[s], hi = e.vmax[s];       // (where the C functions may return either) the earlier member's zero stays
            if (x < lo) e.vmin[s] = x;
            if (x > hi) e.vmax[s] = x;
        }
        for (int i = 0; i < e.n_thr; ++i)
            if (e.thr_col[i] == j) e.exceed[(int64_t)i * e.n_total + g] += x > e.thr_val[i] ? 1 : 0;
    }
}

struct EnsFinishArgs {
    const int32_t* count;
    const double *mean, *m2;
    const float *vmin, *vmax;
    const int32_t* exceed;
    int64_t n, first, n_total, plane;                         // plane = nx * ny (map form), 0 in row form
    int32_t n_products, n_thr;
    int32_t thr_col[DPN_ENS_MAX_THRESHOLDS];
    DpnEnsembleOut out;
};

__global__ __launch_bounds__(THREADS) void dpn_ensemble_finish_kernel(EnsFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= a.n) return;
    const int64_t g = a.first + ic;
    const float nan = __builtin_nanf("");
    int64_t at, at_prob, stride;
    if (a.plane == 0) {                                       // rows [n][P] and [n][E]
        at = ic * a.n_products;
        at_prob = ic * a.n_thr;
        stride = 1;
    } else {                                                  // point g of the lattice: plane it, place r; column j of it lies at plane it * P + j
        const int64_t it = g / a.plane, r = g - it * a.plane;
        at = it * a.n_products * a.plane + r;
        at_prob = it * a.n_thr * a.plane + r;
        stride = a.plane;
    }
    for (int j = 0; j < a.n_products; ++j) {
        const int64_t s = (int64_t)j * a.n_total + g, o = at + j * stride;
        const int32_t c = a.count[s];
        a.out.count[o] = c;
        a.out.mean[o] = c > 0 ? (float)a.mean[s] : nan;
        a.out.spread[o] = c > 1 ? (float)sqrt(a.m2[s] / (double)(c - 1)) : nan;
        a.out.min[o] = c > 0 ? a.vmin[s] : nan;
        a.out.max[o] = c > 0 ? a.vmax[s] : nan;
    }
    for (int e = 0; e < a.n_thr; ++e) {
        const int32_t c = a.count[(int64_t)a.thr_col[e] * a.n_total + g];
        a.out.prob[at_prob + e * stride] = c > 0 ? (float)((double)a.exceed[(int64_t)e * a.n_total + g] / (double)c) : nan;
    }
}

// ids 0..24 and 27 read the Jacobian, id 19 the Coriolis parameter
bool ens_reads_jac(const int id) { return id <= 24 || id == 27; }

}  // namespace

extern "C" {

int dpn_ensemble_accumulate(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnPhysics* phys, int with_clip,
                            const int32_t* products, int n_products, const int32_t* thr_col, const float* thr_val, int n_thr, int64_t first,
                            int64_t n_total, int32_t* count, double* mean, double* m2, float* vmin, float* vmax, int32_t* exceed, void* stream) {
    if (!out_n || !phys || !products || !count || !mean || !m2 || !vmin || !vmax) return -1;
    if (n <= 0 || first < 0 || n_total <= 0 || first > n_total - n) return -1;
    if (n_products < 1 || n_products > DPN_ENS_PRODUCTS || n_thr < 0 || n_thr > DPN_ENS_MAX_THRESHOLDS) return -1;
    if (n_thr > 0 && (!thr_col || !thr_val || !exceed)) return -1;
    EnsArgs a{out_n, jac_n, f, n, first, n_total, *phys, n_products, n_thr, {}, {}, {}, count, mean, m2, vmin, vmax, exceed};
    bool need_j = false, need_f = false;
    for (int j = 0; j < n_products; ++j) {
        if (products[j] < 0 || products[j] >= DPN_ENS_PRODUCTS) return -1;
        a.id[j] = products[j];
        need_j |= ens_reads_jac(products[j]);
        need_f |= products[j] == 19;
    }
    if ((need_j && !jac_n) || (need_f && !f)) return -1;
    for (int e = 0; e < n_thr; ++e) {
        if (thr_col[e] < 0 || thr_col[e] >= n_products || !(thr_val[e] - thr_val[e] == 0.f)) return -1;      // (a NaN or an infinity fails the last)
        a.thr_col[e] = thr_col[e];
        a.thr_val[e] = thr_val[e];
    }
    if (!with_clip)
        for (int k = 0; k < 6; ++k) a.ph.clip_on[k] = 0;                  // the body then neither clips nor masks
    const dim3 grid((unsigned)((n + THREADS - 1) / THREADS)), block(THREADS);
    if (need_f)
        hipLaunchKernelGGL((dpn_ensemble_accumulate_kernel<true, true>), grid, block, 0, (hipStream_t)stream, a);
    else if (need_j)
        hipLaunchKernelGGL((dpn_ensemble_accumulate_kernel<true, false>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((dpn_ensemble_accumulate_kernel<false, false>), grid, block, 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_ensemble_finish(const int32_t* count, const double* mean, const double* m2, const float* vmin, const float* vmax, const int32_t* exceed,
                        int64_t n_total, int n_products, const int32_t* thr_col, int n_thr, int64_t first, int64_t n, const DpnEnsembleOut* rows,
                        const DpnEnsembleOut* maps, const DpnLattice* lattice, void* stream) {
    if (!count || !mean || !m2 || !vmin || !vmax) return -1;
    if (n <= 0 || first < 0 || n_total <= 0 || first > n_total - n) return -1;
    if (n_products < 1 || n_products > DPN_ENS_PRODUCTS || n_thr < 0 || n_thr > DPN_ENS_MAX_THRESHOLDS) return -1;
    if ((rows != nullptr) == (maps != nullptr)) return -1;
    const DpnEnsembleOut* out = rows ? rows : maps;
    if (!out->mean || !out->spread || !out->min || !out->max || !out->count) return -1;
    if (n_thr > 0 && (!thr_col || !exceed || !out->prob)) return -1;
    EnsFinishArgs a{count, mean, m2, vmin, vmax, exceed, n, first, n_total, 0, n_products, n_thr, {}, *out};
    for (int e = 0; e < n_thr; ++e) {
        if (thr_col[e] < 0 || thr_col[e] >= n_products) return -1;
        a.thr_col[e] = thr_col[e];
    }
    if (maps) {
        if (!lattice || lattice->nx < 1 || lattice->ny < 1 || lattice->nt < 1) return -1;
        a.plane = (int64_t)lattice->nx * lattice->ny;
        if (first + n > a.plane * lattice->nt) return -1;
    } else if (lattice) {
        return -1;
    }
    hipLaunchKernelGGL(dpn_ensemble_finish_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
