// Per-point weights and causal time weighting of the PDE losses: a weight per collocation point multiplies the point's
// criterion value and its cotangent.  Causal training (Wang, Sankaran & Perdikaris 2022) is the case where the weight is a function of the point's
// time bin: W_k = exp(-eps * sum_{j<k} l_j), l_j the mean point loss of bin j -- a bin counts only once the earlier bins are fitted.
//   dpn_causal_bins       : the residual body per point, s_i = sum_e factor_e * rho(r_ie) in fp64, the point's time bin, and per block one row of
//                           per-bin (sum s, count);
//   dpn_causal_weights    : one workgroup: the block rows added in a fixed order, l_k, the exclusive prefix sum, W_k;
// One thread per point, wave64, 256 threads per block.  No atomics: every sum has one fixed order, so two runs -- eager or replayed from a captured
// graph -- agree bitwise.  All fp64 arithmetic that defines a result is compiled without contraction (one rounding per operation).  The residual
// body is dpn_residual.hip's (dpn_residual_body.inc), the criterion dpn_criterion.h's.  The kernel that applies the weights is in dpn_residual.hip:
// dpn_residual_kernel<ResWArgs>, behind dpn_residual_weighted.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dpn_criterion.h"

namespace {

constexpr int THREADS = 256, MAX_BINS = DPN_CAUSAL_MAX_BINS;

inline bool finite_host(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }       // false for NaN and +-inf
DEV bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// ------------------------------------------------------------------------------------------------ bins
struct BinArgs {
    const float *out_n, *jac_n, *f, *t;
    int64_t n;
    DpnPhysics ph;
    double fac[6];
    double t_lo, t_span;          // t_span = t_hi - t_lo, formed once on the host in fp64
    int n_bins;
    int32_t* bin;
    double* rows;                 // [blocks][n_bins][2]: sum s, count
};

__global__ __launch_bounds__(THREADS) void dpn_causal_bins_kernel(BinArgs a) {
    __shared__ double s_lds[THREADS];
    __shared__ int b_lds[THREADS];
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool valid = i < a.n;
    const int64_t ic = valid ? i : a.n - 1;
#include "dpn_residual_body.inc"
    // The residuals go through LDS as three float2 rows, the way dpn_residual_points_kernel stores them: the compiler pairs the arithmetic of
    // (r0, r1), (r2, r3), (r4, r5) behind such stores and contracts it accordingly, so the values read back are bitwise that kernel's rows -- what
    // a host restatement of s_i starts from.
    __shared__ float2 r_lds[THREADS][3];
    r_lds[threadIdx.x][0] = make_float2(r[0], r[1]); r_lds[threadIdx.x][1] = make_float2(r[2], r[3]); r_lds[threadIdx.x][2] = make_float2(r[4], r[5]);
    __syncthreads();
    const float2 r01 = r_lds[threadIdx.x][0], r23 = r_lds[threadIdx.x][1], r45 = r_lds[threadIdx.x][2];
    const float rr[6] = {r01.x, r01.y, r23.x, r23.y, r45.x, r45.y};
    double s = 0.0;
    int b = -1;                                             // a lane past the end: in no bin
    if (valid) {
#pragma clang fp contract(off)
#pragma unroll
        for (int e = 0; e < 6; ++e) s = s + a.fac[e] * rho64(rr[e], a.ph.criterion, a.ph.beta);
        const double pos = floor((((double)a.t[i] - a.t_lo) * (double)a.n_bins) / a.t_span);
        b = !(pos >= 0.0) ? 0 : (pos > (double)(a.n_bins - 1) ? a.n_bins - 1 : (int)pos);       // clamped; a NaN time goes to bin 0
        a.bin[i] = b;
    }
    s_lds[threadIdx.x] = s;
    b_lds[threadIdx.x] = b;
    __syncthreads();
    if ((int)threadIdx.x < a.n_bins) {
        // thread k adds bin k's points of the block in point order
#pragma clang fp contract(off)
        const int k = threadIdx.x;
        double sum = 0.0, cnt = 0.0;
        for (int j = 0; j < THREADS; ++j)
            if (b_lds[j] == k) { sum = sum + s_lds[j]; cnt = cnt + 1.0; }
        double* row = a.rows + ((int64_t)blockIdx.x * a.n_bins + k) * 2;
        row[0] = sum; row[1] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------ weights
// One workgroup.  Thread (q, k) = (tid >> 6, tid & 63) adds the rows of blocks q, q + 4, q + 8, ... of bin k in that order; the four parts are added
// ((p0 + p1) + p2) + p3.  Thread 0 then runs the sequential part over the bins.
__global__ __launch_bounds__(THREADS) void dpn_causal_weights_kernel(const double* rows, int64_t nblk, int n_bins, double eps, int relative, float* W32,
                                                                     double* diag) {
#pragma clang fp contract(off)
    __shared__ double part[4][MAX_BINS][2];
    __shared__ double l[MAX_BINS], cnt[MAX_BINS];
    const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
    double sum = 0.0, c = 0.0;
    if (k < n_bins)
        for (int64_t b = q; b < nblk; b += 4) {
            const double* row = rows + (b * n_bins + k) * 2;
            sum = sum + row[0]; c = c + row[1];
        }
    part[q][k][0] = sum; part[q][k][1] = c;
    __syncthreads();
    if (q == 0 && k < n_bins) {
        const double st = ((part[0][k][0] + part[1][k][0]) + part[2][k][0]) + part[3][k][0];
        const double ct = ((part[0][k][1] + part[1][k][1]) + part[2][k][1]) + part[3][k][1];
        l[k] = ct > 0.0 ? st / ct : 0.0;
        cnt[k] = ct;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double norm = 1.0;
    bool ones = false;
    if (relative) {
        double tot = 0.0, occupied = 0.0;
        for (int j = 0; j < n_bins; ++j)
            if (cnt[j] > 0.0) { tot = tot + l[j]; occupied = occupied + 1.0; }
        norm = tot / occupied;                              // occupied >= 1: n >= 1 points
        ones = !(norm > 0.0) || !finite64(norm);            // nothing to weight by
    }
    double cum = 0.0, w_min = 1.0;
    for (int j = 0; j < n_bins; ++j) {
        const double w = ones ? 1.0 : exp(-eps * cum);
        W32[j] = (float)w;
        diag[j] = w; diag[n_bins + j] = l[j]; diag[2 * n_bins + j] = cnt[j];
        if (!(w >= w_min)) w_min = w;                       // a NaN weight shows in the minimum
        cum = cum + (relative ? l[j] / norm : l[j]);
    }
    diag[3 * n_bins] = w_min; diag[3 * n_bins + 1] = norm;
}

inline int64_t blocks_of(int64_t n) { return (n + THREADS - 1) / THREADS; }

}  // namespace

extern "C" {

int64_t dpn_causal_rows_doubles(int64_t n, int n_bins) {
    if (n <= 0 || n_bins < 1 || n_bins > MAX_BINS) return 0;
    return blocks_of(n) * n_bins * 2;
}

int dpn_causal_bins(const float* out_n, const float* jac_n, const float* f, const float* t, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys,
                    const double* factors, double t_lo, double t_hi, int n_bins, int32_t* bin, double* rows, void* stream) {
    if (!out_n || !jac_n || !f || !t || !geo || !phys || !factors || !bin || !rows || n <= 0) return -1;
    if (n_bins < 1 || n_bins > MAX_BINS || !finite_host(t_lo) || !finite_host(t_hi) || !(t_hi > t_lo) || !criterion_ok(phys)) return -1;
    BinArgs a{out_n, jac_n, f, t, n, *phys, {factors[0], factors[1], factors[2], factors[3], factors[4], factors[5]}, t_lo, t_hi - t_lo, n_bins, bin, rows};
    hipLaunchKernelGGL(dpn_causal_bins_kernel, dim3((unsigned)blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_causal_weights(const double* rows, int64_t n, int n_bins, double eps, int relative, float* W32, double* diag, void* stream) {
    if (!rows || !W32 || !diag || n <= 0 || n_bins < 1 || n_bins > MAX_BINS || !(eps >= 0.0) || !finite_host(eps)) return -1;
    hipLaunchKernelGGL(dpn_causal_weights_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, rows, blocks_of(n), n_bins, eps, relative ? 1 : 0, W32,
                       diag);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
