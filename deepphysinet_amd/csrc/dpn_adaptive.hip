// Residual-weighted interior collocation points: a pool of uniform interior draws is scored by its PDE residuals and n points
// are drawn from it with probability p_i ~ s_i^k / mean(s^k) + c (residual-based adaptive sampling, Wu et al. 2023), all on the device.
//   dpn_adaptive_scores : s_i = sum_e factor_e * res_ie^2 in fp64, and sum s^k / the non-finite count / max s reduced in a fixed order;
//   dpn_adaptive_select : weights, their inclusive fp64 prefix sum, an inverse-CDF draw per output point (Philox stream 2 of the pool's own
//                         counters), and the gather of the drawn rows.
// One thread per element, wave64, 256 threads and 1024 elements per block.  No atomics: every sum has one fixed order, so two runs -- eager or replayed
// from a captured graph -- agree bitwise.  All fp64 arithmetic that defines a result is compiled without contraction (one rounding per operation).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dpn_hip.h"

namespace {

constexpr int THREADS = 256, PER_THREAD = 4, BLOCK_ELEMS = THREADS * PER_THREAD, MAX_BLOCKS = 1024;
constexpr int64_t MAX_CANDIDATES = (int64_t)BLOCK_ELEMS * MAX_BLOCKS;          // 2^20: what one block scans of block totals

// Philox-4x32-10 and the 53-bit uniform exactly as dpn_sampler.hip draws them (restated here: that unit's object does not change with this one).
__device__ inline void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ inline double u53(uint32_t hi, uint32_t lo) {
    return (double)((((uint64_t)hi << 21) ^ (uint64_t)(lo >> 11)) & ((1ull << 53) - 1)) * (1.0 / 9007199254740992.0);
}

__device__ inline bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }       // false for NaN and +-inf

// s^k of a score; a score that is negative or not finite counts as 0 (dpn_adaptive_scores never writes one; a caller's own scores may hold one).
// The forms numpy's power takes for these exponents, so that a host reference forms the same weights: 0 -> 1 (also 0^0), 1 -> s, 2 -> s * s, 0.5 -> sqrt.
__device__ inline double pow_k(double s, const double k) {
#pragma clang fp contract(off)
    if (!(s > 0.0) || !finite64(s)) s = 0.0;
    if (k == 0.0) return 1.0;
    if (k == 1.0) return s;
    if (k == 2.0) return s * s;
    if (k == 0.5) return sqrt(s);
    return pow(s, k);
}

// Sum over the block of one value per thread in a fixed tree order; every thread gets the result.  lds: THREADS doubles.
__device__ inline double block_sum(double v, double* lds) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();
    lds[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = lds[tid] + lds[tid + s];
        __syncthreads();
    }
    return lds[0];
}
__device__ inline double block_max(double v, double* lds) {
    const int tid = threadIdx.x;
    __syncthreads();
    lds[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = fmax(lds[tid], lds[tid + s]);
        __syncthreads();
    }
    return lds[0];
}
// The sum of nb <= MAX_BLOCKS block rows v[b * stride]: thread t adds rows t, t + 256, ... in that order, then the tree.  Both entry points reduce
// their block sums of s^k through this, so dpn_adaptive_scores' stats[0] is bitwise the sum dpn_adaptive_select divides by.
__device__ inline double sum_rows(const double* v, const int stride, const int nb, double* lds) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += THREADS) acc = acc + v[(int64_t)b * stride];
    return block_sum(acc, lds);
}

struct ScoreArgs {
    const float* res;
    int64_t m;
    double fac[6];
    double k;
    double* score;
    double* part;          // [nb][3]: sum s^k, non-finite count, max s of the block
};
__global__ __launch_bounds__(THREADS) void dpn_adaptive_score_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
    __shared__ double lds[THREADS];
    const int64_t base = (int64_t)blockIdx.x * BLOCK_ELEMS + threadIdx.x * PER_THREAD;
    double sum = 0.0, bad = 0.0, top = 0.0;
    for (int e = 0; e < PER_THREAD; ++e) {
        const int64_t i = base + e;
        if (i >= a.m) break;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double r = (double)a.res[i * 6 + q];
            const double r2 = r * r;                      // exact: two 24-bit significands
            s = s + a.fac[q] * r2;
        }
        if (!finite64(s)) { s = 0.0; bad = bad + 1.0; }
        a.score[i] = s;
        sum = sum + pow_k(s, a.k);
        top = fmax(top, s);
    }
    sum = block_sum(sum, lds);
    bad = block_sum(bad, lds);
    top = block_max(top, lds);
    if (threadIdx.x == 0) {
        double* p = a.part + (int64_t)blockIdx.x * 3;
        p[0] = sum; p[1] = bad; p[2] = top;
    }
}
__global__ __launch_bounds__(THREADS) void dpn_adaptive_stats_kernel(const double* part, int nb, double* stats) {
    __shared__ double lds[THREADS];
    const double sum = sum_rows(part, 3, nb, lds);
    const double bad = sum_rows(part + 1, 3, nb, lds);
    double top = 0.0;
    for (int b = threadIdx.x; b < nb; b += THREADS) top = fmax(top, part[(int64_t)b * 3 + 2]);
    top = block_max(top, lds);
    if (threadIdx.x == 0) { stats[0] = sum; stats[1] = bad; stats[2] = top; }
}

// select, pass 1: the block sums of s^k
__global__ __launch_bounds__(THREADS) void dpn_adaptive_pow_kernel(const double* score, int64_t m, double k, double* bsum) {
#pragma clang fp contract(off)
    __shared__ double lds[THREADS];
    const int64_t base = (int64_t)blockIdx.x * BLOCK_ELEMS + threadIdx.x * PER_THREAD;
    double sum = 0.0;
    for (int e = 0; e < PER_THREAD; ++e)
        if (base + e < m) sum = sum + pow_k(score[base + e], k);
    sum = block_sum(sum, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// select, pass 2: the weights and their block-local inclusive prefix sum.  The scan is sequential at each of three levels -- four elements of a thread,
// sixteen threads of a group, sixteen groups of the block -- and a level's offset is added last: local[i] = G[group] + (T[thread] + run[e]).  With
// every offset itself the sequential sum of the totals before it, an element of weight 0 repeats its predecessor's value bitwise (also across a
// thread, group or block boundary), and the sequence never decreases: fl(a + x) <= fl(a + y) for x <= y.
__global__ __launch_bounds__(THREADS) void dpn_adaptive_scan_kernel(const double* score, int64_t m, double k, double c, const double* bsum, int nb,
                                                                    double* cdf, double* btot) {
#pragma clang fp contract(off)
    __shared__ double lds[THREADS];
    __shared__ double T[THREADS];
    __shared__ double G[THREADS / 16];
    const int tid = threadIdx.x;
    const double mean = sum_rows(bsum, 1, nb, lds) / (double)m;
    const bool uniform = !(mean > 0.0) || !finite64(mean);          // nothing to weight by: every candidate alike
    const int64_t base = (int64_t)blockIdx.x * BLOCK_ELEMS + tid * PER_THREAD;
    double run[PER_THREAD];
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e) {
        double w = 0.0;
        if (base + e < m) w = uniform ? 1.0 : pow_k(score[base + e], k) / mean + c;
        acc = acc + w;
        run[e] = acc;
    }
    T[tid] = acc;
    __syncthreads();
    if (tid < THREADS / 16) {
        double g = 0.0;
        for (int j = 0; j < 16; ++j) { const double v = T[tid * 16 + j]; T[tid * 16 + j] = g; g = g + v; }
        G[tid] = g;
    }
    __syncthreads();
    if (tid == 0) {
        double g = 0.0;
        for (int j = 0; j < THREADS / 16; ++j) { const double v = G[j]; G[j] = g; g = g + v; }
        btot[blockIdx.x] = g;
    }
    __syncthreads();
    const double toff = T[tid], goff = G[tid >> 4];
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e)
        if (base + e < m) { const double inner = toff + run[e]; cdf[base + e] = goff + inner; }
}

// select, pass 3: block b's offset = the sequential sum of the block totals before it (every block forms its own, from the same numbers in the same
// order), added to the block's local values.
__global__ __launch_bounds__(THREADS) void dpn_adaptive_offset_kernel(int64_t m, const double* btot, double* cdf) {
#pragma clang fp contract(off)
    __shared__ double tot[MAX_BLOCKS];
    __shared__ double off;
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < b; j += THREADS) tot[j] = btot[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        double g = 0.0;
        for (int j = 0; j < b; ++j) g = g + tot[j];
        off = g;
    }
    __syncthreads();
    const double o = off;
    const int64_t base = (int64_t)b * BLOCK_ELEMS + threadIdx.x * PER_THREAD;
#pragma unroll
    for (int e = 0; e < PER_THREAD; ++e)
        if (base + e < m) cdf[base + e] = o + cdf[base + e];
}

struct DrawArgs {
    const double* cdf;
    const double* score;
    int64_t m, n;
    uint64_t seed, offset;
    const int32_t* step_dev;
    uint64_t stride;
    const float *x, *y, *t, *f, *cd;
    float *ox, *oy, *ot, *of, *ocd;
    int32_t* idx;
    double* u;
    double* picked;
};
// select, pass 4: output point j draws u_j, finds the smallest i with cdf[i] > u_j * total and copies candidate i's row.
__global__ __launch_bounds__(THREADS) void dpn_adaptive_draw_kernel(DrawArgs a) {
    const int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (j >= a.n) return;
    uint32_t w[4];
    const uint64_t ctr = a.offset + (a.step_dev ? (uint64_t)(uint32_t)(*a.step_dev) * a.stride : 0ull) + (uint64_t)j;
    philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 2u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);      // stream id 2: the pool took 0 and 1
    const double u = u53(w[0], w[1]);
    const double total = a.cdf[a.m - 1];                                  // > 0: some weight is positive whenever the mean is, else all are 1
    double target;
    {
#pragma clang fp contract(off)
        target = u * total;
    }
    if (!(target < total)) target = __longlong_as_double(__double_as_longlong(total) - 1);     // u * total rounded up to total: the last double below it
    int64_t lo = 0, hi = a.m - 1;                                         // cdf[m - 1] = total > target: the answer exists
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    // cdf[lo - 1] <= target < cdf[lo]: the prefix sum rose at lo, so w[lo] > 0 (a zero weight repeats its predecessor's value)
    a.ox[j] = a.x[lo]; a.oy[j] = a.y[lo]; a.ot[j] = a.t[lo]; a.of[j] = a.f[lo];
#pragma unroll
    for (int q = 0; q < 6; ++q) a.ocd[j * 6 + q] = a.cd[lo * 6 + q];
    if (a.idx) a.idx[j] = (int32_t)lo;
    if (a.u) a.u[j] = u;
    if (a.picked) a.picked[j] = a.score[lo];
}

inline bool exponent_ok(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }       // false for NaN, negative and +inf
inline int blocks_of(int64_t m) { return (int)((m + BLOCK_ELEMS - 1) / BLOCK_ELEMS); }

}  // namespace

extern "C" {

int64_t dpn_adaptive_scratch_doubles(int64_t m) {
    if (m <= 0 || m > MAX_CANDIDATES) return 0;
    return m + 5 * (int64_t)blocks_of(m);          // cdf [m] | block sums of s^k [nb] | block totals [nb] | dpn_adaptive_scores' block rows [nb][3]
}

int dpn_adaptive_scores(const float* res, int64_t m, const double* factors, double k, double* score, double* stats, double* scratch, void* stream) {
    if (!res || !factors || !score || !stats || !scratch || m <= 0 || m > MAX_CANDIDATES || !exponent_ok(k)) return -1;
    const int nb = blocks_of(m);
    ScoreArgs a{res, m, {factors[0], factors[1], factors[2], factors[3], factors[4], factors[5]}, k, score, scratch + m + 2 * (int64_t)nb};
    hipLaunchKernelGGL(dpn_adaptive_score_kernel, dim3((unsigned)nb), dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(dpn_adaptive_stats_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, (const double*)a.part, nb, stats);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_adaptive_select(const double* score, int64_t m, double k, double c, const float* x, const float* y, const float* t, const float* f,
                        const float* coord_data, int64_t n, uint64_t seed, uint64_t offset, const int32_t* step_dev, uint64_t stride,
                        float* out_x, float* out_y, float* out_t, float* out_f, float* out_coord_data, int32_t* idx, double* u, double* picked_score,
                        double* scratch, void* stream) {
    if (!score || !x || !y || !t || !f || !coord_data || !out_x || !out_y || !out_t || !out_f || !out_coord_data || !scratch) return -1;
    if (m <= 0 || m > MAX_CANDIDATES || n <= 0 || n > ((int64_t)1 << 30) || !exponent_ok(k) || !exponent_ok(c)) return -1;
    const int nb = blocks_of(m);
    double *cdf = scratch, *bsum = scratch + m, *btot = bsum + nb;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dpn_adaptive_pow_kernel, dim3((unsigned)nb), dim3(THREADS), 0, s, score, m, k, bsum);
    hipLaunchKernelGGL(dpn_adaptive_scan_kernel, dim3((unsigned)nb), dim3(THREADS), 0, s, score, m, k, c, (const double*)bsum, nb, cdf, btot);
    hipLaunchKernelGGL(dpn_adaptive_offset_kernel, dim3((unsigned)nb), dim3(THREADS), 0, s, m, (const double*)btot, cdf);
    DrawArgs a{cdf, score, m, n, seed, offset, step_dev, stride, x, y, t, f, coord_data, out_x, out_y, out_t, out_f, out_coord_data, idx, u, picked_score};
    hipLaunchKernelGGL(dpn_adaptive_draw_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
