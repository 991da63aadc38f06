// Loss balancing by gradient norms: every few hundred steps each loss term's weight lambda_k is moved towards
// mean_j |grad L_j| / |grad L_k| (Wang, Teng & Perdikaris 2021, "learning-rate annealing"; Wang, Sankaran, Wang & Perdikaris 2023), in the mean
// form: lambda = 1 when all norms are equal.
//   dpn_balance_sumsq    : the sum of squares of a table of fp32 tensors in fp64 -- one partial per 2048-element chunk, the partials in a fixed
//                          order (the scheme of dpn_optim.hip's gradient norm, with fp64 accumulation throughout);
//   dpn_balance_update   : one workgroup, one thread: the norms, their mean over the active terms, the clamped targets, the moving average;
//   dpn_balance_combine  : total = sum_i lambda_map(i) * term_i over the 13 terms of a step, and / or the 13 cotangents cot_in * lambda_map(i).
// lambda lives on the device and is read at run time: no host synchronisation.  No atomics: every sum has one fixed order, so two runs agree
// bitwise.  All arithmetic that defines a result is compiled without contraction (one rounding per operation).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dpn_hip.h"

namespace {

constexpr int THREADS = 256, CHUNK = 2048, TABLE_TENSORS = 160, MAX_TENSORS = DPN_BALANCE_MAX_TENSORS, MAX_TERMS = DPN_BALANCE_MAX_TERMS, STEP_TERMS = DPN_BALANCE_STEP_TERMS;

inline bool finite_host(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }       // false for NaN and +-inf
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// ------------------------------------------------------------------------------------------------ sum of squares
// One launch takes TABLE_TENSORS tensors (the table travels in the kernel arguments); a longer list is cut into several launches that write
// consecutive ranges of the same partials, so the order of the partials -- tensor after tensor -- does not depend on the cut.
struct SumsqTable {
    const float* g[TABLE_TENSORS];
    int chunk_start[TABLE_TENSORS + 1];          // prefix sum of ceil(numel / CHUNK) within this launch
    int numel[TABLE_TENSORS];
    int n;
};
static_assert(sizeof(SumsqTable) + 64 <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ int table_find(const SumsqTable& t, int blk) {
    int lo = 0, hi = t.n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.chunk_start[mid] <= blk) lo = mid; else hi = mid - 1; }
    return lo;
}

// One block per chunk.  Thread j adds the squares of elements j, j + 256, ... of the chunk in that order; a product of two fp32 values is exact in
// fp64, so every rounding is one of the additions.  Wave tree, then (w0 + w1) + (w2 + w3).  A NULL tensor counts as zeros.
__global__ __launch_bounds__(THREADS) void dpn_balance_sumsq_kernel(SumsqTable t, double* partial) {
#pragma clang fp contract(off)
    const int ti = table_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * CHUNK;
    const float* g = t.g[ti];
    const int end = min(base + CHUNK, t.numel[ti]);
    double d = 0.0;
    if (g)
        for (int i = base + threadIdx.x; i < end; i += THREADS) { const double v = (double)g[i]; d = d + v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d = d + __shfl_xor(d, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup: thread j adds partials j, j + 256, ... in that order; the same tree.
__global__ __launch_bounds__(THREADS) void dpn_balance_sumsq_reduce_kernel(const double* partial, int n, double* sumsq) {
#pragma clang fp contract(off)
    double d = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) d = d + partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d = d + __shfl_xor(d, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) *sumsq = (red[0] + red[1]) + (red[2] + red[3]);
}

// Chunks of the table, or 0 for a table this unit does not take.
int64_t table_chunks(int n_tensors, const int64_t* numel) {
    if (n_tensors < 1 || n_tensors > MAX_TENSORS || !numel) return 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 1 || numel[i] > 0x7fffffff - CHUNK) return 0;
        chunks += (numel[i] + CHUNK - 1) / CHUNK;
    }
    return chunks <= 0x7fffffff ? chunks : 0;
}

// ------------------------------------------------------------------------------------------------ update
// The rule of deepphysinet_amd/balance.py: update_reference, one thread, every operation rounded once in fp64, the new lambda rounded once to fp32.
__global__ __launch_bounds__(64) void dpn_balance_update_kernel(const double* sumsq, int K, double momentum, double lam_min, double lam_max, float* lam,
                                                                double* diag) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double nrm[MAX_TERMS];
    bool act[MAX_TERMS];
    bool bad = false;
    double tot = 0.0, n_act = 0.0;
    for (int k = 0; k < K; ++k) {
        const double s = sumsq[k];
        if (!finite64(s)) bad = true;
        nrm[k] = sqrt(s);
        act[k] = finite64(nrm[k]) && nrm[k] > 0.0;
        if (act[k]) { tot = tot + nrm[k]; n_act = n_act + 1.0; }
    }
    const bool flag = bad || n_act < 2.0;
    const double mean = flag ? 0.0 : tot / n_act;
    for (int k = 0; k < K; ++k) {
        const double old = (double)lam[k];
        double hat = 0.0, now = old;
        if (!flag && act[k]) {
            hat = mean / nrm[k];
            hat = hat < lam_min ? lam_min : hat;
            hat = hat > lam_max ? lam_max : hat;
            const float l32 = (float)(momentum * old + (1.0 - momentum) * hat);
            lam[k] = l32;
            now = (double)l32;
        }
        diag[k] = nrm[k]; diag[K + k] = hat; diag[2 * K + k] = now;
    }
    diag[3 * K] = mean; diag[3 * K + 1] = flag ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------ combine
struct CombineArgs {
    const float* term[STEP_TERMS];               // interior terms [6], margin terms [6], data
    int map[STEP_TERMS];
    const float* lam;
    const float* cot_in;
    float* total;
    float* cot_out;
};

// Thread 0: total = lambda * data, + lambda * interior 0..5, + lambda * margin 0..5, fp32, every product and sum rounded once.  Threads 0..12:
// cot_out[i] = cot_in * lambda_map(i).
__global__ __launch_bounds__(64) void dpn_balance_combine_kernel(CombineArgs a) {
#pragma clang fp contract(off)
    const int i = threadIdx.x;
    if (a.cot_out && i < STEP_TERMS) a.cot_out[i] = *a.cot_in * a.lam[a.map[i]];
    if (a.total && i == 0) {
        float acc = a.lam[a.map[STEP_TERMS - 1]] * *a.term[STEP_TERMS - 1];
#pragma unroll
        for (int j = 0; j < STEP_TERMS - 1; ++j) acc = acc + a.lam[a.map[j]] * *a.term[j];
        *a.total = acc;
    }
}

}  // namespace

extern "C" {

int64_t dpn_balance_scratch_doubles(int n_tensors, const int64_t* numel) { return table_chunks(n_tensors, numel); }

int dpn_balance_sumsq(int n_tensors, const float* const* grads, const int64_t* numel, double* scratch_dev, double* sumsq_slot_dev, void* stream) {
    const int64_t chunks = table_chunks(n_tensors, numel);
    if (chunks == 0 || !grads || !scratch_dev || !sumsq_slot_dev) return -1;
    hipStream_t s = (hipStream_t)stream;
    int64_t base = 0;                                       // partials written by the launches before
    for (int t0 = 0; t0 < n_tensors; t0 += TABLE_TENSORS) {
        SumsqTable t;
        t.n = n_tensors - t0 < TABLE_TENSORS ? n_tensors - t0 : TABLE_TENSORS;
        int c = 0;
        for (int i = 0; i < t.n; ++i) {
            t.g[i] = grads[t0 + i];
            t.numel[i] = (int)numel[t0 + i];
            t.chunk_start[i] = c;
            c += (int)((numel[t0 + i] + CHUNK - 1) / CHUNK);
        }
        t.chunk_start[t.n] = c;
        hipLaunchKernelGGL(dpn_balance_sumsq_kernel, dim3((unsigned)c), dim3(THREADS), 0, s, t, scratch_dev + base);
        base += c;
    }
    hipLaunchKernelGGL(dpn_balance_sumsq_reduce_kernel, dim3(1), dim3(THREADS), 0, s, (const double*)scratch_dev, (int)chunks, sumsq_slot_dev);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_balance_update(const double* sumsq_dev, int K, double momentum, double lam_min, double lam_max, float* lambda_dev, double* diag_dev, void* stream) {
    if (!sumsq_dev || !lambda_dev || !diag_dev || K < 1 || K > MAX_TERMS) return -1;
    if (!(momentum >= 0.0 && momentum <= 1.0) || !finite_host(lam_min) || !finite_host(lam_max) || !(lam_min > 0.0 && lam_min <= 1.0 && lam_max >= 1.0))
        return -1;
    hipLaunchKernelGGL(dpn_balance_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq_dev, K, momentum, lam_min, lam_max, lambda_dev,
                       diag_dev);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_balance_combine(const float* const* terms, int K, const int* map, const float* lambda_dev, const float* cot_in_dev, float* total_dev,
                        float* cot_out_dev, void* stream) {
    if ((!terms && total_dev) || !map || !lambda_dev || K < 1 || K > MAX_TERMS || (!total_dev && !cot_out_dev) || (cot_out_dev && !cot_in_dev)) return -1;
    CombineArgs a;
    for (int i = 0; i < STEP_TERMS; ++i) {
        if (map[i] < 0 || map[i] >= K || (total_dev && !terms[i])) return -1;
        a.term[i] = terms ? terms[i] : nullptr;
        a.map[i] = map[i];
    }
    a.lam = lambda_dev; a.cot_in = cot_in_dev; a.total = total_dev; a.cot_out = cot_out_dev;
    hipLaunchKernelGGL(dpn_balance_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
