// Label-side evaluation of the validation pass (reference interface_physics.py:518-530 on the training batch, :629-745 on a validation
// sample): normalised predictions out_n [S][N][6] and labels [S][N][6] are read ONCE and reduced, per segment s (one field sample) and
// variable k (u, v, P, T, q, rho), to the sufficient statistics of the data loss and of the per-variable errors in physical units.
//
// A translation unit of its own: nothing here is shared with the training kernels, whose code objects stay what they were.
//
// Streaming kernel, 48 B per point.  A thread owns two consecutive points = 12 floats per side = three 16-byte loads per side (a pair starts
// at a multiple of 48 B from its segment's base, so it is 16-byte aligned whenever the base is; a base that is only 8-byte aligned -- a row
// slice of an odd number of points, an odd N with s odd -- takes six 8-byte loads instead: every row is 24 B, so 8-byte alignment always
// holds).  Per-thread values go to fp64 before the first addition; wave64 xor-shuffle reduction, the four waves of a block added in a fixed
// order, one row of DPN_EVAL_STATS doubles WRITTEN per block (no atomics), blocks of a segment added in a fixed order by the finish launch:
// results are bitwise reproducible.  The grid is (ceil(N / 512), S): a block never straddles two segments.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dpn_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPointsPerBlock = 2 * kThreads;

struct EvalArgs {
    const float *out_n, *labels;
    int64_t n;                   // points per segment
    DpnPhysics ph;
    float beta;
    int with_clip;
    double* partials;            // [S][blocks][DPN_EVAL_STATS]
};

// inverse_norm (:232-262) of one normalised value: multiply, then add (two roundings, like `v * std + mean` in torch), the three-factor
// min_max square, the optional clip of P, T, q, rho that lets NaN through (torch.clip).  The arithmetic of dpn_fields_out.
__device__ __forceinline__ float eval_denorm(const float out, const int k, const DpnPhysics& ph, const int with_clip) {
    float v;
    {
#pragma clang fp contract(off)
        const float prod = out * ph.std[k];
        v = prod + ph.mean[k];
        if (ph.sq_on[k]) { const float sq = v * v; v = sq + ph.sq_add[k]; }
    }
    if (with_clip && k >= 2) v = v != v ? v : fminf(fmaxf(v, ph.clip_lo[k]), ph.clip_hi[k]);
    return v;
}

struct Acc {
    double sl1, sq[6], ab[6], sd[6];
    float mx[6];
};

// one element (prediction o, label l of variable k) into the thread's accumulators; every fp32 operation is rounded on its own
__device__ __forceinline__ void eval_element(Acc& a, const float o, const float l, const int k, const EvalArgs& e) {
#pragma clang fp contract(off)
    const float dn = o - l;                                          // nn.SmoothL1Loss(beta) in normalised units (weights_loss.py:17-20)
    const float ad = fabsf(dn);
    const float half = 0.5f * dn;
    const float s = ad < e.beta ? __fdiv_rn(half * dn, e.beta) : ad - 0.5f * e.beta;
    a.sl1 += (double)s;
    const float d = eval_denorm(o, k, e.ph, e.with_clip) - eval_denorm(l, k, e.ph, e.with_clip);     // de-normalise both sides, subtract in fp32
    const float d2 = d * d;                                          // MSELoss's (a - b) ** 2 in fp32
    const float da = fabsf(d);
    a.sq[k] += (double)d2;
    a.ab[k] += (double)da;
    a.sd[k] += (double)d;
    a.mx[k] = fmaxf(a.mx[k], da);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kThreads) void dpn_label_errors_kernel(EvalArgs e) {
    const int64_t seg = blockIdx.y;
    const float* o = e.out_n + seg * e.n * 6;
    const float* l = e.labels + seg * e.n * 6;
    const int64_t p0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 2;       // first of this thread's two points
    Acc a;
    a.sl1 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { a.sq[k] = a.ab[k] = a.sd[k] = 0.0; a.mx[k] = 0.f; }
    if (p0 + 1 < e.n) {                                              // a whole pair: 12 floats per side
        float vo[12], vl[12];
        const bool wide = ((((uintptr_t)o) | ((uintptr_t)l)) & 15) == 0;          // uniform over the block
        if (wide) {
            const float4* o4 = reinterpret_cast<const float4*>(o + p0 * 6);
            const float4* l4 = reinterpret_cast<const float4*>(l + p0 * 6);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 x = o4[j], y = l4[j];
                vo[4 * j] = x.x; vo[4 * j + 1] = x.y; vo[4 * j + 2] = x.z; vo[4 * j + 3] = x.w;
                vl[4 * j] = y.x; vl[4 * j + 1] = y.y; vl[4 * j + 2] = y.z; vl[4 * j + 3] = y.w;
            }
        } else {
            const float2* o2 = reinterpret_cast<const float2*>(o + p0 * 6);
            const float2* l2 = reinterpret_cast<const float2*>(l + p0 * 6);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float2 x = o2[j], y = l2[j];
                vo[2 * j] = x.x; vo[2 * j + 1] = x.y;
                vl[2 * j] = y.x; vl[2 * j + 1] = y.y;
            }
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) eval_element(a, vo[j], vl[j], j % 6, e);
    } else if (p0 < e.n) {                                           // the odd last point of the segment
#pragma unroll
        for (int k = 0; k < 6; ++k) eval_element(a, o[p0 * 6 + k], l[p0 * 6 + k], k, e);
    }
    __shared__ double red[kThreads / 64][DPN_EVAL_STATS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double v = wave_sum(a.sl1);
    if (lane == 0) red[w][0] = v;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double s2 = wave_sum(a.sq[k]), s1 = wave_sum(a.ab[k]), s0 = wave_sum(a.sd[k]);
        const float m = wave_max(a.mx[k]);
        if (lane == 0) { red[w][1 + k] = s2; red[w][7 + k] = s1; red[w][13 + k] = s0; red[w][19 + k] = (double)m; }
    }
    __syncthreads();
    if (threadIdx.x < DPN_EVAL_STATS) {
        const int j = threadIdx.x;
        const double r = j < 19 ? (red[0][j] + red[1][j]) + (red[2][j] + red[3][j])
                                : fmax(fmax(red[0][j], red[1][j]), fmax(red[2][j], red[3][j]));
        e.partials[(seg * gridDim.x + blockIdx.x) * DPN_EVAL_STATS + j] = r;
    }
}

// stats[s][j] = the blocks' rows of segment s added (j < 19) or maximised (j >= 19): wave w takes the statistics w, w + 4, ..., lane i the
// blocks i, i + 64, ... in ascending order, then the xor tree -- one fixed order whatever the grid.
__global__ __launch_bounds__(kThreads) void dpn_label_errors_finish_kernel(const double* partials, int64_t blocks, double* stats) {
    const int64_t seg = blockIdx.x;
    const double* p = partials + seg * blocks * DPN_EVAL_STATS;
    const int lane = threadIdx.x & 63;
    for (int j = threadIdx.x >> 6; j < DPN_EVAL_STATS; j += kThreads / 64) {
        double r = 0.0;
        if (j < 19) {
            for (int64_t b = lane; b < blocks; b += 64) r += p[b * DPN_EVAL_STATS + j];
            r = wave_sum(r);
        } else {
            for (int64_t b = lane; b < blocks; b += 64) r = fmax(r, p[b * DPN_EVAL_STATS + j]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) r = fmax(r, __shfl_xor(r, o));
        }
        if (lane == 0) stats[seg * DPN_EVAL_STATS + j] = r;
    }
}

}  // namespace

extern "C" {

int64_t dpn_label_errors_blocks(int64_t n_points) { return n_points <= 0 ? 0 : (n_points + kPointsPerBlock - 1) / kPointsPerBlock; }

int dpn_label_errors(const float* out_n, const float* labels, int64_t n_points, int segments, const DpnPhysics* phys, float beta, int with_clip,
                     double* partials, void* stream) {
    if (!out_n || !labels || !phys || !partials || n_points <= 0 || segments <= 0 || segments > 65535 || !(beta > 0.f)) return -1;
    if ((((uintptr_t)out_n) | ((uintptr_t)labels)) & 7) return -1;                  // rows are read as 8- or 16-byte vectors
    const int64_t blocks = dpn_label_errors_blocks(n_points);
    if (blocks > 0x7fffffff) return -1;
    EvalArgs a{out_n, labels, n_points, *phys, beta, with_clip, partials};
    hipLaunchKernelGGL(dpn_label_errors_kernel, dim3((unsigned)blocks, (unsigned)segments), dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_label_errors_finish(const double* partials, int64_t n_points, int segments, double* stats, void* stream) {
    if (!partials || !stats || n_points <= 0 || segments <= 0) return -1;
    hipLaunchKernelGGL(dpn_label_errors_finish_kernel, dim3((unsigned)segments), dim3(kThreads), 0, (hipStream_t)stream, partials,
                       dpn_label_errors_blocks(n_points), stats);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
