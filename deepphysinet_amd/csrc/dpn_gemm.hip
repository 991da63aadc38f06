// MI355X (gfx950 / CDNA4): the exact-fp32 GEMM family of the per-field tensors (encoder, hyper-network heads).  A unit of its own.
//
// Kernel inventory
//   dpn_sgemm_kernel / dpn_sgemm_reduce_kernel     one LDS-tiled fp32 GEMM, optionally split-K with a fixed-order second pass
//   dpn_sgemm_batch_kernel                         several GEMMs in one launch on the exact-fp32 MFMA, fused epilogues, ride-along column sums
//   dpn_sgemm_ln_kernel                            LayerNorm (forward or backward) folded into the consumer GEMM's A operand
// No kernel in this file uses atomics: every reduction is fixed-order, the whole step is bitwise reproducible.
#include "dpn_device.h"

// ------------------------------------------------------------------------------------------------ small fp32 GEMM
// The encoder (L = 287 tokens, d = 256) and the hyper-network heads are a few dozen tiny fp32 GEMMs per step; library
// GEMMs cost 19-75 us each at these shapes (latency-bound).  One LDS-tiled fp32 kernel serves all of them:
//   C[M][N] = op(A)[M][K] * op(B)[K][N] (+ bias[N]) (+ C)      op = identity or transpose, row-major with leading dims
//   optionally colsum[N] = sum_m op(A)^T ... is NOT needed; instead rowsum of op(A)^T is offered through `asum`:
//   asum[M] = sum_k op(A)[m][k]  (used as the bias gradient when op(A) = grad_out^T).
struct SgemmArgs {
    const float *A, *B, *bias;
    float *C, *asum, *ws;
    int M, N, K, lda, ldb, ldc, ta, tb, accumulate, k_per_split;
};

__global__ __launch_bounds__(256) void dpn_sgemm_kernel(SgemmArgs a) {
    constexpr int BM = 32, BN = 32, BK = 32;
    __shared__ float As[BK][BM + 1];
    __shared__ float Bs[BK][BN + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;      // 16 x 16 threads, 2 x 2 outputs each
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int kbeg = blockIdx.z * a.k_per_split;
    const int kend = (kbeg + a.k_per_split < a.K) ? kbeg + a.k_per_split : a.K;
    const bool split = gridDim.z > 1;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    float rs = 0.f;
    const bool do_asum = a.asum != nullptr && blockIdx.x == 0;
    float ra[4], rb[4];
    auto gload = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;                  // 1024 elements per tile
            {
                const int kk = a.ta ? (e >> 5) : (e & 31), mm = a.ta ? (e & 31) : (e >> 5);
                const int gm = m0 + mm, gk = k0 + kk;
                ra[i] = (gm < a.M && gk < kend) ? (a.ta ? a.A[(int64_t)gk * a.lda + gm] : a.A[(int64_t)gm * a.lda + gk]) : 0.f;
            }
            {
                const int kk = a.tb ? (e & 31) : (e >> 5), nn = a.tb ? (e >> 5) : (e & 31);
                const int gk = k0 + kk, gn = n0 + nn;
                rb[i] = (gk < kend && gn < a.N) ? (a.tb ? a.B[(int64_t)gn * a.ldb + gk] : a.B[(int64_t)gk * a.ldb + gn]) : 0.f;
            }
        }
    };
    gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + 256 * i;
            As[a.ta ? (e >> 5) : (e & 31)][a.ta ? (e & 31) : (e >> 5)] = ra[i];
            Bs[a.tb ? (e & 31) : (e >> 5)][a.tb ? (e >> 5) : (e & 31)] = rb[i];
        }
        __syncthreads();
        if (k0 + BK < kend) gload(k0 + BK);                       // next tile in flight under the FMAs
#pragma unroll
        for (int kk = 0; kk < BK; ++kk) {
            const float a0 = As[kk][ty], a1 = As[kk][ty + 16], b0 = Bs[kk][tx], b1 = Bs[kk][tx + 16];
            acc[0][0] = fmaf(a0, b0, acc[0][0]); acc[0][1] = fmaf(a0, b1, acc[0][1]);
            acc[1][0] = fmaf(a1, b0, acc[1][0]); acc[1][1] = fmaf(a1, b1, acc[1][1]);
        }
        if (do_asum && threadIdx.x < BM) {
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) rs += As[kk][threadIdx.x];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gm = m0 + ty + 16 * i, gn = n0 + tx + 16 * j;
            if (gm < a.M && gn < a.N) {
                if (split) {                                      // deterministic split-K: partial tile -> workspace[z][M][N]
                    a.ws[((int64_t)blockIdx.z * a.M + gm) * a.N + gn] = acc[i][j];
                } else {
                    const float v = acc[i][j] + (a.bias ? a.bias[gn] : 0.f);
                    float* c = a.C + (int64_t)gm * a.ldc + gn;
                    *c = a.accumulate ? (*c + v) : v;
                }
            }
        }
    if (do_asum && threadIdx.x < BM && m0 + threadIdx.x < a.M) {
        if (split) a.ws[(int64_t)gridDim.z * a.M * a.N + (int64_t)blockIdx.z * a.M + m0 + threadIdx.x] = rs;
        else a.asum[m0 + threadIdx.x] = rs;
    }
}

// second pass of the split-K path: fixed-order sum over the splits (+ bias, + C)
__global__ __launch_bounds__(256) void dpn_sgemm_reduce_kernel(SgemmArgs a, int splits) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t mn = (int64_t)a.M * a.N;
    if (idx < mn) {
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += a.ws[z * mn + idx];
        const int gm = (int)(idx / a.N), gn = (int)(idx % a.N);
        v += a.bias ? a.bias[gn] : 0.f;
        float* c = a.C + (int64_t)gm * a.ldc + gn;
        *c = a.accumulate ? (*c + v) : v;
    }
    if (a.asum && idx < a.M) {
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += a.ws[splits * mn + (int64_t)z * a.M + idx];
        a.asum[idx] = v;
    }
}

// Several independent small GEMMs in ONE launch (blockIdx.z = problem), each optionally a sum of up to 3 products
// (C = sum_t op(A_t) op(B_t)): the three q/k/v projections of an attention layer, or the input- and weight-gradient
// GEMMs of a linear layer, cost one launch instead of 2-6.  Two k-tiles are kept in flight in registers.
constexpr int kBatchMaxProblems = DPN_GEMM_MAX_PROBLEMS, kBatchMaxTerms = DPN_GEMM_MAX_TERMS, kBatchTermPool = 32, kBatchMaxJobs = DPN_GEMM_MAX_JOBS;
struct SgemmTerm {
    const float* A;
    const float* B;
    int lda, ldb, K, pad;
};
struct SgemmProblem {
    const float* bias;
    float *C, *asum;
    const float* aux;          // epilogue operand [M][ldc] (epi 2, 3)
    float* aux_out;            // pre-activation output [M][ldc] (epi 1, optional)
    int M, N, ldc, ta, tb, nterms, term0, epi;
};
// exact-erf GELU and its derivative, the formulas of torch's GeluCUDAKernelImpl / GeluBackwardCUDAKernelImpl (approximate='none')
DEV float gelu_exact(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }
DEV float gelu_exact_grad(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;      // M_2_SQRTPI * M_SQRT1_2 * 0.5
    return cdf + x * pdf;
}
struct SgemmColsum { const float* partial; float* out_a; float* out_b; int nblocks, pad; };
struct SgemmBatch {
    SgemmProblem p[kBatchMaxProblems];
    SgemmTerm t[kBatchTermPool];          // the accumulated A.B terms of all problems (problem i owns t[term0 .. term0+nterms))
    SgemmColsum job[kBatchMaxJobs];       // ride-along column sums (LayerNorm parameter gradients): blockIdx.z = n, n + 1, ...
    int n;
};

// exact-fp32 matrix cores: v_mfma_f32_32x32x2_f32 (A: lane l holds A[l&31][l>>5], B: lane l holds B[l>>5][l&31]); bitwise an fmaf chain.
typedef float f32x1;
DEV f32x16 mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

template <int BK, int NBUF, int NT = 256, int TM = 1, int TN = 1>
__global__ __launch_bounds__(NT) void dpn_sgemm_batch_kernel(SgemmBatch batch) {
    // one workgroup = one 32x32 output tile.  K is walked in 32-wide tiles that are loaded COALESCED (the fast index follows each
    // operand's contiguous dimension) into double-buffered LDS, two tiles ahead in registers; inside a tile the four waves take
    // BK/4 k-values each (v_mfma_f32_32x32x2_f32, exact fp32) and their partial tiles are summed through LDS in a fixed order.
    // <64, 2>: double-buffered LDS, two k-tiles in flight (long / multi-term reductions); 64-deep tiles = 34 KB of LDS = four
    // workgroups per CU, so the 500-800 tiles of a backward launch are one round (128-deep: two per CU, measured +7 us per step;
    // 96-deep: slower, the non-power-of-two index arithmetic).  <256, 1>: the whole K of a 256-wide encoder
    // GEMM is ONE tile -- one LDS stage, one barrier pair, 16 loads per operand in flight (used when every problem is a single tile);
    // it runs with EIGHT waves (NT = 512): half the MFMA chain and half the loads per thread of a latency-bound tile, -15 us per step.
    // Round 6: TM x TN 32 x 32 sub-tiles per workgroup (<64, 2, 512, 2, 2>: a 64 x 64 output tile, each of its four quadrants on two waves that split the
    // k-values of a k-tile): half the L2 -> LDS traffic per MAC of the 32 x 32 form (a 32 x 32 tile loads 2 x 32 x K values for 32 x 32 x K MACs: the token
    // convolution moved 74 MB through L2 for 12 MB of operands) and four times the MFMA work per barrier.
    constexpr int BM = 32 * TM, BN = 32 * TN, NLA = BK * BM / NT, NLB = BK * BN / NT;    // loads per operand per thread per k-tile
    constexpr int NW = NT / 64, NQ = TM * TN, KW = NW / NQ;   // waves; sub-tiles; waves per sub-tile, each taking BK / KW k-values of a k-tile
    static_assert(NW % NQ == 0 && BK % (2 * KW) == 0 && (BK * BM) % NT == 0 && (BK * BN) % NT == 0, "tile shape");
    // (Round 6: XCD-contiguous renumbering of the workgroups -- every XCD a contiguous range of the (problem, tile) list, as in dpn_pack_fused_kernel -- is SLOWER
    //  here: the heads' forward 16.2 -> 22.4 us, their backward 27.1 -> 48 us, the token convolution unchanged: a problem's tiles on ONE L2 queue on the same
    //  lines; spread over eight L2s each serves an eighth of them.  A skew of the column tile by (row tile + 3 problem), so that tiles sharing a B panel
    //  leave the XCD they share when gridDim.x is a multiple of 8, changes nothing.  profiles/round6_xcd_contiguous.txt)
    const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (bz >= batch.n) {
        // ride-along job: out_a[c] = sum_b partial[b][c], out_b[c] = sum_b partial[b][256 + c] (fixed order) -- the reduction of
        // dpn_add_ln_bwd's per-block partial sums, finished in the shadow of the GEMM tiles instead of in a launch of its own
        if (bx || by) return;
        const SgemmColsum& j = batch.job[bz - batch.n];
        const int c = threadIdx.x;
        if (c >= 256) return;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll 8
        for (int b = 0; b < j.nblocks; ++b) { s1 += j.partial[(int64_t)b * 512 + c]; s2 += j.partial[(int64_t)b * 512 + 256 + c]; }
        j.out_a[c] = s1;
        j.out_b[c] = s2;
        return;
    }
    const SgemmProblem& a = batch.p[bz];
    const int m0 = by * BM, n0 = bx * BN;
    if (m0 >= a.M || n0 >= a.N) return;
    // 34 KB (<64,2>) or 68 KB (<256,1>) of LDS: four or two workgroups per CU.  The partial tiles of the waves (eight: 33 KB) reuse the
    // staging buffers after the last k-tile.  Both forms run with eight waves: -15 us (<256,1>) and -53 us (<64,2>) per step against four.
    struct Stage { float A[NBUF][BK][BM + 1]; float B[NBUF][BK][BN + 1]; };
    __shared__ Stage stage;
    float (&As)[NBUF][BK][BM + 1] = stage.A;
    float (&Bs)[NBUF][BK][BN + 1] = stage.B;
    float (*part)[32 * 33] = reinterpret_cast<float (*)[32 * 33]>(&stage);           // the partial tiles reuse the staging buffers
    const int wave_q = (threadIdx.x >> 6) % NQ, wave_k = (threadIdx.x >> 6) / NQ, qm = wave_q / TN, qn = wave_q % TN;
    static_assert(sizeof(Stage) >= NW * 32 * 33 * sizeof(float), "partial tiles must fit in the staging buffers");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    f32x16 acc = (f32x16)0.f;
    float rs = 0.f;
    const bool do_asum = a.asum != nullptr && bx == 0;
    int total = 0;
    for (int t = 0; t < a.nterms; ++t) total += (batch.t[a.term0 + t].K + BK - 1) / BK;
    const int ktiles0 = (batch.t[a.term0].K + BK - 1) / BK;
    float ra[NLA], rb[NLB];
    int lt = 0, lk0 = 0;                     // load cursor: term, k offset inside the term (terms may have different K)
    auto gload = [&]() __attribute__((always_inline)) {
        const SgemmTerm& T = batch.t[a.term0 + lt];
        const float* A = T.A;
        const float* B = T.B;
        const int lda = T.lda, ldb = T.ldb, K = T.K, k0 = lk0;
#pragma unroll
        for (int q = 0; q < NLA; ++q) {
            const int e = threadIdx.x + NT * q;
            const int kk = a.ta ? (e / BM) : (e % BK), mm = a.ta ? (e % BM) : (e / BK);
            const int gm = m0 + mm, gk = k0 + kk;
            ra[q] = (gm < a.M && gk < K) ? (a.ta ? A[(int64_t)gk * lda + gm] : A[(int64_t)gm * lda + gk]) : 0.f;
        }
#pragma unroll
        for (int q = 0; q < NLB; ++q) {
            const int e = threadIdx.x + NT * q;
            const int kk = a.tb ? (e % BK) : (e / BN), nn = a.tb ? (e / BK) : (e % BN);
            const int gk = k0 + kk, gn = n0 + nn;
            rb[q] = (gk < K && gn < a.N) ? (a.tb ? B[(int64_t)gn * ldb + gk] : B[(int64_t)gk * ldb + gn]) : 0.f;
        }
        lk0 += BK;
        if (lk0 >= K) { lk0 = 0; ++lt; }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NLA; ++q) {
            const int e = threadIdx.x + NT * q;
            As[buf][a.ta ? (e / BM) : (e % BK)][a.ta ? (e % BM) : (e / BK)] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < NLB; ++q) {
            const int e = threadIdx.x + NT * q;
            Bs[buf][a.tb ? (e % BK) : (e / BN)][a.tb ? (e / BK) : (e % BN)] = rb[q];
        }
    };
    if constexpr (NBUF == 2) {
        gload();
        lstore(0);
        if (total > 1) gload();
        __syncthreads();
        for (int it = 0; it < total; ++it) {
            const int buf = it & 1;
            if (it + 1 < total) lstore(buf ^ 1);                  // tile it+1 (loaded during the previous iteration) -> other LDS buffer
            if (it + 2 < total) gload();                          // tile it+2 in flight under the MFMAs
#pragma unroll
            for (int u = 0; u < BK / (2 * KW); ++u) {
                const int kk = wave_k * (BK / KW) + 2 * u + h;
                acc = mfma_f32(As[buf][kk][32 * qm + i], Bs[buf][kk][32 * qn + i], acc);
            }
            if (do_asum && it < ktiles0 && threadIdx.x < BM) {
#pragma unroll
                for (int kk = 0; kk < BK; ++kk) rs += As[buf][kk][threadIdx.x];
            }
            __syncthreads();
        }
    } else {
        gload();
        for (int it = 0; it < total; ++it) {
            lstore(0);
            __syncthreads();
            if (it + 1 < total) gload();                          // next tile in flight under the MFMAs
#pragma unroll 8
            for (int u = 0; u < BK / (2 * KW); ++u) {
                const int kk = wave_k * (BK / KW) + 2 * u + h;
                acc = mfma_f32(As[0][kk][32 * qm + i], Bs[0][kk][32 * qn + i], acc);
            }
            if (do_asum && it < ktiles0 && threadIdx.x < BM) {
#pragma unroll 8
                for (int kk = 0; kk < BK; ++kk) rs += As[0][kk][threadIdx.x];
            }
            __syncthreads();
        }
    }
    // ---- fixed-order reduction over the waves of a sub-tile (wave = wave_k * NQ + wave_q)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave][drow32(r, h) * 33 + i] = acc[r];
    __syncthreads();
#pragma unroll
    for (int e = threadIdx.x; e < 1024 * NQ; e += NT) {
        const int sq = e >> 10, r = (e >> 5) & 31, c = e & 31, o = r * 33 + c;
        const int gr = m0 + 32 * (sq / TN) + r, gc = n0 + 32 * (sq % TN) + c;
        if (gr < a.M && gc < a.N) {
            float v = part[sq][o];
#pragma unroll
            for (int w_ = 1; w_ < KW; ++w_) v += part[w_ * NQ + sq][o];     // fixed order: k-part 0, 1, ... (left fold)
            v += a.bias ? a.bias[gc] : 0.f;
            const int64_t idx = (int64_t)gr * a.ldc + gc;
            if (a.epi == DPN_EPI_GELU) { if (a.aux_out) a.aux_out[idx] = v; v = gelu_exact(v); }
            else if (a.epi == DPN_EPI_MUL_GELU_GRAD) v *= gelu_exact_grad(a.aux[idx]);
            else if (a.epi == DPN_EPI_ADD) v += a.aux[idx];
            a.C[idx] = v;
        }
    }
    if (do_asum && threadIdx.x < BM && m0 + threadIdx.x < a.M) a.asum[m0 + threadIdx.x] = rs;
}

// ------------------------------------------------------------------------------------------------ LayerNorm folded into a GEMM's A operand
// A dependent kernel costs >= 4.5 us on this machine whatever it does, and LayerNorm (forward or backward) on 287 x 256 does almost
// nothing.  Its consumer is always a GEMM over the FULL 256-wide rows (K = d_model = 256 = one LDS tile), so the consumer can apply it
// to its own A tile: every workgroup of a row block recomputes the 32 row statistics (cheap), the n0 == 0 workgroups write the
// normalised rows / statistics (forward) or the row gradients and the per-block parameter partial sums (backward) for later use.
//   mode 1:  A = LN(x + r) * gamma + beta      (writes y, xhat, rstd)                       -- transformer_net.py:37,44
//   mode 2:  A = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat))               (writes gs and partial[block][2][256])
struct LnGemmArgs {
    int mode, M, N, tb, ldb, ldc, epi;
    const float *x, *r, *gamma, *beta, *rstd_in;
    float *y_out, *xhat_out, *rstd_out, *partial;
    const float *B, *bias;
    float* C;
    const float* aux;
    float* aux_out;
};
template <int MODE, int NT = 512>
__global__ __launch_bounds__(NT) void dpn_sgemm_ln_kernel(LnGemmArgs a) {
    constexpr int BK = 256;
    constexpr int NW = NT / 64;                 // waves: BK / NW k-values each (eight: half the MFMA chain and loads of a latency-bound tile)
    constexpr int TPR = NT / 32, CW = 256 / TPR;  // threads per row of the A tile, columns per thread
    __shared__ float As[BK][33];
    __shared__ float Bs[BK][33];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const bool keep = blockIdx.x == 0;
    // ---- B tile -> registers (stored to LDS after the LayerNorm phase, which may borrow Bs)
    constexpr int NLB = BK * 32 / NT;
    float rb[NLB];
#pragma unroll
    for (int q = 0; q < NLB; ++q) {
        const int e = t + NT * q;
        const int kk = a.tb ? (e & 255) : (e >> 5), nn = a.tb ? (e >> 8) : (e & 31);
        const int gn = n0 + nn;
        rb[q] = (gn < a.N) ? (a.tb ? a.B[(int64_t)gn * a.ldb + kk] : a.B[(int64_t)kk * a.ldb + gn]) : 0.f;
    }
    // ---- A rows in registers: thread t holds columns [CW c, CW c + CW) of row m (c = t % TPR, m = t / TPR): a row is TPR adjacent lanes,
    // so the row statistics are log2(TPR) xor-shuffles -- no LDS pass, no barrier
    const int m = t / TPR, c0 = (t % TPR) * CW, gm = m0 + m;
    const bool ok = gm < a.M;
    float v[CW], w[MODE == 2 ? CW : 1], gam[CW];
#pragma unroll
    for (int j = 0; j < CW / 4; ++j) {
        const float4 x4 = ok ? *reinterpret_cast<const float4*>(a.x + (int64_t)gm * 256 + c0 + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 g4 = *reinterpret_cast<const float4*>(a.gamma + c0 + 4 * j);
        v[4 * j] = x4.x; v[4 * j + 1] = x4.y; v[4 * j + 2] = x4.z; v[4 * j + 3] = x4.w;
        gam[4 * j] = g4.x; gam[4 * j + 1] = g4.y; gam[4 * j + 2] = g4.z; gam[4 * j + 3] = g4.w;
        if (MODE == 1) {
            if (ok && a.r) {
                const float4 r4 = *reinterpret_cast<const float4*>(a.r + (int64_t)gm * 256 + c0 + 4 * j);
                v[4 * j] += r4.x; v[4 * j + 1] += r4.y; v[4 * j + 2] += r4.z; v[4 * j + 3] += r4.w;
            }
        } else {
            const float4 r4 = ok ? *reinterpret_cast<const float4*>(a.r + (int64_t)gm * 256 + c0 + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            w[4 * j] = r4.x; w[4 * j + 1] = r4.y; w[4 * j + 2] = r4.z; w[4 * j + 3] = r4.w;
        }
    }
    auto row_sum = [&](float s_) __attribute__((always_inline)) {            // over the 8 lanes of the row, fixed order
        s_ += __shfl_xor(s_, 1); s_ += __shfl_xor(s_, 2); s_ += __shfl_xor(s_, 4);
        if constexpr (TPR == 16) s_ += __shfl_xor(s_, 8);
        return s_;
    };
    if (MODE == 2 && keep) {
        // parameter partial sums of this row block need g and xhat column-wise: park them in As / Bs (both still unused), one pass
#pragma unroll
        for (int j = 0; j < CW; ++j) { As[c0 + j][m] = v[j]; Bs[c0 + j][m] = w[j]; }
        __syncthreads();
        if (t < 256) {
            float dg = 0.f, db = 0.f;
#pragma unroll 8
            for (int q = 0; q < 32; ++q) { dg = fmaf(As[t][q], Bs[t][q], dg); db += As[t][q]; }
            a.partial[(int64_t)blockIdx.y * 512 + t] = dg;
            a.partial[(int64_t)blockIdx.y * 512 + 256 + t] = db;
        }
        __syncthreads();
    }
    if (MODE == 1) {
        float s_ = 0.f;
#pragma unroll
        for (int j = 0; j < CW; ++j) s_ += v[j];
        const float mean = row_sum(s_) * (1.f / 256.f);
        float q_ = 0.f;
#pragma unroll
        for (int j = 0; j < CW; ++j) { const float d = v[j] - mean; q_ = fmaf(d, d, q_); }
        const float rstd = 1.0f / sqrtf(row_sum(q_) * (1.f / 256.f) + 1e-5f);
        if (keep && ok && (t % TPR) == 0) a.rstd_out[gm] = rstd;
#pragma unroll
        for (int j = 0; j < CW / 4; ++j) {
            const float4 b4 = *reinterpret_cast<const float4*>(a.beta + c0 + 4 * j);
            const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
            float xh[4], yy[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { xh[e] = (v[4 * j + e] - mean) * rstd; yy[e] = fmaf(xh[e], gam[4 * j + e], bb[e]); v[4 * j + e] = yy[e]; }
            if (keep && ok) {
                *reinterpret_cast<float4*>(a.xhat_out + (int64_t)gm * 256 + c0 + 4 * j) = make_float4(xh[0], xh[1], xh[2], xh[3]);
                *reinterpret_cast<float4*>(a.y_out + (int64_t)gm * 256 + c0 + 4 * j) = make_float4(yy[0], yy[1], yy[2], yy[3]);
            }
        }
    } else {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < CW; ++j) { const float tk = v[j] * gam[j]; s1 += tk; s2 = fmaf(tk, w[j], s2); }
        const float m1 = row_sum(s1) * (1.f / 256.f), m2 = row_sum(s2) * (1.f / 256.f);
        const float rs_ = ok ? a.rstd_in[gm] : 0.f;
#pragma unroll
        for (int j = 0; j < CW / 4; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * j + e] = rs_ * (v[4 * j + e] * gam[4 * j + e] - m1 - w[4 * j + e] * m2);
            if (keep && ok) *reinterpret_cast<float4*>(a.y_out + (int64_t)gm * 256 + c0 + 4 * j) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
        }
    }
    // ---- transformed A tile and B tile -> LDS
#pragma unroll
    for (int j = 0; j < CW; ++j) As[c0 + j][m] = v[j];
#pragma unroll
    for (int q = 0; q < NLB; ++q) {
        const int e = t + NT * q;
        Bs[a.tb ? (e & 255) : (e >> 5)][a.tb ? (e >> 8) : (e & 31)] = rb[q];
    }
    __syncthreads();
    // ---- the GEMM proper: NW waves x BK / NW k each (exact fp32 MFMA), partial tiles joined in a fixed order
    f32x16 acc = (f32x16)0.f;
#pragma unroll 8
    for (int u = 0; u < BK / (2 * NW); ++u) {
        const int kk = wave * (BK / NW) + 2 * u + h;
        acc = mfma_f32(As[kk][i], Bs[kk][i], acc);
    }
    __syncthreads();
    float (*partt)[32 * 33] = reinterpret_cast<float (*)[32 * 33]>(&As[0][0]);
#pragma unroll
    for (int r = 0; r < 16; ++r) partt[wave][drow32(r, h) * 33 + i] = acc[r];
    __syncthreads();
#pragma unroll
    for (int e = t; e < 1024; e += NT) {
        const int r = e >> 5, c = e & 31, o = r * 33 + c;
        if (m0 + r < a.M && n0 + c < a.N) {
            float vv = partt[0][o];
#pragma unroll
            for (int w_ = 1; w_ < NW; ++w_) vv += partt[w_][o];            // fixed order: wave 0, 1, ... (left fold)
            vv += a.bias ? a.bias[n0 + c] : 0.f;
            const int64_t idx = (int64_t)(m0 + r) * a.ldc + n0 + c;
            if (a.epi == DPN_EPI_GELU) { if (a.aux_out) a.aux_out[idx] = vv; vv = gelu_exact(vv); }
            else if (a.epi == DPN_EPI_MUL_GELU_GRAD) vv *= gelu_exact_grad(a.aux[idx]);
            else if (a.epi == DPN_EPI_ADD) vv += a.aux[idx];
            a.C[idx] = vv;
        }
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int dpn_sgemm(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
              const float* bias, float* asum, int accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = ((N + 31) / 32) * ((M + 31) / 32);
    int splits = 1;
    if (workspace && tiles < 256 && K >= 1024) {                 // long reductions with few output tiles: split K over the grid
        splits = (512 + tiles - 1) / tiles;
        const int maxs = K / 256;
        if (splits > maxs) splits = maxs;
        if (splits > 32) splits = 32;
        while (splits > 1 && (int64_t)splits * ((int64_t)M * N + M) * 4 > workspace_bytes) --splits;
        if (splits < 1) splits = 1;
    }
    int kps = (K + splits - 1) / splits;
    kps = ((kps + 31) / 32) * 32;
    splits = (K + kps - 1) / kps;
    SgemmArgs a{A, B, bias, C, asum, reinterpret_cast<float*>(workspace), M, N, K, lda, ldb, ldc, ta, tb, accumulate, kps};
    hipLaunchKernelGGL(dpn_sgemm_kernel, dim3((N + 31) / 32, (M + 31) / 32, splits), dim3(256), 0, s, a);
    if (splits > 1) {
        const int64_t work = (int64_t)M * N > M ? (int64_t)M * N : M;
        hipLaunchKernelGGL(dpn_sgemm_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, a, splits);
    }
    return ck(hipGetLastError());
}

// measured on the encoder backward (A2 phase): threshold 1 -> 778 us, 2 -> 804 us, 3 -> 798 us: multi-tile problems want the
// double-buffered <64,2> pipeline
constexpr int kSingleStageMaxTiles = 1;
constexpr long kSingleStageMaxOutTiles = 512;      // one round of <256,1>; thresholds 256 ... 700 measure the same, none or 1024 worse
static int sgemm_batch_launch(int n_problems, const DpnGemmProblem* problems, int n_jobs, const DpnColsumJob* jobs, void* stream) {
    if (n_problems <= 0 || n_problems > kBatchMaxProblems || !problems || n_jobs < 0 || n_jobs > kBatchMaxJobs || (n_jobs && !jobs)) return -1;
    static_assert(sizeof(SgemmBatch) <= 4096, "kernel arguments");
    SgemmBatch b;
    b.n = n_problems;
    int gx = 0, gy = 0, pool = 0;
    for (int i = 0; i < n_problems; ++i) {
        const DpnGemmProblem& q = problems[i];
        if (q.nterms < 1 || q.nterms > kBatchMaxTerms || pool + q.nterms > kBatchTermPool || !q.C || q.M <= 0 || q.N <= 0) return -1;
        if (q.epi < 0 || q.epi > DPN_EPI_ADD || ((q.epi == DPN_EPI_MUL_GELU_GRAD || q.epi == DPN_EPI_ADD) && !q.aux)) return -1;
        if (q.asum && q.nterms != 1) return -1;                       // row sums of A are defined for a single term
        SgemmProblem& p = b.p[i];
        p.term0 = pool;
        for (int t = 0; t < q.nterms; ++t) {
            const int kt = q.k_term[t] > 0 ? q.k_term[t] : q.K;
            if (!q.A[t] || !q.B[t] || kt <= 0) return -1;
            b.t[pool++] = SgemmTerm{q.A[t], q.B[t], q.lda[t], q.ldb[t], kt, 0};
        }
        p.bias = q.bias; p.C = q.C; p.asum = q.asum; p.aux = q.aux; p.aux_out = q.aux_out; p.epi = q.epi;
        p.M = q.M; p.N = q.N; p.ldc = q.ldc; p.ta = q.ta; p.tb = q.tb; p.nterms = q.nterms;
        gx = gx > (q.N + 31) / 32 ? gx : (q.N + 31) / 32;
        gy = gy > (q.M + 31) / 32 ? gy : (q.M + 31) / 32;
    }
    for (int i = 0; i < n_jobs; ++i) {
        if (!jobs[i].partial || !jobs[i].out_a || !jobs[i].out_b || jobs[i].n_blocks <= 0) return -1;
        b.job[i] = SgemmColsum{jobs[i].partial, jobs[i].out_a, jobs[i].out_b, jobs[i].n_blocks, 0};
    }
    const int gz = n_problems + n_jobs;
    // <256,1> (one LDS stage of 256 k) when every problem is a single such tile AND the launch is one round of it (68 KB of LDS: two
    // workgroups per CU, 512 at a time); launches with more output tiles than that (batches of fields: 548 row tiles per GEMM) run
    // better four to a CU in the pipelined <64,2> form (single field: 1.309 -> 1.286 ms per step, the heads' 728-tile launch among
    // them; configs[2]: 51.1 -> 50.4 ms)
    bool single_tile = true;
    long out_tiles = 0;
    for (int i = 0; i < n_problems; ++i) {
        int tiles = 0;
        for (int t = 0; t < b.p[i].nterms; ++t) tiles += (b.t[b.p[i].term0 + t].K + 255) / 256;
        single_tile = single_tile && tiles <= kSingleStageMaxTiles;
        out_tiles += (long)((b.p[i].M + 31) / 32) * ((b.p[i].N + 31) / 32);
    }
    single_tile = single_tile && out_tiles <= kSingleStageMaxOutTiles;
    if (single_tile) {
        hipLaunchKernelGGL((dpn_sgemm_batch_kernel<256, 1, 512>), dim3(gx, gy, gz), dim3(512), 0, reinterpret_cast<hipStream_t>(stream), b);
        return ck(hipGetLastError());
    }
    // Round 6: 64 x 64 output tiles (four 32 x 32 sub-tiles on eight waves: half the L2 -> LDS bytes per MAC) measured slower on every
    // launch of the step -- token convolution + assemble 27.3 against 25.0 us, the heads' forward 17.7 against 16.3, their backward 34.6 against 26.9 us: these
    // GEMMs wait for latency, not for L2 bytes (profiles/round6_sgemm_tile_ab.txt).  The kernel template keeps the parameters; the launch was removed.
    hipLaunchKernelGGL((dpn_sgemm_batch_kernel<64, 2, 512>), dim3(gx, gy, gz), dim3(512), 0, reinterpret_cast<hipStream_t>(stream), b);
    return ck(hipGetLastError());
}

int dpn_sgemm_batch(int n_problems, const DpnGemmProblem* problems, void* stream) {
    return sgemm_batch_launch(n_problems, problems, 0, nullptr, stream);
}

int dpn_sgemm_batch_jobs(int n_problems, const DpnGemmProblem* problems, int n_jobs, const DpnColsumJob* jobs, void* stream) {
    return sgemm_batch_launch(n_problems, problems, n_jobs, jobs, stream);
}

int dpn_sgemm_ln(const DpnLnGemm* q, void* stream) {
    if (!q || (q->mode != 1 && q->mode != 2) || q->M <= 0 || q->N <= 0 || !q->x || !q->gamma || !q->B || !q->C || !q->y_out) return -1;
    if (q->mode == 1 && (!q->beta || !q->xhat_out || !q->rstd_out)) return -1;
    if (q->mode == 2 && (!q->r || !q->rstd_in || !q->partial)) return -1;
    if (q->epi < 0 || q->epi > DPN_EPI_ADD || ((q->epi == DPN_EPI_MUL_GELU_GRAD || q->epi == DPN_EPI_ADD) && !q->aux)) return -1;
    LnGemmArgs a{q->mode, q->M, q->N, q->tb, q->ldb, q->ldc, q->epi, q->x, q->r, q->gamma, q->beta, q->rstd_in, q->y_out, q->xhat_out,
                 q->rstd_out, q->partial, q->B, q->bias, q->C, q->aux, q->aux_out};
    const dim3 grid((q->N + 31) / 32, (q->M + 31) / 32);
    if (q->mode == 1) hipLaunchKernelGGL((dpn_sgemm_ln_kernel<1, 512>), grid, dim3(512), 0, reinterpret_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL((dpn_sgemm_ln_kernel<2, 512>), grid, dim3(512), 0, reinterpret_cast<hipStream_t>(stream), a);
    return ck(hipGetLastError());
}

}  // extern "C"
