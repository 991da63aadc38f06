/* Entry points of SHELVED EXPERIMENTS -- not part of the product library.
 *
 * libdpn_hip.so exports what include/dpn_hip.h declares: the path bench.py / train.py can reach.  The kernels below were built, measured and not adopted
 * (DESIGN.md sections 1, 4c; tools/experiments/README.md); they are compiled only with -DDPN_EXPERIMENTS, into deepphysinet_amd/libdpn_hip_exp.so
 * (`python -m deepphysinet_amd.build --experiments`; it also holds every product symbol, so one handle serves an experiment run), and the Python side
 * reaches them through deepphysinet_amd._lib.load_experiments() only when the matching frozen switch (deepphysinet_amd/config.py) is on. */
#ifndef DPN_HIP_EXPERIMENTS_H
#define DPN_HIP_EXPERIMENTS_H
#include "dpn_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Removed (last present at 3bc40f4): dpn_conv16_split / dpn_conv16_kp / dpn_conv16, the token convolution on pre-split f16 hi+lo planes, and
 * dpn_gemm16 / dpn_gemm16_partial_floats, the weight-gradient kernel as a general small GEMM (tools/experiments/README.md section 15). */

/* The problem description of that GEMM core, C[m][n] = sum_k A(m, k) B(n, k) (+ bias[n]) with element strides, A(m, k) = A[m * a_sm + k * a_sk],
 * B(n, k) = B[n * b_sn + k * b_sk], asum[m] = sum_k A(m, k) (optional).  No entry point takes it any more: dpn_wgrad16 (csrc/dpn_encoder_chain.hip)
 * expresses its problems in it internally, and deepphysinet_amd._lib mirrors it (tests/test_capi_cpu.py checks the mirror's layout). */
typedef struct DpnGemm16Problem {
    const float* A; const float* B; float* C; float* asum; const float* bias;
    int32_t M, N, K, ldc;
    int64_t a_sm, a_sk, b_sn, b_sk;
} DpnGemm16Problem;

/* BASELINE configs[4] experiment (OFF in the product; DPN_ENCODER_FP8=1 routes the encoder layers' forward GEMMs here): C[M][N] =
 * epilogue(A[M][K] . W[N][K]^T + bias[N]) on the fp8 matrix cores (OCP e4m3 operands quantised in the kernel with one scale per row of A
 * and per row of W, fp32 accumulate); K a multiple of 16, lda / ldw multiples of 4; epi = DPN_EPI_NONE or DPN_EPI_GELU (aux_out
 * receives the pre-activation).  Replaces nothing of the reference by default: its measured parity error is why. */
int dpn_gemm_fp8(int M, int N, int K, const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int epi,
                 float* aux_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
