/* libdpn_hip.so -- C ABI of the MI355X (gfx950) point path of the DeepPhysiNet physics-informed step.
 *
 * The reference has no FFI layer: its hot path is Python calling torch ops
 * (DeepPhysiNet/model/variable_net.py:49-87, model/physics_net.py:41-55,
 * interface/interface_physics.py:90-185,232-332).  These entry points are what a
 * ctypes binding on the reference side would call instead;
 * plain device pointers and sizes, no torch types.  All pointers are DEVICE pointers
 * unless said otherwise; `stream` is a hipStream_t.  Every call only enqueues work on
 * `stream` (no allocation, no synchronisation: hipGraph-capturable).  Return value:
 * 0 on success, otherwise a hipError_t (launch/configuration errors) or -1 (bad argument).
 *
 * Precision modes (`prec`): 1 = bf16 MFMA operands, fp32 accumulate ("bf16");
 *                           2 = bf16 hi+lo split operands, 3 MFMAs per product ("bf16x2", fp32-class).
 * Everything that is not a GEMM operand (coordinates, positional features, de-normalisation,
 * residuals, reductions) is fp32 (loss sums fp64) in both modes.
 */
#ifndef DPN_HIP_H
#define DPN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DPN_NETS 6          /* u, v, P, T, q, rho   (physics_net.py:49-54) */
#define DPN_HIDDEN 256
#define DPN_PE 192

/* Per-VariableNet fp32 tensors of ONE field sample (device pointers).
 * w1b1 / w2b2 are the hyper-network heads' outputs (variable_net.py:59-65), evec is
 * fore_h_fc(PE(forecast_h)) (variable_net.py:75-78); the rest are the module's own parameters. */
typedef struct DpnNetPtrs {
    const float* w1b1;   /* [256][193]  rows: [w1 (192) | b1]            */
    const float* w2b2;   /* [256][257]  rows: [w2 (256) | b2]            */
    const float* evec;   /* [256]                                         */
    const float* Wd;     /* [256][192]  data_input_fc.weight             */
    const float* bd;     /* [256]       data_input_fc.bias               */
    const float* W1;     /* [256][256]  cat_fc1.fc.0.weight              */
    const float* bf1;    /* [256]       cat_fc1.fc.0.bias                */
    const float* W2;     /* [256][256]  cat_fc1.fc.2.weight              */
    const float* bf2;    /* [256]       cat_fc1.fc.2.bias                */
    const float* wo;     /* [256]       out_fc.weight                    */
    const float* bo;     /* [1]         out_fc.bias                      */
    int64_t ld_w1b1;     /* row stride of w1b1 in floats (>= 193): lets the six heads live in one GEMM output */
    int64_t ld_w2b2;     /* row stride of w2b2 in floats (>= 257)                                             */
} DpnNetPtrs;

/* Gradient destinations, same shapes as DpnNetPtrs (written, not accumulated). */
typedef struct DpnNetGradPtrs {
    float* w1b1; float* w2b2; float* evec; float* Wd; float* bd; float* W1; float* bf1; float* W2; float* bf2; float* wo; float* bo;
    int64_t ld_w1b1, ld_w2b2;   /* row strides (floats) of the w1b1 / w2b2 gradient destinations */
} DpnNetGradPtrs;

/* Grid constants of encoding_coord (interface_physics.py:322-332). */
typedef struct DpnGeometry {
    float dx, dy;            /* metres                                     */
    float lon_m1, lat_m1;    /* lon_size-1, lat_size-1                     */
    float pred_t_span;       /* seconds                                    */
} DpnGeometry;

/* De-normalisation, clip bounds and loss factors (configs/DeepPhysiNet_NCEP_cfg.py:64-76,139-148). */
typedef struct DpnPhysics {
    float mean[DPN_NETS], std[DPN_NETS];
    float clip_lo[DPN_NETS], clip_hi[DPN_NETS];
    int   clip_on[DPN_NETS];              /* with_clip && bounds apply to this field (u,v: never)  */
    float factor[DPN_NETS];               /* motion_u, motion_v, continuous, energy, vapor, gas     */
    int   criterion;                      /* the PDE criterion `loss(residual, 0)` (train_cfg.losses.pde_loss, interface_physics.py:384; the reference's
                                           * losses/builder.py offers these three): DPN_CRIT_MSE nn.MSELoss, DPN_CRIT_L1 nn.L1Loss, DPN_CRIT_SMOOTH_L1
                                           * WeightSmoothL1Loss(beta) = mean of nn.SmoothL1Loss(beta, reduction='none') (weights_loss.py:12-21)        */
    float beta;                           /* DPN_CRIT_SMOOTH_L1 only (> 0)                                                                        */
    int   sq_on[DPN_NETS];                /* inverse_norm's three-factor min_max form (interface_physics.py:244-247): v = (out * std + mean)^2 + sq_add,
                                           * std = nf[1] - nf[0], mean = nf[0], sq_add = nf[2]; 0: the affine forms                                 */
    float sq_add[DPN_NETS];
    int   reduce_sum;                     /* the criterion's reduction: 0 "mean" (shipped), 1 "sum" (`pde_loss=dict(name='MSELoss', reduction='sum')`)       */
} DpnPhysics;
enum { DPN_CRIT_MSE = 0, DPN_CRIT_L1 = 1, DPN_CRIT_SMOOTH_L1 = 2 };

/* Byte sizes of the caller-allocated work buffers for n_points collocation points. */
typedef struct DpnSizes {
    int64_t n_pad;           /* points padded to the tile size                              */
    int64_t packed;          /* packed bf16 weight fragments + fp32 vectors, all 6 nets     */
    int64_t saved;           /* per-point state saved by dpn_fwd for the backward pass      */
    int64_t operands;        /* per-point operands written by dpn_bwd_points                */
    int64_t partials;        /* split-K partial weight gradients                            */
    int32_t k_splits;        /* number of point ranges dpn_wgrad splits the reduction into  */
} DpnSizes;

int dpn_version(void);
int dpn_sizes(int64_t n_points, int prec, DpnSizes* out);

/* Measurement aid (bench.py): one-thread kernel that appends the device's constant-rate clock (wall_clock64) to ring[cursor++ % cap].  Capturable:
 * it brackets a launch INSIDE a replayed hipGraph, where a HIP event pair cannot be used (event records in a capture are dependencies, not timers).
 * dpn_clock_rate_khz: the counter's rate (hipDeviceAttributeWallClockRate). */
int dpn_clock_stamp(unsigned long long* ring, unsigned int* cursor, unsigned int cap, void* stream);
int dpn_clock_rate_khz(int* khz);

/* fp32 tables: freq32 = 2**linspace(0,4,32), freq16 = 2**linspace(0,4,16) formed in fp32 exactly as
 * utils/position_encoding.py:27 does.  Copied to the device by the caller (8 + 4 = 48 floats: [32 | 16]). */

/* Weight preparation: fp32 tensors -> MFMA-fragment-ordered bf16 (hi/lo) + permuted fp32 vectors + u = W2^T wo.
 * Two forms of the packed block (csrc/dpn_layout.h): form 0 = the matrices of variable_net.py:49-87 as they stand (w1, w2, Wd, W1 and their
 * transposes: seven GEMMs per point and net); form 1 = FUSED: A = cat_fc1.fc.0.weight . w2 and B = cat_fc1.fc.0.weight . data_input_fc.weight
 * are formed once per net in exact fp32 (variable_net.py:81-84 applies fc.0 to c = w2 h1 + Wd pe6 + ..., so pre2 = A h1 + B pe6 + const, and the
 * reverse sweep needs only A^T): five GEMMs per point and net, c and d out / d c never formed.  dpn_fwd_form says which form the forward launch of
 * a precision mode reads (1: hi+lo mode with raw coordinates; 0: plain bf16, or caller-encoded coordinates); dpn_pack_weights packs that form
 * for raw coordinates.  The backward entry points read w1 and the vectors, which sit at the same offsets in both forms. */
int dpn_fwd_form(int prec, int has_pe_in);
int dpn_pack_weights_form(const DpnNetPtrs nets[DPN_NETS], int prec, int form, void* packed, void* stream);
int dpn_pack_weights(const DpnNetPtrs nets[DPN_NETS], int prec, void* packed, void* stream);
/* The same for n_fields field samples in ONE launch (BASELINE configs[2]: a batch of forecast leads, each with its own hyper-network output): nets = the
 * pointer table of field 0; field f reads w1b1 / w2b2 moved by f * heads_stride floats and evec by f * evec_stride floats (the static tensors are
 * shared) and writes its packed block at packed + f * packed_stride bytes (>= DpnSizes.packed, a multiple of 16).  n_fields = 1 ignores the strides. */
int dpn_pack_weights_batch(const DpnNetPtrs nets[DPN_NETS], int n_fields, int64_t heads_stride, int64_t evec_stride, int prec, int form, void* packed,
                           int64_t packed_stride, void* stream);

/* Forward + coordinate Jacobian (replaces PhysicsNet.forward's six VariableNet calls, physics_net.py:49-54,
 * and the 18 unique autograd.grad derivatives of interface_physics.py:90-95).
 *   x,y,t [N] raw coordinates (metres, metres, seconds), OR pe_in [N][192]: coordinates already encoded by the
 *   caller in the reference's SineCosPE channel order (then x,y,t and jac_n must be NULL);
 *   coord_data [N][6]; freqs [48]; out_n [N][6] normalised fields;
 *   jac_n [N][6][3] = d out_n / d(x,y,t)  (may be NULL: value-only); with pe_in it is [N][6][192] = d out_n / d pe_in instead
 *         (the caller chains it through its own coordinate encoding; dpn_contract_gpe contracts it with a cotangent of out_n);
 *   saved: state for the backward pass (may be NULL: inference only). */
int dpn_fwd(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n_points,
            const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
            float* out_n, float* jac_n, void* saved, void* stream);
/* dpn_fwd with the reference's separate ref_data argument (model/variable_net.py:49, :86: `out_fc(y) + ref_data`): ref_data [N][6] is added to
 * out_n in place of coord_data (NULL: coord_data, i.e. dpn_fwd -- PhysicsNet.forward passes coord_data[:, k] as net k's ref_data,
 * physics_net.py:49-54).  VariableNet.forward standalone uses it, so that its output is not rebuilt by subtraction. */
int dpn_fwd_ref(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data,
                int64_t n_points, const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
                float* out_n, float* jac_n, void* saved, void* stream);

/* dpn_fwd_ref for the first n_nets VariableNets only (1..6), inference only (nothing is saved for a backward pass): VariableNet.forward
 * standalone (model/variable_net.py:49-87) evaluates ONE net, not six.  Columns >= n_nets of out_n / jac_n are left untouched. */
int dpn_fwd_ref_nets(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data,
                     int64_t n_points, const float* freqs, const DpnGeometry* geo, const void* packed, int prec, int n_nets,
                     float* out_n, float* jac_n, void* stream);

/* dpn_fwd_ref with coordinate derivatives of order 2 and 3 from the same launch (raw coordinates only: pe_in must be NULL):
 *   hess_n [N][6][3] = d2 out_n / dx2, dy2, dt2;  d3_n [N][6][3] = d3 out_n / dx3, dy3, dt3  (either may be NULL; a non-NULL one needs jac_n),
 *   in physical units like jac_n.  Each PE channel depends on one coordinate and the nets are piecewise linear in the features (ReLU), so
 *   these are all the non-zero higher derivatives: every mixed partial is zero (almost everywhere).  hess_n = d3_n = NULL: dpn_fwd_ref. */
int dpn_fwd_ref_derivs(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data,
                       int64_t n_points, const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
                       float* out_n, float* jac_n, float* hess_n, float* d3_n, void* saved, void* stream);

/* g_pe[N][192] = sum_k g_out[N][k] * gpe[N][k][192]: backward of PhysicsNet.forward w.r.t. its encoded-coordinate input. */
int dpn_contract_gpe(const float* g_out, const float* gpe, int64_t n_points, float* g_pe, void* stream);

/* inverse_norm + six residual losses (interface_physics.py:97-185,232-262).
 *   loss_sums [ceil(N/256)][6] fp64: per-block sums over points of residual^2 (written, not accumulated: no zeroing, no atomics;
 *             dpn_residual_finish adds the rows in a fixed order -> deterministic losses);
 *   losses    [7] fp32: [0..5] = factor_i * sum_i / N, [6] = their sum in the reference's order (:301); dpn_residual_finish;
 *   when g_out != NULL also writes d(sum_i w_i * loss_i)/d out_n  [N][6] and d(...)/d J_xi [N][6][3] (cotangent of the
 *   Jacobian w.r.t. the NORMALISED coordinates xi), with w_i = gl[i] + gtot[0] (either may be NULL; both NULL: w_i = 1). */
int dpn_residual(const float* out_n, const float* jac_n, const float* f, int64_t n_points, const DpnGeometry* geo,
                 const DpnPhysics* phys, const float* gl /*[6] or NULL*/, const float* gtot /*[1] or NULL*/, double* loss_sums,
                 float* g_out, float* g_jxi, void* stream);
int dpn_residual_finish(const double* loss_sums, int64_t n_points, const DpnPhysics* phys, float* losses, void* stream);
/* n_fields fields of n_points each in one launch: loss_sums [n_fields][ceil(n_points / 256)][6], losses [n_fields][7]. */
int dpn_residual_finish_batch(const double* loss_sums, int64_t n_points, int n_fields, const DpnPhysics* phys, float* losses, void* stream);

/* Backward, stage 1: per-point cotangent streams -> the operands of the weight-gradient reductions.
 *   g_out [N][6]; g_jxi [N][6][3] or NULL (value-only loss, e.g. the data loss). */
int dpn_bwd_points(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n_points,
                   const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
                   const float* g_out, const float* g_jxi, const void* saved, void* operands, void* stream);
/* The same with a device scalar multiplied into both cotangent streams as they are read: the caller has g_out / g_jxi for a UNIT cotangent of the total
 * loss (dpn_residual evaluated once, losses and cotangents in one pass) and the upstream cotangent arrives later, as a tensor (loss.backward(seed)). */
int dpn_bwd_points_scaled(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n_points,
                          const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
                          const float* g_out, const float* g_jxi, const float* g_scale /* [1] device, or NULL = 1 */, const void* saved, void* operands,
                          void* stream);
/* The same with g_hxi [N][6][3] (or NULL), the cotangent of the second derivatives along the NORMALISED coordinates xi (g_jxi's space): the
 * weight gradients of the Jacobian and of the second derivatives in one pass (raw coordinates only: pe_in must be NULL).  Third derivatives
 * (dpn_fwd_ref_derivs' d3_n) take no cotangent here.  g_hxi = NULL: dpn_bwd_points_scaled. */
int dpn_bwd_points_derivs(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n_points,
                          const float* freqs, const DpnGeometry* geo, const void* packed, int prec,
                          const float* g_out, const float* g_jxi, const float* g_hxi, const float* g_scale, const void* saved, void* operands,
                          void* stream);

/* Backward, stage 2: weight-gradient reductions over points (split-K partial sums). */
int dpn_wgrad(int64_t n_points, int prec, const float* g_out, const void* saved, const void* operands, void* partials, void* stream);

/* Backward, stage 3: reduce the partial sums, undo the fragment permutations and assemble every gradient of DpnNetPtrs from the three
 * points-reduction products S1 = M2^T Z1, S2 = M2^T G6, dw1 = T1^T Z0 and their vector sums (interface_physics.py:506, the backward of
 * variable_net.py:49-87):  d w2b2 / d Wd = W1^T diag(u) S + 2 wo (x) colsum (csrc SavedView);  d cat_fc1.fc.0.weight = diag(u) G with
 * G = M2^T Z = S1 w2^T + S2 Wd^T + (M2^T g) (x) (b2 + bd + e) -- Z itself is never formed per point (csrc dpn_finish_gside_kernel);
 * the rank-1 cat_fc1.fc.2 / out_fc gradients follow from r = rowdot(W1, G) + bf1 (.) M2^T g. */
int dpn_wgrad_finish(const DpnNetPtrs nets[DPN_NETS], const void* packed, int64_t n_points, int prec,
                     const void* partials, const DpnNetGradPtrs grads[DPN_NETS], void* stream);
/* The same in two halves.  parts bit 0: what the hyper-network's backward waits for (d w1b1, d w2b2, d evec; d Wd and d bd ride along);
 * parts bit 1: the gradients of cat_fc1.fc.0 / fc.2 and out_fc (static tensors only).  Half 1 reads what half 0 left in the scratch tail of
 * `partials`: issue it on the same stream, or on another one ordered behind half 0 (a branch beside the encoder's backward chain). */
int dpn_wgrad_finish_parts(const DpnNetPtrs nets[DPN_NETS], const void* packed, int64_t n_points, int prec,
                           const void* partials, const DpnNetGradPtrs grads[DPN_NETS], int parts, void* stream);

/* SmoothL1(beta) data loss on the normalised fields (losses/weights_loss.py:17-20): per-block sums -> loss_sum[ceil(6N/256)] (fp64,
 * written not accumulated; the caller adds them in a fixed order), g_out = scale * dSmoothL1 (may be NULL). */
int dpn_smooth_l1(const float* out_n, const float* labels, int64_t n_points, float beta, float scale,
                  double* loss_sum, float* g_out, int accumulate /* g_out += instead of = */,
                  const float* scale_dev /* optional device scalar multiplied into scale (an upstream cotangent) */, void* stream);

/* Small fp32 GEMM for the per-field tensors (encoder linears of model/attn.py:177-196 and transformer_net.py:28-44, the
 * hyper-network heads of variable_net.py:59-65):  C[M][N] = op(A)[M][K] op(B)[K][N] (+ bias[N]) (+ C if accumulate);
 * ta/tb = 1 reads A as [K][M] / B as [N][K] (row-major, leading dimensions lda/ldb/ldc);
 * asum (may be NULL) receives sum_k op(A)[m][k] -- the bias gradient when op(A) = grad_out^T.
 * workspace (may be NULL): scratch for the deterministic two-pass split-K used when K is long and the output small. */
int dpn_sgemm(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
              const float* bias, float* asum, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* Up to 26 independent small fp32 GEMMs in one launch (exact-fp32 MFMA, fixed reduction order); each
 * C[M][N] = epilogue(sum_{t<nterms} op(A_t)[M][K_t] op(B_t)[K_t][N] + bias[N]); asum as in dpn_sgemm (single-term problems only).
 * Used for the q/k/v projections (attn.py:183-185), the paired input-/weight-gradient GEMMs of every encoder linear, and the
 * twelve hyper-network heads + six lead-time embeddings of the VariableNets (variable_net.py:59-65,75-78) and their backward. */
#define DPN_EPI_NONE 0
#define DPN_EPI_GELU 1            /* C = gelu(v) (exact erf, transformer_net.py:26,41); aux_out (optional) receives v                    */
#define DPN_EPI_MUL_GELU_GRAD 2   /* C = v * gelu'(aux): backward of the activation folded into the GEMM that feeds it                 */
#define DPN_EPI_ADD 3             /* C = v + aux: the residual-branch gradient joins the input gradient without a separate add kernel  */
#define DPN_GEMM_MAX_TERMS 12      /* per problem */
#define DPN_GEMM_MAX_PROBLEMS 26   /* per launch; at most 32 terms per launch in total */
#define DPN_GEMM_MAX_JOBS 10       /* ride-along column-sum jobs per launch */
typedef struct DpnGemmProblem {
    const float* A[DPN_GEMM_MAX_TERMS]; const float* B[DPN_GEMM_MAX_TERMS]; int32_t lda[DPN_GEMM_MAX_TERMS], ldb[DPN_GEMM_MAX_TERMS];
    int32_t k_term[DPN_GEMM_MAX_TERMS];   /* reduction length of term t; 0 = K */
    const float* bias; float* C; float* asum;
    int32_t M, N, K, ldc, ta, tb, nterms;
    const float* aux; float* aux_out;   /* [M][ldc], see DPN_EPI_* */
    int32_t epi;
} DpnGemmProblem;
int dpn_sgemm_batch(int n_problems, const DpnGemmProblem* problems /* host array */, void* stream);
/* The same launch with up to DPN_GEMM_MAX_JOBS ride-along column-sum jobs: out_a[c] = sum_b partial[b][c], out_b[c] = sum_b partial[b][256 + c],
 * c < 256, b < n_blocks (fixed order) -- the LayerNorm parameter gradients from dpn_add_ln_bwd's scratch (n_blocks = ceil(rows/4)),
 * finished inside a GEMM launch that follows it instead of in a launch of their own. */
typedef struct DpnColsumJob { const float* partial; float* out_a; float* out_b; int32_t n_blocks; } DpnColsumJob;
int dpn_sgemm_batch_jobs(int n_problems, const DpnGemmProblem* problems, int n_jobs, const DpnColsumJob* jobs /* host array */, void* stream);

/* LayerNorm folded into the A operand of the GEMM that consumes it (d_model = 256: the GEMM's K is the LayerNorm's row):
 *   mode 1:  C = epilogue((LN(x + r) * gamma + beta) . op(B) + bias); also writes y = LN(..)*gamma+beta [M][256], xhat [M][256], rstd [M]
 *            (EncoderLayer: x1 = norm1(x + attn) feeding conv1, transformer_net.py:37-41);
 *   mode 2:  C = epilogue(gs . op(B) + bias) with gs = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat)) the LayerNorm input
 *            gradient (x = g, r = xhat); also writes gs [M][256] (y_out) and partial[ceil(M/32)][2][256] = per-row-block sums of g*xhat
 *            and g, to be reduced by a DpnColsumJob (n_blocks = ceil(M/32)) of a later dpn_sgemm_batch_jobs launch.
 * op(B) = B^T with B stored [N][256] (tb = 1) or B stored [256][N] (tb = 0).  One launch instead of LayerNorm + GEMM. */
typedef struct DpnLnGemm {
    int32_t mode, M, N, tb, ldb, ldc, epi;
    const float *x, *r, *gamma, *beta, *rstd_in;
    float *y_out, *xhat_out, *rstd_out, *partial;
    const float *B, *bias;
    float* C;
    const float* aux;
    float* aux_out;
} DpnLnGemm;
int dpn_sgemm_ln(const DpnLnGemm* problem, void* stream);

/* FullAttention of the encoder (model/attn.py:50-68): o = softmax(q k^T / sqrt(32)) v for 8 heads x 32 over L <= 288 tokens.
 * q,k,v,o,go,dq,dk,dv: [batch*L][256] fp32 row-major (field b = rows b*L.., head h = columns 32h..32h+31); attention never crosses
 * fields.  P (saved probabilities): [batch][8][288][288] fp32.
 * The backward is one launch: query-tile blocks produce dq, key-tile blocks produce dk and dv (recomputing their columns of dS). */
int dpn_attn_fwd(const float* q, const float* k, const float* v, int L, int batch, float* out, float* P, void* stream);
int dpn_attn_bwd(const float* q, const float* k, const float* v, const float* o, const float* P, const float* go, int L, int batch,
                 float* dq, float* dk, float* dv, void* stream);
/* dpn_attn_fwd on the f16 hi+lo matrix cores with 16-row query tiles (same arguments, same P): q, k, v never pass through LDS -- a lane's
 * eight consecutive head channels of one token row are an MFMA fragment slot.  The encoder's fused forward uses this one. */
int dpn_attn16_fwd(const float* q, const float* k, const float* v, int L, int batch, float* out, float* P, void* stream);

/* ---------------------------------------------------------------- row-local fused encoder nodes (csrc/dpn_encoder_chain.hip)
 * Everything of an EncoderLayer except the attention itself is row-wise (attn.py:183-185,196; transformer_net.py:33-44, :68, :129), so the
 * whole stretch between two attention kernels is ONE launch (a workgroup carries 16 or 32 token rows through up to six 256 x 256 GEMMs).
 * All matrices are [256][256] fp32 as the reference stores them ([out][in]; Conv1d k=1 weights with the last axis squeezed), all row
 * tensors [rows][256] fp32, rows = batch * L.  The GEMMs run on f16 hi+lo split operands (three products, fp32 accumulate: fp32-class).
 *
 * dpn_enc_pack: MFMA-fragment images of n_mats matrices (dpn_enc_pack_bytes(n_mats) bytes: per matrix one image for x W^T and one for
 * g W).  Once per step, after the optimiser changed the weights.  *status_dev (may be NULL) gets bit 0 set when an |entry| >= 32768. */
#define DPN_ENC_MAX_MATS 32
int64_t dpn_enc_pack_bytes(int n_mats);
int dpn_enc_pack(int n_mats, const float* const* weights /* host array of device pointers */, void* packed, int* status_dev, void* stream);

/* dpn_enc_prep: everything of the encoder forward that depends on the step's inputs only, in ONE launch -- the weight images (dpn_enc_pack),
 * the im2col rows of the circular token convolution (dpn_im2col_circ3: x [batch*T][C] -> xu [batch*T][3C]) and the lead-time SineCosPE for one
 * or two frequency tables (dpn_lead_pe: h [batch] -> out_a [batch][2 n_a], out_b [batch][2 n_b]).  Each part is optional (n_mats = 0 / x = NULL
 * / h = NULL). */
typedef struct DpnEncPrep {
    int32_t n_mats; const float* const* weights /* host array of device pointers */; void* packed; int* status_dev;
    const float* x; int32_t T, C, batch; float* xu;
    const float* h; const float* freqs_a; int32_t n_a; float* out_a; const float* freqs_b; int32_t n_b; float* out_b;
} DpnEncPrep;
int dpn_enc_prep(const DpnEncPrep* p, void* stream);

/* Forward.  tail = 1:  x1 = norm1(x + o Wo^T + bo);  pre = x1 Wc1^T + bc1;  act = gelu(pre);  x2 = norm2(x1 + act Wc2^T + bc2)
 *                      (o = the attention output, x = the layer input; x1, xhat1, rstd1, pre, act, x2, xhat2, rstd2 are written);
 *           next = 1:  y0, y1, y2 = t Wn0^T + bn0, ...   the NEXT layer's q / k / v projections of t = x2 (tail = 1) or t = xin (tail = 0);
 *           next = 2:  xf = encoder.norm(x2) (xf, xhatf, rstdf written);  y0 = xf Wn0^T + bn0   (the output projection);
 *           next = 0:  nothing behind norm2.
 * m_*: indices of the matrices in `wpack`.  row_tiles: 1 or 2 sixteen-row tiles per workgroup (2 for batches of fields). */
typedef struct DpnEncFwd {
    const void* wpack; int32_t n_mats, rows, row_tiles, tail, next;
    int32_t m_o, m_c1, m_c2, m_n0, m_n1, m_n2;
    const float *o, *x, *xin;
    const float *bo, *g1, *be1, *bc1, *bc2, *g2, *be2, *gf, *bef, *bn0, *bn1, *bn2;
    float *x1, *xhat1, *rstd1, *pre, *act, *x2, *xhat2, *rstd2, *xf, *xhatf, *rstdf, *y0, *y1, *y2;
    /* tail = 0, one field (round 6): emb_parts != NULL makes this launch ASSEMBLE its input instead of reading xin -- what dpn_embed_assemble does in a
     * launch of its own (embed.py:60-64, transformer_net.py:124-126), same order of additions:
     *   row <  emb_n_tok:  x0[row] = (emb_token[row] + emb_pos[row]) + emb_te
     *   row >= emb_n_tok:  x0[row] = ((sum_p emb_parts[p][row - emb_n_tok], p = 0 .. emb_n_parts - 1, in order) + emb_bias + emb_pos[row]) + emb_te
     * emb_parts [emb_n_parts][emb_part_stride floats] (the token convolution's split-K slices, rows of 256), emb_te [256]; x0 is also written to emb_out [rows][256].
     * One field only (emb_pos and emb_te carry no batch offset).  -1: emb_n_tok > rows, or emb_n_parts > 1 with emb_part_stride < (rows - emb_n_tok) * 256
     * (slices that overlap: a stride of 0 would add slice 0 emb_n_parts times). */
    const float *emb_parts, *emb_bias, *emb_pos, *emb_te, *emb_token;
    float* emb_out;
    int64_t emb_part_stride;
    int32_t emb_n_parts, emb_n_tok;
} DpnEncFwd;
int dpn_enc_fwd(const DpnEncFwd* p, void* stream);

/* Backward of the same stretch, in the order the cotangent travels.
 *   head = 1:  g = res + dq Wh0 + dk Wh1 + dv Wh2      (the q / k / v projections of the layer ABOVE: its attention backward's outputs and
 *                                                      its residual-branch cotangent gs1)
 *   head = 2:  g = encoder.norm backward of (dmeta Wh0) (output projection; partial_f receives the norm's parameter partial sums)
 *   head = 0:  g = gin
 *   body = 1:  gs2 = norm2 backward of g;  dpre = (gs2 Wc2) * gelu'(pre);  gs1 = norm1 backward of (dpre Wc1 + gs2);  dout = gs1 Wo
 *              (gs2, dpre, gs1: the operands of the weight-gradient GEMMs dWc2 = gs2^T act, dWc1 = dpre^T x1, dWo = gs1^T o; dout: the
 *              attention backward's input; gs1 is also the residual-branch cotangent the next launch takes as `res`)
 *   body = 0:  gx = g   (the cotangent of the first layer's input); its first gx_head_rows rows are written to gx_head as well when that is
 *              given (the learnable tokens in front of the field tokens, model/transformer_net.py:123-126: their gradient lands in its own
 *              tensor without a copy)
 * partial_f / partial2 / partial1: [workgroups][512] = per-workgroup sums of (g * xhat | g) of the three LayerNorms, reduced in a fixed order by a
 * DpnColsumJob with n_blocks = ceil(rows / (16 row_tiles)). */
typedef struct DpnEncBwd {
    const void* wpack; int32_t n_mats, rows, row_tiles, head, body;
    int32_t m_h0, m_h1, m_h2, m_c2, m_c1, m_o;
    const float *res, *dq, *dk, *dv, *dmeta, *xhatf, *rstdf, *gin;
    const float *xhat2, *rstd2, *pre, *xhat1, *rstd1, *g2, *g1, *gf;
    float *gs2, *dpre, *gs1, *dout, *gx, *partial_f, *partial2, *partial1;
    float* gx_head; int32_t gx_head_rows;
} DpnEncBwd;
int dpn_enc_bwd(const DpnEncBwd* p, void* stream);

/* Weight gradients of linears over token rows, up to DPN_WGRAD_MAX_PROBLEMS in one launch:  dW[M][N] = G^T X,  db[M] = column sums of G
 * (db may be NULL), G [rows][M] (row stride ldg) the cotangent of the linear's output, X [rows][N] (ldx) its input, dW row stride ldw.
 * f16 hi+lo split operands with a running power-of-two scale per operand strip (any magnitude), fp32 accumulate, fixed order.
 * slices > 1 cuts the row reduction into that many slices (batches of fields): `partials` then needs dpn_wgrad16_partial_floats() floats and
 * a second launch adds the slices in order.  Up to DPN_GEMM_MAX_JOBS DpnColsumJob ride along (the LayerNorm parameter sums of dpn_enc_bwd).
 * Replaces dpn_sgemm_batch for the weight gradients of the encoder stack (attn.py:183-196, transformer_net.py:38-42,129, embed.py:45-47). */
#define DPN_WGRAD_MAX_PROBLEMS 32
typedef struct DpnWgradProblem { const float* G; const float* X; float* dW; float* db; int32_t M, N, rows, ldg, ldx, ldw; } DpnWgradProblem;
int64_t dpn_wgrad16_partial_floats(int n, const DpnWgradProblem* problems, int slices);
int dpn_wgrad16(int n, const DpnWgradProblem* problems /* host array */, int n_jobs, const DpnColsumJob* jobs, int slices, float* partials,
                void* stream);

/* out = LayerNorm_256(x + r) * gamma + beta (eps 1e-5), r may be NULL (transformer_net.py:37,44,68); saves xhat [rows][256] and rstd [rows].
 * Backward: gx = d/d(x + r) (the same tensor is the gradient of x and of r), dgamma, dbeta [256].  With dgamma = dbeta = NULL only gx and the
 * per-block partial sums in `scratch` ([ceil(rows/4)][512]) are produced, to be reduced by a DpnColsumJob of dpn_sgemm_batch_jobs. */
int dpn_add_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, int rows, float* out, float* xhat, float* rstd,
                   void* stream);
int dpn_add_ln_bwd(const float* g, const float* xhat, const float* rstd, const float* gamma, int rows, float* gx, float* dgamma, float* dbeta,
                   float* scratch /* ceil(rows/4) * 512 floats */, void* stream);

/* Data embedding of the encoder (model/embed.py:36-64, transformer_net.py:124-126), d_model = 256:
 *   dpn_lead_pe        SineCosPE of the scalar lead time for one or two frequency tables: out[2f] = sin(h f), out[2f+1] = cos(h f)
 *                      (encoder time embedding, N_freqs = 128, embed.py:58; VariableNet lead-time PE, N_freqs = 96, variable_net.py:46);
 *   dpn_im2col_circ3   out[T][3C], out[t][3c + tap] = x[(t + tap - 1) mod T][c]: the circular k=3 TokenEmbedding conv becomes
 *                      out . W^T with the Conv1d weight [256][C][3] read in place;
 *   dpn_embed_assemble out[n_tok + n_emb][256] = cat(learnable_token, value_embedding) + positional table + lead-time embedding, where the
 *                      value embedding is given as n_parts split-K partial products [n_parts][n_emb][256] (+ bias[256], may be NULL). */
/* out[0 .. count) = sum_p parts[p][0 .. count) (fixed order), out[count .. count + zero_tail) = 0: joins split-K partial products. */
int dpn_sum_parts(const float* parts, int n_parts, int64_t count, int64_t zero_tail, float* out, void* stream);
int dpn_lead_pe(const float* h_dev /* [batch] */, int batch, const float* freqs_a, int n_a, float* out_a /* [batch][2 n_a] */,
                const float* freqs_b, int n_b, float* out_b, void* stream);
int dpn_im2col_circ3(const float* x /* [batch*T][C] */, int T, int C, int batch, float* out /* [batch*T][3C] */, void* stream);
int dpn_embed_assemble(const float* token, int n_tok, const float* emb_parts /* [n_parts][batch*n_emb][256] */, int n_parts, int n_emb, int batch,
                       const float* bias, const float* pos, const float* te /* [batch][256] */, float* out /* [batch*(n_tok+n_emb)][256] */,
                       void* stream);

/* clip_grad_norm_(max_norm) + torch.optim.Adam step (interface_physics.py:514-515; cfg:151-155: L2-in-gradient weight decay)
 * over a list of fp32 tensors.  The pointer arrays and `numel` are HOST arrays of length n_tensors (device pointers inside);
 * scratch_dev: dpn_clip_adam_scratch_doubles(n_tensors, numel) doubles on the device ([0] receives the sum of squares of all
 * gradients, the rest are per-block partials added in a fixed order: the norm is deterministic and there are no atomics);
 * step_dev (int, the Adam step counter, incremented on the device) and out_norm_dev (float, may be NULL) are device scalars.
 * Seven launches for the 155 tensors of a PhysicsNet. */
int64_t dpn_clip_adam_scratch_doubles(int n_tensors, const int64_t* numel);
int dpn_clip_adam(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const int64_t* numel, double* scratch_dev, int* step_dev, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float max_norm, float* out_norm_dev, void* stream);

/* ---------------------------------------------------------------- collocation sampler + full-grid gather
 * Geometry of the fine (label) grid and the coarse forecast cube (dataset/physics_dataset.py:104-126): the fine grid has
 * lon x lat nodes, dlat degrees apart, starting at begin_lat; one fine cell is cells_x / cells_y coarse cells wide
 * (0.25 deg / 1 deg = 0.25 for the shipped data); the coarse cube has t_in time slices, t_step_hours apart
 * (input_time_step = 6, input_time_step_nums + 1 = 5), and collocation times are whole hours in [0, t_hours]. */
typedef struct DpnSampler {
    int32_t lon, lat;                 /* fine grid (label_lon_size, label_lat_size) = (257, 145)     */
    int32_t lon_in, lat_in, t_in;     /* coarse cube (65, 37, 5)                                       */
    int32_t t_hours;                  /* input_time_step * input_time_step_nums = 24                   */
    double cells_x, cells_y;          /* coarse cells per fine cell                                    */
    double t_step_hours;              /* 6                                                             */
    double begin_lat, dlat;           /* degrees                                                       */
    float dx, dy;                     /* metres per fine cell                                          */
} DpnSampler;
#define DPN_SAMPLE_INTERIOR 0   /* get_inter_data       (physics_dataset.py:431-499): x, y continuous uniform, t integer hours */
#define DPN_SAMPLE_MARGIN   1   /* get_item_label_data  (:323-429): x, y integer grid nodes, + label gather                    */
#define DPN_SAMPLE_EXPLICIT 2   /* get_margin_grid      (:528-587): node indices xi, yi and hour ti given by the caller         */
/* Draws n collocation points (Philox-4x32-10, counter = offset + point index, key = seed), interpolates the coarse cube
 * cube[6][lat_in][lon_in][t_in] (fp32, variable order u10,v10,pres,t2,q2,rio) tri-linearly at them (fp64 weights, result
 * cast to fp32: what xarray's .interp + .float() produce) and writes x, y (metres), t (seconds), f (Coriolis),
 * coord_data[n][6].  labels[t_hours+1][6][lat][lon] / label_out[n][6] (node modes only) and raw[n][3] (the draws as
 * doubles: x index, y index, hour) are optional (NULL).
 * Inside rule: the position in coarse index units is fx = x index * cells_x (fy, ft alike), its cell is floor(fx) clamped to the cube and
 * its weight is fx - cell.  A weight within 1e-9 of [0, 1] counts as inside and is clamped to [0, 1] before use; anything further out makes
 * coord_data NaN.  The tolerance absorbs the rounding of fx on the cube's last face when cells_x is no binary fraction (0.1 / 0.3 deg): at
 * most about 2 ulp(fx) < 5e-10 for an axis of up to 2^20 cells; weights already in [0, 1] are used unchanged. */
int dpn_sample_points(const DpnSampler* s, const float* cube, const float* labels, int mode, const int32_t* xi, const int32_t* yi,
                      const int32_t* ti, int64_t n, uint64_t seed, uint64_t offset, float* x, float* y, float* t, float* f,
                      float* coord_data, float* label_out, double* raw, void* stream);
/* The same draw with the Philox counter advanced on the DEVICE: counter = offset + *step_dev * stride + point index.  step_dev is the
 * optimiser's device-side step counter (dpn_clip_adam_flat's step_dev, bumped once per step), stride the points drawn per step, so a
 * sampler launch captured in a hipGraph draws fresh points on every replay (a captured host-side offset would freeze them).
 * step_dev == NULL is dpn_sample_points.  Replaces the per-__getitem__ np.random draws of physics_dataset.py:334-338,442-446 inside a
 * captured training step. */
int dpn_sample_points_replay(const DpnSampler* s, const float* cube, const float* labels, int mode, const int32_t* xi, const int32_t* yi,
                             const int32_t* ti, int64_t n, uint64_t seed, uint64_t offset, const int32_t* step_dev, uint64_t stride,
                             float* x, float* y, float* t, float* f, float* coord_data, float* label_out, double* raw, void* stream);
/* Normalised fields of all lon*lat nodes in the reference's node order (x outer, y inner; interface_physics.py:538-543),
 * out_n[lon*lat][6] -> de-normalised maps[6][lat][lon] (inverse_norm :232-262 + the scatter loop :583-591). */
int dpn_grid_maps(const float* out_n, int lon, int lat, const DpnPhysics* phys, int with_clip, float* maps, void* stream);

/* ---------------------------------------------------------------- inference: given positions, lattices, output planes
 * A regular lattice of nx * ny * nt positions in the sampler's units (fine-grid index units, hours).  Point g = (it * ny + iy) * nx + ix (ix fastest,
 * it slowest) lies at (x0 + ix * xstep, y0 + iy * ystep, t0 + it * tstep), each formed in fp64 with two roundings.  Kernels build the points of a
 * range first .. first + n themselves, so a host walks a long lattice in chunks without any index array. */
typedef struct DpnLattice {
    double x0, xstep, y0, ystep, t0, tstep;
    int32_t nx, ny, nt;
} DpnLattice;
/* The sampler evaluated at GIVEN positions instead of drawn ones: either stations xr, yr, tr [n] (fp64; lattice = NULL, first ignored) or points
 * first .. first + n of *lattice (xr = yr = tr = NULL).  Outputs and arithmetic are dpn_sample_points': x, y (metres), t (seconds), f,
 * coord_data[n][6] (NaN outside the coarse cube: dpn_sample_points' inside rule, a position within 1e-9 of a coarse cell beyond a face of the cube
 * is taken as on the face, anything further out is NaN).  -1: n <= 0, a NULL pointer, both or neither source, nx / ny / nt < 1, first + n > nx * ny * nt. */
int dpn_sample_at(const DpnSampler* s, const float* cube, const double* xr, const double* yr, const double* tr, const DpnLattice* lattice,
                  int64_t first, int64_t n, float* x, float* y, float* t, float* f, float* coord_data, void* stream);
/* Normalised fields out_n[n][6] -> physical values with dpn_grid_maps' arithmetic (multiply, then add; the squared form; the clip of P, T, q, rho that
 * lets NaN through).  Exactly one destination: rows[n][6] (stations; lattice = NULL), or maps[nt][6][ny][nx] where the n points are points
 * first .. first + n of *lattice (stores run along ix; a chunk may begin and end anywhere in a plane). */
int dpn_fields_out(const float* out_n, int64_t n, const DpnPhysics* phys, int with_clip, float* rows, float* maps, const DpnLattice* lattice,
                   int64_t first, void* stream);
/* Label-side evaluation of a validation pass (interface_physics.py:518-530, :629-745): predictions out_n[S][n][6] and labels[S][n][6] (normalised,
 * variable order u, v, P, T, q, rho) are read once; per segment s (one field sample) the DPN_EVAL_STATS sufficient statistics are
 *   [0]        sum SmoothL1_beta(out_n - label) over all 6 n elements (the data loss of weights_loss.py:17-20 is this / (6 n)),
 *   [1 + k]    sum d^2,   [7 + k] sum |d|,   [13 + k] sum d,   [19 + k] max |d|     with d = inverse_norm(pred)_k - inverse_norm(label)_k:
 * both sides de-normalised in fp32 with dpn_fields_out's arithmetic (multiply, then add; the squared min_max form), subtracted and squared in
 * fp32, added in fp64.  with_clip applies the clip bounds of P, T, q, rho to both sides (the reference evaluates these errors without it, :706-713).
 * dpn_label_errors writes one row per block, partials[S][dpn_label_errors_blocks(n)][DPN_EVAL_STATS] (written, not accumulated; a block never
 * straddles two segments); dpn_label_errors_finish adds the rows of every segment in a fixed order -> stats[S][DPN_EVAL_STATS].  No atomics: two
 * runs agree bitwise.  out_n / labels: 8-byte aligned (any row of a contiguous [.., 6] fp32 tensor).  -1: NULL, n <= 0, S <= 0, beta <= 0. */
#define DPN_EVAL_STATS 25
int64_t dpn_label_errors_blocks(int64_t n_points);
int dpn_label_errors(const float* out_n, const float* labels, int64_t n_points, int segments, const DpnPhysics* phys, float beta, int with_clip,
                     double* partials, void* stream);
int dpn_label_errors_finish(const double* partials, int64_t n_points, int segments, double* stats, void* stream);
/* The six signed residuals of every point, res[n][6] = lhs - rhs of (motion-u, motion-v, continuity, energy, vapour, gas), unscaled:
 * factor_i * mean(res_i ** 2) is dpn_residual's MSE loss term.  Inputs as dpn_residual (phys->clip_on etc. apply; the criterion is not read). */
int dpn_residual_points(const float* out_n, const float* jac_n, const float* f, int64_t n_points, const DpnGeometry* geo, const DpnPhysics* phys,
                        float* res, void* stream);
/* Derived diagnostics from the fields and their coordinate Jacobian (csrc/dpn_diag.hip): out_n, jac_n, f, phys as dpn_residual_points (geometry and
 * criterion are not read).  Per point the residual body forms val = inverse_norm(out_n) (u, v, p, T, q, rho = val[0..5]) and
 * J[k][c] = jac_n[k][c] * d val_k / d out_k, the derivative of the de-normalised variable k with respect to x (m), y (m), t (s) for c = 0, 1, 2.
 * with_clip == 0: the clip of *phys is switched off (in the entry point's own copy), nothing is clipped or masked -- inference, as dpn_fields_out
 * with with_clip == 0; with_clip != 0: the body as training runs it, a clipped variable has J[k][.] = 0 where it is clipped.
 * products = n_products (1..DPN_DIAG_PRODUCTS) HOST ids, the column selector; ids may repeat and come in any order.  Every operation below is one
 * fp32 operation rounded on its own (the kernel is compiled without contraction), evaluated left to right as written:
 *   3 k + c (0..17)  du_dx du_dy du_dt dv_dx .. drho_dt    J[k][c]
 *   18  vorticity           J[1][0] - J[0][1]
 *   19  abs_vorticity       (J[1][0] - J[0][1]) + f
 *   20  divergence          J[0][0] + J[1][1]
 *   21  omega               (J[2][2] + u * J[2][0]) + v * J[2][1]                          (Dp/Dt, Pa/s: the body's omega)
 *   22  t_advection         -(u * J[3][0] + v * J[3][1])
 *   23  q_advection         -(u * J[4][0] + v * J[4][1])
 *   24  q_flux_divergence   q * (J[0][0] + J[1][1]) + (u * J[4][0] + v * J[4][1])
 *   25  speed               sqrtf(u * u + v * v)
 *   26  rel_humidity        q / q_s;  tc = T - 273.15f, e_s = ((6.112f * expf((17.67f * tc) / (tc + 243.5f))) * 100.f),
 *                           q_s = max((0.622f * e_s) / (p - 0.378f * e_s), 1e-6f), a NaN passing through (the body's q_s: get_qs)
 *   27  deformation         sqrtf((J[0][0] - J[1][1]) * (J[0][0] - J[1][1]) + (J[1][0] + J[0][1]) * (J[1][0] + J[0][1]))
 * Exactly one destination: rows[n][n_products] (stations; lattice = NULL), or maps[nt][n_products][ny][nx] where the n points are points
 * first .. first + n of *lattice (stores run along ix; a chunk may begin and end anywhere in a plane).  No atomics.
 * NaN: a point with a NaN among its six out_n is NaN in EVERY product (a lattice point outside the coarse cube: the forward kernel's Jacobian is
 * finite there, its ReLU masks being off, and the clip sends a NaN value to its lower bound -- the rule, not the arithmetic, keeps such a point out of
 * the maps); any other NaN input propagates through the expressions.
 * -1 (nothing launched, nothing written): a NULL out_n, jac_n, f, phys or products; n <= 0; n_products outside 1..DPN_DIAG_PRODUCTS; an id outside
 * 0..DPN_DIAG_PRODUCTS - 1; both destinations or neither; maps without lattice, rows with one; nx / ny / nt < 1; first < 0; first + n > nx * ny * nt. */
#define DPN_DIAG_PRODUCTS 28
int dpn_diagnostics_out(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnPhysics* phys, int with_clip,
                        const int32_t* products /* HOST, n_products ids */, int n_products, float* rows, float* maps, const DpnLattice* lattice,
                        int64_t first, void* stream);
/* Ensemble statistics over field samples (csrc/dpn_ensemble.inc, compiled into csrc/dpn_diag.hip): the members of a lagged or perturbed ensemble are
 * folded one by one into a resident state, and one finish call turns the state into mean, spread, min, max, count and exceedance probabilities.
 * Product ids: 0..27 are dpn_diagnostics_out's; 28..33 are the de-normalised variables u, v, p, T, q, rho = val[0..5] of the residual body, the value
 * dpn_fields_out writes for the same out_n, *phys and with_clip.  The products are formed exactly as dpn_diagnostics_out forms them (same expressions,
 * same order, no contraction, the same NaN rule: a point with a NaN among its six out_n is NaN in every product).
 * State of a request of n_total points and P = n_products columns, E = n_thr thresholds, product-major (a wave's accesses run along the points):
 *   int32 count[P][n_total], double mean[P][n_total], double m2[P][n_total], float vmin[P][n_total], float vmax[P][n_total], int32 exceed[E][n_total].
 * The caller zeroes count, mean, m2 and exceed (a plain memset) before the first member; vmin and vmax need no filling: count == 0 means "not yet set".
 * dpn_ensemble_accumulate folds ONE member's values at points first .. first + n (out_n, jac_n, f: that chunk's rows, as dpn_diagnostics_out takes them)
 * into the state.  Per column j, with x the product products[j] at the point: if x is not finite, nothing of the column changes; otherwise, every
 * operation an fp64 operation rounded on its own, left to right:
 *   c = count + 1;  d = (double)x - mean;  mean = mean + d / (double)c;  m2 = m2 + d * ((double)x - mean);  count = c
 *   vmin = (c == 1) ? x : fminf(vmin, x);   vmax = (c == 1) ? x : fmaxf(vmax, x)      (as comparisons, x < vmin and x > vmax: between +0 and -0,
 *                                                                                      where fminf may return either, the earlier member's stays)
 *   for every threshold e with thr_col[e] == j:  exceed[e] += (x > thr_val[e])                       (strict)
 * products, thr_col (the column 0..n_products - 1 a threshold applies to) and thr_val are HOST arrays.  jac_n may be NULL when no selected id reads the
 * Jacobian (ids 0..24 and 27 do), f when id 19 is not selected: the kernel instantiated for such a request reads J = 0 (f = 0) from no memory.
 * One thread per point, 256-thread blocks, no atomics, no LDS, plain vector stores; members follow each other on one stream.
 * dpn_ensemble_finish writes, for points first .. first + n and every column j (c = count):
 *   mean = (float)mean, NaN when c == 0;   spread = (float)sqrt(m2 / (double)(c - 1)), NaN when c < 2;   min, max: NaN when c == 0;   count = c
 *   prob[e] = (float)((double)exceed[e] / (double)count[thr_col[e]]), NaN when that count is 0
 * into exactly one destination form: *rows, five arrays [n][P] (count int32) and prob [n][E] (stations; lattice = NULL), or *maps, [nt][P][ny][nx] and
 * [nt][E][ny][nx] where the n points are points first .. first + n of *lattice (placement as dpn_diagnostics_out: stores run along ix; a chunk may begin
 * and end anywhere in a plane).  prob may be NULL when n_thr == 0.
 * -1 (nothing launched, nothing written), both calls: a NULL required pointer (thr_col, thr_val, exceed, prob: required when n_thr > 0); n <= 0; first < 0;
 * first + n > n_total; n_products outside 1..DPN_ENS_PRODUCTS; n_thr outside 0..DPN_ENS_MAX_THRESHOLDS; a thr_col outside 0..n_products - 1.
 * accumulate: an id outside 0..DPN_ENS_PRODUCTS - 1; a threshold that is not finite; a selected id that reads J (f) while jac_n (f) is NULL.
 * finish: both destination forms or neither; maps without lattice, rows with one; nx / ny / nt < 1; first + n > nx * ny * nt. */
#define DPN_ENS_PRODUCTS 34
#define DPN_ENS_MAX_THRESHOLDS 16
typedef struct DpnEnsembleOut {
    float *mean, *spread, *min, *max;
    int32_t* count;
    float* prob;
} DpnEnsembleOut;
int dpn_ensemble_accumulate(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnPhysics* phys, int with_clip,
                            const int32_t* products /* HOST, n_products ids */, int n_products, const int32_t* thr_col /* HOST [n_thr] */,
                            const float* thr_val /* HOST [n_thr] */, int n_thr, int64_t first, int64_t n_total, int32_t* count, double* mean, double* m2,
                            float* vmin, float* vmax, int32_t* exceed, void* stream);
int dpn_ensemble_finish(const int32_t* count, const double* mean, const double* m2, const float* vmin, const float* vmax, const int32_t* exceed,
                        int64_t n_total, int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr, int64_t first, int64_t n,
                        const DpnEnsembleOut* rows, const DpnEnsembleOut* maps, const DpnLattice* lattice, void* stream);
/* Window extremes and means in time (csrc/dpn_extreme.inc, compiled into csrc/dpn_diag.hip): per point and column the maximum or minimum of a product
 * over the hours [t0, t0 + K * dt] and the hour it occurs at, or the window mean.  A coarse scan of the K + 1 nodes (one fields-only forward each), then
 * bisection on the sign of the network's own d/dt around the best node (one forward with the Jacobian per round, Cr probes per point).
 * A request is C = n_columns (1..DPN_EXT_MAX_COLUMNS; repeats allowed) columns (products[c], senses[c]), HOST arrays.  Products: 28..33, the
 * de-normalised u, v, p, T, q, rho, and 25, speed -- ids, expressions and NaN rule of dpn_ensemble_accumulate (the residual body's val, with_clip as
 * dpn_diagnostics_out takes it, speed = sqrtf(u * u + v * v); a point with a NaN among its six out_n is NaN).  Senses: DPN_EXT_MAX, _MIN, _MEAN.
 * The Cr refined columns are the max / min columns in request order.
 * Clock: node k (0..K) lies at hour t0 + (double)k * dt, two fp64 roundings.  xr, yr [n] fp64: the points, as dpn_sample_at takes stations.
 * State of a chunk of n points, column-major (a wave runs along the points; a map [C][ny][nx] is a view of it), every array [C][n]:
 *   float best_v, double best_t (hours), int32 best_k, double acc, int32 status (DPN_EXT_*), double lo, hi.   Nothing needs filling before node 0.
 * Every operation below is one operation rounded on its own (the kernels are compiled without contraction).
 * dpn_extreme_scan: out_n [n][6] = the fields-only forward at node k.  Per column, x the product at the point:
 *   k > 0 and status != 0:  nothing changes (sticky)
 *   x not finite:           status = DPN_EXT_BAD_SCAN, nothing else changes
 *   k == 0:                 status = 0, best_v = x, best_k = 0, acc = 0.5 * (double)x
 *   else:                   max: x > best_v, min: x < best_v -> best_v = x, best_k = k (a tie keeps the earlier node; a mean column keeps node 0's);
 *                           acc = acc + (k == K ? 0.5 : 1.0) * (double)x
 * and, unless k == K, x, y, t, f, coord_data [n] = the sampler at (xr, yr, hour of node k + 1), dpn_sample_at's arithmetic, for the next forward.
 * dpn_extreme_begin (after node K).  A mean column: best_v = (float)(acc / (double)K), NaN under a non-zero status; best_t = lo = hi = NaN.
 *   A max / min column with status 0: lo = hour of node max(best_k - 1, 0), hi = hour of node min(best_k + 1, K), best_t = m = hour of node best_k;
 *   under DPN_EXT_BAD_SCAN: best_v = best_t = lo = hi = NaN, m = t0.  Refined column r writes the probe inputs x, y, t, f, coord_data [r * n + i] =
 *   the sampler at (xr, yr, m): the five arrays hold Cr * n rows.
 * dpn_extreme_refine, round 0, 1, ..: out_n [Cr * n][6], jac_n [Cr * n][6][3] = the forward with the Jacobian at the probes.  A probe whose column
 *   has status != 0 is skipped: its inputs stay, its forwards are ignored.  Otherwise m = the probe's hour (round 0: the hour of node best_k; later:
 *   lo + 0.5 * (hi - lo) of the state, the expression the probe was written with), g = the product, s = its slope in time up to a positive factor:
 *   J[k][2] for a variable, u * J[0][2] + v * J[1][2] for speed (only the sign is used, nothing is divided), J the residual body's, clip included.
 *     g or s not finite:  status = DPN_EXT_STOPPED; the best so far stands
 *     g strictly better than best_v:  best_v = g, best_t = m
 *     max: s > 0 -> lo = m, else hi = m;    min: s < 0 -> lo = m, else hi = m
 *     lo == hi:  status = best_k == 0 ? DPN_EXT_AT_START : DPN_EXT_AT_END (the extreme sits on a face of the window, the slope pointing outward; the
 *                host keeps dt / 2^rounds above the spacing of the hours, so that a bracket closes nowhere else)
 *     otherwise: the probe's x, y, t, f, coord_data = the sampler at (xr, yr, lo + 0.5 * (hi - lo))
 *   Round 0 probes the best scan node itself and chooses the side; every later round halves the bracket.
 * Results: value best_v, hour best_t, lo, hi, status.  A (value, hour) pair always comes from one evaluation, and is never worse than the best node.
 * 256-thread blocks, one thread per (column, point) -- refine: per probe --, no atomics, no LDS, plain per-thread vector stores.
 * -1 (nothing launched, nothing written): a NULL pointer (the state's seven included); n <= 0; K < 1; k outside 0..K; round < 0; t0 or dt not finite;
 * dt <= 0; n_columns outside 1..DPN_EXT_MAX_COLUMNS; an id other than 25, 28..33; a sense outside 0..2; a sampler cube dimension < 2; refine without
 * a max / min column. */
#define DPN_EXT_MAX_COLUMNS 32
#define DPN_EXT_MAX  0
#define DPN_EXT_MIN  1
#define DPN_EXT_MEAN 2
#define DPN_EXT_OK        0
#define DPN_EXT_BAD_SCAN  1   /* a scan node's value was not finite: everything is NaN            */
#define DPN_EXT_STOPPED   2   /* a probe's value or slope was not finite: the best so far stands  */
#define DPN_EXT_AT_START  3   /* the extreme sits at hour t0, the slope pointing out of the window */
#define DPN_EXT_AT_END    4   /* ... at hour t0 + K * dt                                          */
typedef struct DpnExtremeState {
    float* best_v;
    double* best_t;
    int32_t* best_k;
    double* acc;
    int32_t* status;
    double *lo, *hi;
} DpnExtremeState;
int dpn_extreme_scan(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n,
                     const int32_t* products /* HOST */, const int32_t* senses /* HOST */, int n_columns, int k, int K, double t0, double dt,
                     const double* xr, const double* yr, const DpnExtremeState* st, float* x, float* y, float* t, float* f, float* coord_data,
                     void* stream);
int dpn_extreme_begin(const DpnSampler* s, const float* cube, int64_t n, const int32_t* products /* HOST */, const int32_t* senses /* HOST */,
                      int n_columns, int K, double t0, double dt, const double* xr, const double* yr, const DpnExtremeState* st, float* x, float* y,
                      float* t, float* f, float* coord_data, void* stream);
int dpn_extreme_refine(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, const float* jac_n, int64_t n,
                       const int32_t* products /* HOST */, const int32_t* senses /* HOST */, int n_columns, int round, int K, double t0, double dt,
                       const double* xr, const double* yr, const DpnExtremeState* st, float* x, float* y, float* t, float* f, float* coord_data,
                       void* stream);
/* Threshold spells in time (csrc/dpn_spell.inc, compiled into csrc/dpn_diag.hip): per point and column how long a product stays above (below) a
 * threshold over the hours [t0, t0 + K * dt], the hour of the first entry and of the last exit, the number of crossings and the time integral of the
 * margin.  The window extremes' scan of K + 1 nodes, then bisection on the sign of value - threshold inside the scan step of the first entry and the
 * scan step of the last exit: one fields-only forward per round, two probes per point and column.
 * A request is C = n_columns (1..DPN_SPELL_MAX_COLUMNS; repeats allowed) columns (products[c], sides[c], thr[c]), HOST arrays.  Products, their
 * expressions, NaN rule and with_clip: dpn_extreme_scan's (25 speed, 28..33 u, v, p, T, q, rho).  sides[c]: DPN_SPELL_ABOVE or _BELOW; thr[c] finite.
 * x is "in" when x > thr (above) or x < thr (below): strict, compared in float32, as the ensemble's thresholds are.  The margin of x is
 * d(x) = (double)x - (double)thr for above and -((double)x - (double)thr) for below: d(x) > 0 exactly where x is in.
 * Clock: node k (0..K) lies at hour(k) = t0 + (double)k * dt, the extremes' expression.  xr, yr [n] fp64: the points, as dpn_sample_at takes stations.
 * State of a chunk of n points, column-major (a wave runs along the points; a map [C][ny][nx] is a view of it), every array [C][n]:
 *   float prev_x; double hours, excess; int32 crossings, k_first, k_last, status (DPN_SPELL_* bits); double part_first, part_last, f_lo, f_hi, l_lo, l_hi.
 *   k_first / k_last: the first / last scan node that is in, -1: none.  Nothing needs filling before node 0.
 * Every operation below is one operation rounded on its own (the kernels are compiled without contraction), left to right.
 * dpn_spell_scan: out_n [n][6] = the fields-only forward at node k.  Per column, x the product at the point:
 *   k > 0 and status != 0:  nothing changes (sticky)
 *   x not finite:           status = DPN_SPELL_BAD_SCAN, nothing else changes
 *   k == 0:                 status = 0, hours = excess = part_first = part_last = 0, crossings = 0, k_first = k_last = (x in ? 0 : -1), prev_x = x
 *   else, a = d(prev_x), b = d(x), then prev_x = x:
 *     a > 0, b > 0 (both in):   hours = hours + dt;  excess = excess + 0.5 * (a + b) * dt;  k_last = k;  part_last = 0
 *     a <= 0, b <= 0:           nothing
 *     a <= 0 < b (entry):       w = b / (b - a) * dt;  hours = hours + w;  excess = excess + 0.5 * b * w;  crossings += 1;  k_last = k;  part_last = 0;
 *                               if k_first < 0: k_first = k, part_first = w
 *     b <= 0 < a (exit):        w = a / (a - b) * dt;  hours = hours + w;  excess = excess + 0.5 * a * w;  crossings += 1;  part_last = w  (k_last is k - 1)
 *   and, unless k == K, x, y, t, f, coord_data [n] = the sampler at (xr, yr, hour(k + 1)), dpn_sample_at's arithmetic, for the next forward.
 *   hours and excess are the time in and the integral of max(d, 0) of the piecewise-linear series through the nodes (the clipped trapezoid).
 * dpn_spell_begin (after node K), per column:
 *   DPN_SPELL_BAD_SCAN:  hours = excess = f_lo = f_hi = l_lo = l_hi = NaN
 *   k_first < 0:         status |= DPN_SPELL_NEVER;  f_lo = f_hi = l_lo = l_hi = NaN
 *   otherwise  k_first >= 1 (an entry bracket): f_lo = hour(k_first - 1), f_hi = hour(k_first);  k_first == 0: f_lo = f_hi = t0, status |= _HOLDS_AT_START
 *              k_last < K (an exit bracket):    l_lo = hour(k_last), l_hi = hour(k_last + 1);    k_last == K:  l_lo = l_hi = hour(K), status |= _HOLDS_AT_END
 *   Probe e (0 entry, 1 exit) of column c at point i is row (2 * c + e) * n + i of x, y, t, f, coord_data (2 * C * n rows) = the sampler at (xr, yr, m),
 *   m = lo + 0.5 * (hi - lo) of its bracket; a probe without a bracket is written at t0 (a valid input; its forwards are ignored).
 * dpn_spell_refine, round 0, 1, ..: out_n [2 * C * n][6] = the fields-only forward at the probes.  A probe is skipped when its column's status has
 *   _BAD_SCAN, _STOPPED or _NEVER, or when it has no bracket: its inputs stay.  g = the product at the probe, m = lo + 0.5 * (hi - lo) of the state, the
 *   expression the probe was written with.
 *     g of either probe of the column (that has a bracket) not finite:  status |= DPN_SPELL_STOPPED; both brackets stand
 *     entry probe:  g in -> f_hi = m, else f_lo = m;      exit probe:  g in -> l_lo = m, else l_hi = m
 *     then the probe's x, y, t, f, coord_data = the sampler at (xr, yr, lo + 0.5 * (hi - lo)) of the new bracket
 *   f_hi and l_lo are hours at which the network itself was evaluated and found in, f_lo and l_hi hours at which it was found out.
 * dpn_spell_finish (once, after the last round), per column: DPN_SPELL_BAD_SCAN: nothing;  DPN_SPELL_NEVER: hours = excess = 0;  otherwise
 *     with an entry bracket:  hours = hours - part_first;  hours = hours + (hour(k_first) - f_hi)
 *     with an exit bracket:   hours = hours - part_last;   hours = hours + (l_lo - hour(k_last))
 *   the scan's interpolated ends of the spell replaced by the refined ones.  excess stays the scan's clipped trapezoid, as the extremes' mean does.
 * Results: hours, first = f_hi, last = l_lo (first_lo = f_lo, last_hi = l_hi: the other ends of the brackets), excess, crossings, status.
 * 256-thread blocks, one thread per (column, point) -- refine: per probe --, no atomics, no LDS, plain per-thread vector stores.
 * -1 (nothing launched, nothing written): a NULL pointer (the state's thirteen included); n <= 0; K < 1; k outside 0..K; round < 0; t0 or dt not finite;
 * dt <= 0; n_columns outside 1..DPN_SPELL_MAX_COLUMNS; an id other than 25, 28..33; a side outside 0..1; a threshold that is not finite; a sampler
 * cube dimension < 2. */
#define DPN_SPELL_MAX_COLUMNS 16
#define DPN_SPELL_ABOVE 0
#define DPN_SPELL_BELOW 1
#define DPN_SPELL_BAD_SCAN        1   /* a scan node's value was not finite: everything is NaN                */
#define DPN_SPELL_STOPPED         2   /* a probe's value was not finite: the brackets stand as they were      */
#define DPN_SPELL_NEVER           4   /* no scan node is in: hours = excess = 0, first = last = NaN           */
#define DPN_SPELL_HOLDS_AT_START  8   /* node 0 is in: first = t0                                             */
#define DPN_SPELL_HOLDS_AT_END   16   /* node K is in: last = t0 + K * dt                                     */
typedef struct DpnSpellState {
    float* prev_x;
    double *hours, *excess;
    int32_t *crossings, *k_first, *k_last, *status;
    double *part_first, *part_last;
    double *f_lo, *f_hi, *l_lo, *l_hi;
} DpnSpellState;
int dpn_spell_scan(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n,
                   const int32_t* products /* HOST */, const int32_t* sides /* HOST */, const float* thr /* HOST */, int n_columns, int k, int K, double t0,
                   double dt, const double* xr, const double* yr, const DpnSpellState* st, float* x, float* y, float* t, float* f, float* coord_data,
                   void* stream);
int dpn_spell_begin(const DpnSampler* s, const float* cube, int64_t n, const int32_t* products /* HOST */, const int32_t* sides /* HOST */,
                    const float* thr /* HOST */, int n_columns, int K, double t0, double dt, const double* xr, const double* yr, const DpnSpellState* st,
                    float* x, float* y, float* t, float* f, float* coord_data, void* stream);
int dpn_spell_refine(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n,
                     const int32_t* products /* HOST */, const int32_t* sides /* HOST */, const float* thr /* HOST */, int n_columns, int round, int K,
                     double t0, double dt, const double* xr, const double* yr, const DpnSpellState* st, float* x, float* y, float* t, float* f,
                     float* coord_data, void* stream);
int dpn_spell_finish(int64_t n, int n_columns, int K, double t0, double dt, const DpnSpellState* st, void* stream);
/* Regional statistics in space (csrc/dpn_region.inc, compiled into csrc/dpn_diag.hip): per time node and region the weighted mean and total of a
 * product, its minimum and maximum and where they sit, the number of points counted, and the share of the counted weight above thresholds.  A
 * deterministic segmented reduction: no atomics, one fixed order of operations, so two runs and any chunking give the same bits.
 * The plan (DpnRegionPlan; deepphysinet_amd/regions.py builds it) is the region-sorted list of the n_sel selected positions of a plane (or of a
 * station list), DEVICE arrays: seg[n_sel] the region 0..n_regions - 1 of entry j, non-decreasing; wgt[n_sel] its weight, finite and >= 0;
 * offs[n_regions + 1] the first entry of every region (offs[0] = 0, offs[n_regions] = n_sel; an empty region is allowed).  A position in k regions is
 * listed k times; a position in none is not listed and never evaluated.  The flat point list of a request with nt time nodes is time-major:
 * point i = it * n_sel + j (nt * n_sel < 2^31).  Its cell is c = it * n_regions + seg[j], its group g = i / DPN_REG_GROUP, its slot s = g + c: g and c
 * are both non-decreasing in i, so every (group, cell) pair that occurs has a slot of its own.  S = ceil(nt * n_sel / DPN_REG_GROUP) + nt * n_regions.
 * Partial state (DpnRegionState) of P = n_products columns and E = n_thr thresholds, slot-major per column:
 *   double w[P][S], wx[P][S]; int32 count[P][S]; float vmin[P][S], vmax[P][S]; int32 imin[P][S], imax[P][S] (an entry j of the plan); double wexc[E][S].
 * The caller zeroes the whole state once (a plain memset).  A slot is written by exactly one launch, so chunking cannot change a bit.
 * dpn_region_accumulate takes points first .. first + n of the flat list (first a multiple of DPN_REG_GROUP; out_n, jac_n, f: that chunk's rows, *phys,
 * with_clip, products: ids, expressions, order and NaN rule of dpn_ensemble_accumulate; jac_n / f may be NULL as there).  Within a slot the points are
 * taken in increasing i, one after the other.  With x the product and wt = wgt[j], the point is skipped in that column if x is not finite or wt == 0;
 * otherwise, every operation rounded on its own:
 *   the first point of the slot sets vmin = vmax = x, imin = imax = j; a later one: if (x < vmin) vmin = x, imin = j; if (x > vmax) vmax = x, imax = j
 *   (strict: on a tie, +0 against -0 included, the earlier point stays);  count += 1;  w = w + (double)wt;  wx = wx + (double)wt * (double)x  (the
 *   product of two floats is exact in fp64);  for every threshold e with thr_col[e] == the column and x > thr_val[e] (strict, in float32):
 *   wexc[e] = wexc[e] + (double)wt.
 * A slot without a counted point keeps its zeros.  256-thread blocks cover four groups: every thread forms its point's P products into an LDS tile
 * [P][256]; lane L < P of each wave then walks its wave's 64 points for column L, lane P + e for threshold e, and stores at every change of cell.
 * dpn_region_finish, one thread per (cell, column): over the cell's slots (it * n_sel + offs[r]) / 64 + c .. (it * n_sel + offs[r + 1] - 1) / 64 + c
 * in increasing order, a slot with count == 0 skipped: count, w, wx and wexc added one after the other in fp64, min / max merged by the same
 * strict comparisons (the earlier slot stays).  Outputs (DpnRegionOut), [nt][n_regions][P] and frac [nt][n_regions][E]:
 *   mean = (float)(wx / w); total = (float)wx; weight = (float)w; min, max; where_min, where_max = imin, imax; count; frac[e] = (float)(wexc[e] / w)
 *   with w of column thr_col[e].  A cell without a counted point: count = 0, weight = 0, where = -1, the rest NaN.
 * products, thr_col and thr_val are HOST arrays.
 * -1 (nothing launched, nothing written): a NULL required pointer (thr_col, thr_val, wexc, frac: required when n_thr > 0; offs: finish; seg, wgt:
 * accumulate); n_sel < 1; n_regions < 1; nt < 1; nt * n_sel >= 2^31; n_products outside 1..DPN_REG_MAX_COLUMNS; n_thr outside
 * 0..DPN_REG_MAX_THRESHOLDS; a thr_col outside 0..n_products - 1.  accumulate: n <= 0; first < 0; first not a multiple of DPN_REG_GROUP;
 * first + n > nt * n_sel; an id outside 0..DPN_ENS_PRODUCTS - 1; a threshold that is not finite; a selected id that reads J (f) while jac_n (f) is NULL. */
#define DPN_REG_GROUP 64
#define DPN_REG_MAX_COLUMNS 16
#define DPN_REG_MAX_THRESHOLDS 16
typedef struct DpnRegionPlan {
    const int32_t* seg;
    const float* wgt;
    const int32_t* offs;
    int64_t n_sel;
    int32_t n_regions, nt;
} DpnRegionPlan;
typedef struct DpnRegionState {
    double *w, *wx;
    int32_t* count;
    float *vmin, *vmax;
    int32_t *imin, *imax;
    double* wexc;
} DpnRegionState;
typedef struct DpnRegionOut {
    float *mean, *total, *weight, *min, *max;
    int32_t *where_min, *where_max, *count;
    float* frac;
} DpnRegionOut;
int dpn_region_accumulate(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnPhysics* phys, int with_clip,
                          const int32_t* products /* HOST, n_products ids */, int n_products, const int32_t* thr_col /* HOST [n_thr] */,
                          const float* thr_val /* HOST [n_thr] */, int n_thr, int64_t first, const DpnRegionPlan* plan, const DpnRegionState* state,
                          void* stream);
int dpn_region_finish(const DpnRegionPlan* plan, const DpnRegionState* state, int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr,
                      const DpnRegionOut* out, void* stream);
/* Forecast verification against observations (csrc/dpn_verify.inc, compiled into csrc/dpn_diag.hip): per point and column the error of the forecast
 * and of the baseline -- the interpolated coarse forecast, coord_data -- against reports, folded case by case (one forecast date each) into a resident
 * fp64 state, pooled over groups of points in one fixed order, and turned into scores.  No atomics anywhere: two runs give the same bits.
 * Columns: P = n_products (1..DPN_VERIFY_MAX_COLUMNS) HOST ids out of the value products 28..33 (u, v, p, T, q, rho), 25 (speed) and 26
 * (rel_humidity); ids may repeat.  The forecast value x of a column is formed exactly as dpn_ensemble_accumulate forms that id from out_n (the
 * residual body's val, with_clip as dpn_diagnostics_out takes it, J = 0: the fields-only forward; a point with a NaN among its six out_n is NaN in
 * every column).  The baseline value b is formed by the same code from coord_data [n][6] in the place of out_n: for ids 28..33 what dpn_fields_out
 * writes for out_n := coord_data, for 25 and 26 what dpn_diagnostics_out writes; with_clip applies to both sides.  The observation o = obs[i][j]
 * (fp32 [n][P], physical units, NaN = no report) is never clipped.
 * Thresholds: E = n_thr (0..DPN_VERIFY_MAX_THRESHOLDS) HOST triples (thr_col[e] the column, thr_val[e] finite, thr_side[e] = DPN_VERIFY_ABOVE or
 * _BELOW).  A value z is an event when z > thr_val (above) or z < thr_val (below): strict, compared in float32.
 * State (DpnVerifyState) of n_total points, product-major (a wave's accesses run along the points), zeroed by the caller with one memset:
 *   int32 n[P][n_total]; double mean_f, mean_o, m2_f, m2_o, c_fo, sum_d, sum_ad, sum_d2, sum_e, sum_ae, sum_e2 [P][n_total]; float max_ad[P][n_total];
 *   int32 cont[E][6][n_total]: hits, false alarms, misses of the forecast, then of the baseline.
 * dpn_verify_accumulate folds ONE case at points first .. first + n (out_n, coord_data, obs: that chunk's rows).  A (point, column) pair is counted
 * only when x, b and o are all finite; otherwise nothing of that column changes.  Per counted pair, every operation an fp64 operation rounded on
 * its own (the kernels are compiled without contraction), left to right, with X = (double)x, O = (double)o, B = (double)b:
 *   c = n + 1
 *   df = X - mean_f;  mean_f = mean_f + df / (double)c;  dq = O - mean_o;  mean_o = mean_o + dq / (double)c
 *   m2_f = m2_f + df * (X - mean_f);  m2_o = m2_o + dq * (O - mean_o);  c_fo = c_fo + df * (O - mean_o)          (the new means)
 *   d = X - O;  sum_d = sum_d + d;  sum_ad = sum_ad + fabs(d);  sum_d2 = sum_d2 + d * d;  a = (float)fabs(d);  if (a > max_ad) max_ad = a
 *   e = B - O;  sum_e = sum_e + e;  sum_ae = sum_ae + fabs(e);  sum_e2 = sum_e2 + e * e;  n = c
 *   for every threshold t with thr_col[t] == j, ev(.) the event test:   hits += ev(x) && ev(o);  false alarms += ev(x) && !ev(o);
 *   misses += !ev(x) && ev(o);  the same three with b in the place of x.  Correct negatives are n minus the three.
 * One thread per point, 256-thread blocks, the columns looped inside the thread, no atomics, no LDS, plain vector stores.
 * dpn_verify_pool pools the states of N points into the states of G groups (the same layout, n_total = G; written, not accumulated).  order
 * [N] int32 (DEVICE) is a stable sort of the points by group, seg_start [G + 1] int64 (DEVICE, and the same numbers in seg_start_host, which is the
 * copy that is checked) the first place of every group in it; an empty group is allowed, an order entry outside 0..N - 1 is skipped.  One 64-lane
 * wave per (group, column): lane l left-folds the states of places l, l + 64, l + 128, .. of its segment in that order, then lane 0 left-folds the
 * 64 lane results in lane order.  A fold step merges an earlier state A with a later state B: when B is empty (n == 0) A stays as it is, when A is
 * empty the result is B, otherwise (Chan's pairwise merge), every operation rounded on its own, left to right:
 *   n = nA + nB;  w = ((double)nA * (double)nB) / (double)n;  r = (double)nB / (double)n
 *   gf = mean_fB - mean_fA;  go = mean_oB - mean_oA
 *   m2_f = (m2_fA + m2_fB) + (gf * gf) * w;  m2_o = (m2_oA + m2_oB) + (go * go) * w;  c_fo = (c_foA + c_foB) + (gf * go) * w
 *   mean_f = mean_fA + gf * r;  mean_o = mean_oA + go * r
 *   every sum: A + B;  max_ad: B's when it is greater (strict), else A's.
 * The contingency counts of a threshold are added (int32) over the segment of its column.  A fixed order and no atomics: two runs give the same
 * bits, and so does any chunking of the accumulate calls before.
 * dpn_verify_finish writes, for points (or groups) first .. first + n, rows [n][P] (DpnVerifyOut), every float an fp32 cast of the fp64 result, with
 * N = (double)n of the column:
 *   count = n;  bias = sum_d / N;  mae = sum_ad / N;  rmse = sqrt(sum_d2 / N);  max_abs_error = max_ad;  corr = c_fo / sqrt(m2_f * m2_o), NaN when
 *   n < 2 or m2_f == 0 or m2_o == 0;  base_bias = sum_e / N;  base_mae = sum_ae / N;  base_rmse = sqrt(sum_e2 / N);  skill = 1.0 - sum_d2 / sum_e2,
 *   NaN when sum_e2 == 0;  every score NaN when n == 0
 * and per threshold [n][E], for the forecast and (base_*) for the baseline, with h, f, m the three counts as doubles and N of column thr_col[e]:
 *   pod = h / (h + m);  far = f / (h + f);  csi = h / ((h + f) + m);  fbias = (h + f) / (h + m);
 *   ets = (h - hr) / (((h + f) + m) - hr) with hr = ((h + f) * (h + m)) / N                           each NaN where its denominator is 0 (n == 0: all).
 * The ten threshold destinations may be NULL when n_thr == 0.
 * -1 (nothing launched, nothing written), all three: a NULL required pointer (the state's fourteen; cont, thr_col, thr_val, thr_side and the ten
 * threshold destinations: required when n_thr > 0); n <= 0; first < 0; first + n > n_total; n_products outside 1..DPN_VERIFY_MAX_COLUMNS; n_thr outside
 * 0..DPN_VERIFY_MAX_THRESHOLDS; a thr_col outside 0..n_products - 1.  accumulate: an id other than 25, 26, 28..33; a side other than the two; a
 * threshold that is not finite.  pool: N <= 0; G <= 0; seg_start_host not non-decreasing from 0 to N. */
#define DPN_VERIFY_MAX_COLUMNS 16
#define DPN_VERIFY_MAX_THRESHOLDS 16
#define DPN_VERIFY_ABOVE 0
#define DPN_VERIFY_BELOW 1
typedef struct DpnVerifyState {
    int32_t* n;
    double *mean_f, *mean_o, *m2_f, *m2_o, *c_fo;
    double *sum_d, *sum_ad, *sum_d2;
    double *sum_e, *sum_ae, *sum_e2;
    float* max_ad;
    int32_t* cont;
} DpnVerifyState;
typedef struct DpnVerifyOut {
    int32_t* count;
    float *bias, *mae, *rmse, *max_abs_error, *corr, *base_bias, *base_mae, *base_rmse, *skill;
    float *pod, *far, *csi, *fbias, *ets, *base_pod, *base_far, *base_csi, *base_fbias, *base_ets;
} DpnVerifyOut;
int dpn_verify_accumulate(const float* out_n, const float* coord_data, const float* obs, int64_t n, const DpnPhysics* phys, int with_clip,
                          const int32_t* products /* HOST, n_products ids */, int n_products, const int32_t* thr_col /* HOST [n_thr] */,
                          const float* thr_val /* HOST [n_thr] */, const int32_t* thr_side /* HOST [n_thr] */, int n_thr, int64_t first,
                          int64_t n_total, const DpnVerifyState* state, void* stream);
int dpn_verify_pool(const DpnVerifyState* points, int64_t n_points, const int32_t* order /* DEVICE [n_points] */,
                    const int64_t* seg_start /* DEVICE [n_groups + 1] */, const int64_t* seg_start_host /* HOST, the same */, int64_t n_groups,
                    int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr, const DpnVerifyState* groups, void* stream);
int dpn_verify_finish(const DpnVerifyState* state, int64_t n_total, int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr,
                      int64_t first, int64_t n, const DpnVerifyOut* rows, void* stream);
/* Probabilistic verification of ensembles against observations (csrc/dpn_pverify.inc, compiled into csrc/dpn_diag.hip): M members per case (one
 * forecast date), scored as a distribution against the reports -- CRPS, rank histogram, spread against skill, and per threshold the Brier score
 * with its decomposition, the reliability diagram and the ROC area -- for the forecast and for the baseline, folded case by case into a resident
 * state, pooled over groups of points in one fixed order, and turned into scores.  No atomics anywhere: two runs give the same bits.
 * Columns (P, ids 25, 26, 28..33), values x (from out_n) and b (from coord_data), with_clip and thresholds (E triples, strict float32 compares,
 * ev(.) the event test) are those of the dpn_verify_* block above, formed by the same code.  M = n_members, 1..DPN_PV_MAX_MEMBERS, is fixed for
 * a request.
 * dpn_pverify_stage takes ONE member's chunk (out_n, coord_data [n][6]; member 0..M - 1; points first .. first + n of n_total) and writes x and b
 * of every column into plane_f and plane_b, fp32 [M][P][n_total] (member-major, then product-major: a wave's accesses run along the points):
 *   plane[(member * P + j) * n_total + first + i].  One thread per point, plain vector stores.
 * State (DpnPVerifyState) of n_total points, zeroed by the caller with one memset; side 0 is the forecast, side 1 the baseline:
 *   int32 n[P][n_total]; double sum_crps, sum_fair, sum_d, sum_d2, sum_var [2][P][n_total]; int32 rank[2][P][M + 1][n_total];
 *   int32 rel[E][2][2][M + 1][n_total]: per threshold and side, for every probability level k / M, [0] the number of pairs whose ensemble has k
 *   event members and [1] the number of those whose report is an event.
 * dpn_pverify_case runs after the M members of ONE case are staged and folds the case in at points first .. first + n against obs [n][P] (fp32,
 * NaN = no report, never clipped).  A (point, column) pair is counted only when all M values x_m, all M values b_m and o are finite; otherwise
 * nothing of that column changes.  Per counted pair n = n + 1, and per side (x_m the side's values), every operation an fp64 operation rounded
 * on its own, left to right, with X_m = (double)x_m, O = (double)o, Md = (double)M, every sum from 0.0 with m ascending:
 *   a = sum_m fabs(X_m - O);   s = sum_m X_m;   lt = #{x_m < o};  eq = #{x_m == o}                                    (float32 compares)
 *   g = sum_{i < k} fabs(X_i - X_k), i ascending outside, k ascending inside
 *   mean = s / Md;  d = mean - O;  v = sum_m (X_m - mean) * (X_m - mean)
 *   crps = a / Md - g / (Md * Md);   fair = a / Md - g / (Md * (Md - 1.0)), a when M == 1;   var = v / (Md - 1.0), 0.0 when M == 1
 *   sum_crps += crps;  sum_fair += fair;  sum_d += d;  sum_d2 += d * d;  sum_var += var
 *   rank[lt + eq / 2] += 1                            (integer division: the middle of the tie range, a deterministic stand-in for a random draw)
 *   for every threshold t with thr_col[t] == j:  k = #{m: ev(x_m)};  rel[t][side][0][k] += 1;  if ev(o): rel[t][side][1][k] += 1.
 * One 64-thread block per 64 points; a thread copies the 2 * M values of its point and column into LDS as [side][M][64] (lane = point; at most
 * 32 KiB) and walks its own column there, so the pair loop indexes no private array.  No atomics, no barrier.
 * dpn_pverify_pool pools the states of N points into the states of G groups (the same layout, n_total = G; written, not accumulated), with order,
 * seg_start and seg_start_host as dpn_verify_pool takes them.  One 64-lane wave per (group, column): per fp64 field and side, lane l adds, from
 * 0.0, the entries of places l, l + 64, l + 128, .. of its segment in that order (an order entry outside 0..N - 1 is skipped), then lane 0 adds
 * to its own result the results of lanes 1..63 in lane order (a lane without a place holds 0.0).  Every field is a sum, so a merge is A + B; the
 * int32 fields (n, rank, and rel of the thresholds on the column) are added over the segment.
 * dpn_pverify_finish writes, for points (or groups) first .. first + n, every float an fp32 cast of the fp64 result, with N = (double)n of the
 * column, per column [n][P] and side (the baseline's in the base_ destinations):
 *   count = n;  crps = sum_crps / N;  fair_crps = sum_fair / N;  bias = sum_d / N;  rmse = sqrt(sum_d2 / N);  spread = sqrt(sum_var / N);
 *   spread_skill = sqrt(((Md + 1.0) / Md) * (sum_var / N)) / sqrt(sum_d2 / N), NaN when M < 2 or the divisor is 0;
 *   rank_hist [n][P][M + 1] = rank
 * once per column: crpss = 1.0 - sum_crps(forecast) / sum_crps(baseline);  fair_crpss likewise from sum_fair;  NaN when the divisor is 0
 * and per threshold [n][E] and side, from the integer table alone, n_k = rel[..][0][k] and o_k = rel[..][1][k], N of column thr_col[e], Md as above,
 * p = (double)k / Md, every sum from 0.0:
 *   brier = (sum_{k = 0..M} ((double)o_k * ((1.0 - p) * (1.0 - p)) + (double)(n_k - o_k) * (p * p))) / N
 *   obar = (double)(sum_k o_k) / N            (the int32 sum);   f = (double)o_k / (double)n_k
 *   reliability = (sum_{k = 0..M, n_k > 0} (double)n_k * ((p - f) * (p - f))) / N;   resolution = (sum likewise of (double)n_k * ((f - obar) * (f - obar))) / N
 *   uncertainty = obar * (1.0 - obar), written once per threshold (from side 0; both sides hold the same reports);
 *   bss = 1.0 - brier / uncertainty, NaN when uncertainty == 0
 *   roc_area: the trapezoids under the M + 2 points (false-alarm rate, hit rate) of the decisions "at least j members", j = M + 1 (0, 0) down to
 *   0 (1, 1):  area = sum_{k = M..0, descending} (double)(n_k - o_k) * ((double)A_k + (double)(A_k + o_k)) with A_k = sum_{k' > k} o_k' (int32);
 *   roc_area = area / ((2.0 * (double)ev) * (double)(n - ev)) with ev = sum_k o_k, NaN when ev == 0 or ev == n
 *   rel_n, rel_o [n][E][M + 1] = n_k, o_k (the reliability diagram itself).
 * Every score is NaN when n == 0.  The threshold destinations may be NULL when n_thr == 0.
 * -1 (nothing launched, nothing written): a NULL required pointer (the planes, obs, the state's eight -- rel, thr_col, thr_val, thr_side and the
 * threshold destinations: required when n_thr > 0); n <= 0; first < 0; first + n > n_total; n_products outside 1..DPN_VERIFY_MAX_COLUMNS; n_thr
 * outside 0..DPN_VERIFY_MAX_THRESHOLDS; n_members outside 1..DPN_PV_MAX_MEMBERS; a thr_col outside 0..n_products - 1.  stage: a member outside
 * 0..n_members - 1; an id other than 25, 26, 28..33.  case: a side other than the two; a threshold that is not finite.  pool: N <= 0; G <= 0;
 * seg_start_host not non-decreasing from 0 to N. */
#define DPN_PV_MAX_MEMBERS 64
typedef struct DpnPVerifyState {
    int32_t* n;
    double *sum_crps, *sum_fair, *sum_d, *sum_d2, *sum_var;
    int32_t *rank, *rel;
} DpnPVerifyState;
typedef struct DpnPVerifyOut {
    int32_t* count;
    float *crps, *fair_crps, *bias, *rmse, *spread, *spread_skill;
    float *base_crps, *base_fair_crps, *base_bias, *base_rmse, *base_spread, *base_spread_skill;
    float *crpss, *fair_crpss;
    int32_t *rank_hist, *base_rank_hist;
    float *brier, *reliability, *resolution, *bss, *roc_area;
    float *base_brier, *base_reliability, *base_resolution, *base_bss, *base_roc_area;
    float* uncertainty;
    int32_t *rel_n, *rel_o, *base_rel_n, *base_rel_o;
} DpnPVerifyOut;
int dpn_pverify_stage(const float* out_n, const float* coord_data, int64_t n, const DpnPhysics* phys, int with_clip,
                      const int32_t* products /* HOST, n_products ids */, int n_products, int member, int n_members, int64_t first, int64_t n_total,
                      float* plane_f, float* plane_b, void* stream);
int dpn_pverify_case(const float* plane_f, const float* plane_b, const float* obs, int64_t n, int n_products,
                     const int32_t* thr_col /* HOST [n_thr] */, const float* thr_val /* HOST [n_thr] */, const int32_t* thr_side /* HOST [n_thr] */,
                     int n_thr, int n_members, int64_t first, int64_t n_total, const DpnPVerifyState* state, void* stream);
int dpn_pverify_pool(const DpnPVerifyState* points, int64_t n_points, const int32_t* order /* DEVICE [n_points] */,
                     const int64_t* seg_start /* DEVICE [n_groups + 1] */, const int64_t* seg_start_host /* HOST, the same */, int64_t n_groups,
                     int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr, int n_members, const DpnPVerifyState* groups, void* stream);
int dpn_pverify_finish(const DpnPVerifyState* state, int64_t n_total, int n_products, const int32_t* thr_col /* HOST [n_thr] */, int n_thr,
                       int n_members, int64_t first, int64_t n, const DpnPVerifyOut* rows, void* stream);
/* Neighbourhood verification on lattices against gridded analyses (csrc/dpn_nbhd.inc, compiled into csrc/dpn_diag.hip): the fractions skill score
 * (FSS, Roberts & Lean 2008) of the forecast and of the baseline against an analysis that lives on the lattice's own nodes, over square windows
 * of growing width, folded case by case (one forecast date each) into a resident fp64 state.  No atomics anywhere: two runs give the same bits.
 * Request: P columns (ids 25, 26, 28..33, 1..DPN_VERIFY_MAX_COLUMNS) and E = n_thr thresholds, 1..DPN_VERIFY_MAX_THRESHOLDS (at least one: the
 * FSS is a score of events), HOST triples with the strict float32 event test ev(.) of the dpn_verify_* block; K = n_scales half-widths
 * radius[k] >= 0 in lattice nodes, 1..DPN_NBHD_MAX_SCALES, strictly ascending, the window of half-width r being (2 r + 1)^2 nodes; a lattice with
 * nx * ny * nt < 2^31.  Plane p = it * E + e.
 * Values: x from out_n and b from coord_data, formed as dpn_verify_accumulate forms them (with_clip on both); o = analysis[it][j][iy][ix], fp32
 * [nt][P][ny][nx] on the device (the layout dpn_diagnostics_out writes maps in), physical units, never clipped, NaN = none.  A node of a column
 * is valid when x, b and o are all finite.
 * dpn_nbhd_stage takes ONE case's chunk (out_n, coord_data [n][6]: points first .. first + n of *lattice; analysis: the whole array), finds its
 * own (it, iy, ix) and writes, for every threshold e on column j, mask[it][e][iy][ix] (uint8 [nt][E][ny][nx]):
 *   bit 0: valid && ev(x);  bit 1: valid && ev(b);  bit 2: valid && ev(o);  bit 3: valid.        One thread per point, plain byte stores.
 * dpn_nbhd_fold runs once a case's lattice is fully staged, for planes p0 .. p0 + np.  scratch (DEVICE, 16-byte aligned) holds, for the np planes,
 *   int32 S[np][ny + 1][nx + 1][4]; then double part[np][K][ny][5]; then int32 rows[np][K][ny]                  (no gaps)
 * S is the exclusive summed-area table of the four counts f, b, o, valid (mask bits 0..3) of a plane, interleaved so that a corner is one 16-byte
 * load: S[y][x][c] = the number of nodes iy < y, ix < x with bit c set; row 0 and column 0 are zero.  Integer sums are exact: the order of the
 * scan is free (a row pass by wave shuffles, then a column pass).
 * The window of node (ix, iy) at half-width r is clamped to the plane: x0 = max(ix - r, 0), x1 = min(ix + r + 1, nx), y0 = max(iy - r, 0),
 * y1 = min(iy + r + 1, ny); each count c = S[y1][x1] - S[y0][x1] - S[y1][x0] + S[y0][x0] in int32.  A window with c_valid == 0 is skipped.
 * Otherwise, every operation an fp64 operation rounded on its own (the kernels are compiled without contraction):
 *   V = (double)c_valid;  Pf = (double)c_f / V;  Pb = (double)c_b / V;  Po = (double)c_o / V;  a = Pf - Po;  g = Pb - Po
 *   the five terms a * a, Pf * Pf, Po * Po, g * g, Pb * Pb (of sum_fo2, sum_f2, sum_o2, sum_bo2, sum_b2), and the window count + 1.
 * Order of the reduction: one 64-lane wave per (plane, scale, row iy): lane l adds, from +0.0 and 0, the terms of the nodes ix = l, l + 64, .. in
 * that order, then lane 0 adds to its own result those of lanes 1..63 in lane order -> part[pl][k][iy][0..4], rows[pl][k][iy].  One wave per
 * (plane, scale) then folds the rows the same way (lane l the rows l, l + 64, ..; lane 0 the lane results in lane order) and adds the case's
 * total to the state with one fp64 addition per sum (int64 for the count); the plane totals S[ny][nx] are added to n_f, n_b, n_o, n_valid.  Any
 * np gives the same bits.
 * State (DpnNbhdState), zeroed by the caller with one memset:
 *   double sum_fo2, sum_f2, sum_o2, sum_bo2, sum_b2 [nt][E][K]; int64 windows [nt][E][K]; int64 n_valid, n_f, n_b, n_o [nt][E].
 * dpn_nbhd_finish writes two tables (DpnNbhdOut), `hour` per (it, e) and `all` per e, the latter from the state's entries added over it = 0 ..
 * nt - 1 in that order (fp64 and int64).  Every float is an fp32 cast of the fp64 result, NaN where its denominator is 0:
 *   fss = 1.0 - sum_fo2 / (sum_f2 + sum_o2);  base_fss = 1.0 - sum_bo2 / (sum_b2 + sum_o2);  windows                       [..][K]
 *   freq_f, freq_b, freq_o = (double)n_. / (double)n_valid;  fbias = (double)n_f / (double)n_o;  base_fbias = (double)n_b / (double)n_o;
 *   useful = 0.5 + freq_o * 0.5;  count = n_valid;  skilful_scale, base_skilful_scale: the smallest k whose fp64 fss (base_fss) is defined
 *   and >= the fp64 useful, or -1 (also when n_valid == 0).
 * -1 (nothing launched, nothing written): a NULL required pointer; stage: n <= 0, first < 0, first + n past the lattice, n_products outside
 * 1..DPN_VERIFY_MAX_COLUMNS, a thr_col outside 0..n_products - 1, an id other than 25, 26, 28..33, a side other than the two, a threshold that is
 * not finite; all: n_thr outside 1..DPN_VERIFY_MAX_THRESHOLDS; stage, fold: nx, ny or nt < 1, nx * ny * nt >= 2^31; fold, finish: n_scales
 * outside 1..DPN_NBHD_MAX_SCALES; fold: a radius < 0 or not strictly ascending, p0 < 0, np <= 0, p0 + np > nt * E, np * ny or np * ceil((nx + 1)
 * / 64) past 2^31 - 1 (one block per plane and row, and per plane and 64 columns); finish: nt < 1. */
#define DPN_NBHD_MAX_SCALES 8
typedef struct DpnNbhdState {
    double *sum_fo2, *sum_f2, *sum_o2, *sum_bo2, *sum_b2;
    int64_t* windows;
    int64_t *n_valid, *n_f, *n_b, *n_o;
} DpnNbhdState;
typedef struct DpnNbhdOut {
    float *fss, *base_fss;
    int64_t* windows;
    float *freq_f, *freq_b, *freq_o, *fbias, *base_fbias, *useful;
    int64_t* count;
    int32_t *skilful_scale, *base_skilful_scale;
} DpnNbhdOut;
int dpn_nbhd_stage(const float* out_n, const float* coord_data, const float* analysis, int64_t n, const DpnPhysics* phys, int with_clip,
                   const int32_t* products /* HOST, n_products ids */, int n_products, const int32_t* thr_col /* HOST [n_thr] */,
                   const float* thr_val /* HOST [n_thr] */, const int32_t* thr_side /* HOST [n_thr] */, int n_thr, const DpnLattice* lattice,
                   int64_t first, uint8_t* mask, void* stream);
int dpn_nbhd_fold(const uint8_t* mask, const DpnLattice* lattice, int n_thr, const int32_t* radius /* HOST [n_scales] */, int n_scales, int64_t p0,
                  int64_t np, void* scratch, const DpnNbhdState* state, void* stream);
int dpn_nbhd_finish(const DpnNbhdState* state, int nt, int n_thr, int n_scales, const DpnNbhdOut* hour, const DpnNbhdOut* all, void* stream);

/* ---------------------------------------------------------------- parcel trajectories through the learned wind (csrc/dpn_traj.hip)
 * One launch = one stage of an explicit Runge-Kutta step for n parcels whose stage positions depend only on the step's start point and the
 * previous stage's slope (Euler, midpoint, classical RK4; the stage tables live in deepphysinet_amd/trajectory.py).  Between two fields-only
 * forwards it does everything: the wind from the forward's out_n, the accumulators, the next evaluation point, the domain check, and the sampler's
 * x, y, t, f, coord_data at that point for the next forward.
 *   t0        the step's start hour (all parcels share the clock);  h  the step in hours, negative = backward in time
 *   w         weight of this stage's slope in the step's sum;       inv_wsum  1 / (sum of the weights)
 *   a_next, c_next   the next evaluation point lies a_next * h along this slope, at hour t0 + c_next * h (not read when last)
 *   first     the step's first stage (its forward was evaluated at the path point: the optional fields row is written)
 *   last      the stage that closes the step;   step  the step's index: path row step + 1 is written when last, fields row step when first
 *   record_only   only write fields row `step` (the final point's); state, path and the sampler outputs are not touched
 *   with_clip     the clip of P, T, q, rho in the fields rows (as dpn_fields_out); the wind is never clipped */
typedef struct DpnTrajStage {
    double t0, h, w, a_next, c_next, inv_wsum;
    int64_t step;
    int32_t first, last, record_only, with_clip;
} DpnTrajStage;
#define DPN_TRAJ_ALIVE       0
#define DPN_TRAJ_LEFT_GRID   1   /* the next point left [0, lon - 1] x [0, lat - 1] of the fine grid */
#define DPN_TRAJ_LEFT_WINDOW 2   /* the next hour left [0, t_hours]                                  */
#define DPN_TRAJ_BAD_WIND    3   /* u or v not finite                                                */
/* State per parcel: x0, y0 [n] fp64 (the start point of the current step, fine-grid index units as dpn_sample_at takes them), accx, accy [n] fp64
 * (the weighted slope sums), status [n] int32 (DPN_TRAJ_*), steps_done [n] int32.  out_n [n][6]: the forward at the current evaluation point.
 * Per parcel with status 0, every operation an fp64 operation rounded on its own (the kernel is compiled without contraction), left to right:
 *   u  = (double)denorm(out_n[i][0], 0)      v  = (double)denorm(out_n[i][1], 1)       denorm: dpn_fields_out's fp32 arithmetic, no clip
 *   kx = (u * 3600.0) / (double)s->dx        ky = (v * 3600.0) / (double)s->dy         index units per hour
 *   ax = accx + w * kx                       ay = accy + w * ky
 *   not last:  xe = x0 + (a_next * h) * kx   ye = y0 + (a_next * h) * ky   te = t0 + c_next * h
 *   last:      xe = x0 + (h * inv_wsum) * ax ye = y0 + (h * inv_wsum) * ay te = t0 + h
 *   status:    3 when u or v is not finite; else 1 unless 0 <= xe <= lon - 1 and 0 <= ye <= lat - 1; else 2 unless 0 <= te <= t_hours
 *              (a NaN fails every comparison; the faces themselves are inside)
 *   still 0, not last:  accx = ax, accy = ay
 *   still 0, last:      x0 = xe, y0 = ye, accx = accy = 0, steps_done += 1, path[step + 1][i] = (xe, ye)
 *   still 0:            x, y, t, f, coord_data [i] = the sampler at (xe, ye, te), dpn_sample_at's arithmetic
 * A parcel whose status becomes non-zero keeps x0, y0, accx, accy, steps_done and its x, y, t, f, coord_data as they were: the state of its last
 * completed step, and the last valid evaluation point, so that no NaN reaches the next forward (whose result for it is ignored).  When last,
 * path[step + 1][i] of such a parcel, and of every parcel that came in with a non-zero status, is (NaN, NaN); nothing else of a dead parcel is written.
 * fields (optional, [path_rows][n][6]): when first or record_only, fields[step][i][k] = denorm(out_n[i][k], k, with_clip) for parcels that came in
 * with status 0, NaN for the others.  path: [path_rows][n][2] fp64; row 0 (the start points) is the caller's.
 * 256-thread blocks, one parcel per thread, no atomics, no LDS; all stores are per-thread vector stores.
 * -1 (nothing launched, nothing written): a NULL s, cube, phys, out_n, st, state pointer, path or sampler output; n <= 0; a sampler dimension < 2;
 * h == 0 or not finite; t0, w, a_next, c_next or inv_wsum not finite; step < 0, step + 1 >= path_rows (record_only: step >= path_rows); fields
 * with neither first nor record_only; record_only without fields. */
int dpn_traj_stage(const DpnSampler* s, const float* cube, const DpnPhysics* phys, const float* out_n, int64_t n, const DpnTrajStage* st,
                   double* x0, double* y0, double* accx, double* accy, int32_t* status, int32_t* steps_done, double* path, int64_t path_rows,
                   float* fields, float* x, float* y, float* t, float* f, float* coord_data, void* stream);

/* The same step with the optimiser state held as ONE flat fp32 buffer per moment: tensor i lives at offset (sum of ceil(numel_j / 2048)
 * over j < i) * 2048, i.e. every tensor is padded to whole 2048-element chunks; dpn_clip_adam_flat_floats gives the buffer length.
 * No per-tensor state pointers travel in the kernel arguments, so up to 160 tensors are ONE launch per pass: three launches for a
 * PhysicsNet (gradient norm, its fixed-order reduction, update). */
int64_t dpn_clip_adam_flat_floats(int n_tensors, const int64_t* numel);
int dpn_clip_adam_flat(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                       float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float max_norm, float* out_norm_dev, void* stream);

/* The same with the hyper-parameters read from DEVICE memory at run time: hyper_dev[7] = {lr, beta1, beta2, eps, weight_decay, max_norm,
 * grad_scale}.  A step captured in a hipGraph then follows a learning-rate schedule (CosineAnnealingLR stepped per epoch,
 * interface_physics.py:831-833) -- the host rewrites hyper_dev[0] between replays; grad_scale multiplies every gradient before the norm and
 * the update (1 / world_size behind a SUM all-reduce of the flat gradient buffer, replacing DistributedDataParallel's averaging, :903-907). */
int dpn_clip_adam_flat_dev(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                           float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const float* hyper_dev, float* out_norm_dev,
                           void* stream);

/* dpn_clip_adam_flat_dev that also moves an exponential moving average (EMA) of the parameters, in the update launch: the thread that has formed
 * a new parameter value p' updates its shadow element, so the average costs one more read and one more write stream and no launch, and follows a
 * step replayed from a hipGraph.  ema_flat: the shadow, laid out exactly like exp_avg_flat (tensor i at chunk_start[i] * 2048; the padding is
 * never touched).  hyper_dev[8]: the seven values above and hyper_dev[7] = the decay.  ema_base_dev: device int, may be NULL (= 0), the number of
 * EMA updates made before this optimiser state was created (a resumed run).  All fp32, one rounding per operation, one fma:
 *     t = *step_dev after the bump;  te = t + base
 *     d  = ema_warmup ? fminf(decay, (1.f + (float)te) / (10.f + (float)te)) : decay
 *     s' = fmaf(d, s, (1.f - d) * p')
 * p, m, v, out_norm and *step_dev come out bit-identical to dpn_clip_adam_flat_dev.  -1 (nothing launched, nothing written): ema_flat or
 * hyper_dev NULL and everything dpn_clip_adam_flat_dev refuses. */
int dpn_clip_adam_flat_ema(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                           float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const float* hyper_dev, float* out_norm_dev,
                           float* ema_flat, const int* ema_base_dev, int ema_warmup, void* stream);
/* dpn_clip_adam_flat_dev / dpn_clip_adam_flat_ema with PARAMETER GROUPS (fine-tuning: a learning rate, betas, eps and weight decay per group).
 * group_of: HOST array of n_tensors bytes, the group of each tensor; n_groups: 1 .. 16; hyper_dev: device float[n_groups][8], row k =
 * {lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, ema_decay} of group k -- max_norm, grad_scale and ema_decay are read from row 0
 * only: the norm is taken over ALL tensors and the clip coefficient is global, as clip_grad_norm_ over every trainable parameter.  ema_flat
 * NULL: no EMA (ema_base_dev and ema_warmup are not read); otherwise as dpn_clip_adam_flat_ema.  One shared step counter.  Every tensor comes out
 * bit-identical to dpn_clip_adam_flat_dev / _ema called with its group's row as hyper_dev; with one group the call IS that call.  Three launches
 * per 160 tensors, no atomics.  A group without tensors is allowed.  -1 (nothing launched, nothing written): n_groups outside 1 .. 16, a group_of
 * entry >= n_groups, group_of or hyper_dev NULL, and everything dpn_clip_adam_flat_dev refuses. */
int dpn_clip_adam_flat_groups(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                              float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const uint8_t* group_of, int n_groups,
                              const float* hyper_dev, float* out_norm_dev, float* ema_flat, const int* ema_base_dev, int ema_warmup, void* stream);
/* The step guard: dpn_clip_adam_flat_groups that refuses a step whose gradient norm is non-finite or a spike, on the device, inside the same three
 * launches (a step replayed from a hipGraph cannot ask the host).  The state lives in device memory, zero-initialised by the caller: */
typedef struct DpnStepGuard {
    int32_t skipped_nonfinite;   /* calls whose total norm was NaN or +-inf                          */
    int32_t skipped_spike;       /* calls skipped as a spike                                         */
    int32_t verdict;             /* the last call: 0 applied, 1 non-finite, 2 spike                  */
    int32_t seen;                /* applied steps that have entered `running` (saturating)           */
    int32_t consecutive;         /* spike verdicts in a row up to and including the last call        */
    int32_t reserved;
    double  running;             /* running mean of the applied steps' total norms                   */
    double  last;                /* (double) of the last call's fp32 total norm                      */
} DpnStepGuard;
/* Arguments of dpn_clip_adam_flat_groups plus guard_dev and the spike rule (spike_factor = 0: off).  group_of NULL: one group, hyper_dev is one row
 * of 8 and n_groups is not read.  ema_flat NULL: no EMA.  Three launches per 160 tensors, no atomics, every sum in the order of the other entry
 * points; the gradient-norm launch is theirs.  *step_dev is bumped on EVERY call, applied or not (a sampler bound to it draws new points after a
 * skipped step).  One thread of the reduction launch forms the verdict from total = (float)sqrt(sumsq) * hyper_dev[6], the fp32 total exactly as the
 * update forms it; fp64, every operation rounded once, no contraction:
 *     !(fabsf(total) <= FLT_MAX)                                  verdict 1: skipped_nonfinite += 1, consecutive = 0
 *     else spike_factor > 0 && seen >= spike_warmup && (double)total > spike_factor * running && consecutive < spike_patience
 *                                                                 verdict 2: skipped_spike += 1, consecutive += 1
 *     else                                                        verdict 0: if consecutive == spike_patience (the guard is overruled: the level
 *                                                                 of the norms has moved for good) seen = 0; then
 *                                                                 running = seen == 0 ? total : spike_decay * running + (1 - spike_decay) * total,
 *                                                                 seen += 1 (saturating), consecutive = 0
 *     last = total in every case; running and seen move on verdict 0 only.
 * Update launches (all of them obey the one verdict): verdict != 0 -- every block returns without reading or writing p, m, v or the shadow;
 * *out_norm_dev is still written (the norm that was refused).  verdict 0 -- the arithmetic of the unguarded kernels with the step number
 * t = *step_dev - skipped_nonfinite - skipped_spike in both bias corrections and in the EMA's te = t + base.
 * Contracts: (1) while no call has been skipped, p, m, v, the shadow, *out_norm_dev and *step_dev come out bit-identical to dpn_clip_adam_flat_dev,
 * _ema or _groups on the same inputs; (2) after k skips an applied call is bit-identical to the unguarded entry called from the same state with its
 * step counter k lower (with EMA, te lower by k as well); (3) a skipped call leaves every byte of p, m, v and the shadow as it was.
 * What the guard does not see: a loss that is non-finite while all gradients are finite; and a finite gradient whose square overflows the fp32
 * per-thread partial (|g| above about 1.8e19) gives an infinite total and is skipped as non-finite.
 * -1 (nothing launched, nothing written, *step_dev included): guard_dev or hyper_dev NULL, spike_factor negative or not finite, spike_decay outside
 * [0, 1), spike_warmup < 1, spike_patience < 1, and everything dpn_clip_adam_flat_groups refuses (with group_of NULL its group checks do not apply). */
int dpn_clip_adam_flat_guard(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                             float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const uint8_t* group_of, int n_groups,
                             const float* hyper_dev, float* out_norm_dev, float* ema_flat, const int* ema_base_dev, int ema_warmup,
                             DpnStepGuard* guard_dev, double spike_factor, double spike_decay, int spike_warmup, int spike_patience, void* stream);
/* Exchanges every parameter with its shadow in ema_flat in place, bit for bit (validation and inference on the averaged weights without a second
 * model): one launch per 160 tensors over the same chunk table; the padding of ema_flat and everything outside the tensors stay untouched; two
 * calls are the identity.  -1: n_tensors <= 0, a NULL pointer, a numel outside 1 .. 2^31 - 1. */
int dpn_ema_swap(int n_tensors, float* const* params, const int64_t* numel, float* ema_flat, void* stream);

/* L-BFGS on the flat buffers ("vector-free": the inner products of an iteration are taken in ONE pass over the history, the two-loop recursion runs
 * on the small Gram matrix, the direction is formed in one more pass).  All flat buffers use dpn_clip_adam_flat_floats' layout (`total` floats,
 * tensor i at chunk_start[i] * 2048; the padding is never read or written); the parameters are reached through the pointer table, 160 tensors per
 * launch.  History: ring buffers S[m][total] and Y[m][total], 1 <= m <= 32.  Gram matrix G[(2m+1)^2] fp64 and delta[2m+1] fp64 over the basis BY RING
 * SLOT: s slot j = j, y slot j = m + j, g = 2m; entries of slots that hold no pair are never read.  No atomics; every reduction in a fixed order
 * (thread t of a 256-thread block adds elements t, t + 256, ... of its chunk, or partials t, t + 256, ...; lanes by the xor butterfly 32 .. 1, waves
 * as (w0 + w1) + (w2 + w3)); no contraction: deepphysinet_amd/lbfgs.py restates every kernel operation for operation.
 * The state lives in device memory, zero-initialised by the caller (zeroing it again empties the ring): */
typedef struct DpnLbfgsState {
    int32_t count;               /* pairs stored, 0 .. m                                                                 */
    int32_t newest;              /* ring slot of the newest pair (the next push writes slot (newest + 1) % m)            */
    int32_t iters;               /* directions formed (dpn_lbfgs_direction calls)                                        */
    int32_t skipped;             /* pairs refused by the rule s.y > 1e-10                                                */
    int32_t pending;             /* 1: the newest pair has not been judged yet (set by push, cleared by direction)       */
    int32_t reserved;
    double  gamma;               /* s.y / y.y of the newest standing pair (1 with none)                                  */
    double  gtd;                 /* g . d of the last direction                                                          */
    double  dnorm;               /* || d ||_2 of the last direction, sqrt(delta^T G delta)                               */
    double  g_l1;                /* sum |g|, max |g| (NaN-propagating) and g . g of the last dpn_lbfgs_gram call          */
    double  g_inf;
    double  gg;
} DpnLbfgsState;
/* Every entry: -1 with nothing launched and nothing written on n_tensors < 1, a NULL pointer, a numel outside 1 .. 2^31 - 1, m outside 1 .. 32 or a
 * step length t that is not finite.
 * dpn_lbfgs_scratch_doubles: the length of `scratch`, (3 (2m + 1) + 2) partials per 2048-element chunk.
 * dpn_lbfgs_save: x0_flat = the parameters, moved as 32-bit words.
 * dpn_lbfgs_move: p = fl(x0 + fl(t d)), fp32; every trial point is formed from the saved x0.  t == 0 copies x0's words (d is not read): the
 *   parameters are restored bit for bit.
 * dpn_lbfgs_push: slot (newest + 1) % m of S and Y receives s = fl(t d) and y = fl(g - g_prev), then g_prev = g; a one-thread launch then makes
 *   that slot the newest: count = min(count + 1, m), pending = 1.
 * dpn_lbfgs_gram: one pass over the flat buffers forms the inner products of the newest s, the newest y and g with every stored s, every stored y
 *   and g, and sum |g|, max |g|: products of fp32 operands formed in fp64 (exact), accumulated in fp64 per thread, one partial per chunk and
 *   quantity (partial[q * chunks + chunk], q = v (2m + 1) + b, then the two norms); a reduce launch (one block per quantity) adds the partials in
 *   index order and writes the rows and columns of G that belong to the three vectors, and g_l1, g_inf, gg of the state.
 * dpn_lbfgs_gtd: out_dev[0] = a . b of two flat vectors with the same arithmetic and order (the line search's g . d); scratch: one double per chunk.
 * dpn_lbfgs_direction: a one-thread fp64 launch, then one pass.  The thread first judges a pending pair: it stands when G[s_new, y_new] > 1e-10,
 *   otherwise the ring pointer steps back, count -= 1 and skipped += 1 (in a full ring the slot the refused pair overwrote is lost with it).  Then,
 *   basis order s oldest -> newest, y oldest -> newest, g, every product and every sum rounded once:
 *       delta = -e_g
 *       i newest -> oldest:  alpha_i = (delta . G[:, s_i]) / G[s_i, y_i];  delta[y_i] -= alpha_i
 *       delta *= gamma,      gamma = G[s_new, y_new] / G[y_new, y_new]  (no pair: 1)
 *       i oldest -> newest:  beta = (delta . G[:, y_i]) / G[s_i, y_i];     delta[s_i] += alpha_i - beta
 *       gtd = delta . G[:, g];  dnorm = sqrt(max(delta^T G delta, 0));  iters += 1
 *   and the pass forms d = sum_j delta_j b_j per element in fp64 in basis order, rounded once to fp32 (no pair stored: d = -g). */
int64_t dpn_lbfgs_scratch_doubles(int n_tensors, const int64_t* numel, int m);
int dpn_lbfgs_save(int n_tensors, float* const* params, const int64_t* numel, float* x0_flat, void* stream);
int dpn_lbfgs_move(int n_tensors, float* const* params, const int64_t* numel, const float* x0_flat, const float* d_flat, float t, void* stream);
int dpn_lbfgs_push(int n_tensors, float* const* params, const int64_t* numel, const float* g_flat, float* g_prev_flat, const float* d_flat, float t,
                   float* S, float* Y, int m, DpnLbfgsState* state, void* stream);
int dpn_lbfgs_gram(int n_tensors, float* const* params, const int64_t* numel, const float* S, const float* Y, const float* g_flat, int m,
                   DpnLbfgsState* state, double* scratch, double* G, void* stream);
int dpn_lbfgs_gtd(int n_tensors, float* const* params, const int64_t* numel, const float* a_flat, const float* b_flat, double* scratch,
                  double* out_dev, void* stream);
int dpn_lbfgs_direction(int n_tensors, float* const* params, const int64_t* numel, const float* S, const float* Y, const float* g_flat, int m,
                        DpnLbfgsState* state, const double* G, double* delta, float* d_flat, void* stream);

/* BASELINE configs[4] (OFF by default; `bench.py --encoder-fp8` / DPN_ENCODER_FP8=mx routes the encoder layers' forward GEMMs here): C[M][N] =
 * epilogue(A[M][K] . W[N][K]^T + bias[N]) on the block-scaled (MX) fp8 instruction v_mfma_scale_f32_32x32x64_f8f6f4: OCP e4m3 operands quantised in
 * the kernel, one E8M0 power-of-two scale per 32 consecutive k of a row (OCP MX) applied by the hardware, fp32 accumulate; K % 64 == 0; epi =
 * DPN_EPI_NONE or DPN_EPI_GELU (aux_out receives the pre-activation).  Replaces nothing of the reference by default: its measured parity error is why
 * (profiles/round3_fp8_mx_encoder.json).  (The non-scaled fp8 form with per-row scales is a shelved experiment: dpn_hip_experiments.h.) */
int dpn_gemm_fp8_mx(int M, int N, int K, const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int epi,
                 float* aux_out, void* stream);

/* Self-test of the MFMA fragment-layout assumptions in dpn_layout.h (A = I against an asymmetric B). Returns 0 if they hold. */
int dpn_selftest(void* scratch_dev /* >= 64 KiB */, void* stream);

/* Residual-weighted interior collocation points (csrc/dpn_adaptive.hip): m candidates -- a pool of uniform interior draws -- are scored by their PDE
 * residuals and n points are drawn from them, with replacement, with probability p_i ~ w_i = s_i^k / mean_j(s_j^k) + c  (residual-based adaptive
 * sampling; k = c = 1 are the usual defaults).  fp64 throughout, no atomics, every sum in one fixed order: two runs agree bitwise.
 * scratch: dpn_adaptive_scratch_doubles(m) doubles on the device (0 for an m that is not supported: m <= 0 or m > 2^20), shared by both calls;
 * after dpn_adaptive_select its first m doubles hold the inclusive prefix sum of the weights.
 *
 * dpn_adaptive_scores: res[m][6] = dpn_residual_points' rows, factors = six HOST doubles (the loss factors in the order of the residuals);
 *   score[i] = sum_e factors[e] * res[i][e]^2, every product and sum rounded once in fp64, e ascending; a score that is not finite is written as 0
 *   and counted.  stats[3] (device): sum_i score_i^k, the count of non-finite scores, max_i score_i.
 * dpn_adaptive_select: score[m] (negative or non-finite entries count as 0), then
 *   w_i = score_i^k / mean(score^k) + c; all w_i = 1 when the mean is 0 (or not finite); cdf = inclusive prefix sum of w (block-local scans, a scan of
 *   the block totals, a final pass), total = cdf[m - 1];
 *   u_j = the 53-bit uniform of Philox-4x32-10, key = seed, counter = offset + *step_dev * stride + j (step_dev NULL: offset + j), stream id 2 -- the
 *   same counters as points offset .. of dpn_sample_points_replay, whose own draws use stream ids 0 and 1;
 *   idx_j = the smallest i with cdf[i] > u_j * total (a product that rounds up to total is taken as the last double below it), so an entry with w_i = 0 is
 *   never drawn;  out row j = row idx_j of x, y, t, f [m], coord_data [m][6].  idx [n], u [n], picked_score [n] (= score[idx_j]) may be NULL.
 * -1: m <= 0, m > 2^20, n <= 0, a NULL required pointer, k or c negative or not finite. */
int64_t dpn_adaptive_scratch_doubles(int64_t m);
int dpn_adaptive_scores(const float* res, int64_t m, const double* factors, double k, double* score, double* stats, double* scratch, void* stream);
int dpn_adaptive_select(const double* score, int64_t m, double k, double c, const float* x, const float* y, const float* t, const float* f,
                        const float* coord_data, int64_t n, uint64_t seed, uint64_t offset, const int32_t* step_dev, uint64_t stride,
                        float* out_x, float* out_y, float* out_t, float* out_f, float* out_coord_data, int32_t* idx, double* u, double* picked_score,
                        double* scratch, void* stream);

/* Per-point weights and causal time weighting of the PDE losses (bins and weights: csrc/dpn_causal.hip; dpn_residual_weighted: csrc/dpn_residual.hip,
 * dpn_residual's kernel instantiated with the weights).  A weight per collocation point multiplies the point's
 * criterion value and its cotangent; causal training (Wang, Sankaran & Perdikaris 2022) derives it from the point's time bin:
 * W_k = exp(-eps * sum_{j<k} l_j), l_j the mean point loss of bin j.  fp64 wherever a result is defined, no atomics, every sum in one fixed order:
 * two runs agree bitwise.  Weights are constants of the loss: no cotangent is formed for them.
 *
 * dpn_causal_bins: out_n, jac_n, f, geo, phys as dpn_residual; t [n] the points' times (fp32, the forward kernel's t); factors = six HOST doubles
 *   (the loss factors in the order of the residuals; phys->factor is not read).  Per point
 *     s_i = sum_e factors[e] * rho(r_ie), e ascending, every product and sum rounded once in fp64; rho = (double)r * (double)r for MSE, else the
 *           fp32 criterion value cast up (what dpn_residual sums);
 *     b_i = clamp(floor(((double)t_i - t_lo) * n_bins / (t_hi - t_lo)), 0, n_bins - 1), each operation rounded once in fp64 (t_hi - t_lo formed on the
 *           host); a NaN goes to bin 0.
 *   bin [n] int32 = b_i;  rows [ceil(n / 256)][n_bins][2] fp64 (dpn_causal_rows_doubles(n, n_bins) doubles; 0 for unsupported arguments): per block and
 *   bin the sum of s_i in point order and the count.
 *   -1: n <= 0, n_bins outside 1..DPN_CAUSAL_MAX_BINS, t_hi <= t_lo, a bound that is not finite, a NULL pointer, a criterion dpn_residual rejects.
 * dpn_causal_weights (one workgroup): the block rows of bin k are added in a fixed order (blocks q, q + 4, ... for q = 0..3, then ((p0 + p1) + p2) + p3);
 *   l_k = sum_k / count_k, 0 for an empty bin.  relative != 0: l_k is divided by the mean of l over the non-empty bins (added k ascending); when that
 *   mean is not finite or not > 0 every W_k = 1.  cum_k = the sequential exclusive prefix sum of l (normalised if relative); W_k = exp(-eps * cum_k).
 *   W32 [n_bins] fp32 = (float)W_k, what dpn_residual_weighted reads;  diag [3 n_bins + 2] fp64 = W [n_bins] | l [n_bins], un-normalised |
 *   count [n_bins] | min_k W_k | the normaliser (1 when relative == 0).
 *   -1: a NULL pointer, n <= 0, n_bins outside 1..DPN_CAUSAL_MAX_BINS, eps negative or not finite.
 * dpn_residual_weighted: dpn_residual with the point weight wt_i = w[i] * bin_w[bin[i]] (w [n] fp32 or NULL = 1; bin [n] int32 with bin_w, both or
 *   neither, bin[i] an index into bin_w as dpn_causal_bins writes it; neither w nor bin: -1).  wt_i multiplies the point's criterion value in the fp64
 *   block sums (as a double, before the wave tree) and the point's cotangents g_out, g_jxi (multiplied into the fp32 factor 1 / n of d loss_e / d r_e).  loss_sums has
 *   dpn_residual's layout: dpn_residual_finish(_batch) finishes it, dividing by n -- not by the sum of the weights --, so the loss is linear in the
 *   weights and a weight of 1 is the plain mean.  With every wt_i == 1.0f, loss_sums, g_out and g_jxi are bitwise dpn_residual's. */
#define DPN_CAUSAL_MAX_BINS 64
int64_t dpn_causal_rows_doubles(int64_t n, int n_bins);
int dpn_causal_bins(const float* out_n, const float* jac_n, const float* f, const float* t, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys,
                    const double* factors, double t_lo, double t_hi, int n_bins, int32_t* bin, double* rows, void* stream);
int dpn_causal_weights(const double* rows, int64_t n, int n_bins, double eps, int relative, float* W32, double* diag, void* stream);
int dpn_residual_weighted(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnGeometry* geo, const DpnPhysics* phys,
                          const float* gl /*[6] or NULL*/, const float* gtot /*[1] or NULL*/, double* loss_sums, float* g_out, float* g_jxi,
                          const float* w, const int32_t* bin, const float* bin_w, void* stream);

/* Loss balancing by gradient norms (csrc/dpn_balance.hip).  Each of K loss terms carries a weight lambda_k (fp32, on
 * the device, read at run time); every few hundred steps it moves towards mean_j |grad L_j| / |grad L_k| (Wang, Teng & Perdikaris 2021; Wang,
 * Sankaran, Wang & Perdikaris 2023; the mean form: lambda = 1 when all norms are equal).  fp64 wherever a result is defined, no atomics, every sum in
 * one fixed order, no contraction: two runs agree bitwise.
 *
 * dpn_balance_sumsq: grads = a HOST table of n_tensors (1..DPN_BALANCE_MAX_TENSORS; 160 per launch, a longer table is cut into several) fp32 device pointers, numel their lengths (HOST, each 1 .. 2^31 - 2049); a NULL entry
 *   counts as zeros.  *sumsq_slot = sum of (double)x * (double)x (exact products): per 2048-element chunk of a tensor one fp64 partial (thread j of
 *   256 adds elements j, j + 256, ... in that order; wave tree; (w0 + w1) + (w2 + w3)), the partials added the same way by one workgroup.
 *   scratch: dpn_balance_scratch_doubles(n_tensors, numel) doubles (the number of chunks; 0 for a table that is not taken).  -1: such a table, a NULL
 *   table, scratch or slot.
 * dpn_balance_update (one workgroup, one thread; deepphysinet_amd/balance.py: update_reference restates it):
 *     n_k = sqrt(sumsq_k); term k is active when n_k is finite and > 0;
 *     fewer than two active terms, or a sumsq_k that is not finite: lambda is left as it is, flag = 1, mean = 0, every lambda-hat = 0;
 *     otherwise mean = (sum of n_k over the active k, k ascending) / (their number), lambda-hat_k = min(max(mean / n_k, lam_min), lam_max),
 *     lambda_k <- (float)(momentum * (double)lambda_k + (1 - momentum) * lambda-hat_k), every operation rounded once in fp64; an inactive term keeps
 *     its lambda (lambda-hat_k = 0 in diag).
 *   lambda [K] fp32 in / out;  diag [3 K + 2] fp64 = n [K] | lambda-hat [K] | the new lambda [K] | mean | flag.
 *   -1: a NULL pointer, K outside 1..DPN_BALANCE_MAX_TERMS, momentum outside [0, 1], not (0 < lam_min <= 1 <= lam_max, both finite).
 * dpn_balance_combine: terms = a HOST table of DPN_BALANCE_STEP_TERMS = 13 fp32 device scalars: the interior PDE terms [6], the margin PDE terms
 *   [6], the data loss; map = 13 HOST ints, the term's k (0..K - 1).  total (or NULL): *total = lambda_map(12) * data + sum over interior 0..5, then
 *   margin 0..5, of lambda_map(i) * term_i, fp32, in that order, every product and sum rounded once.  cot_out (or NULL; then cot_in [1] is read):
 *   cot_out[i] = *cot_in * lambda_map(i), i = 0..12.  One launch.  -1: neither output, cot_out without cot_in, total without terms (or with a NULL
 *   term), a map entry outside 0..K - 1, K outside 1..DPN_BALANCE_MAX_TERMS, a NULL map or lambda. */
#define DPN_BALANCE_MAX_TERMS 16
#define DPN_BALANCE_STEP_TERMS 13
#define DPN_BALANCE_MAX_TENSORS 4096
int64_t dpn_balance_scratch_doubles(int n_tensors, const int64_t* numel);
int dpn_balance_sumsq(int n_tensors, const float* const* grads, const int64_t* numel, double* scratch_dev, double* sumsq_slot_dev, void* stream);
int dpn_balance_update(const double* sumsq_dev, int K, double momentum, double lam_min, double lam_max, float* lambda_dev, double* diag_dev,
                       void* stream);
int dpn_balance_combine(const float* const* terms, int K, const int* map, const float* lambda_dev, const float* cot_in_dev, float* total_dev,
                        float* cot_out_dev, void* stream);

/* The step body for a lead batch (csrc/dpn_residual.hip): one residual pass per field, one finish launch for all fields.
 *
 * dpn_step_residual: out_n [n][6], jac_n [n][6][3], f [n] of ONE field, the first n_inter rows interior, the other n_m = n - n_inter margin points with
 *   labels [n_m][6].  One launch of blocks(n_inter) + blocks(n_m) workgroups of 256 (blocks(k) = ceil(k / 256)): the first blocks(n_inter) hold the
 *   interior points, the others the margin points from row n_inter on, so a workgroup holds exactly the points that a block of dpn_residual on that
 *   group's slice holds.  rows [blocks][7] fp64 (dpn_step_rows_doubles(n_inter, n) doubles; 0 for n_inter < 1 or n_inter >= n), written, not
 *   accumulated: [0:6] the six criterion sums, bitwise dpn_residual's block rows of the group's slice; [6] the sum of SmoothL1(beta) over the block's
 *   margin points x 6 variables (the fp32 values of dpn_smooth_l1 cast up; elements of a point in order, wave tree, waves in order), 0.0 from an
 *   interior block.  With g_out [n][6] and g_jxi [n][6][3] (both or neither) the same pass writes d total / d (out_n, J_xi) for the cotangent gtot[0]
 *   of the field's total = data loss + interior PDE total + margin PDE total: the PDE part bitwise dpn_residual(gl = NULL, gtot) per group (1 / n of
 *   the point's own group; phys->reduce_sum honoured), and on margin rows + data_scale * gtot[0] * dSmoothL1, added behind it in one rounded addition
 *   (what dpn_smooth_l1(scale = data_scale, accumulate = 1, scale_dev = gtot) adds).  No atomics.
 *   -1 (nothing launched, nothing written): a NULL out_n, jac_n, f, labels, geo, phys, gtot or rows; n_inter < 1; n_inter >= n; g_out without g_jxi; a
 *   criterion dpn_residual rejects; beta <= 0.
 * dpn_step_finish_batch: rows of n_fields fields side by side (stride dpn_step_rows_doubles) -> losses [n_fields][16] fp32, one workgroup per field:
 *   [0:6] the interior terms, [6] their total, [7:13] the margin terms, [13] their total -- bitwise dpn_residual_finish on each group's rows --,
 *   [14] the data loss (float)(S / (6 n_m)) * margin_factor, S = column 6 of the margin rows added in fp64 in a fixed order, [15] the field's total
 *   ([14] + [6]) + [13] in fp32.  -1: a NULL pointer, n_inter < 1, n_inter >= n, n_fields < 1. */
int64_t dpn_step_rows_doubles(int64_t n_inter, int64_t n);
int dpn_step_residual(const float* out_n, const float* jac_n, const float* f, const float* labels /* [n - n_inter][6] */, int64_t n_inter, int64_t n,
                      const DpnGeometry* geo, const DpnPhysics* phys, float beta, float data_scale, const float* gtot /* [1] device */, double* rows,
                      float* g_out, float* g_jxi, void* stream);
int dpn_step_finish_batch(const double* rows, int64_t n_inter, int64_t n, int n_fields, const DpnPhysics* phys, float margin_factor,
                          float* losses /* [n_fields][16] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
