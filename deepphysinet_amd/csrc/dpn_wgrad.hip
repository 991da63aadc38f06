// MI355X (gfx950 / CDNA4) point path, the weight side: packing the hyper-network's weights for the point kernels (dpn_point.hip) and reducing their
// per-point operands to the weight gradients.  DESIGN.md section 3 derives the algorithm (rank-1 fc.2, single-GEMM weight gradients).
//
// Kernel inventory
//   dpn_pack_*          fp32 weights -> MFMA-fragment-ordered bf16 (hi/lo) + permuted vectors
//   dpn_wgrad_kernel    points-reduction GEMMs (split over point ranges)
//   dpn_finish_*        split reduction, un-permutation, rank-1 fc.2 gradients
//   dpn_selftest_kernel, dpn_clock_stamp_kernel    the MFMA layout self-test; a device-clock stamp as a graph node (measurements)
// No kernel of the training step in this file uses atomics: every reduction is fixed-order, the whole step is bitwise reproducible.  (The one atomicAdd
// is dpn_clock_stamp_kernel's ring cursor, a measurement aid.)
//
// Built WITHOUT -amdgpu-mfma-vgpr-form: dpn_wgrad_kernel measures slower with its accumulators in VGPRs (dpn_point.hip).
#include <type_traits>

#include "dpn_point_common.h"

DEV u16 f2bf(float x) {                       // round-to-nearest-even, finite inputs (pack kernels)
    unsigned u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (u16)(u >> 16);
}
DEV float bf2f(u16 b) { return __uint_as_float(((unsigned)b) << 16); }

// ------------------------------------------------------------------------------------------------ weight packing
struct PackArgs {
    DpnNetPtrs net[kNets];
    char* packed;
    int ns;
    int form;              // 0: the seven-GEMM stream (ring kernels), 1: the fused five-GEMM stream (dpn_fwd_tiles_kernel; dpn_layout.h)
    // a batch of fields in ONE launch (grid.y = kNets * n_fields): field f reads the hyper-network outputs of field 0 moved by f * heads_stride /
    // f * evec_stride floats (w1b1, w2b2 | evec; the static tensors are shared) and writes its packed block at packed + f * packed_stride bytes
    int n_fields;
    long heads_stride, evec_stride, packed_stride;
};
// the pointer table of (net, field): wave-uniform scalar arithmetic on a copy of the kernel argument
DEV DpnNetPtrs pack_net(const PackArgs& a, const int net, const int field) {
    DpnNetPtrs P = a.net[net];
    P.w1b1 += field * a.heads_stride;
    P.w2b2 += field * a.heads_stride;
    P.evec += field * a.evec_stride;
    return P;
}

DEV float pack_src(const DpnNetPtrs& P, int kb, int lane, int e) {
    const int i = lane & 31, h = lane >> 5;
    if (kb < kS1) {                                   // S0: w1, rows o, K = PE3 slots
        const int T = kb / 12, ks = kb % 12;
        return P.w1b1[(32 * T + i) * P.ld_w1b1 + pe3_ch(ks, h, e)];
    } else if (kb >= kS5) {                           // S5: w1^T rows rho (PE slots), K over o
        const int rel = kb - kS5, T = rel / 16, ks = rel % 16;
        return P.w1b1[chain_ch(ks, h, e) * P.ld_w1b1 + gpe_row_to_pe3_ch(32 * T + i)];
    }
    if (kb < kS2) {                                   // S1: w2 (8 tiles x 16 k-steps), then Wd (8 tiles x 12 k-steps)
        const int rel = kb - kS1;
        if (rel < 128) return P.w2b2[(32 * (rel / 16) + i) * P.ld_w2b2 + chain_ch(rel % 16, h, e)];
        const int r2 = rel - 128;
        return P.Wd[(32 * (r2 / 12) + i) * kPe + pe6_ch(r2 % 12, h, e)];
    } else if (kb < kS3) {                            // S2: W1 rows o
        const int rel = kb - kS2, T = rel / 16, ks = rel % 16;
        return P.W1[(32 * T + i) * kHidden + chain_ch(ks, h, e)];
    } else if (kb < kS4) {                            // S3: W1^T rows i, K over o
        const int rel = kb - kS3, T = rel / 16, ks = rel % 16;
        return P.W1[chain_ch(ks, h, e) * kHidden + (32 * T + i)];
    } else {                                          // S4: w2^T rows i, K over o
        const int rel = kb - kS4, T = rel / 16, ks = rel % 16;
        return P.w2b2[chain_ch(ks, h, e) * P.ld_w2b2 + (32 * T + i)];
    }
}

// vectors in [h][T][r] order (channel 32T + drow32(r,h)); u = W2^T wo; const0 = wo.bf2 + bo
// form 1 (dpn_layout.h): C2 = W1 cvec + bf1, A2 = w2^T wo, Bv = Wd^T wo (PE6 slot order), const0 += 2 wo.cvec
// EIGHT blocks per net (part = 0..7): block `part` owns the 32 vector entries idx = 32 part .. 32 part + 31; its 256 threads are 8 groups of 32, group og
// sums the reduction index o over [32 og, 32 og + 32) and the eight partial sums are joined in a fixed order through LDS.  (One block per net walking
// 256-long chains of dependent loads -- three of them in the fused form -- was the long pole of the launch: 31-40 us.)
constexpr int kVecParts = 8;
DEV void pack_vectors(const PackArgs& a, const DpnNetPtrs& P, char* packed_net, const int part) {      // packed_net: this (field, net)'s packed block
    float* vec = reinterpret_cast<float*>(packed_net + (long)kPackKB * 1024 * a.ns);
    const int tid = threadIdx.x, og = tid >> 5;
    const int idx = 32 * part + (tid & 31);
    const int h = idx >> 7, T = (idx >> 4) & 7, r = idx & 15;
    const int ch = 32 * T + drow32(r, h);
    const int c6 = idx < kPe ? pe6_ch(idx >> 4, (idx >> 3) & 1, idx & 7) : 0;                // Bv: idx = PE6 slot 16 ks + 8 h + e (idx < 192)
    __shared__ float red[3][8][32];
    float up = 0.f, a2 = 0.f, bv = 0.f;
    if (a.form == 1) {
#pragma unroll 8
        for (int o = 32 * og; o < 32 * og + 32; ++o) {
            const float w = P.wo[o];
            up = fmaf(w, P.W2[o * kHidden + ch], up);
            a2 = fmaf(w, P.w2b2[o * P.ld_w2b2 + ch], a2);                                    // (w2^T wo)[ch]
            bv = fmaf(w, P.Wd[o * kPe + c6], bv);                                            // (Wd^T wo)[pe6 channel of this slot]
        }
    } else {
#pragma unroll 8
        for (int o = 32 * og; o < 32 * og + 32; ++o) up = fmaf(P.wo[o], P.W2[o * kHidden + ch], up);
    }
    red[0][og][tid & 31] = up; red[1][og][tid & 31] = a2; red[2][og][tid & 31] = bv;
    __syncthreads();
    if (og == 0) {
        const int c = tid;
        auto sum8 = [&](const int q) { return ((red[q][0][c] + red[q][1][c]) + (red[q][2][c] + red[q][3][c])) + ((red[q][4][c] + red[q][5][c]) + (red[q][6][c] + red[q][7][c])); };
        vec[kVecB1 * 256 + idx] = P.w1b1[ch * P.ld_w1b1 + kPe];
        vec[kVecU * 256 + idx] = sum8(0);
        vec[kVecWo * 256 + idx] = P.wo[ch];
        if (a.form == 1) {
            // (C2 = W1 cvec + bf1 is written by the fused kernel's own tile role: it needs a pass over W1, i.e. the matrix cores)
            vec[kVecA2 * 256 + idx] = sum8(1);
            vec[kVecBv * 256 + idx] = idx < kPe ? sum8(2) : 0.f;
        } else {
            vec[kVecCvec * 256 + idx] = P.w2b2[ch * P.ld_w2b2 + kHidden] + P.bd[ch] + P.evec[ch];
            vec[kVecBf1 * 256 + idx] = P.bf1[ch];
            vec[kVecB2BdE_unused * 256 + idx] = 0.f;
        }
    }
    if (part != 0) return;
    // const0 = wo . (bf2 [+ 2 cvec]) + bo: block 0 of the net, all 256 threads
    __shared__ float red1[256];
    const float cv_nat = P.w2b2[tid * P.ld_w2b2 + kHidden] + P.bd[tid] + P.evec[tid];        // cvec[tid], natural order
    red1[tid] = P.wo[tid] * (P.bf2[tid] + (a.form == 1 ? 2.0f * cv_nat : 0.f));
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red1[tid] += red1[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        vec[kNumVecs * 256 + 0] = red1[0] + P.bo[0];
        vec[kNumVecs * 256 + 1] = (float)a.form; vec[kNumVecs * 256 + 2] = 0.f; vec[kNumVecs * 256 + 3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void dpn_pack_matrices_kernel(PackArgs a) {
    const int mcols = gridDim.x - kVecParts;                                          // block columns of matrix fragments, then kVecParts of vector blocks
    const int field = blockIdx.y / kNets, net = blockIdx.y - field * kNets;
    const int ns = a.ns;
    const DpnNetPtrs P = pack_net(a, net, field);
    char* packed_net = a.packed + field * a.packed_stride + (long)net * pack_bytes_per_net(ns);
    if ((int)blockIdx.x >= mcols) { pack_vectors(a, P, packed_net, blockIdx.x - mcols); return; }
    uint4* dst = reinterpret_cast<uint4*>(packed_net);
    const int total = kPackKB * 64;                   // (kb, lane) pairs (form 0; the fused form has its own kernel, dpn_pack_fused_kernel)
    for (int u = blockIdx.x * 256 + threadIdx.x; u < total; u += mcols * 256) {
        const int kb = u >> 6;
        const int lane = u & 63;
        u16 hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = pack_src(P, kb, lane, e);
            hi[e] = f2bf(x);
            lo[e] = f2bf(x - bf2f(hi[e]));
        }
        uint4 w;
        w.x = hi[0] | (hi[1] << 16); w.y = hi[2] | (hi[3] << 16); w.z = hi[4] | (hi[5] << 16); w.w = hi[6] | (hi[7] << 16);
        dst[(kb * ns) * 64 + lane] = w;
        if (ns == 2) {
            w.x = lo[0] | (lo[1] << 16); w.y = lo[2] | (lo[3] << 16); w.z = lo[4] | (lo[5] << 16); w.w = lo[6] | (lo[7] << 16);
            dst[(kb * ns + 1) * 64 + lane] = w;
        }
    }
}

// ------------------------------------------------------------------------------------------------ fused form: products + packing in ONE launch
// A = W1 w2, B = W1 Wd (and C2 = W1 cvec + bf1) on the exact-fp32 matrix instruction, each 32 x 32 result tile split hi / lo and written straight into
// the fragment stream (A: rows o AND, transposed, rows j; B: rows o over PE6 slots) -- no fp32 scratch, no second launch (rounds before: a 24-problem
// dpn_sgemm_batch launch + dpn_pack_matrices_kernel, 17 + 10 us on the chain between the hyper-network heads and the forward kernel).
// Block roles per net (blockIdx.x): [0, 64) tiles of A | [64, 112) tiles of B (columns in PE6 SLOT order) | [112, 120) C2 | [120, 132) the w1 / w1^T
// fragments | [132, 140) the vector blocks (pack_vectors).
constexpr int kFusedBlocks = 64 + 48 + 8 + 12 + kVecParts;
DEV f32x16 pk_mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__global__ __launch_bounds__(256) void dpn_pack_fused_kernel(PackArgs a) {
    // Workgroups go to the eight XCDs round-robin in dispatch order: every XCD gets a CONTIGUOUS range of the (net, block) list, so that a net's W1 / w2 / Wd
    // are fetched into one or two L2s instead of all eight: 20.0 -> 16.2 us per launch (tools/pack_probe.py, profiles/round6_xcd_contiguous.txt).
#ifdef PACK_NO_XCD_REMAP
    const int field = blockIdx.y / kNets, net = blockIdx.y - field * kNets, bx = blockIdx.x, ns = a.ns;
#else
    // (a batch of fields: grid.y = kNets * n_fields, the list is (field, net, block): an XCD then works on whole fields)
    const int lin = blockIdx.x + kFusedBlocks * blockIdx.y, virt = (lin & 7) * (kFusedBlocks * kNets / 8 * a.n_fields) + (lin >> 3);
    static_assert(kFusedBlocks * kNets % 8 == 0, "remap");
    const int fnet = virt / kFusedBlocks, bx = virt - fnet * kFusedBlocks, ns = a.ns, field = fnet / kNets, net = fnet - field * kNets;
#endif
#ifdef PACK_ABL_MASK        // ablation builds (wrong results on purpose, timing only: tools/variant_build.py --unit=1 -DPACK_ABL_MASK=m): only the roles in bit mask m run.
    // Round 6, tools/pack_probe.py (us per launch): all 19.9-20.2; role 0 alone 7.7, 1: 6.5, 2: 8.0, 3: 5.7, 4: 5.1; {0,1} 12.1, {0,1,2} 17.7, {3,4} 6.9, {0,1,3,4} 16.8:
    // the three MFMA-tile roles do not hide behind each other.  Staging the block's W1 rows through LDS with coalesced loads (each lane fetches 16-byte pieces
    // of its own row today) was built and changed nothing (21.1-21.9 us): it is not the request pattern.  profiles/round6_pack_fused_roles.txt
    if (!((PACK_ABL_MASK >> (bx < 64 ? 0 : bx < 112 ? 1 : bx < 120 ? 2 : bx < 132 ? 3 : 4)) & 1)) return;
#endif
    const DpnNetPtrs P = pack_net(a, net, field);
    char* packed_net = a.packed + field * a.packed_stride + (long)net * pack_bytes_per_net(ns);
    if (bx >= 132) { pack_vectors(a, P, packed_net, bx - 132); return; }
    uint4* dst = reinterpret_cast<uint4*>(packed_net);
    auto put = [&](const int kb, const int lane, const float (&x)[8]) __attribute__((always_inline)) {
        u16 hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { hi[e] = f2bf(x[e]); lo[e] = f2bf(x[e] - bf2f(hi[e])); }
        uint4 w;
        w.x = hi[0] | (hi[1] << 16); w.y = hi[2] | (hi[3] << 16); w.z = hi[4] | (hi[5] << 16); w.w = hi[6] | (hi[7] << 16);
        dst[(kb * ns) * 64 + lane] = w;
        if (ns == 2) {
            w.x = lo[0] | (lo[1] << 16); w.y = lo[2] | (lo[3] << 16); w.z = lo[4] | (lo[5] << 16); w.w = lo[6] | (lo[7] << 16);
            dst[(kb * ns + 1) * 64 + lane] = w;
        }
    };
    if (bx >= 120) {                                          // w1 (kS0 .. kS1) and w1^T (kS5 .. kPackKB): 192 (kb) x 64 lanes over 12 blocks
        for (int u = (bx - 120) * 256 + threadIdx.x; u < 192 * 64; u += 12 * 256) {
            int kb = u >> 6;
            const int lane = u & 63;
            if (kb >= kS1) kb += kS5 - kS1;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = pack_src(P, kb, lane, e);
            put(kb, lane, x);
        }
        return;
    }
    // ---- a 32 x 32 tile of W1 . R, R = w2 (role 0), Wd with its columns in PE6 slot order (role 1), cvec as a single column (role 2)
    const int role = bx < 64 ? 0 : bx < 112 ? 1 : 2;
    const int rb = role == 0 ? bx : role == 1 ? bx - 64 : bx - 112;
    const int To = rb & 7, Tc = role == 2 ? 0 : rb >> 3;      // row tile (o), column tile (j / slot)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    __shared__ float red[4][16][64];
    __shared__ float tile[32][33];
    const float* W1r = P.W1 + (32 * To + col) * kHidden;
    int ccol = 0;                                             // this lane's column of R
    if (role == 0) ccol = 32 * Tc + col;
    else if (role == 1) { const int sl = 32 * Tc + col; ccol = pe6_ch(sl >> 4, (sl >> 3) & 1, sl & 7); }
    f32x16 acc = (f32x16)0.f;
    float av[32], bv[32];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k0 = 64 * wv + 8 * m + 4 * kh;
        const f32x4 q = *reinterpret_cast<const f32x4*>(W1r + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + e;
            av[4 * m + e] = q[e];
            if (role == 0) bv[4 * m + e] = P.w2b2[(long)k * P.ld_w2b2 + ccol];
            else if (role == 1) bv[4 * m + e] = P.Wd[k * kPe + ccol];
            else bv[4 * m + e] = col == 0 ? (P.w2b2[(long)k * P.ld_w2b2 + kHidden] + P.bd[k] + P.evec[k]) : 0.f;
        }
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = pk_mfma_f32(av[kk], bv[kk], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wv][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = wv + 4 * q;                                         // element (r, lane) of the tile: row drow32(r, kh), column col
        tile[drow32(r, kh)][col] = (red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]);
    }
    __syncthreads();
    if (role == 2) {                                                      // C2[o] = (W1 cvec)[o] + bf1[o], in the vectors' [h][T][r] order
        if (threadIdx.x < 32) {
            const int o = 32 * To + threadIdx.x, w_ = o & 31;
            float* vec = reinterpret_cast<float*>(packed_net + (long)kPackKB * 1024 * ns);
            vec[kVecC2 * 256 + ((w_ >> 2) & 1) * 128 + (o >> 5) * 16 + (w_ & 3) + 4 * (w_ >> 3)] = tile[threadIdx.x][0] + P.bf1[o];
        }
        return;
    }
    // ---- the tile as fragments: thread = (form, k-step of the tile's pair, lane)
    const int form = threadIdx.x >> 7, ksl = (threadIdx.x >> 6) & 1, i = lane & 31, h = lane >> 5;
    float x[8];
    if (role == 1) {
        if (form == 1) return;
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = tile[i][16 * ksl + 8 * h + e];                       // PE6 slot (h, e) of k-step 2 Tc + ksl
        put(kFB + To * 12 + 2 * Tc + ksl, lane, x);
    } else if (form == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = tile[i][16 * ksl + 8 * (e >> 2) + 4 * h + (e & 3)];  // A rows o, K = chain(h1): column j = chain_ch(ks, h, e)
        put(kFA + To * 16 + 2 * Tc + ksl, lane, x);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = tile[16 * ksl + 8 * (e >> 2) + 4 * h + (e & 3)][i];  // A^T rows j, K = chain(t2): row o = chain_ch(ks, h, e)
        put(kFAT + Tc * 16 + 2 * To + ksl, lane, x);
    }
}

// ------------------------------------------------------------------------------------------------ backward, stage 2
// Points-reduction GEMMs  D[so][si] = sum_pt X[pt][so] * Y[pt][si]  for the four products of a net:
//   P0: G    = M2^T Z    (256x256)  + mvec = M2^T g, q  = Z^T 1
//   P1: S1   = M2^T Z1   (256x256)  + mv1  = M2^T g, q1 = Z1^T 1, sum g      dw2 = W1^T diag(u) S1 + 2 wo (x) q1   (dpn_finish_vside_fc2_kernel;
//   P2: S2   = M2^T G6   (256x192)  +                q6 = G6^T 1             dWd = W1^T diag(u) S2 + 2 wo (x) q6    v is affine in m2: SavedView)
//   P3: dw1  = T1^T Z0   (256x192)  + db1 = T1^T g
// grid = (sum of the four products' point-range counts, 6 nets): each workgroup owns the whole output of its product for its range of
// 32-point tiles (SplitPlan below says how many ranges each product is cut into) and writes one partial sum per range;
// dpn_finish_* add the ranges in a fixed order.  Operands are already MFMA fragments in global memory (K-layout, written by
// dpn_fwd / dpn_bwd_points), so a tile travels global -> LDS as a plain byte image.
constexpr int kPartFloats = 65536 + 49152 * 2 + 7 * 256;           // per (split, net)
DPN_HD int part_off(int prod) { return prod == 1 ? 0 : prod == 2 ? 65536 : 114688; }
constexpr int kPartVec = 163840;                                    // -, -, mv1, db1, [sum g], q1, q6 (slots 0, 1 were product 0's mvec, q)

struct WgradArgs {
    int64_t n, n_pad;
    int splits[4];          // point ranges per product (SplitPlan)
    void* saved;
    void* operands;
    float* partials;
#ifdef DPN_WGRAD_PHASES
    unsigned* phases;       // experiment build: [net][workgroup][8 waves][8]: cycles in wait / barrier / issue / compute, tiles
#endif
};
#ifdef DPN_WGRAD_PHASES
#define DPN_WG_CLOCK(V) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); V = (u32)t_; } while (0)
#else
#define DPN_WG_CLOCK(V) do { } while (0)
#endif

// one workgroup = 8 waves (2 x 4): wave (wm, wn) owns rows 128wm.. and columns 64wn.. of the product.  The X and Y fragments
// of each 32-point tile are moved global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KB per wave-instruction, no staging
// registers) into a ring of RING slots, RING-1 tiles ahead; every operand byte is fetched from HBM exactly once per product.
// Synchronisation per tile: counted s_waitcnt vmcnt (this wave's pieces of the tile have landed) + one raw s_barrier (all
// pieces have landed AND everybody is done with the slot that is refilled next).
//
// The body is compiled once per product (WgradShape): the slot holds exactly that product's planes -- X: one plane for the 0/1 mask,
// NS for T1; Y: NS planes of 8 or 6 column tiles -- so every wave issues the same number of 1-KB pieces per tile without dummy loads
// (48 / 48 / 40 / 56 pieces in the hi+lo mode: 6 / 6 / 5 / 7 per wave), and the ring is as deep as 160 KB of LDS allow for THAT slot:
// three slots for the mask products in the hi+lo mode where the common 66-KB slot allowed two.  The kernel's time per tile is the
// latency of a tile's loads under load, not its bytes (measured: halving a product's bytes with the ring depth unchanged changed
// nothing), so the number of tiles in flight is what counts.
template <int NS, int PROD>
struct WgradShape {
    static constexpr int nct = PROD < 2 ? 8 : 6;                        // column tiles of Y (Z, Z1: 256 columns; G6, Z0: 192)
    static constexpr int nsx = PROD == 3 ? NS : 1;                      // planes of X (the mask has no lo part)
    static constexpr int kX = nsx * 16384, kYPlane = nct * 2048, kY = NS * kYPlane;
    static constexpr int kPieces = (kX + kY) / 1024;
    static constexpr int kIssue = (kPieces + 7) / 8;                    // 1-KB pieces per wave per tile; if they do not divide (single bf16, 192 columns:
    static constexpr int kPad = kIssue * 8 - kPieces;                   // 28 pieces), the last waves re-read one fixed kilobyte into a dummy area
    static constexpr int kGOff = kX + kY;                               // 8 per-wave copies of g[64]
    static constexpr int kPadOff = kGOff + 8 * 256;
    static constexpr int kSlot = kPadOff + (kPad ? 1024 : 0);
    static constexpr int PER_TILE = kIssue + 1;                         // DMA instructions per wave per tile
    static constexpr int RING = (160 * 1024) / kSlot < 5 ? (160 * 1024) / kSlot : 5;
};
template <int NS>
constexpr int wgrad_lds_bytes() {
    int m = 0;
    const int v[3] = {WgradShape<NS, 1>::RING * WgradShape<NS, 1>::kSlot, WgradShape<NS, 2>::RING * WgradShape<NS, 2>::kSlot,
                      WgradShape<NS, 3>::RING * WgradShape<NS, 3>::kSlot};
    for (int k = 0; k < 3; ++k) m = v[k] > m ? v[k] : m;
    return m;
}

// TAB: product 3 with Z0 in the table form (OperandView): the Y image is the per-point fp32 pe3 table and Z0 is formed from it in LDS, as product 2 forms G6
template <int NS, int PROD, bool TAB = false>
DEV void wgrad_body(const WgradArgs& a, char* lds, const int split, const int net) {
    static_assert(!TAB || (NS == 2 && PROD == 3), "the table form of Z0: hi+lo mode, product 3");
    using S = WgradShape<NS, PROD>;
    constexpr int nct = S::nct, nsx = S::nsx, kSlot = S::kSlot, RING = S::RING, PER_TILE = S::PER_TILE, ncol = nct * 32;
    const int64_t tiles = a.n_pad / 32;
    const int64_t per = (tiles + a.splits[PROD] - 1) / a.splits[PROD];
    const int64_t t0 = (int64_t)split * per;
    int64_t t1 = t0 + per < tiles ? t0 + per : tiles;
    if (t1 < t0) t1 = t0;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // wave tile: 256-column products (P1) 2 x 4 waves of 128 rows x 64 columns (4 x 2 MFMA tiles); 192-column products (P2, P3) 4 x 2 waves of 64 rows x
    // 96 columns (2 x 3 tiles).  Until the end of round 5 the 192-column products kept the 2 x 4 arrangement with the wn = 3 waves idle: six waves with
    // eight tiles each on THREE SIMDs (wave w runs on SIMD w % 4) -- tools/wgrad_phase_probe.py showed the multiply phase of the wm = 1 waves at 4 200
    // cycles per tile against 2 550 for their SIMD partners and SIMD 3 idle.  Eight waves with six tiles each: 12 tile-products per SIMD instead of 16.
#ifdef DPN_WGRAD_2X4_ONLY                                                   // A/B build (tools/variant_build.py wg2x4 --unit=1 -DDPN_WGRAD_2X4_ONLY): the former arrangement
    constexpr bool kWide = true;
#else
    constexpr bool kWide = nct == 8;
#endif
    constexpr int MT = kWide ? 4 : 2, NT = kWide ? 2 : 3;
    const int wm = kWide ? wave >> 2 : wave >> 1, wn = kWide ? wave & 3 : wave & 1;
    const int i = lane & 31, h = lane >> 5;
    const bool active = wn * NT < nct;                                  // (always true but in the A/B build, whose wn = 3 waves have no columns at 192)
    SavedView sv = saved_view(a.saved, a.n_pad, NS);
    OperandView ov = operand_view(a.operands, a.n_pad, NS);
    const char* xb = (PROD == 3) ? sv.T1.base : sv.M2.base;                                      // 8 column tiles
    static_assert(PROD >= 1 && PROD <= 3, "products: 1 = M2^T Z1, 2 = M2^T G6, 3 = T1^T Z0");
    const char* yb = (PROD == 1) ? ov.Z1.base : (PROD == 2) ? ov.PE6.base : ov.Z0.base;   // nct column tiles; product 2: the per-point TABLE (no net index)
    const int64_t ynet = (PROD == 2 || TAB) ? 0 : net;
    const float* gnet = ov.gnet + (int64_t)net * a.n_pad;
    // the per-tile copy of g is a 64-lane, 4-byte DMA of which the tile's 32 points use lanes 0..31; in the table form lanes 32..63 fetch gJ_c, c the
    // coordinate of this wave's column tile (dpn_layout.h): g at bytes 0..127 of the wave's copy, gJ_c at 128..255
    const char* gsrc = reinterpret_cast<const char*>(gnet) + lane * 4;
    float fr = 0.f;                                                     // table form: the frequency of this lane's column (both of the wave's pairs)
    if constexpr (TAB) {
        const int ct = wgrad_z0_ct(wave);
        if (lane >= 32) gsrc = reinterpret_cast<const char*>(ov.gj + ((int64_t)net * 3 + (ct >> 1)) * a.n_pad) + (lane - 32) * 4;
        fr = __uint_as_float(ov.hdr[4 + z0_freq_index(ct, lane & 31)]);
        asm volatile("" : "+v"(fr));                                    // the load is waited for HERE, in front of the first DMA (not by a vmcnt(0) in the tile loop)
    }

    // every wave issues PER_TILE DMA instructions per tile: piece q = wave + 8*j of the (X planes, Y planes) image, + its own g copy.
    // (Letting only the four waves with wm == tile & 1 issue a tile -- twice the pieces each, in the shadow of their SIMD partners'
    //  MFMAs -- was measured: the issue phase shrinks from 1 900 to 1 100 cycles per tile and the barrier wait grows by as much,
    //  360 us against 364 us in the hi+lo mode.  Not kept.)
    // piece q = wave + 8 j of the slot image: where it comes from (address of tile 0, bytes per tile) and where it goes -- worked out once,
    // so that issuing a tile is straight-line code
    //
    // Product 2 (kCoop) deals the pieces differently: its Y image is the per-point pe6 TABLE, and G6 = g pe6 is formed from it in LDS, in place, ONCE per
    // workgroup (form() below) instead of by each of the four wm waves in registers.  A wave fetches what it forms -- the NS planes of column pair
    // p = wave, and of p = 8 + wave on waves 0..3 (a pair = one k-step of one column tile, 1 KB per plane) -- so the counted wait that says its own
    // pieces have landed is all that forming needs, and the tile's one barrier then covers "landed AND formed".  Waves 4..7 take X pieces instead.
    // Product 3 in the table form (TAB) does the same with the fp32 pe3 table: the two PLANES of a pair are the two halves of its fp32 values, and forming
    // overwrites them with hi and lo of Z0 = g pe3 + gJ_c d pe3 / d xi_c (form_z0() below; the deal is wgrad_z0_piece of dpn_layout.h).
    constexpr bool kCoop = PROD == 2 || TAB;
    static_assert(PROD != 2 || (2 * nct == 12 && nsx == 1 && S::kIssue >= 2 * NS), "product 2: 12 column pairs over 8 waves");
    static_assert(!TAB || (S::kIssue == 7 && S::kPad == 0 && nsx == 2), "product 3, table form: 56 pieces, seven per wave");
    const bool two_pairs = wave < 4;                                    // wave-uniform
    const char* pbase[S::kIssue];
    int pstride[S::kIssue], pdst[S::kIssue];
#pragma unroll
    for (int j = 0; j < S::kIssue; ++j) {
        int q = wave + 8 * j;                                           // the piece of the linear slot image: X planes, then Y planes ...
        if constexpr (TAB) q = wgrad_z0_piece(wave, j);
        else if constexpr (kCoop) q = wgrad_coop_piece(NS, S::kIssue, wave, j);     // ... or the deal of dpn_layout.h (-1: the pad)
        if (S::kPad && (kCoop ? q < 0 : q >= S::kPieces)) {             // a cache hit after the first time
            pbase[j] = xb + ((int64_t)net * nsx * tiles + (t0 < tiles ? t0 : 0)) * 16384; pstride[j] = 0; pdst[j] = S::kPadOff;
        } else if (q < nsx * 16) {
            pbase[j] = xb + ((int64_t)net * nsx + q / 16) * tiles * 16384 + (q % 16) * 1024; pstride[j] = 16384; pdst[j] = q * 1024;
        } else {
            const int qy = q - nsx * 16;
            pbase[j] = yb + (ynet * NS + qy / (2 * nct)) * tiles * S::kYPlane + (qy % (2 * nct)) * 1024; pstride[j] = S::kYPlane; pdst[j] = q * 1024;
        }
    }
    auto issue = [&](int64_t tile, int slot) __attribute__((always_inline)) {
        char* sl = lds + slot * kSlot;
#pragma unroll
        for (int j = 0; j < S::kIssue; ++j) {
            // read-once operand streams carry the non-temporal hint; the per-point pe6 table of product 2 is read by six nets' workgroups and should
            // stay in the memory-side cache (PMC, round 5: with the hint on it the table came from HBM six times: 1 052 MB against 890 algorithmic)
            // (the pe3 table of product 3's table form likewise)
            if (kCoop && (TAB ? wgrad_z0_is_y(wave, j) : wgrad_coop_is_y(NS, wave, j))) dma16(pbase[j] + tile * pstride[j] + lane * 16, sl + pdst[j]);
            else dma16_nt(pbase[j] + tile * pstride[j] + lane * 16, sl + pdst[j]);
        }
        dma4(gsrc + tile * 128, sl + S::kGOff + wave * 256);
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n2 = 0; n2 < NT; ++n2) acc[m][n2] = (f32x16)0.f;
    float vecA[MT], vecB[NT], gsum = 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) vecA[m] = 0.f;
#pragma unroll
    for (int n2 = 0; n2 < NT; ++n2) vecB[n2] = 0.f;
    // which wave of the waves that hold a row tile's (column tile's) fragments adds up its row-side (column-side) vector
    auto owns_row = [&](const int m) __attribute__((always_inline)) { return (kWide && nct == 6) ? wn == m % 3 : wn == m; };   // 4 wn for 4 m | 2 wn for 2 m
    auto owns_col = [&](const int n2) __attribute__((always_inline)) { return wm == n2; };                              // 2 wm for 2 n | 4 wm, three used

    // LDS reads by inline asm with a counted wait: a read hipcc can see is ordered behind ALL outstanding LDS-DMA (s_waitcnt vmcnt(0)
    // in front of the first ds_read of every tile), which serialised fetch and compute -- DMA alone 156 us, compute alone 131 us,
    // together 246 us before this, measured with stage-exit builds
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
    auto rd128 = [&](u32x4& v, const unsigned addr) __attribute__((always_inline)) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    };
    auto compute = [&](const int slot_) __attribute__((always_inline)) {
        const unsigned buf = lds_base + slot_ * kSlot;
        const unsigned gl = buf + S::kGOff + wave * 256;
        constexpr int KB = (NS == 1) ? 2 : 1;                       // single-bf16 fragments: both k-steps of the tile are read up front
        u32x4 gqa[KB][2], faa[KB][nsx][MT], fba[KB][NS][NT];
        // one base register per stream, the fragment index as the instruction's immediate offset (a full address per read costs a VGPR each for its
        // slot-independent part -- ~30 of them, hoisted out of the tile loop -- and spilled once the in-register operand forming of products 2 / 3 came in)
        const unsigned baseG = gl + h * 16;
        const unsigned baseA = buf + wm * (MT * 1024) + lane * 16, baseB = buf + S::kX + wn * (NT * 1024) + lane * 16;
        auto rd128o = [&](u32x4& v, const unsigned base, const int off) __attribute__((always_inline)) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(base), "i"(off) : "memory");
        };
        auto issue_reads = [&](const int kk, const int b) __attribute__((always_inline)) {
            if constexpr (PROD != 2) {                              // (product 2 needs g in form() only)
                rd128o(gqa[b][0], baseG, 64 * kk);
                rd128o(gqa[b][1], baseG, 64 * kk + 32);
            }
#pragma unroll
            for (int s2 = 0; s2 < nsx; ++s2)
#pragma unroll
                for (int m = 0; m < MT; ++m) rd128o(faa[b][s2][m], baseA, s2 * 16384 + (kk * 8 + m) * 1024);
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2)
#pragma unroll
                for (int n2 = 0; n2 < NT; ++n2) rd128o(fba[b][s2][n2], baseB, s2 * S::kYPlane + (kk * nct + n2) * 1024);
        };
        constexpr int kReads = (PROD == 2 ? 0 : 2) + MT * nsx + NT * NS;   // LDS reads per k-step
        if constexpr (NS == 1) { issue_reads(0, 0); issue_reads(1, 1); }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int b = (NS == 1) ? kk : 0;
            if constexpr (NS == 2) issue_reads(kk, 0);
            u32x4 (&fa)[nsx][MT] = faa[b];
            u32x4 (&fb)[NS][NT] = fba[b];
            u32x4& gq0 = gqa[b][0];
            u32x4& gq1 = gqa[b][1];
            // every value passes through the wait, so no use can be scheduled in front of it (LDS reads retire in order: with the
            // second k-step's reads still behind, the first k-step is complete at lgkmcnt(kReads))
            if (NS == 1 && kk == 0) asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(kReads) : "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (PROD == 2) gq0 = gq1 = (u32x4)0u;         // (gp below is dead code for product 2)
            else asm volatile("" : "+v"(gq0), "+v"(gq1));
            asm volatile("" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fb[0][0]), "+v"(fb[0][1]));
            if constexpr (MT == 4) asm volatile("" : "+v"(fa[0][2]), "+v"(fa[0][3]));
            if constexpr (NT == 3) asm volatile("" : "+v"(fb[0][2]));
            if constexpr (NS == 2) asm volatile("" : "+v"(fb[1][0]), "+v"(fb[1][1]));
            if constexpr (NS == 2 && NT == 3) asm volatile("" : "+v"(fb[1][2]));
            if constexpr (nsx == 2) asm volatile("" : "+v"(fa[1][0]), "+v"(fa[1][1]));
            if constexpr (nsx == 2 && MT == 4) asm volatile("" : "+v"(fa[1][2]), "+v"(fa[1][3]));
            const float gp[8] = {__uint_as_float(gq0[0]), __uint_as_float(gq0[1]), __uint_as_float(gq0[2]), __uint_as_float(gq0[3]),
                                 __uint_as_float(gq1[0]), __uint_as_float(gq1[1]), __uint_as_float(gq1[2]), __uint_as_float(gq1[3])};
            // (product 2: the Y fragments just read are this net's G6 = g pe6 already, form() has been over the slot)
            if (PROD == 1 && wave == 0 && i == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) gsum += gp[e];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (owns_row(m) && PROD != 2) {         // row-side vector: sum_pt X[pt][row] * g[pt]; the four waves that
                                                                         // hold this row tile's fragments take one tile each (all on
                                                                         // the wn = 0 waves it made them the workgroup's critical path:
                                                                         // +700 cycles per tile, everybody else waiting at the barrier);
                                                                         // 192-column products: the wn = 3 waves sit idle, three share
                    float d = 0.f;
#pragma unroll
                    for (int s2 = 0; s2 < nsx; ++s2) {
#pragma unroll
                        for (int p = 0; p < 4; ++p) { d = fmaf(bf_lo(fa[s2][m][p]), gp[2 * p], d); d = fmaf(bf_hi(fa[s2][m][p]), gp[2 * p + 1], d); }
                    }
                    vecA[m] += d;
                }
#pragma unroll
                for (int n2 = 0; n2 < NT; ++n2) {
                    if constexpr (NS == 2) {
                        acc[m][n2] = mfma(as_bf(fa[0][m]), as_bf(fb[1][n2]), acc[m][n2]);
                        if constexpr (nsx == 2) acc[m][n2] = mfma(as_bf(fa[1][m]), as_bf(fb[0][n2]), acc[m][n2]);
                    }
                    acc[m][n2] = mfma(as_bf(fa[0][m]), as_bf(fb[0][n2]), acc[m][n2]);
                }
            }
            if (PROD != 3) {                                             // column-side vector: q = sum_pt Y[pt][col] (Z, Z1, G6), one column tile per wm
#pragma unroll
                for (int n2 = 0; n2 < NT; ++n2) {
                    if (!owns_col(n2)) continue;
                    float d = 0.f;
#pragma unroll
                    for (int s2 = 0; s2 < NS; ++s2)
#pragma unroll
                        for (int p = 0; p < 4; ++p) d += bf_lo(fb[s2][n2][p]) + bf_hi(fb[s2][n2][p]);
                    vecB[n2] += d;
                }
            }
        }
    };

    // Product 2: this wave's column pairs of the slot's pe6 table image (hi [+ lo]) become this net's operand G6 = g pe6, in place: the 16 bytes of a lane
    // per plane are the eight points of its column, element e <-> point e of the lane's eight (its own copy of g).  The arithmetic is what each wm wave did
    // on its registers before (S2 and q6 are bit-identical).  Reads and writes are lane-private and touch only pieces this wave fetched itself: the caller
    // has waited for them (vmcnt) and runs the tile's barrier afterwards -- form() ends with all its LDS writes retired.
    auto form = [&](const int slot_) __attribute__((always_inline)) {
        const unsigned buf = lds_base + slot_ * kSlot;
        const unsigned baseG = buf + S::kGOff + wave * 256 + h * 16, baseY = buf + S::kX + wave * 1024 + lane * 16;
        auto pair = [&](auto q_) __attribute__((always_inline)) {
            constexpr int q = decltype(q_)::value;                    // pair p = wave + 8 q: k-step kk = p / nct
            const unsigned ay = baseY + q * 8192, ag = baseG + ((wave + 8 * q) >= nct ? 64 : 0);
            u32x4 t[2], gq0, gq1;
            rd128(gq0, ag);
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(gq1) : "v"(ag) : "memory");
            rd128(t[0], ay);
            if constexpr (NS == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(t[1]) : "v"(ay), "i"(S::kYPlane) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(gq0), "+v"(gq1), "+v"(t[0]));
            if constexpr (NS == 2) asm volatile("" : "+v"(t[1]));
            const float gp[8] = {__uint_as_float(gq0[0]), __uint_as_float(gq0[1]), __uint_as_float(gq0[2]), __uint_as_float(gq0[3]),
                                 __uint_as_float(gq1[0]), __uint_as_float(gq1[1]), __uint_as_float(gq1[2]), __uint_as_float(gq1[3])};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float v0 = bf_lo(t[0][p]), v1 = bf_hi(t[0][p]);
                if constexpr (NS == 2) { v0 += bf_lo(t[1][p]); v1 += bf_hi(t[1][p]); }
                const float z0 = gp[2 * p] * v0, z1 = gp[2 * p + 1] * v1;
                const u32 hi = pack2(z0, z1);
                t[0][p] = hi;
                if constexpr (NS == 2) t[1][p] = pack2(z0 - bf_lo(hi), z1 - bf_hi(hi));
            }
            asm volatile("ds_write_b128 %0, %1" :: "v"(ay), "v"(t[0]) : "memory");
            if constexpr (NS == 2) asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(ay), "v"(t[1]), "i"(S::kYPlane) : "memory");
        };
        pair(std::integral_constant<int, 0>{});
        if (two_pairs) pair(std::integral_constant<int, 1>{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    // Product 3, table form: this wave's pairs of the slot's fp32 pe3 table image become hi (plane 0) and lo (plane 1) of this net's Z0, in place.  A lane
    // owns eight points of one column: its 32 bytes are own[e], the neighbouring lane's (lane ^ 1, the same 1-KB piece: sine <-> cosine of the same angle)
    // partner[e]; with g and gJ_c from the wave's per-tile copy,  gf = gJ_c fr,  z = fmaf(g, own, +-(gf partner))  -- + for a sine column, - for a cosine
    // column -- in ts::z0_frag's operation order, then hi = bf16(z), lo = bf16(z - hi) as frag_set2<2>: the bits the stored form holds.  All of a pair's
    // reads (the wave's own pieces: vmcnt) are back before its writes go out, and the writes are retired before the caller's barrier.
    auto form_z0 = [&](const int slot_) __attribute__((always_inline)) {
        const unsigned buf = lds_base + slot_ * kSlot;
        const int ct = wgrad_z0_ct(wave);
        const unsigned baseG = buf + S::kGOff + wave * 256 + h * 16, baseY = buf + S::kX + ct * 1024;
        const u32 sgn = (lane & 1) ? 0x80000000u : 0u;
        auto pair = [&](const int kk) __attribute__((always_inline)) {
            const unsigned ay = baseY + kk * (nct * 1024) + lane * 16, ap = baseY + kk * (nct * 1024) + (lane ^ 1) * 16, ag = baseG + kk * 64;
            u32x4 gq[2], jq[2], own[2], par[2];
            rd128(gq[0], ag);
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(gq[1]) : "v"(ag) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(jq[0]) : "v"(ag) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:160" : "=v"(jq[1]) : "v"(ag) : "memory");
            rd128(own[0], ay);
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(own[1]) : "v"(ay), "i"(S::kYPlane) : "memory");
            rd128(par[0], ap);
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(par[1]) : "v"(ap), "i"(S::kYPlane) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(gq[0]), "+v"(gq[1]), "+v"(jq[0]), "+v"(jq[1]), "+v"(own[0]), "+v"(own[1]), "+v"(par[0]), "+v"(par[1]));
            float z[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float gf = __uint_as_float(jq[e >> 2][e & 3]) * fr;
                const float t = __uint_as_float(__float_as_uint(gf * __uint_as_float(par[e >> 2][e & 3])) ^ sgn);
                z[e] = fmaf(__uint_as_float(gq[e >> 2][e & 3]), __uint_as_float(own[e >> 2][e & 3]), t);
            }
            u32x4 hi, lo;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                hi[p] = pack2(z[2 * p], z[2 * p + 1]);
                lo[p] = pack2(z[2 * p] - bf_lo(hi[p]), z[2 * p + 1] - bf_hi(hi[p]));
            }
            asm volatile("ds_write_b128 %0, %1" :: "v"(ay), "v"(hi) : "memory");
            asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(ay), "v"(lo), "i"(S::kYPlane) : "memory");
        };
        pair(wgrad_z0_kk(wave, 0));
        if (two_pairs) pair(wgrad_z0_kk(wave, 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    // prologue: RING-1 tiles in flight (out-of-range tiles re-read the last valid one; their data is never used)
    const int64_t tl = t1 > t0 ? t1 - 1 : t0;
#pragma unroll
    for (int r = 0; r < RING - 1; ++r) issue(t0 + r < t1 ? t0 + r : tl, r);
    int slot = 0;
#ifdef DPN_WGRAD_PHASES
    u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, ph_wait = 0, ph_bar = 0, ph_issue = 0, ph_comp = 0;
#endif
    for (int64_t tile = t0; tile < t1; ++tile) {
        DPN_WG_CLOCK(c0);
        wait_vmcnt<(RING - 2) * PER_TILE>();                             // this wave's pieces of `tile` have landed
        if constexpr (TAB) form_z0(slot);
        else if constexpr (kCoop) form(slot);                            // (nobody reads this slot before the barrier, nobody else writes these bytes)
        DPN_WG_CLOCK(c1);
        __builtin_amdgcn_s_barrier();                                    // ... and everybody else's [and formed]; and compute(tile-1) is finished everywhere
        DPN_WG_CLOCK(c2);
        {
            const int64_t nt = tile + RING - 1;
            issue(nt < t1 ? nt : tl, (slot + RING - 1) % RING);          // refill the slot that compute(tile-1) just released
        }
        DPN_WG_CLOCK(c3);
        if (active) compute(slot);
        DPN_WG_CLOCK(c4);
#ifdef DPN_WGRAD_PHASES
        ph_wait += c1 - c0; ph_bar += c2 - c1; ph_issue += c3 - c2; ph_comp += c4 - c3;
#endif
        slot = (slot + 1) % RING;
    }
#ifdef DPN_WGRAD_PHASES
    if (a.phases && lane == 0) {
        unsigned* o = a.phases + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + wave) * 8;
        o[0] = ph_wait; o[1] = ph_bar; o[2] = ph_issue; o[3] = ph_comp; o[4] = (unsigned)(t1 - t0); o[5] = PROD;
    }
#endif
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    // ---- write this split's partial sums: natural [row slot][col] order
    float* part = a.partials + ((int64_t)split * kNets + net) * kPartFloats;
    float* out = part + part_off(PROD);
    if (active) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n2 = 0; n2 < NT; ++n2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = wm * (MT * 32) + 32 * m + drow32(r, h);
                    const int cc = wn * (NT * 32) + 32 * n2 + i;
                    out[rr * ncol + cc] = acc[m][n2][r];
                }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float v = vecA[m] + __shfl_xor(vecA[m], 32);
        if (owns_row(m) && h == 0) {
            const int rr = wm * (MT * 32) + 32 * m + i;
            if (PROD == 1) part[kPartVec + 2 * 256 + rr] = v;          // mv1 (= mvec again: the hyper-network's half of the reduction does not wait for P0)
            if (PROD == 3) part[kPartVec + 3 * 256 + rr] = v;          // db1
        }
    }
    if (PROD == 1 && wave == 0) {
        const float gs = gsum + __shfl_xor(gsum, 32);                  // lanes 0 and 32 hold the two halves
        if (lane == 0) part[kPartVec + 4 * 256] = gs;
    }
    if (PROD != 3 && active) {
        const int qo = kPartVec + (PROD == 1 ? 5 : 6) * 256;                             // q1 = colsum(Z1), q6 = colsum(G6)
#pragma unroll
        for (int n2 = 0; n2 < NT; ++n2) {
            const float v = vecB[n2] + __shfl_xor(vecB[n2], 32);
            if (owns_col(n2) && h == 0) part[qo + wn * (NT * 32) + 32 * n2 + i] = v;
        }
    }
}

template <int NS>
__global__ __launch_bounds__(512, 2) void dpn_wgrad_kernel(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[wgrad_lds_bytes<NS>()];
    // workgroup -> (product, point range): uniform scalar walk.  (Round 5 tried an XCD-aware placement -- the six nets' product-2 workgroups of one range on
    // ONE XCD, so that its L2 serves the per-point pe6 table to five of them: 186.7 / 186.1 us against 184.7 / 188.6 us for this linear walk on one box.
    // No difference: the table's re-reads are served by the memory-side cache either way.)
    int prod = 1, split = blockIdx.x;
    const int net = blockIdx.y;
    while (prod < 3 && split >= a.splits[prod]) { split -= a.splits[prod]; ++prod; }
    if (prod == 1) wgrad_body<NS, 1>(a, lds, split, net);
    else if (prod == 2) wgrad_body<NS, 2>(a, lds, split, net);
    else {
        // product 3 has two bodies: Z0 stored per point and net (plain bf16, caller-encoded coordinates, the second-derivative kernels) or formed from the
        // per-point table (OperandView); the stage-1 launch that filled the operand buffer said which, in the buffer's header -- workgroup-uniform
        if constexpr (NS == 2) {
            const unsigned form = __builtin_amdgcn_readfirstlane(operand_view(a.operands, a.n_pad, NS).hdr[0]);
            if (form == kZ0Table) { wgrad_body<NS, 3, true>(a, lds, split, net); return; }
        }
        wgrad_body<NS, 3>(a, lds, split, net);
    }
}

// ------------------------------------------------------------------------------------------------ backward, stage 3
// Round 5: two halves.  (1) dpn_finish_rows_kernel -> dpn_finish_vside_kernel: what the hyper-network's backward waits for (d w1b1, d w2b2,
// d evec; dWd, d bd ride in the same launch).  (2) dpn_finish_gside_kernel -> dpn_finish_fc2_kernel: gradients of static tensors only
// (cat_fc1.fc.0 / fc.2, out_fc) -- the host may run them on a side branch beside the encoder's backward chain (dpn_wgrad_finish_parts).
struct FinishArgs {
    DpnNetPtrs net[kNets];
    DpnNetGradPtrs grad[kNets];
    const char* packed;
    const float* partials;
    float* scratch_s1;      // [6][256][256] S1 = M2^T Z1, natural order             (dpn_finish_rows_kernel -> vside, gside)
    float* scratch_s2;      // [6][256][192] S2 = M2^T G6
    float* scratch_mv;      // [6][256]      mvec = M2^T g
    float* scratch_u;       // [6][256]      u = W2^T wo, natural order
    float* scratch_q1;      // [6][256]      colsum(Z1)
    float* scratch_q6;      // [6][256]      colsum(G6) (192 used)
    float* scratch_sg;      // [8]           sum g per net
    float* scratch_rp;      // [6][8][256]   per column tile: sum_i W1[o][i] G[o][i]      (gside -> fc2)
    int splits[4], ns;      // point ranges per product, as dpn_wgrad_kernel cut them (splits[0] = 0: the product M2^T Z is gone)
    int64_t n;
};

DEV int slot_of_ch(int ch) { return (ch & ~15) + 8 * ((ch >> 2) & 1) + 4 * ((ch >> 3) & 1) + (ch & 3); }
// original PE3 / PE6 channel -> slot index 16*ks + 8*h + e
DEV int slot_of_pe3(int orig) {
    const int f = orig / 6, fn = (orig % 6) / 3, c = orig % 3;
    const int a = 32 * c + f;
    const int ks = a >> 3, h = (a >> 2) & 1, p = a & 3;
    return 16 * ks + 8 * h + 2 * p + fn;
}
DEV int slot_of_pe6(int orig) {
    const int f = orig / 12, fn = (orig % 12) / 6, c6 = orig % 6;
    const int a = 16 * c6 + f;
    const int ks = a >> 3, h = (a >> 2) & 1, p = a & 3;
    return 16 * ks + 8 * h + 2 * p + fn;
}

// NQ sums over the partial buffers of the point ranges (ks[q] of them for sum q: the count of the product that wrote it), ALL their
// loads in flight at once (a loop of load -> wait -> add, which is what hipcc makes of the obvious code, costs one HBM round trip per
// range and per sum: 40 in a row per thread).  Ranges beyond ks[q] re-read the last one and are not added; the additions keep the
// range order, so the result does not depend on how the loads are grouped.
constexpr int kMaxSplits = 20;                  // choose_plan() never returns more for one product
template <int NQ, int MAXS>
DEV void part_sums_n(const float* partials, const int (&ks)[NQ], int net, const int (&off)[NQ], float (&out)[NQ]) {
    float v[MAXS][NQ];
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            // (plain loads: with the non-temporal hint -- "read once" -- the partials dpn_wgrad has just written are fetched past the memory-side cache: the finish
            //  stage's first half 28.8 against 25.4 us alone, dpn_finish_rows 18.5 against 15.7 us in the step; profiles/round6_nontemporal_hints.txt)
            v[k][q] = partials[((int64_t)min(k, ks[q] - 1) * kNets + net) * kPartFloats + off[q]];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) t += (k < ks[q]) ? v[k][q] : 0.f;
        out[q] = t;
    }
}
template <int NQ>
DEV void part_sums(const float* partials, const int (&ks)[NQ], int net, const int (&off)[NQ], float (&out)[NQ]) {
    int most = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) most = ks[q] > most ? ks[q] : most;
    if (most <= 12) part_sums_n<NQ, 12>(partials, ks, net, off, out);
    else if (most <= 16) part_sums_n<NQ, 16>(partials, ks, net, off, out);
    else part_sums_n<NQ, kMaxSplits>(partials, ks, net, off, out);
}

// one block per (output row o, net): reduces the point ranges, un-permutes: rows o of S1, S2 and of d(w1b1); the row's vector entries
__global__ __launch_bounds__(256) void dpn_finish_rows_kernel(FinishArgs a) {
    const int o = blockIdx.x, net = blockIdx.y, i = threadIdx.x;
    const DpnNetGradPtrs& Gd = a.grad[net];
    const int so = slot_of_ch(o), si = slot_of_ch(i);
    // thread 0..4 also own the row's vector entries: fetched with everything else, not after the reduction
    float rowv[1] = {0.f};
    const bool has_vec = i < 4 || (i == 4 && o == 0);
    if (has_vec) {
        // mv1 = M2^T g and db1 = T1^T g (row slot so), q1 = colsum(Z1) (column slot of channel o), q6 = colsum(G6) (PE6 channel o), sum g
        const int offv[1] = {i == 0 ? kPartVec + 2 * 256 + so : i == 1 ? kPartVec + 3 * 256 + so : i == 2 ? kPartVec + 5 * 256 + so
                             : i == 3 ? kPartVec + 6 * 256 + slot_of_pe6(o < kPe ? o : 0) : kPartVec + 4 * 256};
        const int ksv[1] = {i == 1 ? a.splits[3] : i == 3 ? a.splits[2] : a.splits[1]};
        part_sums<1>(a.partials, ksv, net, offv, rowv);
    }
    if (i < kPe) {
        const int off3[3] = {part_off(1) + so * 256 + si, part_off(2) + so * 192 + slot_of_pe6(i), part_off(3) + so * 192 + slot_of_pe3(i)};
        const int ks3[3] = {a.splits[1], a.splits[2], a.splits[3]};
        float g3[3];
        part_sums<3>(a.partials, ks3, net, off3, g3);
        a.scratch_s1[((int64_t)net * 256 + o) * 256 + i] = g3[0];
        a.scratch_s2[((int64_t)net * 256 + o) * kPe + i] = g3[1];
        Gd.w1b1[o * Gd.ld_w1b1 + i] = g3[2];
    } else {
        const int off1[1] = {part_off(1) + so * 256 + si};
        const int ks1[1] = {a.splits[1]};
        float g1[1];
        part_sums<1>(a.partials, ks1, net, off1, g1);
        a.scratch_s1[((int64_t)net * 256 + o) * 256 + i] = g1[0];
    }
    if (i == 0) {
        // u[o] = (W2^T wo)[o] from the packed vectors ([h][T][r] order)
        const float* vec = reinterpret_cast<const float*>(a.packed + (long)net * pack_bytes_per_net(a.ns) + (long)kPackKB * 1024 * a.ns);
        const int T = o >> 5, w = o & 31, hh = (w >> 2) & 1, r = (w & 3) + 4 * (w >> 3);
        a.scratch_u[net * 256 + o] = vec[kVecU * 256 + hh * 128 + T * 16 + r];
        a.scratch_mv[net * 256 + o] = rowv[0];
    }
    if (i == 1) Gd.w1b1[o * Gd.ld_w1b1 + 192] = rowv[0];
    if (i == 2) a.scratch_q1[net * 256 + o] = rowv[0];
    if (i == 3 && o < kPe) a.scratch_q6[net * 256 + o] = rowv[0];
    if (i == 4 && o == 0) a.scratch_sg[net] = rowv[0];
}

// The factor that turns the mask-side sums into the gradients that used to need v per point (SavedView):
//   d(w2b2)[o][i] = sum_j W1[j][o] u[j] S1[j][i] + 2 wo[o] q1[i]        S1 = M2^T Z1   (i < 256),  column 256: S1 -> M2^T g, q1 -> sum g
//   dWd[o][i]     = sum_j W1[j][o] u[j] S2[j][i] + 2 wo[o] q6[i]        S2 = M2^T G6
// and d evec = d bd = column 256.  One workgroup per 32 x 32 output tile: grid (8 row tiles x 15 column tiles [8 of d w2, the vector, 6 of
// dWd], 6 nets); the four waves take 64 of the 256 j each on the exact-fp32 matrix instruction (operands straight from global memory: both
// are contiguous along the lane index) and their partial tiles are added in a fixed order through LDS.
DEV f32x16 mfma_f32_32x32x2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
constexpr int kVsideBlocks = 8 * 15;
DEV void finish_vside_body(const FinishArgs& a, const int bx, const int net, float (&red)[4][16][64], float (&qs)[32]) {
    const int rt = bx & 7, ctile = bx >> 3;
    const int kind = ctile < 8 ? 0 : ctile == 8 ? 1 : 2;                  // d w2 | vector column | dWd
    const DpnNetPtrs& P = a.net[net];
    const DpnNetGradPtrs& Gd = a.grad[net];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    const int o0 = 32 * rt, n0 = kind == 0 ? 32 * ctile : kind == 2 ? 32 * (ctile - 9) : 0, ncol = kind == 0 ? 256 : kind == 2 ? kPe : 1;
    const float* B = kind == 0 ? a.scratch_s1 + (int64_t)net * 65536 : kind == 2 ? a.scratch_s2 + (int64_t)net * 256 * kPe : a.scratch_mv + net * 256;
    const float* U = a.scratch_u + net * 256;
    const int ldb = ncol;
    const bool colok = n0 + col < ncol;
    // the rank-one term's column factor: q1 / q6 / sum g
    float qv = 0.f;
    if (wv == 0 && colok) qv = kind == 0 ? a.scratch_q1[net * 256 + n0 + col] : kind == 2 ? a.scratch_q6[net * 256 + n0 + col] : a.scratch_sg[net];
    f32x16 acc = (f32x16)0.f;
    float av[32], bv[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        const int j = 64 * wv + 2 * kk + kh;
        av[kk] = P.W1[j * 256 + o0 + col] * U[j];
        bv[kk] = colok ? B[(int64_t)j * ldb + n0 + col] : 0.f;
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = mfma_f32_32x32x2(av[kk], bv[kk], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wv][r][lane] = acc[r];
    if (wv == 0 && kh == 0) qs[col] = qv;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = wv + 4 * q;                                         // element (r, lane) of the tile: row drow32(r, kh), column col
        const float sum = (red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]);
        const int o = o0 + drow32(r, kh), i = n0 + col;
        if (!colok) continue;
        const float v = sum + 2.0f * P.wo[o] * qs[col];
        if (kind == 0) Gd.w2b2[o * Gd.ld_w2b2 + i] = v;
        else if (kind == 2) Gd.Wd[o * kPe + i] = v;
        else { Gd.w2b2[o * Gd.ld_w2b2 + 256] = v; Gd.evec[o] = v; Gd.bd[o] = v; }
    }
}

// G = M2^T Z without Z (round 5).  Z = Z1 w2^T + G6 Wd^T + g cvec^T is linear in the three per-point operands, so
//   G[o][i] = sum_j S1[o][j] w2[i][j] + sum_k S2[o][k] Wd[i][k] + mvec[o] cvec[i]          cvec = b2 + bd + e
// -- a 256 x 256 x 448 exact-fp32 GEMM per net on the sums dpn_wgrad_kernel produces anyway.  From it d cat_fc1.fc.0.weight = diag(u) G and the
// per-tile parts of r[o] = sum_i W1[o][i] G[o][i] (+ bf1 mvec, added by dpn_finish_fc2_kernel).  One workgroup per 32 x 32 tile of G; wave wv
// takes j in [64 wv, 64 wv + 64) and k in [48 wv, 48 wv + 48); lane (col, kh) holds four consecutive reduction indices per load of its row.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
DEV void finish_gside_body(const FinishArgs& a, const int bx, const int net, float (&red)[4][16][64]) {
    const int rt = bx & 7, ct = bx >> 3;
    const DpnNetPtrs& P = a.net[net];
    const DpnNetGradPtrs& Gd = a.grad[net];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31, kh = lane >> 5;
    const int o0 = 32 * rt, i0 = 32 * ct;
    const float* S1 = a.scratch_s1 + ((int64_t)net * 256 + o0 + col) * 256;
    const float* S2 = a.scratch_s2 + ((int64_t)net * 256 + o0 + col) * kPe;
    const float* w2 = P.w2b2 + (int64_t)(i0 + col) * P.ld_w2b2;
    const float* Wd = P.Wd + (i0 + col) * kPe;
    f32x4u a1[8], b1[8], a2[6], b2[6];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = 64 * wv + 8 * m + 4 * kh;
        a1[m] = *reinterpret_cast<const f32x4u*>(S1 + k);
        b1[m] = *reinterpret_cast<const f32x4u*>(w2 + k);
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int k = 48 * wv + 8 * m + 4 * kh;
        a2[m] = *reinterpret_cast<const f32x4u*>(S2 + k);
        b2[m] = *reinterpret_cast<const f32x4u*>(Wd + k);
    }
    f32x16 acc = (f32x16)0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma_f32_32x32x2(a1[m][e], b1[m][e], acc);
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma_f32_32x32x2(a2[m][e], b2[m][e], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wv][r][lane] = acc[r];
    __syncthreads();
    const int i = i0 + col;
    const float cv = P.w2b2[(int64_t)i * P.ld_w2b2 + 256] + P.bd[i] + P.evec[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = wv + 4 * q;                                         // element (r, lane) of the tile: row drow32(r, kh), column col
        const int o = o0 + drow32(r, kh);
        const float G = ((red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane])) + a.scratch_mv[net * 256 + o] * cv;
        Gd.W1[o * 256 + i] = a.scratch_u[net * 256 + o] * G;
        float rp = P.W1[o * 256 + i] * G;                                 // this tile's part of r[o]: the 32 columns sit on the 32 lanes of a half-wave
#pragma unroll
        for (int sft = 16; sft > 0; sft >>= 1) rp += __shfl_xor(rp, sft);
        if (col == 0) a.scratch_rp[((int64_t)net * 8 + ct) * 256 + o] = rp;
    }
}

// ONE launch for the two independent consumers of dpn_finish_rows_kernel's sums: blocks [0, n_v) = the W1^T diag(u) factor (what the hyper-network's
// backward waits for), the rest = G = S1 w2^T + S2 Wd^T + ... (static tensors only) -- side by side instead of one behind the other.  n_v = 0 or
// kVsideBlocks, the grid decides which halves run (dpn_wgrad_finish_parts).
constexpr int kGsideBlocks = 64;
__global__ __launch_bounds__(256) void dpn_finish_sides_kernel(FinishArgs a, int n_v) {
    __shared__ float red[4][16][64];
    __shared__ float qs[32];
    // As dispatched, XCD = blockIdx.x mod 8 = the ROW tile (the grid's x extent is a multiple of 8): the 15 x 6 (or 8 x 6) tiles that read the same 32 columns of
    // W1 (rows of S1: each lane its own row) sat on one L2.  Every XCD takes a contiguous range of the (net, block) list instead, as in dpn_pack_fused_kernel.
#ifdef FINISH_NO_XCD_REMAP
    const int net = blockIdx.y, bx = blockIdx.x;
#else
    const int gx = gridDim.x, total = gx * kNets, lin = blockIdx.x + gx * blockIdx.y, xcd = lin & 7;
    const int virt = xcd * (total >> 3) + min(xcd, total & 7) + (lin >> 3), net = virt / gx, bx = virt - net * gx;
#endif
    if (bx < n_v) finish_vside_body(a, bx, net, red, qs);
    else finish_gside_body(a, bx - n_v, net, red);
}

// one block per (row o', net): r, then dW2 = wo (x) r, dbf2, dwo (with colsum(Z) = w2 q1 + Wd q6 + sum g cvec), dbo, dbf1
__global__ __launch_bounds__(256) void dpn_finish_fc2_kernel(FinishArgs a) {
    __shared__ float red[2][256];
    const int net = blockIdx.y, op = blockIdx.x, o = threadIdx.x;
    const DpnNetPtrs& P = a.net[net];
    const DpnNetGradPtrs& Gd = a.grad[net];
    const float* rp = a.scratch_rp + (int64_t)net * 8 * 256 + o;
    const float mv = a.scratch_mv[net * 256 + o];
    const float r = (((rp[0] + rp[256]) + (rp[512] + rp[768])) + ((rp[1024] + rp[1280]) + (rp[1536] + rp[1792]))) + P.bf1[o] * mv;
    const float wop = P.wo[op];
    Gd.W2[op * 256 + o] = wop * r;
    red[0][o] = P.W2[op * 256 + o] * r;
    red[1][o] = a.scratch_q1[net * 256 + o] * P.w2b2[(int64_t)op * P.ld_w2b2 + o] + (o < kPe ? a.scratch_q6[net * 256 + o] * P.Wd[op * kPe + o] : 0.f);
    if (op == 0) Gd.bf1[o] = a.scratch_u[net * 256 + o] * mv;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (o < s) { red[0][o] += red[0][o + s]; red[1][o] += red[1][o + s]; }
        __syncthreads();
    }
    if (o == 0) {
        const float sg = a.scratch_sg[net];
        const float cv = P.w2b2[(int64_t)op * P.ld_w2b2 + 256] + P.bd[op] + P.evec[op];
        const float zsum = red[1][0] + sg * cv;                           // colsum(Z)[op]
        Gd.bf2[op] = wop * sg;
        Gd.wo[op] = red[0][0] + P.bf2[op] * sg + 2.f * zsum;
        if (op == 0) Gd.bo[0] = sg;
    }
}

// ------------------------------------------------------------------------------------------------ MFMA layout self-test
__global__ void dpn_selftest_kernel(float* out) {
    // A = I (32x32 over two k-steps of 16) against B1[k][j] = k and B2[k][j] = j: D1[i][j] = i, D2[i][j] = j.
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    f32x16 acc1 = (f32x16)0.f, acc2 = (f32x16)0.f;
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 A, B1, B2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 16 * ks + 8 * h + e;        // this (ks,h,e) k-slot <-> index k (any bijection works as long as A and B agree)
            A[e] = (__bf16)((k == i) ? 1.f : 0.f);
            B1[e] = (__bf16)(float)k;
            B2[e] = (__bf16)(float)i;
        }
        acc1 = mfma(A, B1, acc1);
        acc2 = mfma(A, B2, acc2);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { out[lane * 16 + r] = acc1[r]; out[1024 + lane * 16 + r] = acc2[r]; }
}

// Point ranges per product.  One 8-wave workgroup per CU (the LDS ring fills it) and a kernel time that falls as 1 / workgroups up to
// one round (measured, hi+lo mode, 37 265 points: 120 workgroups 671 us, 192 452 us, 240 396 us, 288 562 us -- the tail round), so
// the plan fills one round of the 256 CUs: 42 workgroups per net.  Hi+lo mode: dw1 = T1^T Z0 is the one product whose slot (two X planes)
// leaves room for a ring of two only, so its tiles take longest and it gets the most ranges; measured (tools/wgrad_overlap_probe.py,
// profiles/round3_wgrad_plans.txt): 10,11,10,11 327 us, 11,11,9,11 303 us, 10,10,9,13 277 us, 10,10,8,14 277 us, 9,9,8,16 280 us --
// a plateau at 5.0 TB/s.  Single bf16 (rings of four and five): 10,11,10,11 156 us, 10,10,9,13 160-163 us.
struct SplitPlan { int s[4]; int most; };
// Round 5: three products (s[0] = 0: M2^T Z is gone, dpn_finish_gside_kernel); product 2 forms its Y operand G6 = g pe6 in registers from the
// per-point table (OperandView), which makes ITS tiles the slowest: it gets the most ranges per byte.  Sweeps of the 42 ranges per net
// (tools/wgrad_overlap_probe.py, profiles/round5_wgrad_plans.txt; eager launches back to back): hi+lo 14,12,16 277 us, 15,12,15 244, 14,13,15 234,
// 13,13,16 228, 15,13,14 233, 13,14,15 224; single bf16 14,13,15 163 us, 15,13,14 136, 14,12,16 137, 13,13,16 129, 15,12,15 133, 16,13,13 132.
// Since G6 is formed once per workgroup in LDS (wgrad_body, form()) product 2's tiles are no longer the slowest.  Sweeps with the forming in LDS (the same
// 42 ranges; tools/wgrad_time.py, 3 x 100 launches per plan, two processes per build alternated with the build before; profiles/wgrad_coop_forming_plans.txt):
// hi+lo 13,14,15 215-219 us (before the change: 229-234), 14,13,15 208-211, 15,12,15 211-212, 14,14,14 208-212, 15,13,14 206-208 (before: 239-241) -- and
// on a second box 13,14,15 203-205, 15,14,13 200-201, 14,15,13 198-202, 15,13,14 194-196; single bf16 13,13,16 124-128 us (before: 129-131), 14,12,16
// 124-126, 15,12,15 123-126, 15,11,16 131-132, 14,13,15 121-122.  The plans STAY: 15,13,14 is worth 9 us of the kernel and 15-20 us of the captured step
// (three alternated bench.py rounds, same file), but another plan is another summation order -- every gradient moves by up to 1.2e-06 of its tensor's
// largest magnitude (two plans of one build, n = 5197), and 200 optimiser steps of the benchmark turn that into a different trajectory, where today a
// build can be held to the one before it bit for bit.  (Plain bf16: 14,13,15 also has 15 as its most ranges; k_splits of dpn_sizes is 16 there.)
static inline SplitPlan choose_plan(int64_t n_pad, int ns) {
    int64_t c = n_pad / 32 / 16;
    if (c < 1) c = 1;
    SplitPlan p;
    if (c >= 10) p = (ns == 2) ? SplitPlan{{0, 13, 14, 15}, 15} : SplitPlan{{0, 13, 13, 16}, 16};
    else p = SplitPlan{{0, (int)c, (int)c, (int)c}, (int)c};
#ifdef DPN_EXPERIMENT_SPLITS                     // timing experiments only: DPN_WGRAD_PLAN="9,12,10,11"
    if (const char* e = getenv("DPN_WGRAD_PLAN")) {
        if (sscanf(e, "%d,%d,%d,%d", &p.s[0], &p.s[1], &p.s[2], &p.s[3]) == 4) {
            p.most = 1;
            p.s[0] = 0;
            for (int k = 1; k < 4; ++k) { if (p.s[k] < 1) p.s[k] = 1; if (p.s[k] > kMaxSplits) p.s[k] = kMaxSplits; if (p.s[k] > p.most) p.most = p.s[k]; }
        }
    }
#endif
    return p;
}

// A device-clock stamp as a graph node: HIP event records inside a stream capture are not timing events (and torch refuses external events on ROCm),
// so a measurement INSIDE a replayed hipGraph puts this one-thread kernel in front of and behind the launch it brackets.  wall_clock64() is the
// constant-rate counter HIP events read (hipDeviceAttributeWallClockRate, 100 MHz on gfx950).
__global__ void dpn_clock_stamp_kernel(unsigned long long* ring, unsigned int* cursor, unsigned int cap) {
    const unsigned long long t = wall_clock64();
    ring[atomicAdd(cursor, 1u) % cap] = t;
}

constexpr int64_t kFinishScratchFloats = (int64_t)kNets * 65536 + (int64_t)kNets * 256 * 192 + 4 * kNets * 256 + 8 + (int64_t)kNets * 8 * 256;   // S1 | S2 | mv | u | q1 | q6 | sum g | r parts (FinishArgs)

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int dpn_version(void) { return 2; }

int dpn_clock_stamp(unsigned long long* ring, unsigned int* cursor, unsigned int cap, void* stream) {
    if (!ring || !cursor || cap == 0) return -1;
    hipLaunchKernelGGL(dpn_clock_stamp_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), ring, cursor, cap);
    return ck(hipGetLastError());
}

int dpn_clock_rate_khz(int* khz) {
    if (!khz) return -1;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return ck(e);
    return ck(hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, dev));
}

// which packed form (dpn_pack_weights_form) the forward launch of this precision mode expects: 1 = fused (tile-split kernel), 0 = ring stream
int dpn_fwd_form(int prec, int has_pe_in) { return use_tiles("DPN_FWD_KERNEL", prec, has_pe_in != 0) ? 1 : 0; }

int dpn_sizes(int64_t n, int prec, DpnSizes* out) {
    if (!out || n <= 0 || (prec != 1 && prec != 2)) return -1;
    const int64_t n_pad = pad_points(n);
    out->n_pad = n_pad;
    out->packed = (((int64_t)kNets * pack_bytes_per_net(prec) + 255) / 256) * 256;
    out->saved = saved_state_bytes(n_pad, prec);
    out->operands = operand_bytes(n_pad, prec);
    out->k_splits = choose_plan(n_pad, prec).most;
    out->partials = ((int64_t)out->k_splits * kNets * kPartFloats + kFinishScratchFloats) * 4;
    return 0;
}

// form 0: the seven-GEMM stream of the ring kernels; form 1: the fused five-GEMM stream of dpn_fwd_tiles_kernel (dpn_layout.h) -- ONE launch forms
// A = W1 w2, B = W1 Wd and C2 = W1 cvec + bf1 on the exact-fp32 matrix instruction and writes them as fragments (dpn_pack_fused_kernel)
int dpn_pack_weights_batch(const DpnNetPtrs nets[DPN_NETS], int n_fields, int64_t heads_stride, int64_t evec_stride, int prec, int form, void* packed,
                           int64_t packed_stride, void* stream) {
    if (!nets || !packed || (prec != 1 && prec != 2) || (form != 0 && form != 1) || n_fields < 1 || n_fields > 65535 / kNets) return -1;
    if (n_fields > 1 && (heads_stride <= 0 || evec_stride <= 0 || packed_stride < (int64_t)kNets * pack_bytes_per_net(prec) || (packed_stride & 15))) return -1;
    PackArgs a;
    for (int k = 0; k < kNets; ++k) a.net[k] = nets[k];
    a.packed = reinterpret_cast<char*>(packed);
    a.ns = prec;
    a.form = form;
    a.n_fields = n_fields; a.heads_stride = heads_stride; a.evec_stride = evec_stride; a.packed_stride = packed_stride;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (form == 1) {                                                      // products + packing in one launch (no fp32 scratch)
        hipLaunchKernelGGL(dpn_pack_fused_kernel, dim3(kFusedBlocks, kNets * n_fields), dim3(256), 0, s, a);
        return ck(hipGetLastError());
    }
    hipLaunchKernelGGL(dpn_pack_matrices_kernel, dim3(40 + kVecParts, kNets * n_fields), dim3(256), 0, s, a);
    return ck(hipGetLastError());
}

int dpn_pack_weights_form(const DpnNetPtrs nets[DPN_NETS], int prec, int form, void* packed, void* stream) {
    return dpn_pack_weights_batch(nets, 1, 0, 0, prec, form, packed, 0, stream);
}

int dpn_pack_weights(const DpnNetPtrs nets[DPN_NETS], int prec, void* packed, void* stream) {
    return dpn_pack_weights_form(nets, prec, dpn_fwd_form(prec, 0), packed, stream);
}

#ifdef DPN_WGRAD_PHASES
static unsigned* g_wgrad_phases = nullptr;
int dpn_debug_set_wgrad_phases(void* buf) { g_wgrad_phases = reinterpret_cast<unsigned*>(buf); return 0; }   // experiment build only, not in dpn_hip.h
#endif
int dpn_wgrad(int64_t n, int prec, const float* g_out, const void* saved, const void* operands, void* partials, void* stream) {
    if (!g_out || !saved || !operands || !partials || n <= 0 || (prec != 1 && prec != 2)) return -1;
    const SplitPlan plan = choose_plan(pad_points(n), prec);
    WgradArgs a{n, pad_points(n), {plan.s[0], plan.s[1], plan.s[2], plan.s[3]}, const_cast<void*>(saved), const_cast<void*>(operands),
                reinterpret_cast<float*>(partials)};
#ifdef DPN_WGRAD_PHASES
    a.phases = g_wgrad_phases;
#endif
    (void)g_out;   // the per-net cotangents were staged into `operands` by dpn_bwd_points
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(plan.s[1] + plan.s[2] + plan.s[3], kNets);
    if (prec == 1) hipLaunchKernelGGL(dpn_wgrad_kernel<1>, grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL(dpn_wgrad_kernel<2>, grid, dim3(512), 0, s, a);
    return ck(hipGetLastError());
}

// parts: bit 0 = the hyper-network's half (dpn_finish_rows_kernel, dpn_finish_vside_kernel: d w1b1, d w2b2, d evec; dWd, d bd), bit 1 = the half
// that ends in static tensors only (dpn_finish_gside_kernel, dpn_finish_fc2_kernel: d cat_fc1.fc.0 / fc.2, d out_fc) and reads what half 0 left in
// the scratch tail of `partials`: same stream, or another one ordered behind half 0 (a side branch beside the encoder's backward)
int dpn_wgrad_finish_parts(const DpnNetPtrs nets[DPN_NETS], const void* packed, int64_t n, int prec, const void* partials,
                           const DpnNetGradPtrs grads[DPN_NETS], int parts, void* stream) {
    if (!nets || !packed || !partials || !grads || n <= 0 || (prec != 1 && prec != 2) || !(parts & 3)) return -1;
    FinishArgs a;
    for (int k = 0; k < kNets; ++k) { a.net[k] = nets[k]; a.grad[k] = grads[k]; }
    a.packed = reinterpret_cast<const char*>(packed);
    a.partials = reinterpret_cast<const float*>(partials);
    const SplitPlan plan = choose_plan(pad_points(n), prec);
    for (int k = 0; k < 4; ++k) a.splits[k] = plan.s[k];
    a.ns = prec;
    a.n = n;
    // scratch in the tail of the partials buffer (dpn_sizes)
    a.scratch_s1 = const_cast<float*>(a.partials) + (int64_t)plan.most * kNets * kPartFloats;
    a.scratch_s2 = a.scratch_s1 + (int64_t)kNets * 65536;
    a.scratch_mv = a.scratch_s2 + (int64_t)kNets * 256 * 192;
    a.scratch_u = a.scratch_mv + kNets * 256;
    a.scratch_q1 = a.scratch_u + kNets * 256;
    a.scratch_q6 = a.scratch_q1 + kNets * 256;
    a.scratch_sg = a.scratch_q6 + kNets * 256;
    a.scratch_rp = a.scratch_sg + 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (parts & 1) hipLaunchKernelGGL(dpn_finish_rows_kernel, dim3(256, kNets), dim3(256), 0, s, a);
    const int n_v = (parts & 1) ? kVsideBlocks : 0, n_g = (parts & 2) ? kGsideBlocks : 0;
    hipLaunchKernelGGL(dpn_finish_sides_kernel, dim3(n_v + n_g, kNets), dim3(256), 0, s, a, n_v);
    if (parts & 2) hipLaunchKernelGGL(dpn_finish_fc2_kernel, dim3(256, kNets), dim3(256), 0, s, a);
    return ck(hipGetLastError());
}

int dpn_wgrad_finish(const DpnNetPtrs nets[DPN_NETS], const void* packed, int64_t n, int prec, const void* partials,
                     const DpnNetGradPtrs grads[DPN_NETS], void* stream) {
    return dpn_wgrad_finish_parts(nets, packed, n, prec, partials, grads, 3, stream);
}

int dpn_selftest(void* scratch_dev, void* stream) {
    if (!scratch_dev) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* out = reinterpret_cast<float*>(scratch_dev);
    hipLaunchKernelGGL(dpn_selftest_kernel, dim3(1), dim3(64), 0, s, out);
    float host[2048];
    if (hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess) return -2;
    if (hipStreamSynchronize(s) != hipSuccess) return -3;
    // D layout claimed in dpn_layout.h: lane (j = lane&31, h = lane>>5), register r  ->  row drow32(r,h), column j
    for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 16; ++r) {
            const int j = lane & 31, h = lane >> 5, i = drow32(r, h);
            if (host[lane * 16 + r] != (float)i) return 100 + r;
            if (host[1024 + lane * 16 + r] != (float)j) return 200 + r;
        }
    return 0;
}

}  // extern "C"
