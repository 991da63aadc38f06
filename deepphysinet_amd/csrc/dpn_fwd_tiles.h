// Forward + Jacobian kernel of the parity-grade (hi+lo) mode, TILE-SPLIT form.  Included by dpn_point.hip.
//
// Same arithmetic as dpn_fwd_kernel (reference model/variable_net.py:49-87 restated as in DESIGN.md section 3; same packed weight
// stream, same fragment algebra of dpn_layout.h, same accumulation order per output tile: saved state and Jacobian are bit-identical),
// different decomposition:
//
//   dpn_fwd_kernel        one 512-register wave per SIMD owns 32 points and ALL eight output tiles of a layer; activations stay in its
//                         registers, the weight fragments are shared through an LDS-DMA ring (one barrier + 8 DMA issues per 48 MFMAs,
//                         paid with an idle matrix pipe: MFMA busy 45 % in the hi+lo mode).
//   dpn_fwd_tiles_kernel  a workgroup = 4 waves x 256 registers owns 64 points; wave w owns output tiles 2w, 2w+1 of every layer for
//                         both 32-point column tiles (2 x 2 accumulators).  The ACTIVATIONS are what is shared: each layer's epilogue
//                         writes its output to LDS already as next layer's B fragments (the accumulator-is-next-B-operand layout makes
//                         that a linear 16-byte-per-lane store), every wave reads all of them back with conflict-free ds_read_b128.
//                         The WEIGHTS are private to a wave (its two tiles), so they go L2 -> VGPR directly: plain 1-KB-per-instruction
//                         global loads two k-steps ahead, no LDS-DMA, no ring, no counted-wait choreography.
//                         72 KB of LDS and 256 registers => TWO workgroups per CU, i.e. two waves per SIMD that belong to different
//                         workgroups: they never meet at a barrier, so one multiplies while the other packs / stores / waits / builds
//                         features.  Two barriers per LAYER (192 MFMAs per wave) instead of one per 48 MFMAs.
//   cost                  a workgroup streams the net's 1.6 MB of fragments per 64 points instead of per 128 (L2 -> CU traffic x2:
//                         ~30 B/clk/CU at the MFMA rate reached, under the 64 B/clk of the vector memory path; weights are L2 hits).
//
// Per k-step and wave: 4 global loads (A: 2 tiles x hi, lo), 4 ds_read_b128 (B: 2 column tiles x hi, lo), 12 MFMAs.
#pragma once

namespace ts {
constexpr int kVecFloats = kNumVecs * 256 + 4;
template <int NS>
struct Cfg {
    static constexpr int kXBytes = 16 * 2 * NS * 1024;            // [k-step 16][column tile 2][hi | lo][64 lanes][16 B]
    static constexpr int kVecOff = kXBytes;
    static constexpr int kRedOff = kVecOff + kVecFloats * 4;      // 6160 B of vectors: the offset stays 16-byte aligned
    static constexpr int kLdsBytes = kRedOff + 4 * 64 * 4;        // [wave][column tile * 32 + j] partial field sums
};

// LDS-only workgroup barrier: this wave's LDS reads / writes have completed; global loads (weight prefetch) and stores in flight STAY
// in flight (a plain __syncthreads() would drain vmcnt as well)
DEV void barrier_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct NoSide { DEV void operator()(int) const {} };

// Ablation builds (tools/variant_build.py; wrong results on purpose, timing only): TS_ABL_NOMFMA keeps the operands alive and drops the
// products, TS_ABL_NOSINCOS replaces the feature evaluation by one multiply, TS_ABL_NOALOAD multiplies with whatever is in the registers.
#ifdef TS_ABL_NOSINCOS
template <int NS> DEV void ts_sincos(float th, float& s, float& c) { s = th; c = th * 0.5f; }
#else
template <int NS> DEV void ts_sincos(float th, float& s, float& c) { sincos_t<NS>(th, s, c); }
#endif

// SWAP = false: a = weight fragment (A operand), b = activation fragment (B operand): Out[channel][point], the chained layout.
// SWAP = true : the activation fragment is the A operand, the weight fragment the B operand: Out[point][channel] -- channel per lane, the
//               K-operand layout of the weight-gradient GEMMs (dpn_bwd_tiles_kernel's Z).  Product order as mma_block in both cases.
template <int NS, bool SWAP = false>
DEV void mma3(const u32x4 (&a)[NS], const u32x4 (&b)[NS], f32x16& acc) {
#ifdef TS_ABL_NOMFMA
    if constexpr (NS == 2) asm volatile("" ::"v"(a[0]), "v"(a[1]), "v"(b[0]), "v"(b[1]));
    else asm volatile("" ::"v"(a[0]), "v"(b[0]));
    return;
#endif
    if constexpr (SWAP) {
        if constexpr (NS == 2) {
            acc = mfma(as_bf(b[1]), as_bf(a[0]), acc);
            acc = mfma(as_bf(b[0]), as_bf(a[1]), acc);
        }
        acc = mfma(as_bf(b[0]), as_bf(a[0]), acc);
    } else {
        if constexpr (NS == 2) {
            acc = mfma(as_bf(a[0]), as_bf(b[1]), acc);
            acc = mfma(as_bf(a[1]), as_bf(b[0]), acc);
        }
        acc = mfma(as_bf(a[0]), as_bf(b[0]), acc);
    }
}

// acc[t][p] += W[tile t][k] * X[k][column tile p] over NK k-steps.  wg: this wave's first tile chunk in the packed stream (wave-uniform;
// the second tile's chunk follows it), xl: LDS X + lane * 16.  A fragments kPF - 1 k-steps ahead, B fragments one.
// The first kPF - 1 k-steps' A fragments are loaded by gemm_head, which the kernel calls BEFORE the previous layer's epilogue: the
// weight stream of a layer then starts under that epilogue (packing, saved-state stores, the two barriers) instead of cold behind it --
// and in front of its stores: vmcnt retires in order, a load issued behind the saved-state stores would wait for them as well.
#ifndef TS_PF
#define TS_PF 3      // two k-steps ahead: with the deferred saved-state hand-over (TS_DEFER_SAVES) a fourth slot spills 44 registers (measured slower)
#endif
// Issue priority between the two waves of a SIMD (they belong to different workgroups): 0 = none, 1 = s_setprio 1 around every k-step's
// MFMAs, 2 = s_setprio 1 everywhere EXCEPT the multiply loops (the feature / epilogue / store phases are a workgroup's serial chain; a
// multiplying wave needs one issue slot in eight)
#ifndef TS_PRIO
#define TS_PRIO 2
#endif
// Saved-state hand-over (V, T1, M2 as K-layout rows: two transposing MFMAs, eight packs and two streaming stores per plane and tile) issued
// k-step by k-step inside the NEXT layer's multiply loop instead of in the serial epilogue between two barriers (nobody in the kernel waits
// for it).  0 = in the epilogue.
#ifndef TS_DEFER_SAVES
#define TS_DEFER_SAVES 1
#endif
#ifndef TS_SCHED_GROUPS
#define TS_SCHED_GROUPS 0
#endif
constexpr int kPF = TS_PF;
template <int NS, int NT> struct Head { u32x4 a[kPF - 1][NT][NS]; };

// Weight fragments come through a buffer descriptor (SGPR base, the lane's 16-byte slot as the only VGPR offset, fragment index as scalar /
// immediate offset): no 64-bit address arithmetic between the MFMAs.  tools/microbench/l2_stream2.hip, this loop shape at 3 MFMAs per
// loaded KB: global_load with VGPR addresses 48 % of the bf16 peak, buffer_load 65 %, s_setprio 1 around the MFMAs 62 %.
template <int NS, int NK, int NT>
struct WSrc {
    __amdgpu_buffer_rsrc_t rs;
    int voff;
    int so[NT];                                  // running scalar offsets of the next k-step, one per tile (SALU adds; kept opaque so that
                                                 // the unrolled loop does not turn them into a hundred constants in as many SGPRs)
    DEV void init(const char* wg, const int lane, const int ks0) {
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wg), 0, NT * NK * NS * 1024, 0x00020000);
        voff = lane * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t) { so[t] = (t * NK + ks0) * NS * 1024; asm volatile("" : "+s"(so[t])); }
    }
    DEV void next(u32x4 (&dst)[NT][NS]) {        // fragments of the next k-step
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#ifdef TS_ABL_NOALOAD
                asm volatile("" : "=v"(dst[t][s]));
#else
                dst[t][s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + s * 1024, so[t], 0));
#endif
            }
            so[t] += NS * 1024;
            asm volatile("" : "+s"(so[t]));
        }
    }
};
template <int NS, int NK, int NT>
DEV void gemm_head(const char* wg, const int lane, Head<NS, NT>& H) {
    WSrc<NS, NK, NT> src;
    src.init(wg, lane, 0);
#pragma unroll
    for (int k = 0; k < kPF - 1; ++k) src.next(H.a[k]);
}
// side(ks): work of the PREVIOUS layer that nobody waits for (its saved-state transposes and stores), issued k-step by k-step in the shadow
// of this layer's MFMAs instead of in the serial epilogue between two barriers
template <int NS, int NK, int NT, bool SWAP = false, class Side = NoSide, bool PIN = true, bool SG = PIN>
DEV void gemm(const char* wg, const char* xl, const int lane, const Head<NS, NT>& H, f32x16 (&acc)[2][2], const Side& side = Side()) {
    static_assert(NK >= kPF, "k-steps per chunk");
    WSrc<NS, NK, NT> src;
    src.init(wg, lane, kPF - 1);
    u32x4 A[kPF][NT][NS];
    u32x4 B[2][2][NS];
    auto loadB = [&](const int ks, const int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int s = 0; s < NS; ++s) B[slot][p][s] = *reinterpret_cast<const u32x4*>(xl + ((ks * 2 + p) * NS + s) * 1024);
    };
#pragma unroll
    for (int k = 0; k < kPF - 1; ++k)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s = 0; s < NS; ++s) A[k][t][s] = H.a[k][t][s];
    loadB(0, 0);
#if TS_PRIO == 2
    __builtin_amdgcn_s_setprio(0);            // multiply phases at low priority, everything else (the serial chain of a workgroup) at high
#endif
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        if (ks + kPF - 1 < NK) src.next(A[(ks + kPF - 1) % kPF]);
        if (ks + 1 < NK) loadB(ks + 1, (ks + 1) & 1);
#if TS_SCHED_GROUPS
        // (SG: the forward kernels; the backward stage-1 kernel lives on 168 registers and spills with the longer live ranges)
        // the next k-step's B fragments are READ (4 ds_read_b128) in front of this k-step's MFMAs, not behind them where hipcc's scheduler sinks them to
        // shorten their live ranges (the read latency is then exposed in front of every k-step when no second multiplying wave covers it)
        if (SG && ks + 1 < NK) {
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * NS, 0);        // DS read
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * (NS == 2 ? 3 : 1), 0);   // MFMA
        }
#endif
#if TS_PRIO == 1
        __builtin_amdgcn_s_setprio(1);        // the multiplying wave wins issue arbitration against its SIMD partner's loads / packing
#endif
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p) mma3<NS, SWAP>(A[ks % kPF][t], B[ks & 1][p], acc[t][p]);
#if TS_PRIO == 1
        __builtin_amdgcn_s_setprio(0);
#endif
        side(ks);
        if constexpr (PIN) {
        // k-steps stay k-steps: the MFMAs are pure values without a position of their own, and instruction selection is free to emit all of a
        // layer's 144-192 of them AFTER the fragment loads of all its k-steps (seen after an unrelated change four layers later: 204 spilled
        // registers in the first layer's loop, every load followed by s_waitcnt vmcnt(0) + a scratch store, 628 us instead of 478).  The empty
        // volatile statement gives the accumulators a place in the order of the loads' running offsets (WSrc::next), which are volatile too.
        // (PIN = false in the backward kernel: its loops carry side work in every layer, which holds the order by itself, and the pin costs it
        // 19 us -- 241 -> 260 us measured on one box.)
        asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));
        }
    }
#if TS_PRIO == 2
    __builtin_amdgcn_s_setprio(1);
#endif
}

template <int NS>
DEV void x_store(char* xl, const int ks, const int p, const Frag<NS>& f) {
#pragma unroll
    for (int s = 0; s < NS; ++s) *reinterpret_cast<u32x4*>(xl + ((ks * 2 + p) * NS + s) * 1024) = f.w[s];
}

DEV void acc_init(f32x16& acc, const float* vec, const int which, const int h, const int T, const float scale) {
    const f32x4* v = reinterpret_cast<const f32x4*>(vec + which * 256 + h * 128 + T * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 x = v[q];
        acc[4 * q] = scale * x[0]; acc[4 * q + 1] = scale * x[1]; acc[4 * q + 2] = scale * x[2]; acc[4 * q + 3] = scale * x[3];
    }
}

struct Ident { u32x4 a, b; };
DEV Ident make_ident(const int j, const int h) {          // the identity B fragments of lane_init (MFMA transposes of the saved state)
    Ident I;
    const int mine = (((j >> 3) & 1) == h) ? (j & 7) : -1;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const u32 v = ((mine == 2 * p) ? 0x3F80u : 0u) | ((mine == 2 * p + 1) ? 0x3F800000u : 0u);
        I.a[p] = (j < 16) ? v : 0u;
        I.b[p] = (j >= 16) ? v : 0u;
    }
    return I;
}
// one plane (hi or lo) of one column tile: two transposing MFMAs, eight packs, two 16-byte streaming stores
DEV void save_plane_k(const KMat& m, const int net, const int nstore, const int s, const int64_t tile32, const int ct, const int lane, const Ident& I,
                      const bool zero, u32x4 a0, u32x4 a1) {
    if (zero) { a0 = (u32x4)0u; a1 = (u32x4)0u; }
    f32x16 d = (f32x16)0.f;
    d = mfma(as_bf(a0), as_bf(I.a), d);
    d = mfma(as_bf(a1), as_bf(I.b), d);
    store_d_as_k(m, net, nstore, s, tile32, ct, lane, d);
}
// store_tile_k of the ring kernel: fragments (k-steps 2ct, 2ct+1) of one column tile -> K-layout rows of the 32-point tile
template <int NS, int NSTORE>
DEV void save_tile_k(const KMat& m, const int net, const int64_t tile32, const int ct, const int lane, const Ident& I, const bool zero,
                     const Frag<NS>& f0, const Frag<NS>& f1) {
#pragma unroll
    for (int s = 0; s < NSTORE; ++s) {
        u32x4 a0 = f0.w[s], a1 = f1.w[s];
        if (zero) { a0 = (u32x4)0u; a1 = (u32x4)0u; }
        f32x16 d = (f32x16)0.f;
        d = mfma(as_bf(a0), as_bf(I.a), d);
        d = mfma(as_bf(a1), as_bf(I.b), d);
        store_d_as_k(m, net, NSTORE, s, tile32, ct, lane, d);
    }
}

// the normalised coordinate xi_c of point pc: x / dx / (lon-1), two fp32 divisions in this order (interface_physics.py:324-326); t: / span / 1.
// Evaluated ONCE per lane, point and coordinate by the kernels and handed to the helpers below (each of them used to divide for itself, behind
// barriers where the compiler cannot merge the calls: 18 divisions of ~10 instructions in the forward kernel; 10 now, 8 of them for xi)
template <class Args>
DEV float xi_of(const Args& a, const int c, const int64_t pc) {
    const float* src = (c == 0) ? a.x : (c == 1) ? a.y : a.t;
    const float d1 = (c == 0) ? a.geo.dx : (c == 1) ? a.geo.dy : a.geo.pred_t_span;
    const float d2 = (c == 0) ? a.geo.lon_m1 : (c == 1) ? a.geo.lat_m1 : 1.0f;
    return src[pc] / d1 / d2;
}
// the coordinate features of k-step ks (0..11) for the lane's point (xi: its coordinate ks >> 2): one B fragment (hi [+ lo])
template <int NS, class Args>
DEV void pe3_frag(Frag<NS>& f, const Args& a, const int ks, const int h, const float xi) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s, co;
        ts_sincos<NS>(xi * a.freqs[8 * (ks & 3) + 4 * h + q], s, co);
        frag_set2<NS>(f, q, s, co);
    }
}
// the data features (SineCosPE(6,16) of coord_data, variable_net.py:73) of k-step ks (0..11)
template <int NS, class Args>
DEV void pe6_frag(Frag<NS>& f, const Args& a, const int ks, const int h, const int64_t pc, const float g = 1.0f) {
    const float v = a.coord_data[pc * 6 + (ks >> 1)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s, co;
        ts_sincos<NS>(v * a.freqs[32 + 8 * (ks & 1) + 4 * h + q], s, co);
        frag_set2<NS>(f, q, g * s, g * co);
    }
}
// the same, and dot += sum over the fragment's eight features of feature * bv[slot] (bv: a 192-vector in PE6 slot order 16 ks + 8 h + e, in LDS)
template <int NS, class Args>
DEV void pe6_frag_dot(Frag<NS>& f, const Args& a, const int ks, const int h, const int64_t pc, const float* bv, float& dot) {
    const float v = a.coord_data[pc * 6 + (ks >> 1)];
    const f32x4* b4 = reinterpret_cast<const f32x4*>(bv + 16 * ks + 8 * h);
    const f32x4 b0 = b4[0], b1 = b4[1];
    const float bb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s, co;
        ts_sincos<NS>(v * a.freqs[32 + 8 * (ks & 1) + 4 * h + q], s, co);
        frag_set2<NS>(f, q, s, co);
        dot = fmaf(s, bb[2 * q], dot);
        dot = fmaf(co, bb[2 * q + 1], dot);
    }
}
// backward: Z0 = g * pe + gJ_c * d pe / d xi_c for k-step ks (coordinate c = ks >> 2), build_pe3<BWD> of the ring kernels
template <int NS, class Args>
DEV void z0_frag(Frag<NS>& f, const Args& a, const int ks, const int h, const float xi, const float g, const float gjc, float (&sc)[8]) {   // sc: (s, co) x 4, the table form's features
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float fr = a.freqs[8 * (ks & 3) + 4 * h + q];
        float s, co;
        ts_sincos<NS>(xi * fr, s, co);
        const float gf = gjc * fr;
        frag_set2<NS>(f, q, fmaf(g, s, gf * co), fmaf(g, co, -gf * s));
        sc[2 * q] = s; sc[2 * q + 1] = co;
    }
}
// d pe3 / d xi_c for the 16 accumulator registers of gpe tile 2c + t (register pair rp = one angle: k-step 2T + (rp >> 2) of the coordinate PE)
template <int NS, class Args>
DEV void dpe_tile(float (&d)[16], const Args& a, const int t, const int h, const float xi) {
#pragma unroll
    for (int rp = 0; rp < 8; ++rp) {
        const int r = 2 * rp;
        const float fr = a.freqs[8 * ((2 * t + (r >> 3)) & 3) + 4 * h + ((r & 7) >> 1)];
        float s, co;
        ts_sincos<NS>(xi * fr, s, co);
        d[r] = fr * co;
        d[r + 1] = -fr * s;
    }
}
// z0_frag + gH_c * d2 pe / d xi_c^2 = -gH_c fr^2 pe (dpn_bwd_tiles_deriv_kernel; build_z0_derivs of the ring kernels)
template <int NS, class Args>
DEV void z0_frag_derivs(Frag<NS>& f, const Args& a, const int ks, const int h, const float xi, const float g, const float gjc, const float ghc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float fr = a.freqs[8 * (ks & 3) + 4 * h + q];
        float s, co;
        ts_sincos<NS>(xi * fr, s, co);
        const float gf = gjc * fr;
        const float gs = fmaf(-ghc * fr, fr, g);
        frag_set2<NS>(f, q, fmaf(gs, s, gf * co), fmaf(gs, co, -gf * s));
    }
}
// dpe_tile, and d2 = d2 pe3 / d xi_c^2 = -fr^2 pe3, d3 = d3 pe3 / d xi_c^3 = -fr^2 d (dpn_fwd_tiles_deriv_kernel; d is formed exactly as dpe_tile forms it)
template <int NS, class Args>
DEV void dpe_tile_derivs(float (&d)[16], float (&d2)[16], float (&d3)[16], const Args& a, const int t, const int h, const float xi) {
#pragma unroll
    for (int rp = 0; rp < 8; ++rp) {
        const int r = 2 * rp;
        const float fr = a.freqs[8 * ((2 * t + (r >> 3)) & 3) + 4 * h + ((r & 7) >> 1)];
        float s, co;
        ts_sincos<NS>(xi * fr, s, co);
        d[r] = fr * co;
        d[r + 1] = -fr * s;
        const float f2 = fr * fr;
        d2[r] = -f2 * s;
        d2[r + 1] = -f2 * co;
        d3[r] = -f2 * d[r];
        d3[r + 1] = -f2 * d[r + 1];
    }
}
}  // namespace ts

// Experiment build (-DDPN_TIMELINE -DTS_TIMELINE, tools/tiles_timeline.py): lane 0 of every wave writes the shader clock at the phase
// boundaries below to a.timeline[workgroup][wave][stamp]
#if defined(TS_TIMELINE) && defined(DPN_TIMELINE)
#define TS_STAMP(I) do { if (a.timeline && lane == 0) a.timeline[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + w) * 48 + (I)] = (unsigned)__builtin_readcyclecounter(); } while (0)
#else
#define TS_STAMP(I) do { } while (0)
#endif

// the tile-split kernels (dpn_fwd_tiles_kernel, dpn_bwd_tiles_kernel) and their derivative forms (dpn_fwd_tiles_deriv_kernel, dpn_bwd_tiles_deriv_kernel)
#define DPN_DERIV 0
#include "dpn_tiles_kernels.inc"
#undef DPN_DERIV
#define DPN_DERIV 1
#include "dpn_tiles_kernels.inc"
#undef DPN_DERIV
