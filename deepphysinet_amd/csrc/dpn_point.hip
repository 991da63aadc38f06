// MI355X (gfx950 / CDNA4) point path of the DeepPhysiNet physics-informed training step: the per-point forward and backward kernels.
//
// Reference behaviour restated here (paths relative to the reference's DeepPhysiNet tree):
//   model/variable_net.py:49-87      VariableNet.forward (hyper-network coordinate MLP)
//   model/physics_net.py:49-54       six VariableNets share coord / coord_data
//   utils/position_encoding.py:35-50 SineCosPE
//   interface/interface_physics.py:90-95    gradient()  (autograd.grad, create_graph)
//   interface/interface_physics.py:322-332  encoding_coord
// DESIGN.md section 3 derives the restructured algorithm (reverse-sweep Jacobian, rank-1 fc.2,
// single-GEMM weight gradients) implemented here and in dpn_wgrad.hip; oracle/kernel_model.py states it in torch.
//
// Kernel inventory
//   dpn_fwd_kernel      fused PE + MLP chain + reverse sweep + Jacobian contraction (activations never leave registers)
//   dpn_bwd_kernel      per-point cotangent streams -> operands of the weight-gradient reductions
//   dpn_fwd_deriv_kernel / dpn_bwd_deriv_kernel    the same with second / third coordinate derivatives (dpn_ring_kernels.inc, compiled twice)
//   dpn_fwd_tiles_* / dpn_bwd_tiles_*              the tile-split forms of the four (dpn_fwd_tiles.h; the hi+lo mode's default)
// No kernel in this file uses atomics: every reduction is fixed-order, the whole step is bitwise reproducible.
//
// The only unit of the family compiled with -mllvm -amdgpu-mfma-vgpr-form (deepphysinet_amd/build.py): accumulators in VGPRs -- hipcc otherwise
// parks them in AGPRs and pays a v_accvgpr_read for every element an epilogue touches, 1775 of the forward kernel's 6457 VALU instructions.
// (The weight-gradient kernel measures slower in that form: dpn_wgrad.hip is built without it.)
#include "dpn_point_common.h"
#include "dpn_sincos.h"

// ------------------------------------------------------------------------------------------------ operand fragments
template <int NS>
struct Frag {                                 // one k-step operand fragment: 8 bf16 per lane as 4 packed words, hi [+ lo]
    u32x4 w[NS];
};
template <int NS>
DEV void frag_set2(Frag<NS>& f, const int p, float a, float b) {      // elements 2p, 2p+1
    const u32 hi = pack2(a, b);
    f.w[0][p] = hi;
    if constexpr (NS == 2) f.w[1][p] = pack2(a - bf_lo(hi), b - bf_hi(hi));
}

// (max(x, 0) used to be ONE inline-asm v_max_f32 here -- fmaxf() makes hipcc canonicalise its operand first, an extra v_max x,x per
//  element.  Inline asm is invisible to the compiler's hazard recogniser: when the scheduler made that v_max the FIRST reader of an MFMA
//  result, no wait states were inserted and it read the accumulator before the matrix core had written it (3 % errors in the hi+lo mode,
//  depending on unrelated code around it).  The ReLU is now a select on the compare that builds the mask bit; tools/mfma_hazard_check.py
//  scans the generated assembly for any inline-asm reader of a fresh MFMA result.)

// sincos_precise (Cody-Waite reduction by pi/2 + minimax polynomials, the quadrant as bit arithmetic): dpn_sincos.h, shared with host code
// NS == 1 (plain bf16 operands): the features are rounded to 8 mantissa bits anyway -> hardware v_sin/v_cos
template <int NS>
DEV void sincos_t(float th, float& s, float& c) {
    if constexpr (NS == 1) { s = __sinf(th); c = __cosf(th); }
    else sincos_precise(th, s, c);
}

// ------------------------------------------------------------------------------------------------ weight stream
// All four waves of a workgroup walk the same packed weight block chunk by chunk (one chunk = the A fragments of one 32-row
// output tile for 12 or 16 k-steps).  Chunks travel global -> LDS by LDS-DMA (global_load_lds_dwordx4: 1 KB per
// wave-instruction, no staging registers, no ds_write pass) into a ring of 4 slots, three chunks ahead of the MFMAs.
// Per chunk: counted s_waitcnt vmcnt (my pieces of chunk c have landed; the DMAs of c+1, c+2 stay in flight), one raw
// s_barrier (everybody's pieces have landed, everybody is done with the slot refilled next), issue chunk c+3, multiply chunk c.
// vmcnt retires in order on gfx9-class hardware (the compiler's own counted waits rely on it); other VMEM traffic of the wave
// (saved-state stores) only makes the counted wait stricter, never weaker.
DEV void wait_vmcnt_n(const int n) {        // n is a compile-time constant after unrolling: the switch folds to one s_waitcnt
    switch (n) {
        case 0: wait_vmcnt<0>(); break; case 1: wait_vmcnt<1>(); break; case 2: wait_vmcnt<2>(); break; case 3: wait_vmcnt<3>(); break; case 4: wait_vmcnt<4>(); break; case 5: wait_vmcnt<5>(); break; case 6: wait_vmcnt<6>(); break; case 7: wait_vmcnt<7>(); break; case 8: wait_vmcnt<8>(); break; case 9: wait_vmcnt<9>(); break; case 10: wait_vmcnt<10>(); break; case 11: wait_vmcnt<11>(); break; case 12: wait_vmcnt<12>(); break; case 13: wait_vmcnt<13>(); break; case 14: wait_vmcnt<14>(); break; case 15: wait_vmcnt<15>(); break; case 16: wait_vmcnt<16>(); break; case 17: wait_vmcnt<17>(); break; case 18: wait_vmcnt<18>(); break; case 19: wait_vmcnt<19>(); break; case 20: wait_vmcnt<20>(); break; case 21: wait_vmcnt<21>(); break; case 22: wait_vmcnt<22>(); break; case 23: wait_vmcnt<23>(); break; case 24: wait_vmcnt<24>(); break; case 25: wait_vmcnt<25>(); break; case 26: wait_vmcnt<26>(); break; case 27: wait_vmcnt<27>(); break; case 28: wait_vmcnt<28>(); break; case 29: wait_vmcnt<29>(); break; case 30: wait_vmcnt<30>(); break; case 31: wait_vmcnt<31>(); break; case 32: wait_vmcnt<32>(); break; case 33: wait_vmcnt<33>(); break; case 34: wait_vmcnt<34>(); break; case 35: wait_vmcnt<35>(); break; case 36: wait_vmcnt<36>(); break; case 37: wait_vmcnt<37>(); break; case 38: wait_vmcnt<38>(); break; case 39: wait_vmcnt<39>(); break; case 40: wait_vmcnt<40>(); break; case 41: wait_vmcnt<41>(); break; case 42: wait_vmcnt<42>(); break; case 43: wait_vmcnt<43>(); break; case 44: wait_vmcnt<44>(); break; case 45: wait_vmcnt<45>(); break; case 46: wait_vmcnt<46>(); break; case 47: wait_vmcnt<47>(); break; case 48: wait_vmcnt<48>(); break;
        default: wait_vmcnt<0>(); break;
    }
}
// k-steps of chunk c in stream order (dpn_layout.h): w1 8x12 | w2 8x16 | Wd 8x12 | W1 8x16 | W1^T 8x16 | w2^T 8x16 | w1^T 6x16
DPN_HD __attribute__((always_inline)) int stream_nk(int c, int end) { return (c < 0 || c >= end) ? 0 : (c < 8 ? 12 : c < 16 ? 16 : c < 24 ? 12 : 16); }

template <int NS>
struct Pipe {
    static constexpr int kRing = 4;
    static constexpr int kSlotBytes = 16 * 1024 * NS;
#ifdef DPN_FWD_PHASES
    u32 ph[6] = {0, 0, 0, 0, 0, 0}, pc0 = 0;      // experiment build: cycles in vmcnt wait / barrier / DMA issue / reads + MFMAs / last block / epilogue
#define DPN_PH_CLOCK(V) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); V = (u32)t_; } while (0)
#endif
    const char* g;       // global address of the next chunk to issue (wave-uniform)
    char* lds;
    int end;             // number of chunks this kernel may touch (54 forward, 24 backward)
    int wave, lane;

    DEV void init(const void* gsrc, char* lds_base, int end_chunks) {
        g = reinterpret_cast<const char*>(gsrc); lds = lds_base; end = end_chunks;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); lane = threadIdx.x & 63;
    }
#ifdef DPN_ABL_HALFDMA                        // ablation (wrong results): half of each chunk is fetched -- is the step time the DMA's?
    DEV static int dmas(int nk) { return nk * NS / 8; }
#elif defined(DPN_ABL_QUARTERDMA)
    DEV static int dmas(int nk) { return nk * NS / 16; }
#else
    DEV static int dmas(int nk) { return nk * NS / 4; }                 // DMA instructions per wave for a chunk of nk k-steps
#endif
    DEV void issue(const int c) {                                       // chunk c -> slot c % 4
        const int n = dmas(stream_nk(c, end));
        char* slot = lds + (c & (kRing - 1)) * kSlotBytes;
        // The slot is a byte image of the chunk; wave w copies the CONTIGUOUS quarter [w n KiB, (w+1) n KiB) of it, so that its pieces
        // differ only in the instruction's immediate offset (which moves the global and the LDS address alike, < 4 KiB): one
        // address pair + one M0 per four pieces instead of five address instructions per piece (a sixth of the kernel's issue slots).
        const char* src = g + wave * (n * 1024) + lane * 16;
        char* dst = slot + wave * (n * 1024);
        if (n > 0) dma16_at<0>(src, dst);
        if (n > 1) dma16_at<1024>(src, dst);
        if (n > 2) dma16_at<2048>(src, dst);
        if (n > 3) dma16_at<3072>(src, dst);
        if constexpr (NS == 2) {
            if (n > 4) dma16_at<0>(src + 4096, dst + 4096);
            if (n > 5) dma16_at<1024>(src + 4096, dst + 4096);
            if (n > 6) dma16_at<2048>(src + 4096, dst + 4096);
            if (n > 7) dma16_at<3072>(src + 4096, dst + 4096);
        }
        g += n * 4096;
    }
    DEV void prime() { issue(0); issue(1); issue(2); }
    // (Counting the saved-state stores of the last three epilogues into the allowed vmcnt -- they retire in order with the DMAs, so
    //  leaving them out makes the wait stricter than needed -- was measured with the timeline probe: no change, 3356 vs 3097 cycles per
    //  fc1 chunk in the hi+lo mode.  Not kept.)
    DEV void acquire(const int c) {                                     // after this, every wave may read chunk c from LDS
        __builtin_amdgcn_sched_barrier(0);      // keep the scheduler from stretching live ranges across pipeline steps
#ifdef DPN_FWD_PHASES
        u32 c0, c1, c2, c3;
        DPN_PH_CLOCK(c0);
        if (pc0) ph[5] += c0 - pc0;             // since the end of the previous chunk's multiply: its epilogue
#endif
        wait_vmcnt_n(dmas(stream_nk(c + 1, end)) + dmas(stream_nk(c + 2, end)));
#ifdef DPN_FWD_PHASES
        DPN_PH_CLOCK(c1);
#endif
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // compiler-level ordering only: no s_waitcnt is emitted
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef DPN_FWD_PHASES
        DPN_PH_CLOCK(c2);
#endif
        issue(c + 3);
#ifdef DPN_FWD_PHASES
        DPN_PH_CLOCK(c3);
        ph[0] += c1 - c0; ph[1] += c2 - c1; ph[2] += c3 - c2; pc0 = c3;
#endif
        __builtin_amdgcn_sched_barrier(0);
    }
    DEV unsigned buf(const int c) const {                               // LDS byte address of slot c % 4
        return (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds + (c & (kRing - 1)) * kSlotBytes;
    }
    DEV void drain() { wait_vmcnt<0>(); }                               // no DMA may outlive the workgroup's LDS allocation
};

// SWAP = false: Out[channel][point] (+)= W[channel][k] * Act[k][point]   (weights as A, chained layout)
// SWAP = true : Out[point][channel] (+)= Act[point][k] * W[channel][k]   (same packed weights as B: the result lands
//               channel-per-lane / points-in-registers, which is the K-operand layout of the weight-gradient GEMMs)
// The A fragments are read with inline-asm ds_read_b128: hipcc orders every LDS read it can see behind ALL outstanding
// LDS-DMA (s_waitcnt vmcnt(0)), which would drain the three chunks in flight at every step.  The reads of a chunk are
// issued in blocks of four k-steps, one block ahead of the MFMAs that consume them, with counted lgkmcnt waits
// (LDS operations retire in order; anything else on the counter only makes the wait stricter).
template <int NS>
struct WBlock { u32x4 w[4][NS]; };

template <int NS, int KS0>
DEV void lds_load_block(WBlock<NS>& b, unsigned addr) {
    if constexpr (NS == 1) {
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=&v"(b.w[0][0]), "=&v"(b.w[1][0]), "=&v"(b.w[2][0]), "=&v"(b.w[3][0])
                     : "v"(addr), "n"((KS0 + 0) * 1024), "n"((KS0 + 1) * 1024), "n"((KS0 + 2) * 1024), "n"((KS0 + 3) * 1024)
                     : "memory");
    } else {
        asm volatile("ds_read_b128 %0, %8 offset:%9\n\tds_read_b128 %1, %8 offset:%10\n\tds_read_b128 %2, %8 offset:%11\n\tds_read_b128 %3, %8 offset:%12\n\t"
                     "ds_read_b128 %4, %8 offset:%13\n\tds_read_b128 %5, %8 offset:%14\n\tds_read_b128 %6, %8 offset:%15\n\tds_read_b128 %7, %8 offset:%16"
                     : "=&v"(b.w[0][0]), "=&v"(b.w[0][1]), "=&v"(b.w[1][0]), "=&v"(b.w[1][1]), "=&v"(b.w[2][0]), "=&v"(b.w[2][1]), "=&v"(b.w[3][0]), "=&v"(b.w[3][1])
                     : "v"(addr), "n"((KS0 * 2 + 0) * 1024), "n"((KS0 * 2 + 1) * 1024), "n"((KS0 * 2 + 2) * 1024), "n"((KS0 * 2 + 3) * 1024),
                       "n"((KS0 * 2 + 4) * 1024), "n"((KS0 * 2 + 5) * 1024), "n"((KS0 * 2 + 6) * 1024), "n"((KS0 * 2 + 7) * 1024)
                     : "memory");
    }
}
// wait until at most N LDS operations issued after this block are outstanding; the "+v" ties keep every consumer below the wait
template <int NS, int N>
DEV void lds_wait_block(WBlock<NS>& b) {
    if constexpr (NS == 1)
        asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(b.w[0][0]), "+v"(b.w[1][0]), "+v"(b.w[2][0]), "+v"(b.w[3][0]) : "n"(N) : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(b.w[0][0]), "+v"(b.w[0][1]), "+v"(b.w[1][0]), "+v"(b.w[1][1]), "+v"(b.w[2][0]), "+v"(b.w[2][1]),
                     "+v"(b.w[3][0]), "+v"(b.w[3][1]) : "n"(N) : "memory");
    // hipcc would otherwise hoist register-only MFMAs above the asm wait.  VALU / SALU / VMEM / transcendental instructions
    // (the previous tile's epilogue) MAY cross: they are what fills the issue slots in the shadow of the MFMAs.
    __builtin_amdgcn_sched_barrier(0x2 | 0x4 | 0x10 | 0x20 | 0x40 | 0x400);
}

template <int NS, bool SWAP, int KS0>
DEV void mma_block(const WBlock<NS>& b, const Frag<NS>* act, f32x16& acc) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bf16x8 whi = as_bf(b.w[k][0]);
        if constexpr (NS == 2) {
            const bf16x8 wlo = as_bf(b.w[k][1]);
            if constexpr (SWAP) { acc = mfma(as_bf(act[KS0 + k].w[1]), whi, acc); acc = mfma(as_bf(act[KS0 + k].w[0]), wlo, acc); }
            else { acc = mfma(whi, as_bf(act[KS0 + k].w[1]), acc); acc = mfma(wlo, as_bf(act[KS0 + k].w[0]), acc); }
        }
        if constexpr (SWAP) acc = mfma(as_bf(act[KS0 + k].w[0]), whi, acc);
        else acc = mfma(whi, as_bf(act[KS0 + k].w[0]), acc);
    }
}

template <int NS, int NK, bool SWAP>
DEV void mma_chunk(unsigned slot_addr, const Frag<NS>* act, f32x16& acc) {
    static_assert(NK == 12 || NK == 16, "chunks are 12 or 16 k-steps");
    const unsigned addr = slot_addr + (threadIdx.x & 63) * 16;
    WBlock<NS> b0, b1;
    lds_load_block<NS, 0>(b0, addr);
    lds_load_block<NS, 4>(b1, addr);
    lds_wait_block<NS, 4 * NS>(b0);
    mma_block<NS, SWAP, 0>(b0, act, acc);
    lds_load_block<NS, 8>(b0, addr);
    lds_wait_block<NS, 4 * NS>(b1);
    mma_block<NS, SWAP, 4>(b1, act, acc);
    if constexpr (NK == 16) {
        lds_load_block<NS, 12>(b1, addr);
        lds_wait_block<NS, 4 * NS>(b0);
        mma_block<NS, SWAP, 8>(b0, act, acc);
        lds_wait_block<NS, 0>(b1);
        mma_block<NS, SWAP, 12>(b1, act, acc);
    } else {
        lds_wait_block<NS, 0>(b0);
        mma_block<NS, SWAP, 8>(b0, act, acc);
    }
}

// ------------------------------------------------------------------------------------------------ per-lane context
struct Lane {
    int lane, j, h;
    int64_t pt;        // global point index of this lane's column
    bool valid;
    float xi[3];       // normalised coordinates
    float fr32[16];    // freq32[8*(m>>2) + 4h + (m&3)]
    float fr16[8];     // freq16[8*(m>>2) + 4h + (m&3)]
    u32x4 idA, idB;       // identity B-operand fragments for the MFMA transposes (columns 0..15 / 16..31)
};

DEV void lane_init(Lane& L, const float* x, const float* y, const float* t, int64_t n, const float* freqs, const DpnGeometry& geo,
                   int64_t tile32) {
    L.lane = threadIdx.x & 63;
    L.j = L.lane & 31;
    L.h = L.lane >> 5;
    L.pt = tile32 * 32 + L.j;
    L.valid = L.pt < n;
    const int64_t pc = L.valid ? L.pt : (n - 1);
    L.xi[0] = L.xi[1] = L.xi[2] = 0.f;
    if (x) {
        L.xi[0] = x[pc] / geo.dx / geo.lon_m1;   // interface_physics.py:324-326 (two fp32 divisions, like the reference)
        L.xi[1] = y[pc] / geo.dy / geo.lat_m1;
        L.xi[2] = t[pc] / geo.pred_t_span;
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) L.fr32[m] = freqs[8 * (m >> 2) + 4 * L.h + (m & 3)];
#pragma unroll
    for (int m = 0; m < 8; ++m) L.fr16[m] = freqs[32 + 8 * (m >> 2) + 4 * L.h + (m & 3)];
    // identity: column jj of a 32-column tile <- k-slot (h = (jj>>3)&1, e = jj&7) of k-step (jj>>4)
    const int mine = (((L.j >> 3) & 1) == L.h) ? (L.j & 7) : -1;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const u32 v = ((mine == 2 * p) ? 0x3F80u : 0u) | ((mine == 2 * p + 1) ? 0x3F800000u : 0u);
        L.idA[p] = (L.j < 16) ? v : 0u;
        L.idB[p] = (L.j >= 16) ? v : 0u;
    }
}

// coordinate PE fragments; BWD builds Z0 = g*pe + sum_c gj[c] * dpe/dxi_c instead (backward stream)
template <int NS, bool BWD>
DEV void build_pe3(const Lane& L, Frag<NS>* act, float g, const float* gj) {
#pragma unroll
    for (int ks = 0; ks < 12; ++ks) {
        const int c = ks >> 2;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float fr = L.fr32[4 * (ks & 3) + p];
            float s, co;
            sincos_t<NS>(L.xi[c] * fr, s, co);
            if constexpr (BWD) {
                const float gf = gj[c] * fr;
                frag_set2<NS>(act[ks], p, fmaf(g, s, gf * co), fmaf(g, co, -gf * s));
            } else {
                frag_set2<NS>(act[ks], p, s, co);
            }
        }
    }
}

// Z0 of dpn_bwd_deriv_kernel: build_pe3<BWD> + sum_c gh[c] * d2 pe / d xi_c^2 = -gh[c] fr^2 pe (the cotangent of the second coordinate derivatives;
// exact by linearity in the seed)
template <int NS>
DEV void build_z0_derivs(const Lane& L, Frag<NS>* act, float g, const float* gj, const float* gh) {
#pragma unroll
    for (int ks = 0; ks < 12; ++ks) {
        const int c = ks >> 2;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float fr = L.fr32[4 * (ks & 3) + p];
            float s, co;
            sincos_t<NS>(L.xi[c] * fr, s, co);
            const float gf = gj[c] * fr;
            const float gs = fmaf(-gh[c] * fr, fr, g);
            frag_set2<NS>(act[ks], p, fmaf(gs, s, gf * co), fmaf(gs, co, -gf * s));
        }
    }
}

// coordinate features supplied by the caller in the reference's channel order (f*6 + fn*3 + c), scaled by g
template <int NS>
DEV void load_pe3(const float* row, int h, Frag<NS>* act, float g) {
#pragma unroll
    for (int ks = 0; ks < 12; ++ks)
#pragma unroll
        for (int p = 0; p < 4; ++p) frag_set2<NS>(act[ks], p, g * row[pe3_ch(ks, h, 2 * p)], g * row[pe3_ch(ks, h, 2 * p + 1)]);
}

// data PE fragments (SineCosPE(6,16) of coord_data, variable_net.py:73), scaled by g
template <int NS>
DEV void build_pe6_ks(const Lane& L, const float* cd6, Frag<NS>* act, float g, const int ks) {
    const float v = cd6[ks >> 1];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float s, co;
        sincos_t<NS>(v * L.fr16[4 * (ks & 1) + p], s, co);
        frag_set2<NS>(act[ks], p, g * s, g * co);
    }
}
template <int NS>
DEV void build_pe6(const Lane& L, const float* cd6, Frag<NS>* act, float g) {
#pragma unroll
    for (int ks = 0; ks < 12; ++ks) build_pe6_ks<NS>(L, cd6, act, g, ks);
}

// The permuted bias vectors live in LDS (filled once, before any DMA is in flight) and are read with inline-asm ds_read_b128
// for the same reason as the weight fragments: a read hipcc can see is ordered behind every outstanding LDS-DMA, and a
// global load it can see is waited for with vmcnt(0), which drains the DMA ring as well.
struct Vec16 { f32x4 q[4]; };
DEV void lds_read_vec16(Vec16& v, unsigned addr) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(v.q[0]), "=&v"(v.q[1]), "=&v"(v.q[2]), "=&v"(v.q[3]) : "v"(addr) : "memory");
}
DEV unsigned vec_addr(unsigned vec_base, int which, int h, int T) { return vec_base + (which * 256 + h * 128 + T * 16) * 4; }
DEV void acc_init_vec(f32x16& acc, unsigned vec_base, int which, int h, int T, float scale) {
    Vec16 v;
    lds_read_vec16(v, vec_addr(vec_base, which, h, T));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[4 * q] = scale * v.q[q][0]; acc[4 * q + 1] = scale * v.q[q][1]; acc[4 * q + 2] = scale * v.q[q][2]; acc[4 * q + 3] = scale * v.q[q][3];
    }
}
DEV float lds_read_f32(unsigned addr) {
    float r;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(addr) : "memory");
    return r;
}

// writers of the K-layout operand matrices (dpn_point_common.h) ----------------------------------------
DEV void store_d_as_k(const KMat& m, int net, int ns, int s, int64_t tile32, int ct, int lane, const f32x16& d) {
    uint4 a, b;
    a.x = pack2(d[0], d[1]); a.y = pack2(d[2], d[3]); a.z = pack2(d[4], d[5]); a.w = pack2(d[6], d[7]);
    b.x = pack2(d[8], d[9]); b.y = pack2(d[10], d[11]); b.z = pack2(d[12], d[13]); b.w = pack2(d[14], d[15]);
    // streaming stores: 0.4 GB of operands per launch pass through once and must not evict the L2-resident weight stream
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
#ifdef TS_ABL_NOSTORE            // ablation build (timing only, wrong results on purpose): the packed values stay alive, nothing is written
    asm volatile("" ::"v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w));
    return;
#endif
    __builtin_nontemporal_store(u32x4_t{a.x, a.y, a.z, a.w}, reinterpret_cast<u32x4_t*>(kmat_ptr(m, net, ns, s, tile32, ct, lane, 0)));
    __builtin_nontemporal_store(u32x4_t{b.x, b.y, b.z, b.w}, reinterpret_cast<u32x4_t*>(kmat_ptr(m, net, ns, s, tile32, ct, lane, 1)));
}
// transpose-store the two fragments (k-steps 2ct, 2ct+1) that make up column tile ct; zero rows of invalid points
template <int NS, int NSTORE>
DEV void store_tile_k(const KMat& m, int net, int64_t tile32, int ct, const Lane& L, const Frag<NS>& f0, const Frag<NS>& f1, bool partial) {
#pragma unroll
    for (int s = 0; s < NSTORE; ++s) {
        u32x4 a0 = f0.w[s], a1 = f1.w[s];
        if (partial && !L.valid) { a0 = (u32x4)0u; a1 = (u32x4)0u; }
        f32x16 d = (f32x16)0.f;
        d = mfma(as_bf(a0), as_bf(L.idA), d);
        d = mfma(as_bf(a1), as_bf(L.idB), d);
        store_d_as_k(m, net, NSTORE, s, tile32, ct, L.lane, d);
    }
}

// Table form of Z0 (OperandView): the fp32 features (sin, cos of the four angles of a lane's half, k-steps 2ct and 2ct + 1) of the lane's point -> the
// per-point table's K-layout, column tile ct.  Exact transposition: x = b0 + b1 + b2 with three bf16 parts (8 mantissa bits each, every remainder exact),
// each part through the identity MFMAs, the parts summed in the fp32 accumulator largest first (every partial sum is a prefix of x's mantissa).
DEV void store_table_k(const KMat& z0, const int64_t tile32, const int ct, const int lane, const u32x4& idA, const u32x4& idB, const float (&v0)[8],
                       const float (&v1)[8]) {
    u32x4 a0[3], a1[3];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        auto split = [&](const float x, const float y, u32x4 (&a)[3]) __attribute__((always_inline)) {
            const u32 w0 = pack2(x, y);
            const float rx = x - bf_lo(w0), ry = y - bf_hi(w0);
            const u32 w1 = pack2(rx, ry);
            a[0][p] = w0; a[1][p] = w1; a[2][p] = pack2(rx - bf_lo(w1), ry - bf_hi(w1));
        };
        split(v0[2 * p], v0[2 * p + 1], a0);
        split(v1[2 * p], v1[2 * p + 1], a1);
    }
    f32x16 d = (f32x16)0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        d = mfma(as_bf(a0[q]), as_bf(idA), d);
        d = mfma(as_bf(a1[q]), as_bf(idB), d);
    }
    // d[r] = the lane's column at point drow32(r, lane >> 5): registers 8 kk + 4 s + (0..3) are half s of k-step kk.  Streaming stores as store_d_as_k's
    // (the pe6 table goes out the same way and is served to the six nets from the memory-side cache).
    typedef __attribute__((ext_vector_type(4))) float f32x4_t;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            __builtin_nontemporal_store(f32x4_t{d[8 * kk + 4 * s], d[8 * kk + 4 * s + 1], d[8 * kk + 4 * s + 2], d[8 * kk + 4 * s + 3]},
                                        reinterpret_cast<f32x4_t*>(kmat_ptr(z0, 0, 2, s, tile32, ct, lane, kk)));
}

// ------------------------------------------------------------------------------------------------ forward + Jacobian
struct FwdArgs {
    const float *x, *y, *t, *coord_data, *freqs, *pe_in;
    int64_t n, n_pad;
    DpnGeometry geo;
    const char* packed;
    float* out_n;
    float* jac_n;
    void* saved;
    const float* ref;        // [N][6] added to the output in place of coord_data (VariableNet.forward's own ref_data argument), else null
#ifdef DPN_TIMELINE
    unsigned* timeline;      // [blocks][6 nets][8 wave slots][64]: s_memtime (low word) at the start of every pipeline step (experiment build only)
#endif
};

// Experiment build (-DDPN_TIMELINE, tools/timeline_build.py): every wave keeps the shader clock at the start of each pipeline step in one
// VGPR (lane i <- stamp i, v_writelane: no memory traffic, no counters touched besides the s_memtime's own lgkmcnt, which is empty at a
// step boundary) and writes the register out at the end.  Stamp 0 = kernel entry, 1 = ring primed / prologue done, 2 + C = step C, 62 = exit.
#ifdef DPN_TIMELINE
#define DPN_STAMP(I)                                                                                          \
    do {                                                                                                      \
        unsigned long long t_;                                                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                            \
        asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(tl) : "s"((u32)t_), "n"(I));                         \
    } while (0)
#else
#define DPN_STAMP(I) do { } while (0)
#endif

#ifdef DPN_FWD_PHASES
#define DPN_PH_AFTER_MMA do { u32 c4_; DPN_PH_CLOCK(c4_); pipe.ph[3] += c4_ - pipe.pc0; pipe.pc0 = c4_; } while (0)
#else
#define DPN_PH_AFTER_MMA do { } while (0)
#endif
// One pipeline step on chunk C: make it readable (and put chunk C+3 in flight), multiply it, and run the epilogue of the
// PREVIOUS tile in the shadow of these MFMAs (it only touches that tile's accumulator).
#define DPN_STEP(C, NK, SWAP, ACT, ACC, EPI_PREV)                                    \
    do {                                                                             \
        DPN_STAMP(2 + (C));                                                          \
        pipe.acquire(C);                                                             \
        mma_chunk<NS, (NK), (SWAP)>(pipe.buf(C), (ACT), (ACC));                      \
        DPN_PH_AFTER_MMA;                                                            \
        EPI_PREV;                                                                    \
    } while (0)

// ------------------------------------------------------------------------------------------------ backward, stage 1
struct BwdArgs {
    const float *x, *y, *t, *coord_data, *freqs, *pe_in;
    int64_t n, n_pad;
    DpnGeometry geo;
    const char* packed;
    const float *g_out, *g_jxi;
    const float* g_scale;    // device scalar multiplied into both cotangent streams as they are read (an upstream cotangent on unit-cotangent streams), or null
    void* saved;
    void* operands;
#ifdef DPN_TIMELINE
    unsigned* timeline;      // experiment build: [net][workgroup][4 waves][48] shader clocks at the phase boundaries of dpn_bwd_tiles_kernel
#endif
};

// the ring kernels (dpn_fwd_kernel, dpn_bwd_kernel) and their derivative forms (dpn_fwd_deriv_kernel, dpn_bwd_deriv_kernel)
#define DPN_DERIV 0
#include "dpn_ring_kernels.inc"
#undef DPN_DERIV
#define DPN_DERIV 1
#include "dpn_ring_kernels.inc"
#undef DPN_DERIV

#include "dpn_fwd_tiles.h"                                       // tile-split forward / backward kernels (the hi+lo mode's default)
// (round 6's ping-pong and persistent forms of the tile-split forward, dpn_fwd_pp.h / dpn_fwd_tiles_persist.h, and the eight-wave forward of
//  tools/experiments: measured slower, removed; last present at 3bc40f4)

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

#ifdef DPN_TIMELINE
static unsigned* g_timeline = nullptr;
int dpn_debug_set_timeline(void* buf) { g_timeline = reinterpret_cast<unsigned*>(buf); return 0; }    // experiment build only, not in dpn_hip.h
#endif
static int fwd_launch(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data, int64_t n,
                      const float* freqs, const DpnGeometry* geo, const void* packed, int prec, float* out_n, float* jac_n, void* saved, void* stream,
                      int n_nets) {
    if (!coord_data || !freqs || !geo || !packed || !out_n || n <= 0 || (prec != 1 && prec != 2)) return -1;
    if (!pe_in && (!x || !y || !t)) return -1;
#ifdef DPN_TIMELINE
    FwdArgs a{x, y, t, coord_data, freqs, pe_in, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), out_n, jac_n, saved, ref_data, g_timeline};
#else
    FwdArgs a{x, y, t, coord_data, freqs, pe_in, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), out_n, jac_n, saved, ref_data};
#endif
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(a.n_pad / 128), n_nets);
    // hi+lo mode: the tile-split kernel (dpn_fwd_tiles.h; 64 points per workgroup, two workgroups per CU).  Caller-encoded coordinates
    // and the single-bf16 mode stay on the ring kernel (one bf16 product per fragment pair cannot pay for the doubled weight stream).
    // DPN_FWD_KERNEL=ring|tiles overrides (A/B measurements, bitwise comparison of the two kernels in the tests).
    if (use_tiles("DPN_FWD_KERNEL", prec, pe_in != nullptr)) {    // (expects the FUSED packed form: dpn_fwd_form)
        const dim3 grid64((unsigned)(a.n_pad / 64), n_nets);
        if (prec == 1) hipLaunchKernelGGL(dpn_fwd_tiles_kernel<1>, grid64, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(dpn_fwd_tiles_kernel<2>, grid64, dim3(256), 0, s, a);
        return ck(hipGetLastError());
    }
    if (prec == 1) hipLaunchKernelGGL(dpn_fwd_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dpn_fwd_kernel<2>, grid, dim3(256), 0, s, a);
    return ck(hipGetLastError());
}

int dpn_fwd_ref(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data, int64_t n,
                const float* freqs, const DpnGeometry* geo, const void* packed, int prec, float* out_n, float* jac_n, void* saved, void* stream) {
    return fwd_launch(x, y, t, pe_in, coord_data, ref_data, n, freqs, geo, packed, prec, out_n, jac_n, saved, stream, kNets);
}
// the first n_nets VariableNets only (inference: nothing is saved); the other columns of out_n / jac_n are left untouched
int dpn_fwd_ref_nets(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data, int64_t n,
                     const float* freqs, const DpnGeometry* geo, const void* packed, int prec, int n_nets, float* out_n, float* jac_n, void* stream) {
    if (n_nets < 1 || n_nets > kNets) return -1;
    return fwd_launch(x, y, t, pe_in, coord_data, ref_data, n, freqs, geo, packed, prec, out_n, jac_n, nullptr, stream, n_nets);
}

int dpn_fwd(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n, const float* freqs,
            const DpnGeometry* geo, const void* packed, int prec, float* out_n, float* jac_n, void* saved, void* stream) {
    return dpn_fwd_ref(x, y, t, pe_in, coord_data, nullptr, n, freqs, geo, packed, prec, out_n, jac_n, saved, stream);
}

// dpn_fwd_ref + second / third coordinate derivatives in the same launch (raw coordinates only).  With hess_n = d3_n = NULL it IS dpn_fwd_ref's launch.
int dpn_fwd_ref_derivs(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, const float* ref_data, int64_t n,
                       const float* freqs, const DpnGeometry* geo, const void* packed, int prec, float* out_n, float* jac_n, float* hess_n, float* d3_n,
                       void* saved, void* stream) {
    if (pe_in || !x || !y || !t || ((hess_n || d3_n) && !jac_n)) return -1;
    if (!hess_n && !d3_n) return fwd_launch(x, y, t, nullptr, coord_data, ref_data, n, freqs, geo, packed, prec, out_n, jac_n, saved, stream, kNets);
    if (!coord_data || !freqs || !geo || !packed || !out_n || n <= 0 || (prec != 1 && prec != 2)) return -1;
#ifdef DPN_TIMELINE
    FwdArgs a{x, y, t, coord_data, freqs, nullptr, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), out_n, jac_n, saved, ref_data, g_timeline};
#else
    FwdArgs a{x, y, t, coord_data, freqs, nullptr, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), out_n, jac_n, saved, ref_data};
#endif
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (use_tiles("DPN_FWD_KERNEL", prec, false)) {            // the kernel choice (and so the packed form) of fwd_launch
        const dim3 grid64((unsigned)(a.n_pad / 64), kNets);
        if (prec == 1) hipLaunchKernelGGL(dpn_fwd_tiles_deriv_kernel<1>, grid64, dim3(256), 0, s, a, hess_n, d3_n);
        else hipLaunchKernelGGL(dpn_fwd_tiles_deriv_kernel<2>, grid64, dim3(256), 0, s, a, hess_n, d3_n);
        return ck(hipGetLastError());
    }
    const dim3 grid((unsigned)(a.n_pad / 128), kNets);
    if (prec == 1) hipLaunchKernelGGL(dpn_fwd_deriv_kernel<1>, grid, dim3(256), 0, s, a, hess_n, d3_n);
    else hipLaunchKernelGGL(dpn_fwd_deriv_kernel<2>, grid, dim3(256), 0, s, a, hess_n, d3_n);
    return ck(hipGetLastError());
}

static int bwd_points_launch(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n, const float* freqs,
                             const DpnGeometry* geo, const void* packed, int prec, const float* g_out, const float* g_jxi, const float* g_scale,
                             const void* saved, void* operands, void* stream) {
    if (!coord_data || !freqs || !geo || !packed || !g_out || !saved || !operands || n <= 0 || (prec != 1 && prec != 2)) return -1;
    if (pe_in ? (g_jxi != nullptr) : (!x || !y || !t)) return -1;
#ifdef DPN_TIMELINE
    BwdArgs a{x, y, t, coord_data, freqs, pe_in, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), g_out, g_jxi, g_scale,
              const_cast<void*>(saved), operands, g_timeline};
#else
    BwdArgs a{x, y, t, coord_data, freqs, pe_in, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), g_out, g_jxi, g_scale,
              const_cast<void*>(saved), operands};
#endif
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(a.n_pad / 128), kNets);
    if (use_tiles("DPN_BWD_KERNEL", prec, pe_in != nullptr)) {    // ring | tiles: bit-identical operands (tests); both read w1 at S0 of either packed form
        const dim3 grid64((unsigned)(a.n_pad / 64), kNets);
        if (prec == 1) hipLaunchKernelGGL(dpn_bwd_tiles_kernel<1>, grid64, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(dpn_bwd_tiles_kernel<2>, grid64, dim3(256), 0, s, a);
        return ck(hipGetLastError());
    }
    if (prec == 1) hipLaunchKernelGGL(dpn_bwd_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dpn_bwd_kernel<2>, grid, dim3(256), 0, s, a);
    return ck(hipGetLastError());
}

int dpn_bwd_points(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n, const float* freqs,
                   const DpnGeometry* geo, const void* packed, int prec, const float* g_out, const float* g_jxi, const void* saved,
                   void* operands, void* stream) {
    return bwd_points_launch(x, y, t, pe_in, coord_data, n, freqs, geo, packed, prec, g_out, g_jxi, nullptr, saved, operands, stream);
}
int dpn_bwd_points_scaled(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n, const float* freqs,
                          const DpnGeometry* geo, const void* packed, int prec, const float* g_out, const float* g_jxi, const float* g_scale,
                          const void* saved, void* operands, void* stream) {
    return bwd_points_launch(x, y, t, pe_in, coord_data, n, freqs, geo, packed, prec, g_out, g_jxi, g_scale, saved, operands, stream);
}

// dpn_bwd_points_scaled + g_hxi, the cotangent of the xi-space second derivatives, folded into the same Z0 seed.  g_hxi = NULL: dpn_bwd_points_scaled's launch.
int dpn_bwd_points_derivs(const float* x, const float* y, const float* t, const float* pe_in, const float* coord_data, int64_t n, const float* freqs,
                          const DpnGeometry* geo, const void* packed, int prec, const float* g_out, const float* g_jxi, const float* g_hxi,
                          const float* g_scale, const void* saved, void* operands, void* stream) {
    if (pe_in || !x || !y || !t) return -1;
    if (!g_hxi) return bwd_points_launch(x, y, t, nullptr, coord_data, n, freqs, geo, packed, prec, g_out, g_jxi, g_scale, saved, operands, stream);
    if (!coord_data || !freqs || !geo || !packed || !g_out || !saved || !operands || n <= 0 || (prec != 1 && prec != 2)) return -1;
#ifdef DPN_TIMELINE
    BwdArgs a{x, y, t, coord_data, freqs, nullptr, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), g_out, g_jxi, g_scale,
              const_cast<void*>(saved), operands, g_timeline};
#else
    BwdArgs a{x, y, t, coord_data, freqs, nullptr, n, pad_points(n), *geo, reinterpret_cast<const char*>(packed), g_out, g_jxi, g_scale,
              const_cast<void*>(saved), operands};
#endif
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (use_tiles("DPN_BWD_KERNEL", prec, false)) {
        const dim3 grid64((unsigned)(a.n_pad / 64), kNets);
        if (prec == 1) hipLaunchKernelGGL(dpn_bwd_tiles_deriv_kernel<1>, grid64, dim3(256), 0, s, a, g_hxi);
        else hipLaunchKernelGGL(dpn_bwd_tiles_deriv_kernel<2>, grid64, dim3(256), 0, s, a, g_hxi);
        return ck(hipGetLastError());
    }
    const dim3 grid((unsigned)(a.n_pad / 128), kNets);
    if (prec == 1) hipLaunchKernelGGL(dpn_bwd_deriv_kernel<1>, grid, dim3(256), 0, s, a, g_hxi);
    else hipLaunchKernelGGL(dpn_bwd_deriv_kernel<2>, grid, dim3(256), 0, s, a, g_hxi);
    return ck(hipGetLastError());
}

}  // extern "C"
