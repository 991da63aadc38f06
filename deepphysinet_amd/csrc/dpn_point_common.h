// What the point kernels (dpn_point.hip) and the weight-gradient unit (dpn_wgrad.hip) both need: the LDS-DMA instructions and their counted
// wait, and the layouts of what the point kernels write and dpn_wgrad_kernel reads -- saved state and K-layout operand matrices -- with their
// sizes (dpn_sizes) and the choice of point kernel that the packed form follows (dpn_fwd_form).
#pragma once
#include "dpn_device.h"

// ------------------------------------------------------------------------------------------------ LDS-DMA
// global -> LDS without staging registers and without a ds_write pass (global_load_lds_dwordx4: 1 KB per wave-instruction).  vmcnt retires in
// order on gfx9-class hardware (the compiler's own counted waits rely on it): a counted s_waitcnt vmcnt says which of a wave's pieces have landed.
DEV void dma16(const char* gsrc_lane, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc_lane),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}
template <int OFF> DEV void dma16_at(const char* gsrc_lane, char* lds_wave_base) {     // OFF: the instruction's immediate, added to both addresses
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc_lane),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, OFF, 0);
}
DEV void dma16_nt(const char* gsrc_lane, char* lds_wave_base) {       // read-once streams (weight-gradient operands): non-temporal hint
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc_lane),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 2);
}
DEV void dma4(const char* gsrc_lane, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc_lane),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 4, 0, 0);
}
template <int N> DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ------------------------------------------------------------------------------------------------ K-layout operand matrices
// Every matrix the points-reduction GEMMs consume is stored "channel-per-lane": for each 32-point tile and each 32-column
// tile, lane (col = lane&31, h = lane>>5) owns 16 bf16 = the values of its column at points drow32(r,h), r = 0..15, i.e.
// exactly the A/B fragments of v_mfma_f32_32x32x16_bf16 with K = points (k-step kk = registers 8kk..8kk+7).  Columns are in
// SLOT order (column 32*ct + jj <-> k-step 2ct + (jj>>4), slot (h=(jj>>3)&1, e=jj&7)).
// A matrix held point-per-lane (as chained fragments) is brought into this layout by multiplying with an identity B
// operand: one extra MFMA per 16 channels instead of an LDS round trip.
struct KMat {
    char* base;
    int64_t tiles32;
    int ct_per_tile;      // column tiles: 8 (256 columns) or 6 (192)
};
// one 32-point tile of a matrix = [2 k-steps][ct_per_tile column tiles][64 lanes][16 B]: a linear image of what the
// weight-gradient kernel wants in LDS (its global -> LDS transfer is a plain 1-KB-per-wave-instruction DMA)
DEV char* kmat_ptr(const KMat& m, int net, int ns, int s, int64_t tile32, int ct, int lane, int kk) {
    return m.base + (((int64_t)net * ns + s) * m.tiles32 + tile32) * (m.ct_per_tile * 2048) + ((kk * m.ct_per_tile + ct) * 64 + lane) * 16;
}

// saved-state / operand addressing ---------------------------------------------------------------------------
struct SavedView {       // written by dpn_fwd
    KMat T1;             // [6][NS] x 256 columns: t1 = m1 (.) (w2^T v), the cotangent in front of the first ReLU
    KMat M2;             // [6][1]  x 256 columns, relu-2 mask as bf16 0/1
    uint4* m1;           // [6][tiles32][64] lane-format bits of relu mask 1
};
// v = d out / d c is NOT saved: it is affine in the second mask, v = W1^T (m2 (.) u) + 2 wo (W1 = cat_fc1.fc.0.weight, u = fc.2.weight^T wo),
// so the two weight-gradient products it entered factor through the 0/1 matrix that is saved anyway,
//   sum_pt v (x) z1 = W1^T diag(u) (M2^T Z1) + 2 wo (x) colsum(Z1)      (likewise with G6),
// -- one 512-byte mask row per point and net instead of a 1-KB hi+lo row written once and read twice, two MFMAs per fragment pair instead
// of three, and the 256 x 256 factor applied once per net in fp32 (dpn_finish_vside_fc2_kernel) instead of once per point in split bf16.
DEV SavedView saved_view(void* base, int64_t n_pad, int ns) {
    SavedView s;
    char* b = reinterpret_cast<char*>(base);
    const int64_t mat = (int64_t)kNets * ns * n_pad * 512;
    const int64_t tiles32 = n_pad / 32;
    s.T1 = KMat{b, tiles32, 8};
    s.M2 = KMat{b + mat, tiles32, 8};
    s.m1 = reinterpret_cast<uint4*>(b + mat + (int64_t)kNets * n_pad * 512);
    return s;
}
DPN_HD int64_t saved_state_bytes(int64_t n_pad, int ns) { return (int64_t)kNets * ns * n_pad * 512 + (int64_t)kNets * n_pad * 512 + (int64_t)kNets * n_pad * 32; }

struct OperandView {     // written by dpn_bwd_points
    KMat Z1;             // [6][NS] x 256   (round 5: Z is not an operand any more, dpn_finish_gside_kernel)
    KMat Z0;             // [6][NS] x 192   stored form; table form: planes 0 / 1 of net 0 hold the two 16-byte halves of the per-point fp32 pe3 table
    KMat PE6;            // [1][NS] x 192   per-POINT table of the data features (sin / cos of coord_data), written once by the net-0 workgroups
    float* gnet;         // [6][n_pad]      per-net cotangent of the normalised field, zero for padding points
    float* gj;           // [6][3][n_pad]   table form: the coordinate cotangents gJ_c (g_scale included), zero for padding points; in net 1's Z0 space
    unsigned* hdr;       // [0]: kZ0Stored | kZ0Table, [4 + i]: the 32 coordinate frequencies; in the slack behind gnet, outside every form's Z0
};
constexpr unsigned kZ0Stored = 0u, kZ0Table = 1u;
// Round 5: G6 = g pe6 (the Y operand of S2 = M2^T G6) is no longer written per point AND NET: it is a per-point table times a per-net scalar, so
// dpn_wgrad_kernel forms it from the table and the table -- 768 B per point in the hi+lo mode, shared by the six nets -- stays in the memory-side cache.
// Stage 1 writes 2 560 -> 1 792 B per point and net.  The forming was in registers at first, on the fragment each wave had just read (seven VALU
// instructions per element beside the MFMAs, the same elements on four waves); it is now done once per workgroup, in LDS, in place, by the wave that
// fetched the piece (dpn_wgrad.hip, form()): bit-identical S2, same range plan, dpn_wgrad_kernel<2> alone 229-234 -> 215-219 us and 219.4 -> 203.4 us
// in the captured step (rocprofv3), the step 1.157-1.166 -> 1.140-1.144 ms (five alternated rounds each on one box; profiles/wgrad_coop_forming_ab.txt).
//
// Z0 = g pe3 + gJ_c d pe3 / d xi_c has the same structure -- a per-point table (sin / cos of xi_c fr, no net) and four per-net scalars per point -- and
// in the hi+lo mode on the raw-coordinate route (prec == 2, no pe_in, no second-derivative cotangent) it is not stored either.  TABLE FORM of the Z0 region, inside the bytes the stored form
// occupies (operand_bytes and the C ABI are unchanged):
//   table   fp32, 768 B per point, K-layout: the eight points a lane owns of one column in one k-step are 32 B = two 16-byte halves (points e = 0..3 |
//           4..7 of drow32); half s sits where plane s (hi | lo) of NET 0 keeps its 1-KB piece of that (k-step, column tile) pair, so that the slot image
//           in LDS is overwritten in place with hi and lo.  Column tile ct is written by the workgroups of net ct (six nets, six column tiles).
//   gj      [net][c][n_pad] fp32 behind the table (net 1's space): lanes 32..63 of the weight-gradient kernel's per-tile g copy fetch gJ_c beside g.
//   hdr     the form word and the frequencies (dpn_wgrad has no freqs argument).  EVERY stage-1 launch of every form writes it: one operand buffer may
//           alternate between the routes.  Plain bf16, caller-encoded coordinates and the *_deriv kernels write kZ0Stored and Z0 as before.
// The transposition to the K-layout is exact: a three-way bf16 split (8 + 8 + 8 mantissa bits) through the identity MFMAs of the bf16 planes, summed in
// the fp32 accumulator.  Limits: normal values only (a bf16 part below 2^-126 may be flushed: features below ~2^-100 in magnitude that are not zero),
// and -0.0 arrives as +0.0.  dpn_wgrad_kernel<2> forms Z0 from the table exactly as ts::z0_frag / build_pe3<BWD> did: gf = gJ_c fr,
// z = fmaf(g, own, +-(gf partner)), hi = bf16(z), lo = bf16(z - hi): the same bits the stored form holds.
// (Round 5 built a table form with IN-REGISTER forming -- the partner column through a DPP move -- and measured stage 1 91 us instead of 130 but the
// weight-gradient kernel 198 -> 337 us: product 3's tile loop spilled; profiles/round5_operand_tables.txt.  The forming in LDS holds no fragments beside
// the accumulators.)
DEV OperandView operand_view(void* base, int64_t n_pad, int ns) {
    OperandView o;
    char* b = reinterpret_cast<char*>(base);
    const int64_t m256 = (int64_t)kNets * ns * n_pad * 512, m192 = (int64_t)kNets * ns * n_pad * 384, t192 = (int64_t)ns * n_pad * 384;
    const int64_t tiles32 = n_pad / 32;
    o.Z1 = KMat{b, tiles32, 8};
    o.Z0 = KMat{b + m256, tiles32, 6};
    o.PE6 = KMat{b + m256 + m192, tiles32, 6};
    o.gnet = reinterpret_cast<float*>(b + m256 + m192 + t192);
    o.gj = reinterpret_cast<float*>(b + m256 + t192);                                     // 72 B per point of net 1's 768
    o.hdr = reinterpret_cast<unsigned*>(b + m256 + m192 + t192 + (int64_t)kNets * n_pad * 4 + 256);    // (the last tile's 64-lane g copy reads 128 B of the slack)
    return o;
}
// every stage-1 kernel, its first workgroup of net 0: the form word and the frequencies
DEV void write_operand_header(const OperandView& o, const unsigned form, const float* freqs) {
    if (blockIdx.x != 0 || blockIdx.y != 0 || threadIdx.x >= 32) return;
    if (threadIdx.x == 0) o.hdr[0] = form;
    o.hdr[4 + threadIdx.x] = __float_as_uint(freqs[threadIdx.x]);
}
static inline int64_t operand_bytes(int64_t n_pad, int ns) { return (int64_t)kNets * ns * n_pad * 512 + (int64_t)(kNets + 1) * ns * n_pad * 384 + (int64_t)kNets * n_pad * 4 + 1024; }

static inline int64_t pad_points(int64_t n) { return ((n + 127) / 128) * 128; }
// hi+lo mode: the tile-split kernels (dpn_fwd_tiles.h; 64 points per workgroup, two workgroups per CU).  Caller-encoded coordinates and the
// single-bf16 mode stay on the ring kernels.  DPN_FWD_KERNEL / DPN_BWD_KERNEL = ring | tiles override (read per call: the tests compare the two
// decompositions inside one process).
static inline bool use_tiles(const char* knob, int prec, bool has_pe_in) {
    const char* force = getenv(knob);
    return (force ? (force[0] == 't') : (prec == 2)) && !has_pe_in;
}
