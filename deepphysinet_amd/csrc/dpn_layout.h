// Layout algebra shared by the pack kernel, the point kernels and the host-side unit tests.
//
// Everything the point kernels multiply goes through v_mfma_f32_32x32x16_bf16 in the
// "points-as-columns" orientation:  Out[channel][point] = sum_k Wt[channel][k] * Act[k][point]
//   A operand (weights)     : lane l holds row  i = l&31, k-slots (h = l>>5, e = 0..7)
//   B operand (activations) : lane l holds col  j = l&31 (= the lane's collocation point), k-slots (h, e)
//   D accumulator           : lane l holds col  j = l&31, rows (r&3) + 8*(r>>2) + 4*h, r = 0..15
// Because the hardware pairs A slot (h,e) with B slot (h,e), the meaning of a k-slot is ours to
// choose.  We choose it so that the D registers of one layer ARE the B operand of the next
// (no LDS round trip, no cross-lane traffic): k-step ks, slot (h,e)  <->  channel chain_ch(ks,h,e).
#pragma once

#if defined(__HIPCC__)
#define DPN_HD __host__ __device__ constexpr
#else
#define DPN_HD constexpr
#endif

namespace dpn {

constexpr int kNets = 6;        // u, v, P, T, q, rho  (model/physics_net.py:49-54)
constexpr int kHidden = 256;    // net_cfg.hidden_channels
constexpr int kPe = 192;        // net_cfg.in_channels
constexpr int kW1Stride = 193;  // coord_input_fc output row: [w1 (192) | b1]
constexpr int kW2Stride = 257;  // coord_hidden_fc output row: [w2 (256) | b2]

// row of a 32-row D tile held in accumulator register r by a lane of half h
DPN_HD int drow32(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// channel fed by chained k-slot (ks, h, e): D tile T = ks/2, register r = 8*(ks&1)+e
DPN_HD int chain_ch(int ks, int h, int e) { return 16 * ks + 8 * (e >> 2) + 4 * h + (e & 3); }

// coordinate PE (SineCosPE(3, N_freqs=32), utils/position_encoding.py:35-50): original channel = f*6 + fn*3 + c.
// k-slot (ks,h,e): angle a = 8*ks + 4*h + (e>>1) in [0,96): c = a>>5, f = a&31; fn = e&1 (0 sin, 1 cos).
DPN_HD int pe3_angle(int ks, int h, int e) { return 8 * ks + 4 * h + (e >> 1); }
DPN_HD int pe3_ch(int ks, int h, int e) { return (pe3_angle(ks, h, e) & 31) * 6 + (e & 1) * 3 + (pe3_angle(ks, h, e) >> 5); }
// data PE (SineCosPE(6, N_freqs=16), model/variable_net.py:45): original channel = f*12 + fn*6 + c6; a = c6*16 + f.
DPN_HD int pe6_ch(int ks, int h, int e) { return (pe3_angle(ks, h, e) & 15) * 12 + (e & 1) * 6 + (pe3_angle(ks, h, e) >> 4); }

// The reverse sweep ends with gpe = w1^T t1 laid out so that D tile T, register r of a lane of half h is the
// cotangent of the lane's OWN q-th PE feature, q = 16*T + r = 8*ks + e  (ks = 2T + (r>>3), e = r&7).
// Row rho = 32*T + i of that GEMM's A operand therefore is PE slot:
DPN_HD int gpe_row_to_pe3_ch(int rho) {
    const int T = rho >> 5, i = rho & 31;
    const int r = (i & 3) + 4 * (i >> 3), h = (i >> 2) & 1;
    return pe3_ch(2 * T + (r >> 3), h, r & 7);
}

// ------------------------------------------------------------------ packed per-net weight block
// Stream order (KB = 1024 B units for NS = 1; multiply by NS for the hi/lo split):
//   S0  w1          8 tiles x 12 k-steps   (A rows o,   K = PE3 slots)
//   S1  w2 , Wd     8 x 16 then 8 x 12     (A rows o,   K = chain(h1) / PE6 slots): all w2 tiles, then all Wd tiles
//   S2  W1          8 x 16                 (A rows o,   K = chain(c))
//   S3  W1^T        8 x 16                 (A rows i,   K = chain(t2))
//   S4  w2^T        8 x 16                 (A rows i,   K = chain(v))
//   S5  w1^T        6 x 16                 (A rows rho, K = chain(t1))
// One k-step fragment = 64 lanes x 8 bf16 = 1 KB; with NS = 2 the hi KB is followed by the lo KB.
constexpr int kS0 = 0;
constexpr int kS1 = kS0 + 8 * 12;
constexpr int kS2 = kS1 + 8 * 28;
constexpr int kS3 = kS2 + 8 * 16;
constexpr int kS4 = kS3 + 8 * 16;
constexpr int kS5 = kS4 + 8 * 16;
constexpr int kPackKB = kS5 + 6 * 16;      // 800 KB per net (x NS)
// fp32 vectors appended after the matrices, each 256 floats in [h][T][r] order (index h*128 + T*16 + r):
enum { kVecB1 = 0, kVecCvec, kVecBf1, kVecU, kVecWo, kVecB2BdE_unused, kNumVecs = 6 };
// ... followed by 4 floats: const0 = wo.bf2 + bo, 0, 0, 0
DPN_HD long pack_bytes_per_net(int ns) { return (long)kPackKB * 1024 * ns + kNumVecs * 1024 + 16; }

// ------------------------------------------------------------------ FUSED form of the block (round 5; dpn_fwd_tiles_kernel)
// With A = W1 w2 and B = W1 Wd formed once per net (exact fp32) the forward + Jacobian pass is five GEMMs instead of seven
// (dpn_fwd_tiles.h; dpn_pack_fused_kernel forms the products and writes their fragments in one launch).  Same block size and the same offsets for what the other kernels read (S0 = w1 for the backward stage-1 kernels, S5 = w1^T,
// the vector block), so that one buffer serves either form:
//   F0  = S0  w1     8 x 12        FA  A      8 x 16  (A rows o, K = chain(h1))       FB  B    8 x 12  (A rows o, K = PE6 slots)
//   FAT       A^T    8 x 16  (A rows j, K = chain(t2))                                  F5  = S5  w1^T  6 x 16;   [kS3, kS5) stays unwritten
// vectors: B1 = b1 | C2 = W1 cvec + bf1 | A2 = w2^T wo | U = W2^T wo | Wo | Bv = Wd^T wo in PE6 slot order (192 used);
//          const0 = wo.bf2 + bo + 2 wo.cvec
constexpr int kF0 = kS0, kFA = kS1, kFB = kS1 + 8 * 16, kFAT = kS2, kF5 = kS5;
static_assert(kFB + 8 * 12 == kS2 && kFAT + 8 * 16 == kS3, "fused form fits the block");
enum { kVecC2 = kVecCvec, kVecA2 = kVecBf1, kVecBv = kVecB2BdE_unused };

// ------------------------------------------------------------------ dpn_wgrad_kernel, product 2: which wave fetches which 1-KB piece of a tile
// The slot image of S2 = M2^T G6 is 16 X pieces (the mask) and, per plane s < ns, 12 Y pieces p = (k-step, column tile) of the per-point pe6 table.
// G6 = g pe6 is formed from the table in LDS, in place, by the wave that fetched the piece, so a wave gets BOTH planes of its column pairs:
// pair `wave` in its first ns slots, pair 8 + wave in the next ns on waves 0..3; the other slots take the X pieces (waves 4..7 take more of them) and,
// where 8 * issue > 16 + 12 ns, a pad.  Slot j of `issue` per wave -> -1: pad | 0 .. 15: X piece | 16 + 12 s + p: plane s of pair p.
DPN_HD bool wgrad_coop_is_y(int ns, int wave, int j) { return j < ns || (j < 2 * ns && wave < 4); }
DPN_HD int wgrad_coop_piece(int ns, int issue, int wave, int j) {
    const int xlo = issue - 2 * ns, xhi = (16 - 4 * xlo) / 4;       // X pieces of a wave 0..3 / 4..7 (hi+lo: 1 / 3, plain bf16: 2 / 2)
    if (j < ns) return 16 + 12 * j + wave;
    if (wave < 4) return j < 2 * ns ? 16 + 12 * (j - ns) + 8 + wave : xlo * wave + (j - 2 * ns);
    return j - ns < xhi ? 4 * xlo + xhi * (wave - 4) + (j - ns) : -1;
}


// ------------------------------------------------------------------ dpn_wgrad_kernel, product 3 in the TABLE form of Z0 (dpn_point_common.h, OperandView)
// The slot image of dw1 = T1^T Z0 is 32 X pieces (T1 hi, lo) and 24 Y pieces: plane s < 2 of pair p = 6 kk + ct holds half s (points e = 4 s .. 4 s + 3 of
// a lane's eight) of the fp32 table's k-step kk of column tile ct, and after forming plane 0 = hi, plane 1 = lo of this net's Z0.  56 pieces, seven per
// wave, no pad.  A wave fetches BOTH halves of the pairs it forms, and all its pairs are of ONE column tile -- one coordinate c = ct >> 1 (one gJ_c beside
// g in its per-tile copy) and one frequency per lane: waves 0..3 both k-steps of column tile `wave`, waves 4..7 one k-step of column tile 4 or 5.  The
// table pieces come first in the issue order (they are what forming waits for); waves 0..3 take three X pieces each, waves 4..7 five.
// Slot j of 7 per wave -> 0 .. 31: X piece | 32 + 12 s + p: half s of pair p.
DPN_HD int wgrad_z0_ct(int wave) { return wave < 4 ? wave : 4 + (wave & 1); }
DPN_HD int wgrad_z0_pairs(int wave) { return wave < 4 ? 2 : 1; }
DPN_HD int wgrad_z0_kk(int wave, int q) { return wave < 4 ? q : (wave - 4) >> 1; }             // k-step of the wave's q-th pair
DPN_HD bool wgrad_z0_is_y(int wave, int j) { return j < 2 * wgrad_z0_pairs(wave); }
DPN_HD int wgrad_z0_piece(int wave, int j) {
    if (wgrad_z0_is_y(wave, j)) return 32 + 12 * (j & 1) + 6 * wgrad_z0_kk(wave, j >> 1) + wgrad_z0_ct(wave);
    return wave < 4 ? 3 * wave + (j - 4) : 12 + 5 * (wave - 4) + (j - 2);
}
// Column jj of column tile ct is PE slot (k-step 2 ct + (jj >> 4), h = (jj >> 3) & 1, e = jj & 7): sine for even jj, cosine for odd, of the angle
// xi_c fr with c = ct >> 1 and fr = freqs[z0_freq_index(ct, jj)].  The partner (cosine of a sine column, sine of a cosine column) is column jj ^ 1:
// in the K-layout lane ^ 1, the neighbouring 16 bytes of the same 1-KB piece.
DPN_HD int z0_freq_index(int ct, int jj) { return 16 * (ct & 1) + (jj >> 1); }

}  // namespace dpn
