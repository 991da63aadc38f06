// The point kernels of the tile-split form (dpn_fwd_tiles.h), included twice by it:
//   DPN_DERIV 0:  dpn_fwd_tiles_kernel, dpn_bwd_tiles_kernel -- what the fused step launches;
//   DPN_DERIV 1:  dpn_fwd_tiles_deriv_kernel (+ second and third coordinate derivatives from the Jacobian's accumulators, dpn_fwd_ref_derivs) and
//                 dpn_bwd_tiles_deriv_kernel (+ their cotangent g_hxi in the Z0 seed, dpn_bwd_points_derivs).
// One text, gated by the preprocessor: the first pass is token for token the kernels as they were (dpn_ring_kernels.inc says why).

// Round 5: FIVE GEMMs per point and net instead of seven.  W1 (cat_fc1.fc.0.weight) only ever multiplies c = w2 h1 + Wd pe6 + cvec, and its
// transpose only ever meets w2^T on the way back, so the two static-times-hyper products are formed ONCE per net and step,
//     A = W1 w2 [256, 256],   B = W1 Wd [256, 192]        (exact fp32, dpn_pack_weights: csrc FusedForm)
// and   pre2 = A h1 + B pe6 + (W1 cvec + bf1),    wo . c = (w2^T wo) . h1 + (Wd^T wo) . pe6 + wo . cvec,    y = A^T (m2 (.) u) + 2 w2^T wo:
// neither c nor v = d out / d c is formed per point.  409 600 -> 278 528 executed MACs per point and net, and the weight stream a workgroup
// pulls out of L2 per 64 points shrinks from 800 to 544 KB (x NS).  What the backward pass needs (m1, M2, T1 = m1 (.) y) is unchanged; its
// formulas are in the original parameters (dpn_finish_*).  Identity and operand rounding: tools/precision_fused_algebra.py.
template <int NS>
#if DPN_DERIV
__global__ __launch_bounds__(256, 2) void dpn_fwd_tiles_deriv_kernel(FwdArgs a, float* hess_n, float* d3_n) {
#else
__global__ __launch_bounds__(256, 2) void dpn_fwd_tiles_kernel(FwdArgs a) {
#endif
    using C = ts::Cfg<NS>;
    __shared__ __attribute__((aligned(16))) char lds[C::kLdsBytes];
    const int net = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const char* pk = a.packed + (long)net * pack_bytes_per_net(NS);
#if TS_PRIO == 2
    __builtin_amdgcn_s_setprio(1);
#endif
    TS_STAMP(0);
    float* vec = reinterpret_cast<float*>(lds + C::kVecOff);
    float* red = reinterpret_cast<float*>(lds + C::kRedOff);
    char* xl = lds + lane * 16;
    {   // permuted fp32 vectors of this net -> LDS (published by the first barrier): 385 x 16 bytes, both loads of a thread in flight
        const u32x4* gv = reinterpret_cast<const u32x4*>(pk + (long)kPackKB * 1024 * NS);
        static_assert(ts::kVecFloats % 4 == 0 && ts::kVecFloats / 4 <= 512, "vector block");
        const int i0 = threadIdx.x, i1 = threadIdx.x + 256;
        const u32x4 v0 = gv[i0];
        const u32x4 v1 = gv[i1 < ts::kVecFloats / 4 ? i1 : i0];
        reinterpret_cast<u32x4*>(vec)[i0] = v0;
        if (i1 < ts::kVecFloats / 4) reinterpret_cast<u32x4*>(vec)[i1] = v1;
    }
    const int64_t tile0 = (int64_t)blockIdx.x * 2;                  // first of this workgroup's two 32-point column tiles
    int64_t pc[2];
    bool valid[2], zero_rows[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int64_t pt = (tile0 + p) * 32 + j;
        valid[p] = pt < a.n;
        pc[p] = valid[p] ? pt : (a.n - 1);
        zero_rows[p] = ((tile0 + p) * 32 + 32 > a.n) && !valid[p];    // saved rows of padding points are zero
    }
    const ts::Ident I = ts::make_ident(j, h);
    SavedView sv = saved_view(a.saved, a.n_pad, NS);
    const bool save = a.saved != nullptr;
    const int64_t tiles32 = a.n_pad / 32;
    auto chunk = [&](const int kb) __attribute__((always_inline)) { return pk + (long)kb * 1024 * NS; };

    f32x16 acc[2][2];
    Frag<NS> F[2][2][2];                     // [tile t][column tile p][k-step of the tile's pair]: the epilogue's output fragments
    auto x_store_all = [&]() __attribute__((always_inline)) {      // this wave's tiles 2w, 2w+1 are k-steps 4w .. 4w+3 of the next layer
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) ts::x_store<NS>(xl, 4 * w + 2 * t + kk, p, F[t][p][kk]);
    };
    auto init_all = [&](const int which, const float scale) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            ts::acc_init(acc[t][0], vec, which, h, 2 * w + t, scale);
            acc[t][1] = acc[t][0];
        }
    };

    ts::Head<NS, 2> H;
    ts::gemm_head<NS, 12, 2>(chunk(kF0 + 2 * w * 12), lane, H);
    // the normalised coordinates of the lane's two points, once: the wave's k-steps 3w .. 3w+2 lie in coordinates ca <= cb (wave-uniform), and the
    // Jacobian tail of waves 0..2 contracts with d pe / d xi_w, w == cb there
    const int ca = (3 * w) >> 2, cb = (3 * w + 2) >> 2;
    float xia[2], xib[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        xia[p] = ts::xi_of(a, ca, pc[p]);
        xib[p] = ts::xi_of(a, cb, pc[p]);
    }
    // ---------------- coordinate features pe3 -> X (k-steps 0..11): this thread builds k-steps 3w .. 3w+2 of both column tiles
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            Frag<NS> f;
            ts::pe3_frag<NS>(f, a, 3 * w + kk, h, (((3 * w + kk) >> 2) == ca) ? xia[p] : xib[p]);
            ts::x_store<NS>(xl, 3 * w + kk, p, f);
        }
    TS_STAMP(1);
    ts::barrier_lds();
    // ---------------- L1: pre1 = w1 . pe + b1 ; h1 = relu -> X ; relu mask bits -> m1w ; hdot = (w2^T wo) . h1 (this wave's 64 channels)
    u32 m1w[2] = {0u, 0u};
    init_all(kVecB1, 1.0f);
    TS_STAMP(2);
    ts::gemm<NS, 12, 2>(chunk(kF0 + 2 * w * 12), xl, lane, H, acc);
    TS_STAMP(3);
    float hdot[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {            // hdot first, on max(pre1, 0) by v_med3 (no compare result shared with the mask loop below)
        const f32x4* av = reinterpret_cast<const f32x4*>(vec + kVecA2 * 256 + h * 128 + (2 * w + t) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 aq = av[q];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                hdot[p] = fmaf(aq[0], __builtin_amdgcn_fmed3f(acc[t][p][4 * q], 0.f, __builtin_inff()), hdot[p]);
                hdot[p] = fmaf(aq[1], __builtin_amdgcn_fmed3f(acc[t][p][4 * q + 1], 0.f, __builtin_inff()), hdot[p]);
                hdot[p] = fmaf(aq[2], __builtin_amdgcn_fmed3f(acc[t][p][4 * q + 2], 0.f, __builtin_inff()), hdot[p]);
                hdot[p] = fmaf(aq[3], __builtin_amdgcn_fmed3f(acc[t][p][4 * q + 3], 0.f, __builtin_inff()), hdot[p]);
            }
        }
    }
    asm volatile("" : "+v"(hdot[0]), "+v"(hdot[1]));      // the dot products are finished BEFORE the next layer's first weight fragments are requested (register pressure)
    ts::gemm_head<NS, 16, 2>(chunk(kFA + 2 * w * 16), lane, H);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = acc[t][p][r], p1 = acc[t][p][r + 1];
                const bool on0 = p0 > 0.f, on1 = p1 > 0.f;
                m1w[p] |= (on0 ? (1u << (16 * t + r)) : 0u) | (on1 ? (2u << (16 * t + r)) : 0u);
                frag_set2<NS>(F[t][p][r >> 3], (r & 7) >> 1, on0 ? p0 : 0.f, on1 ? p1 : 0.f);
            }
    // make the mask words opaque HERE: left alone, the compiler proves (m1w >> k) & 1 == the k-th compare and keeps all 64 compare results
    // alive (as lane masks in SGPRs, spilled through v_writelane, and in scratch) until the y layer's epilogue instead of the two words
    asm volatile("" : "+v"(m1w[0]), "+v"(m1w[1]));
    if (save) {
#pragma unroll
        for (int p = 0; p < 2; ++p)          // word w of the lane's uint4 = tiles 2w (low half), 2w+1 (high half): the ring kernel's m1w[T >> 1]
            reinterpret_cast<u32*>(sv.m1 + ((int64_t)net * tiles32 + tile0 + p) * 64 + lane)[w] = m1w[p];
    }
    TS_STAMP(4);
    ts::barrier_lds();                       // everybody is done reading pe3
    x_store_all();
    TS_STAMP(5);
    ts::barrier_lds();
    // ---------------- pre2 = A h1 + B pe6 + (W1 cvec + bf1)
    init_all(kVecC2, 1.0f);
    TS_STAMP(6);
    ts::gemm<NS, 16, 2>(chunk(kFA + 2 * w * 16), xl, lane, H, acc);
    TS_STAMP(7);
    ts::gemm_head<NS, 12, 2>(chunk(kFB + 2 * w * 12), lane, H);
    float ddot[2] = {0.f, 0.f};              // (Wd^T wo) . pe6 over this wave's k-steps
    {   // data features pe6 (SineCosPE(6,16) of coord_data): k-steps 3w .. 3w+2 of both column tiles, built while the accumulators wait
        Frag<NS> f6[3][2];
        const float* bv = vec + kVecBv * 256;
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
#pragma unroll
            for (int p = 0; p < 2; ++p) ts::pe6_frag_dot<NS>(f6[kk][p], a, 3 * w + kk, h, pc[p], bv, ddot[p]);
        TS_STAMP(8);
        ts::barrier_lds();                   // everybody is done reading h1
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
#pragma unroll
            for (int p = 0; p < 2; ++p) ts::x_store<NS>(xl, 3 * w + kk, p, f6[kk][p]);
        TS_STAMP(9);
        ts::barrier_lds();
    }
    TS_STAMP(10);
    ts::gemm<NS, 12, 2>(chunk(kFB + 2 * w * 12), xl, lane, H, acc);
    TS_STAMP(11);
    if (save || a.jac_n) ts::gemm_head<NS, 16, 2>(chunk(kFAT + 2 * w * 16), lane, H);
    // ---------------- out = u . relu(pre2) + 2 wo . c + const ; t2 = m2 (.) u -> X ; M2 -> saved
    float adot[2] = {0.f, 0.f};
    Frag<1> MK[2][2][2];                     // relu-2 mask as bf16 0 / 1 fragments (one plane)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const f32x4* uvp = reinterpret_cast<const f32x4*>(vec + kVecU * 256 + h * 128 + (2 * w + t) * 16);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            Frag<1>& mk0 = MK[t][p][0];
            Frag<1>& mk1 = MK[t][p][1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 uq = uvp[q];
                const float uu[4] = {uq[0], uq[1], uq[2], uq[3]};
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const int r = 4 * q + i;
                    const float p0 = acc[t][p][r], p1 = acc[t][p][r + 1];
                    const bool on0 = p0 > 0.f, on1 = p1 > 0.f;
                    const float t0 = on0 ? uu[i] : 0.f, t1 = on1 ? uu[i + 1] : 0.f;          // t2 = m2 (.) u
                    adot[p] = fmaf(p0, t0, adot[p]);                                       // relu(p) * u == p * (m2 * u)
                    adot[p] = fmaf(p1, t1, adot[p]);
                    frag_set2<NS>(F[t][p][r >> 3], (r & 7) >> 1, t0, t1);
                    const u32 mw = (on0 ? 0x3F80u : 0u) | (on1 ? 0x3F800000u : 0u);
                    if (r < 8) mk0.w[0][(r & 7) >> 1] = mw; else mk1.w[0][(r & 7) >> 1] = mw;
                }
            }
#if !TS_DEFER_SAVES
            if (save) ts::save_tile_k<1, 1>(sv.M2, net, tile0 + p, 2 * w + t, lane, I, zero_rows[p], mk0, mk1);
#endif
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {            // this wave's share of the field: its 64 channels and its 3 k-steps of pe6, both halves of the wave
        float o = adot[p] + 2.0f * (hdot[p] + ddot[p]);
        o += __shfl_xor(o, 32);
        if (h == 0) red[w * 64 + p * 32 + j] = o;
    }
    TS_STAMP(12);
    ts::barrier_lds();
    x_store_all();
    TS_STAMP(13);
    ts::barrier_lds();
    if (w == 0) {                            // lane (j, h) finishes point j of column tile h: the four waves' shares in a fixed order
        const int64_t pt = (tile0 + h) * 32 + j;
        if (pt < a.n) {
            const float const0 = vec[kNumVecs * 256];          // wo . bf2 + bo + 2 wo . cvec
            if (vec[kNumVecs * 256 + 1] != 1.0f) __builtin_trap();     // the packed stream is not in the fused five-GEMM form (its tag sits behind const0): wrong fields otherwise
            const float o = (red[0 * 64 + h * 32 + j] + red[1 * 64 + h * 32 + j]) + (red[2 * 64 + h * 32 + j] + red[3 * 64 + h * 32 + j]);
            a.out_n[pt * 6 + net] = o + const0 + (a.ref ? a.ref : a.coord_data)[pt * 6 + net];           // + ref_data (variable_net.py:86)
        }
    }
    if (!save && !a.jac_n) return;
    // ---------------- reverse sweep: y = A^T t2 + 2 w2^T wo ; t1 = m1 (.) y -> X (+ saved T1)
    init_all(kVecA2, 2.0f);
    TS_STAMP(14);
#if TS_DEFER_SAVES
    {
        auto side = [&](const int ks) __attribute__((always_inline)) {            // M2: four (tile, column tile) units over the 16 k-steps
            if (!save) return;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ks == 4 * u + 1) ts::save_plane_k(sv.M2, net, 1, 0, tile0 + (u & 1), 2 * w + (u >> 1), lane, I, zero_rows[u & 1], MK[u >> 1][u & 1][0].w[0], MK[u >> 1][u & 1][1].w[0]);
        };
        ts::gemm<NS, 16, 2, false>(chunk(kFAT + 2 * w * 16), xl, lane, H, acc, side);
    }
#else
    ts::gemm<NS, 16, 2>(chunk(kFAT + 2 * w * 16), xl, lane, H, acc);
#endif
    TS_STAMP(15);
    if (a.jac_n && w < 3) ts::gemm_head<NS, 16, 2>(chunk(kF5 + 2 * w * 16), lane, H);
    // F (the t2 fragments) is rewritten by this epilogue: every wave has finished reading X(t2) only after the barrier below
    auto side_planes = [&](const KMat& m, const int ks) __attribute__((always_inline)) {       // 4 x NS (tile, column tile, plane) units over 16 k-steps
        if (!save) return;
#pragma unroll
        for (int u = 0; u < 4 * NS; ++u) {
            const int tp = u / NS, s_ = u % NS;
            if (ks == (16 / (4 * NS)) * u + 1)
                ts::save_plane_k(m, net, NS, s_, tile0 + (tp & 1), 2 * w + (tp >> 1), lane, I, zero_rows[tp & 1], F[tp >> 1][tp & 1][0].w[s_], F[tp >> 1][tp & 1][1].w[s_]);
        }
    };
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const u32 bits = m1w[p] >> (16 * t + r);
                frag_set2<NS>(F[t][p][r >> 3], (r & 7) >> 1, (bits & 1u) ? acc[t][p][r] : 0.f, (bits & 2u) ? acc[t][p][r + 1] : 0.f);
            }
#if TS_DEFER_SAVES
            if (save && (!a.jac_n || w >= 3)) ts::save_tile_k<NS, NS>(sv.T1, net, tile0 + p, 2 * w + t, lane, I, zero_rows[p], F[t][p][0], F[t][p][1]);
#else
            if (save) ts::save_tile_k<NS, NS>(sv.T1, net, tile0 + p, 2 * w + t, lane, I, zero_rows[p], F[t][p][0], F[t][p][1]);
#endif
        }
    if (!a.jac_n) return;
    TS_STAMP(16);
    ts::barrier_lds();
    x_store_all();
    TS_STAMP(17);
    ts::barrier_lds();
    // ---------------- gpe = w1^T t1 (6 tiles: waves 0..2; both tiles of wave w belong to coordinate c = w), contracted with d(pe)/d(xi)
    if (w >= 3) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) { acc[t][0] = (f32x16)0.f; acc[t][1] = (f32x16)0.f; }
    TS_STAMP(18);
#if TS_DEFER_SAVES
    {
        auto side = [&](const int ks) __attribute__((always_inline)) { side_planes(sv.T1, ks); };
        ts::gemm<NS, 16, 2, false>(chunk(kF5 + 2 * w * 16), xl, lane, H, acc, side);
    }
#else
    ts::gemm<NS, 16, 2>(chunk(kF5 + 2 * w * 16), xl, lane, H, acc);
#endif
    TS_STAMP(19);
    {
        const int c = w;
        float jc[2] = {0.f, 0.f};
#if DPN_DERIV
        float hc[2] = {0.f, 0.f}, tc[2] = {0.f, 0.f};        // second / third derivatives along xi_c
#endif
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float d[16];
#if DPN_DERIV
                float d2[16], d3[16];
                ts::dpe_tile_derivs<NS>(d, d2, d3, a, t, h, xib[p]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    hc[p] = fmaf(acc[t][p][r], d2[r], hc[p]);
                    tc[p] = fmaf(acc[t][p][r], d3[r], tc[p]);
                }
#else
                ts::dpe_tile<NS>(d, a, t, h, xib[p]);
#endif
#pragma unroll
                for (int r = 0; r < 16; ++r) jc[p] = fmaf(acc[t][p][r], d[r], jc[p]);
            }
            jc[p] += __shfl_xor(jc[p], 32);
#if DPN_DERIV
            hc[p] += __shfl_xor(hc[p], 32);
            tc[p] += __shfl_xor(tc[p], 32);
#endif
        }
        // lane (j, h) stores point j of column tile h; chain rule through x / dx / (lon - 1), in the reference's backward order
        const float mine = h ? jc[1] : jc[0];
        const int64_t pt = (tile0 + h) * 32 + j;
        if (pt < a.n) {
            const float g1 = (c == 0) ? a.geo.lon_m1 : (c == 1) ? a.geo.lat_m1 : a.geo.pred_t_span;
            const float g2 = (c == 0) ? a.geo.dx : (c == 1) ? a.geo.dy : 1.0f;
            a.jac_n[(pt * 6 + net) * 3 + c] = mine / g1 / g2;
#if DPN_DERIV
            if (hess_n) hess_n[(pt * 6 + net) * 3 + c] = (h ? hc[1] : hc[0]) / g1 / g2 / g1 / g2;                  // the factor once per order
            if (d3_n) d3_n[(pt * 6 + net) * 3 + c] = (h ? tc[1] : tc[0]) / g1 / g2 / g1 / g2 / g1 / g2;
#endif
        }
    }
    TS_STAMP(20);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Backward, stage 1 (per-point cotangent streams -> operands of the weight-gradient reductions), tile-split form.  Same arithmetic and same operand
// layout as dpn_bwd_kernel (bit-identical Z0, Z1, pe6 table, gnet); decomposition as dpn_fwd_tiles_kernel: 64 points per workgroup, wave w owns tiles
// 2w, 2w+1 of both column tiles, the cotangent fragments are shared through LDS, the weights come L2 -> VGPR.
//   Z0 = g pe + sum_c gJ_c d pe / d xi_c                      -> X; K-layout rows (operand of dw1 = T1^T Z0) in plain bf16 and in the second-derivative
//                                                                kernel only: in the hi+lo mode the rows are NOT written, dpn_wgrad_kernel forms them from
//                                                                the per-point fp32 pe3 table (column tile ct by the workgroups of net ct), gJ and the header
//                                                                that this kernel writes instead (OperandView: 313 instead of 454 MB per launch at 37 265 points)
//   Z1 = m1 (.) (w1 Z0 + g b1)                                -> K-layout rows (operand of S1 = M2^T Z1)
//   net 0 only: the per-point table pe6                       -> K-layout rows (from which dpn_wgrad_kernel forms G6 = g pe6 of every net: OperandView)
// Round 5: Z = w2 Z1 + Wd G6 + g (b2 + bd + e) is no longer formed.  It existed only as the Y operand of G = M2^T Z, and being linear in
// (Z1, G6, g) that product is S1 w2^T + S2 Wd^T + (M2^T g) (x) cvec: one exact-fp32 GEMM per net behind the reduction (dpn_finish_gside_kernel)
// instead of 114 688 of this kernel's 163 840 MACs per point and net, a 1-KB row written per point and net, and a fourth points-reduction product.
// LDS: the X image of 12 k-steps (48 KB in the hi+lo mode) + the b1 vector: 49 KB, <= 168 registers => THREE workgroups per CU (the kernel is a chain of
// feature evaluation, one short multiply loop and streaming stores: more waves in flight is what hides them).
template <int NS>
#if DPN_DERIV
__global__ __launch_bounds__(256, 3) void dpn_bwd_tiles_deriv_kernel(BwdArgs a, const float* g_hxi) {
#else
__global__ __launch_bounds__(256, 3) void dpn_bwd_tiles_kernel(BwdArgs a) {
#endif
    constexpr int kXBytes = 12 * 2 * NS * 1024;
    __shared__ __attribute__((aligned(16))) char lds[kXBytes + 1024];
    const int net = (int)blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    TS_STAMP(0);
    const char* pk = a.packed + (long)net * pack_bytes_per_net(NS);
#if TS_PRIO == 2
    __builtin_amdgcn_s_setprio(1);
#endif
    float* vec = reinterpret_cast<float*>(lds + kXBytes) - kVecB1 * 256;     // only b1 is read (acc_init indexes vec + which * 256)
    char* xl = lds + lane * 16;
    {
        const float* gv = reinterpret_cast<const float*>(pk + (long)kPackKB * 1024 * NS) + kVecB1 * 256;
        reinterpret_cast<float*>(lds + kXBytes)[threadIdx.x] = gv[threadIdx.x];
    }
    auto chunk = [&](const int kb) __attribute__((always_inline)) { return pk + (long)kb * 1024 * NS; };
    ts::Head<NS, 2> H;
    ts::gemm_head<NS, 12, 2>(chunk(kS0 + 2 * w * 12), lane, H);
    const int64_t tile0 = (int64_t)blockIdx.x * 2;
    const int64_t tiles32 = a.n_pad / 32;
    int64_t pc[2];
    float g[2];                                               // cotangent of the lane's point in column tile p (zero for padding points)
    const float gsc = a.g_scale ? a.g_scale[0] : 1.0f;        // an upstream cotangent on unit-cotangent streams (dpn_bwd_points_scaled)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int64_t pt = (tile0 + p) * 32 + j;
        const bool valid = pt < a.n;
        pc[p] = valid ? pt : (a.n - 1);
        g[p] = valid ? gsc * a.g_out[pc[p] * 6 + net] : 0.f;
    }
    const ts::Ident I = ts::make_ident(j, h);
    SavedView sv = saved_view(a.saved, a.n_pad, NS);
    OperandView ov = operand_view(a.operands, a.n_pad, NS);
    u32 m1w[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) m1w[p] = reinterpret_cast<const u32*>(sv.m1 + ((int64_t)net * tiles32 + tile0 + p) * 64 + lane)[w];
    // Z0 in the table form (OperandView): the hi+lo mode (this kernel never has caller-encoded coordinates); the second-derivative cotangent keeps the stored form
    constexpr bool kTab = NS == 2 && !DPN_DERIV;
    write_operand_header(ov, kTab ? kZ0Table : kZ0Stored, a.freqs);
    if (w == 0) {                                             // lane (j, h): point j of column tile h
        const int64_t pt = (tile0 + h) * 32 + j;
        ov.gnet[(int64_t)net * a.n_pad + pt] = (pt < a.n) ? gsc * a.g_out[pt * 6 + net] : 0.f;
    } else if (kTab) {                                    // waves 1..3: the coordinate cotangent gJ_c, c = w - 1, as the Z0 units below read it
        const int64_t pt = (tile0 + h) * 32 + j;
        ov.gj[((int64_t)net * 3 + (w - 1)) * a.n_pad + pt] = (a.g_jxi && pt < a.n) ? gsc * a.g_jxi[(pt * 6 + net) * 3 + (w - 1)] : 0.f;
    }
    // ---------------- Z0 -> X (k-steps 0..11) and K-layout rows: wave w builds the (column tile of Z0, point tile) units 3w .. 3w+2.  The rows go
    // out at once (not deferred into the multiply loop as in the forward kernel): nothing of them stays live, the kernel fits 168 registers and
    // three workgroups share a CU -- with one short multiply loop per workgroup, other workgroups are what hides the stores
#pragma unroll
    for (int uu = 0; uu < 3; ++uu) {
        const int u = 3 * w + uu, ct = u >> 1, p = u & 1;     // wave-uniform
        const float gp = p ? g[1] : g[0];
        const int64_t pcp = p ? pc[1] : pc[0];
        float gjc = 0.f;
        if (a.g_jxi && ((tile0 + p) * 32 + j) < a.n) gjc = gsc * a.g_jxi[(pcp * 6 + net) * 3 + (ct >> 1)];
        const float xi = ts::xi_of(a, ct >> 1, pcp);          // both k-steps of the unit lie in coordinate ct >> 1
        Frag<NS> f0, f1;
#if DPN_DERIV
        float ghc = 0.f;
        if (g_hxi && ((tile0 + p) * 32 + j) < a.n) ghc = gsc * g_hxi[(pcp * 6 + net) * 3 + (ct >> 1)];
        ts::z0_frag_derivs<NS>(f0, a, 2 * ct, h, xi, gp, gjc, ghc);
        ts::z0_frag_derivs<NS>(f1, a, 2 * ct + 1, h, xi, gp, gjc, ghc);
#else
        float sc0[8], sc1[8];
        ts::z0_frag<NS>(f0, a, 2 * ct, h, xi, gp, gjc, sc0);
        ts::z0_frag<NS>(f1, a, 2 * ct + 1, h, xi, gp, gjc, sc1);
#endif
        ts::x_store<NS>(xl, 2 * ct, p, f0);
        ts::x_store<NS>(xl, 2 * ct + 1, p, f1);
#if !DPN_DERIV
        if constexpr (NS == 2) {                              // table form: the Z0 rows are not written; column tile ct of the fp32 table by the workgroups of net ct
            if (ct == net) store_table_k(ov.Z0, tile0 + p, ct, lane, I.a, I.b, sc0, sc1);
        } else
#endif
        ts::save_tile_k<NS, NS>(ov.Z0, net, tile0 + p, ct, lane, I, false, f0, f1);
    }
    TS_STAMP(1);
    ts::barrier_lds();
    TS_STAMP(2);
    // ---------------- Z1 = m1 (.) (w1 Z0 + g b1) -> K-layout rows
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p) ts::acc_init(acc[t][p], vec, kVecB1, h, 2 * w + t, g[p]);
    ts::gemm<NS, 12, 2, false, ts::NoSide, false>(chunk(kS0 + 2 * w * 12), xl, lane, H, acc);
    TS_STAMP(3);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            Frag<NS> F0, F1;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const u32 bits = m1w[p] >> (16 * t + r);
                frag_set2<NS>(r < 8 ? F0 : F1, (r & 7) >> 1, (bits & 1u) ? acc[t][p][r] : 0.f, (bits & 2u) ? acc[t][p][r + 1] : 0.f);
            }
            ts::save_tile_k<NS, NS>(ov.Z1, net, tile0 + p, 2 * w + t, lane, I, false, F0, F1);
        }
    TS_STAMP(4);
    if (net != 0) return;
    // ---------------- net 0: the per-point pe6 table (OperandView) -> K-layout rows, units as for Z0
#pragma unroll
    for (int uu = 0; uu < 3; ++uu) {
        const int u = 3 * w + uu, ct = u >> 1, p = u & 1;
        const int64_t pcp = p ? pc[1] : pc[0];
        Frag<NS> f0, f1;
        ts::pe6_frag<NS>(f0, a, 2 * ct, h, pcp);
        ts::pe6_frag<NS>(f1, a, 2 * ct + 1, h, pcp);
        ts::save_tile_k<NS, NS>(ov.PE6, 0, tile0 + p, ct, lane, I, false, f0, f1);
    }
    TS_STAMP(5);
}
