// The point kernels of the ring form (one 512-register wave per SIMD owns 32 points; weight fragments through an LDS-DMA ring), included twice by
// dpn_point.hip:
//   DPN_DERIV 0:  dpn_fwd_kernel, dpn_bwd_kernel -- what the fused step launches;
//   DPN_DERIV 1:  dpn_fwd_deriv_kernel (+ second and third coordinate derivatives, dpn_fwd_ref_derivs) and dpn_bwd_deriv_kernel (+ their cotangent g_hxi in
//                 the Z0 seed, dpn_bwd_points_derivs).
// One text, gated by the preprocessor, so that the first pass is token for token the kernels as they were and compiles to the same code (a shared
// always-inline body with a template flag does not: the inlined copy of the argument block reorders the kernel and the schedule with it).

template <int NS>
#if DPN_DERIV
__global__ __launch_bounds__(256, 1) void dpn_fwd_deriv_kernel(FwdArgs a, float* hess_n, float* d3_n) {
#else
__global__ __launch_bounds__(256, 1) void dpn_fwd_kernel(FwdArgs a) {
#endif
    __shared__ __attribute__((aligned(16))) char lds_w[Pipe<NS>::kRing * Pipe<NS>::kSlotBytes];

    const int net = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    const int64_t tile32 = (int64_t)blockIdx.x * 4 + wave;
    const char* pk = a.packed + (long)net * pack_bytes_per_net(NS);
    __shared__ __attribute__((aligned(16))) float lds_vec_store[kNumVecs * 256 + 4];
#ifdef DPN_TIMELINE
    u32 tl = 0;
    DPN_STAMP(0);
#endif
    {   // permuted fp32 vectors of this net -> LDS (published by the barrier below, before the first DMA is issued)
        const float* gv = reinterpret_cast<const float*>(pk + (long)kPackKB * 1024 * NS);
        for (int i = threadIdx.x; i < kNumVecs * 256 + 4; i += 256) lds_vec_store[i] = gv[i];
    }
    const unsigned lds_vec = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds_vec_store;
    Lane L;
    lane_init(L, a.x, a.y, a.t, a.n, a.freqs, a.geo, tile32);
    const int h = L.h;
    const bool partial = (tile32 * 32 + 32 > a.n);
    const int64_t pc = L.valid ? L.pt : (a.n - 1);
    float cd6[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) cd6[c] = a.coord_data[pc * 6 + c];
    const float ref_data = (a.ref ? a.ref : a.coord_data)[pc * 6 + net];
    SavedView sv = saved_view(a.saved, a.n_pad, NS);
    const bool save = a.saved != nullptr;

    Pipe<NS> pipe;
    __syncthreads();
    pipe.init(pk, lds_w, 54);
    pipe.prime();
    DPN_STAMP(1);

    f32x16 acc[8];
    u32 m1w[4] = {0u, 0u, 0u, 0u};
    Frag<NS> actA[16], actB[16];

    // ---------------- L1: pre1 = w1 . pe + b1 ; h1 = relu -> actA ; relu mask -> m1w
    auto epi1 = [&](const int T) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float p0 = acc[T][r], p1 = acc[T][r + 1];
            const bool on0 = p0 > 0.f, on1 = p1 > 0.f;
            m1w[T >> 1] |= (on0 ? (1u << (16 * (T & 1) + r)) : 0u) | (on1 ? (2u << (16 * (T & 1) + r)) : 0u);
            frag_set2<NS>(actA[2 * T + (r >> 3)], (r & 7) >> 1, on0 ? p0 : 0.f, on1 ? p1 : 0.f);
        }
        // pin the mask word HERE: left alone, the scheduler postpones the compares to the first use of m1w (after fc1) and keeps the
        // tile's 16 pre-activations alive until then -- in AGPRs for bf16, in SCRATCH for the hi+lo mode, whose reloads drain the DMA ring
        asm volatile("" : "+v"(m1w[T >> 1]));
    };
    {
        Frag<NS> pe[12];
        if (a.pe_in) load_pe3<NS>(a.pe_in + pc * kPe, h, pe, 1.0f);     // caller-encoded coordinates (PhysicsNet.forward surface)
        else build_pe3<NS, false>(L, pe, 0.f, nullptr);
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            acc_init_vec(acc[T], lds_vec, kVecB1, h, T, 1.0f);
            if (T == 0) DPN_STEP(T, 12, false, pe, acc[T], (void)0);
            else DPN_STEP(T, 12, false, pe, acc[T], epi1(T - 1));
        }
        epi1(7);
    }
    // ---------------- L2 + data: c = w2 . h1 + Wd . pe6 + (b2 + bd + e) -> actB ; cdot = wo . c
    float cdot = 0.f;
    auto epi2 = [&](const int T) __attribute__((always_inline)) {
        Vec16 wv;
        lds_read_vec16(wv, vec_addr(lds_vec, kVecWo, h, T));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cdot = fmaf(wv.q[q][0], acc[T][4 * q], cdot); cdot = fmaf(wv.q[q][1], acc[T][4 * q + 1], cdot);
            cdot = fmaf(wv.q[q][2], acc[T][4 * q + 2], cdot); cdot = fmaf(wv.q[q][3], acc[T][4 * q + 3], cdot);
        }
#pragma unroll
        for (int r = 0; r < 16; r += 2) frag_set2<NS>(actB[2 * T + (r >> 3)], (r & 7) >> 1, acc[T][r], acc[T][r + 1]);
    };
    {
        // pass A: all eight tiles of w2 . h1 (h1 = actA dies here); pass B: + Wd . pe6, epilogue one tile late
        // the data PE (96 sin/cos + packing per lane) is built two k-steps per tile UNDER the MFMAs of pass A, whose tiles have no
        // epilogue of their own, and pinned there (left to the scheduler it lands in one block in front of pass B)
        Frag<NS> pe6[12];
        auto pe6_part = [&](const int T) __attribute__((always_inline)) {
            if (NS == 1 && T < 6) {                              // hi+lo fragments: twice the registers, the early build spills
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    build_pe6_ks<NS>(L, cd6, pe6, 1.0f, 2 * T + j);
#pragma unroll
                    for (int s2 = 0; s2 < NS; ++s2) asm volatile("" : "+v"(pe6[2 * T + j].w[s2]));
                }
            }
        };
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            acc_init_vec(acc[T], lds_vec, kVecCvec, h, T, 1.0f);
            DPN_STEP(8 + T, 16, false, actA, acc[T], pe6_part(T));
        }
        if constexpr (NS == 2) build_pe6<NS>(L, cd6, pe6, 1.0f);
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            if (T == 0) DPN_STEP(16 + T, 12, false, pe6, acc[T], (void)0);
            else DPN_STEP(16 + T, 12, false, pe6, acc[T], epi2(T - 1));
        }
        epi2(7);
    }
    // ---------------- fc1: pre2 = W1 . c + bf1 ; a = relu ; out = u.a + 2 wo.c + const ; t2 = m2 (.) u -> actA ; M2 -> saved
    const float const0 = lds_read_f32(lds_vec + kNumVecs * 256 * 4);
    // the packed stream carries its form behind const0 (dpn_pack_vectors): this kernel multiplies the seven-GEMM stream.  A buffer packed in the fused
    // form (or a DPN_FWD_KERNEL switch flipped between pack and launch, ADVICE r5) would give silently wrong fields: trap instead.
    if (lds_read_f32(lds_vec + (kNumVecs * 256 + 1) * 4) != 0.f) __builtin_trap();
    float adot = 0.f;
    auto epi3 = [&](const int T) __attribute__((always_inline)) {
        Frag<1> mk0, mk1;
        Vec16 uv;
        lds_read_vec16(uv, vec_addr(lds_vec, kVecU, h, T));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float uu[4] = {uv.q[q][0], uv.q[q][1], uv.q[q][2], uv.q[q][3]};
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                const int r = 4 * q + i;
                const float p0 = acc[T][r], p1 = acc[T][r + 1];
                const bool on0 = p0 > 0.f, on1 = p1 > 0.f;
                const float t0 = on0 ? uu[i] : 0.f, t1 = on1 ? uu[i + 1] : 0.f;      // t2 = m2 (.) u
                adot = fmaf(p0, t0, adot);                                           // relu(p) * u == p * (m2 * u): no separate max
                adot = fmaf(p1, t1, adot);
                frag_set2<NS>(actA[2 * T + (r >> 3)], (r & 7) >> 1, t0, t1);
                const u32 mw = (on0 ? 0x3F80u : 0u) | (on1 ? 0x3F800000u : 0u);
                if (r < 8) mk0.w[0][(r & 7) >> 1] = mw; else mk1.w[0][(r & 7) >> 1] = mw;
            }
        }
        // pin t2 and the mask words in VGPRs HERE: left alone, the scheduler keeps the 128 compare results as lane masks in SGPRs
        // (spilling them through v_writelane / v_readlane) and materialises every select in one 1000-instruction block after the GEMM
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) asm volatile("" : "+v"(actA[2 * T].w[s2]), "+v"(actA[2 * T + 1].w[s2]));
        asm volatile("" : "+v"(mk0.w[0]), "+v"(mk1.w[0]));
        // (Saving the mask as bit words instead -- the compares' lane masks ARE the transposed words, 1 KB per tile and net instead of
        //  16 KB, v_writelane into one VGPR -- and expanding them to 0 / 1 fragments in dpn_wgrad_kernel was built and measured: this
        //  kernel unchanged, dpn_wgrad_kernel +4.5 % (the expansion sits in front of the MFMAs of its product's workgroups), step +1.1 %
        //  hi+lo and +3.2 % single bf16 on the same box.  Not kept: tools/experiments/m2_bit_masks.patch.)
        if (save) store_tile_k<1, 1>(sv.M2, net, tile32, T, L, mk0, mk1, partial);
    };
#pragma unroll
    for (int T = 0; T < 8; ++T) {
        acc_init_vec(acc[T], lds_vec, kVecBf1, h, T, 1.0f);
        if (T == 0) DPN_STEP(24 + T, 16, false, actB, acc[T], (void)0);
        else DPN_STEP(24 + T, 16, false, actB, acc[T], epi3(T - 1));
    }
    epi3(7);
    {
        float o = adot + 2.0f * cdot;
        o += __shfl_xor(o, 32);
        if (L.valid && h == 0) a.out_n[L.pt * 6 + net] = o + const0 + ref_data;   // + ref_data (variable_net.py:86)
    }
    if (save) sv.m1[((int64_t)net * (a.n_pad / 32) + tile32) * 64 + L.lane] = make_uint4(m1w[0], m1w[1], m1w[2], m1w[3]);
    if (!save && !a.jac_n) { pipe.drain(); return; }
    // ---------------- reverse sweep: v = W1^T t2 + 2 wo -> actB (not saved: SavedView)
    auto epiv = [&](const int T) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) frag_set2<NS>(actB[2 * T + (r >> 3)], (r & 7) >> 1, acc[T][r], acc[T][r + 1]);
    };
#pragma unroll
    for (int T = 0; T < 8; ++T) {
        acc_init_vec(acc[T], lds_vec, kVecWo, h, T, 2.0f);
        if (T == 0) DPN_STEP(32 + T, 16, false, actA, acc[T], (void)0);
        else DPN_STEP(32 + T, 16, false, actA, acc[T], epiv(T - 1));
    }
    epiv(7);
    // ---------------- y = w2^T v ; t1 = m1 (.) y -> actA (+ saved T1)
    auto epiy = [&](const int T) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const u32 bits = m1w[T >> 1] >> (16 * (T & 1) + r);
            frag_set2<NS>(actA[2 * T + (r >> 3)], (r & 7) >> 1, (bits & 1u) ? acc[T][r] : 0.f, (bits & 2u) ? acc[T][r + 1] : 0.f);
        }
        if (save) store_tile_k<NS, NS>(sv.T1, net, tile32, T, L, actA[2 * T], actA[2 * T + 1], partial);
    };
#pragma unroll
    for (int T = 0; T < 8; ++T) {
        acc[T] = (f32x16)0.f;
        if (T == 0) DPN_STEP(40 + T, 16, false, actB, acc[T], (void)0);
        else DPN_STEP(40 + T, 16, false, actB, acc[T], epiy(T - 1));           // the w1^T chunks always exist: prefetching them is harmless
    }
    epiy(7);
    if (!a.jac_n) { pipe.drain(); return; }
    // ---------------- gpe = w1^T t1 (6 tiles), contracted with d(pe)/d(xi) in registers
    float jc[3] = {0.f, 0.f, 0.f};
#if DPN_DERIV
    float hc[3] = {0.f, 0.f, 0.f}, tc[3] = {0.f, 0.f, 0.f};        // second / third derivatives along xi_c
#endif
    auto epij = [&](const int T) __attribute__((always_inline)) {
        if (a.pe_in) {
            // caller-encoded coordinates (PhysicsNet.forward surface): hand back d out / d pe_in itself, [N][6][192] in the
            // reference's channel order, and let the caller's autograd chain it through its own encoding (generic path, scattered stores)
            if (L.valid) {
                float* o = a.jac_n + (L.pt * 6 + net) * kPe;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[pe3_ch(2 * T + (r >> 3), h, r & 7)] = acc[T][r];
            }
            return;
        }
#pragma unroll
        for (int rp = 0; rp < 8; ++rp) {                // register pair (sin, cos) of one angle
            const int r = 2 * rp;
            const int ks = 2 * T + (r >> 3), p = (r & 7) >> 1, c = ks >> 2;
            const float fr = L.fr32[4 * (ks & 3) + p];
            float s, co;
            sincos_t<NS>(L.xi[c] * fr, s, co);
            jc[c] = fmaf(acc[T][r], fr * co, jc[c]);
            jc[c] = fmaf(acc[T][r + 1], -fr * s, jc[c]);
#if DPN_DERIV
            const float f2 = fr * fr;                   // d2 pe / d xi^2 = -fr^2 pe, d3 pe / d xi^3 = -fr^2 d pe / d xi
            hc[c] = fmaf(acc[T][r], -f2 * s, hc[c]);
            hc[c] = fmaf(acc[T][r + 1], -f2 * co, hc[c]);
            tc[c] = fmaf(acc[T][r], -f2 * (fr * co), tc[c]);
            tc[c] = fmaf(acc[T][r + 1], -f2 * (-fr * s), tc[c]);
#endif
        }
    };
#pragma unroll
    for (int T = 0; T < 6; ++T) {
        acc[T] = (f32x16)0.f;
        if (T == 0) DPN_STEP(48 + T, 16, false, actA, acc[T], (void)0);
        else DPN_STEP(48 + T, 16, false, actA, acc[T], epij(T - 1));
    }
    epij(5);
    pipe.drain();
#ifdef DPN_TIMELINE
    DPN_STAMP(62);
#ifdef DPN_FWD_PHASES
    if (L.lane >= 56 && L.lane < 62) tl = pipe.ph[L.lane - 56];         // slots 56..61: the phase sums of this wave
#endif
    if (a.timeline) a.timeline[(((int64_t)blockIdx.x * kNets + net) * 8 + wave) * 64 + L.lane] = tl;
#endif
#pragma unroll
    for (int c = 0; c < 3; ++c) jc[c] += __shfl_xor(jc[c], 32);
    if (L.valid && h == 0 && !a.pe_in) {
        float* o = a.jac_n + (L.pt * 6 + net) * 3;
        o[0] = jc[0] / a.geo.lon_m1 / a.geo.dx;          // chain rule through x/dx/(lon-1), in the reference's backward order
        o[1] = jc[1] / a.geo.lat_m1 / a.geo.dy;
        o[2] = jc[2] / a.geo.pred_t_span;
    }
#if DPN_DERIV
#pragma unroll
    for (int c = 0; c < 3; ++c) { hc[c] += __shfl_xor(hc[c], 32); tc[c] += __shfl_xor(tc[c], 32); }
    if (L.valid && h == 0) {                              // physical units: the chain-rule factor once per order
        const float s1[3] = {a.geo.lon_m1, a.geo.lat_m1, a.geo.pred_t_span}, s2[3] = {a.geo.dx, a.geo.dy, 1.0f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (hess_n) hess_n[(L.pt * 6 + net) * 3 + c] = hc[c] / s1[c] / s2[c] / s1[c] / s2[c];
            if (d3_n) d3_n[(L.pt * 6 + net) * 3 + c] = tc[c] / s1[c] / s2[c] / s1[c] / s2[c] / s1[c] / s2[c];
        }
    }
#endif
}

template <int NS>
#if DPN_DERIV
__global__ __launch_bounds__(256, 1) void dpn_bwd_deriv_kernel(BwdArgs a, const float* g_hxi) {
#else
__global__ __launch_bounds__(256, 1) void dpn_bwd_kernel(BwdArgs a) {
#endif
    __shared__ __attribute__((aligned(16))) char lds_w[Pipe<NS>::kRing * Pipe<NS>::kSlotBytes];
    const int net = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    const int64_t tile32 = (int64_t)blockIdx.x * 4 + wave;
    const char* pk = a.packed + (long)net * pack_bytes_per_net(NS);
    __shared__ __attribute__((aligned(16))) float lds_vec_store[kNumVecs * 256 + 4];
    {
        const float* gv = reinterpret_cast<const float*>(pk + (long)kPackKB * 1024 * NS);
        for (int i = threadIdx.x; i < kNumVecs * 256 + 4; i += 256) lds_vec_store[i] = gv[i];
    }
    const unsigned lds_vec = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds_vec_store;
    Lane L;
    lane_init(L, a.x, a.y, a.t, a.n, a.freqs, a.geo, tile32);
    const int h = L.h;
    const int64_t pc = L.valid ? L.pt : (a.n - 1);
    float cd6[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) cd6[c] = a.coord_data[pc * 6 + c];
    const float gsc = a.g_scale ? a.g_scale[0] : 1.0f;
    const float g = L.valid ? gsc * a.g_out[pc * 6 + net] : 0.f;   // padding points carry a zero cotangent: every operand row is zero
    float gj[3] = {0.f, 0.f, 0.f};
    if (a.g_jxi && L.valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gj[c] = gsc * a.g_jxi[(pc * 6 + net) * 3 + c];
    }
#if DPN_DERIV
    float gh[3] = {0.f, 0.f, 0.f};
    if (g_hxi && L.valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gh[c] = gsc * g_hxi[(pc * 6 + net) * 3 + c];
    }
#endif
    SavedView sv = saved_view(a.saved, a.n_pad, NS);
    OperandView ov = operand_view(a.operands, a.n_pad, NS);
    const int64_t tiles32 = a.n_pad / 32;
    const uint4 m1v = sv.m1[((int64_t)net * tiles32 + tile32) * 64 + L.lane];
    const u32 m1w[4] = {m1v.x, m1v.y, m1v.z, m1v.w};
    if (h == 0) ov.gnet[(int64_t)net * a.n_pad + tile32 * 32 + L.j] = g;
    // Z0 in the table form (OperandView): the hi+lo mode on raw coordinates; the second-derivative cotangent (DPN_DERIV) keeps the stored form
    const bool z0_table = NS == 2 && !DPN_DERIV && !a.pe_in;
    write_operand_header(ov, z0_table ? kZ0Table : kZ0Stored, a.freqs);
    if (z0_table && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ov.gj[((int64_t)net * 3 + c) * a.n_pad + tile32 * 32 + L.j] = gj[c];
    }

    Pipe<NS> pipe;
    __syncthreads();
    pipe.init(pk, lds_w, 8);                      // the w1 chunks only (round 5: the w2 / Wd products of Z are gone)
    pipe.prime();

    f32x16 acc[8];
    Frag<NS> actA[16];
#ifdef DPN_TIMELINE
    u32 tl = 0;          // the step macro stamps; the backward kernel does not report (experiment build only)
#endif
    // ---------------- Z0 = g * pe + sum_c gJ_c * dpe/dxi_c ; Z1 = m1 (.) (w1 Z0 + g b1)
    auto epi1 = [&](const int T) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const u32 bits = m1w[T >> 1] >> (16 * (T & 1) + r);
            frag_set2<NS>(actA[2 * T + (r >> 3)], (r & 7) >> 1, (bits & 1u) ? acc[T][r] : 0.f, (bits & 2u) ? acc[T][r + 1] : 0.f);
        }
        store_tile_k<NS, NS>(ov.Z1, net, tile32, T, L, actA[2 * T], actA[2 * T + 1], false);
    };
    {
        Frag<NS> z0[12];
        if (net == 0) {                           // the per-point table of the data features (OperandView): written once for the six nets
            build_pe6<NS>(L, cd6, z0, 1.0f);
#pragma unroll
            for (int ct = 0; ct < 6; ++ct) store_tile_k<NS, NS>(ov.PE6, 0, tile32, ct, L, z0[2 * ct], z0[2 * ct + 1], false);
        }
        if (a.pe_in) load_pe3<NS>(a.pe_in + pc * kPe, h, z0, g);
#if DPN_DERIV
        else build_z0_derivs<NS>(L, z0, g, gj, gh);
#else
        else build_pe3<NS, true>(L, z0, g, gj);
#endif
        if (z0_table) {                           // column tile ct of the per-point fp32 table: the workgroups of net ct (features exactly as build_pe3 forms them)
#pragma unroll
            for (int ct = 0; ct < 6; ++ct) {
                if (ct != net) continue;
                float v[2][8];
#pragma unroll
                for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
                    for (int p = 0; p < 4; ++p) sincos_t<NS>(L.xi[ct >> 1] * L.fr32[4 * ((2 * ct + k2) & 3) + p], v[k2][2 * p], v[k2][2 * p + 1]);
                if constexpr (NS == 2) store_table_k(ov.Z0, tile32, ct, L.lane, L.idA, L.idB, v[0], v[1]);
            }
        } else {
#pragma unroll
            for (int ct = 0; ct < 6; ++ct) store_tile_k<NS, NS>(ov.Z0, net, tile32, ct, L, z0[2 * ct], z0[2 * ct + 1], false);
        }
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            acc_init_vec(acc[T], lds_vec, kVecB1, h, T, g);
            if (T == 0) DPN_STEP(T, 12, false, z0, acc[T], (void)0);
            else DPN_STEP(T, 12, false, z0, acc[T], epi1(T - 1));
        }
        epi1(7);
        pipe.drain();
    }
}
