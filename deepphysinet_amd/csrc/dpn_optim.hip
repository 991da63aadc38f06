// MI355X (gfx950 / CDNA4): global-norm clip + Adam over lists of tensors or flat moment buffers.  A unit of its own.
//
// Kernel inventory
//   dpn_gradnorm_kernel / dpn_gradnorm_reduce_kernel   one fp64 partial per 2048-element chunk, added in a fixed order
//   dpn_adam_kernel                                    the clipped update over AdamTable (pointer lists) or AdamFlat<Ema, Groups, Guard> (flat moment
//                                                      buffers): Ema also moves the weight EMA, Groups reads the hyper-parameters from the tensor's
//                                                      group row, Guard obeys the step guard's verdict
//   dpn_gradnorm_reduce_guard_kernel                   the reduction plus the step guard's verdict (skip non-finite and spiking steps)
//   dpn_ema_swap_kernel                                exchanges the parameters with their EMA shadow
//   dpn_lbfgs.inc (included at the end)                L-BFGS on the same flat layout: save / move / push, the Gram pass, the direction
// No kernel in this file uses atomics: every reduction is fixed-order, the whole step is bitwise reproducible.
// Host side: adam_fill writes every table, clip_adam_flat is the two-pass launcher of every flat entry point, adam_args_ok the checks they share.
#include "dpn_device.h"
#include <initializer_list>
#include <type_traits>

// ------------------------------------------------------------------------------------------------ fused clip + Adam
// clip_grad_norm_(max_norm) followed by torch.optim.Adam(lr, betas, eps, weight_decay) (L2-in-gradient, not AdamW), as in
// interface_physics.py:514-515 / cfg:151-155, for a LIST of tensors per launch (pointer table in the kernel arguments).
constexpr int kAdamMaxTensors = 72;
constexpr int kAdamChunk = 2048;                 // elements per block
struct AdamTable {
    float* p[kAdamMaxTensors];
    const float* g[kAdamMaxTensors];
    float* m[kAdamMaxTensors];
    float* v[kAdamMaxTensors];
    int chunk_start[kAdamMaxTensors + 1];        // prefix sum of ceil(numel / kAdamChunk)
    int numel[kAdamMaxTensors];
    int n;
    static constexpr bool ema = false;
    static constexpr bool groups = false;
    static constexpr bool guard_on = false;
};
// Optimiser state kept by the caller as ONE flat buffer per moment, tensor i at offset chunk_start[i] * kAdamChunk (each tensor padded to
// whole chunks): no per-tensor state pointers, so 160 tensors fit in the kernel arguments and a PhysicsNet is one launch per pass.
// AdamFlat<Ema, Groups, Guard> is that table plus the members its options need, composed as a chain of bases in this member order:
//   head -> [Ema: s_flat, ema_base] -> [Guard: guard] -> n -> [Ema: ema_warmup] -> [Groups: group4]
// An option that is off contributes an empty base and no code (`if constexpr` on the three flags in dpn_adam_kernel): every instantiation is the
// kernel it would be with a hand-written struct of its own (tools/kernel_isa_digest.py, profiles/optim_tables_isa_digest_diff.txt).  The options'
// scalars ride in the table, so dpn_adam_kernel has one argument list.
constexpr int kAdamFlatMaxTensors = 160;
constexpr int kAdamMaxGroups = 16;
struct AdamFlatHead {
    float* p[kAdamFlatMaxTensors];
    const float* g[kAdamFlatMaxTensors];
    int chunk_start[kAdamFlatMaxTensors + 1];
    int numel[kAdamFlatMaxTensors];
    float* m_flat;
    float* v_flat;
};
// Ema: an exponential moving average of the parameters (the shadow `s_flat`, laid out like the moments), updated by the thread that has just formed
// the new parameter value
struct AdamEmaPtrs {
    float* s_flat;
    const int* ema_base;                         // device, may be null (= 0): EMA updates made before this optimiser was built
};
// Guard: the DpnStepGuard whose verdict dpn_gradnorm_reduce_guard_kernel formed one launch earlier.  A non-zero verdict returns the block before it
// touches p, m, v or the shadow; a zero one runs the arithmetic of every other table with the step number *step - skipped_nonfinite - skipped_spike
struct AdamGuardPtr { const DpnStepGuard* guard; };
struct AdamCount { int n; };
struct AdamEmaWarmup { int ema_warmup; };
// Groups: a parameter group per tensor (fine-tuning: a learning rate, betas, eps and weight decay per group).  Sixteen groups are four bits, so the
// ids ride as NIBBLES, two tensors per byte (80 bytes, not 160), and `numel` keeps its 31 bits: no tensor size is refused that the other forms take.
// The guard's tables are always grouped: one group rides as group 0 of a one-row hyper_dev (the grouped kernel with one group IS the one-group
// kernel, bit for bit)
struct AdamGroup4 { uint8_t group4[kAdamFlatMaxTensors / 2]; };     // tensor i: (group4[i >> 1] >> 4 (i & 1)) & 15
template <int I> struct AdamNone {};             // distinct empty bases, so that each takes no room
template <bool On, class T, int I> using AdamOpt = std::conditional_t<On, T, AdamNone<I>>;
template <bool Ema, bool Groups, bool Guard>
struct AdamFlat : AdamFlatHead, AdamOpt<Ema, AdamEmaPtrs, 0>, AdamOpt<Guard, AdamGuardPtr, 1>, AdamCount, AdamOpt<Ema, AdamEmaWarmup, 2>,
                  AdamOpt<Groups, AdamGroup4, 3> {
    static constexpr bool ema = Ema, groups = Groups, guard_on = Guard;
};
using AdamFlatPlain = AdamFlat<false, false, false>;     // also the table of every flat entry's gradient-norm pass
static_assert(sizeof(AdamFlat<true, true, true>) + 64 <= 4096, "kernel arguments are limited to 4 KB");
DEV float* table_m(const AdamTable& t, int ti) { return t.m[ti]; }
DEV float* table_v(const AdamTable& t, int ti) { return t.v[ti]; }
DEV float* table_m(const AdamFlatHead& t, int ti) { return t.m_flat + (int64_t)t.chunk_start[ti] * kAdamChunk; }
DEV float* table_v(const AdamFlatHead& t, int ti) { return t.v_flat + (int64_t)t.chunk_start[ti] * kAdamChunk; }
template <class Table>
DEV float* table_s(const Table& t, int ti) { return t.s_flat + (int64_t)t.chunk_start[ti] * kAdamChunk; }
template <class Table>
DEV int table_group(const Table& t, int ti) { return (t.group4[ti >> 1] >> ((ti & 1) * 4)) & 15; }
template <class Table>
DEV int adam_find(const Table& t, int blk) {
    int lo = 0, hi = t.n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.chunk_start[mid] <= blk) lo = mid; else hi = mid - 1; }
    return lo;
}
// One double per thread of a 256-thread block, added in a fixed order: wave by wave through the lanes, then the four waves' sums in LDS.  For the two
// reduce kernels; dpn_gradnorm_kernel keeps the same lines at its tail, where a call of this function compiles to other instructions
DEV double block_sum256(double d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
template <class Table>
__global__ __launch_bounds__(256) void dpn_gradnorm_kernel(Table t, double* partial, int* step, int bump_step) {
    // one fp64 partial per block (no atomics: 2.7k serialised fp64 atomics on one address cost more than reading the gradients);
    // dpn_gradnorm_reduce_kernel adds them in a fixed order -> the clip coefficient is run-to-run deterministic
    if (bump_step && blockIdx.x == 0 && threadIdx.x == 0) *step += 1;       // device-side step counter: graph replays advance it
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    const float* g = t.g[ti];
    const int end = min(base + kAdamChunk, t.numel[ti]);
    float s = 0.f;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {                         // 16-byte loads over the aligned body, scalars for the tail
        const int end4 = base + ((end - base) & ~3);
        for (int i = base + 4 * threadIdx.x; i < end4; i += 1024) {
            const float4 q = *reinterpret_cast<const float4*>(g + i);
            s = fmaf(q.x, q.x, s); s = fmaf(q.y, q.y, s); s = fmaf(q.z, q.z, s); s = fmaf(q.w, q.w, s);
        }
        for (int i = end4 + threadIdx.x; i < end; i += 256) s = fmaf(g[i], g[i], s);
    } else {
        for (int i = base + threadIdx.x; i < end; i += 256) s = fmaf(g[i], g[i], s);
    }
    double d = (double)s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void dpn_gradnorm_reduce_kernel(const double* partial, int n, double* sumsq) {
    double d = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) d += partial[i];
    const double sum = block_sum256(d);
    if (threadIdx.x == 0) *sumsq = sum;
}
// dpn_gradnorm_reduce_kernel (the same sum in the same order) whose thread 0 then forms the step guard's verdict from the fp32 total norm exactly as
// dpn_adam_kernel forms it.  fp64, every operation rounded once (no contraction); the rule is restated on the host in deepphysinet_amd/guard.py.
// hyper: row 0 of hyper_dev (grad_scale = hyper[6]).  Plain vector stores by one thread, no atomics.
__global__ __launch_bounds__(256) void dpn_gradnorm_reduce_guard_kernel(const double* partial, int n, double* sumsq, const float* hyper,
                                                                        DpnStepGuard* guard, double spike_factor, double spike_decay, int spike_warmup,
                                                                        int spike_patience) {
#pragma clang fp contract(off)
    double d = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) d += partial[i];
    const double sum = block_sum256(d);
    if (threadIdx.x != 0) return;
    *sumsq = sum;
    const float total = (float)sqrt(sum) * hyper[6];
    const double tot = (double)total;
    int seen = guard->seen, consecutive = guard->consecutive;
    double running = guard->running;
    int verdict = 0;
    if (!(fabsf(total) <= 3.402823466e+38f)) {                                // NaN, +-inf (a finite sum of squares past FLT_MAX^2 cannot occur: the cast gives inf)
        verdict = 1;
        guard->skipped_nonfinite += 1;
        consecutive = 0;
    } else if (spike_factor > 0.0 && seen >= spike_warmup && tot > spike_factor * running && consecutive < spike_patience) {
        verdict = 2;
        guard->skipped_spike += 1;
        consecutive += 1;
    } else {
        if (consecutive == spike_patience) seen = 0;                          // overruled: the level of the norms has moved, the mean starts again
        if (seen == 0) running = tot;
        else {
            const double a = spike_decay * running;
            const double b = 1.0 - spike_decay;
            const double c = b * tot;
            running = a + c;
        }
        if (seen < 0x7fffffff) seen += 1;
        consecutive = 0;
        guard->running = running;
        guard->seen = seen;
    }
    guard->verdict = verdict;
    guard->consecutive = consecutive;
    guard->last = tot;
}
template <class Table>
__global__ __launch_bounds__(256) void dpn_adam_kernel(Table t, const double* sumsq, const int* step, float lr, float b1, float b2, float eps,
                                                       float wd, float max_norm, float* out_norm, const float* hyper) {
    // hyper (optional, device): [lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale] read at run time, so that a step captured in
    // a hipGraph follows a learning-rate schedule (a by-value lr is frozen into the graph); grad_scale multiplies every gradient
    // before the norm and the update (1 / world_size after a SUM all-reduce).  Table::ema: hyper[7] is the EMA decay, hyper is not null
    // Table::groups: hyper is float[n_groups][8], not null.  This block's tensor gives the group whose row holds lr, the betas, eps and the weight
    // decay -- step_size and the bias corrections below are formed from them, per block; max_norm, grad_scale and the EMA decay are row 0's (the
    // clip is global).  From there on the arithmetic is the one of every other table
    float gscale = 1.f;
    if constexpr (Table::groups) {
        const float* row = hyper + 8 * table_group(t, adam_find(t, blockIdx.x));
        lr = row[0]; b1 = row[1]; b2 = row[2]; eps = row[3]; wd = row[4]; max_norm = hyper[5]; gscale = hyper[6];
    } else if (hyper) { lr = hyper[0]; b1 = hyper[1]; b2 = hyper[2]; eps = hyper[3]; wd = hyper[4]; max_norm = hyper[5]; gscale = hyper[6]; }
    const float total = (float)sqrt(*sumsq) * gscale;
    if (out_norm && blockIdx.x == 0 && threadIdx.x == 0) *out_norm = total;
    // Table::guard_on: a refused step (verdict != 0) ends here, p, m, v and the shadow neither read nor written (out_norm above still shows the norm
    // that was refused); an applied one counts its step number without the skipped calls, in the bias corrections and in the EMA's te alike
    int tstep = *step;
    if constexpr (Table::guard_on) {
        if (t.guard->verdict != 0) return;
        tstep -= t.guard->skipped_nonfinite + t.guard->skipped_spike;
    }
    const float coef = fminf(max_norm / (total + 1e-6f), 1.0f) * gscale;    // clip_grad_norm_'s clamp(max_norm / (norm + 1e-6), max=1)
    const float st = (float)tstep;
    const float bc1 = 1.f - powf(b1, st), bc2s = sqrtf(1.f - powf(b2, st));
    const float step_size = lr / bc1;
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    float* p = t.p[ti]; const float* g = t.g[ti]; float* m = table_m(t, ti); float* v = table_v(t, ti);
    const int end = min(base + kAdamChunk, t.numel[ti]);
    // Table::ema: s' = d s + (1 - d) p' with the p' this thread stores; d = decay, or min(decay, (1 + te) / (10 + te)) during the warm-up,
    // te = the step number + *ema_base.  One rounding per operation, the one fma written here
    float* sh = nullptr;
    float ema_d = 0.f, ema_1md = 0.f;
    if constexpr (Table::ema) {
        sh = table_s(t, ti);
        const float te = (float)(tstep + (t.ema_base ? *t.ema_base : 0));
        ema_d = t.ema_warmup ? fminf(hyper[7], (1.f + te) / (10.f + te)) : hyper[7];
        ema_1md = 1.f - ema_d;
    }
    auto ema_upd = [&](const float si, const float pi) __attribute__((always_inline)) { return fmaf(ema_d, si, ema_1md * pi); };
    auto upd = [&](float& pi, const float graw, float& mi, float& vi) __attribute__((always_inline)) {
        const float gi = fmaf(wd, pi, graw * coef);
        mi = fmaf(b1, mi, (1.f - b1) * gi);                                  // lerp(m, g, 1-b1)
        vi = fmaf(b2, vi, (1.f - b2) * gi * gi);
        pi = pi - step_size * mi / (sqrtf(vi) / bc2s + eps);
    };
    int scalar_from = base;
    if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
          reinterpret_cast<uintptr_t>(sh)) & 15) == 0) {
        const int end4 = base + ((end - base) & ~3);
        for (int i = base + 4 * threadIdx.x; i < end4; i += 1024) {
            // the moments and the gradient are touched by nobody else: streamed past the caches (the parameters stay cacheable, the
            // next step reads them first)
            typedef __attribute__((ext_vector_type(4))) float f32x4_t;
            float4 P = *reinterpret_cast<float4*>(p + i);
            // (round 6 once more, rocprofv3 in the step: the gradient loaded without the hint 27.2, all three loads without 27.6, stores too 28.3 against 25.2 us)
            const f32x4_t Mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(m + i));
            const f32x4_t Vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(v + i));
            const f32x4_t Gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(g + i));
            float4 M = make_float4(Mv[0], Mv[1], Mv[2], Mv[3]), V = make_float4(Vv[0], Vv[1], Vv[2], Vv[3]);
            const float4 G = make_float4(Gv[0], Gv[1], Gv[2], Gv[3]);
            f32x4_t Sv;
            if constexpr (Table::ema) Sv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(sh + i));     // the shadow: nobody else's either
            upd(P.x, G.x, M.x, V.x); upd(P.y, G.y, M.y, V.y); upd(P.z, G.z, M.z, V.z); upd(P.w, G.w, M.w, V.w);
            *reinterpret_cast<float4*>(p + i) = P;
            __builtin_nontemporal_store(f32x4_t{M.x, M.y, M.z, M.w}, reinterpret_cast<f32x4_t*>(m + i));
            __builtin_nontemporal_store(f32x4_t{V.x, V.y, V.z, V.w}, reinterpret_cast<f32x4_t*>(v + i));
            if constexpr (Table::ema)
                __builtin_nontemporal_store(f32x4_t{ema_upd(Sv[0], P.x), ema_upd(Sv[1], P.y), ema_upd(Sv[2], P.z), ema_upd(Sv[3], P.w)},
                                            reinterpret_cast<f32x4_t*>(sh + i));
        }
        scalar_from = end4;
    }
    for (int i = scalar_from + threadIdx.x; i < end; i += 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        upd(pi, g[i], mi, vi);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if constexpr (Table::ema) __builtin_nontemporal_store(ema_upd(__builtin_nontemporal_load(sh + i), pi), sh + i);
    }
}
// p <-> shadow, bit for bit (moved as 32-bit words: no float operation touches a NaN payload), over the chunk table of the Adam kernels
struct EmaSwapTable {
    float* p[kAdamFlatMaxTensors];
    int chunk_start[kAdamFlatMaxTensors + 1];
    int numel[kAdamFlatMaxTensors];
    float* s_flat;
    int n;
};
__global__ __launch_bounds__(256) void dpn_ema_swap_kernel(EmaSwapTable t) {
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    uint32_t* p = reinterpret_cast<uint32_t*>(t.p[ti]);
    uint32_t* sh = reinterpret_cast<uint32_t*>(t.s_flat + (int64_t)t.chunk_start[ti] * kAdamChunk);
    const int end = min(base + kAdamChunk, t.numel[ti]);
    int scalar_from = base;
    if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(sh)) & 15) == 0) {
        const int end4 = base + ((end - base) & ~3);
        for (int i = base + 4 * threadIdx.x; i < end4; i += 1024) {
            const uint4 a = *reinterpret_cast<const uint4*>(p + i), b = *reinterpret_cast<const uint4*>(sh + i);
            *reinterpret_cast<uint4*>(p + i) = b;
            *reinterpret_cast<uint4*>(sh + i) = a;
        }
        scalar_from = end4;
    }
    for (int i = scalar_from + threadIdx.x; i < end; i += 256) { const uint32_t a = p[i]; p[i] = sh[i]; sh[i] = a; }
}

// ------------------------------------------------------------------------------------------------ host side
// The checks every entry shares, all made before the first launch: a refusal bumps no step counter and writes no partial, whichever table the bad
// tensor is in.  `required`: the entry's pointers that must not be NULL.  group_of (optional): every id below n_groups, at most kAdamMaxGroups of them
static bool adam_args_ok(int n_tensors, const int64_t* numel, std::initializer_list<const void*> required, const uint8_t* group_of = nullptr,
                         int n_groups = 0) {
    if (n_tensors <= 0 || !numel) return false;
    for (const void* q : required) if (!q) return false;
    if (group_of && (n_groups < 1 || n_groups > kAdamMaxGroups)) return false;
    for (int i = 0; i < n_tensors; ++i) if (numel[i] <= 0 || numel[i] > 0x7fffffff || (group_of && group_of[i] >= n_groups)) return false;
    return true;
}

static int64_t adam_chunks(int n_tensors, const int64_t* numel) {
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) chunks += (numel[i] + kAdamChunk - 1) / kAdamChunk;
    return chunks;
}

// Table `t` for the caller's tensors [t0, t0 + t.n), as many as the table holds: n, p, numel and the chunk prefix sum; returns the table's chunk
// count.  rest(i, t0 + i) fills what else the table type has per tensor (g, m, v, the group nibble)
template <class Table, class Rest>
static int adam_fill(Table& t, int t0, int n_tensors, float* const* params, const int64_t* numel, Rest rest) {
    constexpr int cap = (int)(sizeof(t.p) / sizeof(t.p[0]));
    t.n = (n_tensors - t0 < cap) ? n_tensors - t0 : cap;
    int chunks = 0;
    for (int i = 0; i < t.n; ++i) {
        t.p[i] = params[t0 + i];
        t.numel[i] = (int)numel[t0 + i];
        t.chunk_start[i] = chunks;
        chunks += (t.numel[i] + kAdamChunk - 1) / kAdamChunk;
        rest(i, t0 + i);
    }
    t.chunk_start[t.n] = chunks;
    return chunks;
}

// The arguments of the flat entry points by name; what an entry does not take keeps its default
struct AdamFlatCall {
    int n_tensors; float* const* params; const float* const* grads; const int64_t* numel;
    float *m_flat, *v_flat;
    double* scratch;                             // [0]: sum of squares of all gradients; [1 ..]: one partial per 2048-element chunk
    int* step; float* out_norm; void* stream;
    const float* hyper = nullptr;
    float lr = 0.f, beta1 = 0.f, beta2 = 0.f, eps = 0.f, weight_decay = 0.f, max_norm = 0.f;     // by value: dpn_clip_adam_flat alone
    const uint8_t* group_of = nullptr;           // NULL in a grouped table: every tensor in group 0
    float* ema_flat = nullptr; const int* ema_base = nullptr; int ema_warmup = 0;
    DpnStepGuard* guard = nullptr; double spike_factor = 0.0, spike_decay = 0.0; int spike_warmup = 0, spike_patience = 0;
};

// One table of a flat call: the tensors from t0 on, their moments (and shadow) from chunk base_chunk of the flat buffers on
template <class Table>
static int adam_flat_table(Table& t, const AdamFlatCall& c, int t0, int base_chunk) {
    const int64_t off = (int64_t)base_chunk * kAdamChunk;
    t.m_flat = c.m_flat + off; t.v_flat = c.v_flat + off;
    if constexpr (Table::ema) { t.s_flat = c.ema_flat + off; t.ema_base = c.ema_base; t.ema_warmup = c.ema_warmup; }
    if constexpr (Table::guard_on) t.guard = c.guard;                                  // every update launch obeys the one verdict
    if constexpr (Table::groups) for (int i = 0; i < kAdamFlatMaxTensors / 2; ++i) t.group4[i] = 0;
    return adam_fill(t, t0, c.n_tensors, c.params, c.numel, [&](int i, int k) {
        t.g[i] = c.grads[k];
        if constexpr (Table::groups) if (c.group_of) t.group4[i >> 1] |= (uint8_t)(c.group_of[k] << ((i & 1) * 4));
    });
}

// Every flat entry point: the norm launches (the norm is global, over every group, and bumps *step whatever the guard's verdict: one instantiation,
// the plain table's, for all of them), the reduce (with the guard's verdict for a guarded table), then the update launches of `Table`
template <class Table>
static int clip_adam_flat(const AdamFlatCall& c) {
    static_assert(std::is_trivially_copyable<Table>::value && std::is_trivially_copyable<AdamFlatPlain>::value, "the tables are passed by value");
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    double* sumsq = c.scratch;
    double* partial = c.scratch + 1;
    int base_chunk = 0;
    for (int t0 = 0; t0 < c.n_tensors; t0 += kAdamFlatMaxTensors) {
        AdamFlatPlain t;
        const int chunks = adam_flat_table(t, c, t0, base_chunk);
        hipLaunchKernelGGL(dpn_gradnorm_kernel<AdamFlatPlain>, dim3(chunks), dim3(256), 0, s, t, partial + base_chunk, c.step, t0 == 0 ? 1 : 0);
        base_chunk += chunks;
    }
    if constexpr (Table::guard_on)
        hipLaunchKernelGGL(dpn_gradnorm_reduce_guard_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, base_chunk, sumsq, c.hyper, c.guard,
                           c.spike_factor, c.spike_decay, c.spike_warmup, c.spike_patience);
    else hipLaunchKernelGGL(dpn_gradnorm_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, base_chunk, sumsq);
    base_chunk = 0;
    for (int t0 = 0; t0 < c.n_tensors; t0 += kAdamFlatMaxTensors) {
        Table t;
        const int chunks = adam_flat_table(t, c, t0, base_chunk);
        hipLaunchKernelGGL(dpn_adam_kernel<Table>, dim3(chunks), dim3(256), 0, s, t, (const double*)sumsq, (const int*)c.step, c.lr, c.beta1, c.beta2,
                           c.eps, c.weight_decay, c.max_norm, c.out_norm, c.hyper);
        base_chunk += chunks;
    }
    return ck(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int64_t dpn_clip_adam_scratch_doubles(int n_tensors, const int64_t* numel) {
    return (n_tensors <= 0 || !numel) ? -1 : 1 + adam_chunks(n_tensors, numel);
}

int64_t dpn_clip_adam_flat_floats(int n_tensors, const int64_t* numel) {
    return (n_tensors <= 0 || !numel) ? -1 : adam_chunks(n_tensors, numel) * kAdamChunk;
}

int dpn_clip_adam(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const int64_t* numel, double* scratch_dev, int* step_dev, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float max_norm, float* out_norm_dev, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, grads, exp_avg, exp_avg_sq, scratch_dev, step_dev})) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* sumsq = scratch_dev;                 // [0]: sum of squares of all gradients; [1 ..]: one partial per 2048-element chunk
    double* partial = scratch_dev + 1;
    for (int pass = 0; pass < 2; ++pass) {
        int base_chunk = 0;
        for (int t0 = 0; t0 < n_tensors; t0 += kAdamMaxTensors) {
            AdamTable t;
            const int chunks = adam_fill(t, t0, n_tensors, params, numel,
                                         [&](int i, int k) { t.g[i] = grads[k]; t.m[i] = exp_avg[k]; t.v[i] = exp_avg_sq[k]; });
            if (pass == 0) hipLaunchKernelGGL(dpn_gradnorm_kernel<AdamTable>, dim3(chunks), dim3(256), 0, s, t, partial + base_chunk, step_dev, t0 == 0 ? 1 : 0);
            else hipLaunchKernelGGL(dpn_adam_kernel<AdamTable>, dim3(chunks), dim3(256), 0, s, t, (const double*)sumsq, (const int*)step_dev, lr, beta1,
                                    beta2, eps, weight_decay, max_norm, out_norm_dev, (const float*)nullptr);
            base_chunk += chunks;
        }
        if (pass == 0) hipLaunchKernelGGL(dpn_gradnorm_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, base_chunk, sumsq);
    }
    return ck(hipGetLastError());
}

int dpn_clip_adam_flat(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                       float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float max_norm, float* out_norm_dev, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, grads, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev})) return -1;
    AdamFlatCall c{n_tensors, params, grads, numel, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, out_norm_dev, stream};
    c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.weight_decay = weight_decay; c.max_norm = max_norm;
    return clip_adam_flat<AdamFlatPlain>(c);
}

int dpn_clip_adam_flat_dev(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                           float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const float* hyper_dev, float* out_norm_dev,
                           void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, grads, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, hyper_dev})) return -1;
    AdamFlatCall c{n_tensors, params, grads, numel, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, out_norm_dev, stream, hyper_dev};
    return clip_adam_flat<AdamFlatPlain>(c);
}

int dpn_clip_adam_flat_ema(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                           float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const float* hyper_dev, float* out_norm_dev,
                           float* ema_flat, const int* ema_base_dev, int ema_warmup, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, grads, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, hyper_dev, ema_flat})) return -1;
    AdamFlatCall c{n_tensors, params, grads, numel, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, out_norm_dev, stream, hyper_dev};
    c.ema_flat = ema_flat; c.ema_base = ema_base_dev; c.ema_warmup = ema_warmup;
    return clip_adam_flat<AdamFlat<true, false, false>>(c);
}

int dpn_clip_adam_flat_groups(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                              float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const uint8_t* group_of, int n_groups,
                              const float* hyper_dev, float* out_norm_dev, float* ema_flat, const int* ema_base_dev, int ema_warmup, void* stream) {
    if (!group_of || !adam_args_ok(n_tensors, numel, {params, grads, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, hyper_dev}, group_of, n_groups))
        return -1;
    AdamFlatCall c{n_tensors, params, grads, numel, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, out_norm_dev, stream, hyper_dev};
    c.group_of = group_of;
    if (!ema_flat) return clip_adam_flat<AdamFlat<false, true, false>>(c);
    c.ema_flat = ema_flat; c.ema_base = ema_base_dev; c.ema_warmup = ema_warmup;
    return clip_adam_flat<AdamFlat<true, true, false>>(c);
}

int dpn_clip_adam_flat_guard(int n_tensors, float* const* params, const float* const* grads, const int64_t* numel, float* exp_avg_flat,
                             float* exp_avg_sq_flat, double* scratch_dev, int* step_dev, const uint8_t* group_of, int n_groups,
                             const float* hyper_dev, float* out_norm_dev, float* ema_flat, const int* ema_base_dev, int ema_warmup,
                             DpnStepGuard* guard_dev, double spike_factor, double spike_decay, int spike_warmup, int spike_patience, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, grads, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, hyper_dev, guard_dev}, group_of, n_groups))
        return -1;
    if (!(spike_factor >= 0.0 && spike_factor <= 1.7976931348623157e308) || !(spike_decay >= 0.0 && spike_decay < 1.0) || spike_warmup < 1 ||
        spike_patience < 1) return -1;
    AdamFlatCall c{n_tensors, params, grads, numel, exp_avg_flat, exp_avg_sq_flat, scratch_dev, step_dev, out_norm_dev, stream, hyper_dev};
    c.group_of = group_of;                                                             // NULL: one group, n_groups is not read
    c.guard = guard_dev; c.spike_factor = spike_factor; c.spike_decay = spike_decay; c.spike_warmup = spike_warmup; c.spike_patience = spike_patience;
    if (!ema_flat) return clip_adam_flat<AdamFlat<false, true, true>>(c);
    c.ema_flat = ema_flat; c.ema_base = ema_base_dev; c.ema_warmup = ema_warmup;
    return clip_adam_flat<AdamFlat<true, true, true>>(c);
}

int dpn_ema_swap(int n_tensors, float* const* params, const int64_t* numel, float* ema_flat, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, ema_flat})) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int base_chunk = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += kAdamFlatMaxTensors) {
        EmaSwapTable t;
        t.s_flat = ema_flat + (int64_t)base_chunk * kAdamChunk;
        const int chunks = adam_fill(t, t0, n_tensors, params, numel, [](int, int) {});
        hipLaunchKernelGGL(dpn_ema_swap_kernel, dim3(chunks), dim3(256), 0, s, t);
        base_chunk += chunks;
    }
    return ck(hipGetLastError());
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ L-BFGS on the flat buffers
#include "dpn_lbfgs.inc"
