// MI355X (gfx950 / CDNA4): L-BFGS on the optimiser's flat buffers, restated so that an iteration reads the history twice ("vector-free" L-BFGS).
// Included at the end of dpn_optim.hip: it shares adam_fill / adam_find, the chunk layout (every tensor padded to whole kAdamChunk-element chunks)
// and the fixed-order fp64 reductions of the clip + Adam kernels.
//
// Kernel inventory
//   dpn_lbfgs_save_kernel / dpn_lbfgs_move_kernel       parameters -> x0_flat;  p = fl(x0 + fl(t d)) through the pointer table (t == 0: x0's words)
//   dpn_lbfgs_push_kernel / dpn_lbfgs_commit_kernel     s = fl(t d), y = fl(g - g_prev) into the next ring slot, g_prev = g;  then the ring pointer
//   dpn_lbfgs_gram_kernel / dpn_lbfgs_gram_reduce_kernel  the inner products of {newest s, newest y, g} with every stored s, y and g, sum |g|, max |g|:
//                                                       one fp64 partial per chunk and quantity, added in index order into the Gram matrix
//   dpn_lbfgs_gtd_kernel / dpn_lbfgs_gtd_reduce_kernel  one inner product of two flat vectors in the same order (the line search's g.d)
//   dpn_lbfgs_coef_kernel                               one thread, fp64: accepts or refuses the newest pair, two-loop recursion on the Gram matrix
//   dpn_lbfgs_direction_kernel                          d = sum_j delta_j b_j per element, fp64, rounded once to fp32
// No atomics; every reduction in a fixed order; no contraction (the arithmetic is restated operation for operation in deepphysinet_amd/lbfgs.py).
// Basis of the Gram matrix G[(2m+1)^2] and of delta[2m+1], by RING SLOT: s slot j = j, y slot j = m + j, g = 2m.

constexpr int kLbfgsMaxM = 32;
constexpr int kLbfgsMaxQ = 3 * (2 * kLbfgsMaxM + 1) + 2;       // three new vectors against the basis, then sum |g| and max |g|
struct LbfgsTable {
    float* p[kAdamFlatMaxTensors];
    int chunk_start[kAdamFlatMaxTensors + 1];
    int numel[kAdamFlatMaxTensors];
    int n;
};
static_assert(sizeof(LbfgsTable) + 128 <= 4096, "kernel arguments are limited to 4 KB");

// The ring as the state describes it, kept inside the buffers whatever the struct holds
DEV void lbfgs_ring(const DpnLbfgsState* st, int m, int& count, int& nw) {
    count = st->count; nw = st->newest;
    if (count < 0) count = 0;
    if (count > m) count = m;
    if (nw < 0 || nw >= m) nw = 0;
}
DEV bool lbfgs_slot_valid(int slot, int nw, int count, int m) { return (nw - slot + m) % m < count; }
// basis index b (by slot) holds a stored vector
DEV bool lbfgs_basis_valid(int b, int nw, int count, int m) { return b == 2 * m || lbfgs_slot_valid(b < m ? b : b - m, nw, count, m); }
// slot of the pair of age rank i, i = 0 the oldest, count - 1 the newest
DEV int lbfgs_slot(int i, int nw, int count, int m) { return (nw - (count - 1 - i) + m) % m; }
// NaN-propagating maximum (a NaN gradient must not hide behind a finite max |g|)
DEV double lbfgs_max(double a, double b) { return (b > a || b != b) ? b : a; }
DEV double wave_sum64(double d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    return d;
}
DEV double wave_max64(double d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d = lbfgs_max(d, __shfl_xor(d, o));
    return d;
}
// This block's chunk: the number of tensor elements in it (the rest of the 2048 is padding, never read or written)
DEV int lbfgs_chunk_len(const LbfgsTable& t) {
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    return min(kAdamChunk, t.numel[ti] - base);
}

__global__ __launch_bounds__(256) void dpn_lbfgs_save_kernel(LbfgsTable t, uint32_t* x0) {
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    const int len = min(kAdamChunk, t.numel[ti] - base);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(t.p[ti]) + base;
    uint32_t* x = x0 + (int64_t)blockIdx.x * kAdamChunk;
    for (int e = threadIdx.x; e < len; e += 256) x[e] = p[e];
}
__global__ __launch_bounds__(256) void dpn_lbfgs_move_kernel(LbfgsTable t, const float* x0, const float* d, float tstep) {
#pragma clang fp contract(off)
    const int ti = adam_find(t, blockIdx.x);
    const int base = (blockIdx.x - t.chunk_start[ti]) * kAdamChunk;
    const int len = min(kAdamChunk, t.numel[ti] - base);
    float* p = t.p[ti] + base;
    const int64_t off = (int64_t)blockIdx.x * kAdamChunk;
    if (tstep == 0.f) {                                                           // the restore: words, no float operation (-0 stays -0, d is not read)
        const uint32_t* x = reinterpret_cast<const uint32_t*>(x0 + off);
        uint32_t* pw = reinterpret_cast<uint32_t*>(p);
        for (int e = threadIdx.x; e < len; e += 256) pw[e] = x[e];
        return;
    }
    for (int e = threadIdx.x; e < len; e += 256) {
        const float td = tstep * d[off + e];
        p[e] = x0[off + e] + td;
    }
}
__global__ __launch_bounds__(256) void dpn_lbfgs_push_kernel(LbfgsTable t, const float* g, float* g_prev, const float* d, float* S, float* Y,
                                                             int64_t stride, int m, float tstep, const DpnLbfgsState* st) {
#pragma clang fp contract(off)
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    const int slot = (nw + 1) % m;                                                // dpn_lbfgs_commit_kernel makes it the newest, one launch later
    const int len = lbfgs_chunk_len(t);
    const int64_t off = (int64_t)blockIdx.x * kAdamChunk;
    float* s = S + slot * stride + off;
    float* y = Y + slot * stride + off;
    for (int e = threadIdx.x; e < len; e += 256) {
        const float gi = g[off + e];
        s[e] = tstep * d[off + e];
        y[e] = gi - g_prev[off + e];
        g_prev[off + e] = gi;
    }
}
__global__ void dpn_lbfgs_commit_kernel(int m, DpnLbfgsState* st) {
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    st->newest = (nw + 1) % m;
    st->count = count < m ? count + 1 : m;
    st->pending = 1;
}

// One block per chunk.  Thread t holds elements t, t + 256, ... of the chunk and adds its fp64 products in that order; the 64 lanes of a wave are
// added by the xor butterfly (32, 16, ... 1), the four waves as (w0 + w1) + (w2 + w3): block_sum256's order.  partial[q * nchunks + chunk]
__global__ __launch_bounds__(256) void dpn_lbfgs_gram_kernel(LbfgsTable t, const float* S, const float* Y, const float* g, int64_t stride, int m,
                                                             const DpnLbfgsState* st, double* partial, int chunk0, int nchunks) {
#pragma clang fp contract(off)
    __shared__ double red[kLbfgsMaxQ][4];
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    const int len = lbfgs_chunk_len(t);
    const int64_t off = (int64_t)blockIdx.x * kAdamChunk;
    const int B = 2 * m + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float sn[8], yn[8], gg[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = threadIdx.x + 256 * k;
        const bool ok = e < len;
        gg[k] = ok ? g[off + e] : 0.f;
        sn[k] = (ok && count > 0) ? S[nw * stride + off + e] : 0.f;
        yn[k] = (ok && count > 0) ? Y[nw * stride + off + e] : 0.f;
    }
    auto against = [&](const float* v, int b) __attribute__((always_inline)) {   // v: the basis vector b at this chunk, or null for g
        float vb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int e = threadIdx.x + 256 * k; vb[k] = v ? (e < len ? v[e] : 0.f) : gg[k]; }
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double w = (double)vb[k];
            a0 = a0 + (double)sn[k] * w; a1 = a1 + (double)yn[k] * w; a2 = a2 + (double)gg[k] * w;
        }
        a0 = wave_sum64(a0); a1 = wave_sum64(a1); a2 = wave_sum64(a2);
        if (lane == 0) { red[b][wave] = a0; red[B + b][wave] = a1; red[2 * B + b][wave] = a2; }
    };
    for (int a = 0; a < count; ++a) {
        const int slot = (nw - a + m) % m;
        against(S + slot * stride + off, slot);
        against(Y + slot * stride + off, m + slot);
    }
    against(nullptr, 2 * m);
    double l1 = 0.0, mx = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { const double w = fabs((double)gg[k]); l1 = l1 + w; mx = lbfgs_max(mx, w); }
    l1 = wave_sum64(l1); mx = wave_max64(mx);
    if (lane == 0) { red[3 * B][wave] = l1; red[3 * B + 1][wave] = mx; }
    __syncthreads();
    const int64_t chunk = (int64_t)chunk0 + blockIdx.x;
    for (int q = threadIdx.x; q < 3 * B + 2; q += 256) {
        if (q < 3 * B && !lbfgs_basis_valid(q % B, nw, count, m)) continue;
        const double r = (q == 3 * B + 1) ? lbfgs_max(lbfgs_max(red[q][0], red[q][1]), lbfgs_max(red[q][2], red[q][3]))
                                          : (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        partial[(int64_t)q * nchunks + chunk] = r;
    }
}
// One block per quantity q: the partials in index order (thread t takes t, t + 256, ...), block_sum256's order, then the rows and columns of G that
// the three new vectors own.  With no pair stored only the g row exists
__global__ __launch_bounds__(256) void dpn_lbfgs_gram_reduce_kernel(const double* partial, int nchunks, int m, DpnLbfgsState* st, double* G) {
    __shared__ double red[4];
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    const int B = 2 * m + 1, q = blockIdx.x;
    const int v = q / B, b = q % B;
    if (q < 3 * B && (!lbfgs_basis_valid(b, nw, count, m) || (v < 2 && count == 0))) return;
    const bool is_max = q == 3 * B + 1;
    const double* row = partial + (int64_t)q * nchunks;
    double d = 0.0;
    if (is_max) { for (int i = threadIdx.x; i < nchunks; i += 256) d = lbfgs_max(d, row[i]); d = wave_max64(d); }
    else { for (int i = threadIdx.x; i < nchunks; i += 256) d += row[i]; d = wave_sum64(d); }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (q == 3 * B) { st->g_l1 = (red[0] + red[1]) + (red[2] + red[3]); return; }
    if (is_max) { st->g_inf = lbfgs_max(lbfgs_max(red[0], red[1]), lbfgs_max(red[2], red[3])); return; }
    const double sum = (red[0] + red[1]) + (red[2] + red[3]);
    const int r = v == 0 ? nw : v == 1 ? m + nw : 2 * m;
    G[r * B + b] = sum;
    const bool b_is_new = b == 2 * m || (count > 0 && (b == nw || b == m + nw));  // that row's own block writes the mirrored entry
    if (!b_is_new) G[b * B + r] = sum;
    if (r == 2 * m && b == 2 * m) st->gg = sum;
}
__global__ __launch_bounds__(256) void dpn_lbfgs_gtd_kernel(LbfgsTable t, const float* a, const float* b, double* partial) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int len = lbfgs_chunk_len(t);
    const int64_t off = (int64_t)blockIdx.x * kAdamChunk;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = threadIdx.x + 256 * k;
        const double x = e < len ? (double)a[off + e] : 0.0, y = e < len ? (double)b[off + e] : 0.0;
        acc = acc + x * y;
    }
    acc = wave_sum64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One thread.  Basis order everywhere: s oldest -> newest, y oldest -> newest, g; every product and every sum rounded once
__global__ void dpn_lbfgs_coef_kernel(int m, DpnLbfgsState* st, const double* G, double* delta) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    __shared__ double dl[2 * kLbfgsMaxM + 1], al[kLbfgsMaxM];
    const int B = 2 * m + 1;
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    if (st->pending) {
        if (count > 0 && !(G[nw * B + m + nw] > 1e-10)) {                         // torch's rule: the pair stands when s.y > 1e-10
            st->skipped += 1;
            nw = (nw - 1 + m) % m;
            count -= 1;
        }
        st->pending = 0;
    }
    for (int b = 0; b < B; ++b) dl[b] = 0.0;
    dl[2 * m] = -1.0;
    auto dotcol = [&](int c) {
        double a = 0.0;
        for (int i = 0; i < count; ++i) { const int sl = lbfgs_slot(i, nw, count, m); a = a + dl[sl] * G[sl * B + c]; }
        for (int i = 0; i < count; ++i) { const int sl = m + lbfgs_slot(i, nw, count, m); a = a + dl[sl] * G[sl * B + c]; }
        a = a + dl[2 * m] * G[2 * m * B + c];
        return a;
    };
    for (int i = count - 1; i >= 0; --i) {
        const int sl = lbfgs_slot(i, nw, count, m);
        al[i] = dotcol(sl) / G[sl * B + m + sl];
        dl[m + sl] = dl[m + sl] - al[i];
    }
    double gamma = 1.0;
    if (count > 0) {
        gamma = G[nw * B + m + nw] / G[(m + nw) * B + m + nw];
        for (int b = 0; b < B; ++b) dl[b] = dl[b] * gamma;
    }
    for (int i = 0; i < count; ++i) {
        const int sl = lbfgs_slot(i, nw, count, m);
        const double beta = dotcol(m + sl) / G[sl * B + m + sl];
        const double up = al[i] - beta;
        dl[sl] = dl[sl] + up;
    }
    const double gtd = dotcol(2 * m);
    double dd = 0.0;
    for (int i = 0; i < count; ++i) { const int sl = lbfgs_slot(i, nw, count, m); dd = dd + dl[sl] * dotcol(sl); }
    for (int i = 0; i < count; ++i) { const int sl = m + lbfgs_slot(i, nw, count, m); dd = dd + dl[sl] * dotcol(sl); }
    dd = dd + dl[2 * m] * gtd;
    for (int b = 0; b < B; ++b) delta[b] = dl[b];
    st->count = count; st->newest = nw; st->iters += 1;
    st->gamma = gamma; st->gtd = gtd; st->dnorm = dd > 0.0 ? sqrt(dd) : 0.0;
}
__global__ __launch_bounds__(256) void dpn_lbfgs_direction_kernel(LbfgsTable t, const float* S, const float* Y, const float* g, int64_t stride, int m,
                                                                  const DpnLbfgsState* st, const double* delta, float* d) {
#pragma clang fp contract(off)
    int count, nw;
    lbfgs_ring(st, m, count, nw);
    const int len = lbfgs_chunk_len(t);
    const int64_t off = (int64_t)blockIdx.x * kAdamChunk;
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        const float* V = pass == 0 ? S : Y;
        for (int i = 0; i < count; ++i) {
            const int sl = lbfgs_slot(i, nw, count, m);
            const double c = delta[pass * m + sl];
            const float* v = V + sl * stride + off;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const int e = threadIdx.x + 256 * k; if (e < len) acc[k] = acc[k] + c * (double)v[e]; }
        }
    }
    const double cg = delta[2 * m];
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int e = threadIdx.x + 256 * k; if (e < len) d[off + e] = (float)(acc[k] + cg * (double)g[off + e]); }
}

// ------------------------------------------------------------------------------------------------ host side
// fn(table, base_chunk, chunks) for every table of the call (160 tensors each); returns the chunk count of the whole call
template <class Fn>
static int lbfgs_tables(int n_tensors, float* const* params, const int64_t* numel, Fn fn) {
    int base_chunk = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += kAdamFlatMaxTensors) {
        LbfgsTable t;
        const int chunks = adam_fill(t, t0, n_tensors, params, numel, [](int, int) {});
        fn(t, base_chunk, chunks);
        base_chunk += chunks;
    }
    return base_chunk;
}
static bool lbfgs_m_ok(int m) { return m >= 1 && m <= kLbfgsMaxM; }
static bool lbfgs_t_ok(float t) { return t == t && t - t == 0.f; }                // finite

extern "C" {

int64_t dpn_lbfgs_scratch_doubles(int n_tensors, const int64_t* numel, int m) {
    if (n_tensors <= 0 || !numel || !lbfgs_m_ok(m)) return -1;
    return (int64_t)(3 * (2 * m + 1) + 2) * adam_chunks(n_tensors, numel);
}

int dpn_lbfgs_save(int n_tensors, float* const* params, const int64_t* numel, float* x0_flat, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, x0_flat})) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        hipLaunchKernelGGL(dpn_lbfgs_save_kernel, dim3(chunks), dim3(256), 0, s, t, reinterpret_cast<uint32_t*>(x0_flat) + (int64_t)base * kAdamChunk);
    });
    return ck(hipGetLastError());
}

int dpn_lbfgs_move(int n_tensors, float* const* params, const int64_t* numel, const float* x0_flat, const float* d_flat, float t_step, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, x0_flat, d_flat}) || !lbfgs_t_ok(t_step)) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        const int64_t off = (int64_t)base * kAdamChunk;
        hipLaunchKernelGGL(dpn_lbfgs_move_kernel, dim3(chunks), dim3(256), 0, s, t, x0_flat + off, d_flat + off, t_step);
    });
    return ck(hipGetLastError());
}

int dpn_lbfgs_push(int n_tensors, float* const* params, const int64_t* numel, const float* g_flat, float* g_prev_flat, const float* d_flat,
                   float t_step, float* S, float* Y, int m, DpnLbfgsState* state, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, g_flat, g_prev_flat, d_flat, S, Y, state}) || !lbfgs_m_ok(m) || !lbfgs_t_ok(t_step)) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t stride = adam_chunks(n_tensors, numel) * kAdamChunk;
    lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        const int64_t off = (int64_t)base * kAdamChunk;
        hipLaunchKernelGGL(dpn_lbfgs_push_kernel, dim3(chunks), dim3(256), 0, s, t, g_flat + off, g_prev_flat + off, d_flat + off, S + off, Y + off,
                           stride, m, t_step, (const DpnLbfgsState*)state);
    });
    hipLaunchKernelGGL(dpn_lbfgs_commit_kernel, dim3(1), dim3(1), 0, s, m, state);
    return ck(hipGetLastError());
}

int dpn_lbfgs_gram(int n_tensors, float* const* params, const int64_t* numel, const float* S, const float* Y, const float* g_flat, int m,
                   DpnLbfgsState* state, double* scratch, double* G, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, S, Y, g_flat, state, scratch, G}) || !lbfgs_m_ok(m)) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nchunks = (int)adam_chunks(n_tensors, numel);
    const int64_t stride = (int64_t)nchunks * kAdamChunk;
    lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        const int64_t off = (int64_t)base * kAdamChunk;
        hipLaunchKernelGGL(dpn_lbfgs_gram_kernel, dim3(chunks), dim3(256), 0, s, t, S + off, Y + off, g_flat + off, stride, m,
                           (const DpnLbfgsState*)state, scratch, base, nchunks);
    });
    hipLaunchKernelGGL(dpn_lbfgs_gram_reduce_kernel, dim3(3 * (2 * m + 1) + 2), dim3(256), 0, s, (const double*)scratch, nchunks, m, state, G);
    return ck(hipGetLastError());
}

int dpn_lbfgs_gtd(int n_tensors, float* const* params, const int64_t* numel, const float* a_flat, const float* b_flat, double* scratch,
                  double* out_dev, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, a_flat, b_flat, scratch, out_dev})) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nchunks = lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        const int64_t off = (int64_t)base * kAdamChunk;
        hipLaunchKernelGGL(dpn_lbfgs_gtd_kernel, dim3(chunks), dim3(256), 0, s, t, a_flat + off, b_flat + off, scratch + base);
    });
    hipLaunchKernelGGL(dpn_gradnorm_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)scratch, nchunks, out_dev);
    return ck(hipGetLastError());
}

int dpn_lbfgs_direction(int n_tensors, float* const* params, const int64_t* numel, const float* S, const float* Y, const float* g_flat, int m,
                        DpnLbfgsState* state, const double* G, double* delta, float* d_flat, void* stream) {
    if (!adam_args_ok(n_tensors, numel, {params, S, Y, g_flat, state, G, delta, d_flat}) || !lbfgs_m_ok(m)) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t stride = adam_chunks(n_tensors, numel) * kAdamChunk;
    hipLaunchKernelGGL(dpn_lbfgs_coef_kernel, dim3(1), dim3(1), 0, s, m, state, G, delta);
    lbfgs_tables(n_tensors, params, numel, [&](const LbfgsTable& t, int base, int chunks) {
        const int64_t off = (int64_t)base * kAdamChunk;
        hipLaunchKernelGGL(dpn_lbfgs_direction_kernel, dim3(chunks), dim3(256), 0, s, t, S + off, Y + off, g_flat + off, stride, m,
                           (const DpnLbfgsState*)state, (const double*)delta, d_flat + off);
    });
    return ck(hipGetLastError());
}

}  // extern "C"
