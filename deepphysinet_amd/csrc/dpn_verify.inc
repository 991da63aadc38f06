// Forecast verification against observations (DESIGN.md section 6b.6), included by dpn_diag.hip behind the regional statistics: the case axis of the
// value products.  include/dpn_hip.h states the state's layout and every operation's order.
//   dpn_verify_accumulate : ONE case's forecast (out_n) and baseline (coord_data) values at points first .. first + n against obs, folded into a resident
//                           state (count, Welford co-moments, error sums of both, contingency counts), one thread per point.
//   dpn_verify_pool       : the states of N points -> the states of G groups, one 64-lane wave per (group, column): 64 strided left folds with
//                           Chan's merge, then lane 0 folds the lane results in lane order.
//   dpn_verify_finish     : a state -> the scores, as rows.
// All three are compiled without contraction: every fp32 and fp64 operation is rounded on its own, so the numpy restatement
// (deepphysinet_amd/verification.py) reproduces them bit for bit.  No atomics, no LDS, plain per-lane stores; the pool exchanges lane results by
// wave shuffles.

namespace {

struct VerArgs {
    const float *out_n, *coord_data, *obs;
    int64_t n, first, n_total;
    DpnPhysics ph;
    int32_t n_products, n_thr;
    int32_t id[DPN_VERIFY_MAX_COLUMNS];
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
    float thr_val[DPN_VERIFY_MAX_THRESHOLDS];
    int32_t thr_side[DPN_VERIFY_MAX_THRESHOLDS];
    DpnVerifyState st;
};

// The eight value products of one side (out_n or coord_data) at point ic: the residual body with J = 0 and f = 0 read from no memory, then the
// expressions and the NaN rule of dpn_ensemble_accumulate.
struct VerValues { float u, v, p, T, q, rho, speed, rh; };

__device__ __forceinline__ VerValues verify_values(const float* src, const DpnPhysics& ph, const int64_t ic) {
#pragma clang fp contract(off)
    const EnsBody<false, false> a{src, EnsSrc<false>(nullptr), EnsSrc<false>(nullptr), ph};
#include "dpn_residual_body.inc"
    bool poisoned = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) { const float o_n = a.out_n[ic * 6 + k]; poisoned |= o_n != o_n; }
    const float nan = __builtin_nanf("");
    if (poisoned) return VerValues{nan, nan, nan, nan, nan, nan, nan, nan};
    return VerValues{u, v, p, T, q, rho, sqrtf(u * u + v * v), q / q_s};
}

__device__ __forceinline__ float verify_pick(const VerValues& s, const int id) {
    switch (id) {
        case 25: return s.speed;
        case 26: return s.rh;
        case 28: return s.u;
        case 29: return s.v;
        case 30: return s.p;
        case 31: return s.T;
        case 32: return s.q;
        default: return s.rho;                                // 33 (the entry point admits 25, 26, 28..33 only)
    }
}

__device__ __forceinline__ bool verify_event(const float z, const float thr, const int side) { return side == DPN_VERIFY_ABOVE ? z > thr : z < thr; }

__global__ __launch_bounds__(THREADS) void dpn_verify_accumulate_kernel(VerArgs e) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= e.n) return;
    const VerValues fc = verify_values(e.out_n, e.ph, ic), bs = verify_values(e.coord_data, e.ph, ic);
    const int64_t g = e.first + ic;
    const DpnVerifyState& t = e.st;
    for (int j = 0; j < e.n_products; ++j) {                  // the selector is uniform: a scalar branch per column
        const float x = verify_pick(fc, e.id[j]), b = verify_pick(bs, e.id[j]), o = e.obs[ic * e.n_products + j];
        if (!__builtin_isfinite(x) || !__builtin_isfinite(b) || !__builtin_isfinite(o)) continue;
        const int64_t s = (int64_t)j * e.n_total + g;
        const int32_t c = t.n[s] + 1;
        const double X = (double)x, O = (double)o, B = (double)b;
        double mean_f = t.mean_f[s], mean_o = t.mean_o[s];
        const double df = X - mean_f;
        mean_f = mean_f + df / (double)c;
        const double dq = O - mean_o;
        mean_o = mean_o + dq / (double)c;
        t.m2_f[s] = t.m2_f[s] + df * (X - mean_f);
        t.m2_o[s] = t.m2_o[s] + dq * (O - mean_o);
        t.c_fo[s] = t.c_fo[s] + df * (O - mean_o);
        t.mean_f[s] = mean_f;
        t.mean_o[s] = mean_o;
        const double d = X - O;
        t.sum_d[s] = t.sum_d[s] + d;
        t.sum_ad[s] = t.sum_ad[s] + fabs(d);
        t.sum_d2[s] = t.sum_d2[s] + d * d;
        const float ad = (float)fabs(d);
        if (ad > t.max_ad[s]) t.max_ad[s] = ad;
        const double er = B - O;
        t.sum_e[s] = t.sum_e[s] + er;
        t.sum_ae[s] = t.sum_ae[s] + fabs(er);
        t.sum_e2[s] = t.sum_e2[s] + er * er;
        t.n[s] = c;
        for (int i = 0; i < e.n_thr; ++i) {
            if (e.thr_col[i] != j) continue;
            const bool ex = verify_event(x, e.thr_val[i], e.thr_side[i]), eb = verify_event(b, e.thr_val[i], e.thr_side[i]),
                       eo = verify_event(o, e.thr_val[i], e.thr_side[i]);
            int32_t* cont = t.cont + (int64_t)i * 6 * e.n_total + g;
            if (ex && eo) cont[0] += 1;
            if (ex && !eo) cont[e.n_total] += 1;
            if (!ex && eo) cont[2 * e.n_total] += 1;
            if (eb && eo) cont[3 * e.n_total] += 1;
            if (eb && !eo) cont[4 * e.n_total] += 1;
            if (!eb && eo) cont[5 * e.n_total] += 1;
        }
    }
}

// One (point or group, column) entry of a state in registers.
struct VerCell {
    int32_t n;
    double mean_f, mean_o, m2_f, m2_o, c_fo, sum_d, sum_ad, sum_d2, sum_e, sum_ae, sum_e2;
    float max_ad;
};

__device__ __forceinline__ VerCell verify_load(const DpnVerifyState& t, const int64_t s) {
    return VerCell{t.n[s], t.mean_f[s], t.mean_o[s], t.m2_f[s], t.m2_o[s], t.c_fo[s], t.sum_d[s], t.sum_ad[s], t.sum_d2[s], t.sum_e[s], t.sum_ae[s],
                   t.sum_e2[s], t.max_ad[s]};
}

// An earlier state A and a later state B -> A (include/dpn_hip.h: the order of Chan's merge).
__device__ __forceinline__ void verify_merge(VerCell& A, const VerCell& B) {
#pragma clang fp contract(off)
    if (B.n == 0) return;
    if (A.n == 0) { A = B; return; }
    const int32_t n = A.n + B.n;
    const double w = ((double)A.n * (double)B.n) / (double)n, r = (double)B.n / (double)n;
    const double gf = B.mean_f - A.mean_f, go = B.mean_o - A.mean_o;
    A.m2_f = (A.m2_f + B.m2_f) + (gf * gf) * w;
    A.m2_o = (A.m2_o + B.m2_o) + (go * go) * w;
    A.c_fo = (A.c_fo + B.c_fo) + (gf * go) * w;
    A.mean_f = A.mean_f + gf * r;
    A.mean_o = A.mean_o + go * r;
    A.sum_d = A.sum_d + B.sum_d;
    A.sum_ad = A.sum_ad + B.sum_ad;
    A.sum_d2 = A.sum_d2 + B.sum_d2;
    A.sum_e = A.sum_e + B.sum_e;
    A.sum_ae = A.sum_ae + B.sum_ae;
    A.sum_e2 = A.sum_e2 + B.sum_e2;
    if (B.max_ad > A.max_ad) A.max_ad = B.max_ad;
    A.n = n;
}

__device__ __forceinline__ VerCell verify_from_lane(const VerCell& c, const int lane) {
    return VerCell{__shfl(c.n, lane, 64), __shfl(c.mean_f, lane, 64), __shfl(c.mean_o, lane, 64), __shfl(c.m2_f, lane, 64), __shfl(c.m2_o, lane, 64),
                   __shfl(c.c_fo, lane, 64), __shfl(c.sum_d, lane, 64), __shfl(c.sum_ad, lane, 64), __shfl(c.sum_d2, lane, 64), __shfl(c.sum_e, lane, 64),
                   __shfl(c.sum_ae, lane, 64), __shfl(c.sum_e2, lane, 64), __shfl(c.max_ad, lane, 64)};
}

struct VerPoolArgs {
    DpnVerifyState src, dst;
    const int32_t* order;
    const int64_t* seg_start;
    int64_t n_points, n_groups;
    int32_t n_products, n_thr;
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
};

// One 64-thread block = one wave = one (group, column).
__global__ __launch_bounds__(64) void dpn_verify_pool_kernel(VerPoolArgs a) {
#pragma clang fp contract(off)
    const int64_t w = blockIdx.x;
    const int64_t grp = w / a.n_products;
    const int j = (int)(w - grp * a.n_products), lane = threadIdx.x;
    const int64_t lo = a.seg_start[grp], hi = a.seg_start[grp + 1];
    VerCell acc{};                                            // empty: n == 0
    for (int64_t k = lo + lane; k < hi; k += 64) {
        const int64_t pt = a.order[k];
        if (pt < 0 || pt >= a.n_points) continue;
        verify_merge(acc, verify_load(a.src, (int64_t)j * a.n_points + pt));
    }
    VerCell all = acc;                                        // lane 0's: the fold of the 64 lane results in lane order
    for (int l = 1; l < 64; ++l) verify_merge(all, verify_from_lane(acc, l));
    if (lane == 0) {
        const int64_t s = (int64_t)j * a.n_groups + grp;
        const DpnVerifyState& t = a.dst;
        t.n[s] = all.n; t.mean_f[s] = all.mean_f; t.mean_o[s] = all.mean_o; t.m2_f[s] = all.m2_f; t.m2_o[s] = all.m2_o; t.c_fo[s] = all.c_fo;
        t.sum_d[s] = all.sum_d; t.sum_ad[s] = all.sum_ad; t.sum_d2[s] = all.sum_d2; t.sum_e[s] = all.sum_e; t.sum_ae[s] = all.sum_ae;
        t.sum_e2[s] = all.sum_e2; t.max_ad[s] = all.max_ad;
    }
    for (int i = 0; i < a.n_thr; ++i) {                       // the counts of the thresholds on this column: integer sums, any order is the same
        if (a.thr_col[i] != j) continue;
        for (int c = 0; c < 6; ++c) {
            const int32_t* src = a.src.cont + ((int64_t)i * 6 + c) * a.n_points;
            int32_t sum = 0;
            for (int64_t k = lo + lane; k < hi; k += 64) {
                const int64_t pt = a.order[k];
                if (pt >= 0 && pt < a.n_points) sum += src[pt];
            }
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
            if (lane == 0) a.dst.cont[((int64_t)i * 6 + c) * a.n_groups + grp] = sum;
        }
    }
}

struct VerFinishArgs {
    DpnVerifyState st;
    int64_t n, first, n_total;
    int32_t n_products, n_thr;
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
    DpnVerifyOut out;
};

// pod, far, csi, fbias, ets of the counts h, f, m among N pairs into place o of the five destinations
__device__ __forceinline__ void verify_table(const int32_t hi, const int32_t fi, const int32_t mi, const int32_t ni, float* pod, float* far, float* csi,
                                             float* fbias, float* ets, const int64_t o) {
#pragma clang fp contract(off)
    const float nan = __builtin_nanf("");
    const double h = (double)hi, f = (double)fi, m = (double)mi, N = (double)ni;
    const double hm = h + m, hf = h + f, hfm = (h + f) + m;
    pod[o] = hm != 0.0 ? (float)(h / hm) : nan;
    far[o] = hf != 0.0 ? (float)(f / hf) : nan;
    csi[o] = hfm != 0.0 ? (float)(h / hfm) : nan;
    fbias[o] = hm != 0.0 ? (float)(hf / hm) : nan;
    float e = nan;
    if (ni > 0) {
        const double hr = (hf * hm) / N, den = hfm - hr;
        if (den != 0.0) e = (float)((h - hr) / den);
    }
    ets[o] = e;
}

__global__ __launch_bounds__(THREADS) void dpn_verify_finish_kernel(VerFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= a.n) return;
    const int64_t g = a.first + ic;
    const float nan = __builtin_nanf("");
    const DpnVerifyState& t = a.st;
    for (int j = 0; j < a.n_products; ++j) {
        const int64_t s = (int64_t)j * a.n_total + g, o = ic * a.n_products + j;
        const int32_t c = t.n[s];
        const double N = (double)c;
        a.out.count[o] = c;
        const bool any = c > 0;
        const double m2_f = t.m2_f[s], m2_o = t.m2_o[s], sum_d2 = t.sum_d2[s], sum_e2 = t.sum_e2[s];
        a.out.bias[o] = any ? (float)(t.sum_d[s] / N) : nan;
        a.out.mae[o] = any ? (float)(t.sum_ad[s] / N) : nan;
        a.out.rmse[o] = any ? (float)sqrt(sum_d2 / N) : nan;
        a.out.max_abs_error[o] = any ? t.max_ad[s] : nan;
        a.out.corr[o] = (c > 1 && m2_f != 0.0 && m2_o != 0.0) ? (float)(t.c_fo[s] / sqrt(m2_f * m2_o)) : nan;
        a.out.base_bias[o] = any ? (float)(t.sum_e[s] / N) : nan;
        a.out.base_mae[o] = any ? (float)(t.sum_ae[s] / N) : nan;
        a.out.base_rmse[o] = any ? (float)sqrt(sum_e2 / N) : nan;
        a.out.skill[o] = (any && sum_e2 != 0.0) ? (float)(1.0 - sum_d2 / sum_e2) : nan;
    }
    for (int e = 0; e < a.n_thr; ++e) {
        const int32_t c = t.n[(int64_t)a.thr_col[e] * a.n_total + g];
        const int32_t* cont = t.cont + (int64_t)e * 6 * a.n_total + g;
        const int64_t o = ic * a.n_thr + e;
        verify_table(cont[0], cont[a.n_total], cont[2 * a.n_total], c, a.out.pod, a.out.far, a.out.csi, a.out.fbias, a.out.ets, o);
        verify_table(cont[3 * a.n_total], cont[4 * a.n_total], cont[5 * a.n_total], c, a.out.base_pod, a.out.base_far, a.out.base_csi,
                     a.out.base_fbias, a.out.base_ets, o);
    }
}

bool verify_state_ok(const DpnVerifyState* s, const int n_thr) {
    return s && s->n && s->mean_f && s->mean_o && s->m2_f && s->m2_o && s->c_fo && s->sum_d && s->sum_ad && s->sum_d2 && s->sum_e && s->sum_ae &&
           s->sum_e2 && s->max_ad && (n_thr == 0 || s->cont);
}

bool verify_sizes_ok(const int n_products, const int n_thr, const int32_t* thr_col) {
    if (n_products < 1 || n_products > DPN_VERIFY_MAX_COLUMNS || n_thr < 0 || n_thr > DPN_VERIFY_MAX_THRESHOLDS) return false;
    if (n_thr > 0 && !thr_col) return false;
    for (int e = 0; e < n_thr; ++e)
        if (thr_col[e] < 0 || thr_col[e] >= n_products) return false;
    return true;
}

// The host checks that the seven entry points of this file and of dpn_pverify.inc share.
// Points first .. first + n of a state of n_total.
bool verify_range_ok(const int64_t n, const int64_t first, const int64_t n_total) { return n > 0 && first >= 0 && n_total > 0 && first <= n_total - n; }

// The column selectors into id[]: the value products 25, 26, 28..33 and no other.
bool verify_ids_ok(const int32_t* products, const int n_products, int32_t* id) {
    for (int j = 0; j < n_products; ++j) {
        id[j] = products[j];
        if (!(id[j] == 25 || id[j] == 26 || (id[j] >= 28 && id[j] <= 33))) return false;
    }
    return true;
}

// The thresholds into the launch arguments: every value finite, every side above or below.
bool verify_thresholds_ok(const int32_t* thr_col, const float* thr_val, const int32_t* thr_side, const int n_thr, int32_t* col, float* val,
                          int32_t* side) {
    if (n_thr > 0 && (!thr_val || !thr_side)) return false;
    for (int e = 0; e < n_thr; ++e) {
        if (!(thr_val[e] - thr_val[e] == 0.f)) return false;             // (a NaN or an infinity fails this)
        if (thr_side[e] != DPN_VERIFY_ABOVE && thr_side[e] != DPN_VERIFY_BELOW) return false;
        col[e] = thr_col[e];
        val[e] = thr_val[e];
        side[e] = thr_side[e];
    }
    return true;
}

// A pooling plan: segments that run from 0 to n_points without going back, and one block per (group, column).
bool verify_plan_ok(const int32_t* order, const int64_t* seg_start, const int64_t* seg_start_host, const int64_t n_points, const int64_t n_groups,
                    const int n_products) {
    if (!order || !seg_start || !seg_start_host || n_points <= 0 || n_groups <= 0) return false;
    if (n_groups * (int64_t)n_products > 0x7fffffff) return false;
    if (seg_start_host[0] != 0 || seg_start_host[n_groups] != n_points) return false;
    for (int64_t g = 0; g < n_groups; ++g)
        if (seg_start_host[g + 1] < seg_start_host[g]) return false;
    return true;
}

// with_clip == 0: the body then neither clips nor masks.
void verify_clip(DpnPhysics& ph, const int with_clip) {
    if (!with_clip)
        for (int k = 0; k < 6; ++k) ph.clip_on[k] = 0;
}

}  // namespace

extern "C" {

int dpn_verify_accumulate(const float* out_n, const float* coord_data, const float* obs, int64_t n, const DpnPhysics* phys, int with_clip,
                          const int32_t* products, int n_products, const int32_t* thr_col, const float* thr_val, const int32_t* thr_side, int n_thr,
                          int64_t first, int64_t n_total, const DpnVerifyState* state, void* stream) {
    if (!out_n || !coord_data || !obs || !phys || !products || !verify_range_ok(n, first, n_total)) return -1;
    if (!verify_sizes_ok(n_products, n_thr, thr_col) || !verify_state_ok(state, n_thr)) return -1;
    VerArgs a{out_n, coord_data, obs, n, first, n_total, *phys, n_products, n_thr, {}, {}, {}, {}, *state};
    if (!verify_ids_ok(products, n_products, a.id) || !verify_thresholds_ok(thr_col, thr_val, thr_side, n_thr, a.thr_col, a.thr_val, a.thr_side)) return -1;
    verify_clip(a.ph, with_clip);
    hipLaunchKernelGGL(dpn_verify_accumulate_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_verify_pool(const DpnVerifyState* points, int64_t n_points, const int32_t* order, const int64_t* seg_start, const int64_t* seg_start_host,
                    int64_t n_groups, int n_products, const int32_t* thr_col, int n_thr, const DpnVerifyState* groups, void* stream) {
    if (!verify_sizes_ok(n_products, n_thr, thr_col) || !verify_state_ok(points, n_thr) || !verify_state_ok(groups, n_thr)) return -1;
    if (!verify_plan_ok(order, seg_start, seg_start_host, n_points, n_groups, n_products)) return -1;
    VerPoolArgs a{*points, *groups, order, seg_start, n_points, n_groups, n_products, n_thr, {}};
    for (int e = 0; e < n_thr; ++e) a.thr_col[e] = thr_col[e];
    hipLaunchKernelGGL(dpn_verify_pool_kernel, dim3((unsigned)(n_groups * n_products)), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_verify_finish(const DpnVerifyState* state, int64_t n_total, int n_products, const int32_t* thr_col, int n_thr, int64_t first, int64_t n,
                      const DpnVerifyOut* rows, void* stream) {
    if (!rows || !verify_range_ok(n, first, n_total)) return -1;
    if (!verify_sizes_ok(n_products, n_thr, thr_col) || !verify_state_ok(state, n_thr)) return -1;
    const DpnVerifyOut& r = *rows;
    if (!r.count || !r.bias || !r.mae || !r.rmse || !r.max_abs_error || !r.corr || !r.base_bias || !r.base_mae || !r.base_rmse || !r.skill) return -1;
    if (n_thr > 0 && (!r.pod || !r.far || !r.csi || !r.fbias || !r.ets || !r.base_pod || !r.base_far || !r.base_csi || !r.base_fbias || !r.base_ets))
        return -1;
    VerFinishArgs a{*state, n, first, n_total, n_products, n_thr, {}, r};
    for (int e = 0; e < n_thr; ++e) a.thr_col[e] = thr_col[e];
    hipLaunchKernelGGL(dpn_verify_finish_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
