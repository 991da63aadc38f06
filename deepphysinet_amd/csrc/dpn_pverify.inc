// Probabilistic verification of ensembles against observations (DESIGN.md section 6b.7), included by dpn_diag.hip behind dpn_verify.inc, whose
// verify_values / verify_pick / verify_event and host checks (verify_*_ok, verify_clip) it reuses: the member axis and the case axis of the value products together.
// include/dpn_hip.h states the layouts and every operation's order.
//   dpn_pverify_stage  : ONE member's forecast (out_n) and baseline (coord_data) values of every column at points first .. first + n into two resident
//                        fp32 planes [M][P][n_total], one thread per point.
//   dpn_pverify_case   : the M staged members of ONE case at points first .. first + n against obs, folded into a resident state (count, CRPS and
//                        error sums, rank histogram, reliability table).  One 64-thread block per 64 points; a thread copies the 2 x M values of
//                        its point and column into LDS as [side][M][64], lane = point, and walks its own column there, so the M^2 pair loop indexes
//                        LDS and no private array: every ds_read_b32 of the wave hits 64 consecutive dwords.  A thread reads only what it wrote
//                        itself: no barrier.
//   dpn_pverify_pool   : the states of N points -> the states of G groups, one 64-lane wave per (group, column): 64 strided left folds, then lane 0
//                        folds the lane results in lane order.  Every field is a sum.
//   dpn_pverify_finish : a state -> the scores, as rows.
// All four are compiled without contraction: every fp32 and fp64 operation is rounded on its own, so the numpy restatement
// (deepphysinet_amd/prob_verification.py) reproduces them bit for bit.  No atomics, plain per-lane vector stores.

namespace {

constexpr int PV_TILE = 64;                                   // points per block of dpn_pverify_case: one wave
constexpr int PV_SUMS = 5;                                    // sum_crps, sum_fair, sum_d, sum_d2, sum_var

struct PvStageArgs {
    const float *out_n, *coord_data;
    int64_t n, first, n_total;
    DpnPhysics ph;
    int32_t n_products, member;
    int32_t id[DPN_VERIFY_MAX_COLUMNS];
    float *plane_f, *plane_b;
};

__global__ __launch_bounds__(THREADS) void dpn_pverify_stage_kernel(PvStageArgs a) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= a.n) return;
    const VerValues fc = verify_values(a.out_n, a.ph, ic), bs = verify_values(a.coord_data, a.ph, ic);
    const int64_t at = (int64_t)a.member * a.n_products * a.n_total + a.first + ic;
    for (int j = 0; j < a.n_products; ++j) {                  // the selector is uniform: a scalar branch per column
        a.plane_f[at + (int64_t)j * a.n_total] = verify_pick(fc, a.id[j]);
        a.plane_b[at + (int64_t)j * a.n_total] = verify_pick(bs, a.id[j]);
    }
}

// The arrays of a state as the kernels index them: the five sums in DpnPVerifyState's order.
struct PvState {
    int32_t* n;
    double* sum[PV_SUMS];
    int32_t *rank, *rel;
};

PvState pv_state(const DpnPVerifyState& s) { return PvState{s.n, {s.sum_crps, s.sum_fair, s.sum_d, s.sum_d2, s.sum_var}, s.rank, s.rel}; }

struct PvCaseArgs {
    const float *plane_f, *plane_b, *obs;
    int64_t n, first, n_total;
    int32_t n_products, n_thr, n_members;
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
    float thr_val[DPN_VERIFY_MAX_THRESHOLDS];
    int32_t thr_side[DPN_VERIFY_MAX_THRESHOLDS];
    PvState st;
};

__global__ __launch_bounds__(PV_TILE) void dpn_pverify_case_kernel(PvCaseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float pv_tile[];       // [2][M][PV_TILE]
    const int lane = threadIdx.x;
    const int64_t ic = (int64_t)blockIdx.x * PV_TILE + lane;
    if (ic >= a.n) return;                                    // (no barrier below: a thread reads its own LDS column only)
    const int64_t g = a.first + ic, N = a.n_total;
    const int M = a.n_members, P = a.n_products;
    const double Md = (double)M;
    const PvState& t = a.st;
    for (int j = 0; j < P; ++j) {
        const float o = a.obs[ic * P + j];
        bool ok = __builtin_isfinite(o);
        for (int side = 0; side < 2; ++side) {
            const float* src = (side ? a.plane_b : a.plane_f) + (int64_t)j * N + g;
            for (int m = 0; m < M; ++m) {
                const float x = src[(int64_t)m * P * N];
                ok &= __builtin_isfinite(x);
                pv_tile[(side * M + m) * PV_TILE + lane] = x;
            }
        }
        if (!ok) continue;
        const double O = (double)o;
        t.n[(int64_t)j * N + g] += 1;
        for (int side = 0; side < 2; ++side) {
            const float* col = pv_tile + side * M * PV_TILE + lane;
            double A = 0.0, S = 0.0;
            int lt = 0, eq = 0;
            for (int m = 0; m < M; ++m) {
                const float x = col[m * PV_TILE];
                const double X = (double)x;
                A = A + fabs(X - O);
                S = S + X;
                lt += x < o;
                eq += x == o;
            }
            double G = 0.0;
            for (int i = 0; i < M; ++i) {
                const double Xi = (double)col[i * PV_TILE];
                for (int k = i + 1; k < M; ++k) G = G + fabs(Xi - (double)col[k * PV_TILE]);
            }
            const double mean = S / Md, d = mean - O;
            double V = 0.0;
            for (int m = 0; m < M; ++m) {
                const double r = (double)col[m * PV_TILE] - mean;
                V = V + r * r;
            }
            const double am = A / Md;
            const double crps = am - G / (Md * Md);
            const double fair = M > 1 ? am - G / (Md * (Md - 1.0)) : A;
            const double var = M > 1 ? V / (Md - 1.0) : 0.0;
            const int64_t s = ((int64_t)side * P + j) * N + g;
            t.sum[0][s] = t.sum[0][s] + crps;
            t.sum[1][s] = t.sum[1][s] + fair;
            t.sum[2][s] = t.sum[2][s] + d;
            t.sum[3][s] = t.sum[3][s] + d * d;
            t.sum[4][s] = t.sum[4][s] + var;
            t.rank[(((int64_t)side * P + j) * (M + 1) + (lt + eq / 2)) * N + g] += 1;
            for (int i = 0; i < a.n_thr; ++i) {
                if (a.thr_col[i] != j) continue;
                int k = 0;
                for (int m = 0; m < M; ++m) k += verify_event(col[m * PV_TILE], a.thr_val[i], a.thr_side[i]);
                int32_t* rel = t.rel + ((((int64_t)i * 2 + side) * 2) * (M + 1) + k) * N + g;
                rel[0] += 1;                                  // pairs at probability level k / M
                if (verify_event(o, a.thr_val[i], a.thr_side[i])) rel[(int64_t)(M + 1) * N] += 1;      // .. whose report is an event
            }
        }
    }
}

struct PvPoolArgs {
    PvState src, dst;
    const int32_t* order;
    const int64_t* seg_start;
    int64_t n_points, n_groups;
    int32_t n_products, n_thr, n_members;
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
};

// The int32 sum of src[pt] over the valid places lo + lane, lo + lane + 64, .. < hi of `order`, in every lane of the result's lane 0.
__device__ __forceinline__ int32_t pv_segment_sum(const int32_t* src, const int32_t* order, const int64_t lo, const int64_t hi, const int64_t n_points,
                                                  const int lane) {
    int32_t sum = 0;
    for (int64_t k = lo + lane; k < hi; k += 64) {
        const int64_t pt = order[k];
        if (pt >= 0 && pt < n_points) sum += src[pt];
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    return sum;
}

// One 64-thread block = one wave = one (group, column).
__global__ __launch_bounds__(64) void dpn_pverify_pool_kernel(PvPoolArgs a) {
#pragma clang fp contract(off)
    const int64_t w = blockIdx.x;
    const int64_t grp = w / a.n_products;
    const int j = (int)(w - grp * a.n_products), lane = threadIdx.x;
    const int64_t lo = a.seg_start[grp], hi = a.seg_start[grp + 1], N = a.n_points, G = a.n_groups;
    const int P = a.n_products, M1 = a.n_members + 1;
    double acc[2][PV_SUMS] = {};
    for (int64_t k = lo + lane; k < hi; k += 64) {
        const int64_t pt = a.order[k];
        if (pt < 0 || pt >= N) continue;
#pragma unroll
        for (int side = 0; side < 2; ++side)
#pragma unroll
            for (int f = 0; f < PV_SUMS; ++f) acc[side][f] = acc[side][f] + a.src.sum[f][((int64_t)side * P + j) * N + pt];
    }
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int f = 0; f < PV_SUMS; ++f) {
            double all = acc[side][f];                        // lane 0's: the fold of the 64 lane results in lane order
            for (int l = 1; l < 64; ++l) all = all + __shfl(acc[side][f], l, 64);
            if (lane == 0) a.dst.sum[f][((int64_t)side * P + j) * G + grp] = all;
        }
    // the integer fields: sums, any order is the same
    const int32_t c = pv_segment_sum(a.src.n + (int64_t)j * N, a.order, lo, hi, N, lane);
    if (lane == 0) a.dst.n[(int64_t)j * G + grp] = c;
    for (int side = 0; side < 2; ++side)
        for (int b = 0; b < M1; ++b) {
            const int64_t row = ((int64_t)side * P + j) * M1 + b;
            const int32_t r = pv_segment_sum(a.src.rank + row * N, a.order, lo, hi, N, lane);
            if (lane == 0) a.dst.rank[row * G + grp] = r;
        }
    for (int i = 0; i < a.n_thr; ++i) {
        if (a.thr_col[i] != j) continue;
        for (int c4 = 0; c4 < 4 * M1; ++c4) {                 // (side, pairs | events, level): the rows of this threshold
            const int64_t row = (int64_t)i * 4 * M1 + c4;
            const int32_t r = pv_segment_sum(a.src.rel + row * N, a.order, lo, hi, N, lane);
            if (lane == 0) a.dst.rel[row * G + grp] = r;
        }
    }
}

struct PvFinishArgs {
    PvState st;
    int64_t n, first, n_total;
    int32_t n_products, n_thr, n_members;
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
    DpnPVerifyOut out;
};

__global__ __launch_bounds__(THREADS) void dpn_pverify_finish_kernel(PvFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= a.n) return;
    const int64_t g = a.first + ic, N = a.n_total;
    const int M = a.n_members, M1 = M + 1, P = a.n_products;
    const double Md = (double)M;
    const float nan = __builtin_nanf("");
    const PvState& t = a.st;
    const DpnPVerifyOut& r = a.out;
    for (int j = 0; j < P; ++j) {
        const int64_t o = ic * P + j;
        const int32_t c = t.n[(int64_t)j * N + g];
        const double Nd = (double)c;
        const bool any = c > 0;
        r.count[o] = c;
        for (int side = 0; side < 2; ++side) {
            const int64_t s = ((int64_t)side * P + j) * N + g;
            const double mse = t.sum[3][s] / Nd, mvar = t.sum[4][s] / Nd;
            const double rmse = sqrt(mse);
            (side ? r.base_crps : r.crps)[o] = any ? (float)(t.sum[0][s] / Nd) : nan;
            (side ? r.base_fair_crps : r.fair_crps)[o] = any ? (float)(t.sum[1][s] / Nd) : nan;
            (side ? r.base_bias : r.bias)[o] = any ? (float)(t.sum[2][s] / Nd) : nan;
            (side ? r.base_rmse : r.rmse)[o] = any ? (float)rmse : nan;
            (side ? r.base_spread : r.spread)[o] = any ? (float)sqrt(mvar) : nan;
            (side ? r.base_spread_skill : r.spread_skill)[o] = (any && M > 1 && rmse != 0.0) ? (float)(sqrt(((Md + 1.0) / Md) * mvar) / rmse) : nan;
            int32_t* hist = (side ? r.base_rank_hist : r.rank_hist) + o * M1;
            for (int b = 0; b < M1; ++b) hist[b] = t.rank[(((int64_t)side * P + j) * M1 + b) * N + g];
        }
        const int64_t sf = (int64_t)j * N + g, sb = ((int64_t)P + j) * N + g;
        r.crpss[o] = (any && t.sum[0][sb] != 0.0) ? (float)(1.0 - t.sum[0][sf] / t.sum[0][sb]) : nan;
        r.fair_crpss[o] = (any && t.sum[1][sb] != 0.0) ? (float)(1.0 - t.sum[1][sf] / t.sum[1][sb]) : nan;
    }
    for (int e = 0; e < a.n_thr; ++e) {
        const int64_t o = ic * a.n_thr + e;
        const int32_t c = t.n[(int64_t)a.thr_col[e] * N + g];
        const double Nd = (double)c;
        const bool any = c > 0;
        for (int side = 0; side < 2; ++side) {
            const int32_t* rel_n = t.rel + (((int64_t)e * 2 + side) * 2) * M1 * N + g;
            const int32_t* rel_o = rel_n + (int64_t)M1 * N;
            int32_t* dn = (side ? r.base_rel_n : r.rel_n) + o * M1;
            int32_t* dob = (side ? r.base_rel_o : r.rel_o) + o * M1;
            int32_t events = 0;
            double bacc = 0.0;
            for (int k = 0; k < M1; ++k) {
                const int32_t nk = rel_n[(int64_t)k * N], ok = rel_o[(int64_t)k * N];
                dn[k] = nk;
                dob[k] = ok;
                events += ok;
                const double p = (double)k / Md, q = 1.0 - p;
                bacc = bacc + ((double)ok * (q * q) + (double)(nk - ok) * (p * p));
            }
            const double obar = (double)events / Nd;
            double racc = 0.0, sacc = 0.0;
            for (int k = 0; k < M1; ++k) {
                const int32_t nk = rel_n[(int64_t)k * N];
                if (nk <= 0) continue;
                const double nd = (double)nk, f = (double)rel_o[(int64_t)k * N] / nd, p = (double)k / Md;
                const double u = p - f, v = f - obar;
                racc = racc + nd * (u * u);
                sacc = sacc + nd * (v * v);
            }
            double area = 0.0;                                // the trapezoids from "at least M + 1 members" (0, 0) down to "at least 0" (1, 1)
            int32_t above = 0;                                // the events at the levels above k
            for (int k = M; k >= 0; --k) {
                const int32_t nk = rel_n[(int64_t)k * N], ok = rel_o[(int64_t)k * N];
                area = area + (double)(nk - ok) * ((double)above + (double)(above + ok));
                above += ok;
            }
            const double brier = bacc / Nd, unc = obar * (1.0 - obar);
            (side ? r.base_brier : r.brier)[o] = any ? (float)brier : nan;
            (side ? r.base_reliability : r.reliability)[o] = any ? (float)(racc / Nd) : nan;
            (side ? r.base_resolution : r.resolution)[o] = any ? (float)(sacc / Nd) : nan;
            (side ? r.base_bss : r.bss)[o] = (any && unc != 0.0) ? (float)(1.0 - brier / unc) : nan;
            (side ? r.base_roc_area : r.roc_area)[o] =
                (any && events > 0 && c - events > 0) ? (float)(area / ((2.0 * (double)events) * (double)(c - events))) : nan;
            if (side == 0) r.uncertainty[o] = any ? (float)unc : nan;
        }
    }
}

bool pv_state_ok(const DpnPVerifyState* s, const int n_thr) {
    return s && s->n && s->sum_crps && s->sum_fair && s->sum_d && s->sum_d2 && s->sum_var && s->rank && (n_thr == 0 || s->rel);
}

bool pv_members_ok(const int n_members) { return n_members >= 1 && n_members <= DPN_PV_MAX_MEMBERS; }

}  // namespace

extern "C" {

int dpn_pverify_stage(const float* out_n, const float* coord_data, int64_t n, const DpnPhysics* phys, int with_clip, const int32_t* products,
                      int n_products, int member, int n_members, int64_t first, int64_t n_total, float* plane_f, float* plane_b, void* stream) {
    if (!out_n || !coord_data || !phys || !products || !plane_f || !plane_b) return -1;
    if (!verify_range_ok(n, first, n_total) || !verify_sizes_ok(n_products, 0, nullptr) || !pv_members_ok(n_members)) return -1;
    if (member < 0 || member >= n_members) return -1;
    PvStageArgs a{out_n, coord_data, n, first, n_total, *phys, n_products, member, {}, plane_f, plane_b};
    if (!verify_ids_ok(products, n_products, a.id)) return -1;
    verify_clip(a.ph, with_clip);
    hipLaunchKernelGGL(dpn_pverify_stage_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_pverify_case(const float* plane_f, const float* plane_b, const float* obs, int64_t n, int n_products, const int32_t* thr_col,
                     const float* thr_val, const int32_t* thr_side, int n_thr, int n_members, int64_t first, int64_t n_total,
                     const DpnPVerifyState* state, void* stream) {
    if (!plane_f || !plane_b || !obs) return -1;
    if (!verify_range_ok(n, first, n_total) || !verify_sizes_ok(n_products, n_thr, thr_col) || !pv_members_ok(n_members)) return -1;
    if (!pv_state_ok(state, n_thr)) return -1;
    PvCaseArgs a{plane_f, plane_b, obs, n, first, n_total, n_products, n_thr, n_members, {}, {}, {}, pv_state(*state)};
    if (!verify_thresholds_ok(thr_col, thr_val, thr_side, n_thr, a.thr_col, a.thr_val, a.thr_side)) return -1;
    const size_t lds = (size_t)2 * n_members * PV_TILE * sizeof(float);  // at most 32 KiB
    hipLaunchKernelGGL(dpn_pverify_case_kernel, dim3((unsigned)((n + PV_TILE - 1) / PV_TILE)), dim3(PV_TILE), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_pverify_pool(const DpnPVerifyState* points, int64_t n_points, const int32_t* order, const int64_t* seg_start, const int64_t* seg_start_host,
                     int64_t n_groups, int n_products, const int32_t* thr_col, int n_thr, int n_members, const DpnPVerifyState* groups, void* stream) {
    if (!verify_sizes_ok(n_products, n_thr, thr_col) || !pv_members_ok(n_members)) return -1;
    if (!pv_state_ok(points, n_thr) || !pv_state_ok(groups, n_thr)) return -1;
    if (!verify_plan_ok(order, seg_start, seg_start_host, n_points, n_groups, n_products)) return -1;
    PvPoolArgs a{pv_state(*points), pv_state(*groups), order, seg_start, n_points, n_groups, n_products, n_thr, n_members, {}};
    for (int e = 0; e < n_thr; ++e) a.thr_col[e] = thr_col[e];
    hipLaunchKernelGGL(dpn_pverify_pool_kernel, dim3((unsigned)(n_groups * n_products)), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_pverify_finish(const DpnPVerifyState* state, int64_t n_total, int n_products, const int32_t* thr_col, int n_thr, int n_members, int64_t first,
                       int64_t n, const DpnPVerifyOut* rows, void* stream) {
    if (!rows || !verify_range_ok(n, first, n_total)) return -1;
    if (!verify_sizes_ok(n_products, n_thr, thr_col) || !pv_members_ok(n_members) || !pv_state_ok(state, n_thr)) return -1;
    const DpnPVerifyOut& r = *rows;
    if (!r.count || !r.crps || !r.fair_crps || !r.bias || !r.rmse || !r.spread || !r.spread_skill || !r.base_crps || !r.base_fair_crps || !r.base_bias ||
        !r.base_rmse || !r.base_spread || !r.base_spread_skill || !r.crpss || !r.fair_crpss || !r.rank_hist || !r.base_rank_hist)
        return -1;
    if (n_thr > 0 && (!r.brier || !r.reliability || !r.resolution || !r.bss || !r.roc_area || !r.base_brier || !r.base_reliability || !r.base_resolution ||
                      !r.base_bss || !r.base_roc_area || !r.uncertainty || !r.rel_n || !r.rel_o || !r.base_rel_n || !r.base_rel_o))
        return -1;
    PvFinishArgs a{pv_state(*state), n, first, n_total, n_products, n_thr, n_members, {}, r};
    for (int e = 0; e < n_thr; ++e) a.thr_col[e] = thr_col[e];
    hipLaunchKernelGGL(dpn_pverify_finish_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
