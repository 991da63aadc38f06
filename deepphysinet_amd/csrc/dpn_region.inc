// Regional statistics (DESIGN.md section 6b.5), included by dpn_diag.hip behind dpn_spell.inc: the space axis of the product table.  include/dpn_hip.h
// states the plan, the partial state and every operation's order.
//   dpn_region_accumulate : the products of points first .. first + n of a region-sorted, time-major point list folded into per-slot partial sums
//                           (weight, weighted sum, count, min, max and their places, weight above thresholds): the residual body per point and
//                           dpn_ensemble_accumulate's product expressions into an LDS tile [P][256], then lane L of each wave walks its wave's 64 points
//                           for column L (lanes P .. P + E - 1: for threshold L - P) in increasing order and flushes at every change of cell.
//   dpn_region_finish     : per (cell, column) the cell's slots merged in increasing order -> mean, total, weight, min, max, where, count, frac.
// Both kernels are compiled without contraction: every fp32 and fp64 operation is rounded on its own, so the numpy restatement
// (deepphysinet_amd/regions.py) reproduces partials and outputs bit for bit.  No atomics: a slot belongs to one (64-point group, cell) pair, hence to one
// lane of one launch.  Plain per-lane vector stores.

namespace {

constexpr int REG_TILE_LD = THREADS + 1;                      // the walk reads column L at lane L: rows one bank apart

struct RegArgs {
    const float *out_n, *jac_n, *f;
    int64_t n, first, n_slots;
    DpnPhysics ph;
    int32_t n_products, n_thr, n_sel, n_regions;
    int32_t id[DPN_REG_MAX_COLUMNS];                          // the column selector, in output order
    int32_t thr_col[DPN_REG_MAX_THRESHOLDS];                  // the column a threshold applies to
    float thr_val[DPN_REG_MAX_THRESHOLDS];
    const int32_t* seg;
    const float* wgt;
    DpnRegionState st;
};

template <bool WITH_J, bool WITH_F>
__global__ __launch_bounds__(THREADS) void dpn_region_accumulate_kernel(RegArgs e) {
#pragma clang fp contract(off)
    __shared__ float tile[DPN_REG_MAX_COLUMNS * REG_TILE_LD];
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic < e.n) {
        const EnsBody<WITH_J, WITH_F> a{e.out_n, EnsSrc<WITH_J>(e.jac_n), EnsSrc<WITH_F>(e.f), e.ph};
#include "dpn_residual_body.inc"
        const float zeta = J[1][0] - J[0][1];                 // the expressions of dpn_diagnostics_kernel, in its order
        const float div = J[0][0] + J[1][1];
        const float adv_T = u * J[3][0] + v * J[3][1];
        const float adv_q = u * J[4][0] + v * J[4][1];
        const float stretch = J[0][0] - J[1][1], shear = J[1][0] + J[0][1];
        bool poisoned = false;                                // its NaN rule: a NaN among the six normalised fields is a NaN in every product
#pragma unroll
        for (int k = 0; k < 6; ++k) { const float o_n = a.out_n[ic * 6 + k]; poisoned |= o_n != o_n; }
        for (int j = 0; j < e.n_products; ++j) {              // the selector is uniform: a scalar branch per product
            float x;
            switch (e.id[j]) {
#define DPN_REG_J(k) case 3 * k: x = J[k][0]; break; case 3 * k + 1: x = J[k][1]; break; case 3 * k + 2: x = J[k][2]; break;
                DPN_REG_J(0) DPN_REG_J(1) DPN_REG_J(2) DPN_REG_J(3) DPN_REG_J(4) DPN_REG_J(5)
#undef DPN_REG_J
                case 18: x = zeta; break;
                case 19: x = zeta + fc; break;
                case 20: x = div; break;
                case 21: x = omega; break;
                case 22: x = -adv_T; break;
                case 23: x = -adv_q; break;
                case 24: x = q * div + adv_q; break;
                case 25: x = sqrtf(u * u + v * v); break;
                case 26: x = q / q_s; break;
                case 27: x = sqrtf(stretch * stretch + shear * shear); break;
                case 28: x = u; break;
                case 29: x = v; break;
                case 30: x = p; break;
                case 31: x = T; break;
                case 32: x = q; break;
                default: x = rho; break;                      // 33 (the entry point admits 0..33 only)
            }
            tile[j * REG_TILE_LD + threadIdx.x] = poisoned ? __builtin_nanf("") : x;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (DPN_REG_GROUP - 1), wave = threadIdx.x / DPN_REG_GROUP;
    const int64_t base = (int64_t)blockIdx.x * THREADS + wave * DPN_REG_GROUP;          // the chunk row of the wave's first point
    if (base >= e.n || lane >= e.n_products + e.n_thr) return;
    const int cnt = e.n - base < DPN_REG_GROUP ? (int)(e.n - base) : DPN_REG_GROUP;
    const bool is_thr = lane >= e.n_products;
    const int col = is_thr ? e.thr_col[lane - e.n_products] : lane;
    const float thr = is_thr ? e.thr_val[lane - e.n_products] : 0.f;
    const int64_t i0 = e.first + base, grp = i0 / DPN_REG_GROUP;                         // first and base are multiples of the group
    int32_t it = (int32_t)(i0 / e.n_sel), j = (int32_t)(i0 - (int64_t)it * e.n_sel);
    const float* xs = tile + col * REG_TILE_LD + wave * DPN_REG_GROUP;
    int64_t cell = -1;
    double w = 0.0, wx = 0.0;
    int32_t count = 0, imin = 0, imax = 0;
    float vmin = 0.f, vmax = 0.f;
    const auto flush = [&]() {
        const int64_t s = grp + cell;
        if (is_thr) {
            e.st.wexc[(int64_t)(lane - e.n_products) * e.n_slots + s] = w;
        } else if (count > 0) {                               // (an uncounted slot keeps the memset's zeros)
            const int64_t o = (int64_t)col * e.n_slots + s;
            e.st.w[o] = w;
            e.st.wx[o] = wx;
            e.st.count[o] = count;
            e.st.vmin[o] = vmin;
            e.st.vmax[o] = vmax;
            e.st.imin[o] = imin;
            e.st.imax[o] = imax;
        }
    };
    for (int k = 0; k < cnt; ++k) {
        const int32_t sg = e.seg[j];
        if ((uint32_t)sg < (uint32_t)e.n_regions) {           // (a plan's seg lies in 0 .. R - 1; an entry outside is no point of any cell)
            const int64_t c = (int64_t)it * e.n_regions + sg;
            if (c != cell) {
                if (cell >= 0) flush();
                cell = c;
                w = 0.0; wx = 0.0; count = 0;
            }
            const float x = xs[k], wt = e.wgt[j];
            if (__builtin_isfinite(x) && wt != 0.f) {
                if (is_thr) {
                    if (x > thr) w = w + (double)wt;
                } else {
                    if (count == 0) {                         // min and max are not read before they are set
                        vmin = x; vmax = x; imin = j; imax = j;
                    } else {                                  // strict: a tie, +0 against -0 included, keeps the earlier point
                        if (x < vmin) { vmin = x; imin = j; }
                        if (x > vmax) { vmax = x; imax = j; }
                    }
                    count += 1;
                    w = w + (double)wt;
                    wx = wx + (double)wt * (double)x;         // the product of two floats is exact in fp64: one rounding
                }
            }
        }
        if (++j == e.n_sel) { j = 0; ++it; }
    }
    if (cell >= 0) flush();
}

struct RegFinishArgs {
    const int32_t* offs;
    int64_t n_slots, n_sel;
    int32_t n_regions, nt, n_products, n_thr;
    int32_t thr_col[DPN_REG_MAX_THRESHOLDS];
    DpnRegionState st;
    DpnRegionOut out;
};

__global__ __launch_bounds__(THREADS) void dpn_region_finish_kernel(RegFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (tid >= (int64_t)a.nt * a.n_regions * a.n_products) return;
    const int64_t c = tid / a.n_products;
    const int col = (int)(tid - c * a.n_products);
    const int64_t it = c / a.n_regions;
    const int r = (int)(c - it * a.n_regions);
    const int64_t o0 = a.offs[r], o1 = a.offs[r + 1];
    int64_t s0 = 0, s1 = -1;                                  // an empty region has no slot
    if (o1 > o0) {
        s0 = (it * a.n_sel + o0) / DPN_REG_GROUP + c;
        s1 = (it * a.n_sel + o1 - 1) / DPN_REG_GROUP + c;
    }
    const int64_t at = (int64_t)col * a.n_slots;
    double w = 0.0, wx = 0.0;
    int32_t count = 0, imin = -1, imax = -1;
    float vmin = 0.f, vmax = 0.f;
    for (int64_t s = s0; s <= s1; ++s) {
        const int32_t cs = a.st.count[at + s];
        if (cs == 0) continue;
        const float lo = a.st.vmin[at + s], hi = a.st.vmax[at + s];
        if (count == 0) {
            vmin = lo; vmax = hi; imin = a.st.imin[at + s]; imax = a.st.imax[at + s];
        } else {                                              // the earlier slot's stays on a tie
            if (lo < vmin) { vmin = lo; imin = a.st.imin[at + s]; }
            if (hi > vmax) { vmax = hi; imax = a.st.imax[at + s]; }
        }
        count += cs;
        w = w + a.st.w[at + s];
        wx = wx + a.st.wx[at + s];
    }
    const float nan = __builtin_nanf("");
    const int64_t o = c * a.n_products + col;
    a.out.count[o] = count;
    a.out.weight[o] = (float)w;
    a.out.mean[o] = count > 0 ? (float)(wx / w) : nan;
    a.out.total[o] = count > 0 ? (float)wx : nan;
    a.out.min[o] = count > 0 ? vmin : nan;
    a.out.max[o] = count > 0 ? vmax : nan;
    a.out.where_min[o] = imin;
    a.out.where_max[o] = imax;
    for (int t = 0; t < a.n_thr; ++t) {
        if (a.thr_col[t] != col) continue;
        double wexc = 0.0;
        for (int64_t s = s0; s <= s1; ++s)
            if (a.st.count[at + s] != 0) wexc = wexc + a.st.wexc[(int64_t)t * a.n_slots + s];
        a.out.frac[c * a.n_thr + t] = count > 0 ? (float)(wexc / w) : nan;
    }
}

// -1 unless the plan is one of nt * n_sel < 2^31 points in at least one region; -> the number of slots
int64_t reg_slots(const DpnRegionPlan* p) {
    if (!p || p->n_sel < 1 || p->n_regions < 1 || p->nt < 1) return -1;
    if (p->n_sel > INT32_MAX || (int64_t)p->nt * p->n_sel > INT32_MAX) return -1;
    return ((int64_t)p->nt * p->n_sel + DPN_REG_GROUP - 1) / DPN_REG_GROUP + (int64_t)p->nt * p->n_regions;
}

bool reg_counts_ok(const int n_products, const int n_thr) {
    return n_products >= 1 && n_products <= DPN_REG_MAX_COLUMNS && n_thr >= 0 && n_thr <= DPN_REG_MAX_THRESHOLDS;
}

bool reg_state_ok(const DpnRegionState* s, const int n_thr) {
    return s && s->w && s->wx && s->count && s->vmin && s->vmax && s->imin && s->imax && (n_thr == 0 || s->wexc);
}

}  // namespace

extern "C" {

int dpn_region_accumulate(const float* out_n, const float* jac_n, const float* f, int64_t n, const DpnPhysics* phys, int with_clip,
                          const int32_t* products, int n_products, const int32_t* thr_col, const float* thr_val, int n_thr, int64_t first,
                          const DpnRegionPlan* plan, const DpnRegionState* state, void* stream) {
    const int64_t n_slots = reg_slots(plan);
    if (!out_n || !phys || !products || n_slots < 0 || !plan->seg || !plan->wgt) return -1;
    if (!reg_counts_ok(n_products, n_thr) || !reg_state_ok(state, n_thr)) return -1;
    if (n_thr > 0 && (!thr_col || !thr_val)) return -1;
    if (n <= 0 || first < 0 || first % DPN_REG_GROUP != 0 || first > (int64_t)plan->nt * plan->n_sel - n) return -1;
    RegArgs a{out_n, jac_n, f, n, first, n_slots, *phys, n_products, n_thr, (int32_t)plan->n_sel, plan->n_regions, {}, {}, {}, plan->seg, plan->wgt, *state};
    bool need_j = false, need_f = false;
    for (int j = 0; j < n_products; ++j) {
        if (products[j] < 0 || products[j] >= DPN_ENS_PRODUCTS) return -1;
        a.id[j] = products[j];
        need_j |= ens_reads_jac(products[j]);
        need_f |= products[j] == 19;
    }
    if ((need_j && !jac_n) || (need_f && !f)) return -1;
    for (int t = 0; t < n_thr; ++t) {
        if (thr_col[t] < 0 || thr_col[t] >= n_products || !(thr_val[t] - thr_val[t] == 0.f)) return -1;      // (a NaN or an infinity fails the last)
        a.thr_col[t] = thr_col[t];
        a.thr_val[t] = thr_val[t];
    }
    if (!with_clip)
        for (int k = 0; k < 6; ++k) a.ph.clip_on[k] = 0;                  // the body then neither clips nor masks
    const dim3 grid((unsigned)((n + THREADS - 1) / THREADS)), block(THREADS);
    if (need_f)
        hipLaunchKernelGGL((dpn_region_accumulate_kernel<true, true>), grid, block, 0, (hipStream_t)stream, a);
    else if (need_j)
        hipLaunchKernelGGL((dpn_region_accumulate_kernel<true, false>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((dpn_region_accumulate_kernel<false, false>), grid, block, 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_region_finish(const DpnRegionPlan* plan, const DpnRegionState* state, int n_products, const int32_t* thr_col, int n_thr,
                      const DpnRegionOut* out, void* stream) {
    const int64_t n_slots = reg_slots(plan);
    if (n_slots < 0 || !plan->offs || !reg_counts_ok(n_products, n_thr) || !reg_state_ok(state, n_thr) || !out) return -1;
    if (!out->mean || !out->total || !out->weight || !out->min || !out->max || !out->where_min || !out->where_max || !out->count) return -1;
    if (n_thr > 0 && (!thr_col || !out->frac)) return -1;
    RegFinishArgs a{plan->offs, n_slots, plan->n_sel, plan->n_regions, plan->nt, n_products, n_thr, {}, *state, *out};
    for (int t = 0; t < n_thr; ++t) {
        if (thr_col[t] < 0 || thr_col[t] >= n_products) return -1;
        a.thr_col[t] = thr_col[t];
    }
    const int64_t threads = (int64_t)plan->nt * plan->n_regions * n_products;
    if ((threads + THREADS - 1) / THREADS > INT32_MAX) return -1;
    hipLaunchKernelGGL(dpn_region_finish_kernel, dim3((unsigned)((threads + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
