// Window extremes and means in time (DESIGN.md section 6b.3), included by dpn_diag.hip behind dpn_ensemble.inc: a coarse scan of the window, then
// bisection on the sign of the network's own d/dt around the best scan node.  include/dpn_hip.h states the state's layout and every operation's order.
//   dpn_extreme_scan   : scan node k's fields-only forward folded into the state (best value and node, the trapezoid sum), and the sampler at node
//                        k + 1 written where the next forward reads it.
//   dpn_extreme_begin  : the scan's close: the bracket around the best node and the first probe of every max / min column; the mean of a mean column.
//   dpn_extreme_refine : one round: the probe's value and slope from the forward with the Jacobian, the best so far, the halved bracket, the next probe.
// One thread per (column, point), 256-thread blocks; the state is column-major ([column][point]), so a wave runs along the points.  The kernels are
// compiled without contraction: every fp32 and fp64 operation is rounded on its own, and the numpy restatement (deepphysinet_amd/extremes.py)
// reproduces them bit for bit.  No atomics (a (column, point) belongs to one thread, launches follow each other on one stream), no LDS, plain per-lane
// stores.  sample_point is the sampler unit's own (dpn_sample_point.h); the product values come from the residual body, as the ensemble's do.

namespace {

struct ExtArgs {
    DpnSampler s;
    const float* cube;
    DpnPhysics ph;
    const float *out_n, *jac_n;
    int64_t n;
    int32_t n_columns, n_refined, k, K, round;
    double t0, dt;
    const double *xr, *yr;
    int32_t id[DPN_EXT_MAX_COLUMNS], sense[DPN_EXT_MAX_COLUMNS];
    int32_t column_of[DPN_EXT_MAX_COLUMNS];                   // refined column r -> its column in the request
    int32_t refined_of[DPN_EXT_MAX_COLUMNS];                  // column -> its place among the refined ones (max / min columns in request order)
    DpnExtremeState st;
    float *x, *y, *t, *f, *coord_data;
};

// Product `id` (25 speed, 28..33 u, v, p, T, q, rho) at row ic of out_n / jac_n: the value x as dpn_ensemble_accumulate forms it (the residual body,
// its NaN rule) and, WITH_J, its slope in time s = d x / d t up to a positive factor.
template <bool WITH_J>
__device__ __forceinline__ void ext_product(const float* out_n, const float* jac_n, const DpnPhysics& ph, const int64_t ic, const int32_t id, float& x,
                                            float& s) {
#pragma clang fp contract(off)
    const EnsBody<WITH_J, false> a{out_n, EnsSrc<WITH_J>(jac_n), EnsSrc<false>(nullptr), ph};
#include "dpn_residual_body.inc"
    bool poisoned = false;                                    // a NaN among the six normalised fields is a NaN in every product
#pragma unroll
    for (int k = 0; k < 6; ++k) { const float o_n = a.out_n[ic * 6 + k]; poisoned |= o_n != o_n; }
    switch (id) {
        case 25: x = sqrtf(u * u + v * v); s = u * J[0][2] + v * J[1][2]; break;      // the sign of d speed / dt: nothing is divided
        case 28: x = u; s = J[0][2]; break;
        case 29: x = v; s = J[1][2]; break;
        case 30: x = p; s = J[2][2]; break;
        case 31: x = T; s = J[3][2]; break;
        case 32: x = q; s = J[4][2]; break;
        default: x = rho; s = J[5][2]; break;                 // 33 (the entry points admit 25 and 28..33 only)
    }
    if (poisoned) x = __builtin_nanf("");
}

__global__ __launch_bounds__(THREADS) void dpn_extreme_scan_kernel(ExtArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.n * a.n_columns) return;
    const int64_t c = idx / a.n, i = idx - c * a.n;           // idx is the state's place [c][i]
    if (c == 0 && a.k < a.K)                                  // the next node's forward reads these; whatever the columns' status
        sample_point(a.s, a.cube, a.xr[i], a.yr[i], a.t0 + (double)(a.k + 1) * a.dt, i, a.x, a.y, a.t, a.f, a.coord_data);
    float x, s;
    ext_product<false>(a.out_n, nullptr, a.ph, i, a.id[c], x, s);
    if (a.k > 0 && a.st.status[idx] != DPN_EXT_OK) return;    // sticky
    if (!__builtin_isfinite(x)) { a.st.status[idx] = DPN_EXT_BAD_SCAN; return; }
    if (a.k == 0) {
        a.st.status[idx] = DPN_EXT_OK;
        a.st.best_v[idx] = x;
        a.st.best_k[idx] = 0;
        a.st.acc[idx] = 0.5 * (double)x;
        return;
    }
    const float best = a.st.best_v[idx];
    const int32_t sense = a.sense[c];
    if ((sense == DPN_EXT_MAX && x > best) || (sense == DPN_EXT_MIN && x < best)) {          // a tie keeps the earlier node
        a.st.best_v[idx] = x;
        a.st.best_k[idx] = a.k;
    }
    a.st.acc[idx] = a.st.acc[idx] + (a.k == a.K ? 0.5 : 1.0) * (double)x;
}

__global__ __launch_bounds__(THREADS) void dpn_extreme_begin_kernel(ExtArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.n * a.n_columns) return;
    const int64_t c = idx / a.n, i = idx - c * a.n;
    const bool ok = a.st.status[idx] == DPN_EXT_OK;
    const double qnan = __builtin_nan("");
    if (a.sense[c] == DPN_EXT_MEAN) {
        a.st.best_v[idx] = ok ? (float)(a.st.acc[idx] / (double)a.K) : __builtin_nanf("");
        a.st.best_t[idx] = qnan; a.st.lo[idx] = qnan; a.st.hi[idx] = qnan;
        return;
    }
    double m = a.t0;                                          // a column the scan gave up probes node 0: a valid input for forwards that are ignored
    if (ok) {
        const int32_t kb = a.st.best_k[idx];
        const int32_t klo = kb - 1 < 0 ? 0 : kb - 1, khi = kb + 1 > a.K ? a.K : kb + 1;
        m = a.t0 + (double)kb * a.dt;
        a.st.lo[idx] = a.t0 + (double)klo * a.dt;
        a.st.hi[idx] = a.t0 + (double)khi * a.dt;
        a.st.best_t[idx] = m;
    } else {
        a.st.best_v[idx] = __builtin_nanf("");
        a.st.best_t[idx] = qnan; a.st.lo[idx] = qnan; a.st.hi[idx] = qnan;
    }
    sample_point(a.s, a.cube, a.xr[i], a.yr[i], m, (int64_t)a.refined_of[c] * a.n + i, a.x, a.y, a.t, a.f, a.coord_data);
}

__global__ __launch_bounds__(THREADS) void dpn_extreme_refine_kernel(ExtArgs a) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;        // the probe: row p of out_n, jac_n and of the sampler outputs
    if (p >= a.n * a.n_refined) return;
    const int64_t r = p / a.n, i = p - r * a.n;
    const int32_t c = a.column_of[r];
    const int64_t idx = (int64_t)c * a.n + i;
    if (a.st.status[idx] != DPN_EXT_OK) return;
    double lo = a.st.lo[idx], hi = a.st.hi[idx];
    const int32_t kb = a.st.best_k[idx];
    const double m = a.round == 0 ? a.t0 + (double)kb * a.dt : lo + 0.5 * (hi - lo);      // the hour this probe was written at
    float g, s;
    ext_product<true>(a.out_n, a.jac_n, a.ph, p, a.id[c], g, s);
    if (!(__builtin_isfinite(g) && __builtin_isfinite(s))) { a.st.status[idx] = DPN_EXT_STOPPED; return; }      // the best so far stands
    const bool is_max = a.sense[c] == DPN_EXT_MAX;
    const float best = a.st.best_v[idx];
    if (is_max ? g > best : g < best) {
        a.st.best_v[idx] = g;
        a.st.best_t[idx] = m;
    }
    if (is_max ? s > 0.f : s < 0.f) { lo = m; a.st.lo[idx] = m; }         // the extreme lies later
    else                            { hi = m; a.st.hi[idx] = m; }
    if (lo == hi) {                                           // on a face of the window, the slope pointing outward
        a.st.status[idx] = kb == 0 ? DPN_EXT_AT_START : DPN_EXT_AT_END;
        return;
    }
    sample_point(a.s, a.cube, a.xr[i], a.yr[i], lo + 0.5 * (hi - lo), p, a.x, a.y, a.t, a.f, a.coord_data);
}

// the clock of a time-window request (extremes here, spells in dpn_spell.inc): n points, 1..max_columns columns, K >= 1 steps of dt > 0 from t0
bool window_clock_ok(int64_t n, int n_columns, int max_columns, int K, double t0, double dt) {
    if (n <= 0 || K < 1 || n_columns < 1 || n_columns > max_columns) return false;
    return t0 - t0 == 0.0 && dt - dt == 0.0 && dt > 0.0;      // (a NaN or an infinity fails the first two)
}

// the checks the scan, begin and refine entry points of both time-window products share -- the pointers, the clock, the sampler's dimensions, the
// product ids (25 or 28..33) --, and what they all fill of `a` (an ExtArgs or a SpellArgs).  false: refuse.
template <class Args>
bool window_request(Args& a, int max_columns, const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, int64_t n,
                    const int32_t* products, int n_columns, int K, double t0, double dt, const double* xr, const double* yr, float* x, float* y,
                    float* t, float* f, float* coord_data) {
    if (!s || !cube || !phys || !products || !xr || !yr || !x || !y || !t || !f || !coord_data) return false;
    if (!window_clock_ok(n, n_columns, max_columns, K, t0, dt)) return false;
    if (s->lon_in < 2 || s->lat_in < 2 || s->t_in < 2) return false;
    a.s = *s; a.cube = cube; a.ph = *phys; a.n = n; a.n_columns = n_columns; a.K = K; a.t0 = t0; a.dt = dt; a.xr = xr; a.yr = yr;
    a.x = x; a.y = y; a.t = t; a.f = f; a.coord_data = coord_data;
    for (int c = 0; c < n_columns; ++c) {
        if (!(products[c] == 25 || (products[c] >= 28 && products[c] <= 33))) return false;
        a.id[c] = products[c];
    }
    if (!with_clip)
        for (int k = 0; k < 6; ++k) a.ph.clip_on[k] = 0;      // the body then neither clips nor masks
    return true;
}

// the checks the three entry points share; fills the column tables of `a`.  false: refuse.
bool ext_request(ExtArgs& a, const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, int64_t n, const int32_t* products,
                 const int32_t* senses, int n_columns, int K, double t0, double dt, const double* xr, const double* yr, const DpnExtremeState* st,
                 float* x, float* y, float* t, float* f, float* coord_data) {
    if (!senses || !st || !st->best_v || !st->best_t || !st->best_k || !st->acc || !st->status || !st->lo || !st->hi) return false;
    if (!window_request(a, DPN_EXT_MAX_COLUMNS, s, cube, phys, with_clip, n, products, n_columns, K, t0, dt, xr, yr, x, y, t, f, coord_data)) return false;
    a.st = *st;
    a.n_refined = 0;
    for (int c = 0; c < n_columns; ++c) {
        if (senses[c] != DPN_EXT_MAX && senses[c] != DPN_EXT_MIN && senses[c] != DPN_EXT_MEAN) return false;
        a.sense[c] = senses[c];
        a.refined_of[c] = -1;
        if (senses[c] != DPN_EXT_MEAN) { a.refined_of[c] = a.n_refined; a.column_of[a.n_refined++] = c; }
    }
    return true;
}

inline dim3 ext_grid(const int64_t threads) { return dim3((unsigned)((threads + THREADS - 1) / THREADS)); }

}  // namespace

extern "C" {

int dpn_extreme_scan(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n,
                     const int32_t* products, const int32_t* senses, int n_columns, int k, int K, double t0, double dt, const double* xr, const double* yr,
                     const DpnExtremeState* st, float* x, float* y, float* t, float* f, float* coord_data, void* stream) {
    ExtArgs a{};
    if (!out_n || !ext_request(a, s, cube, phys, with_clip, n, products, senses, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data)) return -1;
    if (k < 0 || k > K) return -1;
    a.out_n = out_n; a.k = k;
    hipLaunchKernelGGL(dpn_extreme_scan_kernel, ext_grid(n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_extreme_begin(const DpnSampler* s, const float* cube, int64_t n, const int32_t* products, const int32_t* senses, int n_columns, int K, double t0,
                      double dt, const double* xr, const double* yr, const DpnExtremeState* st, float* x, float* y, float* t, float* f, float* coord_data,
                      void* stream) {
    ExtArgs a{};
    const DpnPhysics none{};
    if (!ext_request(a, s, cube, &none, 0, n, products, senses, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data)) return -1;
    hipLaunchKernelGGL(dpn_extreme_begin_kernel, ext_grid(n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_extreme_refine(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, const float* jac_n, int64_t n,
                       const int32_t* products, const int32_t* senses, int n_columns, int round, int K, double t0, double dt, const double* xr,
                       const double* yr, const DpnExtremeState* st, float* x, float* y, float* t, float* f, float* coord_data, void* stream) {
    ExtArgs a{};
    if (!out_n || !jac_n || !ext_request(a, s, cube, phys, with_clip, n, products, senses, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data))
        return -1;
    if (round < 0 || a.n_refined < 1) return -1;
    a.out_n = out_n; a.jac_n = jac_n; a.round = round;
    hipLaunchKernelGGL(dpn_extreme_refine_kernel, ext_grid(n * a.n_refined), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
