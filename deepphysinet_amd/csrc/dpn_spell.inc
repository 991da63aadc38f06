// Threshold spells in time (DESIGN.md section 6b.4), included by dpn_diag.hip behind dpn_extreme.inc: how long a product stays above (below) a threshold
// in a window of hours, from when until when.  The same coarse scan as the window extremes, then bisection on the sign of value - threshold in the scan
// steps of the first entry and of the last exit.  include/dpn_hip.h states the state's layout and every operation's order.
//   dpn_spell_scan   : scan node k's fields-only forward folded into the state (the clipped trapezoid of the margin, the crossings, the first and the
//                      last node that is in), and the sampler at node k + 1 written where the next forward reads it.
//   dpn_spell_begin  : the scan's close: the entry and the exit bracket of every column and their first probes.
//   dpn_spell_refine : one round: the probes' values from the fields-only forward, the halved brackets, the next probes.
//   dpn_spell_finish : the scan's interpolated ends of the spell replaced by the refined ones in `hours`.
// One thread per (column, point) -- refine: per probe --, 256-thread blocks; the state is column-major ([column][point]), so a wave runs along the
// points.  Compiled without contraction: every fp32 and fp64 operation is rounded on its own, and the numpy restatement (deepphysinet_amd/spells.py)
// reproduces them bit for bit.  No atomics, no LDS, plain per-lane stores.  ext_product (dpn_extreme.inc) forms the products, sample_point
// (dpn_sample_point.h) the forward's inputs.

namespace {

struct SpellArgs {
    DpnSampler s;
    const float* cube;
    DpnPhysics ph;
    const float* out_n;
    int64_t n;
    int32_t n_columns, k, K;
    double t0, dt;
    const double *xr, *yr;
    int32_t id[DPN_SPELL_MAX_COLUMNS], side[DPN_SPELL_MAX_COLUMNS];
    float thr[DPN_SPELL_MAX_COLUMNS];
    DpnSpellState st;
    float *x, *y, *t, *f, *coord_data;
};

// the margin of x: > 0 exactly where x is in (both casts and the difference of two floats are exact in fp64 up to one rounding; the negation is exact)
__device__ __forceinline__ double spell_margin(const float x, const float thr, const int32_t side) {
#pragma clang fp contract(off)
    const double d = (double)x - (double)thr;
    return side == DPN_SPELL_BELOW ? -d : d;
}

__device__ __forceinline__ bool spell_in(const float x, const float thr, const int32_t side) { return side == DPN_SPELL_BELOW ? x < thr : x > thr; }

__device__ __forceinline__ double spell_hour(const SpellArgs& a, const int32_t k) {
#pragma clang fp contract(off)
    return a.t0 + (double)k * a.dt;
}

__global__ __launch_bounds__(THREADS) void dpn_spell_scan_kernel(SpellArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.n * a.n_columns) return;
    const int64_t c = idx / a.n, i = idx - c * a.n;           // idx is the state's place [c][i]
    if (c == 0 && a.k < a.K)                                  // the next node's forward reads these; whatever the columns' status
        sample_point(a.s, a.cube, a.xr[i], a.yr[i], a.t0 + (double)(a.k + 1) * a.dt, i, a.x, a.y, a.t, a.f, a.coord_data);
    float x, s;
    ext_product<false>(a.out_n, nullptr, a.ph, i, a.id[c], x, s);
    if (a.k > 0 && a.st.status[idx] != 0) return;             // sticky (only BAD_SCAN is set before begin)
    if (!__builtin_isfinite(x)) { a.st.status[idx] = DPN_SPELL_BAD_SCAN; return; }
    const float thr = a.thr[c];
    const int32_t side = a.side[c];
    if (a.k == 0) {
        const int32_t at = spell_in(x, thr, side) ? 0 : -1;
        a.st.status[idx] = 0;
        a.st.hours[idx] = 0.0; a.st.excess[idx] = 0.0; a.st.crossings[idx] = 0;
        a.st.part_first[idx] = 0.0; a.st.part_last[idx] = 0.0;
        a.st.k_first[idx] = at; a.st.k_last[idx] = at;
        a.st.prev_x[idx] = x;
        return;
    }
    const double p = spell_margin(a.st.prev_x[idx], thr, side), q = spell_margin(x, thr, side);      // a and b of the header's table
    a.st.prev_x[idx] = x;
    if (p > 0.0 && q > 0.0) {                                 // both in
        a.st.hours[idx] = a.st.hours[idx] + a.dt;
        a.st.excess[idx] = a.st.excess[idx] + 0.5 * (p + q) * a.dt;
        a.st.k_last[idx] = a.k;
        a.st.part_last[idx] = 0.0;
    } else if (q > 0.0) {                                     // entry: p <= 0 < q
        const double w = q / (q - p) * a.dt;
        a.st.hours[idx] = a.st.hours[idx] + w;
        a.st.excess[idx] = a.st.excess[idx] + 0.5 * q * w;
        a.st.crossings[idx] = a.st.crossings[idx] + 1;
        a.st.k_last[idx] = a.k;
        a.st.part_last[idx] = 0.0;
        if (a.st.k_first[idx] < 0) { a.st.k_first[idx] = a.k; a.st.part_first[idx] = w; }
    } else if (p > 0.0) {                                     // exit: q <= 0 < p; k_last stays k - 1
        const double w = p / (p - q) * a.dt;
        a.st.hours[idx] = a.st.hours[idx] + w;
        a.st.excess[idx] = a.st.excess[idx] + 0.5 * p * w;
        a.st.crossings[idx] = a.st.crossings[idx] + 1;
        a.st.part_last[idx] = w;
    }
}

__global__ __launch_bounds__(THREADS) void dpn_spell_begin_kernel(SpellArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.n * a.n_columns) return;
    const int64_t c = idx / a.n, i = idx - c * a.n;
    const double qnan = __builtin_nan("");
    int32_t status = a.st.status[idx];
    double f_lo = qnan, f_hi = qnan, l_lo = qnan, l_hi = qnan;
    double m_entry = a.t0, m_exit = a.t0;                     // a probe without a bracket sits at node 0: a valid input for forwards that are ignored
    if (status & DPN_SPELL_BAD_SCAN) {
        a.st.hours[idx] = qnan; a.st.excess[idx] = qnan;
    } else {
        const int32_t kf = a.st.k_first[idx], kl = a.st.k_last[idx];
        if (kf < 0) {
            status |= DPN_SPELL_NEVER;
        } else {
            if (kf >= 1) {
                f_lo = spell_hour(a, kf - 1); f_hi = spell_hour(a, kf);
                m_entry = f_lo + 0.5 * (f_hi - f_lo);
            } else {
                f_lo = a.t0; f_hi = a.t0;
                status |= DPN_SPELL_HOLDS_AT_START;
            }
            if (kl < a.K) {
                l_lo = spell_hour(a, kl); l_hi = spell_hour(a, kl + 1);
                m_exit = l_lo + 0.5 * (l_hi - l_lo);
            } else {
                l_lo = spell_hour(a, a.K); l_hi = l_lo;
                status |= DPN_SPELL_HOLDS_AT_END;
            }
        }
        a.st.status[idx] = status;
    }
    a.st.f_lo[idx] = f_lo; a.st.f_hi[idx] = f_hi; a.st.l_lo[idx] = l_lo; a.st.l_hi[idx] = l_hi;
    sample_point(a.s, a.cube, a.xr[i], a.yr[i], m_entry, (2 * c) * a.n + i, a.x, a.y, a.t, a.f, a.coord_data);
    sample_point(a.s, a.cube, a.xr[i], a.yr[i], m_exit, (2 * c + 1) * a.n + i, a.x, a.y, a.t, a.f, a.coord_data);
}

__global__ __launch_bounds__(THREADS) void dpn_spell_refine_kernel(SpellArgs a) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;        // the probe: row p of out_n and of the sampler outputs
    if (p >= 2 * a.n * a.n_columns) return;
    const int64_t r = p / a.n, i = p - r * a.n;
    const int32_t c = (int32_t)(r >> 1), e = (int32_t)(r & 1);
    const int64_t idx = (int64_t)c * a.n + i;
    const int32_t status = a.st.status[idx];
    if (status & (DPN_SPELL_BAD_SCAN | DPN_SPELL_STOPPED | DPN_SPELL_NEVER)) return;
    const bool has_entry = a.st.k_first[idx] >= 1, has_exit = a.st.k_last[idx] < a.K;
    if (e == 0 ? !has_entry : !has_exit) return;
    // The column's two probes belong to two threads.  Each forms both values, so that both reach the same verdict on STOPPED whichever runs first:
    // the verdict moves no bracket, and a thread that reads the other's STOPPED would have stopped anyway.
    float g = 0.f, g_other = 0.f, s;
    ext_product<false>(a.out_n, nullptr, a.ph, p, a.id[c], g, s);
    const bool has_other = e == 0 ? has_exit : has_entry;
    if (has_other) ext_product<false>(a.out_n, nullptr, a.ph, (int64_t)(r ^ 1) * a.n + i, a.id[c], g_other, s);
    if (!__builtin_isfinite(g) || !__builtin_isfinite(g_other)) {
        if (e == 0 || !has_entry) a.st.status[idx] = status | DPN_SPELL_STOPPED;       // one writer; both brackets stand
        return;
    }
    double* const lo_p = e == 0 ? a.st.f_lo : a.st.l_lo;
    double* const hi_p = e == 0 ? a.st.f_hi : a.st.l_hi;
    double lo = lo_p[idx], hi = hi_p[idx];
    const double m = lo + 0.5 * (hi - lo);                    // the hour this probe was written at
    const bool in = spell_in(g, a.thr[c], a.side[c]);
    if (in == (e == 0)) { hi = m; hi_p[idx] = m; }            // entry: in -> f_hi = m; exit: out -> l_hi = m
    else                { lo = m; lo_p[idx] = m; }            // entry: out -> f_lo = m; exit: in -> l_lo = m
    sample_point(a.s, a.cube, a.xr[i], a.yr[i], lo + 0.5 * (hi - lo), p, a.x, a.y, a.t, a.f, a.coord_data);
}

__global__ __launch_bounds__(THREADS) void dpn_spell_finish_kernel(SpellArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= a.n * a.n_columns) return;
    const int32_t status = a.st.status[idx];
    if (status & DPN_SPELL_BAD_SCAN) return;                  // everything is NaN since begin
    if (status & DPN_SPELL_NEVER) { a.st.hours[idx] = 0.0; a.st.excess[idx] = 0.0; return; }
    const int32_t kf = a.st.k_first[idx], kl = a.st.k_last[idx];
    double h = a.st.hours[idx];
    if (kf >= 1) {
        h = h - a.st.part_first[idx];
        h = h + (spell_hour(a, kf) - a.st.f_hi[idx]);
    }
    if (kl < a.K) {
        h = h - a.st.part_last[idx];
        h = h + (a.st.l_lo[idx] - spell_hour(a, kl));
    }
    a.st.hours[idx] = h;
}

bool spell_state_ok(const DpnSpellState* st) {
    return st && st->prev_x && st->hours && st->excess && st->crossings && st->k_first && st->k_last && st->status && st->part_first && st->part_last &&
           st->f_lo && st->f_hi && st->l_lo && st->l_hi;
}

// the checks scan, begin and refine share (window_request: dpn_extreme.inc); fills the column tables of `a`.  false: refuse.
bool spell_request(SpellArgs& a, const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, int64_t n, const int32_t* products,
                   const int32_t* sides, const float* thr, int n_columns, int K, double t0, double dt, const double* xr, const double* yr,
                   const DpnSpellState* st, float* x, float* y, float* t, float* f, float* coord_data) {
    if (!sides || !thr || !spell_state_ok(st)) return false;
    if (!window_request(a, DPN_SPELL_MAX_COLUMNS, s, cube, phys, with_clip, n, products, n_columns, K, t0, dt, xr, yr, x, y, t, f, coord_data)) return false;
    a.st = *st;
    for (int c = 0; c < n_columns; ++c) {
        if (sides[c] != DPN_SPELL_ABOVE && sides[c] != DPN_SPELL_BELOW) return false;
        if (!(thr[c] - thr[c] == 0.f)) return false;
        a.side[c] = sides[c];
        a.thr[c] = thr[c];
    }
    return true;
}

}  // namespace

extern "C" {

int dpn_spell_scan(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n, const int32_t* products,
                   const int32_t* sides, const float* thr, int n_columns, int k, int K, double t0, double dt, const double* xr, const double* yr,
                   const DpnSpellState* st, float* x, float* y, float* t, float* f, float* coord_data, void* stream) {
    SpellArgs a{};
    if (!out_n || !spell_request(a, s, cube, phys, with_clip, n, products, sides, thr, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data)) return -1;
    if (k < 0 || k > K) return -1;
    a.out_n = out_n; a.k = k;
    hipLaunchKernelGGL(dpn_spell_scan_kernel, ext_grid(n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_spell_begin(const DpnSampler* s, const float* cube, int64_t n, const int32_t* products, const int32_t* sides, const float* thr, int n_columns,
                    int K, double t0, double dt, const double* xr, const double* yr, const DpnSpellState* st, float* x, float* y, float* t, float* f,
                    float* coord_data, void* stream) {
    SpellArgs a{};
    const DpnPhysics none{};
    if (!spell_request(a, s, cube, &none, 0, n, products, sides, thr, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data)) return -1;
    hipLaunchKernelGGL(dpn_spell_begin_kernel, ext_grid(n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_spell_refine(const DpnSampler* s, const float* cube, const DpnPhysics* phys, int with_clip, const float* out_n, int64_t n, const int32_t* products,
                     const int32_t* sides, const float* thr, int n_columns, int round, int K, double t0, double dt, const double* xr, const double* yr,
                     const DpnSpellState* st, float* x, float* y, float* t, float* f, float* coord_data, void* stream) {
    SpellArgs a{};
    if (!out_n || !spell_request(a, s, cube, phys, with_clip, n, products, sides, thr, n_columns, K, t0, dt, xr, yr, st, x, y, t, f, coord_data)) return -1;
    if (round < 0) return -1;
    a.out_n = out_n;
    hipLaunchKernelGGL(dpn_spell_refine_kernel, ext_grid(2 * n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_spell_finish(int64_t n, int n_columns, int K, double t0, double dt, const DpnSpellState* st, void* stream) {
    SpellArgs a{};
    if (!spell_state_ok(st) || !window_clock_ok(n, n_columns, DPN_SPELL_MAX_COLUMNS, K, t0, dt)) return -1;
    a.n = n; a.n_columns = n_columns; a.K = K; a.t0 = t0; a.dt = dt; a.st = *st;
    hipLaunchKernelGGL(dpn_spell_finish_kernel, ext_grid(n * n_columns), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
