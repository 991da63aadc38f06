// Neighbourhood verification on lattices against gridded analyses (DESIGN.md section 6b.8), included by dpn_diag.hip behind dpn_pverify.inc: the
// fractions skill score of the forecast (out_n) and of the baseline (coord_data) against an analysis on the lattice's own nodes, over windows of
// growing width.  The values, the event test and the host checks are those of dpn_verify.inc (verify_values / verify_pick / verify_event,
// verify_*_ok, verify_clip).  include/dpn_hip.h states the layouts and every operation's order.
//   dpn_nbhd_stage  : ONE case's chunk at points first .. first + n of the lattice -> the mask bytes of those nodes for all E thresholds, one thread
//                     per point, plain byte stores that run along ix.
//   dpn_nbhd_fold   : planes p0 .. p0 + np of a fully staged case, four launches on one stream:
//                       rows    one wave per (plane, row): the four counts of a node from its mask byte, a wave-level inclusive scan by shuffles,
//                               the carry of the four counts handed from one 64-node segment to the next; one 16-byte store per node;
//                       columns one lane per (column, count) walks the rows, so a wave's loads and stores run along x;
//                       windows one wave per (plane, row), the K scales looped inside: four 16-byte corners per node and scale, neighbouring lanes
//                               read neighbouring corners; 64 strided left folds, then lane 0 folds the lane results in lane order;
//                       total   one wave per (plane, scale) folds the rows the same way and adds the case's total to the resident state.
//   dpn_nbhd_finish : a state -> the tables per hour and over all hours.
// All are compiled without contraction: every fp64 operation is rounded on its own, so the numpy restatement (deepphysinet_amd/neighbourhood.py)
// reproduces them bit for bit.  No atomics, no LDS, plain per-lane vector stores.

namespace {

constexpr int NB_SUMS = 5;                                    // sum_fo2, sum_f2, sum_o2, sum_bo2, sum_b2

struct NbStageArgs {
    const float *out_n, *coord_data, *analysis;
    int64_t n, first, plane;                                  // plane = nx * ny
    DpnPhysics ph;
    int32_t n_products, n_thr;
    int32_t id[DPN_VERIFY_MAX_COLUMNS];
    int32_t thr_col[DPN_VERIFY_MAX_THRESHOLDS];
    float thr_val[DPN_VERIFY_MAX_THRESHOLDS];
    int32_t thr_side[DPN_VERIFY_MAX_THRESHOLDS];
    uint8_t* mask;
};

__global__ __launch_bounds__(THREADS) void dpn_nbhd_stage_kernel(NbStageArgs a) {
#pragma clang fp contract(off)
    const int64_t ic = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (ic >= a.n) return;
    const VerValues fc = verify_values(a.out_n, a.ph, ic), bs = verify_values(a.coord_data, a.ph, ic);
    const int64_t g = a.first + ic, it = g / a.plane, r = g - it * a.plane;
    for (int e = 0; e < a.n_thr; ++e) {                       // thresholds and selectors are uniform: scalar branches
        const int j = a.thr_col[e];
        const float x = verify_pick(fc, a.id[j]), b = verify_pick(bs, a.id[j]), o = a.analysis[(it * a.n_products + j) * a.plane + r];
        const bool valid = __builtin_isfinite(x) && __builtin_isfinite(b) && __builtin_isfinite(o);
        const float thr = a.thr_val[e];
        const int side = a.thr_side[e];
        const unsigned m = !valid ? 0u : ((verify_event(x, thr, side) ? 1u : 0u) | (verify_event(b, thr, side) ? 2u : 0u) |
                                          (verify_event(o, thr, side) ? 4u : 0u) | 8u);
        a.mask[(it * a.n_thr + e) * a.plane + r] = (uint8_t)m;
    }
}

// The scratch of np planes: the tables, then the row partials (include/dpn_hip.h: the scratch of dpn_nbhd_fold).
struct NbScratch {
    int4* S;                                                  // [np][ny + 1][nx + 1], the four counts f, b, o, valid of a node in x, y, z, w
    double* part;                                             // [np][K][ny][NB_SUMS]
    int32_t* rows_n;                                          // [np][K][ny]
};

struct NbFoldArgs {
    const uint8_t* mask;
    NbScratch s;
    int32_t nx, ny, K;
    int64_t p0, np;
    int32_t radius[DPN_NBHD_MAX_SCALES];
    DpnNbhdState st;
};

__device__ __forceinline__ int4 nb_add(const int4 a, const int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// One 64-thread block = one wave = one (plane, row iy): the inclusive prefix along x of the four counts into row iy + 1 of the table; the wave of
// row 0 also writes the zero row.  The column pass turns the row prefixes into the table.
__global__ __launch_bounds__(64) void dpn_nbhd_rows_kernel(NbFoldArgs a) {
    const int64_t w = blockIdx.x, pl = w / a.ny;
    const int iy = (int)(w - pl * a.ny), lane = threadIdx.x;
    const int64_t nx1 = a.nx + 1;
    const uint8_t* src = a.mask + ((a.p0 + pl) * a.ny + iy) * (int64_t)a.nx;
    int4* table = a.s.S + pl * (a.ny + 1) * nx1;
    int4* dst = table + (iy + 1) * nx1;
    const int4 zero = make_int4(0, 0, 0, 0);
    if (iy == 0)
        for (int64_t x = lane; x < nx1; x += 64) table[x] = zero;
    if (lane == 0) dst[0] = zero;
    int4 carry = zero;
    for (int x0 = 0; x0 < a.nx; x0 += 64) {                   // (uniform: every lane takes part in the shuffles of every segment)
        const int ix = x0 + lane;
        const unsigned m = ix < a.nx ? src[ix] : 0u;
        int4 v = make_int4((int)(m & 1u), (int)((m >> 1) & 1u), (int)((m >> 2) & 1u), (int)((m >> 3) & 1u));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int4 up = make_int4(__shfl_up(v.x, off, 64), __shfl_up(v.y, off, 64), __shfl_up(v.z, off, 64), __shfl_up(v.w, off, 64));
            if (lane >= off) v = nb_add(v, up);
        }
        v = nb_add(v, carry);
        if (ix < a.nx) dst[ix + 1] = v;
        carry = make_int4(__shfl(v.x, 63, 64), __shfl(v.y, 63, 64), __shfl(v.z, 63, 64), __shfl(v.w, 63, 64));
    }
}

// One lane per (column, count) of a plane: int32 place c of a table row, c in 0 .. 4 (nx + 1) - 1, summed down the rows 1 .. ny.
__global__ __launch_bounds__(THREADS) void dpn_nbhd_cols_kernel(NbFoldArgs a) {
    const int64_t row = 4 * ((int64_t)a.nx + 1), blocks = (row + THREADS - 1) / THREADS, pl = blockIdx.x / blocks;
    const int64_t c = (blockIdx.x - pl * blocks) * THREADS + threadIdx.x;
    if (c >= row) return;
    int32_t* t = reinterpret_cast<int32_t*>(a.s.S) + pl * (a.ny + 1) * row + c;
    int32_t acc = 0;
    for (int iy = 1; iy <= a.ny; ++iy) {
        acc += t[iy * row];
        t[iy * row] = acc;
    }
}

struct NbCell {
    double s[NB_SUMS];
    int32_t n;
};

// One 64-thread block = one wave = one (plane, row iy), the scales looped inside.
__global__ __launch_bounds__(64) void dpn_nbhd_windows_kernel(NbFoldArgs a) {
#pragma clang fp contract(off)
    const int64_t w = blockIdx.x, pl = w / a.ny;
    const int iy = (int)(w - pl * a.ny), lane = threadIdx.x;
    const int64_t nx1 = a.nx + 1;
    const int4* S = a.s.S + pl * (a.ny + 1) * nx1;
    for (int k = 0; k < a.K; ++k) {
        const int r = a.radius[k];
        const int y0 = iy - r > 0 ? iy - r : 0, y1 = iy + 1 < a.ny - r ? iy + r + 1 : a.ny;        // (no sum that could leave int32)
        const int4 *top = S + y0 * nx1, *bot = S + y1 * nx1;
        NbCell acc{};
        for (int ix = lane; ix < a.nx; ix += 64) {
            const int x0 = ix - r > 0 ? ix - r : 0, x1 = ix + 1 < a.nx - r ? ix + r + 1 : a.nx;
            const int4 c11 = bot[x1], c01 = top[x1], c10 = bot[x0], c00 = top[x0];
            const int cf = c11.x - c01.x - c10.x + c00.x, cb = c11.y - c01.y - c10.y + c00.y, co = c11.z - c01.z - c10.z + c00.z,
                      cv = c11.w - c01.w - c10.w + c00.w;
            if (cv == 0) continue;
            const double V = (double)cv, Pf = (double)cf / V, Pb = (double)cb / V, Po = (double)co / V;
            const double d = Pf - Po, g = Pb - Po;
            acc.s[0] = acc.s[0] + d * d;
            acc.s[1] = acc.s[1] + Pf * Pf;
            acc.s[2] = acc.s[2] + Po * Po;
            acc.s[3] = acc.s[3] + g * g;
            acc.s[4] = acc.s[4] + Pb * Pb;
            acc.n += 1;
        }
        NbCell all = acc;                                     // lane 0's: the fold of the 64 lane results in lane order
        for (int l = 1; l < 64; ++l) {
#pragma unroll
            for (int q = 0; q < NB_SUMS; ++q) all.s[q] = all.s[q] + __shfl(acc.s[q], l, 64);
            all.n += __shfl(acc.n, l, 64);
        }
        if (lane == 0) {
            const int64_t at = (pl * a.K + k) * a.ny + iy;
#pragma unroll
            for (int q = 0; q < NB_SUMS; ++q) a.s.part[at * NB_SUMS + q] = all.s[q];
            a.s.rows_n[at] = all.n;
        }
    }
}

// One 64-thread block = one wave = one (plane, scale): the rows folded as the nodes of a row were, then the case's total into the state.
__global__ __launch_bounds__(64) void dpn_nbhd_total_kernel(NbFoldArgs a) {
#pragma clang fp contract(off)
    const int64_t w = blockIdx.x, pl = w / a.K;
    const int k = (int)(w - pl * a.K), lane = threadIdx.x;
    const int64_t base = (pl * a.K + k) * a.ny;
    double s[NB_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t n = 0;
    for (int iy = lane; iy < a.ny; iy += 64) {
#pragma unroll
        for (int q = 0; q < NB_SUMS; ++q) s[q] = s[q] + a.s.part[(base + iy) * NB_SUMS + q];
        n += a.s.rows_n[base + iy];
    }
    double all[NB_SUMS];
#pragma unroll
    for (int q = 0; q < NB_SUMS; ++q) all[q] = s[q];
    int64_t all_n = n;
    for (int l = 1; l < 64; ++l) {
#pragma unroll
        for (int q = 0; q < NB_SUMS; ++q) all[q] = all[q] + __shfl(s[q], l, 64);
        all_n += __shfl(n, l, 64);
    }
    if (lane != 0) return;
    const int64_t plane = a.p0 + pl, at = plane * a.K + k;
    const DpnNbhdState& t = a.st;
    t.sum_fo2[at] = t.sum_fo2[at] + all[0];
    t.sum_f2[at] = t.sum_f2[at] + all[1];
    t.sum_o2[at] = t.sum_o2[at] + all[2];
    t.sum_bo2[at] = t.sum_bo2[at] + all[3];
    t.sum_b2[at] = t.sum_b2[at] + all[4];
    t.windows[at] += all_n;
    if (k == 0) {                                             // the plane totals, once per plane
        const int4 c = a.s.S[(pl + 1) * (a.ny + 1) * ((int64_t)a.nx + 1) - 1];
        t.n_f[plane] += c.x;
        t.n_b[plane] += c.y;
        t.n_o[plane] += c.z;
        t.n_valid[plane] += c.w;
    }
}

struct NbFinishArgs {
    DpnNbhdState st;
    int32_t nt, E, K;
    DpnNbhdOut hour, all;
};

// Thread i < nt * E: the (hour, threshold) entry i of the hour tables; nt * E <= i < (nt + 1) * E: threshold i - nt * E of the tables over all hours.
__global__ __launch_bounds__(THREADS) void dpn_nbhd_finish_kernel(NbFinishArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x, hours = (int64_t)a.nt * a.E;
    if (i >= hours + a.E) return;
    const bool pooled = i >= hours;
    const int64_t o = pooled ? i - hours : i;
    const int64_t lo = pooled ? o : i, step = a.E, count = pooled ? a.nt : 1;       // the state entries lo, lo + step, ..: it ascending
    const DpnNbhdState& t = a.st;
    const DpnNbhdOut& out = pooled ? a.all : a.hour;
    const float nan = __builtin_nanf("");
    int64_t nv = 0, nf = 0, nb = 0, no = 0;
    for (int64_t c = 0; c < count; ++c) {
        const int64_t s = lo + c * step;
        nv += t.n_valid[s]; nf += t.n_f[s]; nb += t.n_b[s]; no += t.n_o[s];
    }
    const double V = (double)nv, F = (double)nf, B = (double)nb, O = (double)no;
    const double freq_o = O / V, useful = 0.5 + freq_o * 0.5;
    out.count[o] = nv;
    out.freq_f[o] = nv != 0 ? (float)(F / V) : nan;
    out.freq_b[o] = nv != 0 ? (float)(B / V) : nan;
    out.freq_o[o] = nv != 0 ? (float)freq_o : nan;
    out.fbias[o] = no != 0 ? (float)(F / O) : nan;
    out.base_fbias[o] = no != 0 ? (float)(B / O) : nan;
    out.useful[o] = nv != 0 ? (float)useful : nan;
    int32_t first = -1, base_first = -1;
    for (int k = 0; k < a.K; ++k) {
        double fo2 = 0.0, f2 = 0.0, o2 = 0.0, bo2 = 0.0, b2 = 0.0;
        int64_t wn = 0;
        for (int64_t c = 0; c < count; ++c) {
            const int64_t s = (lo + c * step) * a.K + k;
            fo2 = fo2 + t.sum_fo2[s]; f2 = f2 + t.sum_f2[s]; o2 = o2 + t.sum_o2[s]; bo2 = bo2 + t.sum_bo2[s]; b2 = b2 + t.sum_b2[s];
            wn += t.windows[s];
        }
        const double den = f2 + o2, base_den = b2 + o2;
        const double fss = 1.0 - fo2 / den, base_fss = 1.0 - bo2 / base_den;
        out.fss[o * a.K + k] = den != 0.0 ? (float)fss : nan;
        out.base_fss[o * a.K + k] = base_den != 0.0 ? (float)base_fss : nan;
        out.windows[o * a.K + k] = wn;
        if (nv != 0 && den != 0.0 && first < 0 && fss >= useful) first = k;
        if (nv != 0 && base_den != 0.0 && base_first < 0 && base_fss >= useful) base_first = k;
    }
    out.skilful_scale[o] = first;
    out.base_skilful_scale[o] = base_first;
}

bool nbhd_lattice_ok(const DpnLattice* lat) {
    if (!lat || lat->nx < 1 || lat->ny < 1 || lat->nt < 1) return false;
    return (int64_t)lat->nx * lat->ny < ((int64_t)1 << 31) && (int64_t)lat->nx * lat->ny * lat->nt < ((int64_t)1 << 31);
}

bool nbhd_scales_ok(const int32_t* radius, const int n_scales) {
    if (!radius || n_scales < 1 || n_scales > DPN_NBHD_MAX_SCALES) return false;
    for (int k = 0; k < n_scales; ++k)
        if (radius[k] < 0 || (k > 0 && radius[k] <= radius[k - 1])) return false;
    return true;
}

bool nbhd_state_ok(const DpnNbhdState* s) {
    return s && s->sum_fo2 && s->sum_f2 && s->sum_o2 && s->sum_bo2 && s->sum_b2 && s->windows && s->n_valid && s->n_f && s->n_b && s->n_o;
}

bool nbhd_out_ok(const DpnNbhdOut* r) {
    return r && r->fss && r->base_fss && r->windows && r->freq_f && r->freq_b && r->freq_o && r->fbias && r->base_fbias && r->useful && r->count &&
           r->skilful_scale && r->base_skilful_scale;
}

}  // namespace

extern "C" {

int dpn_nbhd_stage(const float* out_n, const float* coord_data, const float* analysis, int64_t n, const DpnPhysics* phys, int with_clip,
                   const int32_t* products, int n_products, const int32_t* thr_col, const float* thr_val, const int32_t* thr_side, int n_thr,
                   const DpnLattice* lattice, int64_t first, uint8_t* mask, void* stream) {
    if (!out_n || !coord_data || !analysis || !phys || !products || !mask || !nbhd_lattice_ok(lattice)) return -1;
    const int64_t plane = (int64_t)lattice->nx * lattice->ny;
    if (!verify_range_ok(n, first, plane * lattice->nt)) return -1;
    if (n_thr < 1 || !verify_sizes_ok(n_products, n_thr, thr_col)) return -1;
    NbStageArgs a{out_n, coord_data, analysis, n, first, plane, *phys, n_products, n_thr, {}, {}, {}, {}, mask};
    if (!verify_ids_ok(products, n_products, a.id) || !verify_thresholds_ok(thr_col, thr_val, thr_side, n_thr, a.thr_col, a.thr_val, a.thr_side)) return -1;
    verify_clip(a.ph, with_clip);
    hipLaunchKernelGGL(dpn_nbhd_stage_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_nbhd_fold(const uint8_t* mask, const DpnLattice* lattice, int n_thr, const int32_t* radius, int n_scales, int64_t p0, int64_t np,
                  void* scratch, const DpnNbhdState* state, void* stream) {
    if (!mask || !scratch || !nbhd_lattice_ok(lattice) || !nbhd_state_ok(state)) return -1;
    if (n_thr < 1 || n_thr > DPN_VERIFY_MAX_THRESHOLDS || !nbhd_scales_ok(radius, n_scales)) return -1;
    const int64_t planes = (int64_t)lattice->nt * n_thr;
    if (p0 < 0 || np <= 0 || p0 > planes - np) return -1;
    const int32_t nx = lattice->nx, ny = lattice->ny;
    const int64_t table = ((int64_t)nx + 1) * ((int64_t)ny + 1);
    const int64_t col_blocks = (4 * ((int64_t)nx + 1) + THREADS - 1) / THREADS;
    if (np * ny > 0x7fffffff || np * col_blocks > 0x7fffffff) return -1;  // one block per (plane, row), and per (plane, 64 columns)
    NbFoldArgs a{mask, {}, nx, ny, n_scales, p0, np, {}, *state};
    a.s.S = static_cast<int4*>(scratch);
    a.s.part = reinterpret_cast<double*>(a.s.S + np * table);
    a.s.rows_n = reinterpret_cast<int32_t*>(a.s.part + np * n_scales * ny * NB_SUMS);
    for (int k = 0; k < n_scales; ++k) a.radius[k] = radius[k];
    hipStream_t q = (hipStream_t)stream;
    hipLaunchKernelGGL(dpn_nbhd_rows_kernel, dim3((unsigned)(np * ny)), dim3(64), 0, q, a);
    hipLaunchKernelGGL(dpn_nbhd_cols_kernel, dim3((unsigned)(np * col_blocks)), dim3(THREADS), 0, q, a);
    hipLaunchKernelGGL(dpn_nbhd_windows_kernel, dim3((unsigned)(np * ny)), dim3(64), 0, q, a);
    hipLaunchKernelGGL(dpn_nbhd_total_kernel, dim3((unsigned)(np * n_scales)), dim3(64), 0, q, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_nbhd_finish(const DpnNbhdState* state, int nt, int n_thr, int n_scales, const DpnNbhdOut* hour, const DpnNbhdOut* all, void* stream) {
    if (!nbhd_state_ok(state) || !nbhd_out_ok(hour) || !nbhd_out_ok(all)) return -1;
    if (nt < 1 || n_thr < 1 || n_thr > DPN_VERIFY_MAX_THRESHOLDS || n_scales < 1 || n_scales > DPN_NBHD_MAX_SCALES) return -1;
    NbFinishArgs a{*state, nt, n_thr, n_scales, *hour, *all};
    const int64_t threads = ((int64_t)nt + 1) * n_thr;
    hipLaunchKernelGGL(dpn_nbhd_finish_kernel, dim3((unsigned)((threads + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
