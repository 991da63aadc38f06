// Collocation sampler + trilinear interpolation of the coarse forecast cube, and the full-grid de-normalise/scatter
// (SURVEY.md section 8 rows f1 / f3).  HBM-bound gather kernels: one thread per point, all index / weight arithmetic in
// fp64 exactly as the reference's numpy/xarray code does it (dataset/physics_dataset.py:334-338, 383-415, 442-446,
// 454-499, 521-526, 528-587), outputs cast to fp32 at the end like the reference's `.float()`.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dpn_hip.h"
#include "dpn_sample_point.h"      // sample_point, denorm (shared with dpn_traj.hip)

namespace {

// Philox-4x32-10 (Salmon et al. 2011), counter = (point index, stream id), key = seed.
__device__ inline void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ inline double u53(uint32_t hi, uint32_t lo) {               // uniform double in [0,1), 53 random bits (np.random.rand)
    return (double)((((uint64_t)hi << 21) ^ (uint64_t)(lo >> 11)) & ((1ull << 53) - 1)) * (1.0 / 9007199254740992.0);
}
__device__ inline uint32_t below(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }   // randint(0, n)

struct SampleArgs {
    DpnSampler s;
    const float* cube;
    const float* labels;
    const int32_t *xi, *yi, *ti;
    int64_t n;
    uint64_t seed, offset;
    const int32_t* step_dev;      // optional device-side step counter: the draw counter starts at offset + *step_dev * stride
    uint64_t stride;
    int mode;
    float *x, *y, *t, *f, *coord_data, *label_out;
    double* raw;
};

__global__ __launch_bounds__(256) void dpn_sample_kernel(SampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const DpnSampler& s = a.s;
    double xr, yr, tr;
    if (a.mode == DPN_SAMPLE_EXPLICIT) {
        xr = a.xi[i]; yr = a.yi[i]; tr = a.ti[i];
    } else {
        uint32_t w[4], v[4];
        const uint64_t ctr = a.offset + (a.step_dev ? (uint64_t)(uint32_t)(*a.step_dev) * a.stride : 0ull) + (uint64_t)i;
        philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
        philox4x32((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), v);
        if (a.mode == DPN_SAMPLE_INTERIOR) {                            // np.random.rand(n) * (size - 1)   (:442-443)
            xr = u53(w[0], w[1]) * (double)(s.lon - 1);
            yr = u53(w[2], w[3]) * (double)(s.lat - 1);
        } else {                                                        // np.random.randint(0, size)        (:334-335)
            xr = below(w[0], (uint32_t)s.lon);
            yr = below(w[2], (uint32_t)s.lat);
        }
        tr = below(v[0], (uint32_t)(s.t_hours + 1));                    // randint(0, step * nums + 1)       (:338, :446)
    }
    sample_point(s, a.cube, xr, yr, tr, i, a.x, a.y, a.t, a.f, a.coord_data);
    if (a.raw) { a.raw[i * 3] = xr; a.raw[i * 3 + 1] = yr; a.raw[i * 3 + 2] = tr; }
    if (a.labels && a.label_out) {                                      // read_point of the ERA5 label at (x, y, t)  (:347-365)
        const int X = (int)xr, Y = (int)yr, T = (int)tr;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            a.label_out[i * 6 + k] = a.labels[(((int64_t)T * 6 + k) * s.lat + Y) * s.lon + X];
    }
}

struct MapArgs {
    const float* out_n;
    int lon, lat;
    DpnPhysics ph;
    int with_clip;
    float* maps;
};
// out_n [lon*lat, 6] in the reference's node order (x outer, y inner; interface_physics.py:538-543) -> maps [6][lat][lon]
// de-normalised (inverse_norm, :232-262).  Reads are strided by node order, writes are coalesced along lon.
__global__ __launch_bounds__(256) void dpn_grid_maps_kernel(MapArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nodes = (int64_t)a.lon * a.lat;
    if (j >= nodes * 6) return;
    const int k = (int)(j / nodes);
    const int64_t r = j - k * nodes;
    const int yy = (int)(r / a.lon), xx = (int)(r - (int64_t)yy * a.lon);
    const float v = denorm(a.out_n[((int64_t)xx * a.lat + yy) * 6 + k], k, a.ph, a.with_clip);
    a.maps[j] = v;
}

// The point of a lattice with running index g: (it, iy, ix), ix fastest, it slowest.
__device__ __forceinline__ void lattice_index(const DpnLattice& l, const int64_t g, int& it, int& iy, int& ix) {
    const int64_t plane = (int64_t)l.nx * l.ny;
    it = (int)(g / plane);
    const int64_t r = g - (int64_t)it * plane;
    iy = (int)(r / l.nx);
    ix = (int)(r - (int64_t)iy * l.nx);
}

struct SampleAtArgs {
    DpnSampler s;
    const float* cube;
    const double *xr, *yr, *tr;      // stations (NULL: the lattice)
    DpnLattice lat;
    int64_t first, n;
    float *x, *y, *t, *f, *coord_data;
};
// The sampler at given positions: stations (three arrays) or points first .. first + n of a lattice built here (no index arrays).
__global__ __launch_bounds__(256) void dpn_sample_at_kernel(SampleAtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double xr, yr, tr;
    if (a.xr) {
        xr = a.xr[i]; yr = a.yr[i]; tr = a.tr[i];
    } else {
        int it, iy, ix;
        lattice_index(a.lat, a.first + i, it, iy, ix);
        {                                         // origin + index * step in two roundings, as a host forms the same positions
#pragma clang fp contract(off)
            xr = a.lat.x0 + (double)ix * a.lat.xstep;
            yr = a.lat.y0 + (double)iy * a.lat.ystep;
            tr = a.lat.t0 + (double)it * a.lat.tstep;
        }
    }
    sample_point(a.s, a.cube, xr, yr, tr, i, a.x, a.y, a.t, a.f, a.coord_data);
}

struct FieldsOutArgs {
    const float* out_n;
    int64_t n, first;
    DpnPhysics ph;
    int with_clip;
    float *rows, *maps;
    DpnLattice lat;
};
// out_n [n][6] normalised -> physical values (inverse_norm): rows [n][6], or the places of lattice points first .. first + n in
// maps [nt][6][ny][nx].  Map mode: thread j = (k, point), points fastest -> stores run along ix (a chunk may begin and end anywhere in a plane).
__global__ __launch_bounds__(256) void dpn_fields_out_kernel(FieldsOutArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n * 6) return;
    if (a.rows) {
        const int k = (int)(j % 6);
        a.rows[j] = denorm(a.out_n[j], k, a.ph, a.with_clip);
        return;
    }
    const int k = (int)(j / a.n);
    const int64_t p = j - (int64_t)k * a.n, g = a.first + p;
    const int64_t plane = (int64_t)a.lat.nx * a.lat.ny;
    const int64_t it = g / plane, r = g - it * plane;
    a.maps[(it * 6 + k) * plane + r] = denorm(a.out_n[p * 6 + k], k, a.ph, a.with_clip);
}

}  // namespace

extern "C" {

int dpn_sample_points(const DpnSampler* s, const float* cube, const float* labels, int mode, const int32_t* xi, const int32_t* yi,
                      const int32_t* ti, int64_t n, uint64_t seed, uint64_t offset, float* x, float* y, float* t, float* f,
                      float* coord_data, float* label_out, double* raw, void* stream) {
    return dpn_sample_points_replay(s, cube, labels, mode, xi, yi, ti, n, seed, offset, nullptr, 0, x, y, t, f, coord_data, label_out, raw, stream);
}

int dpn_sample_points_replay(const DpnSampler* s, const float* cube, const float* labels, int mode, const int32_t* xi, const int32_t* yi,
                             const int32_t* ti, int64_t n, uint64_t seed, uint64_t offset, const int32_t* step_dev, uint64_t stride,
                             float* x, float* y, float* t, float* f, float* coord_data, float* label_out, double* raw, void* stream) {
    if (!s || !cube || !x || !y || !t || !f || !coord_data || n <= 0) return -1;
    if (mode != DPN_SAMPLE_INTERIOR && mode != DPN_SAMPLE_MARGIN && mode != DPN_SAMPLE_EXPLICIT) return -1;
    if (mode == DPN_SAMPLE_EXPLICIT && (!xi || !yi || !ti)) return -1;
    if (s->lon_in < 2 || s->lat_in < 2 || s->t_in < 2 || s->lon < 2 || s->lat < 2) return -1;
    if (label_out && (!labels || mode == DPN_SAMPLE_INTERIOR)) return -1;          // labels exist at grid nodes only
    SampleArgs a{*s, cube, labels, xi, yi, ti, n, seed, offset, step_dev, stride, mode, x, y, t, f, coord_data, label_out, raw};
    hipLaunchKernelGGL(dpn_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_grid_maps(const float* out_n, int lon, int lat, const DpnPhysics* phys, int with_clip, float* maps, void* stream) {
    if (!out_n || !phys || !maps || lon <= 0 || lat <= 0) return -1;
    MapArgs a{out_n, lon, lat, *phys, with_clip, maps};
    const int64_t total = (int64_t)lon * lat * 6;
    hipLaunchKernelGGL(dpn_grid_maps_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

static bool lattice_ok(const DpnLattice* l, int64_t first, int64_t n) {
    return l && l->nx >= 1 && l->ny >= 1 && l->nt >= 1 && first >= 0 && first + n <= (int64_t)l->nx * l->ny * l->nt;
}

int dpn_sample_at(const DpnSampler* s, const float* cube, const double* xr, const double* yr, const double* tr, const DpnLattice* lattice,
                  int64_t first, int64_t n, float* x, float* y, float* t, float* f, float* coord_data, void* stream) {
    if (!s || !cube || !x || !y || !t || !f || !coord_data || n <= 0) return -1;
    if (s->lon_in < 2 || s->lat_in < 2 || s->t_in < 2 || s->lon < 2 || s->lat < 2) return -1;
    const bool stations = xr || yr || tr;
    if (stations ? (!xr || !yr || !tr || lattice) : !lattice_ok(lattice, first, n)) return -1;
    SampleAtArgs a{*s, cube, xr, yr, tr, stations ? DpnLattice{} : *lattice, first, n, x, y, t, f, coord_data};
    hipLaunchKernelGGL(dpn_sample_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int dpn_fields_out(const float* out_n, int64_t n, const DpnPhysics* phys, int with_clip, float* rows, float* maps, const DpnLattice* lattice,
                   int64_t first, void* stream) {
    if (!out_n || !phys || n <= 0 || (rows != nullptr) == (maps != nullptr)) return -1;
    if (maps ? !lattice_ok(lattice, first, n) : lattice != nullptr) return -1;
    FieldsOutArgs a{out_n, n, first, *phys, with_clip, rows, maps, maps ? *lattice : DpnLattice{}};
    hipLaunchKernelGGL(dpn_fields_out_kernel, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
