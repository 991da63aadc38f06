"""Cases, host models and bars for the sampler family of csrc/dpn_sampler.hip (dpn_sample_points, dpn_sample_points_replay, dpn_sample_at,
dpn_grid_maps, dpn_fields_out; the shared point function sample_point of csrc/dpn_sample_point.h) and for the uniforms of dpn_adaptive_select.
Imports without a GPU: tests/test_sampler_cases_cpu.py checks the models, the oracle and the bars, tests/test_gpu_sampler_cases.py runs the kernels.

The draws.  `philox4x32_10` is Philox-4x32-10 (Salmon et al. 2011) in plain Python integers, `u53` the 53-bit uniform and `below` the
multiply-shift bounded integer the kernel uses.  `draws` returns the fp64 raw[n, 3] the kernel must write, bit for bit: point i has counter
(lo32, hi32, stream, 0) of (offset + step * stride + i) mod 2^64, key (lo32, hi32) of the seed; stream 0 gives x (words 0, 1) and y (words 2, 3),
stream 1 gives t (word 0), stream 2 (`select_uniforms`) the uniforms of dpn_adaptive_select (words 0, 1).  Every operation is an exact integer
operation or one fp64 product, so there is no bar: equality.

The values.  Two references:
  * `oracle_points`: oracle/sampler_oracle.points_from_draws (scipy's RegularGridInterpolator in degrees, what the reference's xarray calls), on any
    geometry of the table;
  * `sample_model`: the kernel's documented arithmetic in numpy fp64, in index units, gathering from the cube as flat memory (behind it: NaN),
    with the inside rule: a weight within 1e-9 of [0, 1] is inside and clamped to [0, 1], anything further out is NaN.
`denorm_model` is the fp32 de-normalisation (multiply, then add: two roundings; the squared form; the clip of variables 2..5 that lets NaN
through), `grid_maps_model` and `fields_out_model` place it as dpn_grid_maps and dpn_fields_out do.  numpy's fp32 arithmetic rounds once per
operation, as the kernel compiled without contraction does: equality.

Bars (u = 2^-53).
  x, y, t     one fp64 product and one cast on both sides: equality with the oracle.
  f           lat_deg may be contracted to one fma in the kernel and the device sin is not numpy's: both move the fp64 value by a few u, the
              cast moves that by at most one fp32 ulp of the oracle value.
  coord_data  |kernel - oracle| <= ulp32(oracle) + (W + 16 u) max|corner|, the maximum over the eight corners of the point's cell, per variable.
    ulp32: both sides cast an fp64 value once; values that close round to the same or to neighbouring fp32 numbers.
    W: the two sides form their weights differently.  The oracle takes x_deg = begin + x res (a product and a sum, errors u S and u (B + S), with
       B = |begin| and S = the axis' span in degrees), the grid lines g_i = begin + i in_res alike, and w = (x_deg - g_i) / (g_i+1 - g_i): its
       sensitivity to x_deg is 1 / in_res, to the two grid lines (1 - w) / in_res and w / in_res, so to first order
           |dw_oracle| <= 2 u (B + 2 S) / in_res.
       The kernel takes fx = x cells with cells = fl(res / in_res): two relative roundings of a number <= S / in_res, |dw_kernel| <= 2 u S / in_res.
       Together u (2 B + 6 S) / in_res, which the issue's per-axis allowance W_axis = 4 u (B + S) / in_res covers whenever S <= B; where the
       resolutions are binary fractions the products are exact and only the sums' u (B + S) remains.  `axis_allowance_holds` states this condition
       and the CPU test asserts it for every axis of every geometry of the table (the time axis: B = 0, integer grid lines, one rounding in
       ft = t / t_step and one in the oracle's quotient: 2 u S / in_res).  The cell ratios that are no binary fractions sit on small cubes next
       to begin = 72 / 18 degrees, S <= 2.1.  A weight difference dw moves a lerp a (1 - w) + b w by dw (b - a): at most |dw| max|corner| between
       corners of one sign, up to twice that between corners of opposite sign and full size.  The allowance is kept as the issue
       states it: the first-order worst case, every rounding at u (which a rounding reaches only at a tie), for corners of one sign; it is not
       widened for the other case.  Its size, W ~ 1e-13, is what makes the bar a statement: one fp32 ulp everywhere except where a value
       cancels to below 1e-6 of its corners; the summaries of both test files print how many elements differ from the oracle at all.
    16 u: the evaluation itself.  Kernel: three nested lerps a (1 - w) + b w, four roundings each on a convex combination, <= 3 u max|corner| per
       level.  Oracle: eight terms value * (w1 w2 w3), each weight carrying up to five roundings and the term one, summed in sequence.  A first-order
       worst case of every rounding at its maximum and all aligned is 9 u + 13 u; the issue allots 16 u, which a sum of that many independent
       roundings (each reaching u only at a tie) does not approach -- the recorded ratios of the CPU test show the room.
  Where the oracle is NaN (more than 1e-6 of a cell outside the cube in the cases) the kernel must be NaN and nowhere else.

Seeded mistakes are named switches of the models (`MISTAKES`); the CPU test shows that each breaks a condition on at least one case.
"""
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from gemm_cases import SENTINEL, SENTINEL_BITS  # noqa: F401  (re-exported for the GPU test)
from oracle import sampler_oracle as SO

from deepphysinet_amd import _lib as L
from deepphysinet_amd.sampler import SamplerConfig

U53 = 2.0 ** -53
TOL_INSIDE = 1e-9
INTERIOR, MARGIN, EXPLICIT = L.SAMPLE_INTERIOR, L.SAMPLE_MARGIN, L.SAMPLE_EXPLICIT
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SENTINEL64_BITS = 0xCAFEBABECAFEBABE
SENTINEL64 = np.array([SENTINEL64_BITS], np.uint64).view(np.float64)[0]
GUARD_ROWS = 8

MISTAKES = ('drop_high_counter', 'one_stream', 'u53_no_low', 'below_modulo', 'swap_xy_weights', 'time_unclamped', 'half_open',
            'label_strides_swapped', 'map_order_swapped')

PHILOX_KNOWN_ANSWERS = (          # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---------------------------------------------------------------------------------------------- generator and draws
def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(v) & MASK32 for v in counter)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def u53(hi, lo, mistakes=()):
    """Uniform double in [0, 1) from 53 bits: the 32 of hi above the top 21 of lo."""
    bits = (hi << 21) if 'u53_no_low' in mistakes else ((hi << 21) ^ (lo >> 11))
    return float(bits & ((1 << 53) - 1)) * U53


def below(w, n, mistakes=()):
    """Integer in [0, n) from one 32-bit word: the high word of w * n."""
    return w % n if 'below_modulo' in mistakes else (w * n) >> 32


def _words(seed, ctr, stream, mistakes=()):
    hi = 0 if 'drop_high_counter' in mistakes else (ctr >> 32) & MASK32
    return philox4x32_10((ctr & MASK32, hi, stream, 0), (seed & MASK32, (seed >> 32) & MASK32))


def draws(mode, seed, offset, step, stride, n, sampler, mistakes=()):
    """raw[n, 3] fp64 (x index, y index, hour) of dpn_sample_points(_replay) in mode INTERIOR or MARGIN; sampler: a DpnSampler (or a Geo)."""
    s = sampler.struct() if isinstance(sampler, Geo) else sampler
    raw = np.empty((n, 3), np.float64)
    for i in range(n):
        ctr = (offset + step * stride + i) & MASK64
        w = _words(seed, ctr, 0, mistakes)
        v = w if 'one_stream' in mistakes else _words(seed, ctr, 1, mistakes)
        if mode == INTERIOR:
            raw[i, 0] = u53(w[0], w[1], mistakes) * float(s.lon - 1)
            raw[i, 1] = u53(w[2], w[3], mistakes) * float(s.lat - 1)
        elif mode == MARGIN:
            raw[i, 0] = below(w[0], s.lon, mistakes)
            raw[i, 1] = below(w[2], s.lat, mistakes)
        else:
            raise ValueError('draws: mode INTERIOR or MARGIN')
        raw[i, 2] = below(v[0], s.t_hours + 1, mistakes)
    return raw


def select_uniforms(seed, offset, step, stride, n, mistakes=()):
    """u[n] fp64 of dpn_adaptive_select: stream 2 of the counters offset + step * stride + j."""
    out = np.empty(n, np.float64)
    for j in range(n):
        w = _words(seed, (offset + step * stride + j) & MASK64, 2, mistakes)
        out[j] = u53(w[0], w[1], mistakes)
    return out


# ---------------------------------------------------------------------------------------------- geometries
@dataclass(frozen=True)
class Geo:
    """A fine grid over a coarse cube.  cfg given: the DpnSampler is SamplerConfig.c_struct(); otherwise it is built here (cells_x != cells_y)."""
    name: str
    lon: int
    lat: int
    lon_in: int
    lat_in: int
    t_in: int
    t_step: int
    out_res: float
    in_res_x: float
    in_res_y: float
    begin_lon: float
    begin_lat: float
    dx: float
    dy: float
    cfg: object = None

    @property
    def t_hours(self):
        return self.t_step * (self.t_in - 1)

    @property
    def in_lon(self):
        return self.begin_lon + np.arange(self.lon_in) * self.in_res_x

    @property
    def in_lat(self):
        return self.begin_lat + np.arange(self.lat_in) * self.in_res_y

    def struct(self):
        if self.cfg is not None:
            return self.cfg.c_struct()
        return L.DpnSampler(self.lon, self.lat, self.lon_in, self.lat_in, self.t_in, self.t_hours, self.out_res / self.in_res_x,
                            self.out_res / self.in_res_y, float(self.t_step), float(self.begin_lat), float(self.out_res), self.dx, self.dy)

    def axes(self):
        """(name, |begin|, span, in_res, exact products) per axis, in degrees (hours for t)."""
        dyadic = lambda v: float(v * 1024).is_integer()
        return (('x', abs(self.begin_lon), (self.lon_in - 1) * self.in_res_x, self.in_res_x, dyadic(self.out_res) and dyadic(self.in_res_x)),
                ('y', abs(self.begin_lat), (self.lat_in - 1) * self.in_res_y, self.in_res_y, dyadic(self.out_res) and dyadic(self.in_res_y)),
                ('t', 0.0, float(self.t_hours), float(self.t_step), True))

    def weight_allowance(self):
        """W of the module docstring: 4 u (|begin| + span) / in_res, summed over the three axes."""
        return sum(4.0 * U53 * (b + s) / r for _, b, s, r, _ in self.axes())

    def n_nodes(self):
        return self.lon * self.lat


def _from_cfg(name, **kw):
    c = SamplerConfig(**kw)
    return Geo(name, c.lon_size, c.lat_size, c.in_lon_size, c.in_lat_size, c.input_time_step_nums + 1, c.input_time_step, c.out_res_deg,
               c.in_res_deg, c.in_res_deg, c.begin_lon, c.begin_lat, c.dx, c.dy, c)


GEOMETRIES = (
    _from_cfg('default'),
    _from_cfg('minimal', lon_size=5, lat_size=5, in_lon_size=2, in_lat_size=2, input_time_step_nums=1),
    _from_cfg('r01_03', lon_size=10, lat_size=16, in_lon_size=4, in_lat_size=6, out_res_deg=0.1, in_res_deg=0.3),
    _from_cfg('r01_07', lon_size=22, lat_size=15, in_lon_size=4, in_lat_size=3, out_res_deg=0.1, in_res_deg=0.7),
    _from_cfg('r02_10', lon_size=11, lat_size=16, in_lon_size=3, in_lat_size=4, out_res_deg=0.2, in_res_deg=1.0),
    Geo('aniso', 13, 9, 7, 3, 3, 6, 0.25, 0.5, 1.0, 100.0, 30.0, 20000.0, 27000.0),          # cells_x = 0.5, cells_y = 0.25, dx != dy
    _from_cfg('equator', lon_size=9, lat_size=13, in_lon_size=3, in_lat_size=4, begin_lat=-1.5, begin_lon=10.0),
    _from_cfg('t3', lon_size=9, lat_size=9, in_lon_size=3, in_lat_size=3, input_time_step=3, input_time_step_nums=3),
)
GEO = {g.name: g for g in GEOMETRIES}
CUBES = ('normal', 'scaled')
NON_DYADIC = ('r01_03', 'r01_07')


def axis_allowance_holds(geo):
    """The condition under which 4 u (B + S) / in_res covers the first-order weight difference u (2 B + 6 S) / in_res (module docstring)."""
    return all(exact or s <= b for _, b, s, _, exact in geo.axes())


@lru_cache(maxsize=None)
def cube(name, kind):
    """[6, lat_in, lon_in, t_in] fp32.  'normal': N(0, 1); 'scaled': per-variable magnitudes, two of them pressure-like (1e5 + O(1): the trilinear
    sum cancels five digits)."""
    g = GEO[name]
    rng = np.random.default_rng(zlib.crc32(('%s/%s' % (name, kind)).encode()))
    z = rng.standard_normal((6, g.lat_in, g.lon_in, g.t_in))
    if kind == 'scaled':
        scale = np.array([1e-6, 1.0, 1.0, 10.0, 1e-3, 1.0]).reshape(6, 1, 1, 1)
        shift = np.array([0.0, 0.0, 1e5, 273.0, 0.0, 1e5]).reshape(6, 1, 1, 1)
        z = z * scale + shift
    out = z.astype(np.float32)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def labels(name):
    """[t_hours + 1, 6, lat, lon] fp32, every element distinct (its own flat index), so a wrong stride cannot hit an equal value."""
    g = GEO[name]
    shape = (g.t_hours + 1, 6, g.lat, g.lon)
    out = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
    assert out[-1, -1, -1, -1] < 2 ** 24
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- point sets
def node_points(geo):
    """Every fine node in the order x outer, y inner; small geometries at every hour, the default at hours cycling with the node (its last node
    at the last hour).  -> int32 xi, yi, ti."""
    xi, yi = np.repeat(np.arange(geo.lon), geo.lat), np.tile(np.arange(geo.lat), geo.lon)
    if geo.n_nodes() > 1000:
        ti = np.arange(xi.size) % (geo.t_hours + 1)
        ti[-1] = geo.t_hours
    else:
        hours = np.arange(geo.t_hours + 1)
        xi, yi, ti = np.tile(xi, hours.size), np.tile(yi, hours.size), np.repeat(hours, xi.size)
    return xi.astype(np.int32), yi.astype(np.int32), ti.astype(np.int32)


def station_points(geo):
    """fp64 positions: 300 random inside, every combination of positions on coarse cell faces (first, an inner one, last; as x = j / cells rounds),
    the first and the last node, and `n_out` positions outside the cube by 2e-6 and by half a coarse cell, one axis at a time (the last rows).
    -> xr, yr, tr, n_out."""
    rng = np.random.default_rng(zlib.crc32(geo.name.encode()) + 1)
    s = geo.struct()
    xr, yr, tr = rng.random(300) * (geo.lon - 1), rng.random(300) * (geo.lat - 1), rng.random(300) * geo.t_hours
    fx = [min(j / s.cells_x, geo.lon - 1.0) for j in sorted({0, (geo.lon_in - 1) // 2, geo.lon_in - 1})]
    fy = [min(j / s.cells_y, geo.lat - 1.0) for j in sorted({0, (geo.lat_in - 1) // 2, geo.lat_in - 1})]
    ft = [float(j * geo.t_step) for j in sorted({0, (geo.t_in - 1) // 2, geo.t_in - 1})]
    faces = np.array([(a, b, c) for a in fx for b in fy for c in ft] + [(0.0, 0.0, 0.0), (geo.lon - 1.0, geo.lat - 1.0, float(geo.t_hours))])
    mid = (0.5 * (geo.lon - 1), 0.5 * (geo.lat - 1), 0.5 * geo.t_hours)
    top = ((geo.lon_in - 1) / s.cells_x, (geo.lat_in - 1) / s.cells_y, float(geo.t_hours))
    cell = (1.0 / s.cells_x, 1.0 / s.cells_y, float(geo.t_step))
    out = []
    for ax in range(3):
        for d in (2e-6, 0.5):
            for v in (-d * cell[ax], top[ax] + d * cell[ax]):
                p = list(mid)
                p[ax] = v
                out.append(p)
    out = np.array(out)
    cat = lambda k: np.ascontiguousarray(np.concatenate([(xr, yr, tr)[k], faces[:, k], out[:, k]]))
    return cat(0), cat(1), cat(2), len(out)


def tolerance_points(geo):
    """The inside rule's two sides: positions 1e-10 of a coarse cell beyond each face of the cube (inside, taken as on the face) and 1e-8 beyond
    (NaN), one axis at a time, the other two mid-domain.  -> (xr, yr, tr), inside [n] bool, (the same positions clipped onto the domain)."""
    s = geo.struct()
    mid = (0.5 * (geo.lon - 1), 0.5 * (geo.lat - 1), 0.5 * geo.t_hours)
    top = (geo.lon - 1.0, geo.lat - 1.0, float(geo.t_hours))
    cell = (1.0 / s.cells_x, 1.0 / s.cells_y, float(geo.t_step))
    pts, inside = [], []
    for ax in range(3):
        for d in (1e-10, 1e-8):
            for v in (-d * cell[ax], top[ax] + d * cell[ax]):
                p = list(mid)
                p[ax] = v
                pts.append(p)
                inside.append(d < TOL_INSIDE)
    pts = np.array(pts)
    clipped = np.clip(pts, 0.0, np.array(top))
    cols = lambda a: tuple(np.ascontiguousarray(a[:, k]) for k in range(3))
    return cols(pts), np.array(inside), cols(clipped)


def lattice_of(geo):
    """nx = 7, ny = 3, nt = 2 strictly inside the domain: (x0, xstep, y0, ystep, t0, tstep, nx, ny, nt)."""
    return (0.25, (geo.lon - 1.5) / 6.0, 0.25, (geo.lat - 1.5) / 2.0, 0.5, geo.t_hours - 1.0, 7, 3, 2)


LATTICE_CHUNKS = ((16, 10), (0, 16), (26, 16), (5, 37))        # (first, n): begin and end mid-row, cross the time plane


def lattice_positions(lat):
    """The positions of a lattice tuple, formed as the kernel forms them: origin + index * step in two fp64 roundings."""
    x0, xs, y0, ys, t0, ts, nx, ny, nt = lat
    it, iy, ix = np.meshgrid(np.arange(nt), np.arange(ny), np.arange(nx), indexing='ij')
    return (x0 + ix * float(xs)).reshape(-1), (y0 + iy * float(ys)).reshape(-1), (t0 + it * float(ts)).reshape(-1)


# ---------------------------------------------------------------------------------------------- models of sample_point and the label gather
def _cells(geo, xr, yr, tr, mistakes=()):
    s = geo.struct()
    xr, yr, tr = (np.asarray(v, np.float64) for v in (xr, yr, tr))
    fx, fy, ft = xr * s.cells_x, yr * s.cells_y, tr / s.t_step_hours
    clamp = lambda f, top: np.clip(np.floor(f), 0, top - 2).astype(np.int64)
    ix, iy = clamp(fx, s.lon_in), clamp(fy, s.lat_in)
    it = np.floor(ft).astype(np.int64) if 'time_unclamped' in mistakes else clamp(ft, s.t_in)
    return s, (fx, fy, ft), (ix, iy, it)


def sample_model(geo, cube_, xr, yr, tr, mistakes=()):
    """sample_point in numpy fp64 -> x, y, t, f [n] and coord_data [n, 6] fp32.  The cube is read as flat memory with NaN behind it."""
    s, (fx, fy, ft), (ix, iy, it) = _cells(geo, xr, yr, tr, mistakes)
    xr, yr, tr = (np.asarray(v, np.float64) for v in (xr, yr, tr))
    wx, wy, wt = fx - ix, fy - iy, ft - it
    if 'half_open' in mistakes:
        inside = (wx >= 0) & (wx <= 1) & (wy >= 0) & (wy <= 1) & (wt >= 0) & (wt <= 1)
    else:
        ok = lambda w: (w >= -TOL_INSIDE) & (w <= 1.0 + TOL_INSIDE)
        inside = ok(wx) & ok(wy) & ok(wt)
        wx, wy, wt = (np.clip(w, 0.0, 1.0) for w in (wx, wy, wt))
    if 'swap_xy_weights' in mistakes:
        wx, wy = wy, wx
    sy, sx = s.lon_in * s.t_in, s.t_in
    sk = s.lat_in * sy
    flat = np.concatenate([np.asarray(cube_, np.float32).reshape(-1).astype(np.float64), np.full(sy + sx + 2, np.nan)])
    base = iy * sy + ix * sx + it
    base = np.where((base >= 0) & (base < 6 * sk), base, 6 * sk)               # (an unclamped index that leaves the buffer reads NaN)
    cd = np.empty((xr.size, 6), np.float32)
    for k in range(6):
        c = np.minimum(base + k * sk, flat.size - sy - sx - 2)
        v = lambda o: flat[c + o]
        lo = (v(0) * (1 - wt) + v(1) * wt) * (1 - wx) + (v(sx) * (1 - wt) + v(sx + 1) * wt) * wx
        hi = (v(sy) * (1 - wt) + v(sy + 1) * wt) * (1 - wx) + (v(sy + sx) * (1 - wt) + v(sy + sx + 1) * wt) * wx
        cd[:, k] = np.where(inside, lo * (1 - wy) + hi * wy, np.nan).astype(np.float32)
    lat_deg = s.begin_lat + yr * s.dlat
    f = (2.0 * 7.29e-5 * np.sin(lat_deg / 180.0 * 3.141592653589793)).astype(np.float32)
    return ((xr * float(s.dx)).astype(np.float32), (yr * float(s.dy)).astype(np.float32), (tr * 3600.0).astype(np.float32), f, cd)


def corner_max(geo, cube_, xr, yr, tr):
    """max |corner| over the eight corners of each point's (clamped) cell -> [n, 6] fp64."""
    s, _, (ix, iy, it) = _cells(geo, xr, yr, tr)
    a = np.abs(np.asarray(cube_, np.float64))
    m = np.zeros((6, ix.size))
    for dy in (0, 1):
        for dx in (0, 1):
            for dt in (0, 1):
                m = np.maximum(m, a[:, iy + dy, ix + dx, it + dt])
    return m.T


def oracle_points(geo, cube_, xr, yr, tr):
    """oracle/sampler_oracle.points_from_draws on this geometry -> x, y, t, f [n], coord_data [n, 6] (the model's order)."""
    x, y, t, cd, f = SO.points_from_draws(np.asarray(cube_), xr, yr, tr, geo.begin_lon, geo.begin_lat, geo.in_lon, geo.in_lat, geo.t_step,
                                          geo.dx, geo.dy, out_res=geo.out_res)
    return x, y, t, f[:, 0], cd


def labels_model(geo, labels_, X, Y, T, mistakes=()):
    """label_out[n, 6] of the node modes: labels read as flat memory at (((T * 6 + k) * lat + Y) * lon + X)."""
    X, Y, T = (np.asarray(v).astype(np.int64) for v in (X, Y, T))
    flat = np.asarray(labels_).reshape(-1)
    k = np.arange(6)[None, :]
    if 'label_strides_swapped' in mistakes:
        idx = (((T[:, None] * 6 + k) * geo.lon + X[:, None]) * geo.lat + Y[:, None])
    else:
        idx = (((T[:, None] * 6 + k) * geo.lat + Y[:, None]) * geo.lon + X[:, None])
    return flat[idx]


def cd_bar(geo, cube_, xr, yr, tr, oracle_cd):
    """The coord_data bar of the module docstring, [n, 6] fp64 (NaN where the oracle is NaN)."""
    return np.spacing(np.abs(oracle_cd)).astype(np.float64) + (geo.weight_allowance() + 16.0 * U53) * corner_max(geo, cube_, xr, yr, tr)


def check_points(geo, cube_, xr, yr, tr, got, ref=None):
    """got = (x, y, t, f, coord_data) against the oracle (ref: its result, computed once) -> dict: `exact` (x, y, t bitwise), `f_ratio`, `cd_ratio`
    (largest error / bar), `nan_match` (NaN exactly where the oracle is NaN), `n_nan`, and how many of the `n_compared` finite elements differ at
    all (`n_differ`)."""
    ox, oy, ot, of, ocd = oracle_points(geo, cube_, xr, yr, tr) if ref is None else ref
    x, y, t, f, cd = (np.asarray(v) for v in got)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    exact = bool(np.array_equal(bits(x), bits(ox)) and np.array_equal(bits(y), bits(oy)) and np.array_equal(bits(t), bits(ot)))
    f_err = np.abs(f.astype(np.float64) - of.astype(np.float64))
    f_ratio = float(np.max(f_err / np.maximum(np.spacing(np.abs(of)).astype(np.float64), 1e-300)))
    nan_o, nan_g = np.isnan(ocd), np.isnan(cd)
    bar = cd_bar(geo, cube_, xr, yr, tr, ocd)
    both = ~nan_o & ~nan_g
    err = np.abs(cd.astype(np.float64) - ocd.astype(np.float64))
    cd_ratio = float(np.max(err[both] / bar[both])) if both.any() else 0.0
    return dict(exact=exact, f_ratio=f_ratio, cd_ratio=cd_ratio, nan_match=bool(np.array_equal(nan_o, nan_g)), n_nan=int(nan_g.sum()),
                n_differ=int((err[both] > 0).sum()), n_compared=int(both.sum()))


def check_tolerance_points(geo, cube_, cd):
    """coord_data [n, 6] at tolerance_points(geo): finite exactly at the positions within 1e-9 of a cell of a face, NaN at the others, and the
    finite rows within the bar of the oracle ON the face (the clamp puts the weight there) -> (pattern ok, largest error / bar, differing elements)."""
    _, inside, clipped = tolerance_points(geo)
    ocd = oracle_points(geo, cube_, *clipped)[4]
    assert np.isfinite(ocd).all()
    cd = np.asarray(cd)
    pattern = bool(np.array_equal(np.isfinite(cd).all(axis=1), inside) and np.array_equal(np.isnan(cd).all(axis=1), ~inside))
    bar = cd_bar(geo, cube_, *clipped, ocd)
    err = np.abs(cd.astype(np.float64) - ocd.astype(np.float64))
    return pattern, float(np.nanmax(np.where(inside[:, None], err / bar, 0.0))), int((err[inside] > 0).sum())


def passes(res):
    return res['exact'] and res['nan_match'] and res['f_ratio'] <= 1.0 and res['cd_ratio'] <= 1.0


# ---------------------------------------------------------------------------------------------- de-normalisation
PHYS_TABLES = {
    # the shipped scales (u, v, P, T, q, rho), affine
    'affine': dict(mean=(0.5, -0.3, 1.0e5, 288.0, 8e-3, 1.2), std=(5.0, 4.0, 1.2e3, 12.0, 4e-3, 0.1), clip_lo=(0, 0, 5e4, 200.0, 0.0, 0.5),
                   clip_hi=(0, 0, 1.1e5, 330.0, 0.04, 2.0), sq_on=(0,) * 6, sq_add=(0.0,) * 6),
    # the three-factor squared form on an unclipped variable (u) and on a clipped one (q)
    'squared': dict(mean=(0.5, -0.3, 1.0e5, 288.0, 0.05, 1.2), std=(5.0, 4.0, 1.2e3, 12.0, 0.1, 0.1), clip_lo=(0, 0, 5e4, 200.0, 1e-6, 0.5),
                    clip_hi=(0, 0, 1.1e5, 330.0, 0.04, 2.0), sq_on=(1, 0, 0, 0, 1, 0), sq_add=(-2.0, 0.0, 0.0, 0.0, 1e-6, 0.0)),
}


def phys_struct(name):
    t = PHYS_TABLES[name]
    p = L.DpnPhysics()
    for k in range(6):
        p.mean[k], p.std[k], p.clip_lo[k], p.clip_hi[k] = t['mean'][k], t['std'][k], t['clip_lo'][k], t['clip_hi'][k]
        p.clip_on[k], p.factor[k], p.sq_on[k], p.sq_add[k] = int(k >= 2), 1.0, t['sq_on'][k], t['sq_add'][k]
    p.criterion, p.beta, p.reduce_sum = 0, 1.0, 0
    return p


def denorm_inputs(n, seed=0):
    """out_n [n, 6] fp32 ~ 2 N(0, 1) (both clip bounds are reached) with NaN, +inf and -inf in every column."""
    rng = np.random.default_rng(1000 + seed)
    out = (2.0 * rng.standard_normal((n, 6))).astype(np.float32)
    for k in range(6):
        rows = rng.choice(n, 3, replace=False)
        out[rows[0], k], out[rows[1], k], out[rows[2], k] = np.nan, np.inf, -np.inf
    return out


def denorm_model(out_n, table, with_clip):
    """[.., 6] fp32 -> physical values in fp32: out * std, + mean (two roundings); squared form v * v + sq_add; variables 2..5 clipped, NaN kept."""
    t = PHYS_TABLES[table]
    f = lambda key: np.asarray(t[key], np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        v = (np.asarray(out_n, np.float32) * f('std')).astype(np.float32) + f('mean')
        sq = (v * v).astype(np.float32) + f('sq_add')
        v = np.where(np.asarray(t['sq_on'], bool), sq, v).astype(np.float32)
        if with_clip:
            c = np.minimum(np.maximum(v, f('clip_lo')), f('clip_hi'))
            c = np.where(np.isnan(v), v, c)
            v = np.where(np.arange(6) >= 2, c, v).astype(np.float32)
    return v


def grid_maps_model(out_n, lon, lat, table, with_clip):
    """dpn_grid_maps: out_n [lon * lat, 6] in node order x outer, y inner -> maps [6, lat, lon]."""
    return np.ascontiguousarray(denorm_model(out_n, table, with_clip).reshape(lon, lat, 6).transpose(2, 1, 0))


def fields_out_model(out_n, table, with_clip, lattice=None, first=0, maps=None, mistakes=()):
    """dpn_fields_out: rows [n, 6], or -- lattice given -- the n points written to their places in maps [nt, 6, ny, nx] (changed in place; every
    other element is left alone)."""
    if lattice is None:
        return denorm_model(out_n, table, with_clip)
    nx, ny = lattice[6], lattice[7]
    n = out_n.shape[0]
    src = np.asarray(out_n, np.float32)
    if 'map_order_swapped' in mistakes:                     # reads out_n[k * n + p] in the place of out_n[p * 6 + k]
        src = src.reshape(-1).reshape(6, n).T
    v = denorm_model(np.ascontiguousarray(src), table, with_clip)
    g = first + np.arange(n)
    it, r = g // (nx * ny), g % (nx * ny)
    flat = maps.reshape(maps.shape[0], 6, nx * ny)
    for k in range(6):
        flat[it, k, r] = v[:, k]
    return maps
