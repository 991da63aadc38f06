"""On-device collocation sampler.

Mirrors the three point generators of the reference's dataset (dataset/physics_dataset.py): `get_inter_data` (:431-499),
`get_item_label_data` (:323-429) and `get_margin_grid` (:528-587) -- same names, same return tuples -- but the coarse
forecast cube and the labels are resident in HBM and one HIP kernel (`dpn_sample_points`) draws the points, interpolates
the cube tri-linearly (what `xarray.DataArray.interp` does there, six times per call) and evaluates the Coriolis parameter.
The host is out of the per-step loop.  The draws come from Philox-4x32-10 instead of numpy's global Mersenne state (the
reference's sequence depends on DataLoader worker seeding and is not reproducible either); everything downstream of the
draws is parity-tested against `oracle/sampler_oracle.py`.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .point_path import _ptr, _stream, require_gpu


@dataclass
class SamplerConfig:
    """Grid constants of PhysicsDataset (physics_dataset.py:83-126; configs/DeepPhysiNet_NCEP_cfg.py:93-111)."""
    lon_size: int = 257            # label_lon_size
    lat_size: int = 145            # label_lat_size
    in_lon_size: int = 65          # len(in_lon)
    in_lat_size: int = 37          # len(in_lat)
    input_time_step: int = 6
    input_time_step_nums: int = 4
    out_res_deg: float = 0.25      # spacing of the fine grid (the literal 0.25 of :336-337, :444-445)
    in_res_deg: float = 1.0        # spacing of in_lon / in_lat
    begin_lat: float = 18.0        # out_lat[0]
    dx: float = 27000.0
    dy: float = 27000.0
    begin_lon: float = 72.0        # out_lon[0] (host side only: at_lonlat's degrees -> index units)

    def c_struct(self) -> L.DpnSampler:
        ratio = self.out_res_deg / self.in_res_deg
        return L.DpnSampler(self.lon_size, self.lat_size, self.in_lon_size, self.in_lat_size, self.input_time_step_nums + 1,
                            self.input_time_step * self.input_time_step_nums, ratio, ratio, float(self.input_time_step),
                            float(self.begin_lat), float(self.out_res_deg), float(self.dx), float(self.dy))


@dataclass
class Lattice:
    """A regular lattice of nx * ny * nt positions in the sampler's units (fine-grid index units, hours); mirrors DpnLattice.  Point
    g = (it * ny + iy) * nx + ix (ix fastest, it slowest) lies at (x0 + ix * xstep, y0 + iy * ystep, t0 + it * tstep).  A lattice may reach
    outside the coarse cube: coord_data, and every field evaluated from it, is NaN there.  Inside rule (sample_point): a position whose weight in
    its coarse cell lies within 1e-9 of [0, 1] is inside and the weight is clamped to [0, 1]; the last node of a geometry whose cell ratio is no
    binary fraction (0.1 / 0.3 degrees) is therefore inside, a position more than 1e-9 of a coarse cell beyond a face is NaN."""
    x0: float
    xstep: float
    y0: float
    ystep: float
    t0: float
    tstep: float
    nx: int
    ny: int
    nt: int

    def __post_init__(self):
        if min(int(self.nx), int(self.ny), int(self.nt)) < 1:
            raise ValueError('a lattice needs nx, ny, nt >= 1, got (%s, %s, %s)' % (self.nx, self.ny, self.nt))

    @property
    def n_points(self) -> int:
        return int(self.nx) * int(self.ny) * int(self.nt)

    def c_struct(self) -> L.DpnLattice:
        return L.DpnLattice(float(self.x0), float(self.xstep), float(self.y0), float(self.ystep), float(self.t0), float(self.tstep),
                            int(self.nx), int(self.ny), int(self.nt))

    def positions(self):
        """(x_idx, y_idx, hours): three fp64 arrays [n_points] in point order, formed as the kernel forms them (origin + index * step)."""
        it, iy, ix = np.meshgrid(np.arange(self.nt), np.arange(self.ny), np.arange(self.nx), indexing='ij')
        return ((self.x0 + ix * float(self.xstep)).reshape(-1), (self.y0 + iy * float(self.ystep)).reshape(-1),
                (self.t0 + it * float(self.tstep)).reshape(-1))


class CollocationSampler:
    """cube: [6, in_lat, in_lon, t_in] fp32 normalised coarse forecast (obs_name_order u10,v10,pres,t2,q2,rio; the per-variable
    [y, x, t] arrays of physics_dataset.py:400 stacked); labels (optional): [t_hours + 1, 6, lat, lon] fp32 normalised ERA5."""

    def __init__(self, cfg: SamplerConfig, cube: torch.Tensor, labels: torch.Tensor = None, seed: int = 0):
        require_gpu(cube, 'cube')
        c = cfg
        if tuple(cube.shape) != (6, c.in_lat_size, c.in_lon_size, c.input_time_step_nums + 1):
            raise ValueError('cube must be [6, %d, %d, %d], got %s' % (c.in_lat_size, c.in_lon_size, c.input_time_step_nums + 1, tuple(cube.shape)))
        if (c.lon_size - 1) * c.out_res_deg > (c.in_lon_size - 1) * c.in_res_deg + 1e-9 or \
           (c.lat_size - 1) * c.out_res_deg > (c.in_lat_size - 1) * c.in_res_deg + 1e-9:
            raise ValueError('the fine grid must lie inside the coarse cube')
        self.cfg, self._s = cfg, cfg.c_struct()
        self.cube = cube.detach().float().contiguous()
        self.labels = None
        if labels is not None:
            require_gpu(labels, 'labels')
            hours = c.input_time_step * c.input_time_step_nums + 1
            if tuple(labels.shape) != (hours, 6, c.lat_size, c.lon_size):
                raise ValueError('labels must be [%d, 6, %d, %d]' % (hours, c.lat_size, c.lon_size))
            self.labels = labels.detach().float().contiguous()
        self.seed, self.offset = int(seed), 0
        self._step_dev, self._stride = None, 0

    def bind_step_counter(self, step_count: torch.Tensor, points_per_step: int):
        """Draw from the DEVICE-side step counter: after this, every draw uses Philox counter = (offset inside the step) +
        step_count * points_per_step, step_count being read by the kernel (FusedClipAdam.step_count: int32[1] on the device, bumped
        once per optimiser step).  A sampler launch captured in a hipGraph then draws fresh points on every replay; host-side state no
        longer advances between steps (begin_step() rewinds the offset inside the step; training_batch() calls it)."""
        require_gpu(step_count, 'step_count')
        if step_count.dtype != torch.int32 or step_count.numel() != 1:
            raise ValueError('step_count must be one int32 on the device')
        self._step_dev, self._stride, self.offset = step_count, int(points_per_step), 0

    def begin_step(self):
        if self._step_dev is not None:
            self.offset = 0

    def _run(self, mode, n, xi=None, yi=None, ti=None, want_labels=False, want_raw=False):
        dev = self.cube.device
        x, y, t, f = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        cd = torch.empty((n, 6), dtype=torch.float32, device=dev)
        lab = torch.empty((n, 6), dtype=torch.float32, device=dev) if want_labels else None
        raw = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_raw else None
        if want_labels and self.labels is None:
            raise RuntimeError('this sampler was built without labels')
        lib = L.load()
        if self._step_dev is not None and mode != L.SAMPLE_EXPLICIT and self.offset + n > self._stride:
            raise RuntimeError('more points drawn in one step (%d) than bind_step_counter() reserved (%d)' % (self.offset + n, self._stride))
        L.check(lib.dpn_sample_points_replay(ctypes.byref(self._s), _ptr(self.cube), _ptr(self.labels) if want_labels else None, mode,
                                             _ptr(xi), _ptr(yi), _ptr(ti), n, self.seed, self.offset, _ptr(self._step_dev), self._stride,
                                             _ptr(x), _ptr(y), _ptr(t), _ptr(f), _ptr(cd), _ptr(lab), _ptr(raw), _stream()),
                'dpn_sample_points_replay')
        if mode != L.SAMPLE_EXPLICIT:
            self.offset += n                                   # the next call continues the Philox counter
        return x, y, t, f, cd, lab, raw

    def get_inter_data(self, n: int = 4096, with_raw: bool = False):
        """-> inter_x, inter_y, inter_t, inter_data, inter_f  (physics_dataset.py:499); shapes [n], [n], [n], [n,6], [n,1]."""
        x, y, t, f, cd, _, raw = self._run(L.SAMPLE_INTERIOR, n, want_raw=with_raw)
        out = (x, y, t, cd, f.unsqueeze(1))
        return out + (raw,) if with_raw else out

    def select_weighted(self, score, pool_rows, n, k=1.0, c=1.0, offset=0, scratch=None, with_details=False):
        """dpn_adaptive_select: n rows drawn with replacement from the m candidates pool_rows = (x, y, t, f [m], coord_data [m, 6]) with probability
        ~ score ** k / mean(score ** k) + c (score [m] fp64 on the device), by the inverse of the weights' fp64 prefix sum at the uniforms of Philox
        stream 2, counters offset .. offset + n (on top of the bound step counter's share).  Returns (x, y, t, f, coord_data) of the drawn rows, and with
        with_details also (idx int32 [n], u fp64 [n], picked_score fp64 [n], scratch: its first m doubles are the prefix sum)."""
        require_gpu(score, 'score', 'select_weighted')
        if score.dtype != torch.float64 or score.dim() != 1 or not score.is_contiguous():
            raise ValueError('score must be a contiguous fp64 vector')
        lib = L.load()
        m, dev = score.shape[0], score.device
        size = int(lib.dpn_adaptive_scratch_doubles(m))
        if size <= 0:
            raise ValueError('select_weighted: %d candidates; dpn_adaptive_select takes 1 .. 2**20' % m)
        x, y, t, f, cd = pool_rows
        if any(v.shape[0] != m or v.dtype != torch.float32 or not v.is_contiguous() for v in pool_rows) or tuple(cd.shape) != (m, 6):
            raise ValueError('pool_rows: x, y, t, f [m] and coord_data [m, 6], contiguous fp32, one row per score')
        if int(n) < 1:
            raise ValueError('n must be positive, got %r' % (n,))
        if not (k >= 0.0 and c >= 0.0 and np.isfinite(k) and np.isfinite(c)):
            raise ValueError('k and c must be finite and >= 0, got k = %r, c = %r' % (k, c))
        if scratch is None:
            scratch = torch.empty(size, dtype=torch.float64, device=dev)
        elif scratch.dtype != torch.float64 or scratch.numel() < size:
            raise ValueError('scratch: at least %d fp64 values' % size)
        ox, oy, ot, of = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        ocd = torch.empty((n, 6), dtype=torch.float32, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev) if with_details else None
        u, picked = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)) if with_details else (None, None)
        L.check(lib.dpn_adaptive_select(_ptr(score), m, float(k), float(c), _ptr(x), _ptr(y), _ptr(t), _ptr(f), _ptr(cd), n, self.seed, int(offset),
                                        _ptr(self._step_dev), self._stride, _ptr(ox), _ptr(oy), _ptr(ot), _ptr(of), _ptr(ocd), _ptr(idx), _ptr(u),
                                        _ptr(picked), _ptr(scratch), _stream()), 'dpn_adaptive_select')
        out = (ox, oy, ot, of, ocd)
        return out + (idx, u, picked, scratch) if with_details else out

    def get_inter_data_adaptive(self, packed_field, factors, n: int = 4096, pool: int = None, k: float = 1.0, c: float = 1.0, with_details: bool = False):
        """get_inter_data with the n interior points placed where the PDE residuals are large (residual-based adaptive sampling, Wu et al. 2023):
        `pool` (default 8 n) points are drawn as get_inter_data draws them, scored by packed_field (point_path.PackedField of the field's current
        weights) with score_i = sum_e factors[e] * residual_ie ** 2 (factors: six floats in LOSS_ORDER), and n of them are drawn with replacement with
        probability ~ score ** k / mean(score ** k) + c.  k = 0 is uniform sampling again; c = 0 never draws a point of zero residual.
        -> inter_x, inter_y, inter_t, inter_data, inter_f as get_inter_data; with_details adds a dict: idx [n] (rows of the pool), u [n], picked_score
        [n], score [pool], nonfinite (device scalar: scores that were not finite and count as 0), stats [3], pool (x, y, t, f, coord_data), res, cdf.
        The pool advances the Philox offset by `pool` (and counts against bind_step_counter's reservation); the selection's uniforms are stream 2 of
        the pool's first n counters.  Nothing here allocates outside torch's caching allocator or synchronises."""
        n, pool = int(n), int(8 * n if pool is None else pool)
        if n < 1 or pool < 1:
            raise ValueError('n and pool must be positive, got %d, %d' % (n, pool))
        first = self.offset
        x, y, t, f, cd, _, _ = self._run(L.SAMPLE_INTERIOR, pool)
        score, stats, res, scratch = packed_field.residual_scores(x, y, t, f, cd, factors, k)
        sel = self.select_weighted(score, (x, y, t, f, cd), n, k, c, offset=first, scratch=scratch, with_details=with_details)
        out = (sel[0], sel[1], sel[2], sel[4], sel[3].unsqueeze(1))
        if not with_details:
            return out
        return out + ({'idx': sel[5], 'u': sel[6], 'picked_score': sel[7], 'score': score, 'nonfinite': stats[1], 'stats': stats,
                       'pool': (x, y, t, f, cd), 'res': res, 'cdf': scratch[:pool]},)

    def get_item_label_data(self, n: int = 20480, with_raw: bool = False):
        """-> margin_x, margin_y, margin_t, margin_data, margin_f, margin_input_data  (physics_dataset.py:429)."""
        x, y, t, f, cd, lab, raw = self._run(L.SAMPLE_MARGIN, n, want_labels=self.labels is not None, want_raw=with_raw)
        out = (x, y, t, lab, f.unsqueeze(1), cd)
        return out + (raw,) if with_raw else out

    def get_margin_grid(self, margin_x_list, margin_y_list, margin_t_list):
        """-> inter_x, inter_y, inter_t, inter_data, inter_f for caller-given node indices and hours (physics_dataset.py:587)."""
        dev = self.cube.device
        xi, yi, ti = (torch.as_tensor(v, dtype=torch.int32, device=dev).contiguous() for v in (margin_x_list, margin_y_list, margin_t_list))
        c = self.cfg
        if xi.numel() and (int(xi.min()) < 0 or int(xi.max()) >= c.lon_size or int(yi.min()) < 0 or int(yi.max()) >= c.lat_size
                           or int(ti.min()) < 0 or int(ti.max()) > c.input_time_step * c.input_time_step_nums):
            raise IndexError('grid node / hour outside the domain')
        x, y, t, f, cd, _, _ = self._run(L.SAMPLE_EXPLICIT, xi.numel(), xi, yi, ti)
        return x, y, t, cd, f.unsqueeze(1)

    def full_grid(self, time_id: int):
        """All lon*lat nodes at one hour in the reference's visualisation order (x outer, y inner; interface_physics.py:538-543)."""
        c = self.cfg
        dev = self.cube.device
        xs = torch.arange(c.lon_size, dtype=torch.int32, device=dev).repeat_interleave(c.lat_size)
        ys = torch.arange(c.lat_size, dtype=torch.int32, device=dev).repeat(c.lon_size)
        ts = torch.full_like(xs, int(time_id))
        return self.get_margin_grid(xs, ys, ts)

    # ---- given positions (inference): stations and lattices -------------------------------------------------------------------------
    def lattice(self, refine: int = 1, hours=0, x_range=None, y_range=None) -> Lattice:
        """A lattice over the training domain with steps of 1 / refine node: nx = (lon - 1) * refine + 1, ny alike.  x_range / y_range = (first,
        last) in node units cut a window out of it.  hours: a tuple (t0, tstep, nt), one hour, or a sequence of equally spaced hours."""
        r = int(refine)
        if r < 1 or r != refine:
            raise ValueError('refine must be a positive integer, got %r' % (refine,))
        c = self.cfg

        def axis(rng, size):
            lo, hi = (0.0, float(size - 1)) if rng is None else (float(rng[0]), float(rng[1]))
            if hi < lo:
                raise ValueError('empty range %r' % (rng,))
            return lo, int(np.floor((hi - lo) * r + 1e-9)) + 1
        x0, nx = axis(x_range, c.lon_size)
        y0, ny = axis(y_range, c.lat_size)
        if isinstance(hours, tuple) and len(hours) == 3:
            t0, tstep, nt = float(hours[0]), float(hours[1]), int(hours[2])
        else:
            h = np.atleast_1d(np.asarray(hours, dtype=np.float64))
            if h.ndim != 1 or h.size == 0:
                raise ValueError('hours: a tuple (t0, tstep, nt), one hour or a 1-d sequence of hours')
            t0, nt = float(h[0]), int(h.size)
            tstep = float(h[1] - h[0]) if nt > 1 else 1.0
            if nt > 2 and not np.allclose(np.diff(h), tstep, rtol=0, atol=1e-9 * max(1.0, abs(tstep))):
                raise ValueError('hours must be equally spaced (evaluate other sets with at_positions)')
        return Lattice(x0, 1.0 / r, y0, 1.0 / r, t0, tstep, nx, ny, nt)

    def sample_at(self, n, xr=None, yr=None, tr=None, lattice: Lattice = None, first: int = 0, out=None):
        """dpn_sample_at: n stations (xr, yr, tr fp64 device tensors) or points first .. first + n of a lattice -> x, y, t, f [n], coord_data [n, 6];
        out = the five buffers of an earlier call with at least n rows (a chunk loop reuses them)."""
        dev = self.cube.device
        if out is None:
            out = tuple(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)) + (torch.empty((n, 6), dtype=torch.float32, device=dev),)
        x, y, t, f, cd = (v[:n] for v in out)
        lat = None if lattice is None else lattice.c_struct()
        L.check(L.load().dpn_sample_at(ctypes.byref(self._s), _ptr(self.cube), _ptr(xr), _ptr(yr), _ptr(tr), None if lat is None else ctypes.byref(lat),
                                       int(first), int(n), _ptr(x), _ptr(y), _ptr(t), _ptr(f), _ptr(cd), _stream()), 'dpn_sample_at')
        return x, y, t, f, cd

    def check_positions(self, x_idx, y_idx, hours):
        """Station positions checked on the host and put on the device: (xr, yr, tr), fp64 [n], as sample_at takes them.  IndexError outside the fine
        grid or outside [0, input_time_step * input_time_step_nums] hours."""
        c = self.cfg
        pos = [np.ascontiguousarray(np.atleast_1d(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)), dtype=np.float64).reshape(-1)
               for v in (x_idx, y_idx, hours)]
        n = pos[0].size
        if n == 0 or any(v.size != n for v in pos):
            raise ValueError('x_idx, y_idx and hours must have the same, non-zero length')
        hi = (c.lon_size - 1, c.lat_size - 1, c.input_time_step * c.input_time_step_nums)
        for v, top in zip(pos, hi):
            if not (np.all(v >= 0.0) and np.all(v <= top)):          # (NaN fails both)
                raise IndexError('position / hour outside the domain')
        return tuple(torch.from_numpy(v).to(self.cube.device) for v in pos)

    def at_positions(self, x_idx, y_idx, hours):
        """-> x, y, t, coord_data, f (as get_margin_grid) at given positions: fractional fine-grid indices and fractional hours, one per station.
        IndexError outside the fine grid or outside [0, input_time_step * input_time_step_nums] hours."""
        xr, yr, tr = self.check_positions(x_idx, y_idx, hours)
        x, y, t, f, cd = self.sample_at(xr.shape[0], xr, yr, tr)
        return x, y, t, cd, f.unsqueeze(1)

    def lonlat_to_index(self, lon_deg, lat_deg):
        """Degrees -> fine-grid index units, in fp64 on the host: (lon - begin_lon) / out_res_deg, (lat - begin_lat) / out_res_deg."""
        c = self.cfg
        return ((np.asarray(lon_deg, dtype=np.float64) - c.begin_lon) / c.out_res_deg, (np.asarray(lat_deg, dtype=np.float64) - c.begin_lat) / c.out_res_deg)

    def at_lonlat(self, lon_deg, lat_deg, hours):
        """at_positions for stations given in degrees east / north."""
        xi, yi = self.lonlat_to_index(lon_deg, lat_deg)
        return self.at_positions(xi, yi, hours)

    def training_batch(self, field_data, forecast_h, n_margin: int = 20480, n_inter: int = 4096):
        """One sample of PhysicsDataset.__getitem__ (physics_dataset.py:501-519) as the dict InterfacePhysics.training_step takes: the
        field sample and lead time given by the caller, 20 480 margin (grid-node, labelled) and 4 096 interior collocation points drawn,
        interpolated and labelled on the device (batch sizes: cfg:111, physics_dataset.py:30)."""
        self.begin_step()
        mx, my, mt, mlab, mf, mcd = self.get_item_label_data(n_margin)
        ix, iy, it, icd, if_ = self.get_inter_data(n_inter)
        col = lambda v: v.reshape(-1, 1)
        return {'field_data': field_data, 'forecast_h': forecast_h,
                'margin_x': col(mx), 'margin_y': col(my), 'margin_t': col(mt), 'margin_f': mf, 'margin_data': mlab, 'margin_input_data': mcd,
                'inter_x': col(ix), 'inter_y': col(iy), 'inter_t': col(it), 'inter_f': if_, 'inter_data': icd}



class SyntheticSamples:
    """Default `samples` source of run_train_interface when the configuration names none: one epoch = the 61 six-hourly lead times of the
    reference's file map (tools/generate_input_map.py:41), each a synthetic field sample [1,159,2405] (normalised forecasts ~ N(0,1), the
    four constant rows ~ U[0,1]: SURVEY 8d) whose collocation batch is drawn by the on-device CollocationSampler from synthetic coarse /
    label cubes of the configured shapes.  It stands in for PhysicsDataset's GeoTIFF / xarray reader (dataset/physics_dataset.py: file I/O
    outside this build, no data offline) so that the reference's two-keyword call `run_train_interface(checkpoint_path=, log_path=)`
    (train.py:47) runs end to end.  A sequence: data-parallel ranks index only their own samples."""

    def __init__(self, device, n_margin=20480, n_inter=4096, leads=61, seed=0, lat=145, lon=257):
        g = torch.Generator().manual_seed(seed)
        self.device = torch.device(device)
        cube = torch.randn(6, 37, 65, 5, generator=g).to(self.device)
        labels = torch.randn(25, 6, lat, lon, generator=g).to(self.device)
        self.sampler = CollocationSampler(SamplerConfig(), cube, labels, seed=seed + 1)
        self.n_margin, self.n_inter, self.leads, self.seed = int(n_margin), int(n_inter), int(leads), int(seed)

    def __len__(self):
        return self.leads

    def __getitem__(self, i):
        if not 0 <= i < self.leads:
            raise IndexError(i)
        g = torch.Generator().manual_seed(self.seed * 1000 + 17 + i)
        field = torch.randn(1, 159, 2405, generator=g)
        field[:, 155:, :] = torch.rand(1, 4, 2405, generator=g)
        fh = torch.full((1, 1, 1), 6.0 * i / 360.0)
        return self.sampler.training_batch(field.to(self.device), fh.to(self.device), n_margin=self.n_margin, n_inter=self.n_inter)
