"""Host side of the HIP point path: buffers, pointer tables and the two autograd entry points.

`point_fields`  : six VariableNets evaluated at N collocation points (PhysicsNet.forward's hot part,
                  reference model/physics_net.py:49-54), differentiable w.r.t. all weights.
`pde_losses`    : place_one_batch's hot part (reference interface/interface_physics.py:278-301): fields,
                  6x3 coordinate Jacobian, inverse_norm (+clip), six residual losses; backward gives every
                  weight gradient without building an autograd graph over the points.

PyTorch is used for device memory, the current HIP stream and autograd bookkeeping only; all arithmetic on
points happens in libdpn_hip.so (deepphysinet_amd/csrc/dpn_point.hip, dpn_wgrad.hip, dpn_residual.hip).  There is no CPU path.
"""
import ctypes
import math
import os
from dataclasses import dataclass, field
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import branch, config
from .ensemble import reads_coriolis, reads_jacobian
from .regions import FLOAT_OUTPUTS as REGION_FLOAT_OUTPUTS, INT_OUTPUTS as REGION_INT_OUTPUTS, n_slots as region_slots
from .grad_arena import new_grad, slot_of
from . import verification as VF
from . import prob_verification as PV
from . import neighbourhood as NB

# configs/DeepPhysiNet_NCEP_cfg.py:64-76 -- order u10, v10, pres, t2, q2, rio (network output order)
OBS_ORDER = ('u10', 'v10', 'pres', 't2', 'q2', 'rio')
LOSS_ORDER = ('motion_u_factor', 'motion_v_factor', 'continuous_factor', 'energy_factor', 'vapor_factor', 'gas_factor')
STATIC_NAMES = ('Wd', 'bd', 'W1', 'bf1', 'W2', 'bf2', 'wo', 'bo')      # per-net parameter tensors, in this order
STATIC_SHAPES = ((256, 192), (256,), (256, 256), (256,), (256, 256), (256,), (1, 256), (1,))


@dataclass
class PointConfig:
    """Geometry + physics constants of one InterfacePhysics instance."""
    dx: float = 27000.0
    dy: float = 27000.0
    lon_size: int = 257
    lat_size: int = 145
    pred_t_span: float = 86400.0
    mean: Sequence[float] = (0.14507186950562942, -0.17325370241478535, 89741.36105771353, 283.58054561520305,
                             0.007909478276582905, 1.0966503643401704)
    std: Sequence[float] = (3.0050219075895894, 3.006602165591562, 13296.749084125422, 15.583177935722373,
                            0.006304067969976075, 0.15166081218127583)
    clip_lo: Sequence[float] = (-500.0, -500.0, 10000.0, 50.0, 1e-6, 1e-6)
    clip_hi: Sequence[float] = (500.0, 500.0, 500000.0, 500.0, 10.0, 10.0)
    with_clip: bool = True
    clip_vars: Sequence[bool] = (False, False, True, True, True, True)      # which variables torch.clip applies to when with_clip (never u, v; not a variable
                                                                            # whose obs_norm_cfg says use_norm: False -- interface_physics.py:236-257)
    factors: Sequence[float] = (1.e3, 1.e3, 1.e10, 1e1, 1.e14, 1.e-7)
    prec: int = L.PREC_BF16X2
    sq_add: Sequence[Optional[float]] = (None,) * 6      # three-factor min_max (:244-247): (out * std + mean) ** 2 + sq_add; None: the affine forms
    criterion: int = L.CRIT_MSE            # the PDE criterion (train_cfg.losses.pde_loss): MSELoss | L1Loss | WeightSmoothL1Loss(beta)
    beta: float = 0.0
    reduce_sum: bool = False               # the criterion's reduction: "mean" (shipped) or "sum"

    def geometry(self) -> L.DpnGeometry:
        return L.DpnGeometry(float(self.dx), float(self.dy), float(self.lon_size - 1), float(self.lat_size - 1), float(self.pred_t_span))

    def physics(self) -> L.DpnPhysics:
        ph = L.DpnPhysics()
        for k in range(L.NETS):
            ph.mean[k], ph.std[k] = float(self.mean[k]), float(self.std[k])
            ph.clip_lo[k], ph.clip_hi[k] = float(self.clip_lo[k]), float(self.clip_hi[k])
            ph.clip_on[k] = int(bool(self.with_clip) and k >= 2 and bool(self.clip_vars[k]))     # u, v are never clipped (interface_physics.py:256-257)
            ph.factor[k] = float(self.factors[k])
        ph.criterion, ph.beta, ph.reduce_sum = int(self.criterion), float(self.beta), int(bool(self.reduce_sum))
        for k in range(L.NETS):
            ph.sq_on[k], ph.sq_add[k] = (0, 0.0) if self.sq_add[k] is None else (1, float(self.sq_add[k]))
        return ph


_freq_cache = {}


def _freqs(device):
    key = str(device)
    if key not in _freq_cache:
        f32 = 2.0 ** torch.linspace(0.0, 4.0, steps=32)       # fp32, exactly utils/position_encoding.py:27
        f16 = 2.0 ** torch.linspace(0.0, 4.0, steps=16)
        _freq_cache[key] = torch.cat([f32, f16]).to(device=device, dtype=torch.float32).contiguous()
    return _freq_cache[key]


def require_gpu(t: torch.Tensor, name: str, what: str = 'point path'):
    if not t.is_cuda:
        raise RuntimeError('deepphysinet_amd %s needs HIP device tensors (%s is on %s); there is no CPU fallback' % (what, name, t.device))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    """Device pointer for the C ABI.  Every tensor handed to the library goes through here: a host tensor raises instead of reaching a kernel."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('deepphysinet_amd: a %s tensor on %s was passed to a HIP kernel; there is no CPU fallback' % (tuple(t.shape), t.device))
    return ctypes.c_void_p(t.data_ptr())


_ones = {}


def _one(device):
    """A persistent device scalar 1.0 (the unit cotangent of a total loss)."""
    k = (device.type, device.index)
    if k not in _ones:
        _ones[k] = torch.ones(1, dtype=torch.float32, device=device)
    return _ones[k]


HEADS_COLS = 6 * 193 + 6 * 257          # one GEMM output row: [w1b1 of net 0..5 | w2b2 of net 0..5]
HEADS_W2_OFF = 6 * 193


def _net_ptrs(heads, evec, statics, cls=None):
    """Pointer table over the hyper-network output `heads` [256, 2700] (row stride 2700), evec [6,256] and the 48 static tensors."""
    arr = ((cls or L.DpnNetPtrs) * L.NETS)()
    for k in range(L.NETS):
        arr[k].w1b1 = heads.data_ptr() + k * 193 * 4
        arr[k].w2b2 = heads.data_ptr() + (HEADS_W2_OFF + k * 257) * 4
        arr[k].ld_w1b1 = HEADS_COLS
        arr[k].ld_w2b2 = HEADS_COLS
        arr[k].evec = evec.data_ptr() + k * 256 * 4
        for j, nm in enumerate(STATIC_NAMES):
            setattr(arr[k], nm, statics[k * 8 + j].data_ptr())
    return arr


class _Workspace:
    """Buffers of one forward call that its backward needs again."""

    def __init__(self, n, prec, device, packed=None):
        lib = L.load()
        self.sizes = L.DpnSizes()
        L.check(lib.dpn_sizes(n, prec, ctypes.byref(self.sizes)), 'dpn_sizes')
        self.n, self.prec, self.device = n, prec, device
        # packed: this field's block of a batch packed in ONE launch (_FieldBatch); the forward call then has no packing launch of its own
        self.prepacked = packed is not None
        self.packed = packed if packed is not None else torch.empty(self.sizes.packed, dtype=torch.uint8, device=device)
        self.saved = None

    def alloc_saved(self):
        self.saved = torch.empty(self.sizes.saved, dtype=torch.uint8, device=self.device)


class _Operands(namedtuple('_Operands', 'x y t f pe cd hd ev lab st')):
    """fp32 contiguous device copies of an entry point's x, y, t, f, pe_in, coord_data, heads, evec, labels and statics (_operands)."""

    def nets(self, b=None):
        """Pointer table of the field, or of field b of a batch."""
        return _net_ptrs(self.hd, self.ev, self.st) if b is None else _net_ptrs(self.hd[b], self.ev[b], self.st)


def _operands(what, x, y, t, f, coord_data, heads, evec, statics, pe_in=None, labels=None, batch=False, split=None):
    """The GPU check and the fp32 copies of entry point `what`, before any launch: a host tensor among x, coord_data, heads, labels raises
    (RuntimeError, in that order), then a bad [interior | margin] split = (n_inter, with_pde) (ValueError: every launch takes its row counts
    from it; n_inter = 0 only without the PDE losses).  x, y, t, f come back flat: [N] for one field, [B, N] for a batch (coord_data [B, N, 6],
    heads [B, 256, 2700], evec [B, 6, 256], labels [B, N - n_inter, 6]); absent tensors stay None."""
    for nm, v in (('x', x), ('coord_data', coord_data), ('heads', heads), ('labels', labels)):
        if v is not None:
            require_gpu(v, nm, what)
    if split is not None:
        (n_inter, with_pde), n, n_lab = split, coord_data.shape[int(batch)], labels.shape[int(batch)]
        if not ((0 < n_inter < n if with_pde else 0 <= n_inter < n) and n_lab == n - n_inter):
            raise ValueError('%s: n_inter = %d of %d points leaves %d margin points for %d label rows; need %s n_inter < %d and one label row '
                             'per margin point' % (what, n_inter, n, n - n_inter, n_lab, '0 <' if with_pde else '0 <=', n))
    shape = tuple(coord_data.shape[:2]) if batch else (-1,)
    x_, y_, t_, f_ = (None if v is None else _f32c(v).reshape(shape) for v in (x, y, t, f))
    pe_, cd_, hd_, ev_, lab_ = (None if v is None else _f32c(v) for v in (pe_in, coord_data, heads, evec, labels))
    return _Operands(x_, y_, t_, f_, pe_, cd_, hd_, ev_, lab_, [_f32c(s) for s in statics])


class KernelClock:
    """Measurement aid (bench.py): device-clock stamps around the three point kernels INSIDE a captured step.  While `point_path.clock` holds one,
    every launch of dpn_fwd / dpn_bwd_points / dpn_wgrad through this module is bracketed by two dpn_clock_stamp nodes (one-thread kernels appending
    wall_clock64 to a ring); `durations()` turns the ring into per-kernel microseconds.  The product path runs with `clock = None`."""
    NAMES = ('pair', 'fwd', 'bwd', 'wgrad')          # 'pair': two stamps back to back -- the stamp's own cost, subtracted from the others

    def __init__(self, device, cap=4096):
        self.cap = cap
        self.ring = torch.zeros(cap, dtype=torch.int64, device=device)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=device)
        khz = ctypes.c_int(0)
        L.check(L.load().dpn_clock_rate_khz(ctypes.byref(khz)), 'dpn_clock_rate_khz')
        self.khz = khz.value
        self.order = []                               # names in stamp order within one replay (recorded while capturing)
        self.recording = True

    def stamp(self, name):
        if self.recording:
            self.order.append(name)
        L.check(L.load().dpn_clock_stamp(_ptr(self.ring), _ptr(self.cursor), self.cap, _stream()), 'dpn_clock_stamp')

    def reset(self):
        self.cursor.zero_()
        self.recording = False

    def durations(self):
        """{name: [us per replay]} from the stamps written since reset(); the 'pair' interval of the same replay is subtracted from the kernels'."""
        n = int(self.cursor.item())
        per = len(self.order)
        if per == 0 or n == 0 or n > self.cap or n % per:
            return {}
        t = self.ring[:n].cpu().view(-1, per).double() * (1e3 / self.khz)          # us
        out = {}
        for name in self.NAMES:
            idx = [i for i, nm in enumerate(self.order) if nm == name]
            if len(idx) == 2:
                out[name] = (t[:, idx[1]] - t[:, idx[0]]).tolist()
        pair = out.get('pair')
        if pair:
            for name in ('fwd', 'bwd', 'wgrad'):
                if name in out:
                    out[name] = [v - p_ for v, p_ in zip(out[name], pair)]
        return out


clock = None            # a KernelClock while bench.py captures its instrumented copy of the step


def _forward_points(cfg: PointConfig, ws: _Workspace, nets, x, y, t, pe_in, coord_data, want_jac, want_saved, ref6=None):
    lib = L.load()
    n = coord_data.shape[0]
    dev = coord_data.device
    # the packed form the forward launch reads: fused (A = W1 w2, B = W1 Wd: five GEMMs per point and net) for the hi+lo mode's tile-split kernel,
    # the plain matrices for the ring kernels (plain bf16, caller-encoded coordinates)
    form = lib.dpn_fwd_form(cfg.prec, 0 if pe_in is None else 1)
    if not ws.prepacked:
        L.check(lib.dpn_pack_weights_form(nets, cfg.prec, form, _ptr(ws.packed), _stream()), 'dpn_pack_weights')
    out_n = torch.empty((n, 6), dtype=torch.float32, device=dev)
    # with caller-encoded coordinates the kernel hands back d out / d pe_in [n, 6, 192] in place of the (x, y, t) Jacobian
    jac_n = torch.empty((n, 6, 3 if pe_in is None else 192), dtype=torch.float32, device=dev) if want_jac else None
    if want_saved:
        ws.alloc_saved()
    geo = cfg.geometry()
    # ref6 [N,6]: the reference's separate ref_data argument (VariableNet.forward standalone); None: coord_data's columns (PhysicsNet.forward)
    n_nets = int(getattr(cfg, 'n_nets', 6) or 6)
    if n_nets < 6 and not want_saved and not want_jac:             # VariableNet.forward standalone, inference: only the nets that are asked for
        out_n.zero_()
        L.check(lib.dpn_fwd_ref_nets(_ptr(x), _ptr(y), _ptr(t), _ptr(pe_in), _ptr(coord_data), _ptr(ref6), n, _ptr(_freqs(dev)), ctypes.byref(geo),
                                     _ptr(ws.packed), cfg.prec, n_nets, _ptr(out_n), None, _stream()), 'dpn_fwd_ref_nets')
        return out_n, jac_n
    if clock is not None:
        clock.stamp('pair'), clock.stamp('pair'), clock.stamp('fwd')
    L.check(lib.dpn_fwd_ref(_ptr(x), _ptr(y), _ptr(t), _ptr(pe_in), _ptr(coord_data), _ptr(ref6), n, _ptr(_freqs(dev)), ctypes.byref(geo),
                            _ptr(ws.packed), cfg.prec, _ptr(out_n), _ptr(jac_n), _ptr(ws.saved), _stream()), 'dpn_fwd')
    if clock is not None:
        clock.stamp('fwd')
    return out_n, jac_n


def _forward_derivs(cfg: PointConfig, ws: _Workspace, nets, x, y, t, coord_data, want_saved):
    """out_n [N,6] and its first, second and third derivatives along x, y, t [N,6,3] (physical units) in ONE forward launch (dpn_fwd_ref_derivs)."""
    lib = L.load()
    n = coord_data.shape[0]
    dev = coord_data.device
    if not ws.prepacked:
        L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0), _ptr(ws.packed), _stream()), 'dpn_pack_weights')
    out_n = torch.empty((n, 6), dtype=torch.float32, device=dev)
    jac_n, hess_n, d3_n = (torch.empty((n, 6, 3), dtype=torch.float32, device=dev) for _ in range(3))
    if want_saved:
        ws.alloc_saved()
    geo = cfg.geometry()
    L.check(lib.dpn_fwd_ref_derivs(_ptr(x), _ptr(y), _ptr(t), None, _ptr(coord_data), None, n, _ptr(_freqs(dev)), ctypes.byref(geo), _ptr(ws.packed),
                                   cfg.prec, _ptr(out_n), _ptr(jac_n), _ptr(hess_n), _ptr(d3_n), _ptr(ws.saved), _stream()), 'dpn_fwd_ref_derivs')
    return out_n, jac_n, hess_n, d3_n


def _backward_points(cfg: PointConfig, ws: _Workspace, nets, x, y, t, pe_in, coord_data, g_out, g_jxi, statics, into=None, fork=False, keep=(), g_scale=None,
                     g_hxi=None):
    """Weight gradients from per-point cotangents.  Returns (g_heads [256,2700], g_evec [6,256], [48 static grads]); `into` = the same
    triple preallocated by the caller (a batch of fields writes each field's gradients side by side).

    fork (callers inside an autograd backward pass): the finish stage's second half -- G = S1 w2^T + S2 Wd^T + ..., the gradients of
    cat_fc1.fc.0 / fc.2 and out_fc, static tensors that nothing in the backward pass reads -- goes to the side branch (branch.py) and runs
    beside the hyper-network's and the encoder's backward; `keep` = what that branch reads through raw pointers besides the buffers here.

    (Round 3 had tried a two-stream form with half of dpn_wgrad itself on the side stream: no gain, profiles/round3_two_stream_wgrad.txt.)"""
    lib = L.load()
    n = coord_data.shape[0]
    dev = coord_data.device
    operands = torch.empty(ws.sizes.operands, dtype=torch.uint8, device=dev)
    partials = torch.empty(ws.sizes.partials, dtype=torch.uint8, device=dev)
    geo = cfg.geometry()
    # g_scale: a device scalar multiplied into both cotangent streams as stage 1 reads them (they were formed for a unit cotangent of the total)
    if clock is not None:
        clock.stamp('bwd')
    if g_hxi is not None:           # + the cotangent of the second coordinate derivatives (point_fields_xyt), same launch
        L.check(lib.dpn_bwd_points_derivs(_ptr(x), _ptr(y), _ptr(t), None, _ptr(coord_data), n, _ptr(_freqs(dev)), ctypes.byref(geo), _ptr(ws.packed),
                                          cfg.prec, _ptr(g_out), _ptr(g_jxi), _ptr(g_hxi), _ptr(g_scale), _ptr(ws.saved), _ptr(operands), _stream()),
                'dpn_bwd_points_derivs')
    else:
        L.check(lib.dpn_bwd_points_scaled(_ptr(x), _ptr(y), _ptr(t), _ptr(pe_in), _ptr(coord_data), n, _ptr(_freqs(dev)), ctypes.byref(geo),
                                          _ptr(ws.packed), cfg.prec, _ptr(g_out), _ptr(g_jxi), _ptr(g_scale), _ptr(ws.saved), _ptr(operands), _stream()),
                'dpn_bwd_points')
    if clock is not None:
        clock.stamp('bwd')
    arena = False
    if into is None:
        g_heads = torch.empty((256, HEADS_COLS), dtype=torch.float32, device=dev)
        g_evec = torch.empty((6, 256), dtype=torch.float32, device=dev)
        # the 48 static parameters' gradients go straight into the optimiser's flat gradient buffer when one is registered (grad_arena)
        # (not when one tensor fills several slots -- VariableNet.forward standalone -- whose gradients must stay separate tensors)
        arena = len({s.data_ptr() for s in statics}) == len(statics)
        slots = [slot_of(statics[k * 8 + j]) if arena else None for k in range(6) for j in range(8)]
        g_stat = [s_.view(STATIC_SHAPES[i % 8]) if s_ is not None else torch.empty(STATIC_SHAPES[i % 8], dtype=torch.float32, device=dev)
                  for i, s_ in enumerate(slots)]
        arena = arena and all(s_ is not None for s_ in slots)
    else:
        g_heads, g_evec, g_stat = into
    garr = _net_ptrs(g_heads, g_evec, g_stat, cls=L.DpnNetGradPtrs)
    if clock is not None:
        clock.stamp('wgrad')
    L.check(lib.dpn_wgrad(n, cfg.prec, _ptr(g_out), _ptr(ws.saved), _ptr(operands), _ptr(partials), _stream()), 'dpn_wgrad')
    if clock is not None:
        clock.stamp('wgrad')
    # (only when every static gradient is a freshly leased slot of the optimiser's flat buffer: autograd then keeps the view as param.grad without
    # touching it; a gradient it would have to ADD to an existing one on the main stream must be complete when the node returns)
    if fork and arena and branch.enabled('finish'):
        L.check(lib.dpn_wgrad_finish_parts(nets, _ptr(ws.packed), n, cfg.prec, _ptr(partials), garr, 1, _stream()), 'dpn_wgrad_finish')
        # keep: what the branch READS (not the 48 gradient slots: they are persistent, and a second reference to a returned gradient makes
        # autograd copy it instead of keeping the view as param.grad)
        with branch.side(keep=(partials, ws.packed, statics) + tuple(keep)):
            L.check(lib.dpn_wgrad_finish_parts(nets, _ptr(ws.packed), n, cfg.prec, _ptr(partials), garr, 2, _stream()), 'dpn_wgrad_finish')
    else:
        L.check(lib.dpn_wgrad_finish(nets, _ptr(ws.packed), n, cfg.prec, _ptr(partials), garr, _stream()), 'dpn_wgrad_finish')
    return g_heads, g_evec, g_stat


def _stamp(tensors):
    """Version counters of the tensors a backward pass will read again through raw pointers (the point path keeps them in ctx.ops, not in
    save_for_backward: most are detached fp32 views).  _check_stamp raises when one was modified in place between forward and backward
    (e.g. an optimiser step before a delayed backward), which autograd's own check would catch for saved tensors."""
    from . import grad_arena
    owners = {}
    for t in tensors:                       # fused optimisers that own one of these tensors (they rewrite it through a raw pointer)
        e = grad_arena._slots.get(t.data_ptr()) if t is not None else None
        o = e[0]() if e is not None else None
        if o is not None:
            owners[id(o)] = (e[0], o.steps_done)
    return (('owners', tuple(owners.values())),) + tuple((t, t._version) for t in tensors if t is not None)


def _check_stamp(stamp, what):
    if stamp and stamp[0][0] == 'owners':
        # the fused optimiser rewrites parameters through raw pointers (no version bump): its own step count says whether it ran between
        # this forward and its backward (steps replayed from a hipGraph are invisible to the host: not covered)
        for ref, steps in stamp[0][1]:
            o = ref()
            if o is not None and o.steps_done != steps:
                raise RuntimeError('deepphysinet_amd %s: a fused optimiser step ran between the forward pass and its backward pass' % what)
        stamp = stamp[1:]
    for t, v in stamp:
        if t._version != v:
            raise RuntimeError('deepphysinet_amd %s: a tensor of shape %s needed by the backward pass was modified in place after the '
                               'forward pass (version %d -> %d)' % (what, tuple(t.shape), v, t._version))


class _NoSecondOrder(torch.autograd.Function):
    """Identity whose backward raises: marks a first derivative that cannot be differentiated again."""

    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('deepphysinet_amd: d(fields)/d(coordinates) of PhysicsNet.forward is first-order only; training through the '
                           'standalone *_equation methods needs its parameter derivative -- use InterfacePhysics.place_one_batch (fused '
                           'residual kernels) for that; InterfacePhysics.fields_at (raw x, y, t) gives fields whose coordinate derivatives train')


class _PointFieldsFn(torch.autograd.Function):
    """out_n [N,6] = six VariableNets at N points.  First-order differentiable w.r.t. the weights and -- when the coordinates come in
    already encoded (pe_in, the reference's PhysicsNet.forward surface) -- w.r.t. pe_in, so that the reference's `gradient(u, x)`
    (interface_physics.py:90-95) evaluates on the outputs of the HIP model.  Differentiating such a derivative again (training through the
    standalone equation methods) raises (_NoSecondOrder); place_one_batch is the fused path for that."""

    @staticmethod
    def forward(ctx, cfg, x, y, t, pe_in, coord_data, heads, evec, *statics):
        ops = _operands('point_fields', x, y, t, None, coord_data, heads, evec, statics, pe_in=pe_in)
        need_grad = any(v.requires_grad for v in (heads, evec) + tuple(statics)) and int(getattr(cfg, 'n_nets', 6) or 6) == 6
        want_gpe = pe_in is not None and pe_in.requires_grad        # (n_nets < 6: the caller has established that nothing is differentiated)
        ws = _Workspace(ops.cd.shape[0], cfg.prec, ops.cd.device)
        ref6 = getattr(cfg, 'ref6', None)                 # VariableNet.forward's own ref_data (a constant: no gradient flows to it here)
        out_n, gpe = _forward_points(cfg, ws, ops.nets(), ops.x, ops.y, ops.t, ops.pe, ops.cd, want_jac=want_gpe, want_saved=need_grad,
                                     ref6=None if ref6 is None else _f32c(ref6.detach()))
        ctx.cfg, ctx.ws, ctx.gpe, ctx.ops = cfg, ws, gpe, ops
        ctx.stamp = _stamp((heads, evec) + tuple(statics))
        return out_n

    @staticmethod
    def backward(ctx, g_out):
        _check_stamp(ctx.stamp, 'point_fields')
        ops = ctx.ops
        st = ops.st
        g = _f32c(g_out)
        g_pe = None
        if ctx.needs_input_grad[4] and ctx.gpe is not None:
            g_pe = torch.empty((g.shape[0], 192), dtype=torch.float32, device=g.device)
            L.check(L.load().dpn_contract_gpe(_ptr(g), _ptr(ctx.gpe), g.shape[0], _ptr(g_pe), _stream()), 'dpn_contract_gpe')
            if torch.is_grad_enabled():                # create_graph=True (the reference's gradient()): a later backward through this
                g_pe = _NoSecondOrder.apply(g_pe.requires_grad_(True))      # derivative must fail loudly, not drop its parameter part
        if not any(ctx.needs_input_grad[6:]):
            return (None, None, None, None, g_pe) + (None,) * (3 + len(st))
        ghd, gev, gst = _backward_points(ctx.cfg, ctx.ws, ops.nets(), ops.x, ops.y, ops.t, ops.pe, ops.cd, g, None, st, fork=True,
                                         keep=(ops.hd, ops.ev))
        return (None, None, None, None, g_pe, None, ghd, gev, *gst)


class _PointDerivsFn(torch.autograd.Function):
    """Core node of point_fields_xyt: (out [N,6], J, H, D3 [N,6,3]) as functions of the WEIGHTS (the coordinates are constants here; _AttachFn
    makes them functions of x, y, t).  J, H, D3 = first, second, third derivatives of out along x, y, t (physical units), all from one forward
    launch.  The backward takes the cotangents of out, J and H -- autograd has added up every use of them before this node runs, so one
    loss.backward() is ONE point backward -- and makes one dpn_bwd_points_derivs call, then the usual weight-gradient and finish launches."""

    @staticmethod
    def forward(ctx, cfg, x, y, t, coord_data, heads, evec, *statics):
        ops = _operands('point_fields_xyt', x, y, t, None, coord_data, heads, evec, statics)
        need_grad = any(v.requires_grad for v in (heads, evec) + tuple(statics))
        ws = _Workspace(ops.cd.shape[0], cfg.prec, ops.cd.device)
        out_n, jac_n, hess_n, d3_n = _forward_derivs(cfg, ws, ops.nets(), ops.x, ops.y, ops.t, ops.cd, want_saved=need_grad)
        ctx.cfg, ctx.ws, ctx.ops = cfg, ws, ops
        ctx.stamp = _stamp((heads, evec) + tuple(statics))
        ctx.set_materialize_grads(False)
        return out_n, jac_n, hess_n, d3_n

    @staticmethod
    def backward(ctx, g_out, g_jac, g_hess, g_d3):
        if g_d3 is not None:
            raise RuntimeError(_ORDER_LIMIT)
        ops = ctx.ops
        if not any(ctx.needs_input_grad[5:]) or (g_out is None and g_jac is None and g_hess is None):
            return (None,) * (7 + len(ops.st))
        _check_stamp(ctx.stamp, 'point_fields_xyt')
        cfg = ctx.cfg
        n, dev = ops.cd.shape[0], ops.cd.device
        g = torch.zeros((n, 6), dtype=torch.float32, device=dev) if g_out is None else _f32c(g_out)
        # the kernels take the derivative cotangents along the NORMALISED coordinates xi = x / dx / (lon - 1), y / dy / (lat - 1), t / span:
        # d J / d J_xi = 1 / (dx (lon - 1)) per coordinate, squared for the second derivatives
        s1 = _xi_scale(cfg, dev)
        g_jxi = None if g_jac is None else (_f32c(g_jac) * s1).contiguous()
        g_hxi = None if g_hess is None else (_f32c(g_hess) * (s1 * s1)).contiguous()
        ghd, gev, gst = _backward_points(cfg, ctx.ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, g, g_jxi, ops.st, fork=True,
                                         keep=(ops.hd, ops.ev), g_hxi=g_hxi)
        return (None,) * 5 + (ghd, gev, *gst)


_ORDER_LIMIT = ('deepphysinet_amd point_fields_xyt: the fields are differentiable in (x, y, t) up to third order and train losses that contain '
                'derivatives up to second order; a third derivative cannot be differentiated again (neither to a fourth derivative nor w.r.t. the '
                'weights)')
_xi_scales = {}


def _xi_scale(cfg: PointConfig, device):
    """[3] = 1 / (dx (lon - 1)), 1 / (dy (lat - 1)), 1 / pred_t_span as an fp32 device tensor: d (physical derivative) / d (xi derivative)."""
    key = (float(cfg.dx), float(cfg.dy), int(cfg.lon_size), int(cfg.lat_size), float(cfg.pred_t_span), str(device))
    if key not in _xi_scales:
        v = [1.0 / (cfg.dx * (cfg.lon_size - 1)), 1.0 / (cfg.dy * (cfg.lat_size - 1)), 1.0 / cfg.pred_t_span]
        _xi_scales[key] = torch.tensor(v, dtype=torch.float64).float().to(device)
    return _xi_scales[key]


class _AttachFn(torch.autograd.Function):
    """v as a function of the coordinates too: the identity on v, and the coordinate cotangent sum_k g[:, k, c] * nxt[:, k, c], where nxt is the
    next order's tensor, itself attached: d out / d x_c = J[..., c]; d J[..., c] / d x_c' = delta_cc' H[..., c] (each PE channel depends on one
    coordinate and the nets are piecewise linear in it: the mixed partials are zero); d H / d x = D3.  The cotangent is a torch expression in
    nxt, so under create_graph it is differentiable again, by the same rule one order up.  nxt travels in a tuple: it is not an input of this
    node (v does not depend on it), so a backward pass through v never visits nxt's own node."""

    @staticmethod
    def forward(ctx, v, x, y, t, nxt):
        ctx.nxt = nxt[0]
        ctx.shapes = (x.shape, y.shape, t.shape)
        ctx.set_materialize_grads(False)
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        gx = gy = gt = None
        if any(ctx.needs_input_grad[1:4]):
            gc = ((g if g.dim() == 3 else g.unsqueeze(2)) * ctx.nxt).sum(1)          # [N, 3]
            gx, gy, gt = (gc[:, c].reshape(shape) for c, shape in enumerate(ctx.shapes))
        return g, gx, gy, gt, None


class _OrderLimitFn(torch.autograd.Function):
    """Identity on the third derivatives (and a function of x, y, t, so that it is part of every coordinate graph); a cotangent that reaches it
    raises."""

    @staticmethod
    def forward(ctx, d3, x, y, t):
        ctx.set_materialize_grads(False)
        return d3.view_as(d3)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        raise RuntimeError(_ORDER_LIMIT)


def point_fields_xyt(cfg: PointConfig, x, y, t, coord_data, heads, evec, statics):
    """Normalised fields out_n [N,6] at raw coordinates x, y, t ([N] or [N,1]), differentiable w.r.t. every weight input AND w.r.t. x, y, t: first
    derivatives with create_graph=True, second derivatives, and the coordinate gradient of a loss that contains second derivatives.  Every
    derivative comes from ONE forward launch (dpn_fwd_ref_derivs); a backward pass through all of them is ONE point backward (_PointDerivsFn).
    Mixed partials are zero; a third derivative cannot be differentiated again (RuntimeError)."""
    out, jac, hess, d3 = _PointDerivsFn.apply(cfg, x.detach(), y.detach(), t.detach(), coord_data, heads, evec, *statics)
    d3 = _OrderLimitFn.apply(d3, x, y, t)
    hess = _AttachFn.apply(hess, x, y, t, (d3,))
    jac = _AttachFn.apply(jac, x, y, t, (hess,))
    return _AttachFn.apply(out, x, y, t, (jac,))


def _causal_group(cfg, causal, out_n, jac_n, f_, t_, a0, a1):
    """Causal time weights of the row group (a0, a1) (causal: a causal.CausalWeights): dpn_causal_bins, then dpn_causal_weights.  Returns
    (bin [m] int32, W32 [bins] fp32, diag [3 bins + 2] fp64), all on the device; nothing is read back."""
    lib = L.load()
    m, bins, dev = a1 - a0, int(causal.bins), out_n.device
    t_lo, t_hi = causal.bounds(cfg.pred_t_span)
    geo, ph = cfg.geometry(), cfg.physics()
    fac = (ctypes.c_double * 6)(*[float(v) for v in cfg.factors])
    bin_ = torch.empty(m, dtype=torch.int32, device=dev)
    rows = torch.empty(int(lib.dpn_causal_rows_doubles(m, bins)), dtype=torch.float64, device=dev)
    w32 = torch.empty(bins, dtype=torch.float32, device=dev)
    diag = torch.empty(3 * bins + 2, dtype=torch.float64, device=dev)
    L.check(lib.dpn_causal_bins(_ptr(out_n[a0:]), _ptr(jac_n[a0:]), _ptr(f_[a0:]), _ptr(t_[a0:]), m, ctypes.byref(geo), ctypes.byref(ph), fac,
                                float(t_lo), float(t_hi), bins, _ptr(bin_), _ptr(rows), _stream()), 'dpn_causal_bins')
    L.check(lib.dpn_causal_weights(_ptr(rows), m, bins, float(causal.eps), int(causal.relative), _ptr(w32), _ptr(diag), _stream()),
            'dpn_causal_weights')
    return bin_, w32, diag


def _point_weights(what, w, n, device):
    """A caller's per-point weights as an fp32 contiguous device tensor [n] (constants: detached)."""
    require_gpu(w, 'point weights', what)
    w = _f32c(w).reshape(-1)
    if w.shape[0] != n:
        raise ValueError('%s: %d point weights for %d points' % (what, w.shape[0], n))
    return w


def _group_weights(what, cfg, extra, out_n, jac_n, f_, t_, groups):
    """Per row group (a0, a1) the weight sources of dpn_residual_weighted: (w [m] or None, bin or None, W32 or None), or None for a group with
    neither (it takes the plain dpn_residual); None for extra None (_weight_options: no option given, nothing is launched or allocated).
    extra = (the caller's weights of the FIRST group or None, causal or None, a list that receives the groups' diag tensors or None); causal: bins
    and weights per group, each group its own (_causal_group)."""
    if extra is None:
        return None
    given, causal, diag_out = extra
    if given is not None:
        given = _point_weights(what, given, groups[0][1] - groups[0][0], out_n.device)
    out, diags = [], []
    for gi, (a0, a1) in enumerate(groups):
        w = given if gi == 0 else None
        bin_ = w32 = diag = None
        if causal is not None:
            bin_, w32, diag = _causal_group(cfg, causal, out_n, jac_n, f_, t_, a0, a1)
        out.append(None if (w is None and bin_ is None) else (w, bin_, w32))
        diags.append(diag)
    if diag_out is not None:
        diag_out[:] = diags
    return out


def _residual_launch(what, geo, ph, out_n, jac_n, f_, m, gl, gt, sums, g_out, g_jxi, wt):
    """One residual launch over the m points at the head of out_n, jac_n, f_ (a group's slices; gl [6], gt [1]: fp32 device cotangents; sums,
    g_out, g_jxi: what the launch writes; each may be None).  wt None: dpn_residual; wt = (w, bin, W32) (_group_weights): dpn_residual_weighted,
    the same arguments and the three weight sources.  what: '' or '(grad)', for the error message."""
    name, sources = ('dpn_residual', ()) if wt is None else ('dpn_residual_weighted', tuple(_ptr(v) for v in wt))
    L.check(getattr(L.load(), name)(_ptr(out_n), _ptr(jac_n), _ptr(f_), m, ctypes.byref(geo), ctypes.byref(ph), _ptr(gl), _ptr(gt), _ptr(sums),
                                    _ptr(g_out), _ptr(g_jxi), *sources, _stream()), name + what)


def _residual_losses(cfg, out_n, jac_n, f_, groups, losses, unit=None, sums=None, weights=None):
    """The residual-loss sums of row groups (a0, a1) of out_n [n, 6], jac_n [n, 6, 3], f_ [n]: per group one residual launch (_residual_launch)
    into per-block rows and one dpn_residual_finish into its `losses` row [7] (the six scaled terms, their total).  unit = (scale, g_out, g_jxi):
    the same pass over the points also writes d total / d (out, Jacobian) for the cotangent `scale` (a device 1.0) of the total.  sums: the block
    rows of one group given by the caller; losses None leaves them to a later finish launch (_residual_finish, or dpn_residual_finish_batch for a
    batch).  weights: per group None or (w, bin, W32) (_group_weights): same rows, same finish."""
    geo, ph = cfg.geometry(), cfg.physics()
    for gi, (a0, a1) in enumerate(groups):
        m = a1 - a0
        s_ = torch.empty(((m + 255) // 256) * 6, dtype=torch.float64, device=out_n.device) if sums is None else sums
        sc, g_out, g_jxi = (None, None, None) if unit is None else (unit[0], unit[1][a0:], unit[2][a0:])
        _residual_launch('', geo, ph, out_n[a0:], jac_n[a0:], f_[a0:], m, None, sc, s_, g_out, g_jxi, None if weights is None else weights[gi])
        if losses is not None:
            _residual_finish(cfg, s_, m, losses[gi])


def _residual_finish(cfg, sums, n, losses):
    ph = cfg.physics()
    L.check(L.load().dpn_residual_finish(_ptr(sums), n, ctypes.byref(ph), _ptr(losses), _stream()), 'dpn_residual_finish')


def _residual_cotangent(cfg, out_n, jac_n, f_, groups, g_out=None, g_jxi=None, weights=None):
    """d loss / d (out, Jacobian) of the residual losses (the residual launch in gradient mode) into g_out [n, 6], g_jxi [n, 6, 3] (allocated when
    not given), group by group: groups = [(a0, a1, cotangent of the terms [6] or None, cotangent of the total [1] or None)]; a group with neither
    takes a zero cotangent on its terms (its rows are written all the same).  weights: per group None or (w, bin, W32), the weight sources the
    forward pass used (saved, never recomputed).  Returns (g_out, g_jxi)."""
    n, dev = out_n.shape[0], out_n.device
    g_out = torch.empty((n, 6), dtype=torch.float32, device=dev) if g_out is None else g_out
    g_jxi = torch.empty((n, 6, 3), dtype=torch.float32, device=dev) if g_jxi is None else g_jxi
    geo, ph = cfg.geometry(), cfg.physics()
    zero6 = None
    for gi, (a0, a1, gl, gt) in enumerate(groups):
        if gl is None and gt is None:
            zero6 = torch.zeros(6, dtype=torch.float32, device=dev) if zero6 is None else zero6
            gl = zero6
        _residual_launch('(grad)', geo, ph, out_n[a0:], jac_n[a0:], f_[a0:], a1 - a0, None if gl is None else _f32c(gl),
                         None if gt is None else _f32c(gt).reshape(1), None, g_out[a0:], g_jxi[a0:], None if weights is None else weights[gi])
    return g_out, g_jxi


class _PdeLossFn(torch.autograd.Function):
    """losses [6] = (motion_u, motion_v, continuous, energy, vapor, gas), each already scaled by its factor."""

    @staticmethod
    def forward(ctx, cfg, extra, x, y, t, f, coord_data, heads, evec, *statics):
        # extra: None (the launches of before), or (point weights [n] or None, causal.CausalWeights or None, a list that receives the diag tensor)
        ops = _operands('pde_losses', x, y, t, f, coord_data, heads, evec, statics)
        n, dev = ops.cd.shape[0], ops.cd.device
        need_grad = any(v.requires_grad for v in (heads, evec) + tuple(statics))
        ws = _Workspace(n, cfg.prec, dev)
        out_n, jac_n = _forward_points(cfg, ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, want_jac=True, want_saved=need_grad)
        losses = torch.empty((1, 7), dtype=torch.float32, device=dev)
        # With gradients wanted, the SAME pass over the points also writes d total / d (out, Jacobian) for a unit cotangent of the total (the usual
        # backward: loss.backward(seed) on the sum of the six terms): the backward pass then has no residual launch of its own, stage 1 multiplies
        # the cotangent that arrives into the streams as it reads them (dpn_bwd_points_scaled).  A cotangent on the individual terms takes the
        # separate pass, as before.
        ctx.unit = None
        if need_grad:
            ctx.unit = (torch.empty((n, 6), dtype=torch.float32, device=dev), torch.empty((n, 6, 3), dtype=torch.float32, device=dev))
        # bins, weights, then the weighted residual pass; bin, W32 and the caller's w stay in ctx for the backward pass
        ctx.weights = _group_weights('pde_losses', cfg, extra, out_n, jac_n, ops.f, ops.t, ((0, n),))
        _residual_losses(cfg, out_n, jac_n, ops.f, ((0, n),), losses, unit=None if ctx.unit is None else (_one(dev),) + ctx.unit,
                         weights=ctx.weights)
        ctx.cfg, ctx.ws, ctx.ops, ctx.fields = cfg, ws, ops, (out_n, jac_n)
        ctx.stamp = _stamp((heads, evec) + tuple(statics))
        ctx.set_materialize_grads(False)
        return losses[0, :6], losses[0, 6]

    @staticmethod
    def backward(ctx, g_losses, g_total):
        cfg, ops = ctx.cfg, ctx.ops
        _check_stamp(ctx.stamp, 'pde_losses')
        gl = None if g_losses is None else _f32c(g_losses)
        gt = None if g_total is None else _f32c(g_total).reshape(1)
        if gl is None and gt is None:
            return (None,) * (9 + len(ops.st))
        if gl is None and ctx.unit is not None:                  # cotangent on the total only: the unit-cotangent streams of the forward pass, scaled on load
            g_out, g_jxi = ctx.unit
            ghd, gev, gst = _backward_points(cfg, ctx.ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, g_out, g_jxi, ops.st, fork=True,
                                             keep=(ops.hd, ops.ev), g_scale=gt)
            return (None, None, None, None, None, None, None, ghd, gev, *gst)
        out_n, jac_n = ctx.fields
        g_out, g_jxi = _residual_cotangent(cfg, out_n, jac_n, ops.f, ((0, ops.cd.shape[0], gl, gt),), weights=ctx.weights)
        ghd, gev, gst = _backward_points(cfg, ctx.ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, g_out, g_jxi, ops.st, fork=True,
                                         keep=(ops.hd, ops.ev))
        return (None, None, None, None, None, None, None, ghd, gev, *gst)


_STATIC_STARTS = [0]                    # offsets of the 48 static tensors in a flat gradient row
for _i in range(48):
    _STATIC_STARTS.append(_STATIC_STARTS[-1] + int(torch.Size(STATIC_SHAPES[_i % 8]).numel()))


def _static_views(flat):
    """The 48 static-parameter gradients as views of one flat row [_STATIC_STARTS[-1]]."""
    return [flat[_STATIC_STARTS[i]:_STATIC_STARTS[i + 1]].view(STATIC_SHAPES[i % 8]) for i in range(48)]


class _FieldBatch:
    """B fields of one batch (ops: _operands with batch=True) for n-point forwards: field b's workspace and pointer table, and the weight
    gradients of all B fields side by side (heads [B, 256, 2700], evec [B, 6, 256], statics flat [B, 48 tensors]).  pack: every field's
    weight block in ONE launch (dpn_pack_weights_batch), issued here in front of whatever the caller launches next; otherwise each field's forward packs
    its own."""

    def __init__(self, cfg, ops, n, pack):
        self.cfg, self.ops, self.n = cfg, ops, n
        self.packed = None
        if pack:            # row b of packed [B, stride] is field b's _Workspace.packed (per field the launch is 17 us of latency-bound tiles: DESIGN.md 6a)
            lib, B = L.load(), ops.hd.shape[0]
            stride = (point_sizes(n, cfg.prec)[1] + 255) // 256 * 256
            self.packed = torch.empty((B, stride), dtype=torch.uint8, device=ops.hd.device)
            L.check(lib.dpn_pack_weights_batch(ops.nets(0), B, ops.hd.stride(0), ops.ev.stride(0), cfg.prec, lib.dpn_fwd_form(cfg.prec, 0),
                                               _ptr(self.packed), stride, _stream()), 'dpn_pack_weights_batch')

    def field(self, b):
        ws = _Workspace(self.n, self.cfg.prec, self.ops.cd.device, packed=None if self.packed is None else self.packed[b])
        return ws, self.ops.nets(b)

    def grads(self):
        B, dev = self.ops.hd.shape[0], self.ops.cd.device
        return (torch.empty((B, 256, HEADS_COLS), dtype=torch.float32, device=dev), torch.empty((B, 6, 256), dtype=torch.float32, device=dev),
                torch.empty((B, _STATIC_STARTS[-1]), dtype=torch.float32, device=dev))


class _PdeLossBatchFn(torch.autograd.Function):
    """BASELINE configs[2]: B field samples (distinct field / lead time => distinct hyper-network weights) with N collocation points each
    in ONE step.  losses [B, 6] and totals [B]; heads [B, 256, 2700], evec [B, 6, 256], point tensors [B, N(,6)].  The point kernels run
    field after field (each launch already fills the chip); the static-parameter gradients of the fields are written side by side and
    added in a fixed order by one dpn_sum_parts launch, so nothing is accumulated through autograd.

    When gradients are wanted, each field's point BACKWARD runs right behind its forward, for a unit cotangent of that field's total
    (the gradients are linear in it; the backward pass scales them by the cotangent that arrives): the field's saved state (0.35 GB) is
    consumed while it is still warm in the memory-side cache and freed at once, instead of 61 of them (21 GB) waiting for the backward
    pass -- measured on the stage-1 backward kernel: 252 us per field at 2 fields, 273 at 8, 293 at 24, 295 at 61 with the state parked, 249
    at 61 this way; the 61-field step 80.5 -> 78.6 ms on the same box.  A
    cotangent on the individual loss terms (not only on the totals) takes the general path: forward again, field by field."""

    @staticmethod
    def forward(ctx, cfg, grad_enabled, x, y, t, f, coord_data, heads, evec, *statics):
        ops = _operands('pde_losses_batch', x, y, t, f, coord_data, heads, evec, statics, batch=True)
        B, n = ops.cd.shape[0], ops.cd.shape[1]
        dev = ops.cd.device
        # Function.forward always runs with grad mode off: the caller's mode arrives as an argument (pde_losses_batch), so that a no-grad
        # evaluation (validation, place_lead_batch scoring) neither saves state nor runs each field's point backward
        need_grad = bool(grad_enabled) and any(v.requires_grad for v in (heads, evec) + tuple(statics))
        eager = need_grad and config.FROZEN.batch_eager_backward
        losses7 = torch.empty((B, 7), dtype=torch.float32, device=dev)
        sums = torch.empty((B, ((n + 255) // 256) * 6), dtype=torch.float64, device=dev)      # per field: block rows, all reduced by ONE launch behind the loop
        fields = []
        one_launch = config.FROZEN.batch_pack                     # every field's weight block: one launch in front of the loop
        batch = _FieldBatch(cfg, ops, n, pack=one_launch)
        unit = grads = None
        if eager:
            unit = (torch.ones(1, dtype=torch.float32, device=dev), torch.empty((n, 6), dtype=torch.float32, device=dev),
                    torch.empty((n, 6, 3), dtype=torch.float32, device=dev))
            grads = batch.grads()
        for b in range(B):
            ws, nets = batch.field(b)
            out_n, jac_n = _forward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], want_jac=True, want_saved=need_grad)
            # eager: the block sums of the losses AND d total_b / d (out, Jacobian) for a unit cotangent in ONE pass over the points
            _residual_losses(cfg, out_n, jac_n, ops.f[b], ((0, n),), None, unit=unit, sums=sums[b])
            if eager:                                             # d total_b / d (this field's weights)
                _backward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], unit[1], unit[2], ops.st,
                                 into=(grads[0][b], grads[1][b], _static_views(grads[2][b])))
                del ws, out_n, jac_n
            elif need_grad:
                fields.append((ws, out_n, jac_n))
            if not one_launch:
                _residual_finish(cfg, sums[b], n, losses7[b])
        if one_launch:
            ph = cfg.physics()
            L.check(L.load().dpn_residual_finish_batch(_ptr(sums), n, B, ctypes.byref(ph), _ptr(losses7), _stream()), 'dpn_residual_finish')
        ctx.cfg, ctx.fields, ctx.eager, ctx.ops = cfg, fields, grads, ops
        ctx.stamp = _stamp((heads, evec) + tuple(statics))
        ctx.set_materialize_grads(False)
        return losses7[:, :6], losses7[:, 6]

    @staticmethod
    def backward(ctx, g_losses, g_total):
        cfg, ops = ctx.cfg, ctx.ops
        _check_stamp(ctx.stamp, 'pde_losses_batch')
        B, n = ops.cd.shape[0], ops.cd.shape[1]
        dev = ops.cd.device
        if g_losses is None and g_total is None:
            return (None,) * (9 + len(ops.st))
        if ctx.eager is not None and g_losses is None:
            # the gradients are there for unit cotangents of the B totals: scale them by the cotangents that arrived
            g_heads, g_evec, flat = ctx.eager
            ctx.eager = None
            gt = _f32c(g_total).reshape(B)
            g_heads.mul_(gt.view(B, 1, 1))
            g_evec.mul_(gt.view(B, 1, 1))
            flat.mul_(gt.view(B, 1))
        else:
            gl = None if g_losses is None else _f32c(g_losses)
            gt = None if g_total is None else _f32c(g_total)
            g_out = torch.empty((n, 6), dtype=torch.float32, device=dev)
            g_jxi = torch.empty((n, 6, 3), dtype=torch.float32, device=dev)
            recompute = ctx.eager is not None                      # cotangents on the individual terms: the general path, forward again
            ctx.eager = None
            if not recompute and (len(ctx.fields) != B or any(fld is None for fld in ctx.fields)):
                raise RuntimeError('deepphysinet_amd pde_losses_batch: the per-field state saved by the forward pass is released as the backward '
                                   'pass consumes it (21 GB at 61 fields); run the forward pass again instead of a second backward')
            batch = _FieldBatch(cfg, ops, n, pack=False)           # (the recompute packs field by field, in its forward launches)
            g_heads, g_evec, flat = batch.grads()
            for b in range(B):
                if recompute:
                    ws, nets = batch.field(b)
                    out_n, jac_n = _forward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], want_jac=True, want_saved=True)
                else:
                    (ws, out_n, jac_n), nets = ctx.fields[b], ops.nets(b)
                _residual_cotangent(cfg, out_n, jac_n, ops.f[b], ((0, n, None if gl is None else gl[b], None if gt is None else gt[b:b + 1]),),
                                    g_out, g_jxi)
                _backward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], g_out, g_jxi, ops.st,
                                 into=(g_heads[b], g_evec[b], _static_views(flat[b])))
                if not recompute:
                    ctx.fields[b] = None                          # this field's saved state is no longer needed
        total = torch.empty(_STATIC_STARTS[-1], dtype=torch.float32, device=dev)
        L.check(L.load().dpn_sum_parts(_ptr(flat), B, _STATIC_STARTS[-1], 0, _ptr(total), _stream()), 'dpn_sum_parts')
        return (None, None, None, None, None, None, None, g_heads, g_evec, *_static_views(total))


def _step_pass(what, cfg, ws, nets, n_inter, x_, y_, t_, f_, cd_, losses, want_saved=False, extra=None):
    """The step body's point pass over [interior | margin] rows (the first n_inter interior): ONE forward with the Jacobian, then the residual-loss
    sums of the two groups into losses [2, 7].  _StepLossFn.forward (want_saved, for its backward) and eval_step(_batch) both run exactly this, so
    their PDE losses are the same bitwise.  extra (_weight_options): per group bins, weights, the weighted residual pass, finish; interior and
    margin each their own bins and weights.  Returns (out_n, jac_n, the groups' weight sources or None)."""
    out_n, jac_n = _forward_points(cfg, ws, nets, x_, y_, t_, None, cd_, want_jac=True, want_saved=want_saved)
    groups = ((0, n_inter), (n_inter, cd_.shape[0]))
    weights = _group_weights(what, cfg, extra, out_n, jac_n, f_, t_, groups)
    _residual_losses(cfg, out_n, jac_n, f_, groups, losses, weights=weights)
    return out_n, jac_n, weights


class _StepLossFn(torch.autograd.Function):
    """The loss of the reference's step body (interface_physics.py:464-501) in ONE point pass: the first n_inter points are the interior
    collocation points, the rest the margin (grid-node, labelled) points.  Returns (inter_terms [6], inter_total, margin_terms [6],
    margin_total, data_loss): the PDE means are taken per group, the SmoothL1 data loss over the margin points; the margin points'
    forward serves both of their losses, and all 24 576 points share one backward / weight-gradient / finish sequence."""

    @staticmethod
    def forward(ctx, cfg, extra, n_inter, beta, margin_factor, x, y, t, f, coord_data, labels, heads, evec, *statics):
        # extra: None (the launches of before), or (interior point weights [n_inter] or None, causal.CausalWeights or None, a list that receives
        # the diag tensors of the two groups)
        ops = _operands('step_losses', x, y, t, f, coord_data, heads, evec, statics, labels=labels, split=(n_inter, True))
        n = ops.cd.shape[0]
        n_m = n - n_inter
        dev = ops.cd.device
        need_grad = any(v.requires_grad for v in (heads, evec) + tuple(statics))
        ws = _Workspace(n, cfg.prec, dev)
        losses = torch.empty((2, 7), dtype=torch.float32, device=dev)
        # the data loss below is not weighted
        out_n, jac_n, ctx.weights = _step_pass('step_losses', cfg, ws, ops.nets(), n_inter, ops.x, ops.y, ops.t, ops.f, ops.cd, losses,
                                               want_saved=need_grad, extra=extra)
        dsum = torch.empty((n_m * 6 + 255) // 256, dtype=torch.float64, device=dev)
        L.check(L.load().dpn_smooth_l1(_ptr(out_n[n_inter:]), _ptr(ops.lab), n_m, beta, 1.0, _ptr(dsum), None, 0, None, _stream()), 'dpn_smooth_l1')
        data = (dsum.sum() / (6.0 * n_m)).float() * margin_factor
        ctx.cfg, ctx.ws, ctx.n_inter, ctx.beta, ctx.margin_factor = cfg, ws, n_inter, beta, margin_factor
        ctx.ops, ctx.fields = ops, (out_n, jac_n)
        ctx.stamp = _stamp((heads, evec) + tuple(statics))
        ctx.set_materialize_grads(False)
        return losses[0, :6], losses[0, 6], losses[1, :6], losses[1, 6], data

    @staticmethod
    def backward(ctx, g_la, g_ta, g_lb, g_tb, g_data):
        cfg, n_inter, ops = ctx.cfg, ctx.n_inter, ctx.ops
        _check_stamp(ctx.stamp, 'step_losses')
        out_n, jac_n = ctx.fields
        n = ops.cd.shape[0]
        n_m = n - n_inter
        if all(v is None for v in (g_la, g_ta, g_lb, g_tb, g_data)):
            return (None,) * (13 + len(ops.st))
        g_out, g_jxi = _residual_cotangent(cfg, out_n, jac_n, ops.f, ((0, n_inter, g_la, g_ta), (n_inter, n, g_lb, g_tb)), weights=ctx.weights)
        if g_data is not None:                                # + d(data loss)/d out on the margin rows
            L.check(L.load().dpn_smooth_l1(_ptr(out_n[n_inter:]), _ptr(ops.lab), n_m, ctx.beta, ctx.margin_factor / (6.0 * n_m), None,
                                           _ptr(g_out[n_inter:]), 1, _ptr(_f32c(g_data).reshape(1)), _stream()), 'dpn_smooth_l1(grad)')
        ghd, gev, gst = _backward_points(cfg, ctx.ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, g_out, g_jxi, ops.st, fork=True,
                                         keep=(ops.hd, ops.ev))
        return (None,) * 11 + (ghd, gev, *gst)


class _StepLossBatchFn(torch.autograd.Function):
    """The step body (_StepLossFn: data loss on the margin rows, PDE means of the interior and of the margin group) for B field samples in ONE
    optimiser step; tensors carry a leading B (eval_step_batch's shapes).  Built like _PdeLossBatchFn's eager path: the B weight blocks are packed in
    one launch, then field after field one forward over the [interior | margin] rows (the tiles of step_losses and eval_step), ONE dpn_step_residual
    (both groups' block rows, the data sums and, with gradients wanted, d total_b / d (out, Jacobian) for a unit cotangent), and right behind it the
    field's point backward: its saved state is consumed warm and freed, never parked.  One dpn_step_finish_batch behind the loop writes every
    field's 16 losses.  Returns losses [B, 16] (include/dpn_hip.h) and totals [B]; only the totals carry gradient: the backward pass scales the
    gradient blocks by the cotangents that arrive and adds the static gradients in a fixed order (dpn_sum_parts)."""

    @staticmethod
    def forward(ctx, cfg, grad_enabled, n_inter, beta, margin_factor, x, y, t, f, coord_data, labels, heads, evec, *statics):
        ops = _operands('step_losses_batch', x, y, t, f, coord_data, heads, evec, statics, labels=labels, batch=True, split=(n_inter, True))
        lib = L.load()
        B, n = ops.cd.shape[0], ops.cd.shape[1]
        n_m, dev = n - n_inter, ops.cd.device
        # (Function.forward runs with grad mode off: the caller's mode arrives as an argument, as in _PdeLossBatchFn)
        need_grad = bool(grad_enabled) and any(v.requires_grad for v in (heads, evec) + tuple(statics))
        geo, ph = cfg.geometry(), cfg.physics()
        losses = torch.empty((B, L.STEP_LOSSES), dtype=torch.float32, device=dev)
        rows = torch.empty((B, int(lib.dpn_step_rows_doubles(n_inter, n))), dtype=torch.float64, device=dev)
        batch = _FieldBatch(cfg, ops, n, pack=True)
        g_out = g_jxi = grads = None
        if need_grad:
            g_out, g_jxi = torch.empty((n, 6), dtype=torch.float32, device=dev), torch.empty((n, 6, 3), dtype=torch.float32, device=dev)
            grads = batch.grads()
        for b in range(B):
            ws, nets = batch.field(b)
            out_n, jac_n = _forward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], want_jac=True, want_saved=need_grad)
            L.check(lib.dpn_step_residual(_ptr(out_n), _ptr(jac_n), _ptr(ops.f[b]), _ptr(ops.lab[b]), n_inter, n, ctypes.byref(geo), ctypes.byref(ph),
                                          beta, margin_factor / (6.0 * n_m), _ptr(_one(dev)), _ptr(rows[b]), _ptr(g_out), _ptr(g_jxi), _stream()),
                    'dpn_step_residual')
            if need_grad:                                         # d total_b / d (this field's weights)
                _backward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], g_out, g_jxi, ops.st,
                                 into=(grads[0][b], grads[1][b], _static_views(grads[2][b])))
            del ws, out_n, jac_n
        L.check(lib.dpn_step_finish_batch(_ptr(rows), n_inter, n, B, ctypes.byref(ph), margin_factor, _ptr(losses), _stream()), 'dpn_step_finish_batch')
        ctx.grads, ctx.n_static = grads, len(statics)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(losses)
        return losses, losses[:, 15].clone()

    @staticmethod
    def backward(ctx, _g_losses, g_total):
        if g_total is None:
            return (None,) * (13 + ctx.n_static)
        return (None,) * 11 + _scaled_batch_grads(ctx, 'step_losses_batch', g_total)


def _scaled_batch_grads(ctx, what, g_total):
    """The backward pass of a batch whose forward pass ran every field's point backward for a unit cotangent of its total (ctx.grads: heads
    [B, 256, 2700], evec [B, 6, 256], statics flat [B, ...]): the blocks times the cotangents that arrived, the static gradients added over the
    fields in a fixed order (dpn_sum_parts).  -> (g_heads, g_evec, the 48 static gradients)."""
    if ctx.grads is None:
        raise RuntimeError('deepphysinet_amd %s: the per-field state saved by the forward pass is released as the backward '
                           'pass consumes it (21 GB at 61 fields); run the forward pass again instead of a second backward' % what)
    g_heads, g_evec, flat = ctx.grads
    ctx.grads = None
    B = flat.shape[0]
    gt = _f32c(g_total).reshape(B)
    g_heads.mul_(gt.view(B, 1, 1))
    g_evec.mul_(gt.view(B, 1, 1))
    flat.mul_(gt.view(B, 1))
    total = torch.empty(_STATIC_STARTS[-1], dtype=torch.float32, device=flat.device)
    L.check(L.load().dpn_sum_parts(_ptr(flat), B, _STATIC_STARTS[-1], 0, _ptr(total), _stream()), 'dpn_sum_parts')
    return (g_heads, g_evec, *_static_views(total))


class _DataLossBatchFn(torch.autograd.Function):
    """The data loss alone for B field samples in one step (the reference's first 2 000 steps): the B weight blocks packed in one launch, then per
    field the margin rows' fields (no Jacobian), dpn_smooth_l1 (block sums and the cotangent of a unit total in one launch) and the point backward
    right behind it.  Existing kernels only.  totals [B] = mean SmoothL1(beta) * margin_factor, step_losses' expression."""

    @staticmethod
    def forward(ctx, cfg, grad_enabled, beta, margin_factor, x, y, t, coord_data, labels, heads, evec, *statics):
        ops = _operands('data_losses_batch', x, y, t, None, coord_data, heads, evec, statics, labels=labels, batch=True, split=(0, False))
        lib = L.load()
        B, n = ops.cd.shape[0], ops.cd.shape[1]
        dev = ops.cd.device
        need_grad = bool(grad_enabled) and any(v.requires_grad for v in (heads, evec) + tuple(statics))
        dsum = torch.empty((B, (n * 6 + 255) // 256), dtype=torch.float64, device=dev)
        batch = _FieldBatch(cfg, ops, n, pack=True)
        g_out = grads = None
        if need_grad:
            g_out, grads = torch.empty((n, 6), dtype=torch.float32, device=dev), batch.grads()
        for b in range(B):
            ws, nets = batch.field(b)
            out_n, _ = _forward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], want_jac=False, want_saved=need_grad)
            L.check(lib.dpn_smooth_l1(_ptr(out_n), _ptr(ops.lab[b]), n, beta, margin_factor / (6.0 * n), _ptr(dsum[b]), _ptr(g_out), 0, None, _stream()),
                    'dpn_smooth_l1')
            if need_grad:
                _backward_points(cfg, ws, nets, ops.x[b], ops.y[b], ops.t[b], None, ops.cd[b], g_out, None, ops.st,
                                 into=(grads[0][b], grads[1][b], _static_views(grads[2][b])))
            del ws, out_n
        ctx.grads, ctx.n_static = grads, len(statics)
        ctx.set_materialize_grads(False)
        return (dsum.sum(dim=1) / (6.0 * n)).float() * margin_factor

    @staticmethod
    def backward(ctx, g_total):
        if g_total is None:
            return (None,) * (11 + ctx.n_static)
        return (None,) * 9 + _scaled_batch_grads(ctx, 'data_losses_batch', g_total)


def data_losses_batch(cfg: PointConfig, x, y, t, coord_data, labels, heads, evec, statics, beta=0.1, margin_factor=1.0):
    """totals [B]: the data loss (mean SmoothL1(beta) over [N, 6], times margin_factor) of B field samples' labelled rows -- x, y, t [B, N],
    coord_data and labels [B, N, 6], heads [B, 256, 2700], evec [B, 6, 256], shared statics -- in one step (_DataLossBatchFn)."""
    return _DataLossBatchFn.apply(cfg, torch.is_grad_enabled(), float(beta), float(margin_factor), x, y, t, coord_data, labels, heads, evec, *statics)


def step_losses_batch(cfg: PointConfig, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta=0.1, margin_factor=1.0):
    """step_losses for B field samples in one step (distinct field / lead time, so distinct hyper-network weights): x, y, t, f [B, N], coord_data
    [B, N, 6], labels [B, N - n_inter, 6], heads [B, 256, 2700], evec [B, 6, 256], shared statics (eval_step_batch's shapes).  Returns (terms
    [B, 2, 6]: interior | margin, parts [B, 3]: data loss, interior total, margin total, totals [B] = (data + interior) + margin): the PDE values
    bitwise step_losses' per field.  Only `totals` carries gradient; terms and parts are detached diagnostics.  Under no_grad nothing is saved and no
    point backward runs.  One backward pass per forward (_StepLossBatchFn).  Point weights, causal weights and loss balancing are implemented for
    one field at a time only (step_losses)."""
    losses, totals = _StepLossBatchFn.apply(cfg, torch.is_grad_enabled(), int(n_inter), float(beta), float(margin_factor), x, y, t, f, coord_data, labels,
                                            heads, evec, *statics)
    B = losses.shape[0]
    return losses[:, :14].view(B, 2, 7)[:, :, :6], torch.stack((losses[:, 14], losses[:, 6], losses[:, 13]), dim=1), totals


def _weight_options(what, weights, causal, diag):
    """The `extra` argument of _PdeLossFn / _StepLossFn: None when neither option is given (the launches of before)."""
    if weights is None and causal is None:
        return None
    if causal is not None and not all(hasattr(causal, k) for k in ('eps', 'bins', 'relative', 'bounds')):
        raise TypeError('%s: causal must be a deepphysinet_amd.causal.CausalWeights, got %r' % (what, causal))
    return (None if weights is None else weights.detach(), causal, diag)


def step_losses(cfg: PointConfig, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta=0.1, margin_factor=1.0, inter_weights=None,
                causal=None, diag=None):
    """(inter_terms [6], inter_total, margin_terms [6], margin_total, data_loss) of the reference's step body in one point pass; the first
    n_inter rows of x, y, t, f, coord_data are the interior points, the rest the margin points whose labels are `labels` (_StepLossFn).
    inter_weights [n_inter]: constant per-point weights of the interior group's PDE losses; causal (causal.CausalWeights): causal time weights, the
    interior and the margin group each with bins and weights of its own; a list given as `diag` receives the two groups' diag tensors (device,
    include/dpn_hip.h: dpn_causal_weights).  The data loss is not weighted.  Neither given: the launches of before."""
    return _StepLossFn.apply(cfg, _weight_options('step_losses', inter_weights, causal, diag), int(n_inter), float(beta), float(margin_factor), x, y, t, f,
                             coord_data, labels, heads, evec, *statics)


def _term_table(inter_terms, margin_terms, data):
    """The 13 device scalars of dpn_balance_combine as a host pointer table (and the tensors it points into, to be kept alive by the caller)."""
    it, mt, d = _f32c(inter_terms.detach()), _f32c(margin_terms.detach()), _f32c(data.detach()).reshape(1)
    if it.numel() != 6 or mt.numel() != 6:
        raise ValueError('balanced_total: inter_terms and margin_terms hold six terms each, got %d, %d' % (it.numel(), mt.numel()))
    ptrs = [it.data_ptr() + 4 * i for i in range(6)] + [mt.data_ptr() + 4 * i for i in range(6)] + [d.data_ptr()]
    return (ctypes.c_void_p * L.BALANCE_STEP_TERMS)(*ptrs), (it, mt, d)


class _BalancedTotalFn(torch.autograd.Function):
    """total = sum_i lambda_map(i) * term_i over the step's 13 terms (dpn_balance_combine: one launch; its backward one launch for the 13
    cotangents).  lambda is a constant of the loss, read on the device when the launch runs."""

    @staticmethod
    def forward(ctx, inter_terms, margin_terms, data, lam, term_map):
        require_gpu(data, 'data', 'balanced_total')
        table, keep = _term_table(inter_terms, margin_terms, data)
        K = lam.numel()
        cmap = (ctypes.c_int * L.BALANCE_STEP_TERMS)(*term_map)
        total = torch.empty((), dtype=torch.float32, device=data.device)
        L.check(L.load().dpn_balance_combine(table, K, cmap, _ptr(lam), None, _ptr(total), None, _stream()), 'dpn_balance_combine')
        ctx.lam, ctx.K, ctx.cmap, ctx.data_shape = lam, K, cmap, data.shape
        return total

    @staticmethod
    def backward(ctx, g):
        cot = torch.empty(L.BALANCE_STEP_TERMS, dtype=torch.float32, device=g.device)
        L.check(L.load().dpn_balance_combine(None, ctx.K, ctx.cmap, _ptr(ctx.lam), _ptr(_f32c(g).reshape(1)), None, _ptr(cot), _stream()),
                'dpn_balance_combine(grad)')
        return cot[:6], cot[6:12], cot[12].reshape(ctx.data_shape), None, None


def balanced_total(inter_terms, margin_terms, data, lam, groups='equations'):
    """The balanced loss of a step: sum_i lam[k(i)] * term_i over step_losses' interior terms [6], margin terms [6] and
    data loss, fp32, in the order data, interior 0..5, margin 0..5.  lam: fp32 [K] on the device (a constant: no cotangent is formed for it);
    groups: 'equations' (K = 7) or 'parts' (K = 3), balance.group_map.  The backward pass hands the 13 cotangents lam[k(i)] * g to the terms' node."""
    from .balance import GROUPS, group_map
    term_map = group_map(groups)
    if lam.dtype != torch.float32 or not lam.is_cuda or not lam.is_contiguous() or lam.numel() != len(GROUPS[groups]):
        raise ValueError('balanced_total: lam must be a contiguous fp32 device tensor of %d weights for groups=%r' % (len(GROUPS[groups]), groups))
    return _BalancedTotalFn.apply(inter_terms, margin_terms, data, lam.detach(), term_map)


def balance_sumsq(grads, shapes, out):
    """out (one fp64 device slot) = the sum of squares of the fp32 device tensors `grads` in fp64 (dpn_balance_sumsq); an entry None counts as zeros
    of shape shapes[i]."""
    lib = L.load()
    gs = [None if g is None else _f32c(g) for g in grads]
    for g in gs:
        if g is not None:
            require_gpu(g, 'a gradient', 'balance_sumsq')
    numel = (ctypes.c_int64 * len(gs))(*[int(torch.Size(s).numel()) for s in shapes])
    table = (ctypes.c_void_p * len(gs))(*[None if g is None else g.data_ptr() for g in gs])
    n_scratch = int(lib.dpn_balance_scratch_doubles(len(gs), numel))
    if n_scratch == 0:
        raise ValueError('balance_sumsq: a table of %d tensors is not taken (1..4096 non-empty tensors, include/dpn_hip.h)' % len(gs))
    scratch = torch.empty(n_scratch, dtype=torch.float64, device=out.device)
    L.check(lib.dpn_balance_sumsq(len(gs), table, numel, _ptr(scratch), _ptr(out), _stream()), 'dpn_balance_sumsq')
    return out


def balance_update(sumsq, lam, balance, diag):
    """dpn_balance_update: lam [K] (fp32, in place) from the K sums of squares by the rule of balance.update_reference; diag [3 K + 2] fp64."""
    K = lam.numel()
    L.check(L.load().dpn_balance_update(_ptr(sumsq), K, float(balance.momentum), float(balance.lam_min), float(balance.lam_max), _ptr(lam), _ptr(diag),
                                        _stream()), 'dpn_balance_update')


def pde_losses_batch(cfg: PointConfig, x, y, t, f, coord_data, heads, evec, statics, point_weights=None, causal=None):
    """(losses [B,6], totals [B]) for B field samples with N points each; tensors carry a leading B (see _PdeLossBatchFn).  Point weights and causal
    time weights are not implemented for lead batches."""
    if point_weights is not None or causal is not None:
        raise NotImplementedError('pde_losses_batch: point_weights / causal are implemented for one field at a time (pde_losses, step_losses), not for '
                                  'lead batches')
    return _PdeLossBatchFn.apply(cfg, torch.is_grad_enabled(), x, y, t, f, coord_data, heads, evec, *statics)


def point_fields(cfg: PointConfig, coord_data, heads, evec, statics, x=None, y=None, t=None, pe_in=None):
    """Normalised fields [N,6].  Give either raw (x,y,t) [N] or caller-encoded coordinates pe_in [N,192].
    heads [256, 2700]: one row per hidden channel, columns [w1b1 of nets 0..5 (193 each) | w2b2 of nets 0..5 (257 each)]."""
    if (pe_in is None) == (x is None):
        raise ValueError('give exactly one of (x,y,t) or pe_in')
    if x is not None:
        x, y, t = (v.reshape(-1) for v in (x, y, t))
    return _PointFieldsFn.apply(cfg, x, y, t, pe_in, coord_data, heads, evec, *statics)


def pde_losses(cfg: PointConfig, x, y, t, f, coord_data, heads, evec, statics, with_total=False, point_weights=None, causal=None, diag=None):
    """The six scaled residual losses [6] of place_one_batch (and, with_total, their sum in the reference's order as a 0-dim tensor).
    point_weights [N] (or [N, 1]): constant per-point weights -- loss_e = factor_e * sum_i w_i rho(r_ie) / N, linear in the weights, no gradient
    flows into them; causal (causal.CausalWeights): causal time weights W_bin(t_i), multiplied with point_weights when both are given; a list given
    as `diag` receives the diag tensor (device).  Neither given: the launches of before."""
    terms, total = _PdeLossFn.apply(cfg, _weight_options('pde_losses', point_weights, causal, diag), x, y, t, f, coord_data, heads, evec, *statics)
    return (terms, total) if with_total else terms


def pde_fields_and_jacobian(cfg: PointConfig, x, y, t, coord_data, heads, evec, statics):
    """No-grad helper: normalised fields [N,6] and d(fields_n)/d(x,y,t) [N,6,3] straight from the forward kernel."""
    with torch.no_grad():
        ops = _operands('pde_fields_and_jacobian', x, y, t, None, coord_data, heads, evec, statics)
        ws = _Workspace(ops.cd.shape[0], cfg.prec, ops.cd.device)
        return _forward_points(cfg, ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, want_jac=True, want_saved=False)


def decode_masks(saved, n, prec):
    """(m1, m2), bool [6, n, 256] in natural channel order, decoded from a saved-state buffer (uint8, as dpn_fwd_ref wrote it for n points in precision
    prec: 1 plain bf16 | 2 hi+lo; any device): what relu_masks returns for the buffer of its own forward pass."""
    n_pad, ns, raw, dev = (n + 127) // 128 * 128, int(prec), saved, saved.device
    tiles = n_pad // 32
    mat = 6 * ns * n_pad * 512                                                      # T1 (hi, lo planes) | M2 | m1: SavedView
    # M2: [6][tiles][kk 2][ct 8][lane 64][8 bf16 of 0/1]: register r = 8 kk + e of lane (col jj = lane & 31, h = lane >> 5) is the mask of
    # channel chain_ch(2 ct + (jj >> 4), (jj >> 3) & 1, jj & 7) at point drow32(r, h) of the tile
    m2_raw = raw[mat:mat + 6 * n_pad * 512].view(torch.int16).view(6, tiles, 2, 8, 64, 8) != 0
    lane = torch.arange(64, device=dev)
    jj, hh = lane & 31, lane >> 5
    ct = torch.arange(8, device=dev)
    ks = 2 * ct[:, None] + (jj >> 4)[None, :]                                       # [ct, lane]
    chan = 16 * ks + 8 * ((jj & 7) >> 2)[None, :] + 4 * ((jj >> 3) & 1)[None, :] + (jj & 3)[None, :]
    r = torch.arange(16, device=dev)
    prow = (r & 3)[:, None] + 8 * (r >> 2)[:, None] + 4 * hh[None, :]              # [r, lane] point row inside the tile
    m2 = torch.zeros((6, tiles, 32, 256), dtype=torch.bool, device=dev)
    src = m2_raw.permute(0, 1, 3, 4, 2, 5).reshape(6, tiles, 8, 64, 16)            # [net, tile, ct, lane, r]
    pi = prow.t()[None, :, :].expand(8, 64, 16)                                    # [ct, lane, r]
    ci = chan[:, :, None].expand(8, 64, 16)
    m2[:, :, pi, ci] = src
    # m1: uint4 per (net, tile, lane): bit 16 (T & 1) + r of word T >> 1 = mask of channel 32 T + drow32(r, h) at point lane & 31
    m1_raw = raw[mat + 6 * n_pad * 512:mat + 6 * n_pad * 512 + 6 * n_pad * 32].view(torch.int32).view(6, tiles, 64, 4)
    T = torch.arange(8, device=dev)
    words = m1_raw[:, :, :, T >> 1]                                                # [net, tile, lane, T]
    bits = (words[..., None] >> (16 * (T & 1)[:, None] + r[None, :])) & 1           # [net, tile, lane, T, r]
    ch1 = 32 * T[None, :, None] + (r & 3)[None, None, :] + 8 * (r >> 2)[None, None, :] + 4 * hh[:, None, None]       # [lane, T, r]
    m1 = torch.zeros((6, tiles, 32, 256), dtype=torch.bool, device=dev)
    p1 = jj[:, None, None].expand(64, 8, 16)
    m1[:, :, p1, ch1] = bits.bool()
    return m1.reshape(6, n_pad, 256)[:, :n], m2.reshape(6, n_pad, 256)[:, :n]


def relu_masks(cfg: PointConfig, x, y, t, coord_data, heads, evec, statics):
    """Diagnostic export of the two ReLU masks of every VariableNet at every point, decoded from the state dpn_fwd saves for the backward
    pass: (m1, m2), bool [6, N, 256] in natural channel order -- m1 = (w1 . pe + b1 > 0) (variable_net.py:67-68), m2 = (cat_fc1.fc.0 pre-
    activation > 0) (ResMLP, :13-24).  The Jacobian and every gradient are piecewise constant / linear in these bits, so a point whose
    pre-activation lies within rounding distance of zero may carry a different bit than another arithmetic's (the parity tests list those
    points and hold everything else to the tight bounds).  Layouts: csrc/dpn_point_common.h SavedView, dpn_layout.h."""
    with torch.no_grad():
        ops = _operands('relu_masks', x, y, t, None, coord_data, heads, evec, statics)
        n, dev = ops.cd.shape[0], ops.cd.device
        ws = _Workspace(n, cfg.prec, dev)
        _forward_points(cfg, ws, ops.nets(), ops.x, ops.y, ops.t, None, ops.cd, want_jac=True, want_saved=True)
        return decode_masks(ws.saved, n, cfg.prec)


def smooth_l1_data_loss(out_n, labels, beta=0.1, factor=1.0):
    """mean(SmoothL1(beta)) * factor as a differentiable torch scalar (losses/weights_loss.py:17-20); HIP kernel for both passes."""
    return _SmoothL1Fn.apply(out_n, labels, float(beta), float(factor))


class _SmoothL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_n, labels, beta, factor):
        require_gpu(out_n, 'out_n', 'smooth_l1_data_loss')
        lib = L.load()
        o, l = _f32c(out_n), _f32c(labels)
        n = o.shape[0]
        s = torch.empty((n * 6 + 255) // 256, dtype=torch.float64, device=o.device)      # per-block partial sums
        g = torch.empty_like(o)
        L.check(lib.dpn_smooth_l1(_ptr(o), _ptr(l), n, beta, factor / (6.0 * n), _ptr(s), _ptr(g), 0, None, _stream()), 'dpn_smooth_l1')
        ctx.save_for_backward(g)
        return ((s.sum() / (6.0 * n)).float() * factor)

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        return g * gl, None, None, None


# ------------------------------------------------------------------------------------------------ validation: no-grad evaluation of the step's losses
EVAL_VARIABLES = ('u', 'v', 'p', 'T', 'q', 'rio')       # the reference's names of the six outputs in its log lines (interface_physics.py:609-618)


def _label_partials(cfg: PointConfig, out_n, labels, n, segments, beta, with_clip, partials):
    lib = L.load()
    ph = cfg.physics()
    L.check(lib.dpn_label_errors(_ptr(out_n), _ptr(labels), n, segments, ctypes.byref(ph), float(beta), int(bool(with_clip)), _ptr(partials),
                                 _stream()), 'dpn_label_errors')


def label_errors(cfg: PointConfig, out_n, labels, beta=0.1, with_clip=False):
    """Sufficient statistics [S, 25] (fp64) of normalised predictions out_n [S, N, 6] (or [N, 6]: S = 1) against labels of the same shape, one
    row per segment: [0] sum SmoothL1_beta, then per variable (u, v, P, T, q, rho) sum d^2 [1:7], sum |d| [7:13], sum d [13:19], max |d| [19:25]
    of d = inverse_norm(pred) - inverse_norm(label) (include/dpn_hip.h: dpn_label_errors).  One pass over the data, bitwise reproducible."""
    require_gpu(out_n, 'out_n', 'label_errors')
    require_gpu(labels, 'labels', 'label_errors')
    o, l = _f32c(out_n), _f32c(labels)
    if o.shape != l.shape or o.dim() not in (2, 3) or o.shape[-1] != 6 or o.numel() == 0:
        raise ValueError('label_errors: out_n %s and labels %s must both be [N, 6] or [S, N, 6]' % (tuple(out_n.shape), tuple(labels.shape)))
    S, n = (1, o.shape[0]) if o.dim() == 2 else (o.shape[0], o.shape[1])
    lib = L.load()
    partials = torch.empty((S, int(lib.dpn_label_errors_blocks(n)), L.EVAL_STATS), dtype=torch.float64, device=o.device)
    stats = torch.empty((S, L.EVAL_STATS), dtype=torch.float64, device=o.device)
    _label_partials(cfg, o, l, n, S, beta, with_clip, partials)
    L.check(lib.dpn_label_errors_finish(_ptr(partials), n, S, _ptr(stats), _stream()), 'dpn_label_errors_finish')
    return stats


def _eval(what, cfg, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta, with_pde, with_clip, batch):
    """eval_step (batch False: one field, its forward packs the weights) and eval_step_batch (batch True: B fields packed in one launch).  Per
    field: with_pde, the step body's point pass (_step_pass, no saved state) and the label statistics' block rows of its margin rows; without,
    the margin rows' fields only.  One finish launch adds the statistics of all fields.  Returns (losses [B, 2, 7] or None, stats [B, 25])."""
    n_inter = int(n_inter)
    ops = _operands(what, x, y, t, f, coord_data, heads, evec, statics, labels=labels, batch=batch, split=(n_inter, with_pde))
    lib = L.load()
    B, n = (ops.cd.shape[0], ops.cd.shape[1]) if batch else (1, ops.cd.shape[0])
    dev = ops.cd.device
    n_m = n - n_inter
    n_fwd = n if with_pde else n_m
    losses = torch.empty((B, 2, 7), dtype=torch.float32, device=dev) if with_pde else None
    partials = torch.empty((B, int(lib.dpn_label_errors_blocks(n_m)), L.EVAL_STATS), dtype=torch.float64, device=dev)
    stats = torch.empty((B, L.EVAL_STATS), dtype=torch.float64, device=dev)
    fields = _FieldBatch(cfg, ops, n_fwd, pack=True) if batch else None
    for b in range(B):
        ws, nets = fields.field(b) if batch else (_Workspace(n_fwd, cfg.prec, dev), ops.nets())
        x_, y_, t_, f_, cd_, lab_ = (v[b] for v in ops[:4] + (ops.cd, ops.lab)) if batch else ops[:4] + (ops.cd, ops.lab)
        if with_pde:
            out_n = _step_pass(what, cfg, ws, nets, n_inter, x_, y_, t_, f_, cd_, losses[b])[0][n_inter:]
        else:                                              # the reference's first 2 000 steps: fields only, no Jacobian
            out_n, _ = _forward_points(cfg, ws, nets, x_[n_inter:], y_[n_inter:], t_[n_inter:], None, cd_[n_inter:], want_jac=False,
                                       want_saved=False)
        _label_partials(cfg, out_n, lab_, n_m, 1, beta, with_clip, partials[b:b + 1])
    L.check(lib.dpn_label_errors_finish(_ptr(partials), n_m, B, _ptr(stats), _stream()), 'dpn_label_errors_finish')
    return losses, stats


@torch.no_grad()
def eval_step(cfg: PointConfig, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta=0.1, with_pde=True, with_clip=False):
    """The losses of the step body (_StepLossFn.forward: same launches, same tiles, same fixed-order sums) evaluated with nothing kept for a
    backward pass: no saved state, no operands / partials buffers, no autograd node.  The first n_inter rows of x, y, t, f, coord_data are the
    interior points, the rest the margin points whose labels are `labels`.  Returns (losses [2, 7] fp32: rows interior | margin, columns the
    six scaled PDE terms and their total -- None without with_pde, which evaluates the margin rows' fields only, no Jacobian --, stats [25]
    fp64: label_errors of the margin rows, stats[0] / (6 n_margin) = the unscaled data loss).  The cfg's own with_clip governs the PDE
    residuals as in training; `with_clip` here is the label statistics' alone (off in the reference, interface_physics.py:706-713)."""
    losses, stats = _eval('eval_step', cfg, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta, with_pde, with_clip, False)
    return None if losses is None else losses[0], stats[0]


@torch.no_grad()
def eval_step_batch(cfg: PointConfig, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta=0.1, with_pde=True, with_clip=False):
    """eval_step for B field samples (distinct field / lead time, so distinct hyper-network weights): point tensors [B, N(, 6)], labels
    [B, N - n_inter, 6], heads [B, 256, 2700], evec [B, 6, 256], shared statics.  The B weight blocks are packed in one launch (_FieldBatch); each
    sample then takes ONE point pass over its [interior | margin] rows -- the pass of eval_step and of the training step, so that a sample's row
    equals eval_step's bitwise (two passes, one per group, would form other 128-point tiles at the group boundary) --, and one finish launch
    adds the label statistics of all B samples.  Returns (losses [B, 2, 7] or None, stats [B, 25])."""
    return _eval('eval_step_batch', cfg, n_inter, x, y, t, f, coord_data, labels, heads, evec, statics, beta, with_pde, with_clip, True)


# ------------------------------------------------------------------------------------------------ inference: fields and residuals, no autograd
def point_sizes(n, prec):
    """(n_pad, packed) of an n-point forward (dpn_sizes): n rounded up to the point kernels' padding unit (n = 1: the unit itself), and the
    bytes of one field's packed weight block."""
    sizes = L.DpnSizes()
    L.check(L.load().dpn_sizes(int(n), int(prec), ctypes.byref(sizes)), 'dpn_sizes')
    return int(sizes.n_pad), int(sizes.packed)


def point_buffers(m, device):
    """The five input buffers of an m-point forward, not filled: x, y, t, f [m], coord_data [m, 6] fp32 (what dpn_sample_at and the time-window
    kernels write)."""
    return tuple(torch.empty(m, dtype=torch.float32, device=device) for _ in range(4)) + (torch.empty((m, 6), dtype=torch.float32, device=device),)


def grid_maps(cfg: PointConfig, out_n, lon_size, lat_size, with_clip=False):
    """Normalised fields of all lon x lat nodes (out_n [lon * lat, 6], x outer, y inner) de-normalised and scattered into maps [6, lat, lon]
    (dpn_grid_maps)."""
    maps = torch.empty((6, lat_size, lon_size), dtype=torch.float32, device=out_n.device)
    ph = cfg.physics()
    L.check(L.load().dpn_grid_maps(_ptr(out_n), lon_size, lat_size, ctypes.byref(ph), int(bool(with_clip)), _ptr(maps), _stream()), 'dpn_grid_maps')
    return maps


class PackedField:
    """One field's weights (heads [256, 2700], evec [6, 256], the 48 statics) packed once for forwards of up to n_chunk points with no saved
    state: station rows and lattice chunks (fields), or residual rows.  Nothing here is differentiable."""

    def __init__(self, cfg: PointConfig, heads, evec, statics, n_chunk):
        self.cfg = cfg
        self.keep = (_f32c(heads), _f32c(evec), [_f32c(s) for s in statics])        # the pointer table points into these
        self.nets = _net_ptrs(*self.keep)
        self.ws = _Workspace(n_chunk, cfg.prec, self.keep[0].device)
        lib = L.load()
        L.check(lib.dpn_pack_weights_form(self.nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0), _ptr(self.ws.packed), _stream()), 'dpn_pack_weights')
        self.ws.prepacked = True
        self._traj_ph = None
        self._clip_ph = {}

    def _forward(self, x, y, t, coord_data, want_jac=False):
        """The forward every product here starts with, no saved state: (out_n [n, 6], jac_n [n, 6, 3] or None)."""
        return _forward_points(self.cfg, self.ws, self.nets, x, y, t, None, coord_data, want_jac=want_jac, want_saved=False)

    def fields(self, x, y, t, coord_data, with_clip=False, rows=None, maps=None, lattice=None, first=0):
        """The six physical fields at points x, y, t [n], coord_data [n, 6] (dpn_fields_out): into rows [n, 6], or into the places of points
        first .. first + n of `lattice` in maps [nt, 6, ny, nx]."""
        out_n, _ = self._forward(x, y, t, coord_data)
        ph = self.cfg.physics()
        lat = None if lattice is None else ctypes.byref(lattice.c_struct())
        L.check(L.load().dpn_fields_out(_ptr(out_n), out_n.shape[0], ctypes.byref(ph), int(bool(with_clip)), _ptr(rows), _ptr(maps), lat, first,
                                        _stream()), 'dpn_fields_out')

    def residuals(self, x, y, t, f, coord_data, res):
        """The six signed residuals lhs - rhs at points x, y, t, f [n], coord_data [n, 6] into res [n, 6] (dpn_residual_points)."""
        out_n, jac_n = self._forward(x, y, t, coord_data, True)
        geo, ph = self.cfg.geometry(), self.cfg.physics()
        L.check(L.load().dpn_residual_points(_ptr(out_n), _ptr(jac_n), _ptr(f), out_n.shape[0], ctypes.byref(geo), ctypes.byref(ph), _ptr(res),
                                             _stream()), 'dpn_residual_points')

    def diagnostics(self, x, y, t, f, coord_data, products, with_clip=False, rows=None, maps=None, lattice=None, first=0):
        """Derived diagnostics (dpn_diagnostics_out; deepphysinet_amd.diagnostics.PRODUCTS) at points x, y, t, f [n], coord_data [n, 6]: `products`, a
        sequence of P product ids, into rows [n, P], or into the places of points first .. first + n of `lattice` in maps [nt, P, ny, nx]."""
        out_n, jac_n = self._forward(x, y, t, coord_data, True)
        ph = self._clip_physics(with_clip)
        ids = (ctypes.c_int32 * len(products))(*products)
        lat = None if lattice is None else ctypes.byref(lattice.c_struct())
        L.check(L.load().dpn_diagnostics_out(_ptr(out_n), _ptr(jac_n), _ptr(f), out_n.shape[0], ctypes.byref(ph), int(bool(with_clip)), ids, len(ids),
                                             _ptr(rows), _ptr(maps), lat, first, _stream()), 'dpn_diagnostics_out')

    def ensemble_accumulate(self, x, y, t, f, coord_data, state, first=0, with_clip=False):
        """This field, as one member of an ensemble, at points x, y, t, f [n], coord_data [n, 6], folded into `state` (an EnsembleState) at its points
        first .. first + n (dpn_ensemble_accumulate).  The request chooses the forward: with the Jacobian (as `diagnostics`) iff a selected product
        reads it, otherwise the fields-only one (as `fields`).  with_clip as `diagnostics` takes it."""
        need_j = reads_jacobian(state.ids)
        out_n, jac_n = self._forward(x, y, t, coord_data, need_j)
        ph = self._clip_physics(with_clip)
        s = state
        L.check(L.load().dpn_ensemble_accumulate(_ptr(out_n), _ptr(jac_n) if need_j else None, _ptr(f) if reads_coriolis(s.ids) else None, out_n.shape[0],
                                                 ctypes.byref(ph), int(bool(with_clip)), s.c_ids, len(s.ids), s.c_thr_col, s.c_thr_val, len(s.thr_col),
                                                 int(first), s.n_total, _ptr(s.count), _ptr(s.mean), _ptr(s.m2), _ptr(s.vmin), _ptr(s.vmax),
                                                 _ptr(s.exceed), _stream()), 'dpn_ensemble_accumulate')

    def region_accumulate(self, x, y, t, f, coord_data, state, first=0, with_clip=False):
        """This field at points first .. first + n of the flat point list of `state` (a RegionState; first a multiple of 64): x, y, t, f [n],
        coord_data [n, 6], folded into the state's slots (dpn_region_accumulate).  The forward is chosen as `ensemble_accumulate` chooses it."""
        need_j = reads_jacobian(state.ids)
        out_n, jac_n = self._forward(x, y, t, coord_data, need_j)
        state.accumulate(out_n, jac_n if need_j else None, f if reads_coriolis(state.ids) else None, self._clip_physics(with_clip), first, with_clip)

    def verify_accumulate(self, x, y, t, coord_data, obs, state, first=0, with_clip=False):
        """This field, as one case (forecast date) of a verification, at points x, y, t [n], coord_data [n, 6], against the reports obs [n, P] fp32
        (NaN: none), folded into `state` (a VerifyState) at its points first .. first + n: the fields-only forward, then one dpn_verify_accumulate
        launch, which forms the baseline from coord_data itself.  with_clip as `diagnostics` takes it, on forecast and baseline alike."""
        out_n, _ = self._forward(x, y, t, coord_data)
        state.accumulate(out_n, coord_data, obs, self._clip_physics(with_clip), first, with_clip)

    def pverify_stage(self, x, y, t, coord_data, state, member, first=0, with_clip=False):
        """This field, as member `member` of the case that `state` (a ProbVerifyState) is staging, at points x, y, t [n], coord_data [n, 6]: the
        fields-only forward, then one dpn_pverify_stage launch, which writes the forecast and the baseline values (from coord_data itself) of every
        column into the state's planes at points first .. first + n.  with_clip as `diagnostics` takes it, on forecast and baseline alike."""
        out_n, _ = self._forward(x, y, t, coord_data)
        state.stage(out_n, coord_data, self._clip_physics(with_clip), member, first, with_clip)

    def nbhd_stage(self, x, y, t, coord_data, analysis, state, first=0, with_clip=False):
        """This field, as the case that `state` (an NbhdState) is staging, at points first .. first + n of the state's lattice: x, y, t [n],
        coord_data [n, 6]; the fields-only forward, then one dpn_nbhd_stage launch, which forms the baseline from coord_data itself, reads the
        analysis [nt, P, ny, nx] at its own nodes and writes their mask bytes.  with_clip as `diagnostics` takes it, on forecast and baseline."""
        out_n, _ = self._forward(x, y, t, coord_data)
        state.stage(out_n, coord_data, analysis, self._clip_physics(with_clip), first, with_clip)

    def residual_scores(self, x, y, t, f, coord_data, factors, k=1.0):
        """Scores of a pool of candidate points for residual-weighted sampling (CollocationSampler.get_inter_data_adaptive): `residuals` on the m
        points, then dpn_adaptive_scores -- score_i = sum_e factors[e] * res_ie ** 2 in fp64, factors = six floats in LOSS_ORDER.  Returns
        (score [m] fp64, stats [3] fp64: sum score ** k, the count of non-finite scores (written as 0), max score; res [m, 6] fp32; scratch, the
        dpn_adaptive_scratch_doubles(m) doubles the selection goes on to use)."""
        lib = L.load()
        m, dev = coord_data.shape[0], coord_data.device
        if m > self.ws.n:
            raise ValueError('residual_scores: %d points, but this PackedField was packed for chunks of %d' % (m, self.ws.n))
        size = int(lib.dpn_adaptive_scratch_doubles(m))
        if size <= 0:
            raise ValueError('residual_scores: %d candidates; dpn_adaptive_select takes 1 .. 2**20' % m)
        res = torch.empty((m, 6), dtype=torch.float32, device=dev)
        self.residuals(x, y, t, f, coord_data, res)
        score, scratch = torch.empty(m, dtype=torch.float64, device=dev), torch.empty(size, dtype=torch.float64, device=dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        fac = (ctypes.c_double * 6)(*[float(v) for v in factors])
        L.check(lib.dpn_adaptive_scores(_ptr(res), m, fac, float(k), _ptr(score), _ptr(stats), _ptr(scratch), _stream()), 'dpn_adaptive_scores')
        return score, stats, res, scratch

    def trajectory_stage(self, sampler, parcels, stage, t0, h, inv_wsum, step, fields=None, with_clip=False, record_only=False):
        """One Runge-Kutta stage for the parcels of `parcels` (a ParcelState): the fields-only forward at their current evaluation points, then
        dpn_traj_stage (traj_stage), which writes the next evaluation points into the same buffers.  Two launches, nothing read back."""
        x, y, t, _, cd = parcels.points
        out_n, _ = self._forward(x, y, t, cd)
        if self._traj_ph is None:                  # the table is built once per field, not once per stage (384 stages a day)
            self._traj_ph = self.cfg.physics()
        traj_stage(sampler, self._traj_ph, out_n, parcels, stage, t0, h, inv_wsum, step, fields, with_clip, record_only)

    def _clip_physics(self, with_clip):
        """The physics table of a call with a clip setting of its own (`with_clip` is the call's, as `fields` takes it: the training clip of P, T, q,
        rho), built once per field and setting: a lattice is many chunks, a time-window request K + R + 2 launches per chunk."""
        key = bool(with_clip)
        if key not in self._clip_ph:
            ph = self.cfg.physics()
            for k in range(2, L.NETS):
                ph.clip_on[k] = int(key and bool(self.cfg.clip_vars[k]))
            self._clip_ph[key] = ph
        return self._clip_ph[key]

    def window_scan(self, sampler, state, k, with_clip=False):
        """Scan node k of a time-window request for the points of `state` (an ExtremeState or a SpellState): the fields-only forward at the node,
        then the state's scan launch (dpn_extreme_scan, dpn_spell_scan), which folds it into the state and writes the next node's inputs into the
        same buffers; after the last node the state's begin launch closes the scan and writes the first probes.  Two launches (three at node K),
        nothing read back."""
        x, y, t, _, cd = state.points
        out_n, _ = self._forward(x, y, t, cd)
        state.scan(sampler, self._clip_physics(with_clip), with_clip, out_n, k)
        if k == state.K:
            state.begin(sampler)

    def window_refine(self, sampler, state, rnd, with_clip=False):
        """Round `rnd` of the refinement: the forward at the state's probes -- with the Jacobian where the state bisects on d/dt (extremes),
        fields-only where it bisects on the value (spells) --, then the state's refine launch, which moves the brackets and rewrites the probes.  Two
        launches, nothing read back."""
        x, y, t, _, cd = state.probes
        out_n, jac_n = self._forward(x, y, t, cd, state.REFINE_JACOBIAN)
        state.refine(sampler, self._clip_physics(with_clip), with_clip, out_n, jac_n, rnd)


def _request_arrays(ids, thr_col, thr_val, thr_side=None):
    """The ctypes arrays of a request, as the launchers take them: ids [P] int32, thr_col int32 and thr_val float [max(E, 1)] and, where the
    thresholds have sides, thr_side int32 [max(E, 1)]."""
    E = max(len(thr_col), 1)
    arrays = (ctypes.c_int32 * len(ids))(*ids), (ctypes.c_int32 * E)(*thr_col), (ctypes.c_float * E)(*thr_val)
    return arrays if thr_side is None else arrays + ((ctypes.c_int32 * E)(*thr_side),)


class EnsembleState:
    """Device state of an ensemble request between dpn_ensemble_accumulate launches (include/dpn_hip.h): for n_total points, the P columns `ids`
    (ensemble.ensemble_ids) and the E thresholds (thr_col, thr_val of ensemble.check_thresholds), product-major: count [P, n_total] int32, mean, m2
    [P, n_total] fp64, vmin, vmax [P, n_total] fp32, exceed [E, n_total] int32.  count, mean, m2 and exceed start at zero; vmin and vmax are not
    filled (count == 0 means "not yet set").  `finish` turns points first .. first + n into the six outputs, as rows or as maps."""

    POINT_BYTES = 4 + 8 + 8 + 4 + 4                        # per point and column; 4 more per point and threshold

    def __init__(self, n_total, ids, thr_col, thr_val, device):
        self.n_total, self.ids, self.thr_col, self.thr_val = int(n_total), list(ids), list(thr_col), [float(v) for v in thr_val]
        P, E = len(self.ids), len(self.thr_col)
        if not 1 <= P <= L.ENS_PRODUCTS or E > L.ENS_MAX_THRESHOLDS or len(self.thr_val) != E or self.n_total < 1:
            raise ValueError('EnsembleState: %d points, %d products (1..%d), %d thresholds (0..%d)' % (self.n_total, P, L.ENS_PRODUCTS, E, L.ENS_MAX_THRESHOLDS))
        self.c_ids, self.c_thr_col, self.c_thr_val = _request_arrays(self.ids, self.thr_col, self.thr_val)
        self.count = torch.zeros((P, self.n_total), dtype=torch.int32, device=device)
        self.mean, self.m2 = (torch.zeros((P, self.n_total), dtype=torch.float64, device=device) for _ in range(2))
        self.vmin, self.vmax = (torch.empty((P, self.n_total), dtype=torch.float32, device=device) for _ in range(2))
        self.exceed = torch.zeros((E, self.n_total), dtype=torch.int32, device=device) if E else None

    def finish(self, first, n, rows=None, maps=None, lattice=None):
        """dpn_ensemble_finish for points first .. first + n: rows / maps = dict(mean, spread, min, max, count, prob) of tensors in row form ([n, P],
        [n, E]) or in map form ([nt, P, ny, nx], [nt, E, ny, nx] of `lattice`); prob may be None without thresholds."""
        def table(d):
            return None if d is None else ctypes.byref(L.DpnEnsembleOut(*[_ptr(d.get(k)) for k in ('mean', 'spread', 'min', 'max', 'count', 'prob')]))
        lat = None if lattice is None else ctypes.byref(lattice.c_struct())
        L.check(L.load().dpn_ensemble_finish(_ptr(self.count), _ptr(self.mean), _ptr(self.m2), _ptr(self.vmin), _ptr(self.vmax), _ptr(self.exceed),
                                             self.n_total, len(self.ids), self.c_thr_col, len(self.thr_col), int(first), int(n), table(rows), table(maps),
                                             lat, _stream()), 'dpn_ensemble_finish')


class _ScoreState:
    """What the device states of the two verification requests share (VerifyState, ProbVerifyState): n_total points (or groups), the P columns `ids`
    (verification.verify_ids), the E thresholds (thr_col, thr_val, thr_side of verification.check_thresholds) and the arrays of `layout()` -- rows
    (name, dtype, shape) in the order of the C struct STATE -- as views of ONE zeroed byte buffer: the fp64 arrays first, so that every view is
    aligned, then the others in their order, no gaps; an array of no elements (the threshold array without thresholds) is None.  `pool` makes the
    state of groups of points (the launch POOL), `finish` turns points first .. first + n into the scores (the launch FINISH into the C struct
    OUT, whose destinations `out_rows()` lists as (name, dtype, shape behind the point axis)).  A subclass checks its own sizes (`_check`), and
    names what its launches take between the thresholds and the rest (`_extra`) and what its pooled states are made with (POOLED)."""

    STATE = OUT = POOL = FINISH = None
    POOLED = {}

    def __init__(self, n_total, ids, thr_col, thr_val, thr_side, device):
        self.n_total, self.ids = int(n_total), list(ids)
        self.thr_col, self.thr_val, self.thr_side = list(thr_col), [float(v) for v in thr_val], list(thr_side)
        self._check()
        self.c_ids, self.c_thr_col, self.c_thr_val, self.c_thr_side = _request_arrays(self.ids, self.thr_col, self.thr_val, self.thr_side)
        rows = sorted(self.layout(), key=lambda row: row[1] != torch.float64)         # (stable) the doubles first: every view aligned
        sizes = [math.prod(shape) * dtype.itemsize for _, dtype, shape in rows]
        self.buffer = torch.zeros(sum(sizes), dtype=torch.uint8, device=device)
        at = 0
        for (name, dtype, shape), size in zip(rows, sizes):
            setattr(self, name, self.buffer[at:at + size].view(dtype).view(shape) if size else None)
            at += size

    def _extra(self):
        return ()

    def clear(self):
        """Back to the state before the first case: one memset."""
        self.buffer.zero_()

    def arrays(self):
        """The arrays by STATE's names, in its order (the threshold array None without thresholds)."""
        return {k: getattr(self, k) for k, _ in self.STATE._fields_}

    def c_state(self):
        return self.STATE(*[_ptr(v) for v in self.arrays().values()])

    def upload_plan(self, order, seg_start):
        """A plan of verification.pool_plan's (order [N] int32, seg_start [G + 1] int64, numpy) checked and put on the device, for `pool`: a caller
        that must not wait for the device between its launches uploads its plans before the first of them."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        seg_start = np.ascontiguousarray(seg_start, dtype=np.int64)
        if order.shape != (self.n_total,) or seg_start.ndim != 1 or seg_start.size < 2:
            raise ValueError('%s.pool: order [%d] and seg_start [G + 1], got %s and %s' % (type(self).__name__, self.n_total, order.shape, seg_start.shape))
        dev = self.buffer.device
        return seg_start, torch.from_numpy(order).to(dev), torch.from_numpy(seg_start).to(dev)

    def _like(self, n_total):
        """An empty state of this one's class and request for n_total groups."""
        return type(self)(n_total, self.ids, self.thr_col, self.thr_val, self.thr_side, *self._extra(), self.buffer.device, **self.POOLED)

    def pool(self, order=None, seg_start=None, plan=None):
        """POOL: the state of the G = len(seg_start) - 1 groups of verification.pool_plan's (order, seg_start), or of a `plan` that `upload_plan`
        returned; a new state of the same class, columns and thresholds (`_like`)."""
        seg_start, d_order, d_seg = self.upload_plan(order, seg_start) if plan is None else plan
        G = seg_start.size - 1
        out = self._like(G)
        L.check(getattr(L.load(), self.POOL)(ctypes.byref(self.c_state()), self.n_total, _ptr(d_order), _ptr(d_seg),
                                             seg_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), G, len(self.ids), self.c_thr_col,
                                             len(self.thr_col), *self._extra(), ctypes.byref(out.c_state()), _stream()), self.POOL)
        out._plan = (d_order, d_seg)                                      # alive until the launch has read them
        return out

    def new_rows(self, n):
        """The destinations of `finish` for n points: a dict of tensors [n, ...] by OUT's names, in its order (the threshold ones None without
        thresholds)."""
        dev = self.buffer.device
        return {k: torch.empty((n,) + shape, dtype=dtype, device=dev) if all(shape) else None for k, dtype, shape in self.out_rows()}

    def finish(self, first=0, n=None, rows=None):
        """FINISH for points first .. first + n (default: all) into rows (`new_rows`, made here when not given).  Returns rows."""
        n = self.n_total - int(first) if n is None else int(n)
        rows = self.new_rows(n) if rows is None else rows
        table = self.OUT(*[_ptr(rows.get(k)) for k, _ in self.OUT._fields_])
        L.check(getattr(L.load(), self.FINISH)(ctypes.byref(self.c_state()), self.n_total, len(self.ids), self.c_thr_col, len(self.thr_col),
                                               *self._extra(), int(first), n, ctypes.byref(table), _stream()), self.FINISH)
        return rows


class VerifyState(_ScoreState):
    """Device state of a verification request (include/dpn_hip.h: DpnVerifyState): for n_total points (or groups), the P columns `ids` and the E
    thresholds, product-major: n [P, n_total] int32, the eleven fp64 arrays of verification.STATE_F64, max_ad [P, n_total] fp32 and cont
    [E, 6, n_total] int32 (_ScoreState).  `accumulate` folds one case's chunk in; the scores of `finish` are verification.OUT_FIELDS, [n, P] and,
    per threshold, [n, E]."""

    STATE, OUT, POOL, FINISH = L.DpnVerifyState, L.DpnVerifyOut, 'dpn_verify_pool', 'dpn_verify_finish'

    def _check(self):
        P, E, N = len(self.ids), len(self.thr_col), self.n_total
        if not 1 <= P <= L.VERIFY_MAX_COLUMNS or E > L.VERIFY_MAX_THRESHOLDS or len(self.thr_val) != E or len(self.thr_side) != E or N < 1:
            raise ValueError('VerifyState: %d points, %d products (1..%d), %d thresholds (0..%d)'
                             % (N, P, L.VERIFY_MAX_COLUMNS, E, L.VERIFY_MAX_THRESHOLDS))

    def layout(self):
        P, E, N = len(self.ids), len(self.thr_col), self.n_total
        return ([('n', torch.int32, (P, N))] + [(k, torch.float64, (P, N)) for k in VF.STATE_F64]
                + [('max_ad', torch.float32, (P, N)), ('cont', torch.int32, (E, 6, N))])

    def out_rows(self):
        P, E = len(self.ids), len(self.thr_col)
        return ([('count', torch.int32, (P,))] + [(k, torch.float32, (P,)) for k in VF.SCORES]
                + [(k, torch.float32, (E,)) for k in VF.THRESHOLD_SCORES])

    def accumulate(self, out_n, coord_data, obs, ph, first=0, with_clip=False):
        """dpn_verify_accumulate: one case's out_n [n, 6], coord_data [n, 6] and obs [n, P] (fp32, contiguous) at points first .. first + n."""
        n, P = out_n.shape[0], len(self.ids)
        if tuple(obs.shape) != (n, P) or obs.dtype != torch.float32 or not obs.is_contiguous() or tuple(coord_data.shape) != (n, 6):
            raise ValueError('VerifyState.accumulate: obs must be a contiguous fp32 [%d, %d] and coord_data [%d, 6], got %s %s and %s'
                             % (n, P, n, tuple(obs.shape), obs.dtype, tuple(coord_data.shape)))
        L.check(L.load().dpn_verify_accumulate(_ptr(out_n), _ptr(_f32c(coord_data)), _ptr(obs), n, ctypes.byref(ph), int(bool(with_clip)), self.c_ids, P,
                                               self.c_thr_col, self.c_thr_val, self.c_thr_side, len(self.thr_col), int(first), self.n_total,
                                               ctypes.byref(self.c_state()), _stream()), 'dpn_verify_accumulate')


class ProbVerifyState(_ScoreState):
    """Device state of a probabilistic verification request (include/dpn_hip.h: DpnPVerifyState): for n_total points (or groups), the P columns
    `ids`, the E thresholds and M members per case: n [P, N] int32, the five fp64 sums of prob_verification.STATE_F64 [2, P, N], rank
    [2, P, M + 1, N] int32 and rel [E, 2, 2, M + 1, N] int32 (_ScoreState) and, unless planes=False (a pooled state stages nothing), the two
    staging planes [M, P, N] fp32, which `clear` leaves: the next case's stages rewrite them.  `stage` writes one member's chunk into the planes,
    `case` folds the staged case in; the scores of `finish` are prob_verification.OUT_FIELDS.  ValueError: sizes out of range, an array of more
    than 2^31 - 1 elements."""

    STATE, OUT, POOL, FINISH = L.DpnPVerifyState, L.DpnPVerifyOut, 'dpn_pverify_pool', 'dpn_pverify_finish'
    POOLED = {'planes': False}

    def __init__(self, n_total, ids, thr_col, thr_val, thr_side, members, device, planes=True):
        self.members = members
        super().__init__(n_total, ids, thr_col, thr_val, thr_side, device)
        shape = (self.members, len(self.ids), self.n_total)
        self.plane_f, self.plane_b = (torch.zeros(shape, dtype=torch.float32, device=device) for _ in range(2)) if planes else (None, None)

    def _check(self):
        E = len(self.thr_col)
        if len(self.thr_val) != E or len(self.thr_side) != E:
            raise ValueError('ProbVerifyState: %d threshold columns, %d values, %d sides' % (E, len(self.thr_val), len(self.thr_side)))
        PV.check_state_size(self.n_total, len(self.ids), E, self.members)
        self.members = int(self.members)

    def _extra(self):
        return (self.members,)

    def layout(self):
        P, E, N, M1 = len(self.ids), len(self.thr_col), self.n_total, self.members + 1
        return ([('n', torch.int32, (P, N))] + [(k, torch.float64, (2, P, N)) for k in PV.STATE_F64]
                + [('rank', torch.int32, (2, P, M1, N)), ('rel', torch.int32, (E, 2, 2, M1, N))])

    def out_rows(self):
        P, E, M1 = len(self.ids), len(self.thr_col), self.members + 1
        return ([('count', torch.int32, (P,))] + [(k, torch.float32, (P,)) for k in PV.SCORES] + [(k, torch.int32, (P, M1)) for k in PV.HISTS]
                + [(k, torch.float32, (E,)) for k in PV.THRESHOLD_SCORES] + [(k, torch.int32, (E, M1)) for k in PV.DIAGRAMS])

    def stage(self, out_n, coord_data, ph, member, first=0, with_clip=False):
        """dpn_pverify_stage: member `member`'s out_n [n, 6] and coord_data [n, 6] (fp32, contiguous) at points first .. first + n."""
        n = out_n.shape[0]
        if self.plane_f is None or tuple(coord_data.shape) != (n, 6):
            raise ValueError('ProbVerifyState.stage: a state with planes and coord_data [%d, 6], got %s' % (n, tuple(coord_data.shape)))
        L.check(L.load().dpn_pverify_stage(_ptr(out_n), _ptr(_f32c(coord_data)), n, ctypes.byref(ph), int(bool(with_clip)), self.c_ids, len(self.ids),
                                           int(member), self.members, int(first), self.n_total, _ptr(self.plane_f), _ptr(self.plane_b), _stream()),
                'dpn_pverify_stage')

    def case(self, obs, first=0):
        """dpn_pverify_case: the staged case at points first .. first + n against obs [n, P] (fp32, contiguous)."""
        n, P = obs.shape[0], len(self.ids)
        if self.plane_f is None or tuple(obs.shape) != (n, P) or obs.dtype != torch.float32 or not obs.is_contiguous():
            raise ValueError('ProbVerifyState.case: a state with planes and obs a contiguous fp32 [n, %d], got %s %s' % (P, tuple(obs.shape), obs.dtype))
        L.check(L.load().dpn_pverify_case(_ptr(self.plane_f), _ptr(self.plane_b), _ptr(obs), n, P, self.c_thr_col, self.c_thr_val, self.c_thr_side,
                                          len(self.thr_col), self.members, int(first), self.n_total, ctypes.byref(self.c_state()), _stream()),
                'dpn_pverify_case')


class NbhdState:
    """Device state of a neighbourhood verification request (include/dpn_hip.h: DpnNbhdState) on `lattice`: the P columns `ids`, the E >= 1
    thresholds and the K half-widths `radius` (neighbourhood.check_scales).  The ten arrays of neighbourhood.STATE_FIELDS are views of ONE zeroed
    byte buffer, laid out as _ScoreState lays its own out (the fp64 arrays first, no gaps; here every array is 8 bytes wide); beside it the
    staging mask [nt, E, ny, nx] uint8, which `clear` leaves (the next case's stages rewrite every byte), and the scratch of `fold` for
    `planes_per_fold` planes -- as many as `budget_bytes` hold of tables and row partials, at least one.  `stage` writes one chunk's mask bytes,
    `fold` folds the staged case in, `finish` turns the state into the two tables.  ValueError: sizes out of range."""

    def __init__(self, lattice, ids, thr_col, thr_val, thr_side, radius, device, budget_bytes):
        self.lattice, self.ids = lattice, list(ids)
        self.thr_col, self.thr_val, self.thr_side = list(thr_col), [float(v) for v in thr_val], list(thr_side)
        self.radius = [int(r) for r in radius]
        P, E, K = len(self.ids), len(self.thr_col), len(self.radius)
        nx, ny, nt = int(lattice.nx), int(lattice.ny), int(lattice.nt)
        if not 1 <= P <= L.VERIFY_MAX_COLUMNS or not 1 <= E <= L.VERIFY_MAX_THRESHOLDS or len(self.thr_val) != E or len(self.thr_side) != E \
                or not 1 <= K <= L.NBHD_MAX_SCALES or lattice.n_points >= 2 ** 31:
            raise ValueError('NbhdState: %d products (1..%d), %d thresholds (1..%d), %d scales (1..%d), %d nodes (below 2^31)'
                             % (P, L.VERIFY_MAX_COLUMNS, E, L.VERIFY_MAX_THRESHOLDS, K, L.NBHD_MAX_SCALES, lattice.n_points))
        self.c_ids, self.c_thr_col, self.c_thr_val, self.c_thr_side = _request_arrays(self.ids, self.thr_col, self.thr_val, self.thr_side)
        self.c_radius = (ctypes.c_int32 * K)(*self.radius)
        self.c_lattice = lattice.c_struct()
        shapes = [(k, torch.float64, (nt, E, K)) for k in NB.SUMS] + [('windows', torch.int64, (nt, E, K))] \
            + [(k, torch.int64, (nt, E)) for k in ('n_valid', 'n_f', 'n_b', 'n_o')]
        sizes = [math.prod(shape) * 8 for _, _, shape in shapes]
        self.buffer = torch.zeros(sum(sizes), dtype=torch.uint8, device=device)
        at = 0
        for (name, dtype, shape), size in zip(shapes, sizes):
            setattr(self, name, self.buffer[at:at + size].view(dtype).view(shape))
            at += size
        self.mask = torch.zeros((nt, E, ny, nx), dtype=torch.uint8, device=device)
        self.plane_bytes = self.scratch_bytes(nx, ny, K, 1)
        blocks = max(ny, (nx + 1 + 63) // 64)                                 # dpn_nbhd_fold: one block per (plane, row) and per (plane, 64 columns)
        self.planes_per_fold = max(1, min(nt * E, int(budget_bytes) // self.plane_bytes, (2 ** 31 - 1) // blocks))
        self.scratch = torch.empty(self.planes_per_fold * self.plane_bytes, dtype=torch.uint8, device=device)

    @staticmethod
    def scratch_bytes(nx, ny, K, n_planes):
        """The scratch of dpn_nbhd_fold for n_planes planes: int32 S [np, ny + 1, nx + 1, 4], fp64 part [np, K, ny, 5], int32 rows [np, K, ny]."""
        return n_planes * (16 * (ny + 1) * (nx + 1) + 40 * K * ny + 4 * K * ny)

    def scratch_views(self, n_planes):
        """(S, part, rows) of the scratch as the last fold of n_planes planes left it."""
        nx, ny, K = int(self.lattice.nx), int(self.lattice.ny), len(self.radius)
        a, b = 16 * (ny + 1) * (nx + 1) * n_planes, 40 * K * ny * n_planes
        return (self.scratch[:a].view(torch.int32).view(n_planes, ny + 1, nx + 1, 4), self.scratch[a:a + b].view(torch.float64).view(n_planes, K, ny, 5),
                self.scratch[a + b:a + b + 4 * K * ny * n_planes].view(torch.int32).view(n_planes, K, ny))

    def clear(self):
        """Back to the state before the first case: one memset."""
        self.buffer.zero_()

    def arrays(self):
        """The arrays by DpnNbhdState's names, in its order."""
        return {k: getattr(self, k) for k in NB.STATE_FIELDS}

    def c_state(self):
        return L.DpnNbhdState(*[_ptr(v) for v in self.arrays().values()])

    def stage(self, out_n, coord_data, analysis, ph, first=0, with_clip=False):
        """dpn_nbhd_stage: one case's out_n [n, 6] and coord_data [n, 6] (fp32, contiguous) at points first .. first + n of the lattice against
        analysis [nt, P, ny, nx] (fp32, contiguous: the whole array)."""
        n, lat = out_n.shape[0], self.lattice
        shape = (int(lat.nt), len(self.ids), int(lat.ny), int(lat.nx))
        if tuple(analysis.shape) != shape or analysis.dtype != torch.float32 or not analysis.is_contiguous() or tuple(coord_data.shape) != (n, 6):
            raise ValueError('NbhdState.stage: analysis must be a contiguous fp32 %s and coord_data [%d, 6], got %s %s and %s'
                             % (list(shape), n, tuple(analysis.shape), analysis.dtype, tuple(coord_data.shape)))
        L.check(L.load().dpn_nbhd_stage(_ptr(out_n), _ptr(_f32c(coord_data)), _ptr(analysis), n, ctypes.byref(ph), int(bool(with_clip)), self.c_ids,
                                        len(self.ids), self.c_thr_col, self.c_thr_val, self.c_thr_side, len(self.thr_col),
                                        ctypes.byref(self.c_lattice), int(first), _ptr(self.mask), _stream()), 'dpn_nbhd_stage')

    def fold(self, planes_per_fold=None):
        """dpn_nbhd_fold over all nt * E planes of the staged case, `planes_per_fold` at a time (default: what the scratch holds; any number
        gives the same bits)."""
        total = int(self.lattice.nt) * len(self.thr_col)
        step = self.planes_per_fold if planes_per_fold is None else int(planes_per_fold)
        if not 1 <= step <= self.planes_per_fold:
            raise ValueError('NbhdState.fold: %d planes per launch; the scratch holds 1..%d' % (step, self.planes_per_fold))
        for p0, n_planes in _spans(total, step):
            L.check(L.load().dpn_nbhd_fold(_ptr(self.mask), ctypes.byref(self.c_lattice), len(self.thr_col), self.c_radius, len(self.radius), p0,
                                           n_planes, _ptr(self.scratch), ctypes.byref(self.c_state()), _stream()), 'dpn_nbhd_fold')

    def finish(self):
        """dpn_nbhd_finish: {'hour': table, 'all': table}, a table a dict of tensors by neighbourhood.OUT_FIELDS ([nt, E, K] and [nt, E]; [E, K]
        and [E])."""
        nt, E, K = int(self.lattice.nt), len(self.thr_col), len(self.radius)
        dev = self.buffer.device
        tables = {}
        for name, lead in (('hour', (nt, E)), ('all', (E,))):
            tables[name] = {k: torch.empty(lead + ((K,) if k in NB.SCALE_FIELDS else ()), dtype=getattr(torch, np.dtype(NB.OUT_DTYPES[k]).name), device=dev)
                            for k in NB.OUT_FIELDS}
        c_out = [L.DpnNbhdOut(*[_ptr(t[k]) for k in NB.OUT_FIELDS]) for t in (tables['hour'], tables['all'])]
        L.check(L.load().dpn_nbhd_finish(ctypes.byref(self.c_state()), nt, E, K, ctypes.byref(c_out[0]), ctypes.byref(c_out[1]), _stream()),
                'dpn_nbhd_finish')
        return tables


def _spans(total, step):
    """(first, n) of the spans of `step` that cover 0 .. total."""
    return [(first, min(step, total - first)) for first in range(0, total, step)]


class RegionState:
    """Device state of a regional-statistics request (include/dpn_hip.h: DpnRegionPlan, DpnRegionState): the plan's seg, wgt and offs on the device
    and, for nt time nodes, the P columns `ids` and the E thresholds (thr_col, thr_val of ensemble.check_thresholds), the slot-major partials w, wx
    [P, S] fp64, count, imin, imax [P, S] int32, vmin, vmax [P, S] fp32, wexc [E, S] fp64, all zeroed once.  `accumulate` folds a chunk of the flat
    point list in, `finish` turns the partials into the nine outputs.  ValueError: more than 16 columns or thresholds, nt * n_sel >= 2^31."""

    def __init__(self, plan, nt, ids, thr_col, thr_val, device):
        self.plan, self.nt, self.ids, self.thr_col, self.thr_val = plan, int(nt), list(ids), list(thr_col), [float(v) for v in thr_val]
        P, E = len(self.ids), len(self.thr_col)
        if not 1 <= P <= L.REG_MAX_COLUMNS or E > L.REG_MAX_THRESHOLDS or len(self.thr_val) != E:
            raise ValueError('RegionState: %d products (1..%d), %d thresholds (0..%d)' % (P, L.REG_MAX_COLUMNS, E, L.REG_MAX_THRESHOLDS))
        self.n_slots = S = region_slots(plan, self.nt)
        self.n_points = self.nt * plan.n_sel
        self.c_ids, self.c_thr_col, self.c_thr_val = _request_arrays(self.ids, self.thr_col, self.thr_val)
        self.seg, self.wgt, self.offs = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (plan.seg, plan.wgt, plan.offs))
        self.c_plan = L.DpnRegionPlan(_ptr(self.seg), _ptr(self.wgt), _ptr(self.offs), plan.n_sel, plan.n_regions, self.nt)
        self.w, self.wx = (torch.zeros((P, S), dtype=torch.float64, device=device) for _ in range(2))
        self.count, self.imin, self.imax = (torch.zeros((P, S), dtype=torch.int32, device=device) for _ in range(3))
        self.vmin, self.vmax = (torch.zeros((P, S), dtype=torch.float32, device=device) for _ in range(2))
        self.wexc = torch.zeros((E, S), dtype=torch.float64, device=device) if E else None

    def partials(self):
        """The eight partial arrays by DpnRegionState's names (wexc None without thresholds)."""
        return {k: getattr(self, k) for k in ('w', 'wx', 'count', 'vmin', 'vmax', 'imin', 'imax', 'wexc')}

    def c_state(self):
        return L.DpnRegionState(*[_ptr(v) for v in self.partials().values()])

    def accumulate(self, out_n, jac_n, f, ph, first, with_clip=False):
        """dpn_region_accumulate: out_n [n, 6] (jac_n [n, 6, 3], f [n], or None where no column reads them) of points first .. first + n."""
        L.check(L.load().dpn_region_accumulate(_ptr(out_n), _ptr(jac_n), _ptr(f), out_n.shape[0], ctypes.byref(ph), int(bool(with_clip)), self.c_ids,
                                               len(self.ids), self.c_thr_col, self.c_thr_val, len(self.thr_col), int(first), ctypes.byref(self.c_plan),
                                               ctypes.byref(self.c_state()), _stream()), 'dpn_region_accumulate')

    def finish(self):
        """dpn_region_finish -> dict(mean, total, weight, min, max [nt, R, P] fp32, where_min, where_max, count [nt, R, P] int32, frac [nt, R, E] fp32
        or None without thresholds), on the device."""
        dev, shape = self.w.device, (self.nt, self.plan.n_regions, len(self.ids))
        out = {k: torch.empty(shape, dtype=torch.float32, device=dev) for k in REGION_FLOAT_OUTPUTS}
        out.update({k: torch.empty(shape, dtype=torch.int32, device=dev) for k in REGION_INT_OUTPUTS})
        out['frac'] = torch.empty(shape[:2] + (len(self.thr_col),), dtype=torch.float32, device=dev) if self.thr_col else None
        table = L.DpnRegionOut(*[_ptr(out[k]) for k in REGION_FLOAT_OUTPUTS + REGION_INT_OUTPUTS + ('frac',)])
        L.check(L.load().dpn_region_finish(ctypes.byref(self.c_plan), ctypes.byref(self.c_state()), len(self.ids), self.c_thr_col, len(self.thr_col),
                                           ctypes.byref(table), _stream()), 'dpn_region_finish')
        return out


class ParcelState:
    """Device state of n parcels between two dpn_traj_stage launches: x0, y0, accx, accy [n] fp64, status, steps_done [n] int32, path
    [rows, n, 2] fp64 (row 0 = the start points; row k + 1 is written when step k closes), and `points` = x, y, t, f [n], coord_data [n, 6], the
    sampler at the current evaluation points (the next forward's input)."""

    def __init__(self, sampler, xr, yr, hour, rows):
        dev, n = xr.device, xr.shape[0]
        self.n, self.rows = n, int(rows)
        self.x0, self.y0 = xr.clone(), yr.clone()
        self.accx, self.accy = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(2))
        self.status, self.steps_done = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        self.path = torch.empty((self.rows, n, 2), dtype=torch.float64, device=dev)
        self.path[0, :, 0], self.path[0, :, 1] = xr, yr
        self.points = sampler.sample_at(n, xr, yr, torch.full((n,), float(hour), dtype=torch.float64, device=dev))


def traj_stage(sampler, ph, out_n, parcels, stage, t0, h, inv_wsum, step, fields=None, with_clip=False, record_only=False):
    """dpn_traj_stage on the parcels of a ParcelState with the forward's out_n [n, 6] at their evaluation points: stage (trajectory.Stage), the
    step's start hour t0, the step h (hours), inv_wsum, the step's index; fields [rows, n, 6] fp32 or None (written by a step's first stage and by
    record_only)."""
    st = L.DpnTrajStage(float(t0), float(h), float(stage.w), float(stage.a_next), float(stage.c_next), float(inv_wsum), int(step),
                        int(bool(stage.first)), int(bool(stage.last)), int(bool(record_only)), int(bool(with_clip)))
    p = parcels
    x, y, t, f, cd = p.points
    want_fields = fields is not None and (stage.first or record_only)
    L.check(L.load().dpn_traj_stage(ctypes.byref(sampler._s), _ptr(sampler.cube), ctypes.byref(ph), _ptr(out_n), p.n, ctypes.byref(st), _ptr(p.x0),
                                    _ptr(p.y0), _ptr(p.accx), _ptr(p.accy), _ptr(p.status), _ptr(p.steps_done), _ptr(p.path), p.rows,
                                    _ptr(fields) if want_fields else None, _ptr(x), _ptr(y), _ptr(t), _ptr(f), _ptr(cd), _stream()), 'dpn_traj_stage')


class _WindowState:
    """What the device states of the two time-window products share (ExtremeState, SpellState): n points, the request's clock K, t0, dt, their
    fp64 positions xr, yr, the state arrays KEYS [C, n] (fp64 but for those DTYPES names; nothing is filled: node 0 sets what is read), `points` =
    x, y, t, f [n], coord_data [n, 6], the sampler at the current scan node (node 0 to begin with), `probes`, the same five with probe_rows * n
    rows (None without a row), and the launches.  A subclass sets ids and c_columns (its column tables, as its entry points take them) before this
    constructor, and says what a walk must know: probe_rows, point_bytes and rounds of a request, REFINE_JACOBIAN: whether the forward at the
    probes is the one with the Jacobian."""

    def __init__(self, sampler, xr, yr, request):
        dev, n = xr.device, xr.shape[0]
        self.n, self.K, self.t0, self.dt = n, int(request.K), float(request.t0), float(request.dt)
        self.xr, self.yr = xr.contiguous(), yr.contiguous()
        for key in self.KEYS:
            setattr(self, key, torch.empty((len(self.ids), n), dtype=self.DTYPES.get(key, torch.float64), device=dev))
        self.points = sampler.sample_at(n, self.xr, self.yr, torch.full((n,), self.t0, dtype=torch.float64, device=dev))
        rows = self.probe_rows(request)
        self.probes = point_buffers(rows * n, dev) if rows else None

    def c_struct(self):
        return self.C_STATE(*[_ptr(getattr(self, key)) for key in self.KEYS])

    def _launch(self, name, sampler, bufs, head, index):
        """The entry point `name` with the argument list the scan, begin and refine launches of both products share: sampler, cube, head, n, the
        column tables, C, index, K, t0, dt, xr, yr, the state, the five buffers `bufs` it samples into, the stream.  head: () or (the physics table,
        with_clip, the forward's tensors ...); index: () or (the node or the round,)."""
        if head:
            ph, with_clip, *forward = head
            head = [ctypes.byref(ph), int(bool(with_clip))] + [_ptr(v) for v in forward]
        L.check(getattr(L.load(), name)(ctypes.byref(sampler._s), _ptr(sampler.cube), *head, self.n, *self.c_columns, len(self.ids), *index, self.K,
                                        self.t0, self.dt, _ptr(self.xr), _ptr(self.yr), ctypes.byref(self.c_struct()), *[_ptr(v) for v in bufs],
                                        _stream()), name)

    def scan(self, sampler, ph, with_clip, out_n, k):
        """The scan launch with the fields-only forward's out_n [n, 6] at scan node k."""
        self._launch(self.ENTRY + '_scan', sampler, self.points, (ph, with_clip, out_n), (int(k),))

    def begin(self, sampler):
        """The begin launch: closes the scan and writes the probes (a request without a probe row samples nothing)."""
        self._launch(self.ENTRY + '_begin', sampler, self.probes or self.points, (), ())

    def finish(self):
        """Once per chunk, after the last round (or after the scan when there is none): nothing, unless the product has a finish launch."""


class ExtremeState(_WindowState):
    """Device state of n points of a window-extremes request between its launches (include/dpn_hip.h): for the C columns of `request` (an
    extremes.Request) best_v [C, n] fp32, best_t, acc, lo, hi [C, n] fp64, best_k, status [C, n] int32 -- column-major, so a map [C, ny, nx] is a
    view of it --; `points` = x, y, t, f [n], coord_data [n, 6], the sampler at the current scan node (node 0 to begin with), and `probes`, the same
    five with Cr * n rows for the probes of the Cr max / min columns (None without one).  Nothing is filled: node 0 sets what is read."""

    ENTRY, C_STATE = 'dpn_extreme', L.DpnExtremeState
    KEYS = ('best_v', 'best_t', 'best_k', 'acc', 'status', 'lo', 'hi')
    DTYPES = {'best_v': torch.float32, 'best_k': torch.int32, 'status': torch.int32}
    REFINE_JACOBIAN = True                                    # bisection on the sign of d/dt
    POINT_BYTES = 4 * (4 + 6 + 6) + 16                       # per point: the scan's buffers and xr, yr
    COLUMN_BYTES = 4 + 8 + 4 + 8 + 4 + 8 + 8                  # per point and column: the state
    PROBE_BYTES = 4 * (4 + 6 + 6 + 18)                        # per point and refined column: the probe's buffers, its out_n and Jacobian

    def __init__(self, sampler, xr, yr, request):
        self.ids, self.senses = list(request.ids), list(request.senses)
        C, n = len(self.ids), xr.shape[0]
        self.n_refined = self.probe_rows(request)
        if not 1 <= C <= L.EXT_MAX_COLUMNS or len(self.senses) != C or n < 1:
            raise ValueError('ExtremeState: %d points, %d columns (1..%d)' % (n, C, L.EXT_MAX_COLUMNS))
        self.c_ids, self.c_senses = self.c_columns = (ctypes.c_int32 * C)(*self.ids), (ctypes.c_int32 * C)(*self.senses)
        super().__init__(sampler, xr, yr, request)

    @staticmethod
    def probe_rows(request):
        """Probe rows per point: one per max / min column."""
        return sum(1 for s in request.senses if s != L.EXT_MEAN)

    @classmethod
    def point_bytes(cls, request):
        return cls.POINT_BYTES + len(request.ids) * cls.COLUMN_BYTES + cls.probe_rows(request) * cls.PROBE_BYTES

    @classmethod
    def rounds(cls, request):
        """Refine launches of a request: round 0 probes the best node, R halve the bracket; none without a max / min column."""
        return request.R + 1 if cls.probe_rows(request) else 0

    def refine(self, sampler, ph, with_clip, out_n, jac_n, rnd):
        """dpn_extreme_refine, round rnd, with the forward's out_n [Cr * n, 6] and jac_n [Cr * n, 6, 3] at the probes."""
        self._launch('dpn_extreme_refine', sampler, self.probes, (ph, with_clip, out_n, jac_n), (int(rnd),))

    def results(self):
        """value, hour, lo, hi, status [C, n]: the state's own arrays, complete after the last round."""
        return {'value': self.best_v, 'hour': self.best_t, 'lo': self.lo, 'hi': self.hi, 'status': self.status}


class SpellState(_WindowState):
    """Device state of n points of a threshold-spells request between its launches (include/dpn_hip.h): for the C columns of `request` (a
    spells.Request) prev_x [C, n] fp32; hours, excess, part_first, part_last, f_lo, f_hi, l_lo, l_hi [C, n] fp64; crossings, k_first, k_last, status
    [C, n] int32 -- column-major, so a map [C, ny, nx] is a view of it --; `points` = x, y, t, f [n], coord_data [n, 6], the sampler at the current
    scan node (node 0 to begin with), and `probes`, the same five with 2 * C * n rows: the entry and the exit probe of every column.  Nothing is
    filled: node 0 sets what is read."""

    ENTRY, C_STATE = 'dpn_spell', L.DpnSpellState
    KEYS = ('prev_x', 'hours', 'excess', 'crossings', 'k_first', 'k_last', 'status', 'part_first', 'part_last', 'f_lo', 'f_hi', 'l_lo', 'l_hi')
    DTYPES = dict({key: torch.int32 for key in ('crossings', 'k_first', 'k_last', 'status')}, prev_x=torch.float32)
    REFINE_JACOBIAN = False                                   # bisection on the sign of value - threshold
    POINT_BYTES = 4 * (4 + 6 + 6) + 16                       # per point: the scan's buffers and xr, yr
    COLUMN_BYTES = 4 + 8 * 8 + 4 * 4 + 2 * 4 * (4 + 6 + 6)    # per point and column: the state; the two probes' buffers and their out_n

    def __init__(self, sampler, xr, yr, request):
        self.ids, self.sides, self.thr = list(request.ids), list(request.sides), [float(v) for v in request.thr]
        C, n = len(self.ids), xr.shape[0]
        if not 1 <= C <= L.SPELL_MAX_COLUMNS or len(self.sides) != C or len(self.thr) != C or n < 1:
            raise ValueError('SpellState: %d points, %d columns (1..%d)' % (n, C, L.SPELL_MAX_COLUMNS))
        self.c_ids, self.c_sides, self.c_thr = self.c_columns = \
            (ctypes.c_int32 * C)(*self.ids), (ctypes.c_int32 * C)(*self.sides), (ctypes.c_float * C)(*self.thr)
        super().__init__(sampler, xr, yr, request)

    @staticmethod
    def probe_rows(request):
        """Probe rows per point: the entry and the exit probe of every column."""
        return 2 * len(request.ids)

    @classmethod
    def point_bytes(cls, request):
        return cls.POINT_BYTES + len(request.ids) * cls.COLUMN_BYTES

    @staticmethod
    def rounds(request):
        """Refine launches of a request: R halvings of both brackets."""
        return request.R

    def refine(self, sampler, ph, with_clip, out_n, jac_n, rnd):
        """dpn_spell_refine, round rnd, with the fields-only forward's out_n [2 * C * n, 6] at the probes (jac_n: None, not read)."""
        self._launch('dpn_spell_refine', sampler, self.probes, (ph, with_clip, out_n), (int(rnd),))

    def finish(self):
        """dpn_spell_finish: once, after the last round (or after the scan when there is none)."""
        L.check(L.load().dpn_spell_finish(self.n, len(self.ids), self.K, self.t0, self.dt, ctypes.byref(self.c_struct()), _stream()), 'dpn_spell_finish')

    def results(self):
        """hours, first, last, first_lo, last_hi, excess, crossings, status [C, n]: the state's own arrays, complete after dpn_spell_finish."""
        return {'hours': self.hours, 'first': self.f_hi, 'last': self.l_lo, 'first_lo': self.f_lo, 'last_hi': self.l_hi, 'excess': self.excess,
                'crossings': self.crossings, 'status': self.status}


