"""Fused clip_grad_norm_ + Adam on the HIP library (reference: interface_physics.py:514-515, cfg:151-155).

Same arithmetic as `torch.nn.utils.clip_grad_norm_(params, max_norm)` followed by `torch.optim.Adam(lr, betas, eps,
weight_decay)` (weight decay added to the gradient), but three kernel launches for the whole model instead of ~60, and
hipGraph-capturable: the step counter AND the hyper-parameters (learning rate included) live on the device, so a captured step follows
a learning-rate schedule (`CosineAnnealingLR` stepped once per epoch, interface_physics.py:396-397, :831-833).

It is a `torch.optim.Optimizer`: `param_groups`, `state` (per parameter `step`, `exp_avg`, `exp_avg_sq` -- the keys of
torch.optim.Adam, so the state dicts load both ways: a torch.optim.Adam state dict gets this optimiser's own extras, max_norm, from its
defaults), `state_dict` / `load_state_dict`, and every torch LR scheduler attaches.

Gradients: the optimiser owns ONE flat fp32 gradient buffer laid out like its flat moment buffers (grad_arena.py).  The autograd
nodes of this package write parameter gradients straight into it, the data-parallel all-reduce (distributed.GradientAllReduce) runs in
place on its bucket slices, and the kernels read it -- gradients that arrive elsewhere (foreign autograd nodes) are copied in first.
`layout`: optional list of parameter lists = the buckets in the order their gradients become ready in the backward pass.

Weight EMA (`ema_decay`, off by default): a shadow copy of the parameters, s' = d s + (1 - d) p', moved inside the update launch by the thread
that has just formed p' (dpn_clip_adam_flat_ema: no extra launch, and a step replayed from a hipGraph moves it too).  With `ema_warmup` the decay
is min(ema_decay, (1 + n) / (10 + n)), n = the number of EMA updates so far (device step counter + `ema_base`), so a young average is not
dominated by the initial weights.  `ema_weights()` exchanges parameters and shadow for validation, `ema_state_dict()` writes the shadow out as a
module state dict.

Parameter groups (fine-tuning): the constructor takes torch's list-of-dicts form, every group with its own lr, betas, eps and weight_decay; the
clip stays global (one max_norm, the norm over every optimised parameter) and so do the step counter and the EMA decay.  Several groups run
dpn_clip_adam_flat_groups (the same three launches; the update kernel looks up its tensor's group row), one group runs exactly the entry points it
always ran.  The optimiser owns only the parameters it is given: a frozen parameter of the module has no slot, no moments and no shadow.
`resolve_param_groups` turns name patterns (train_cfg['optimizer']['freeze'] / ['param_groups']) into those groups.

Step guard (`skip_nonfinite`, `spike_factor`; off by default): the update is refused on the device when the total gradient norm is NaN / +-inf, or
-- with a spike_factor -- more than spike_factor times the running mean of the applied steps' norms (after spike_warmup applied steps, at most
spike_patience times in a row; guard.py states the rule).  It runs inside the same three launches (dpn_clip_adam_flat_guard: one thread of the
reduction launch forms the verdict, the update launch returns early), so a step replayed from a hipGraph is guarded too.  A refused step leaves
every byte of the parameters, the moments and the EMA shadow as it was; the device step counter `step_count` -- and `state[p]['step']`, which keeps
pointing at it -- still advances: with the guard it counts CALLS, not updates (a sampler bound to it draws new points after a skipped step);
`effective_step()` is the number of updates, the t of the bias corrections.  Without these options the optimiser makes exactly the calls it made
before.  Not seen: a non-finite loss whose gradients are all finite; a finite |g| above about 1.8e19 overflows the fp32 partial and is skipped as
non-finite.
"""
import contextlib
import ctypes
import fnmatch
import math
import weakref
from collections import OrderedDict

import warnings

import numpy as np
import torch

from . import _lib as L
from . import grad_arena
from .guard import FIELDS as GUARD_FIELDS, StepGuard

_CHUNK = 2048            # dpn_clip_adam_flat: every tensor is padded to whole 2048-element chunks
MAX_GROUPS = 16          # dpn_clip_adam_flat_groups: kAdamMaxGroups
GROUP_KEYS = ('lr', 'betas', 'eps', 'weight_decay')       # what a parameter group may set: Adam's hyper-parameters


def resolve_param_groups(named_parameters, freeze=None, groups=None, defaults=None):
    """Name patterns -> parameter groups, without touching a parameter (no GPU needed).

    named_parameters: (name, parameter) pairs in the module's order (state-dict names); a parameter whose `requires_grad` is already False counts
    as frozen.  freeze: fnmatch patterns of the parameters to freeze.  groups: [dict(match=[patterns], lr=..., weight_decay=..., betas=..., eps=...)]
    -- a trainable parameter belongs to the FIRST group one of whose patterns matches its name; the trainable parameters no group claims form the
    last group, with `defaults` (a dict of the same four keys, may be empty) and nothing else.  A group's missing keys are filled from `defaults`.
    Returns (frozen names, [dict(names=[...], params=[...], **hyper-parameters)]).
    ValueError: a pattern (of freeze or of a group) that matches no name at all, a freeze that leaves nothing trainable, a group key that is not
    one of match, lr, betas, eps, weight_decay, a group left without parameters (everything it matches is frozen or claimed by an earlier
    group), more than 16 groups."""
    named = [(str(k), p) for k, p in named_parameters]
    names = [k for k, _ in named]
    defaults = dict(defaults or {})
    for k in defaults:
        if k not in GROUP_KEYS:
            raise ValueError('param_groups: %r is not an Adam hyper-parameter of a group (%s)' % (k, ', '.join(GROUP_KEYS)))
    as_list = lambda x: [x] if isinstance(x, str) else list(x or ())

    def matching(pattern, what):
        hit = set(fnmatch.filter(names, pattern))
        if not hit:
            raise ValueError('%s: the pattern %r matches no parameter name' % (what, pattern))
        return hit

    frozen = {k for k, p in named if not getattr(p, 'requires_grad', True)}
    for pat in as_list(freeze):
        frozen |= matching(pat, 'freeze')
    if len(frozen) == len(names):
        raise ValueError('freeze: no trainable parameter is left')
    out, claimed = [], set(frozen)
    for gi, g in enumerate(groups or ()):
        g = dict(g)
        pats = as_list(g.pop('match', None))
        if not pats:
            raise ValueError('param_groups[%d]: `match` (a list of name patterns) is required' % gi)
        for k in g:
            if k not in GROUP_KEYS:
                raise ValueError('param_groups[%d]: %r is not an Adam hyper-parameter of a group (%s)' % (gi, k, ', '.join(GROUP_KEYS)))
        if 'betas' in g:
            g['betas'] = tuple(float(b) for b in g['betas'])
        hit = set()
        for pat in pats:
            hit |= matching(pat, 'param_groups[%d]' % gi)
        mine = [k for k in names if k in hit and k not in claimed]
        if not mine:
            raise ValueError('param_groups[%d]: every parameter it matches is frozen or belongs to an earlier group' % gi)
        claimed |= set(mine)
        out.append(dict(defaults, **g, names=mine))
    rest = [k for k in names if k not in claimed]
    if rest:
        out.append(dict(defaults, names=rest))
    if len(out) > MAX_GROUPS:
        raise ValueError('param_groups: %d groups, the fused optimiser takes at most %d' % (len(out), MAX_GROUPS))
    by_name = dict(named)
    for g in out:
        g['params'] = [by_name[k] for k in g['names']]
    return [k for k in names if k in frozen], out


class FusedClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=2.5e7, layout=None, ema_decay=None, ema_warmup=True,
                 skip_nonfinite=False, spike_factor=None, spike_decay=0.99, spike_warmup=100, spike_patience=5):
        # the step guard: a spike_factor implies the non-finite rule; neither: None, and step() never reaches dpn_clip_adam_flat_guard
        self.step_guard = (StepGuard(spike_factor, spike_decay, spike_warmup, spike_patience)
                           if (skip_nonfinite or (spike_factor is not None and float(spike_factor) != 0.0)) else None)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=float(max_norm))
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not (math.isfinite(ema_decay) and 0.0 <= ema_decay < 1.0):
                raise ValueError('FusedClipAdam: ema_decay must be a finite number in [0, 1), got %r' % (ema_decay,))
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)       # attributes, not param_groups entries: state dicts keep their keys
        self._built = False
        super().__init__(params, defaults)
        self._built = True                                          # from here on add_param_group refuses
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError('FusedClipAdam takes at most %d parameter groups, got %d' % (MAX_GROUPS, len(self.param_groups)))
        for g in self.param_groups:                                 # the clip is global: one norm over every optimised parameter, one max_norm
            if float(g['max_norm']) != defaults['max_norm']:
                raise ValueError('FusedClipAdam: max_norm is one value for the optimiser (%r), a parameter group names %r'
                                 % (defaults['max_norm'], g['max_norm']))
            g['betas'] = tuple(g['betas'])
        given = [p for g in self.param_groups for p in g['params']]   # the optimised set: what the groups hold, nothing else of the module
        if not given or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in given):
            raise RuntimeError('FusedClipAdam needs contiguous fp32 HIP parameters (no CPU fallback)')
        if layout is None:
            layout = [given]
        flat_order = [p for b in layout for p in b]
        if len(flat_order) != len(given) or {id(p) for p in flat_order} != {id(p) for p in given}:
            raise ValueError('layout must partition exactly the optimised parameters')
        self.params = flat_order                                   # kernel / flat-buffer order (bucket after bucket)
        dev = self.params[0].device
        n = len(self.params)
        lib = L.load()
        self._numel = (ctypes.c_int64 * n)(*[p.numel() for p in self.params])
        # [0] = sum of squares of all gradients, then one fp64 partial per 2048-element chunk (fixed-order reduction, no atomics)
        self._sumsq = torch.zeros(int(lib.dpn_clip_adam_scratch_doubles(n, self._numel)), dtype=torch.float64, device=dev)
        total = int(lib.dpn_clip_adam_flat_floats(n, self._numel))
        # moments and gradients as ONE flat buffer each: no per-tensor state pointers in the kernel arguments, one launch per pass
        self._m_flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v_flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._g_flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._offsets, off = [], 0
        for p in self.params:
            self._offsets.append(off)
            off += ((p.numel() + _CHUNK - 1) // _CHUNK) * _CHUNK
        self.layout_ids = [[id(p) for p in b] for b in layout]       # which parameters each bucket of the flat buffers holds
        self.bucket_bounds, pos, k = [], 0, 0                       # [(start, end)] float offsets of each layout bucket in the flat buffers
        for b in layout:
            end = self._offsets[k + len(b)] if k + len(b) < n else total
            self.bucket_bounds.append((pos, end))
            pos, k = end, k + len(b)
        self.exp_avg = [self._m_flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.params)]
        self.exp_avg_sq = [self._v_flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.params)]
        self._slots = [self._g_flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.params)]
        for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq):       # torch.optim.Adam's state keys
            self.state[p] = {'step': self.step_count, 'exp_avg': m, 'exp_avg_sq': v}
        self._p = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.params])
        self._g = (ctypes.c_void_p * n)(*[s.data_ptr() for s in self._slots])
        # [lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale] on the device, read by the kernels at run time; several groups: a row each,
        # and the group of every tensor in kernel order (dpn_clip_adam_flat_groups)
        n_groups = len(self.param_groups)
        self._hyper = torch.zeros(8 if n_groups == 1 else (n_groups, 8), dtype=torch.float32, device=dev)
        group_of = {id(p): k for k, g in enumerate(self.param_groups) for p in g['params']}
        self._group_of = (ctypes.c_uint8 * n)(*[group_of[id(p)] for p in self.params])
        self._hyper_host = None
        self.grad_scale = 1.0
        self.steps_done = 0                                         # host-side count of step() calls (point_path's forward / backward stamps)
        self._leased = set()                                        # offsets of the slots a live gradient may alias (grad_arena)
        self._ptrs = [p.data_ptr() for p in self.params]            # what the kernels write through: checked against the live tensors every step
        self._ema_flat, self.ema, self.ema_base, self._ema_swapped, self._module = None, None, None, False, None
        if ema_decay is not None:
            self._ema_flat = torch.zeros(total, dtype=torch.float32, device=dev)
            self.ema = [self._ema_flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.params)]
            self.ema_base = torch.zeros(1, dtype=torch.int32, device=dev)       # EMA updates made before this optimiser was built (load_ema)
            self.reset_ema()
        # DpnStepGuard on the device, zero-initialised: 6 int32 + 2 fp64 = 5 eight-byte words
        self._guard = torch.zeros(5, dtype=torch.int64, device=dev) if self.step_guard is not None else None
        self.sync_hyper()
        grad_arena.register(self, self.params, self._offsets)

    def add_param_group(self, param_group):
        if getattr(self, '_built', False):
            raise NotImplementedError('FusedClipAdam.add_param_group: the flat buffers are laid out at construction; build a new optimiser over the '
                                      'new groups and load_state_dict the old state into it')
        super().add_param_group(param_group)

    def __del__(self):
        try:
            grad_arena.unregister(self)
        except Exception:                                           # interpreter shutdown
            pass

    def _check_pointers(self):
        """The kernels update the parameters through the raw pointers taken at construction: a `model.to(...)` / `param.data = ...` after
        build_optimizer would leave them writing into freed memory."""
        for p, ptr in zip(self.params, self._ptrs):
            if p.data_ptr() != ptr:
                raise RuntimeError('%s: a parameter of shape %s was re-allocated after the optimiser was built (model.to() / '
                                   'param.data assignment); build the optimiser again' % (type(self).__name__, tuple(p.shape)))

    # ---- hyper-parameters ----------------------------------------------------------------------------------------------
    @property
    def max_norm(self):
        return self.param_groups[0]['max_norm']

    @max_norm.setter
    def max_norm(self, v):
        for g in self.param_groups:
            g['max_norm'] = float(v)

    def _hyper_values(self):
        """One group: its row; several: a tuple of rows (max_norm, grad_scale and the decay are read from row 0, every row carries them)."""
        rows = tuple((float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), float(self.max_norm),
                      float(self.grad_scale), 0.0 if self.ema_decay is None else self.ema_decay) for g in self.param_groups)
        return rows[0] if len(rows) == 1 else rows

    def sync_hyper(self):
        """Upload every group's row (lr after a scheduler step, ...) to the device scalars the kernels read.  step() does it by itself
        outside a graph capture; call it after `scheduler.step()` when the optimiser step is replayed from a hipGraph."""
        vals = self._hyper_values()
        if vals != self._hyper_host:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FusedClipAdam: hyper-parameters changed during a graph capture; call sync_hyper() before capturing')
            self._hyper.copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=False)
            self._hyper_host = vals

    # ---- gradients -----------------------------------------------------------------------------------------------------
    def flat_gradients(self):
        """The flat gradient buffer (every tensor padded to whole 2048-element chunks, buckets back to back: `bucket_bounds`)."""
        return self._g_flat

    def gather_gradients(self, zero_missing=False):
        """Make `p.grad` of every parameter the view of its arena slot: gradients produced elsewhere are copied in (none on the fused
        path); a parameter without gradient raises, or -- zero_missing, for ranks whose graphs differ -- contributes zeros."""
        for p, s in zip(self.params, self._slots):
            g = p.grad
            if g is None:
                if not zero_missing:
                    raise RuntimeError('%s: a parameter has no gradient' % type(self).__name__)
                s.zero_()
            elif g.data_ptr() != s.data_ptr() or not g.is_contiguous():
                s.copy_(g)
            else:
                continue
            p.grad = s

    def place_gradients(self, params, grads):
        """`p.grad = g` for gradients handed back by torch.autograd.grad (staged backward): a gradient that is not already the
        parameter's slot is copied into it (None: zeros), so that the bucket's all-reduce -- which may start right after -- sees it."""
        if getattr(self, '_slot_of', None) is None:
            self._slot_of = {id(p): s for p, s in zip(self.params, self._slots)}
        for p, g in zip(params, grads):
            s = self._slot_of.get(id(p))
            if s is None:                           # not this optimiser's (a frozen parameter): its gradient is dropped
                continue
            if g is None:
                s.zero_()
            elif g.data_ptr() != s.data_ptr() or not g.is_contiguous():
                s.copy_(g)
            p.grad = s

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()
        if set_to_none:
            self._leased.clear()                                    # no param.grad aliases a slot any more: the next backward writes in place

    # ---- step ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_pointers()
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam: step() inside ema_weights(): the parameters hold the averaged weights')
        self.gather_gradients()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        else:
            grad_arena.captured_step[0] = True      # replays of this step rewrite the parameters without passing through here
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        grouped, ema, sg = len(self.param_groups) > 1, self._ema_flat is not None, self.step_guard
        # what every entry point takes first, then the tails of the options
        head = (len(self.params), self._p, self._g, self._numel, ptr(self._m_flat), ptr(self._v_flat), ptr(self._sumsq), ptr(self.step_count))
        hyper = (ptr(self._hyper), ptr(self.grad_norm))
        ema_tail = (ptr(self._ema_flat), ptr(self.ema_base), int(self.ema_warmup)) if ema else (None, None, int(self.ema_warmup))
        if sg is not None:
            # one path for one group or several, with or without EMA, eager or captured
            entry, args = 'dpn_clip_adam_flat_guard', (head + (self._group_of if grouped else None, len(self.param_groups)) + hyper + ema_tail +
                                                       (ptr(self._guard), sg.spike_factor, sg.spike_decay, sg.spike_warmup, sg.spike_patience))
        elif grouped:
            entry, args = 'dpn_clip_adam_flat_groups', head + (self._group_of, len(self.param_groups)) + hyper + ema_tail
        elif ema:
            entry, args = 'dpn_clip_adam_flat_ema', head + hyper + ema_tail
        else:
            entry, args = 'dpn_clip_adam_flat_dev', head + hyper
        L.check(getattr(L.load(), entry)(*args, torch.cuda.current_stream().cuda_stream), entry)
        grad_arena.param_epoch[0] += 1
        self.steps_done += 1
        return self.grad_norm if closure is None else loss

    # ---- step guard ----------------------------------------------------------------------------------------------------
    def guard_stats(self):
        """The DpnStepGuard struct as a dict (skipped_nonfinite, skipped_spike, verdict, seen, consecutive, reserved, running, last).  Reads the
        device, so it synchronises: meant for log steps."""
        if self._guard is None:
            raise RuntimeError('FusedClipAdam.guard_stats: the optimiser was built without skip_nonfinite / spike_factor')
        raw = self._guard.cpu().numpy()
        ints, dbl = raw.view(np.int32), raw.view(np.float64)
        out = {k: int(ints[i]) for i, k in enumerate(GUARD_FIELDS[:6])}
        out.update(running=float(dbl[3]), last=float(dbl[4]))
        return out

    def _load_guard(self, stats):
        raw = np.zeros(5, np.int64)
        if stats is not None:
            raw.view(np.int32)[:6] = [int(stats.get(k, 0)) for k in GUARD_FIELDS[:6]]
            raw.view(np.float64)[3:] = [float(stats.get('running', 0.0)), float(stats.get('last', 0.0))]
        self._guard.copy_(torch.from_numpy(raw))

    def effective_step(self):
        """The number of updates applied, the t of the bias corrections: the device step counter minus the skipped calls (reads the device)."""
        if self._guard is None:
            return int(self.step_count)
        st = self.guard_stats()
        return int(self.step_count) - st['skipped_nonfinite'] - st['skipped_spike']

    # ---- weight EMA ----------------------------------------------------------------------------------------------------
    def _need_ema(self, what):
        if self._ema_flat is None:
            raise RuntimeError('FusedClipAdam.%s: the optimiser was built without ema_decay' % what)

    @torch.no_grad()
    def reset_ema(self):
        """The shadow becomes the parameters' current values (the EMA update counters stay)."""
        self._need_ema('reset_ema')
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam.reset_ema inside ema_weights()')
        for s, p in zip(self.ema, self.params):
            s.copy_(p.detach())

    def ema_updates(self):
        """EMA updates made so far: the applied steps (the device step counter, without the calls the step guard skipped) plus `ema_base` (reads
        the device)."""
        self._need_ema('ema_updates')
        return self.effective_step() + int(self.ema_base)

    def bind_module(self, module):
        """The module whose parameter names `load_ema` uses (kept as a weak reference)."""
        self._module = weakref.ref(module)

    def _ema_swap(self):
        L.check(L.load().dpn_ema_swap(len(self.params), self._p, self._numel, ctypes.c_void_p(self._ema_flat.data_ptr()),
                                      torch.cuda.current_stream().cuda_stream), 'dpn_ema_swap')
        grad_arena.param_epoch[0] += 1             # the parameters changed through raw pointers, as in step(): caches keyed on the epoch miss

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameters hold the averaged weights and the shadow the raw ones (one in-place exchange each way, no copy of the
        model): validation and inference on the EMA.  No nesting, no step() inside, not during a graph capture."""
        self._need_ema('ema_weights')
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam.ema_weights() does not nest')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedClipAdam.ema_weights() during a graph capture: a replay would exchange the weights again')
        self._check_pointers()
        self._ema_swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_swapped = False

    def ema_state_dict(self, module):
        """`module.state_dict()` with every optimised parameter replaced by a clone of its shadow: same names, shapes and order; buffers and
        parameters this optimiser does not hold (frozen ones) come from the module with their own values, so the result is a complete state dict."""
        self._need_ema('ema_state_dict')
        self.bind_module(module)
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam.ema_state_dict inside ema_weights()')
        shadow = {id(p): s for p, s in zip(self.params, self.ema)}
        named = {k: shadow[id(p)] for k, p in module.named_parameters(remove_duplicate=False) if id(p) in shadow}
        return OrderedDict((k, (named[k] if k in named else v).detach().clone()) for k, v in module.state_dict().items())

    @torch.no_grad()
    def load_ema(self, state_dict, updates, module=None):
        """Fill the shadow from an `ema_state_dict` (strict: every optimised parameter's name must be there with its shape; entries for parameters
        this optimiser does not own are ignored) and set `ema_base` so
        that step counter + base = `updates`: the warm-up of a resumed run does not restart.  The names are those of `module`, or of the module
        last given to `bind_module` / `ema_state_dict`."""
        self._need_ema('load_ema')
        module = self._module() if module is None and self._module is not None else module
        if module is None:
            raise RuntimeError('FusedClipAdam.load_ema: no module to take the parameter names from (bind_module)')
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam.load_ema inside ema_weights()')
        shadow = {id(p): s for p, s in zip(self.params, self.ema)}
        names = {k: shadow[id(p)] for k, p in module.named_parameters(remove_duplicate=False) if id(p) in shadow}
        missing = [k for k in names if k not in state_dict]
        if missing:
            raise KeyError('FusedClipAdam.load_ema: the state dict lacks %s' % ', '.join(missing[:5]))
        for k, s in names.items():
            if tuple(state_dict[k].shape) != tuple(s.shape):
                raise ValueError('FusedClipAdam.load_ema: %s has shape %s, expected %s' % (k, tuple(state_dict[k].shape), tuple(s.shape)))
        for k, s in names.items():
            s.copy_(state_dict[k])
        self.ema_base.fill_(int(updates) - self.effective_step())

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        step = self.step_count.detach().to(torch.float32).reshape(()).cpu()
        # copies, detached from the flat buffers (the packed state shares its per-parameter dicts with self.state); `step` as
        # torch.optim.Adam stores it
        sd['state'] = {k: {'step': step.clone(), 'exp_avg': st['exp_avg'].detach().clone(), 'exp_avg_sq': st['exp_avg_sq'].detach().clone()}
                       for k, st in sd['state'].items()}
        if self._ema_flat is not None:
            # sd['state'] is keyed by the parameter's index over the groups' 'params' lists, group after group (the order they were given in)
            shadow = {id(p): s for p, s in zip(self.params, self.ema)}
            for k, p in enumerate(p for g in self.param_groups for p in g['params']):
                sd['state'][k]['ema'] = shadow[id(p)].detach().clone()
            sd['ema_updates'] = self.ema_updates()
        if self._guard is not None:                 # the guard's struct and its parameters: a resumed run keeps its running mean and its counts
            sd['step_guard'] = dict(self.step_guard.as_dict(), state=self.guard_stats())
        return sd

    def load_state_dict(self, state_dict):
        views = {id(p): (m, v) for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq)}
        if self._ema_swapped:
            raise RuntimeError('FusedClipAdam.load_state_dict inside ema_weights()')
        ema_updates = state_dict.get('ema_updates')
        saved_guard = state_dict.get('step_guard')
        if ema_updates is not None or saved_guard is not None:      # torch's load_state_dict knows 'state' and 'param_groups' only
            state_dict = {k: v for k, v in state_dict.items() if k not in ('ema_updates', 'step_guard')}
        if saved_guard is not None and self._guard is None:
            warnings.warn('FusedClipAdam.load_state_dict: the state dict carries a step guard (%d + %d skipped calls), this optimiser was built '
                          'without one: ignored' % (saved_guard['state']['skipped_nonfinite'], saved_guard['state']['skipped_spike']))
        super().load_state_dict(state_dict)
        for g in self.param_groups:                 # a torch.optim.Adam state dict has no 'max_norm' (load_state_dict replaces the groups wholesale)
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        self.max_norm = self.param_groups[0]['max_norm']
        step = None
        shadow = {id(p): s for p, s in zip(self.params, self.ema)} if self._ema_flat is not None else {}
        have_ema = bool(shadow) and ema_updates is not None
        for p in (p for g in self.param_groups for p in g['params']):
            st = self.state.get(p, {})
            m, v = views[id(p)]
            if have_ema and 'ema' in st:
                shadow[id(p)].copy_(st['ema'])
            elif shadow:                            # a state dict without EMA: the average starts from the current parameters
                have_ema = False
            if 'exp_avg' in st:
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                step = st.get('step', step)
            self.state[p] = {'step': self.step_count, 'exp_avg': m, 'exp_avg_sq': v}
        if step is not None:
            self.step_count.fill_(int(float(step)))
        if self._guard is not None:                 # a state dict without the guard: a zeroed one (every call so far counts as applied)
            self._load_guard(None if saved_guard is None else saved_guard['state'])
        if shadow:
            if have_ema:
                self.ema_base.fill_(int(ema_updates) - self.effective_step())
            else:
                self.reset_ema()
                self.ema_base.zero_()
        self._hyper_host = None
        self.sync_hyper()
