"""Per-point weights and causal time weighting of the PDE losses (csrc/dpn_causal.hip): the option's value type and
the host references in numpy fp64.

Causal training (Wang, Sankaran & Perdikaris 2022, "Respecting causality is all you need for training physics-informed neural networks") cuts the time
axis into bins and lets a bin's residual loss count only once the earlier bins are fitted: W_k = exp(-eps * sum_{j<k} l_j), l_j the mean point loss of
bin j.  `CausalWeights` carries the option through pde_losses / step_losses / InterfacePhysics; the three references restate what the kernels define --
the bin of a time, the weights of the bins, the weighted losses -- from the kernels' own per-point residuals, and the GPU tests hold the kernels to
them.  Nothing here runs in training.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

MAX_BINS = 64          # DPN_CAUSAL_MAX_BINS (include/dpn_hip.h)
CRIT_MSE, CRIT_L1, CRIT_SMOOTH_L1 = 0, 1, 2          # DpnPhysics.criterion


@dataclass(frozen=True)
class CausalWeights:
    """eps: the causality parameter (>= 0; 0 switches the weighting off: every W_k = 1).  bins: the number of equal time bins over t_range (1..64).
    relative: divide every bin loss by the mean over the non-empty bins before the prefix sum, so that eps is a pure number (the loss factors here span
    1e-7 .. 1e14: an absolute eps is unusable without knowing the loss scale); False is the paper's literal form.  t_range = (t_lo, t_hi) in the units
    of the points' t; None: (0, the geometry's pred_t_span)."""
    eps: float
    bins: int = 16
    relative: bool = True
    t_range: Optional[Tuple[float, float]] = None

    def __post_init__(self):
        eps = float(self.eps)
        if not (np.isfinite(eps) and eps >= 0.0):
            raise ValueError('CausalWeights: eps must be finite and >= 0, got %r' % (self.eps,))
        if isinstance(self.bins, bool) or int(self.bins) != self.bins or not 1 <= int(self.bins) <= MAX_BINS:
            raise ValueError('CausalWeights: bins must be an integer in 1..%d, got %r' % (MAX_BINS, self.bins))
        if self.t_range is not None:
            if len(self.t_range) != 2:
                raise ValueError('CausalWeights: t_range must be (t_lo, t_hi), got %r' % (self.t_range,))
            lo, hi = float(self.t_range[0]), float(self.t_range[1])
            if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
                raise ValueError('CausalWeights: t_range must be finite with t_hi > t_lo, got %r' % (self.t_range,))
            object.__setattr__(self, 't_range', (lo, hi))
        object.__setattr__(self, 'eps', eps)
        object.__setattr__(self, 'bins', int(self.bins))
        object.__setattr__(self, 'relative', bool(self.relative))

    def bounds(self, pred_t_span):
        """(t_lo, t_hi) as doubles: t_range, or (0, pred_t_span)."""
        return self.t_range if self.t_range is not None else (0.0, float(pred_t_span))


def bin_index(t, t_lo, t_hi, bins):
    """The time bin of every t (fp32 values, as the point kernels read them): clamp(floor((t - t_lo) * bins / (t_hi - t_lo)), 0, bins - 1), every
    operation in fp64 in this order, as dpn_causal_bins forms it; a NaN goes to bin 0.  -> int32 [n]."""
    t_lo, t_hi, bins = float(t_lo), float(t_hi), int(bins)
    if not (np.isfinite(t_lo) and np.isfinite(t_hi) and t_hi > t_lo and 1 <= bins <= MAX_BINS):
        raise ValueError('bin_index: need finite t_lo < t_hi and 1 <= bins <= %d, got %r, %r, %r' % (MAX_BINS, t_lo, t_hi, bins))
    t64 = np.ascontiguousarray(t, dtype=np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        pos = np.floor(((t64 - t_lo) * float(bins)) / (t_hi - t_lo))
        pos = np.where(pos >= 0.0, np.minimum(pos, float(bins - 1)), 0.0)          # (NaN >= 0 is False)
    return pos.astype(np.int32)


def _rho(res, criterion, beta):
    """rho(r) in fp64 as dpn_residual sums it: MSE squares in fp64, L1 / SmoothL1 take the fp32 criterion value cast up."""
    r32 = np.ascontiguousarray(res, dtype=np.float32)
    if criterion == CRIT_MSE:
        r = r32.astype(np.float64)
        return r * r
    ar = np.abs(r32)
    if criterion == CRIT_L1:
        return ar.astype(np.float64)
    if criterion != CRIT_SMOOTH_L1 or not float(beta) > 0.0:
        raise ValueError('criterion must be 0 (MSE), 1 (L1) or 2 (SmoothL1 with beta > 0), got %r, beta %r' % (criterion, beta))
    b = np.float32(beta)
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.where(ar < b, np.float32(0.5) * r32 * r32 / b, ar - np.float32(0.5) * b)           # fp32 throughout, the kernel's order
    return v.astype(np.float64)


def point_loss_reference(res, factors, criterion=CRIT_MSE, beta=0.0):
    """s_i = sum_e factors[e] * rho(res[i, e]), e ascending, fp64 (dpn_causal_bins' point loss) from residual rows res [n, 6]."""
    rho = _rho(np.asarray(res).reshape(-1, 6), criterion, beta)
    s = np.zeros(rho.shape[0], dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for e in range(6):
            s = s + float(factors[e]) * rho[:, e]
    return s


def bin_weights_reference(point_loss, bin, bins, eps, relative=True):
    """-> W [bins], l [bins] (un-normalised), count [bins]: l_k = the mean of point_loss over bin k (0 for an empty bin); relative: l is divided by its
    mean over the non-empty bins (all W = 1 when that mean is not finite or not > 0); W_k = exp(-eps * cum_k), cum the sequential exclusive prefix sum."""
    eps, bins = float(eps), int(bins)
    if not (np.isfinite(eps) and eps >= 0.0 and 1 <= bins <= MAX_BINS):
        raise ValueError('bin_weights_reference: need finite eps >= 0 and 1 <= bins <= %d, got %r, %r' % (MAX_BINS, eps, bins))
    s = np.ascontiguousarray(point_loss, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(bin).reshape(-1).astype(np.int64)
    if s.size == 0 or s.size != b.size or b.min() < 0 or b.max() >= bins:
        raise ValueError('bin_weights_reference: point_loss and bin must be the same non-zero length, bin in 0..bins - 1')
    l, count = np.zeros(bins), np.zeros(bins)
    for k in range(bins):
        sel = s[b == k]
        count[k] = sel.size
        if sel.size:
            tot = 0.0
            for v in sel:                                   # sequential, point order
                tot = tot + v
            l[k] = tot / sel.size
    norm = 1.0
    if relative:
        tot = 0.0
        for k in range(bins):
            if count[k] > 0:
                tot = tot + l[k]
        norm = tot / float((count > 0).sum())
        if not (norm > 0.0 and np.isfinite(norm)):
            return np.ones(bins), l, count
    W, cum = np.zeros(bins), 0.0
    with np.errstate(over='ignore', invalid='ignore'):
        for k in range(bins):
            W[k] = np.exp(-eps * cum)
            cum = cum + (l[k] / norm if relative else l[k])
    return W, l, count


def weighted_losses_reference(res, weights, factors, criterion=CRIT_MSE, beta=0.0, reduce_sum=False):
    """The six weighted losses factor_e * sum_i w_i rho(res[i, e]) / n (reduce_sum: not divided) in fp64 from residual rows res [n, 6] and point
    weights [n]: what dpn_residual_weighted + dpn_residual_finish compute in fp64 block sums and one fp32 rounding each."""
    rho = _rho(np.asarray(res).reshape(-1, 6), criterion, beta)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size != rho.shape[0]:
        raise ValueError('weighted_losses_reference: %d weights for %d points' % (w.size, rho.shape[0]))
    tot = (w[:, None] * rho).sum(0)
    if not reduce_sum:
        tot = tot / rho.shape[0]
    return tot * np.asarray([float(v) for v in factors], dtype=np.float64)
