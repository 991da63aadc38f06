"""Host reference of the residual-weighted selection (csrc/dpn_adaptive.hip) in numpy fp64.

`select_reference` restates what dpn_adaptive_select defines -- weights, inclusive prefix sum, inverse-CDF draw -- from the kernel's own scores and
uniforms, so it needs no Philox of its own.  The GPU tests hold the kernel to it; a user who wants the selection probabilities of a pool gets them from
`probabilities`.  Nothing here runs in training.
"""
import numpy as np


def weights(scores, k=1.0, c=1.0):
    """w_i = s_i ** k / mean(s ** k) + c in fp64; all 1 when the mean is 0 (or not finite).  A score that is negative or not finite counts as 0."""
    k, c = float(k), float(c)
    if not (np.isfinite(k) and np.isfinite(c) and k >= 0.0 and c >= 0.0):
        raise ValueError('k and c must be finite and >= 0, got k = %r, c = %r' % (k, c))
    s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    if s.size == 0:
        raise ValueError('no candidates')
    s = np.where(np.isfinite(s) & (s > 0.0), s, 0.0)
    with np.errstate(over='ignore'):
        p = np.ones_like(s) if k == 0.0 else s ** k                 # (0 ** 0 = 1 on both sides)
        mean = p.sum() / s.size
    if not (mean > 0.0 and np.isfinite(mean)):
        return np.ones_like(s)
    return p / mean + c


def probabilities(scores, k=1.0, c=1.0):
    """p_i = w_i / sum(w): the probability that one draw picks candidate i."""
    w = weights(scores, k, c)
    return w / w.sum()


def select_reference(scores, u, k=1.0, c=1.0):
    """-> idx [n] (int64), w [m], cdf [m]: cdf = np.cumsum(w) (sequential, fp64), idx_j = the smallest i with cdf[i] > u_j * cdf[-1]; a product that
    rounds up to the total is taken as the last double below it, so the answer always exists and always has w > 0."""
    w = weights(scores, k, c)
    cdf = np.cumsum(w)
    total = cdf[-1]
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    if u.size and not (np.all(u >= 0.0) and np.all(u < 1.0)):
        raise ValueError('u must lie in [0, 1)')
    target = u * total
    target = np.where(target < total, target, np.nextafter(total, 0.0))
    idx = np.searchsorted(cdf, target, side='right')
    return idx.astype(np.int64), w, cdf
