"""Loss balancing by gradient norms (csrc/dpn_balance.hip): the option's value type and the host references in numpy
fp64.

One training step minimises margin_loss + inter_pde_loss + margin_pde_loss, the six equations inside each PDE loss summed under the hand-set
loss_factor table.  With the option every term k carries a weight lambda_k that is refreshed every `every` steps from the norms of the terms'
parameter gradients, n_k = |grad_theta L_k| (Wang, Teng & Perdikaris 2021, "Understanding and mitigating gradient flow pathologies in
physics-informed neural networks": learning-rate annealing; Wang, Sankaran, Wang & Perdikaris 2023, "An expert's guide to training
physics-informed neural networks": grad-norm weighting).  `LossBalance` carries the option through InterfacePhysics.training_step and the loops;
`sumsq_reference` and `update_reference` restate what dpn_balance_sumsq and dpn_balance_update define, and the GPU tests hold the kernels to them.
Nothing here runs in training.
"""
from dataclasses import dataclass

import numpy as np

MAX_TERMS = 16          # DPN_BALANCE_MAX_TERMS (include/dpn_hip.h)
STEP_TERMS = 13         # DPN_BALANCE_STEP_TERMS: interior terms [6] | margin terms [6] | data
EQUATIONS = ('motion_u', 'motion_v', 'continuous', 'energy', 'vapor', 'gas')
GROUPS = {'equations': ('data',) + EQUATIONS, 'parts': ('data', 'inter', 'margin')}


@dataclass(frozen=True)
class LossBalance:
    """every: the weights are refreshed on every every-th step, counted from the first (an integer >= 1).  momentum in [0, 1]: the share of the old
    lambda in the moving average (0: the new target at once; 1: lambda never moves).  groups: the terms that are balanced against each other --
    'equations', K = 7: [data, motion_u, motion_v, continuous, energy, vapor, gas], equation e the interior term e plus the margin term e;
    'parts', K = 3: [data, interior total, margin total], the three entries of the step's `parts`.  lam_min, lam_max: the clamp of a refresh's
    target, 0 < lam_min <= 1 <= lam_max, both finite."""
    every: int = 100
    momentum: float = 0.9
    groups: str = 'equations'
    lam_min: float = 1e-3
    lam_max: float = 1e3

    def __post_init__(self):
        if isinstance(self.every, bool) or not isinstance(self.every, (int, np.integer)) or int(self.every) < 1:
            raise ValueError('LossBalance: every must be an integer >= 1, got %r' % (self.every,))
        momentum = float(self.momentum)
        if not 0.0 <= momentum <= 1.0:
            raise ValueError('LossBalance: momentum must lie in [0, 1], got %r' % (self.momentum,))
        if self.groups not in GROUPS:
            raise ValueError('LossBalance: groups must be one of %s, got %r' % (sorted(GROUPS), self.groups))
        lo, hi = float(self.lam_min), float(self.lam_max)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= 1.0 <= hi):
            raise ValueError('LossBalance: need finite 0 < lam_min <= 1 <= lam_max, got %r, %r' % (self.lam_min, self.lam_max))
        object.__setattr__(self, 'every', int(self.every))
        object.__setattr__(self, 'momentum', momentum)
        object.__setattr__(self, 'lam_min', lo)
        object.__setattr__(self, 'lam_max', hi)

    @property
    def names(self):
        """The K terms' names, k ascending."""
        return GROUPS[self.groups]

    @property
    def n_terms(self):
        return len(GROUPS[self.groups])

    def term_map(self):
        """k of each of the 13 terms of a step in dpn_balance_combine's order: interior terms [6], margin terms [6], data."""
        return group_map(self.groups)


def group_map(groups):
    """-> 13 ints: the k of interior term 0..5, margin term 0..5, the data loss."""
    if groups == 'equations':
        return tuple(range(1, 7)) + tuple(range(1, 7)) + (0,)
    if groups == 'parts':
        return (1,) * 6 + (2,) * 6 + (0,)
    raise ValueError('groups must be one of %s, got %r' % (sorted(GROUPS), groups))


def sumsq_reference(arrays):
    """The sum of x * x over every element of every array (fp32 values; None counts as zeros) in fp64, added sequentially in the order given: what
    dpn_balance_sumsq forms in another (fixed) order.  A product of two fp32 values is exact in fp64, so every rounding is one of the additions."""
    tot = np.float64(0.0)
    for a in arrays:
        if a is None:
            continue
        v = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).astype(np.float64)
        for s in v * v:                                     # sequential
            tot = tot + s
    return float(tot)


def update_reference(sumsq, lam, momentum, lam_min, lam_max, with_diag=False):
    """-> (lam_new [K] fp32, flag), and with_diag the diag row [3 K + 2] of dpn_balance_update (n | lambda-hat | new lambda | mean | flag).

    n_k = sqrt(sumsq_k); term k is active when n_k is finite and > 0.  Fewer than two active terms, or a sumsq_k that is not finite: lam is returned
    unchanged and flag = 1.  Otherwise mean = (sum of n_k over the active k, k ascending) / (the number of active terms),
    lambda-hat_k = clamp(mean / n_k, lam_min, lam_max) and lambda_k <- momentum * lambda_k + (1 - momentum) * lambda-hat_k in fp64 from the fp32
    lambda_k, rounded once to fp32; an inactive term keeps its lambda.

    This is the MEAN form, not the sum form: lambda = 1 when all norms are equal, so the learning rate keeps its meaning when the option is switched
    on.  The papers' sum form (lambda-hat_k = sum_j n_j / n_k) is K times this."""
    s = np.ascontiguousarray(sumsq, dtype=np.float64).reshape(-1)
    lam32 = np.ascontiguousarray(lam, dtype=np.float32).reshape(-1)
    K = s.size
    momentum, lam_min, lam_max = float(momentum), float(lam_min), float(lam_max)
    if not (1 <= K <= MAX_TERMS and lam32.size == K):
        raise ValueError('update_reference: need 1 <= K <= %d sums and as many lambdas, got %d, %d' % (MAX_TERMS, K, lam32.size))
    if not (0.0 <= momentum <= 1.0 and np.isfinite(lam_min) and np.isfinite(lam_max) and 0.0 < lam_min <= 1.0 <= lam_max):
        raise ValueError('update_reference: need momentum in [0, 1] and finite 0 < lam_min <= 1 <= lam_max, got %r, %r, %r' % (momentum, lam_min, lam_max))
    with np.errstate(invalid='ignore', over='ignore'):
        n = np.sqrt(s)
    active = np.isfinite(n) & (n > 0.0)
    flag = int(not np.isfinite(s).all() or int(active.sum()) < 2)
    new, hat, mean = lam32.copy(), np.zeros(K), 0.0
    if not flag:
        tot = 0.0
        for k in range(K):
            if active[k]:
                tot = tot + float(n[k])
        mean = tot / float(active.sum())
        for k in range(K):
            if active[k]:
                with np.errstate(over='ignore'):
                    hat[k] = min(max(mean / float(n[k]), lam_min), lam_max)
                new[k] = np.float32(momentum * float(lam32[k]) + (1.0 - momentum) * hat[k])
    if not with_diag:
        return new, flag
    return new, flag, np.concatenate([n, hat, new.astype(np.float64), [mean, float(flag)]])
