"""Case table, fp64 reference, bound and fp32 model for the weight EMA that dpn_clip_adam_flat_ema moves inside the Adam update launch
(dpn_adam_kernel<AdamFlat<true, false, false>>), and the inputs of dpn_ema_swap.  Imports without a GPU: tests/test_ema_cases_cpu.py runs the table through
the numpy fp32 model below, tests/test_gpu_ema.py through the C ABI.  The Adam side (inputs, placements, hyper-parameters, arenas) is
tests/optim_cases.py's; only what the shadow adds is here.

The definition (all fp32, one rounding per operation, one fma; p' is the fp32 parameter value the launch has just stored; decay = hyper[7]):
    t = *step after the bump                 te = t + base (base = *ema_base_dev, 0 when the pointer is null)
    d  = warmup ? fminf(decay, (1 + te) / (10 + te)) : decay
    s' = fmaf(d, s, (1 - d) * p')
The reference is this recursion in fp64 applied to the kernel's OWN fp32 p' (so that the Adam bounds of optim_cases.py do not enter), with the
fp32 value of the decay as an exact number.

Bound on |s - s'|, from the operation count (u = 2^-24), not measured.  Write A = d |s0| + (1 - d) |p'|.
  * Without warm-up d is the exact decay.  Three roundings follow -- 1 - d, the product with p', the fma -- each a relative error of at most u on a
    quantity whose magnitude is at most A (times the factors already collected): (1 + u)^3 - 1 <= c3 := 3u + 4u^2, so the error is at most c3 A.
  * With warm-up, three more operations form d (1 + te, 10 + te, the quotient; fminf selects and is 1-Lipschitz), so the kernel's d is off by at
    most c3 d.  A changed d moves the exact result by |delta d| |s0 - p'| <= c3 d (|s0| + |p'|), and the three roundings above then act on
    quantities at most (1 + c3) times as large.
  * A product that underflows loses at most the smallest normal number, whether denormals are flushed or kept: + 2^-126.
    bound = c3 A + w c3 (1 + c3) d (|s0| + |p'|) + 2^-126            w = 1 with warm-up, else 0
Decay 0 gives d = 0 exactly on either route ((1 + te) / (10 + te) > 0), 1 - d = 1 and s' = fma(0, s, p') = p' bit for bit (finite s).
tests/test_ema_cases_cpu.py records how much of the bound a plain numpy fp32 evaluation uses.

Optimiser level (several steps on one state): each step is held to the one-step bound against the fp64 recursion started from the kernel's own
previous shadow; against the fp64 recursion carried over k steps the error of step j is damped by the later decays, so the sum of
prod(d_i, i > j) * bound_j bounds it (`propagated_bound`).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import optim_cases as O
from optim_cases import CHUNK, F32, FLAT_TABLE, GUARD, HYPER, NUMEL_EDGES, SENTINEL, U, long_list  # noqa: F401  (the Adam side's, not copied)

STEPS = (1, 2, 10, 1000)
BASES = (0, 5)
WARMUPS = (True, False)
DECAYS = (0.0, 0.9, 0.9999)
PLACES = ('aligned', 'shifted', 'mixed')
LISTS = (160, 161, 321)
C3 = 3 * U + 4 * U * U
TINY = 2.0 ** -126
COMBOS = [(t, b, w, d) for d in DECAYS for w in WARMUPS for b in BASES for t in STEPS]        # 48


@dataclass(frozen=True)
class Case:
    name: str
    numels: tuple
    place: str
    t: int
    base: int
    warmup: bool
    decay: float
    hyper: str = 'shipped'
    sshift: int = 0           # floats the whole shadow buffer is off a 16-byte boundary (the fifth role; 'shifted': 1 .. 3, 'mixed': see shifts_of)

    @property
    def adam(self):
        """The optim_cases.Case that builds p, g, m, v and places p and g ('dev' form)."""
        return O.Case(self.name, 'W', self.hyper, self.t, self.numels, place=self.place)


def _cases():
    c, k = [], 0
    hy = ('shipped', 'test_active')
    sizes = [('single_%d' % n, (n,)) for n in NUMEL_EDGES] + [('list%d' % n, long_list(n, FLAT_TABLE)) for n in LISTS]
    for label, numels in sizes:
        for place in PLACES:
            t, b, w, d = COMBOS[k % len(COMBOS)]
            # the fifth role: 'shifted' moves the shadow too; 'mixed' alternates between p or g alone off (shadow on 16 bytes) and, every second
            # case, the shadow ALONE off (p and g of every tensor on 16 bytes: shifts_of)
            sshift = {'aligned': 0, 'shifted': 1 + k % 3, 'mixed': (0, 2)[(k // 3) % 2]}[place]
            c.append(Case('%s_%s' % (label, place), numels, place, t, b, w, d, hy[k % 2], sshift))
            k += 1
    # every combination of step, base, warm-up and decay on one list past a table boundary
    for i, (t, b, w, d) in enumerate(COMBOS):
        c.append(Case('combo_t%d_b%d_%s_d%g' % (t, b, 'warm' if w else 'flat', d), long_list(161, FLAT_TABLE), 'aligned', t, b, w, d, hy[i % 2]))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def shifts_of(case):
    """Per tensor (p, g, 0, 0) as optim_cases.shifts_of gives them for the _dev form -- except 'mixed' with a shifted shadow: there the shadow is
    the one role off, p and g stay on 16 bytes -- and the shadow buffer's shift."""
    if case.place == 'mixed' and case.sshift:
        return [(0, 0, 0, 0)] * len(case.numels), case.sshift
    return O.shifts_of(case.adam, 'dev'), case.sshift


def path_of(case):
    """'vector' where p, g and the shadow are all on 16 bytes (m and v always are in the flat forms)."""
    sh, ss = shifts_of(case)
    return ['vector' if not (s[0] or s[1] or ss) else 'scalar' for s in sh]


@lru_cache(maxsize=None)
def built(name):
    """(optim_cases.Inputs, shadow before the step as a list of fp32 arrays): computed once, shared, never written to."""
    case = case_by_name(name)
    inp = O.build(case.adam)
    rng = np.random.default_rng([11, sum(map(ord, name)), len(case.numels)])
    s0 = [(p * (1.0 + 0.1 * rng.standard_normal(len(p))) + 1e-3 * rng.standard_normal(len(p))).astype(F32) for p in inp.p]
    return inp, s0


# ---------------------------------------------------------------------------------------------- fp64 reference and bound
def decay64(decay, t, base, warmup):
    d = O.f32(decay)
    te = t + base
    return min(d, (1.0 + te) / (10.0 + te)) if warmup else d


def reference(s0, p_new, decay, t, base, warmup):
    """The recursion in fp64: lists of fp64 arrays."""
    d = decay64(decay, t, base, warmup)
    return [d * s.astype(np.float64) + (1.0 - d) * p.astype(np.float64) for s, p in zip(s0, p_new)]


def bound(s0, p_new, decay, t, base, warmup):
    """The one-step bound of the module docstring, elementwise: a list of fp64 arrays."""
    d = decay64(decay, t, base, warmup)
    out = []
    for s, p in zip(s0, p_new):
        s, p = np.abs(s.astype(np.float64)), np.abs(p.astype(np.float64))
        out.append(C3 * (d * s + (1.0 - d) * p) + (C3 * (1.0 + C3) * d * (s + p) if warmup else 0.0) + TINY)
    return out


def ratio(got, ref, bnd):
    """Largest |got - ref| / bound over the lists."""
    return max(O._ratio(np.abs(np.asarray(g, np.float64) - r), b) for g, r, b in zip(got, ref, bnd))


def propagated_bound(bounds, decays):
    """Bound after k steps against the fp64 recursion carried over all of them: bounds[j] (the one-step bound of step j, lists of arrays) damped
    by the decays of the later steps."""
    k = len(bounds)
    out = [np.zeros_like(b) for b in bounds[0]]
    for j in range(k):
        damp = float(np.prod(decays[j + 1:])) if j + 1 < k else 1.0
        out = [o + damp * b for o, b in zip(out, bounds[j])]
    return out


# ---------------------------------------------------------------------------------------------- fp32 model, with seeded mistakes
MISTAKES = ('decay_swapped', 'p_before_update', 'warmup_t_minus_1', 'base_ignored')


def model_fp32(s0, p_old, p_new, decay, t, base, warmup, mistake=None):
    """A plain numpy.float32 evaluation of the definition: no fused multiply-add (one rounding more than the kernel).  p_old: the parameters
    before the step, used by a mistake only."""
    assert mistake is None or mistake in MISTAKES
    one, dec = F32(1), F32(decay)
    te = t + (0 if mistake == 'base_ignored' else base) - (1 if mistake == 'warmup_t_minus_1' else 0)
    d = min(dec, (one + F32(te)) / (F32(10) + F32(te))) if warmup else dec
    assert isinstance(d, np.float32)
    a, b = (d, one - d) if mistake != 'decay_swapped' else (one - d, d)
    src = p_old if mistake == 'p_before_update' else p_new
    out = [a * s + b * p for s, p in zip(s0, src)]
    assert all(x.dtype == F32 for x in out)
    return out
