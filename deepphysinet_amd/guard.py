"""The step guard of the fused clip + Adam step, restated on the host (numpy only, no GPU): skip the update when the gradient norm is non-finite
or a spike.

The rule runs on the device, in one thread of dpn_clip_adam_flat_guard's reduction launch (csrc/dpn_optim.hip, dpn_gradnorm_reduce_guard_kernel;
the contract is the comment of include/dpn_hip.h), because the step is replayed from a hipGraph and the host never sees a norm in time.
`guard_reference` is that thread's arithmetic operation for operation -- the pattern of balance.update_reference and lead_step.finish_reference --
and `StepGuard` the option with the C ABI's own argument rules, which FusedClipAdam and the training loops build from.

Input of every call: the fp32 total norm exactly as dpn_adam_kernel forms it, (float)sqrt(sumsq) * grad_scale.  fp64 from there, every operation
rounded once:
    not (|total| <= FLT_MAX)                       verdict 1 (non-finite): skipped_nonfinite += 1, consecutive = 0
    else factor > 0 and seen >= warmup and total > factor * running and consecutive < patience
                                                   verdict 2 (spike):      skipped_spike += 1, consecutive += 1
    else                                           verdict 0 (applied):    consecutive == patience (overruled: the level of the norms has moved
                                                   for good, e.g. the PDE losses switching on): seen = 0 first; then
                                                   running = total if seen == 0 else decay * running + (1 - decay) * total; seen += 1; consecutive = 0
    last = total in every case; running and seen move on verdict 0 only.
The step number of an applied update is t = calls - skipped_nonfinite - skipped_spike.

What the guard does not see: a loss that is non-finite while all gradients are finite.  A finite gradient whose square overflows the fp32
per-thread partial (|g| above about 1.8e19) gives an infinite total and is skipped as non-finite.
"""
import math

import numpy as np

FIELDS = ('skipped_nonfinite', 'skipped_spike', 'verdict', 'seen', 'consecutive', 'reserved', 'running', 'last')
INT_FIELDS = FIELDS[:6]
APPLIED, NONFINITE, SPIKE = 0, 1, 2
FLT_MAX = np.float32(3.4028234663852886e38)
INT32_MAX = 2 ** 31 - 1
MISTAKES = ('running_on_skip', 'patience_off_by_one', 't_not_reduced', 'inf_passes', 'warmup_off_by_one', 'no_restart')


def zero_state():
    """DpnStepGuard as the caller hands it over: all zero."""
    return dict(skipped_nonfinite=0, skipped_spike=0, verdict=0, seen=0, consecutive=0, reserved=0, running=np.float64(0.0), last=np.float64(0.0))


class StepGuard:
    """The option: skip_nonfinite alone (spike_factor None or 0: the spike rule is off), or the spike rule on top of it (a spike_factor implies
    the non-finite rule).  The arguments are checked with dpn_clip_adam_flat_guard's own rules: spike_factor finite and >= 0, spike_decay in
    [0, 1), spike_warmup >= 1, spike_patience >= 1."""

    KEYS = ('spike_factor', 'spike_decay', 'spike_warmup', 'spike_patience')

    def __init__(self, spike_factor=None, spike_decay=0.99, spike_warmup=100, spike_patience=5):
        factor = 0.0 if spike_factor is None else float(spike_factor)
        decay = float(spike_decay)
        if not (math.isfinite(factor) and factor >= 0.0):
            raise ValueError('step guard: spike_factor must be a finite number >= 0 (0 or None: no spike rule), got %r' % (spike_factor,))
        if not (0.0 <= decay < 1.0):
            raise ValueError('step guard: spike_decay must lie in [0, 1), got %r' % (spike_decay,))
        for name, v in (('spike_warmup', spike_warmup), ('spike_patience', spike_patience)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1 or int(v) > INT32_MAX:
                raise ValueError('step guard: %s must be an integer >= 1, got %r' % (name, v))
        self.spike_factor, self.spike_decay = factor, decay
        self.spike_warmup, self.spike_patience = int(spike_warmup), int(spike_patience)

    @classmethod
    def from_option(cls, opt):
        """None / False -> None; True -> the non-finite rule alone; a StepGuard passes through; a dict of KEYS -> StepGuard(**dict)."""
        if opt is None or opt is False:
            return None
        if isinstance(opt, cls):
            return opt
        if opt is True:
            return cls()
        unknown = set(opt) - set(cls.KEYS)
        if unknown:
            raise ValueError('step_guard: unknown keys %s (known: %s)' % (sorted(unknown), ', '.join(cls.KEYS)))
        return cls(**opt)

    def as_dict(self):
        return dict(spike_factor=self.spike_factor, spike_decay=self.spike_decay, spike_warmup=self.spike_warmup, spike_patience=self.spike_patience)

    def __eq__(self, other):
        return isinstance(other, StepGuard) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return 'StepGuard(%s)' % ', '.join('%s=%r' % kv for kv in self.as_dict().items())


def guard_step(state, total, spike_factor, decay, warmup, patience, mistake=None):
    """One call: (verdict, new state).  `total`: the fp32 total norm.  `mistake`: one of MISTAKES, for the tests of the case table."""
    assert mistake is None or mistake in MISTAKES
    total = np.float32(total)
    tot = np.float64(total)
    factor, decay = np.float64(spike_factor), np.float64(decay)
    st = dict(state)
    seen, consecutive, running = int(st['seen']), int(st['consecutive']), np.float64(st['running'])
    with np.errstate(all='ignore'):
        if mistake == 'inf_passes':
            nonfinite = bool(np.isnan(total))
        else:
            nonfinite = not bool(np.abs(total) <= FLT_MAX)
        patience_cmp = patience + 1 if mistake == 'patience_off_by_one' else patience
        warm = warmup + 1 if mistake == 'warmup_off_by_one' else warmup
        if nonfinite:
            verdict = NONFINITE
            st['skipped_nonfinite'] += 1
            consecutive = 0
        elif factor > 0.0 and seen >= warm and bool(tot > factor * running) and consecutive < patience_cmp:
            verdict = SPIKE
            st['skipped_spike'] += 1
            consecutive += 1
        else:
            verdict = APPLIED
            if consecutive == patience_cmp and mistake != 'no_restart':
                seen = 0
        if verdict == APPLIED or mistake == 'running_on_skip':
            if seen == 0:
                running = tot
            else:
                a = decay * running                     # three roundings and the sum: no fused multiply-add
                b = np.float64(1.0) - decay
                c = b * tot
                running = a + c
            if verdict == APPLIED:
                if seen < INT32_MAX:
                    seen += 1
                consecutive = 0
    st.update(verdict=verdict, seen=seen, consecutive=consecutive, running=np.float64(running), last=tot)
    return verdict, st


def effective_step(calls, state, mistake=None):
    """The step number t an applied update uses after `calls` calls: the calls that were not skipped."""
    if mistake == 't_not_reduced':
        return int(calls)
    return int(calls) - int(state['skipped_nonfinite']) - int(state['skipped_spike'])


def guard_reference(totals, spike_factor, decay, warmup, patience, state=None, mistake=None):
    """The verdict of each call and the struct after each call: ([verdict], [state dict]) for the sequence `totals` of fp32 total norms, from
    `state` (None: zeros).  spike_factor None counts as 0 (the spike rule off)."""
    st = zero_state() if state is None else dict(state)
    verdicts, states = [], []
    for total in totals:
        v, st = guard_step(st, total, 0.0 if spike_factor is None else spike_factor, decay, warmup, patience, mistake)
        verdicts.append(v)
        states.append(dict(st))
    return verdicts, states


def state_equal(a, b):
    """Field for field, `running` and `last` by their fp64 bits (NaN equals NaN of the same bits)."""
    ints = all(int(a[k]) == int(b[k]) for k in INT_FIELDS)
    bits = lambda x: np.float64(x).view(np.uint64)
    return ints and all(bits(a[k]) == bits(b[k]) for k in ('running', 'last'))
