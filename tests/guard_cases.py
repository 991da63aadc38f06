"""Case table of the step guard (dpn_clip_adam_flat_guard; kernel dpn_gradnorm_reduce_guard_kernel; host restatement deepphysinet_amd/guard.py).
Imports without a GPU: tests/test_guard_cases_cpu.py runs the table through guard.guard_reference, tests/test_gpu_step_guard.py runs the scripted
sequence and the tensor lists through the C ABI.

SEQUENCES are written by hand from the rule in include/dpn_hip.h, with spike_decay = 0.5 and small binary numbers so that every running mean below
is exact and can be checked on paper:
    want['verdict'], and per call the struct's fields after it; want['t'] the step number calls - skips an applied update would use.
"""
from dataclasses import dataclass

import numpy as np

NAN, INF = float('nan'), float('inf')


@dataclass(frozen=True)
class Sequence:
    name: str
    factor: float
    decay: float
    warmup: int
    patience: int
    totals: tuple
    want: dict


SEQUENCES = (
    # the warm-up boundary: call 3 (20 > 10 * 1) comes with seen = 2 < 3 and is applied; call 5 (100 > 10 * 5.75) is a spike; one spike below the
    # patience does not restart the mean
    Sequence('warmup_boundary', 10.0, 0.5, 3, 2, (1.0, 1.0, 20.0, 1.0, 100.0, 1.0), dict(
        verdict=[0, 0, 0, 0, 2, 0], running=[1.0, 1.0, 10.5, 5.75, 5.75, 3.375], seen=[1, 2, 3, 4, 4, 5], consecutive=[0, 0, 0, 0, 1, 0],
        skipped_nonfinite=[0] * 6, skipped_spike=[0, 0, 0, 0, 1, 1], t=[1, 2, 3, 4, 4, 5])),
    # ... and the first call AT the boundary (seen == warmup) is tested
    Sequence('warmup_exact', 10.0, 0.5, 3, 2, (1.0, 1.0, 1.0, 20.0, 10.0), dict(
        verdict=[0, 0, 0, 2, 0], running=[1.0, 1.0, 1.0, 1.0, 5.5], seen=[1, 2, 3, 3, 4], consecutive=[0, 0, 0, 1, 0],
        skipped_nonfinite=[0] * 5, skipped_spike=[0, 0, 0, 1, 1], t=[1, 2, 3, 3, 4])),
    # patience reached: two spikes in a row, the third call of that level overrules the guard and the mean starts again from it
    Sequence('patience_restart', 10.0, 0.5, 1, 2, (1.0, 50.0, 50.0, 50.0, 1.0, 600.0), dict(
        verdict=[0, 2, 2, 0, 0, 2], running=[1.0, 1.0, 1.0, 50.0, 25.5, 25.5], seen=[1, 1, 1, 1, 2, 2], consecutive=[0, 1, 2, 0, 0, 1],
        skipped_nonfinite=[0] * 6, skipped_spike=[0, 1, 2, 2, 2, 3], t=[1, 1, 1, 2, 3, 3])),
    # NaN, +inf and -inf; a non-finite call between spikes sets `consecutive` back
    Sequence('nonfinite', 10.0, 0.5, 1, 2, (2.0, NAN, INF, -INF, 2.0, 50.0, NAN, 50.0, 50.0, 50.0), dict(
        verdict=[0, 1, 1, 1, 0, 2, 1, 2, 2, 0], running=[2.0] * 9 + [50.0], seen=[1, 1, 1, 1, 2, 2, 2, 2, 2, 1],
        consecutive=[0, 0, 0, 0, 0, 1, 0, 1, 2, 0], skipped_nonfinite=[0, 1, 2, 3, 3, 3, 4, 4, 4, 4], skipped_spike=[0, 0, 0, 0, 0, 1, 1, 2, 3, 3],
        t=[1, 1, 1, 1, 2, 2, 2, 2, 2, 3])),
    # spike_factor = 0: the spike rule is off, the mean still runs, the non-finite rule still holds
    Sequence('factor_zero', 0.0, 0.5, 1, 2, (1.0, 1e6, NAN, 0.25), dict(
        verdict=[0, 0, 1, 0], running=[1.0, 500000.5, 500000.5, 250000.375], seen=[1, 2, 2, 3], consecutive=[0, 0, 0, 0],
        skipped_nonfinite=[0, 0, 1, 1], skipped_spike=[0] * 4, t=[1, 2, 2, 3])),
)
SEQUENCE_IDS = [s.name for s in SEQUENCES]

# which sequence shows which seeded mistake of guard.guard_reference (every mistake at least once)
CAUGHT_BY = {'running_on_skip': 'patience_restart', 'patience_off_by_one': 'patience_restart', 't_not_reduced': 'patience_restart',
             'inf_passes': 'nonfinite', 'warmup_off_by_one': 'warmup_exact', 'no_restart': 'patience_restart'}


def sequence_by_name(name):
    return next(s for s in SEQUENCES if s.name == name)


def mismatches(seq, verdicts, states, ts):
    """The (call, field, got, want) entries in which a run of `seq` differs from the hand-written table; [] = agreement."""
    out = []
    for i, total in enumerate(seq.totals):
        if verdicts[i] != seq.want['verdict'][i] or states[i]['verdict'] != seq.want['verdict'][i]:
            out.append((i, 'verdict', verdicts[i], seq.want['verdict'][i]))
        for k in ('seen', 'consecutive', 'skipped_nonfinite', 'skipped_spike'):
            if int(states[i][k]) != seq.want[k][i]:
                out.append((i, k, int(states[i][k]), seq.want[k][i]))
        if np.float64(states[i]['running']).view(np.uint64) != np.float64(seq.want['running'][i]).view(np.uint64):
            out.append((i, 'running', float(states[i]['running']), seq.want['running'][i]))
        last, want_last = np.float64(states[i]['last']), np.float64(np.float32(total))
        if not (last == want_last or (np.isnan(last) and np.isnan(want_last))):
            out.append((i, 'last', float(last), float(want_last)))
        if ts[i] != seq.want['t'][i]:
            out.append((i, 't', ts[i], seq.want['t'][i]))
        if int(states[i]['reserved']) != 0:
            out.append((i, 'reserved', int(states[i]['reserved']), 0))
    return out


# ---------------------------------------------------------------------------------------------- the GPU test's scripted sequence and tensor lists
SCRIPT_SCALES = (1, 1, 1, 1, 50, 1, 50, 50, 50, 1)                  # gradient scale of call k
SCRIPT = dict(spike_factor=10.0, spike_decay=0.99, spike_warmup=3, spike_patience=2)
# with norms n, n, n, n, 50n, n, 50n, 50n, 50n, n: call 5 is a spike; call 6 applied; calls 7 and 8 spikes (patience 2); call 9 overrules; call 10 applied
SCRIPT_VERDICTS = (0, 0, 0, 0, 2, 0, 2, 2, 0, 0)

# the smallest tensor lists at which the update can go wrong: 1, the scalar tail (3), the chunk edges, more than one chunk
NUMELS_SMALL = (1, 3, 2047, 2048, 2049, 4100)
NUMELS_161 = (1,) * 161                                            # two update launches under one verdict
FINITE_OVERFLOW = 3e19                                             # its square overflows the fp32 partial: an infinite total
