"""Host restatement of the lead-batch step's finish kernel (csrc/dpn_residual.hip: dpn_step_finish_batch) and of the size of dpn_step_residual's
block rows: the GPU tests hold the kernel's 16 values per field to finish_reference bit for bit.  numpy only, no GPU."""
import numpy as np

from ._lib import STEP_LOSSES as LOSSES            # one field's row of dpn_step_finish_batch (include/dpn_hip.h)


def blocks(n):
    """Workgroups of 256 points that hold n points."""
    return (int(n) + 255) // 256


def rows_doubles(n_inter, n):
    """dpn_step_rows_doubles: 7 doubles per block of the interior and of the margin group; 0 for a split the entry points refuse."""
    n_inter, n = int(n_inter), int(n)
    if n_inter < 1 or n_inter >= n:
        return 0
    return 7 * (blocks(n_inter) + blocks(n - n_inter))


def _lane_tree_sum(col):
    """dpn_residual_finish_kernel's order in fp64: lane l adds rows l, l + 64, ... in order, then the xor shuffle tree (32, 16, ..., 1)."""
    lanes = np.zeros(64, dtype=np.float64)
    for b, v in enumerate(np.asarray(col, dtype=np.float64)):
        lanes[b % 64] = lanes[b % 64] + v
    o = 32
    while o > 0:
        lanes = lanes + lanes[np.arange(64) ^ o]
        o >>= 1
    return lanes[0]


def finish_reference(rows, n_inter, n, factors, margin_factor, reduce_sum=False):
    """dpn_step_finish_batch for one field: rows [blocks(n_inter) + blocks(n - n_inter), 7] fp64 -> [16] fp32:
    [0:6] interior terms, [6] their total, [7:13] margin terms, [13] their total, [14] the data loss, [15] (data + interior) + margin.
    A term is float32(float64(float32(S or S / n_group)) * float64(factor)); a group's total adds its terms in the reference's order u, v, energy,
    continuity, vapour, gas (indices 0, 1, 3, 2, 4, 5); the data loss is float32(S6 / (6 n_m)) * float32(margin_factor); all totals in fp32."""
    rows = np.asarray(rows, dtype=np.float64)
    n_inter, n = int(n_inter), int(n)
    n_m = n - n_inter
    nb_i = blocks(n_inter)
    if rows_doubles(n_inter, n) == 0 or rows.shape != (nb_i + blocks(n_m), 7):
        raise ValueError('finish_reference: rows %s for n_inter = %d of n = %d points' % (rows.shape, n_inter, n))
    out = np.zeros(LOSSES, dtype=np.float32)
    for g, (part, m) in enumerate(((rows[:nb_i], n_inter), (rows[nb_i:], n_m))):
        t = np.zeros(6, dtype=np.float32)
        for e in range(6):
            s = _lane_tree_sum(part[:, e])
            t[e] = np.float32(np.float64(np.float32(s if reduce_sum else s / np.float64(m))) * np.float64(np.float32(factors[e])))
        out[7 * g:7 * g + 6] = t
        out[7 * g + 6] = ((((t[0] + t[1]) + t[3]) + t[2]) + t[4]) + t[5]
    out[14] = np.float32(_lane_tree_sum(rows[nb_i:, 6]) / (6.0 * np.float64(n_m))) * np.float32(margin_factor)
    out[15] = (out[14] + out[6]) + out[13]
    return out
