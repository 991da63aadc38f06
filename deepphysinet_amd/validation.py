"""Host side of the validation pass that needs no device: the sufficient statistics of the per-variable errors and how they are merged and
turned into metrics, and the two log lines of the reference's training loop (interface/interface_physics.py:609-618, :720-733).

A statistics row is an fp64 vector of ROW entries:
    [0]      sum SmoothL1_beta(out_n - label) over the 6 n elements          [1:7]   sum d^2      [7:13]  sum |d|
    [13:19]  sum d                                                           [19:25] max |d|      (d in physical units, per variable)
    [25]     margin points n          [26] samples          [27:31] sums over the samples of valid_loss, margin_loss, inter_pde_loss, margin_pde_loss
The first 25 entries are what the kernel writes (include/dpn_hip.h: dpn_label_errors).  Rows are merged entry by entry -- sums and counts added,
maxima maximised --, never by averaging metrics: the pooled RMSE of two shards is sqrt((S1 + S2) / (n1 + n2)), not the mean of their RMSEs.
"""
import json
import math
import os
import time

import torch

VARIABLES = ('u', 'v', 'p', 'T', 'q', 'rio')          # the reference's names of the six outputs (margin_<v>_loss, :518-530)
LOSS_KEYS = ('valid_loss', 'margin_loss', 'inter_pde_loss', 'margin_pde_loss')
KERNEL_STATS = 25
ROW = 31
_MAX = slice(19, 25)


def stats_row(kernel_stats, n_points, losses=None):
    """One sample's row from the kernel's 25 statistics, its number of margin points and its losses {key: value} (missing keys count 0)."""
    row = torch.zeros(ROW, dtype=torch.float64)
    row[:KERNEL_STATS] = torch.as_tensor(kernel_stats, dtype=torch.float64).reshape(-1).cpu()
    row[25], row[26] = float(n_points), 1.0
    for i, k in enumerate(LOSS_KEYS):
        if losses and k in losses:
            row[27 + i] = float(losses[k])
    return row


def merge_stats(rows):
    """The row of the union of the shards / samples whose rows are given ([R, ROW] or a sequence of [ROW]); added in the order given."""
    if not torch.is_tensor(rows):
        rows = list(rows)
        if not rows:
            raise ValueError('merge_stats: no rows')
        rows = torch.stack([torch.as_tensor(r, dtype=torch.float64).reshape(ROW) for r in rows])
    rows = rows.reshape(-1, ROW).double()
    if rows.shape[0] == 0:
        raise ValueError('merge_stats: no rows')
    out = rows[0].clone()
    for r in rows[1:]:
        mx = torch.maximum(out[_MAX], r[_MAX])
        out += r
        out[_MAX] = mx
    return out


def metrics_from_stats(row):
    """{variables: {v: {mse, rmse, mae, bias, max_abs}}, data_loss (unscaled SmoothL1 mean), n_points, n_samples, and the mean of every loss over
    the samples} of a (merged) row.  `mse` is the reference's margin_<v>_loss (nn.MSELoss on the de-normalised values)."""
    row = torch.as_tensor(row, dtype=torch.float64).reshape(ROW)
    n, m = float(row[25]), float(row[26])
    if n <= 0:
        raise ValueError('metrics_from_stats: a row without points')
    out = {'variables': {}, 'data_loss': float(row[0]) / (6.0 * n), 'n_points': int(n), 'n_samples': int(m)}
    for k, v in enumerate(VARIABLES):
        mse = float(row[1 + k]) / n
        out['variables'][v] = {'mse': mse, 'rmse': math.sqrt(mse), 'mae': float(row[7 + k]) / n, 'bias': float(row[13 + k]) / n,
                               'max_abs': float(row[19 + k])}
    if m > 0:
        for i, k in enumerate(LOSS_KEYS):
            out[k] = float(row[27 + i]) / m
    return out


# ------------------------------------------------------------------------------------------------ the reference's log lines
def _head(epoch, num_epoch, batch_id, n_batches, global_step):
    return 'epoch:%d/%d,batch:%d/%d,iter:%d/%d,' % (epoch, num_epoch, batch_id, n_batches, global_step, n_batches * num_epoch)


def format_train_line(epoch, num_epoch, batch_id, n_batches, global_step, train_loss, loss_dict, forecast_hours, fps, grad=None):
    """:609-618.  `grad` (the reference's sum of the parameters' gradient norms) is written only when the caller has it."""
    s = _head(epoch, num_epoch, batch_id, n_batches, global_step) + '%s:%f,' % ('train loss', float(train_loss))
    for k, v in loss_dict.items():
        s += '%s:%f,' % (k, float(v))
    s += '%s:%03dh,' % ('forecast', forecast_hours)
    if grad is not None:
        s += '%s:%f,' % ('grad', float(grad))
    return s + '%s:%f' % ('fps', fps)


def format_valid_line(epoch, num_epoch, batch_id, n_batches, global_step, valid_loss, loss_dict, forecast_hours, fps):
    """:720-733."""
    s = _head(epoch, num_epoch, batch_id, n_batches, global_step) + '%s:%f,' % ('valid loss', float(valid_loss))
    for k, v in loss_dict.items():
        s += '%s:%f,' % (k, float(v))
    return s + '%s:%03dh,' % ('forecast', forecast_hours) + '%s:%f' % ('fps', fps)


def _plain(v):
    if torch.is_tensor(v):
        return v.detach().cpu().tolist()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


class TrainLog:
    """`log_<date>.txt` (the reference's lines, :346-348 opens it the same way) and `metrics.jsonl` (one JSON object per event) under log_path;
    both appended to and flushed line by line.  Rank 0 owns one."""

    def __init__(self, log_path):
        os.makedirs(log_path, exist_ok=True)
        self.text_path = os.path.join(log_path, 'log_%s.txt' % time.strftime('%Y-%m-%d_%H_%M_%S', time.localtime()))
        self.json_path = os.path.join(log_path, 'metrics.jsonl')

    def line(self, text):
        with open(self.text_path, 'a') as fp:
            fp.write('%s\n' % text)

    def event(self, kind, **fields):
        rec = {'event': kind}
        rec.update(_plain(fields))
        with open(self.json_path, 'a') as fp:
            fp.write(json.dumps(rec) + '\n')
