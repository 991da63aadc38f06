"""bench.py --dump-outputs of two libraries: per tensor the largest difference relative to the tensor's largest magnitude.  usage: compare_dumps.py A B"""
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
names = sorted(os.listdir(a_dir))
assert names == sorted(os.listdir(b_dir)), 'different sets of tensors'
rows, same = [], 0
for nm in names:
    a, b = np.load(os.path.join(a_dir, nm)).astype(np.float64), np.load(os.path.join(b_dir, nm)).astype(np.float64)
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), nm
    mx = np.abs(a).max()
    rel = float(np.abs(a - b).max() / mx) if mx > 0 else float(np.abs(b).max())
    same += int(np.array_equal(a, b))
    rows.append((rel, nm))
rows.sort(reverse=True)
print('%d tensors, %d bit-identical; largest difference relative to the tensor\'s largest magnitude:' % (len(names), same))
for kind in ('loss', 'grad_norm', 'grad.', 'param.'):
    sel = [r for r in rows if r[1].startswith(kind)]
    if sel:
        print('  %-10s worst %.3e (%s) over %d tensors' % (kind, sel[0][0], sel[0][1], len(sel)))
for rel, nm in rows[:12]:
    print('  %.3e  %s' % (rel, nm))
