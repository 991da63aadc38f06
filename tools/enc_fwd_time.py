#!/usr/bin/env python
"""Launch times of dpn_enc_fwd (and of dpn_enc_bwd head 1 without body) through the C ABI (the inputs of tools/enc_digest.py), for the library in DPN_LIB (default: the product build).

    python tools/enc_fwd_time.py [ROWS ...]          # default 287 574 1148: one field, B = 2, B = 4

Per row count and launch kind: microseconds per launch over 300 back-to-back launches between two events, best and median of five such
blocks.  Back to back the weight images stay in the L2s, so these are the L2-warm figures -- what the replication bound of dpn_enc_fwd is
decided on (batches of fields warm the L2s by themselves); the launches inside the captured step are in the rocprofv3 kernel trace."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location('enc_digest', os.path.join(ROOT, 'tools', 'enc_digest.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)
import ctypes
import torch
from deepphysinet_amd import _lib as L

N, BLOCKS = 300, 5


def time_case(rows, kind):
    lib = L.load()
    calls = []
    name = 'dpn_enc_bwd' if kind == 'bwd_qkv' else 'dpn_enc_fwd'
    orig = getattr(lib, name)

    def grab(p, stream):                       # run_case builds the argument block; keep it (and its tensors) for the timed loop
        calls.append(p)
        return orig(p, stream)
    setattr(lib, name, grab)
    try:
        out = D.run_case(rows, kind)
    finally:
        setattr(lib, name, orig)
    p = calls[0]
    for _ in range(20):
        orig(p, None)
    res = []
    for _ in range(BLOCKS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            orig(p, None)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1000.0 / N)
    del out
    res.sort()
    return res[0], res[len(res) // 2]


def main():
    rows_list = [int(a) for a in sys.argv[1:]] or [287, 574, 1148]
    lib = L.load()
    reps = lib.dpn_enc_fwd_replicas if hasattr(lib, 'dpn_enc_fwd_replicas') else None
    breps = lib.dpn_enc_bwd_replicas if hasattr(lib, 'dpn_enc_bwd_replicas') else None
    for fn in (reps, breps):
        if fn is not None:
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    print('library', os.path.basename(L.LIB_PATH))
    for rows in rows_list:
        for kind in D.KINDS:
            if kind == 'bwd_qkv':
                r = breps(rows, D.row_tiles(rows), 1, 0) if breps is not None else 1
            else:
                tail, nxt = (0, 1) if kind.startswith('first') else (1, int(kind[-1]))
                r = reps(rows, D.row_tiles(rows), tail, nxt) if reps is not None else 1
            best, med = time_case(rows, kind)
            print('rows %5d  %-11s replicas %d   best %7.2f us   median %7.2f us' % (rows, kind, r, best, med), flush=True)


if __name__ == '__main__':
    main()
