#!/usr/bin/env python
"""Digests of what the row-local encoder forward launches and the first layer's q / k / v backward write (dpn_enc_pack -> dpn_enc_fwd | dpn_enc_bwd
through the C ABI), for the library in DPN_LIB
(default: the product build).  tests/test_gpu_enc_replicas.py holds the product build to tests/golden/enc_replicas_parent.json, which this
tool writes:

    DPN_LIB=<library of the commit to pin against> python tools/enc_digest.py            # on the GPU; rewrites the fixture
    python tools/enc_digest.py --print                                                   # digests of the product build, nothing written

Per case (rows, launch kind): the SHA-256 of the bytes of every output tensor of the launch -- y0, y1, y2, the eight saved tensors x1, xhat1,
rstd1, pre, act, x2, xhat2, rstd2, emb_out, and xf / xhatf / rstdf -- as far as the launch kind writes them.  Every output buffer is ZERO
before the launch, so a store that no workgroup makes shows up as a run of zeros.  Launch kinds: 'first' (tail 0, next 1, rows read from
xin), 'first_emb' (tail 0, next 1, rows assembled from the token convolution's slices), 'tail_next0' / 'tail_next1' / 'tail_next2' (tail 1),
'bwd_qkv' (dpn_enc_bwd head 1 without body: gx = res + dq Wq + dk Wk + dv Wv, and gx_head, its first 30 rows once more).
Inputs, weights and vectors come from CPU generators with fixed seeds, so they do not depend on the device's random numbers."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'enc_replicas_parent.json')
ROWS = (1, 16, 17, 287, 574, 2296)              # one padded block | one exact block | a second block of one row | one field | B = 2 | B = 8 (32-row workgroups)
KINDS = ('first', 'first_emb', 'tail_next0', 'tail_next1', 'tail_next2', 'bwd_qkv')
N_MATS = 7                                      # q, k, v, o, c1, c2 of one layer, then the output projection
N_PARTS = 19                                    # split-K slices of the token convolution in the workload
SAVED = ('x1', 'xhat1', 'rstd1', 'pre', 'act', 'x2', 'xhat2', 'rstd2')
_state = {}


def case_key(rows, kind):
    return '%d/%s' % (rows, kind)


def all_cases():
    return [(r, k) for r in ROWS for k in KINDS]


def row_tiles(rows):
    return 1 if rows <= 2048 else 2             # as deepphysinet_amd.encoder_ops picks it


def _randn(shape, seed, dev, scale=1.0):
    import torch
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev).contiguous()


def _weights(dev):
    """Seven [256, 256] matrices and the twelve parameter vectors, packed once per process."""
    import torch
    from deepphysinet_amd import _lib as L
    if 'wpack' not in _state:
        lib = L.load()
        mats = [_randn((256, 256), 100 + i, dev, 1.0 / 16.0) for i in range(N_MATS)]
        arr = (ctypes.c_void_p * N_MATS)(*[m.data_ptr() for m in mats])
        wpack = torch.zeros(int(lib.dpn_enc_pack_bytes(N_MATS)), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.dpn_enc_pack(N_MATS, arr, wpack.data_ptr(), status.data_ptr(), None), 'dpn_enc_pack')
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        vecs = {}
        for i, n in enumerate(('bo', 'be1', 'bc1', 'bc2', 'be2', 'bef', 'bn0', 'bn1', 'bn2')):
            vecs[n] = _randn((256,), 200 + i, dev, 0.1)
        for i, n in enumerate(('g1', 'g2', 'gf')):
            vecs[n] = 1.0 + _randn((256,), 300 + i, dev, 0.1)
        _state.update(mats=mats, wpack=wpack, vecs=vecs)
    return _state['wpack'], _state['vecs']


def run_case(rows, kind):
    """One dpn_enc_fwd launch on zero-filled outputs.  Returns {name: tensor} of everything the launch kind writes."""
    import torch
    from deepphysinet_amd import _lib as L
    dev = torch.device('cuda:0')
    lib = L.load()
    wpack, v = _weights(dev)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    if kind == 'bwd_qkv':
        b = L.DpnEncBwd()
        ins = [_randn((rows, 256), 20 + i, dev, sc) for i, sc in enumerate((1.0, 3.0, 0.5, 40.0))]       # res, dq, dk, dv: one row scale for three magnitudes
        out = {'gx': zeros(rows, 256), 'gx_head': zeros(min(30, rows), 256)}
        b.wpack, b.n_mats, b.rows, b.row_tiles, b.head, b.body = wpack.data_ptr(), N_MATS, rows, row_tiles(rows), 1, 0
        b.m_h0, b.m_h1, b.m_h2 = 0, 1, 2
        b.res, b.dq, b.dk, b.dv = (t.data_ptr() for t in ins)
        b.gx, b.gx_head, b.gx_head_rows = out['gx'].data_ptr(), out['gx_head'].data_ptr(), min(30, rows)
        L.check(lib.dpn_enc_bwd(ctypes.byref(b), None), 'dpn_enc_bwd')
        torch.cuda.synchronize()
        _state['last_inputs'] = ins
        return out
    f = L.DpnEncFwd()
    f.wpack, f.n_mats, f.rows, f.row_tiles = wpack.data_ptr(), N_MATS, rows, row_tiles(rows)
    keep, out = [], {}

    def put(**kw):
        for k_, t in kw.items():
            keep.append(t)
            setattr(f, k_, t.data_ptr() if isinstance(t, torch.Tensor) else t)

    if kind.startswith('first'):
        put(tail=0, next=1, m_n0=0, m_n1=1, m_n2=2, bn0=v['bn0'], bn1=v['bn1'], bn2=v['bn2'])
        if kind == 'first_emb':
            n_tok = 30 if rows > 30 else rows // 2
            T = rows - n_tok
            out['emb_out'] = zeros(rows, 256)
            put(xin=out['emb_out'], emb_parts=_randn((N_PARTS, max(T, 1), 256), 1, dev, 0.25), emb_bias=_randn((256,), 2, dev, 0.1),
                emb_pos=_randn((rows, 256), 3, dev), emb_te=_randn((256,), 4, dev), emb_token=_randn((max(n_tok, 1), 256), 5, dev),
                emb_out=out['emb_out'], emb_part_stride=max(T, 1) * 256, emb_n_parts=N_PARTS, emb_n_tok=n_tok)
        else:
            put(xin=_randn((rows, 256), 6, dev))
    else:
        nxt = int(kind[-1])
        for n in SAVED:
            out[n] = zeros(rows) if n.startswith('rstd') else zeros(rows, 256)
        put(tail=1, next=nxt, o=_randn((rows, 256), 7, dev), x=_randn((rows, 256), 8, dev), m_o=3, m_c1=4, m_c2=5, bo=v['bo'], g1=v['g1'], be1=v['be1'],
            bc1=v['bc1'], bc2=v['bc2'], g2=v['g2'], be2=v['be2'], **out)
        if nxt == 1:
            put(m_n0=0, m_n1=1, m_n2=2, bn0=v['bn0'], bn1=v['bn1'], bn2=v['bn2'])
        elif nxt == 2:
            fin = {'xf': zeros(rows, 256), 'xhatf': zeros(rows, 256), 'rstdf': zeros(rows)}
            out.update(fin)
            put(m_n0=6, gf=v['gf'], bef=v['bef'], bn0=v['bn0'], **fin)
    ys = ('y0', 'y1', 'y2') if f.next == 1 else (('y0',) if f.next == 2 else ())
    for n in ys:
        out[n] = zeros(rows, 256)
        put(**{n: out[n]})
    L.check(lib.dpn_enc_fwd(ctypes.byref(f), None), 'dpn_enc_fwd')
    torch.cuda.synchronize()
    _state['last_inputs'] = keep                 # (tools/enc_fwd_time.py repeats the launch: its inputs stay alive until the next case)
    return out


def digest(res):
    return {k: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, t in res.items()}


def write_fixture(out):
    """One line per case."""
    with open(FIXTURE, 'w') as f:
        f.write('{"library": %s, "cases": {\n' % json.dumps(out['library']))
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(d, sort_keys=True)) for k, d in sorted(out['cases'].items())))
        f.write('\n}}\n')


def main():
    from deepphysinet_amd import _lib as L
    out = {'library': os.path.basename(L.LIB_PATH), 'cases': {}}
    for rows, kind in all_cases():
        d = digest(run_case(rows, kind))
        out['cases'][case_key(rows, kind)] = d
        print(case_key(rows, kind), ' '.join('%s=%s' % (k, h[:8]) for k, h in sorted(d.items())), flush=True)
    if '--print' in sys.argv:
        return
    write_fixture(out)
    print('wrote', FIXTURE)


if __name__ == '__main__':
    main()
