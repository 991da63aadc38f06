"""GPU (MI355X): the row-local encoder launches and the attention kernels through the C ABI, stage by stage against fp64
(tests/encoder_cases.py, DESIGN.md section 5 "encoder launches").

Every output tensor of every launch is compared with the fp64 evaluation of ITS stage, started from the upstream tensor the GPU itself wrote,
so each condition is a one-stage condition:
  bit-exact (value equality, as torch.equal)
      * every GEMM-only output with integer operands (kinds A, AL: y0 / y1 / y2 of the first launch, gx of the q / k / v backward) and with
        selection weights (kinds S, MS: pre, y0 / y1 / y2, gx, dout -- the operand split, the x W^T and g W images, the fragment order of
        dpn_enc_pack and the matrix slots, at any row magnitude), including the fp32 bias / residual additions behind the GEMM;
      * emb_out of the launch that assembles its input (fp32 additions in the header's order);
      * the LayerNorm backward and its partial sums with integers and power-of-two rstd, where fp32 makes no rounding;
      * field b of a batch of three against the same field alone and in a batch of two (out, P, dq, dk, dv); P for q = 0; one-hot P and the
        row of v it selects; dpn_enc_prep's three parts against the three separate launches; dpn_im2col_circ3 against an index model;
        dpn_wgrad16 on integers;
      * every refused launch: -1 and every output buffer untouched.
  derived bounds, no element left out
      * a GEMM on arbitrary fp32 operands: gemm_bound();  a LayerNorm (forward or backward) behind it: ln_fwd_stage() / ln_bwd_stage();
      * attention: attn_forward_bounds() / attn_backward64().
  measured yardsticks (torch's fp32 evaluation of the same function on the same inputs against fp64, on the CPU, times MARGIN = 4)
      * GELU, GELU', the softmax's exp, sin / cos of dpn_lead_pe.  Nothing else.
Every input and output lives inside a larger owned buffer: input guards are NaN, output buffers hold a sentinel bit pattern, P is allocated
[batch][8][288][288] and its rows >= L must keep the sentinel.  The last test prints the largest error / bound seen per stage."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_cases as E

pytestmark = pytest.mark.gpu

RATIOS, YARDS = {}, {}
_PACKS = {}
PRE = E.GUARD_ROWS * E.D             # guard elements before and after every window


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _lib():
    from deepphysinet_amd import _lib as L
    return L, L.load()


class Buf:
    """A window of `shape` fp32 inside an owned 1-D buffer with PRE guard elements on both sides.  values given: an input, guards NaN;
    otherwise an output full of the sentinel."""

    def __init__(self, values=None, shape=None):
        if values is not None:
            values = np.ascontiguousarray(values, np.float32)
            shape = values.shape
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        host = np.full(self.n + 2 * PRE, np.nan if values is not None else E.SENTINEL, np.float32)
        if values is not None:
            host[PRE:PRE + self.n] = values.ravel()
        self.full = torch.from_numpy(host).to(_dev())
        self.ptr = self.full.data_ptr() + 4 * PRE

    def get(self):
        return self.full[PRE:PRE + self.n].cpu().numpy().reshape(self.shape)

    def guards_kept(self):
        h = self.full.cpu().numpy().view(np.uint32)
        return bool((h[:PRE] == E.SENTINEL_BITS).all() and (h[PRE + self.n:] == E.SENTINEL_BITS).all())

    def untouched(self):
        return bool((self.full.cpu().numpy().view(np.uint32) == E.SENTINEL_BITS).all())


def _pack(wkind):
    """The N_MATS matrices of a weight kind, packed once per process; the pack buffer's guards are checked too."""
    if wkind not in _PACKS:
        L, lib = _lib()
        mats, vec = E.weights(wkind)
        dmats = [Buf(m) for m in mats]
        arr = (ctypes.c_void_p * E.N_MATS)(*[b.ptr for b in dmats])
        assert int(lib.dpn_enc_pack_bytes(E.N_MATS)) == E.N_MATS * 2 * 256 * 1024
        wpack = Buf(shape=(E.N_MATS * 2 * 256 * 1024 // 4,))
        status = torch.zeros(1, dtype=torch.int32, device=_dev())
        L.check(lib.dpn_enc_pack(E.N_MATS, arr, wpack.ptr, status.data_ptr(), None), 'dpn_enc_pack')
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and wpack.guards_kept()
        dvec = {n: Buf(a) for n, a in vec.items()}
        _PACKS[wkind] = dict(mats=mats, vec=vec, dmats=dmats, wpack=wpack, dvec=dvec)
    return _PACKS[wkind]


def _record(stage, ratio):
    RATIOS[stage] = max(RATIOS.get(stage, 0.0), ratio)


def _check_outputs(direction, kind, okind, outs, st, yard, where):
    names = E.outputs_of(direction, kind)
    assert sorted(names) == sorted(st) == sorted(outs), where
    must = E.exact_outputs(direction, kind, okind)
    for n in names:
        assert outs[n].guards_kept(), (where, n, 'a store outside the logical extent')
        got = outs[n].get()
        assert not np.isnan(got).any(), (where, n, 'NaN: a load past the logical extent')
        if n in must:
            assert st[n].exact is not None, (where, n)
        bad, ratio = E.violations(got, st[n])
        print('%s %s: %s, error / bound %.3g' % (where, n, 'exact' if st[n].exact is not None else 'bounded', ratio))
        assert bad == 0, (where, n, '%d elements outside the condition' % bad, ratio)
        if st[n].exact is None:
            _record('%s %s' % (direction, n), ratio)
    for k, y in yard.items():
        YARDS[k] = max(YARDS.get(k, 0.0), y)


# ---------------------------------------------------------------------------------------------- dpn_enc_fwd
def _fill_fwd(kind, rows, rt, okind, ins):
    L, lib = _lib()
    pk = _pack(E.WEIGHT_KIND[okind])
    f = L.DpnEncFwd()
    f.wpack, f.n_mats, f.rows, f.row_tiles = pk['wpack'].ptr, E.N_MATS, rows, rt
    keep, outs = [], {}
    S, v = E.SLOT, pk['dvec']
    if kind.startswith('first'):
        f.tail, f.next = 0, 1
    else:
        f.tail, f.next = 1, int(kind[-1])
    if kind == 'first':
        keep.append(Buf(ins['xin']))
        f.xin = keep[-1].ptr
    elif kind == 'first_emb':
        n_tok, T, n_parts = E.emb_layout(rows)
        parts = np.full((n_parts, max(T, 1) + 3, E.D), np.nan, np.float32)       # a slice stride larger than the extent, NaN between the slices
        parts[:, :max(T, 1)] = ins['emb_parts']
        bufs = {n: Buf(ins[n]) for n in ('emb_token', 'emb_pos', 'emb_bias', 'emb_te')}
        bufs['emb_parts'] = Buf(parts)
        keep += list(bufs.values())
        outs['emb_out'] = Buf(shape=(rows, E.D))
        for n, b in bufs.items():
            setattr(f, n, b.ptr)
        f.emb_out, f.emb_part_stride, f.emb_n_parts, f.emb_n_tok = outs['emb_out'].ptr, (max(T, 1) + 3) * E.D, n_parts, n_tok
    else:
        keep += [Buf(ins['o']), Buf(ins['x'])]
        f.o, f.x = keep[0].ptr, keep[1].ptr
        f.m_o, f.m_c1, f.m_c2 = S['o'], S['c1'], S['c2']
        for n in ('bo', 'g1', 'be1', 'bc1', 'bc2', 'g2', 'be2'):
            setattr(f, n, v[n].ptr)
        for n in ('x1', 'xhat1', 'rstd1', 'pre', 'act', 'x2', 'xhat2', 'rstd2'):
            outs[n] = Buf(shape=(rows,) if n.startswith('rstd') else (rows, E.D))
            setattr(f, n, outs[n].ptr)
    if f.next == 1:
        f.m_n0, f.m_n1, f.m_n2 = S['q'], S['k'], S['v']
        for i in range(3):
            setattr(f, 'bn%d' % i, v['bn%d' % i].ptr)
            outs['y%d' % i] = Buf(shape=(rows, E.D))
            setattr(f, 'y%d' % i, outs['y%d' % i].ptr)
    elif f.next == 2:
        f.m_n0, f.bn0, f.gf, f.bef = S['p'], v['bn0'].ptr, v['gf'].ptr, v['bef'].ptr
        for n in ('xf', 'xhatf', 'rstdf', 'y0'):
            outs[n] = Buf(shape=(rows,) if n == 'rstdf' else (rows, E.D))
            setattr(f, n, outs[n].ptr)
    return f, outs, keep, pk


def _run_fwd(kind, rt, rows, okind):
    L, lib = _lib()
    ins = E.fwd_inputs(kind, rows, okind)
    f, outs, keep, pk = _fill_fwd(kind, rows, rt, okind, ins)
    L.check(lib.dpn_enc_fwd(ctypes.byref(f), None), 'dpn_enc_fwd')
    torch.cuda.synchronize()
    gpu = {n: b.get() for n, b in outs.items()}
    st, yard = E.fwd_reference(kind, ins, gpu, pk['mats'], pk['vec'])
    _check_outputs('fwd', kind, okind, outs, st, yard, 'fwd %s rt%d rows%d %s' % (kind, rt, rows, okind))


FWD_GROUPS = [(k, rt, o) for k in E.FWD_KINDS for rt in (1, 2) for o in E.OPERAND_KINDS]
BWD_GROUPS = [(k, rt, o) for k in E.BWD_KINDS for rt in (1, 2) for o in E.OPERAND_KINDS]
_ID = lambda g: '%s-rt%d-%s' % (g[0] if isinstance(g[0], str) else 'head%d_body%d' % g[0], g[1], g[2])


@pytest.mark.parametrize('group', FWD_GROUPS, ids=_ID)
def test_forward_launch_stage_by_stage(group):
    """Every row count of the table (and 2049 rows once per launch kind, kind A) for one (launch kind, row_tiles, operand kind)."""
    kind, rt, okind = group
    for c in E.fwd_cases():
        if (c[0], c[1], c[3]) == group:
            _run_fwd(kind, rt, c[2], okind)


# ---------------------------------------------------------------------------------------------- dpn_enc_bwd
def _fill_bwd(kind, rows, rt, okind, ins, gx_head_rows=None):
    L, lib = _lib()
    head, body = kind
    pk = _pack(E.WEIGHT_KIND[okind])
    b = L.DpnEncBwd()
    b.wpack, b.n_mats, b.rows, b.row_tiles, b.head, b.body = pk['wpack'].ptr, E.N_MATS, rows, rt, head, body
    S, v = E.SLOT, pk['dvec']
    keep = {n: Buf(a) for n, a in ins.items()}
    for n, buf in keep.items():
        setattr(b, n, buf.ptr)
    nb = (rows + 16 * rt - 1) // (16 * rt)
    outs = {}
    if head == 1:
        b.m_h0, b.m_h1, b.m_h2 = S['q'], S['k'], S['v']
    elif head == 2:
        b.m_h0, b.gf = S['p'], v['gf'].ptr
        outs['partial_f'] = Buf(shape=(nb, 512))
    if body:
        b.m_c2, b.m_c1, b.m_o, b.g2, b.g1 = S['c2'], S['c1'], S['o'], v['g2'].ptr, v['g1'].ptr
        for n in ('gs2', 'dpre', 'gs1', 'dout'):
            outs[n] = Buf(shape=(rows, E.D))
        outs['partial2'], outs['partial1'] = Buf(shape=(nb, 512)), Buf(shape=(nb, 512))
    else:
        outs['gx'] = Buf(shape=(rows, E.D))
    for n, buf in outs.items():
        setattr(b, n, buf.ptr)
    gx_head = None
    if gx_head_rows is not None:
        gx_head = Buf(shape=(rows, E.D))
        b.gx_head, b.gx_head_rows = gx_head.ptr, gx_head_rows
    return b, outs, keep, pk, gx_head


def _run_bwd(kind, rt, rows, okind, gx_head_rows=None):
    L, lib = _lib()
    ins = E.bwd_inputs(kind, rows, okind)
    b, outs, keep, pk, gx_head = _fill_bwd(kind, rows, rt, okind, ins, gx_head_rows)
    L.check(lib.dpn_enc_bwd(ctypes.byref(b), None), 'dpn_enc_bwd')
    torch.cuda.synchronize()
    gpu = {n: o.get() for n, o in outs.items()}
    st, yard = E.bwd_reference(kind, ins, gpu, pk['mats'], pk['vec'], rt)
    where = 'bwd head%d body%d rt%d rows%d %s' % (kind[0], kind[1], rt, rows, okind)
    _check_outputs('bwd', kind, okind, outs, st, yard, where)
    if gx_head is not None:                      # the first gx_head_rows rows of gx once more, nothing behind them
        n = min(gx_head_rows, rows)
        h = gx_head.get()
        assert np.array_equal(h[:n].view(np.uint32), gpu['gx'][:n].view(np.uint32)), where
        assert (h[n:].view(np.uint32) == E.SENTINEL_BITS).all() and gx_head.guards_kept(), where
    return outs, st, keep


@pytest.mark.parametrize('group', BWD_GROUPS, ids=_ID)
def test_backward_launch_stage_by_stage(group):
    kind, rt, okind = group
    for c in E.bwd_cases():
        if (c[0], c[1], c[3]) == group:
            if kind == (1, 0):
                for gh in E.GX_HEAD_ROWS:
                    _run_bwd(kind, rt, c[2], okind, c[2] if gh == 'rows' else gh)
            else:
                _run_bwd(kind, rt, c[2], okind)


@pytest.mark.parametrize('case', E.replica_cases(), ids=lambda c: '%s-%s-%d-%s' % (c[0], c[1] if isinstance(c[1], str) else 'head%d_body%d' % c[1], c[2], c[4]))
def test_replica_rule_edges(case):
    """The q / k / v launches on both sides of the replica rules' edges; what the host functions return is asserted first, so it is known
    which kernel ran.  Kinds A and S only: every output is an equality."""
    direction, kind, rows, expect, okind = case
    L, lib = _lib()
    for fn in (lib.dpn_enc_fwd_replicas, lib.dpn_enc_bwd_replicas):
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    if direction == 'fwd':
        assert lib.dpn_enc_fwd_replicas(rows, 1, int(kind.startswith('tail')), 1) == expect
        _run_fwd(kind, 1, rows, okind)
    else:
        assert lib.dpn_enc_bwd_replicas(rows, 1, kind[0], kind[1]) == expect
        _run_bwd(kind, 1, rows, okind, 30)


@pytest.mark.parametrize('rt,rows', [(1, 33), (2, 33), (1, 287), (2, 2049)])
def test_partial_sums_through_a_colsum_job(rt, rows):
    """partial_f / partial2 / partial1 of a launch with the output-projection head through DpnColsumJobs of a dpn_wgrad16 launch that carries only
    jobs: dgamma / dbeta against fp64 sums over the rows.  Bound: the partial sums' own bounds added up, plus n_blocks additions in fp32."""
    L, lib = _lib()
    okind = 'A' if rows == E.ROWS_BIG else 'C'
    outs, st, keep = _run_bwd((2, 1), rt, rows, okind)
    nb = (rows + 16 * rt - 1) // (16 * rt)
    names = ('partial_f', 'partial2', 'partial1')
    res = {n: (Buf(shape=(256,)), Buf(shape=(256,))) for n in names}
    jobs = (L.DpnColsumJob * 3)()
    for j, n in zip(jobs, names):
        j.partial, j.out_a, j.out_b, j.n_blocks = outs[n].ptr, res[n][0].ptr, res[n][1].ptr, nb
    L.check(lib.dpn_wgrad16(0, None, 3, jobs, 1, None, None), 'dpn_wgrad16 (jobs only)')
    torch.cuda.synchronize()
    for n in names:
        part = outs[n].get().astype(np.float64)
        ref = st[n].ref.sum(axis=0)
        bound = (st[n].bound.sum(axis=0) if st[n].bound is not None else 0.0) + nb * E.U * np.abs(part).sum(axis=0)
        got = np.concatenate([res[n][0].get(), res[n][1].get()]).astype(np.float64)
        assert res[n][0].guards_kept() and res[n][1].guards_kept()
        err = np.abs(got - ref)
        if st[n].exact is not None and E._sum_exact(part, 0):
            assert np.array_equal(got, ref), n
        else:
            assert np.all(err <= bound), (n, float((err / bound).max()))
            _record('colsum job ' + n, float((err / np.maximum(bound, 1e-300)).max()))


def test_pack_status_flag():
    """An |entry| >= 32768 sets bit 0 of status_dev, 32767.5 leaves it clear; a clear flag is not written at all."""
    L, lib = _lib()
    for value, expect in ((32767.5, 0), (-32767.5, 0), (32768.0, 1), (-32768.0, 1), (float('inf'), 1)):
        mats = [np.zeros((256, 256), np.float32) for _ in range(2)]
        mats[1][200, 3] = value
        d = [Buf(m) for m in mats]
        arr = (ctypes.c_void_p * 2)(*[b.ptr for b in d])
        wp = Buf(shape=(2 * 2 * 256 * 1024 // 4,))
        status = torch.full((3,), 4, dtype=torch.int32, device=_dev())
        L.check(lib.dpn_enc_pack(2, arr, wp.ptr, status.data_ptr() + 4, None), 'dpn_enc_pack')
        torch.cuda.synchronize()
        assert status.tolist() == [4, 4 | expect, 4] and wp.guards_kept(), value


# ---------------------------------------------------------------------------------------------- refusals
def _fwd_refusals():
    NULL = None
    out = []
    for kind, muts in (
        ('tail_next1', [('rows', 0), ('rows', -1), ('n_mats', 0), ('n_mats', 33), ('next', 3), ('next', -1), ('row_tiles', 3), ('row_tiles', 0), ('wpack', NULL),
                        ('m_o', E.N_MATS), ('m_c1', E.N_MATS), ('m_c2', -1), ('m_n0', E.N_MATS), ('m_n1', E.N_MATS), ('m_n2', E.N_MATS)] +
         [(n, NULL) for n in ('o', 'x', 'bo', 'g1', 'be1', 'bc1', 'bc2', 'g2', 'be2', 'x1', 'xhat1', 'rstd1', 'pre', 'act', 'x2', 'xhat2', 'rstd2', 'y0', 'y1', 'y2')]),
        ('tail_next2', [('m_n0', E.N_MATS)] + [(n, NULL) for n in ('y0', 'gf', 'bef', 'xf', 'xhatf', 'rstdf')]),
        ('first', [('next', 0), ('next', 2), ('xin', NULL), ('m_n0', -1), ('y1', NULL)]),
        ('first_emb', [('emb_pos', NULL), ('emb_te', NULL), ('emb_out', NULL), ('emb_n_parts', 0), ('emb_n_tok', -1), ('emb_token', NULL), ('emb_part_stride', -256),
                       ('emb_n_tok', 34), ('emb_part_stride', 0), ('emb_part_stride', 2 * 256)]),
    ):
        out += [(kind, m) for m in muts]
    return out


@pytest.mark.parametrize('kind,mut', _fwd_refusals(), ids=lambda x: x if isinstance(x, str) else '%s=%s' % x)
def test_forward_refuses_bad_arguments(kind, mut):
    """Every -1 path of dpn_enc_fwd a wrong struct can reach: the host code rejects it before any launch, every output keeps the sentinel.
    (rows = 33: 30 learnable tokens + 3 convolution rows in 19 slices -- emb_n_tok = 34 > rows, and a slice stride of 0 or 2 rows < 3 rows with
    more than one slice, are the two checks of ADVICE.md's first finding.)"""
    L, lib = _lib()
    rows = 33
    ins = E.fwd_inputs(kind, rows, 'C')
    f, outs, keep, pk = _fill_fwd(kind, rows, 1, 'C', ins)
    setattr(f, mut[0], mut[1])
    assert lib.dpn_enc_fwd(ctypes.byref(f), None) == -1
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values())
    assert lib.dpn_enc_fwd(None, None) == -1


def _bwd_refusals():
    NULL = None
    out = [((1, 1), m) for m in [('rows', 0), ('head', 3), ('head', -1), ('row_tiles', 3), ('wpack', NULL), ('n_mats', 0), ('n_mats', 33), ('m_h0', E.N_MATS),
                                 ('m_h1', -1), ('m_h2', E.N_MATS), ('m_c2', E.N_MATS), ('m_c1', E.N_MATS), ('m_o', E.N_MATS)] +
           [(n, NULL) for n in ('res', 'dq', 'dk', 'dv', 'xhat2', 'rstd2', 'pre', 'xhat1', 'rstd1', 'g2', 'g1', 'gs2', 'dpre', 'gs1', 'dout', 'partial2', 'partial1')]]
    out += [((2, 1), m) for m in [('m_h0', E.N_MATS)] + [(n, NULL) for n in ('dmeta', 'xhatf', 'rstdf', 'gf', 'partial_f')]]
    out += [((0, 1), m) for m in [('gin', NULL), ('body', 0)]]
    out += [((1, 0), m) for m in [('gx', NULL), ('head', 0), ('head', 2)]]       # (head 2 without a body: dmeta is missing)
    return out


@pytest.mark.parametrize('kind,mut', _bwd_refusals(), ids=lambda x: 'head%d_body%d' % x if isinstance(x[0], int) else '%s=%s' % x)
def test_backward_refuses_bad_arguments(kind, mut):
    L, lib = _lib()
    rows = 33
    ins = E.bwd_inputs(kind, rows, 'C')
    b, outs, keep, pk, gx_head = _fill_bwd(kind, rows, 1, 'C', ins, 30 if kind == (1, 0) else None)
    setattr(b, mut[0], mut[1])
    assert lib.dpn_enc_bwd(ctypes.byref(b), None) == -1
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values()) and (gx_head is None or gx_head.untouched())
    assert lib.dpn_enc_bwd(None, None) == -1


# ---------------------------------------------------------------------------------------------- attention
def _attn_run(q, k, v, go, L, batch):
    """dpn_attn_fwd, dpn_attn16_fwd and dpn_attn_bwd (from the f16 kernel's P and out: what the product saves) on one set of inputs."""
    Lb, lib = _lib()
    ins = {n: Buf(a) for n, a in (('q', q), ('k', k), ('v', v), ('go', go))}
    r = {'ins': ins}
    for name, fn in (('f32', lib.dpn_attn_fwd), ('f16', lib.dpn_attn16_fwd)):
        out, P = Buf(shape=(batch * L, E.D)), Buf(shape=(batch, E.HEADS, E.LMAX, E.LMAX))
        Lb.check(fn(ins['q'].ptr, ins['k'].ptr, ins['v'].ptr, L, batch, out.ptr, P.ptr, None), 'attention forward ' + name)
        r[name] = (out, P)
    out, P = r['f16']
    d = {n: Buf(shape=(batch * L, E.D)) for n in ('dq', 'dk', 'dv')}
    Lb.check(lib.dpn_attn_bwd(ins['q'].ptr, ins['k'].ptr, ins['v'].ptr, out.ptr, P.ptr, ins['go'].ptr, L, batch, d['dq'].ptr, d['dk'].ptr, d['dv'].ptr, None),
             'dpn_attn_bwd')
    torch.cuda.synchronize()
    r['bwd'] = d
    return r


def _p_window(P, L):
    """(P[:, :, :L, :L], everything of rows < L behind column L, whether the rows >= L and the guards still hold the sentinel)."""
    full = P.get()
    rest = full[:, :, L:, :].view(np.uint32)
    return full[:, :, :L, :L], full[:, :, :L, L:], bool((rest == E.SENTINEL_BITS).all()) and P.guards_kept()


def _check_attention(q, k, v, go, L, batch, r, tag):
    s64, P64, out64 = E.attn_forward64(q, k, v, L, batch)
    arg = np.maximum(s64 - s64.max(axis=-1, keepdims=True), -87.0)
    y_exp = E.yardstick(E.torch_exp32, np.exp, arg.astype(np.float32), lambda a: np.exp(a))
    YARDS['exp'] = max(YARDS.get('exp', 0.0), y_exp)
    for name, split in (('f32', False), ('f16', True)):
        out, P = r[name]
        Pw, Ptail, kept = _p_window(P, L)
        assert kept, (tag, name, 'P rows >= L or a guard were written')
        assert not np.isnan(Pw).any() and not np.isnan(out.get()).any(), (tag, name, 'NaN: a load past L')
        assert (Ptail.view(np.uint32) & 0x7fffffff == 0).all(), (tag, name, 'columns L .. 287 of a written row are 0.0')
        bP, bo = E.attn_forward_bounds(q, k, v, L, batch, s64, P64, split, y_exp)
        eP, eo = np.abs(Pw - P64), np.abs(out.get() - out64)
        assert np.all(eP <= bP), (tag, name, 'P', float((eP / bP).max()))
        assert np.all(eo <= bo), (tag, name, 'out', float((eo / bo).max()))
        assert out.guards_kept()
        _record('attention %s P' % name, float((eP / bP).max()))
        _record('attention %s out' % name, float((eo / bo).max()))
    out, P = r['f16']
    st = E.attn_backward64(q, k, v, out.get(), _p_window(P, L)[0], go, L, batch)
    for n in ('dq', 'dk', 'dv'):
        got = r['bwd'][n].get()
        assert r['bwd'][n].guards_kept() and not np.isnan(got).any(), (tag, n)
        bad, ratio = E.violations(got, st[n])
        assert bad == 0, (tag, n, ratio)
        _record('attention ' + n, ratio)


@pytest.mark.parametrize('L', E.ATTN_L)
def test_attention_three_entry_points_vs_fp64(L):
    """All three entry points on L x batch {1, 2, 3}: both forward kernels against the same fp64 P and out, the backward against fp64 from the
    saved P and out; field b of the batch of three bit for bit the same field alone and in a batch of two (three roles in the backward for
    batch 1 and 2, two for batch 3)."""
    runs = {}
    for batch in E.ATTN_BATCH:
        q, k, v, go = E.attn_inputs(L, batch)
        runs[batch] = (q, k, v, go, _attn_run(q, k, v, go, L, batch))
        _check_attention(q, k, v, go, L, batch, runs[batch][4], 'L%d batch%d' % (L, batch))
    q, k, v, go, r3 = runs[3]
    rows = lambda a, b0, nb: a[b0 * L:(b0 + nb) * L]
    for b0, nb in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2)):
        r = _attn_run(rows(q, b0, nb), rows(k, b0, nb), rows(v, b0, nb), rows(go, b0, nb), L, nb)
        for name in ('f32', 'f16'):
            assert np.array_equal(r[name][0].get(), rows(r3[name][0].get(), b0, nb)), (L, b0, nb, name, 'out')
            assert np.array_equal(_p_window(r[name][1], L)[0], _p_window(r3[name][1], L)[0][b0:b0 + nb]), (L, b0, nb, name, 'P')
        for n in ('dq', 'dk', 'dv'):
            assert np.array_equal(r['bwd'][n].get(), rows(r3['bwd'][n].get(), b0, nb)), (L, b0, nb, n)


@pytest.mark.parametrize('L,batch', [(33, 2), (287, 1)])
def test_attention_large_logits(L, batch):
    """Scores of order +-80: the non-maximal probabilities underflow."""
    q, k, v, go = E.attn_inputs(L, batch, 'large')
    s64, P64, _ = E.attn_forward64(q, k, v, L, batch)
    assert np.abs(s64).max() > 80 and (P64 < 2.0 ** -126).mean() > 0.2
    _check_attention(q, k, v, go, L, batch, _attn_run(q, k, v, go, L, batch), 'large L%d' % L)


@pytest.mark.parametrize('L', E.ATTN_L)
def test_attention_zero_queries_give_uniform_probabilities_bitwise(L):
    q, k, v, go = E.attn_inputs(L, 1, 'zero_q')
    r = _attn_run(q, k, v, go, L, 1)
    want = np.float32(1.0) * (np.float32(1.0) / np.float32(L))
    for name in ('f32', 'f16'):
        Pw, Ptail, kept = _p_window(r[name][1], L)
        assert kept and (Pw.view(np.uint32) == want.view(np.uint32)).all() and (Ptail.view(np.uint32) == 0).all(), (L, name)


@pytest.mark.parametrize('L', [1, 17, 33])
def test_attention_one_hot_scores_select_a_row_of_v(L):
    """One key per query wins by more than 104 after scaling: P is exactly one-hot.  dpn_attn_fwd (an fp32 fmaf chain over zeros and 1 v)
    returns that row of v bit for bit.  dpn_attn16_fwd returns it through the split -- EXACTLY, but with the power-of-two scale of the wave
    that owns the key block (the maximum over all values of key blocks w, w + 4, w + 8 of the head, not the row's own maximum): P's 1.0 is
    exact in f16, so main = hi, cross = lo' and fmaf(lo', 1/2048, hi) is the split value."""
    q, k, v, go = E.attn_inputs(L, 1, 'one_hot')
    r = _attn_run(q, k, v, go, L, 1)
    win = E.one_hot_winner(L)
    onehot = np.zeros((1, E.HEADS, L, L), np.float32)
    onehot[:, :, np.arange(L), win] = 1.0
    for name in ('f32', 'f16'):
        assert np.array_equal(_p_window(r[name][1], L)[0], onehot), (L, name)
    assert np.array_equal(r['f32'][0].get(), v[win]), L
    vh = v.reshape(L, E.HEADS, E.HD)
    want = np.zeros_like(vh)
    for h in range(E.HEADS):
        for i, j in enumerate(win):
            w = (j // 32) % 4
            keys = [t for t in range(L) if (t // 32) % 4 == w]
            s = E.split22(vh[j:j + 1, h, :], extra_max=[np.abs(vh[keys, h, :]).max()])
            want[i, h] = s.recombined()[0]
    assert np.array_equal(r['f16'][0].get(), want.reshape(L, E.D)), L


def test_attention_refuses_bad_arguments():
    Lb, lib = _lib()
    L, batch = 17, 1
    q, k, v, go = E.attn_inputs(L, batch)
    ins = [Buf(a) for a in (q, k, v, go)]
    for fn in (lib.dpn_attn_fwd, lib.dpn_attn16_fwd):
        out, P = Buf(shape=(batch * L, E.D)), Buf(shape=(batch, E.HEADS, E.LMAX, E.LMAX))
        good = [ins[0].ptr, ins[1].ptr, ins[2].ptr, L, batch, out.ptr, P.ptr, None]
        bad = [(3, 0), (3, 289), (3, -1), (4, 0), (4, 32768)] + [(i, None) for i in (0, 1, 2, 5, 6)]
        for i, val in bad:
            a = list(good)
            a[i] = val
            assert fn(*a) == -1, (i, val)
        torch.cuda.synchronize()
        assert out.untouched() and P.untouched()
    d = [Buf(shape=(batch * L, E.D)) for _ in range(3)]
    o, P = Buf(q), Buf(np.zeros((batch, E.HEADS, E.LMAX, E.LMAX), np.float32))
    good = [ins[0].ptr, ins[1].ptr, ins[2].ptr, o.ptr, P.ptr, ins[3].ptr, L, batch, d[0].ptr, d[1].ptr, d[2].ptr, None]
    for i, val in [(6, 0), (6, 289), (7, 0), (7, 16384)] + [(i, None) for i in (0, 1, 2, 3, 4, 5, 8, 9, 10)]:
        a = list(good)
        a[i] = val
        assert lib.dpn_attn_bwd(*a) == -1, (i, val)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in d)


# ---------------------------------------------------------------------------------------------- dpn_wgrad16
class Mat:
    """[rows][cols] with leading dimension cols + 5 inside a Buf: pad columns NaN (input) or sentinel (output)."""

    def __init__(self, values=None, shape=None):
        rows, cols = values.shape if values is not None else shape
        self.cols, self.ld = cols, cols + 5
        if values is not None:
            host = np.full((rows, self.ld), np.nan, np.float32)
            host[:, :cols] = values
            self.buf = Buf(host)
        else:
            self.buf = Buf(shape=(rows, self.ld))
        self.ptr = self.buf.ptr

    def get(self):
        return self.buf.get()[:, :self.cols]

    def guards_kept(self):
        return self.buf.guards_kept() and bool((self.buf.get()[:, self.cols:].view(np.uint32) == E.SENTINEL_BITS).all())


def _wgrad_launch(probs, slices):
    """probs: [(G, X, with_db)] host arrays.  Returns [(dW Mat, db Buf or None)]."""
    L, lib = _lib()
    n = len(probs)
    arr = (L.DpnWgradProblem * n)()
    keep, outs = [], []
    for q, (g, x, with_db) in zip(arr, probs):
        dg, dx, dw = Mat(g), Mat(x), Mat(shape=(g.shape[1], x.shape[1]))
        db = Buf(shape=(g.shape[1],)) if with_db else None
        keep += [dg, dx]
        outs.append((dw, db))
        q.G, q.X, q.dW, q.db = dg.ptr, dx.ptr, dw.ptr, db.ptr if with_db else None
        q.M, q.N, q.rows, q.ldg, q.ldx, q.ldw = g.shape[1], x.shape[1], g.shape[0], dg.ld, dx.ld, dw.ld
    partials = None
    if slices > 1:
        nf = int(lib.dpn_wgrad16_partial_floats(n, arr, slices))
        assert nf == slices * sum(g.shape[1] * x.shape[1] + (g.shape[1] if w else 0) for g, x, w in probs)
        partials = Buf(shape=(nf,))
    L.check(lib.dpn_wgrad16(n, arr, 0, None, slices, partials.ptr if partials else None, None), 'dpn_wgrad16')
    torch.cuda.synchronize()
    assert partials is None or partials.guards_kept()
    return outs


@pytest.mark.parametrize('slices', E.WGRAD_SLICES)
@pytest.mark.parametrize('rows', E.WGRAD_ROWS)
@pytest.mark.parametrize('kind', ['A', 'C', 'M'])
def test_wgrad16_ragged_list(kind, rows, slices):
    """The ragged problem list in one launch, db NULL and given, ldg / ldx / ldw larger than the extents: integers bit for bit, normal values
    and rows 2^60 apart inside wgrad_stage()'s bound (relative to |G|^T |X| and to the operand strips' maxima)."""
    probs = E.wgrad_inputs(rows, kind)
    for (g, x, with_db), (dw, db) in zip(probs, _wgrad_launch(probs, slices)):
        st, sb = E.wgrad_stage(g, x, slices)
        assert (st.exact is not None) == (kind == 'A')
        where = 'wgrad16 %s rows%d slices%d %dx%d' % (kind, rows, slices, g.shape[1], x.shape[1])
        for got, stage, name in ((dw, st, 'dW'),) + (((db, sb, 'db'),) if with_db else ()):
            assert got.guards_kept(), (where, name)
            v = got.get()
            assert not np.isnan(v).any(), (where, name, 'NaN: a load past the logical extent')
            bad, ratio = E.violations(v, stage)
            assert bad == 0, (where, name, bad, ratio)
            if stage.exact is None:
                _record('wgrad16 %s kind %s' % (name, kind), ratio)


def test_wgrad16_refuses_bad_arguments():
    L, lib = _lib()
    g, x, _ = E.wgrad_inputs(33, 'A')[3]
    dg, dx, dw, db = Mat(g), Mat(x), Mat(shape=(g.shape[1], x.shape[1])), Buf(shape=(g.shape[1],))
    part, oa, ob = Buf(np.zeros((3, 512), np.float32)), Buf(shape=(256,)), Buf(shape=(256,))

    def problem(**kw):
        arr = (L.DpnWgradProblem * 1)()
        q = arr[0]
        q.G, q.X, q.dW, q.db = dg.ptr, dx.ptr, dw.ptr, db.ptr
        q.M, q.N, q.rows, q.ldg, q.ldx, q.ldw = g.shape[1], x.shape[1], 33, dg.ld, dx.ld, dw.ld
        for k, v in kw.items():
            setattr(q, k, v)
        return arr

    def job(**kw):
        arr = (L.DpnColsumJob * 1)()
        arr[0].partial, arr[0].out_a, arr[0].out_b, arr[0].n_blocks = part.ptr, oa.ptr, ob.ptr, 3
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr
    calls = [(1, problem(**{k: v}), 0, None, 1, None) for k, v in
             [('G', None), ('X', None), ('dW', None), ('M', 0), ('N', 0), ('rows', 0), ('ldg', g.shape[1] - 1), ('ldx', x.shape[1] - 1), ('ldw', x.shape[1] - 1)]]
    calls += [(-1, problem(), 0, None, 1, None), (33, problem(), 0, None, 1, None), (1, None, 0, None, 1, None), (0, None, 0, None, 1, None),
              (1, problem(), -1, None, 1, None), (1, problem(), 11, job(), 1, None), (1, problem(), 1, None, 1, None), (1, problem(), 0, None, 0, None),
              (1, problem(), 0, None, 2, None)]
    calls += [(0, None, 1, job(**{k: v}), 1, None) for k, v in [('partial', None), ('out_a', None), ('out_b', None), ('n_blocks', 0)]]
    for c in calls:
        assert lib.dpn_wgrad16(*c, None) == -1, c
    torch.cuda.synchronize()
    assert all(b.buf.untouched() if isinstance(b, Mat) else b.untouched() for b in (dw, db, oa, ob))


# ---------------------------------------------------------------------------------------------- dpn_enc_prep
def _prep_parts(T, C, batch, seed):
    rng = np.random.default_rng(seed)
    mats = [rng.standard_normal((256, 256)).astype(np.float32) for _ in range(3)]
    x = rng.standard_normal((batch * T, C)).astype(np.float32)
    h = rng.uniform(0.05, 0.95, size=batch).astype(np.float32)
    fa = (2.0 ** np.linspace(0, 8, 128)).astype(np.float32)
    fb = (2.0 ** np.linspace(0, 6, 96)).astype(np.float32)
    return mats, x, h, fa, fb


@pytest.mark.parametrize('batch', E.PREP_BATCH)
@pytest.mark.parametrize('C', E.PREP_C)
@pytest.mark.parametrize('T', E.PREP_T)
def test_enc_prep_equals_the_three_separate_launches(T, C, batch):
    """Weight images, im2col rows and both PE tables of ONE dpn_enc_prep launch bit for bit what dpn_enc_pack, dpn_im2col_circ3 and dpn_lead_pe
    write, every subset of the three parts present (and the second PE table present and absent); im2col against the integer index model (the
    circular wrap at T = 1 and T = 2); the PE tables against fp64 sin / cos of the fp32 product h f."""
    L, lib = _lib()
    mats, x, h, fa, fb = _prep_parts(T, C, batch, 100 * T + 10 * C + batch)
    dm, dx, dh, dfa, dfb = [Buf(m) for m in mats], Buf(x), Buf(h), Buf(fa), Buf(fb)
    warr = (ctypes.c_void_p * 3)(*[b.ptr for b in dm])
    nbytes = int(lib.dpn_enc_pack_bytes(3))
    # the separate launches
    wp0, xu0, oa0, ob0 = Buf(shape=(nbytes // 4,)), Buf(shape=(batch * T, 3 * C)), Buf(shape=(batch, 256)), Buf(shape=(batch, 192))
    L.check(lib.dpn_enc_pack(3, warr, wp0.ptr, None, None), 'dpn_enc_pack')
    L.check(lib.dpn_im2col_circ3(dx.ptr, T, C, batch, xu0.ptr, None), 'dpn_im2col_circ3')
    L.check(lib.dpn_lead_pe(dh.ptr, batch, dfa.ptr, 128, oa0.ptr, dfb.ptr, 96, ob0.ptr, None), 'dpn_lead_pe')
    torch.cuda.synchronize()
    assert all(b.guards_kept() for b in (wp0, xu0, oa0, ob0))
    assert np.array_equal(xu0.get(), E.im2col_circ3_model(x, T, C, batch))
    for got, freqs, name in ((oa0, fa, 'lead_pe a'), (ob0, fb, 'lead_pe b')):
        st, Y = E.lead_pe_stage(h, freqs)
        YARDS['sin/cos'] = max(YARDS.get('sin/cos', 0.0), Y)
        bad, ratio = E.violations(got.get(), st)
        assert bad == 0, (name, ratio)
        _record(name, ratio)
    for mask in range(1, 8):
        for with_b in ((True, False) if mask & 4 else (True,)):
            p = L.DpnEncPrep()
            wp, xu, oa, ob = Buf(shape=(nbytes // 4,)), Buf(shape=(batch * T, 3 * C)), Buf(shape=(batch, 256)), Buf(shape=(batch, 192))
            status = torch.zeros(1, dtype=torch.int32, device=_dev())
            p.batch = batch
            if mask & 1:
                p.n_mats, p.weights, p.packed, p.status_dev = 3, ctypes.cast(warr, ctypes.c_void_p), wp.ptr, status.data_ptr()
            if mask & 2:
                p.x, p.T, p.C, p.xu = dx.ptr, T, C, xu.ptr
            if mask & 4:
                p.h, p.freqs_a, p.n_a, p.out_a = dh.ptr, dfa.ptr, 128, oa.ptr
                if with_b:
                    p.freqs_b, p.n_b, p.out_b = dfb.ptr, 96, ob.ptr
            L.check(lib.dpn_enc_prep(ctypes.byref(p), None), 'dpn_enc_prep')
            torch.cuda.synchronize()
            for present, got, want in ((mask & 1, wp, wp0), (mask & 2, xu, xu0), (mask & 4, oa, oa0), (mask & 4 and with_b, ob, ob0)):
                if present:
                    assert got.guards_kept() and np.array_equal(got.get().view(np.uint32), want.get().view(np.uint32)), (mask, with_b)
                else:
                    assert got.untouched(), (mask, with_b)
            assert int(status.item()) == 0


def test_enc_prep_refuses_bad_arguments():
    L, lib = _lib()
    T, C, batch = 3, 5, 3
    mats, x, h, fa, fb = _prep_parts(T, C, batch, 1)
    dm, dx, dh, dfa, dfb = [Buf(m) for m in mats], Buf(x), Buf(h), Buf(fa), Buf(fb)
    warr = (ctypes.c_void_p * 3)(*[b.ptr for b in dm])
    holed = (ctypes.c_void_p * 3)(dm[0].ptr, None, dm[2].ptr)
    wp, xu, oa, ob = Buf(shape=(int(lib.dpn_enc_pack_bytes(3)) // 4,)), Buf(shape=(batch * T, 3 * C)), Buf(shape=(batch, 256)), Buf(shape=(batch, 192))

    def full():
        p = L.DpnEncPrep()
        p.n_mats, p.weights, p.packed, p.batch = 3, ctypes.cast(warr, ctypes.c_void_p), wp.ptr, batch
        p.x, p.T, p.C, p.xu = dx.ptr, T, C, xu.ptr
        p.h, p.freqs_a, p.n_a, p.out_a, p.freqs_b, p.n_b, p.out_b = dh.ptr, dfa.ptr, 128, oa.ptr, dfb.ptr, 96, ob.ptr
        return p
    muts = [('n_mats', -1), ('n_mats', 33), ('weights', None), ('packed', None), ('weights', ctypes.cast(holed, ctypes.c_void_p)), ('x', None), ('xu', None),
            ('T', 0), ('C', 0), ('batch', 0), ('freqs_a', None), ('out_a', None), ('n_a', 0), ('n_b', -1), ('freqs_b', None), ('out_b', None)]
    for k, v in muts:
        p = full()
        setattr(p, k, v)
        assert lib.dpn_enc_prep(ctypes.byref(p), None) == -1, (k, v)
    assert lib.dpn_enc_prep(ctypes.byref(L.DpnEncPrep()), None) == -1 and lib.dpn_enc_prep(None, None) == -1       # nothing to do is an error too
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (wp, xu, oa, ob))


# ---------------------------------------------------------------------------------------------- summary
def test_zz_summary_of_error_to_bound_ratios():
    """Printed for the reviewer: how much room each derived bound leaves (a ratio far below 1 is expected of worst-case bounds and no reason to
    tighten them), and the measured yardsticks (of the tests above that ran in this process)."""
    print()
    for k in sorted(RATIOS):
        print('largest error / bound   %-28s %.4f' % (k, RATIOS[k]))
        assert RATIOS[k] <= 1.0
    for k in sorted(YARDS):
        print('yardstick (torch fp32 against fp64, CPU, same inputs)   %-10s %.3f' % (k, YARDS[k]))
