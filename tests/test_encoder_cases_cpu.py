"""CPU: the references and pass conditions of tests/encoder_cases.py, before any GPU sees them.
  * split22 is the split the header describes, within the error model gemm_bound() is derived from;
  * the fp64 stage references compose to the reference's layer expression and to torch.autograd.grad of it (1e-12 relative);
  * a numpy emulation of the kernels' arithmetic stays inside every condition on every case of the tables, bit for bit where the condition is
    equality -- the reference within its own condition;
  * the conditions have teeth: six wrong kernels / references are caught in every case they affect;
  * the tables hold what they claim, and the replica-rule rows straddle what the host functions return."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_cases as E

_W = {}


def _weights(okind):
    k = E.WEIGHT_KIND[okind]
    if k not in _W:
        _W[k] = E.weights(k)
    return _W[k]


def _bad(outs, st, names):
    """{output: number of violating elements} over the launch's outputs (all of them must have a stage)."""
    assert sorted(names) == sorted(st), (sorted(names), sorted(st))
    return {n: E.violations(outs[n], st[n])[0] for n in names}


# ---------------------------------------------------------------------------------------------- the split
def test_split22_is_within_its_error_model_and_recombines_exactly():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4096, 256)).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.0
    x[1, 5] = 3.25
    x[2] *= np.float32(2.0 ** 46)
    x[3] *= np.float32(2.0 ** -60)
    s = E.split22(x)
    scaled = x.astype(np.float64) * s.sc.astype(np.float64)[:, None]
    m = np.abs(scaled).max(axis=1)
    assert np.all((m[2:] >= 8) & (m[2:] < 16)) and m[0] == 0 and 8 <= m[1] < 16
    rec = s.hi.astype(np.float64) + s.lo.astype(np.float64) / 2048.0
    assert np.array_equal(rec.astype(np.float32).astype(np.float64), rec)              # <= 24 significant bits: the kernel's fmaf is exact
    err = np.abs(rec - scaled)
    assert np.all(err <= 2.0 ** -22 * np.abs(scaled) + E.ABS_SPLIT)                      # the model gemm_bound() uses
    big = np.abs(scaled) >= 2.0 ** -14
    assert np.all(err[big] <= 2.0 ** -23 * np.abs(scaled[big])) and np.all(err[~big] <= E.ABS_SPLIT)
    assert np.array_equal(s.recombined().astype(np.float64), rec * s.inv.astype(np.float64)[:, None])
    # power-of-two row factors commute with the split
    f = E.row_factors(4096, E.M_EXPONENTS)
    s2 = E.split22(x * f[:, None])
    keep = np.arange(4096) != 3                                                          # (2^-60 2^-100 is below fp32's range)
    assert np.array_equal(s2.hi[keep], s.hi[keep]) and np.array_equal(s2.lo[keep], s.lo[keep])
    # a shared maximum (the q / k / v backward) is the maximum of the concatenation
    a, b = x[:64], x[64:128] * np.float32(40.0)
    both = E.split22(np.concatenate([a, b], axis=1))
    alone = E.split22(a, extra_max=np.abs(b).max(axis=1))
    assert np.array_equal(both.hi[:, :256], alone.hi) and np.array_equal(both.inv, alone.inv)


def test_weight_status_threshold_model():
    hi, _ = E.split_w(np.array([[32767.5, 32768.0]], np.float32))
    assert np.isfinite(hi.astype(np.float32)).all()                                      # f16 holds both; the flag is the kernel's |w| >= 32768 test


# ---------------------------------------------------------------------------------------------- composition
def _layer64(rows, nxt, seed):
    """The reference's layer expression in torch fp64 (F.linear, scaled_dot_product_attention, LayerNorm, exact gelu) on kind C operands, with
    every intermediate the launches write."""
    mats, vec = _weights('C')
    W = {n: torch.tensor(mats[E.SLOT[n]], dtype=torch.float64) for n in E.MAT_NAMES}
    v = {n: torch.tensor(a, dtype=torch.float64, requires_grad=True) for n, a in vec.items()}
    g = torch.Generator().manual_seed(seed)
    t = {'xin': torch.randn(rows, 256, generator=g, dtype=torch.float64).requires_grad_()}
    t['y0'], t['y1'], t['y2'] = (F.linear(t['xin'], W[n], v['bn%d' % i]) for i, n in enumerate('qkv'))
    sh = lambda a: a.view(1, rows, 8, 32).transpose(1, 2)
    t['o'] = F.scaled_dot_product_attention(sh(t['y0']), sh(t['y1']), sh(t['y2'])).transpose(1, 2).reshape(rows, 256)
    t['v1'] = t['xin'] + F.linear(t['o'], W['o'], v['bo'])
    t['x1'] = F.layer_norm(t['v1'], (256,), v['g1'], v['be1'], 1e-5)
    t['pre'] = F.linear(t['x1'], W['c1'], v['bc1'])
    t['act'] = F.gelu(t['pre'])
    t['v2'] = t['x1'] + F.linear(t['act'], W['c2'], v['bc2'])
    t['x2'] = F.layer_norm(t['v2'], (256,), v['g2'], v['be2'], 1e-5)
    if nxt == 1:
        t['n0'], t['n1'], t['n2'] = (F.linear(t['x2'], W[n], v['bn%d' % i]) for i, n in enumerate('qkv'))
    elif nxt == 2:
        t['xf'] = F.layer_norm(t['x2'], (256,), v['gf'], v['bef'], 1e-5)
        t['n0'] = F.linear(t['xf'], W['p'], v['bn0'])
    return t, W, v, mats, vec


def _close(a, b, what, floor=1e-300):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), floor), (what, np.abs(a - b).max(), np.abs(b).max())


def _xhat_rstd(v):
    d = v - v.mean(axis=1, keepdims=True)
    r = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + E.EPS)
    return d * r, r[:, 0]


@pytest.mark.parametrize('rows', [17, 33])
@pytest.mark.parametrize('nxt', [0, 1, 2])
def test_forward_stage_references_compose_to_the_layer_expression(rows, nxt):
    t, W, v, mats, vec = _layer64(rows, nxt, 5)
    n = {k: a.detach().numpy() for k, a in t.items()}
    st, _ = E.fwd_reference('first', {'xin': n['xin']}, {}, mats, vec)
    for i in range(3):
        _close(st['y%d' % i].ref, n['y%d' % i], 'first y%d' % i)
    kind = 'tail_next%d' % nxt
    # every stage reads the upstream tensor of the fp64 expression itself: what the stages compute, composed
    gpu = {k: n[k] for k in ('x1', 'pre', 'act', 'x2')}
    if nxt == 2:
        gpu['xf'] = n['xf']
    st, _ = E.fwd_reference(kind, {'o': n['o'], 'x': n['xin']}, gpu, mats, vec)
    assert sorted(st) == sorted(E.outputs_of('fwd', kind))
    for k in ('x1', 'pre', 'act', 'x2'):
        _close(st[k].ref, n[k], k)
    for k, src in (('1', 'v1'), ('2', 'v2')):
        xh, r = _xhat_rstd(n[src])
        _close(st['xhat' + k].ref, xh, 'xhat' + k)
        _close(st['rstd' + k].ref, r, 'rstd' + k)
    if nxt == 1:
        for i in range(3):
            _close(st['y%d' % i].ref, n['n%d' % i], 'next y%d' % i)
    if nxt == 2:
        xh, r = _xhat_rstd(n['x2'])
        _close(st['xf'].ref, n['xf'], 'xf'), _close(st['xhatf'].ref, xh, 'xhatf'), _close(st['rstdf'].ref, r, 'rstdf'), _close(st['y0'].ref, n['n0'], 'y0')


@pytest.mark.parametrize('rows', [17, 33])
@pytest.mark.parametrize('row_tiles', [1, 2])
@pytest.mark.parametrize('kind', E.BWD_KINDS, ids=lambda k: 'head%d_body%d' % k)
def test_backward_stage_references_compose_to_autograd(kind, row_tiles, rows):
    head, body = kind
    t, W, v, mats, vec = _layer64(rows, {0: 0, 1: 1, 2: 2}[head] if body else 1, 6)
    g = torch.Generator().manual_seed(7)
    rnd = lambda: torch.randn(rows, 256, generator=g, dtype=torch.float64)
    n = {k: a.detach().numpy() for k, a in t.items()}
    if not body:                                 # the first layer's q / k / v backward: gx = d loss / d xin
        res, dq, dk, dv = rnd(), rnd(), rnd(), rnd()
        loss = (res * t['xin']).sum() + (dq * t['y0']).sum() + (dk * t['y1']).sum() + (dv * t['y2']).sum()
        gx, = torch.autograd.grad(loss, [t['xin']])
        st, _ = E.bwd_reference(kind, {'res': res.numpy(), 'dq': dq.numpy(), 'dk': dk.numpy(), 'dv': dv.numpy()}, {}, mats, vec, row_tiles)
        _close(st['gx'].ref, gx.numpy(), 'gx')
        return
    ins = {}
    if head == 0:
        gin = rnd()
        loss = (gin * t['x2']).sum()
        ins['gin'] = gin.numpy()
    elif head == 1:
        res, dq, dk, dv = rnd(), rnd(), rnd(), rnd()
        loss = (res * t['x2']).sum() + (dq * t['n0']).sum() + (dk * t['n1']).sum() + (dv * t['n2']).sum()
        ins.update(res=res.numpy(), dq=dq.numpy(), dk=dk.numpy(), dv=dv.numpy())
    else:
        dmeta = rnd()
        loss = (dmeta * t['n0']).sum()
        ins['dmeta'] = dmeta.numpy()
        ins['xhatf'], ins['rstdf'] = _xhat_rstd(n['x2'])
    ins['xhat2'], ins['rstd2'] = _xhat_rstd(n['v2'])
    ins['xhat1'], ins['rstd1'] = _xhat_rstd(n['v1'])
    ins['pre'] = n['pre']
    pairs = [('partial2', 'g2', 'be2'), ('partial1', 'g1', 'be1')] + ([('partial_f', 'gf', 'bef')] if head == 2 else [])
    params = [v[n] for _, gn, bn in pairs for n in (gn, bn)]
    want = [a.numpy() for a in torch.autograd.grad(loss, [t['v2'], t['pre'], t['v1'], t['o']] + params)]
    gs2, dpre, gs1, dout = want[:4]
    st, _ = E.bwd_reference(kind, ins, {'gs2': gs2, 'dpre': dpre, 'gs1': gs1}, mats, vec, row_tiles)
    assert sorted(st) == sorted(E.outputs_of('bwd', kind))
    _close(st['gs2'].ref, gs2, 'gs2'), _close(st['dpre'].ref, dpre, 'dpre'), _close(st['gs1'].ref, gs1, 'gs1'), _close(st['dout'].ref, dout, 'dout')
    # the LayerNorm parameter gradients are the sums of the per-workgroup partial sums: ceil(rows / (16 row_tiles)) blocks
    for i, (pn, _, _) in enumerate(pairs):
        assert st[pn].ref.shape == ((rows + 16 * row_tiles - 1) // (16 * row_tiles), 512)
        _close(st[pn].ref[:, :256].sum(axis=0), want[4 + 2 * i], pn + ' dgamma')
        _close(st[pn].ref[:, 256:].sum(axis=0), want[5 + 2 * i], pn + ' dbeta')


@pytest.mark.parametrize('L,batch', [(1, 1), (17, 2), (33, 3), (288, 1)])
def test_attention_references_are_fp64_autograd_of_sdpa(L, batch):
    q, k, v, go = (torch.tensor(a, dtype=torch.float64) for a in E.attn_inputs(L, batch))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    sh = lambda a: a.view(batch, L, 8, 32).transpose(1, 2)
    o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v)).transpose(1, 2).reshape(batch * L, 256)
    dq, dk, dv = torch.autograd.grad((o * go).sum(), [q, k, v])
    n = lambda a: a.detach().numpy()
    s64, P64, out64 = E.attn_forward64(n(q), n(k), n(v), L, batch)
    _close(out64, n(o), 'out')
    _close(P64.sum(axis=-1), np.ones((batch, 8, L)), 'P rows')
    st = E.attn_backward64(n(q), n(k), n(v), out64, P64, n(go), L, batch)
    # (one key: dq and dk are mathematically zero, rounding noise on both sides -- measured against the size of dv there)
    floor = float(np.abs(n(dv)).max())
    _close(st['dq'].ref, n(dq), 'dq', floor), _close(st['dk'].ref, n(dk), 'dk', floor), _close(st['dv'].ref, n(dv), 'dv')


# ---------------------------------------------------------------------------------------------- the emulation inside every condition
FWD_GROUPS = [(k, rt, o) for k in E.FWD_KINDS for rt in (1, 2) for o in E.OPERAND_KINDS]
BWD_GROUPS = [(k, rt, o) for k in E.BWD_KINDS for rt in (1, 2) for o in E.OPERAND_KINDS]
_ID = lambda g: '%s-rt%d-%s' % (g[0] if isinstance(g[0], str) else 'head%d_body%d' % g[0], g[1], g[2])


def _rows_of_group(cases, group):
    return [c[2] for c in cases if (c[0], c[1], c[3]) == group]


@pytest.mark.parametrize('group', FWD_GROUPS, ids=_ID)
def test_forward_emulation_is_inside_every_condition(group):
    kind, rt, okind = group
    mats, vec = _weights(okind)
    for rows in _rows_of_group(E.fwd_cases(), group):
        ins = E.fwd_inputs(kind, rows, okind)
        outs = E.emulate_fwd(kind, ins, mats, vec)
        st, _ = E.fwd_reference(kind, ins, outs, mats, vec)
        bad = _bad(outs, st, E.outputs_of('fwd', kind))
        assert not any(bad.values()), (rows, bad)
        assert all(st[n].exact is not None for n in E.exact_outputs('fwd', kind, okind)), rows


@pytest.mark.parametrize('group', BWD_GROUPS, ids=_ID)
def test_backward_emulation_is_inside_every_condition(group):
    kind, rt, okind = group
    mats, vec = _weights(okind)
    for rows in _rows_of_group(E.bwd_cases(), group):
        ins = E.bwd_inputs(kind, rows, okind)
        outs = E.emulate_bwd(kind, ins, mats, vec, rt)
        st, _ = E.bwd_reference(kind, ins, outs, mats, vec, rt)
        bad = _bad(outs, st, E.outputs_of('bwd', kind))
        assert not any(bad.values()), (rows, bad)
        assert all(st[n].exact is not None for n in E.exact_outputs('bwd', kind, okind)), rows


# ---------------------------------------------------------------------------------------------- teeth
def _caught(outs, st):
    return any(E.violations(outs[n], st[n])[0] for n in st)


@pytest.mark.parametrize('alter,okinds', [('no_hi_lo', ('AL', 'C', 'MC')), ('no_lo_hi', ('S', 'C', 'MS', 'MC')), ('w_for_wt', E.OPERAND_KINDS),
                                           ('slot_plus_1', E.OPERAND_KINDS)])
def test_wrong_gemm_arithmetic_is_caught_in_every_case_it_affects(alter, okinds):
    """Dropping hi.lo' needs a weight with a lo' plane (kinds AL and C), dropping lo'.hi an activation with one (everything but integers).
    The K = 768 reduction of the q / k / v backward is the one place where kind C's worst-case bound, (K + 16) 2^-24 |X||B|, is wider than
    a dropped lo' plane (2^-12 per product with random signs): there the bit-exact kinds AL (weights) and S / MS (activations) catch it."""
    wide_k = alter in ('no_hi_lo', 'no_lo_hi')
    for okind in okinds:
        mats, vec = _weights(okind)
        for kind in E.FWD_KINDS:
            for rows in (1, 17, 33):
                ins = E.fwd_inputs(kind, rows, okind)
                outs = E.emulate_fwd(kind, ins, mats, vec, alter)
                assert _caught(outs, E.fwd_reference(kind, ins, outs, mats, vec)[0]), (alter, okind, kind, rows)
        for kind in E.BWD_KINDS:
            if wide_k and kind[0] == 1 and okind in ('C', 'MC'):
                continue
            for rows in (1, 17, 33):
                ins = E.bwd_inputs(kind, rows, okind)
                outs = E.emulate_bwd(kind, ins, mats, vec, 1, alter)
                assert _caught(outs, E.bwd_reference(kind, ins, outs, mats, vec, 1)[0]), (alter, okind, kind, rows)


def test_a_padding_row_in_a_layernorm_partial_sum_is_caught():
    """One padding row of ones in the last workgroup's sums.  (Kind M is left out with a reason: beside a 2^100 row a 1.0 is below the rounding
    of the sum, in the kernel and in any reference.)"""
    for okind in ('A', 'AL', 'S', 'C'):
        mats, vec = _weights(okind)
        for kind in ((0, 1), (1, 1), (2, 1)):
            for rt, rows in ((1, 1), (1, 17), (2, 33), (2, 65)):
                ins = E.bwd_inputs(kind, rows, okind)
                outs = E.emulate_bwd(kind, ins, mats, vec, rt, 'pad_row')
                st, _ = E.bwd_reference(kind, ins, outs, mats, vec, rt)
                for n in [n for n in st if n.startswith('partial')]:
                    assert E.violations(outs[n], st[n])[0] > 0, (okind, kind, rows, n)


@pytest.mark.parametrize('batch', E.ATTN_BATCH)
def test_an_attention_reference_with_one_key_too_many_is_caught(batch):
    for L in E.ATTN_L:
        q, k, v, _ = E.attn_inputs(L, batch)
        s64, P64, out64 = E.attn_forward64(q, k, v, L, batch)
        _, Pw, outw = E.attn_forward64(q, k, v, L, batch, n_keys=L + 1)
        for split in (False, True):
            bP, bo = E.attn_forward_bounds(q, k, v, L, batch, s64, P64, split, 2.0)
            assert np.any(np.abs(Pw[..., :L] - P64) > bP), (L, split)
            assert np.any(np.abs(outw - out64) > bo), (L, split)


# ---------------------------------------------------------------------------------------------- the tables
def test_tables_hold_every_kind_at_every_row_count():
    f, b = E.fwd_cases(), E.bwd_cases()
    for rt in (1, 2):
        for rows in E.rows_table(rt):
            for o in E.OPERAND_KINDS:
                assert all((k, rt, rows, o) in f for k in E.FWD_KINDS) and all((k, rt, rows, o) in b for k in E.BWD_KINDS)
    assert all((k, 2, E.ROWS_BIG, 'A') in f for k in E.FWD_KINDS) and all((k, 2, E.ROWS_BIG, 'A') in b for k in E.BWD_KINDS)
    assert len(f) == len(set(f)) == 5 * 12 * 6 + 5 and len(b) == len(set(b)) == 4 * 12 * 6 + 4
    assert len(E.replica_cases()) == 2 * 4 * 2 + 4 * 2
    print('forward: %d cases (%d launch kinds x %d row counts x %d operand kinds + %d at %d rows); backward: %d cases; replica edges: %d'
          % (len(f), len(E.FWD_KINDS), 12, len(E.OPERAND_KINDS), 5, E.ROWS_BIG, len(b), len(E.replica_cases())))
    # row counts: one padded block, an exact block, a block of one row behind it, more than two blocks, one field
    assert set(E.ROWS_RT1) >= {1, 16, 17, 287} and set(E.ROWS_RT2) >= {1, 32, 33, 287}
    assert sorted({E.SLOT[n] for n in E.MAT_NAMES}) != list(range(7)) and E.N_MATS >= 9
    assert [E.SLOT[n] for n in E.MAT_NAMES] != sorted(E.SLOT[n] for n in E.MAT_NAMES)
    mats, _ = E.weights('S')
    for i, m in enumerate(mats):
        assert not np.array_equal(m, m.T) and all(not np.array_equal(m, o) for o in mats[:i])
        assert ((m != 0).sum(axis=0) == 1).all() and ((m != 0).sum(axis=1) == 1).all()
    f16 = E.row_factors(16, E.M_EXPONENTS)
    assert len(set(f16.tolist())) == len(E.M_EXPONENTS)                                    # all five magnitudes inside one 16-row block


def test_replica_rows_straddle_what_the_host_functions_return():
    from deepphysinet_amd import _lib
    lib = _lib.load()
    for fn in (lib.dpn_enc_fwd_replicas, lib.dpn_enc_bwd_replicas):
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 4
    seen = set()
    for direction, kind, rows, expect, _ in E.replica_cases():
        if direction == 'fwd':
            got = lib.dpn_enc_fwd_replicas(rows, 1, int(kind.startswith('tail')), 1)
        else:
            got = lib.dpn_enc_bwd_replicas(rows, 1, kind[0], kind[1])
        assert got == expect, (direction, kind, rows, got)
        seen.add((direction, got))
    assert seen == {('fwd', 3), ('fwd', 1), ('bwd', 2), ('bwd', 1)}
    # the edges sit where the rule changes: the helpers go at 1025 rows, the replicas at 1361 (forward) and 2049 (backward)
    assert lib.dpn_enc_fwd_replicas(1360, 1, 1, 1) == 3 and lib.dpn_enc_fwd_replicas(1361, 1, 1, 1) == 1
    assert lib.dpn_enc_bwd_replicas(2048, 1, 1, 0) == 2 and lib.dpn_enc_bwd_replicas(2049, 1, 1, 0) == 1


# ---------------------------------------------------------------------------------------------- dpn_wgrad16, dpn_enc_prep
@pytest.mark.parametrize('rows', E.WGRAD_ROWS)
def test_wgrad_emulation_is_inside_its_conditions_and_a_dropped_plane_is_not(rows):
    for kind in ('A', 'C', 'M'):
        for slices in E.WGRAD_SLICES:
            for g, x, _ in E.wgrad_inputs(rows, kind)[:2 if kind != 'A' else 5]:
                st, sb = E.wgrad_stage(g, x, slices)
                assert (st.exact is not None) == (kind == 'A')
                assert E.violations(E.emulate_wgrad(g, x, slices), st)[0] == 0, (rows, kind, slices)
                assert E.violations(g.astype(np.float64).sum(axis=0).astype(np.float32), sb)[0] == 0
    # teeth: the X lo' plane dropped -- caught wherever the reduction is short enough for the worst-case bound (rows <= 33)
    if rows <= 33:
        g, x, _ = E.wgrad_inputs(rows, 'C')[0]
        assert E.violations(E.emulate_wgrad(g, x, 1, 'no_hi_lo'), E.wgrad_stage(g, x, 1)[0])[0] > 0
    g, x, _ = E.wgrad_inputs(rows, 'M')[0]
    if rows > 2:
        assert np.abs(g).max() / np.abs(g[g != 0]).min() > 2.0 ** 60


def test_im2col_model_wraps():
    for T in E.PREP_T:
        x = np.arange(3 * T * 5, dtype=np.float32).reshape(3 * T, 5)
        out = E.im2col_circ3_model(x, T, 5, 3)
        assert out.shape == (3 * T, 15)
        for b in range(3):
            for t in range(T):
                for tap in range(3):
                    assert np.array_equal(out[b * T + t, tap::3], x[b * T + (t + tap - 1) % T])
