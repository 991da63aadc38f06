"""GPU (MI355X): the exact-fp32 GEMM family -- dpn_sgemm, dpn_sgemm_batch(_jobs), dpn_sgemm_ln, dpn_sum_parts -- through the C ABI against
an fp64 evaluation of its definition, C = epilogue(sum_t op(A_t) op(B_t) + bias), over the whole surface of the ABI: ta / tb, three
leading dimensions, terms of different length, problems of different shape in one launch, the four epilogues, row sums, accumulate,
column-sum jobs, both template instantiations of the batch kernel and every split count of the two-pass split-K.

Pass conditions (tests/gemm_cases.py): integer-valued operands (kind A) and full-mantissa pass-through (kind B) are
torch.equal to the reference; standard normal operands (kind C) are inside (K + 16) 2^-24 |A||B| + 2^-24 |C64|; only the GELU epilogues carry
a measured tolerance, with torch's own fp32 GELU as the yardstick.  Every operand sits inside a larger owned buffer whose guards are NaN
(inputs) or a sentinel bit pattern (outputs): a load outside the logical extent poisons the result, a store outside it changes the sentinel.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

PADS = [pytest.param(True, id='padded'), pytest.param(False, id='tight')]
TTS = [pytest.param(tt, id='ta%d_tb%d' % tt) for tt in G.TT]


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


class _D:
    """A gemm_cases.Buf on the device: the owned buffer and the view of its logical window (whose data_ptr and ld are what the ABI gets)."""

    def __init__(self, buf):
        self.buf = buf
        self.full = torch.from_numpy(buf.full).to(_dev())
        self.view = self.full[G.GUARD_ROWS:G.GUARD_ROWS + buf.rows, :buf.cols]
        self.ld = buf.ld

    def window(self):
        return self.view.cpu()

    def guards_kept(self):
        return G.outside_is_sentinel(self.full.cpu().numpy(), self.buf)


def _d(buf):
    return None if buf is None else _D(buf)


def _v(d):
    return None if d is None else d.view


def _f32(ref64):
    return torch.from_numpy(np.asarray(ref64, np.float64)).to(torch.float32)


def _upload_batch(probs, jobs):
    from deepphysinet_amd.linear import _problem
    dev_probs, structs = [], []
    for q in probs:
        p = q.spec
        e = dict(A=[_D(a) for a in q.A], B=[_D(b) for b in q.B], bias=_d(q.bias), aux=_d(q.aux), C=_D(q.C), aux_out=_d(q.aux_out), asum=_d(q.asum))
        terms = [(e['A'][t].view, e['A'][t].ld, e['B'][t].view, e['B'][t].ld, q.k_term[t]) for t in range(len(p.ks))]
        structs.append(_problem(p.M, p.N, q.K, terms, e['C'].view, e['C'].ld, q.ta, q.tb, bias=_v(e['bias']), asum=_v(e['asum']), epi=p.epi,
                                aux=_v(e['aux']), aux_out=_v(e['aux_out'])))
        dev_probs.append(e)
    dev_jobs = [(_D(j[0]), _D(j[1]), _D(j[2]), j[3]) for j in jobs]
    return dev_probs, structs, dev_jobs


def _run_batch(launch, kind, tt, pad):
    from deepphysinet_amd.linear import _launch
    probs, jobs = G.build_batch(launch, kind, tt, pad)
    dev_probs, structs, dev_jobs = _upload_batch(probs, jobs)
    _launch(structs, [(j[0].view, 0, j[1].view, j[2].view, j[3]) for j in dev_jobs])
    torch.cuda.synchronize()
    return probs, jobs, dev_probs, dev_jobs


def _assert_guards(e, name):
    for k in ('C', 'aux_out', 'asum'):
        if e[k] is not None:
            assert e[k].guards_kept(), '%s: a store outside the logical extent of %s' % (name, k)


def _assert_jobs_exact(jobs, dev_jobs, name):
    for i, (job, dj) in enumerate(zip(jobs, dev_jobs)):
        a, b = G.reference_job(job)
        assert torch.equal(dj[1].window()[0], _f32(a)) and torch.equal(dj[2].window()[0], _f32(b)), (name, 'job', i)
        assert dj[1].guards_kept() and dj[2].guards_kept(), (name, 'job', i)


# ---------------------------------------------------------------------------------------------- dpn_sgemm_batch
@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('name', G.batch_ids('A'))
def test_batch_integer_operands_are_bit_exact(name, tt, pad):
    """Kind A over the whole case table: C, asum and the column-sum jobs torch.equal to fp64, every guard untouched.  A dropped, duplicated or
    mis-indexed k-value, tile, term or problem changes an integer; a load past an extent reads NaN."""
    launch = G.batch_by_name(name)
    probs, jobs, dev_probs, dev_jobs = _run_batch(launch, 'A', tt, pad)
    for i, (q, e) in enumerate(zip(probs, dev_probs)):
        ref = G.reference_problem(q)
        assert torch.equal(e['C'].window(), _f32(ref['C'])), (name, 'problem', i)
        if q.spec.asum:
            assert torch.equal(e['asum'].window()[0], _f32(ref['asum'])), (name, 'asum of problem', i)
        _assert_guards(e, (name, i))
    _assert_jobs_exact(jobs, dev_jobs, name)


def test_batch_dispatch_edge_forms_agree():
    """512 output tiles of one k-tile run <256,1>, 513 run <64,2>: the shared 512 x 1024 problem is the same bits from both (each is
    torch.equal to the reference in test_batch_integer_operands_are_bit_exact; here the two launches get the SAME operands)."""
    from deepphysinet_amd.linear import _launch
    l512, l513 = G.batch_by_name('dispatch_512_tiles'), G.batch_by_name('dispatch_513_tiles')
    assert G.host_form(l512.probs) == '256x1' and G.host_form(l513.probs) == '64x2'
    probs, _ = G.build_batch(l513, 'A', (0, 1), True)
    out = []
    for n in (1, 2):
        dev_probs, structs, _ = _upload_batch(probs[:n], [])
        _launch(structs)
        out.append(dev_probs[0]['C'].window())
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], _f32(G.reference_problem(probs[0])['C']))


@pytest.mark.parametrize('kind', ['B1', 'B2'])
@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('name', G.batch_ids('B1'))
def test_batch_full_mantissa_operands_pass_through_unchanged(name, tt, kind):
    """Kind B: one operand random fp32 with all 24 mantissa bits, the other a selection matrix of powers of two, so every output is ONE exact
    product.  Fails if either operand loses mantissa bits on its way through LDS or the matrix instruction (both instantiations)."""
    launch = G.batch_by_name(name)
    probs, _, dev_probs, _ = _run_batch(launch, kind, tt, True)
    for q, e in zip(probs, dev_probs):
        ref = G.reference_problem(q)
        full = q.A[0].win if kind == 'B1' else q.B[0].win
        assert (full.view(np.uint32) & 0xFFF).any() and (full.view(np.uint32) & 1).any()        # the low mantissa bits are in use
        assert torch.equal(e['C'].window(), _f32(ref['C'])), name
        _assert_guards(e, name)


@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('name', G.batch_ids('C'))
def test_batch_random_operands_have_fp32_class_error(name, tt):
    """Kind C: |C - C64| <= (K_total + 16) 2^-24 (|A||B|) + 2^-24 |C64|, the bound of any summation order of K products with one rounding each
    (test_gemm_cases_cpu shows that bfloat16 operands leave it at these shapes)."""
    launch = G.batch_by_name(name)
    probs, _, dev_probs, _ = _run_batch(launch, 'C', tt, True)
    for i, (q, e) in enumerate(zip(probs, dev_probs)):
        ref, kt = G.reference_problem(q), sum(q.spec.ks)
        err = np.abs(e['C'].window().numpy().astype(np.float64) - ref['C'])
        bound = G.kind_c_bound(kt, ref['absprod'], ref['C'])
        print('%s problem %d: worst error / bound = %.3f' % (name, i, float((err / bound).max())))
        assert (err <= bound).all(), (name, i, float((err / bound).max()))
        if q.spec.asum:
            a = np.abs(G.op_read(q.A[0], q.spec.M, kt, q.ta).astype(np.float64)).sum(1)
            assert (np.abs(e['asum'].window()[0].numpy().astype(np.float64) - ref['asum']) <= (kt + 16) * G.U * a).all(), (name, i)
        _assert_guards(e, (name, i))


@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('name', G.batch_ids('G'))
def test_batch_gelu_epilogues_against_fp64_with_torch_as_yardstick(name, tt):
    """DPN_EPI_GELU (with and without aux_out) and DPN_EPI_MUL_GELU_GRAD on exact integer pre-activations |v| <= 6, aux in [-6, 6], ldc > N.
    erff / expf are not exact, so this is the one measured tolerance: the kernel's maximum absolute error against fp64 may be at most 4 x the
    error of torch's own fp32 F.gelu / its autograd derivative on the device on the same inputs, floored at 4 * 2^-24 (the kernel uses torch's
    formulas; a different libm rounding is allowed for).  aux_out is the exact pre-activation, bit for bit.
    Measured on MI355X, maxima over all cases: gelu(v): torch 1.537e-07, kernel 1.537e-07; v * gelu'(aux): torch 4.900e-07, kernel
    4.900e-07 (in every case the kernel's maximum is torch's own)."""
    import torch.nn.functional as F
    launch = G.batch_by_name(name)
    probs, _, dev_probs, _ = _run_batch(launch, 'G', tt, True)
    for i, (q, e) in enumerate(zip(probs, dev_probs)):
        ref = G.reference_problem(q)
        v = _f32(ref['v']).to(_dev())
        if q.spec.epi == G.EPI_GELU:
            yard = F.gelu(v)
        else:
            aux = e['aux'].view.clone().requires_grad_(True)
            F.gelu(aux).backward(v)
            yard = aux.grad
        err_torch = float(np.abs(yard.cpu().numpy().astype(np.float64) - ref['C']).max())
        err_kernel = float(np.abs(e['C'].window().numpy().astype(np.float64) - ref['C']).max())
        print('%s problem %d epi %d: max abs error torch %.3e kernel %.3e' % (name, i, q.spec.epi, err_torch, err_kernel))
        assert err_kernel <= max(4.0 * err_torch, 4.0 * G.U), (name, i, err_torch, err_kernel)
        if q.spec.aux_out:
            assert torch.equal(e['aux_out'].window(), _f32(ref['v'])), (name, i)
        _assert_guards(e, (name, i))


# ---------------------------------------------------------------------------------------------- dpn_sgemm
_WS_GUARD, _WS_FILL = 4096, 0xA5


def _run_sgemm(s, kind, tt, pad, d=None):
    from deepphysinet_amd import _lib as L
    d = G.build_sgemm(s, kind, tt, pad) if d is None else d
    e = {k: _d(d[k]) for k in ('A', 'B', 'bias', 'C', 'asum')}
    has_ws, ws_bytes, splits, kps = G.sgemm_workspace(s)
    ws = torch.full((ws_bytes + _WS_GUARD,), _WS_FILL, dtype=torch.uint8, device=_dev()) if has_ws else None
    p = lambda x: None if x is None else x.view.data_ptr()
    L.check(L.load().dpn_sgemm(tt[0], tt[1], s.M, s.N, s.K, p(e['A']), e['A'].ld, p(e['B']), e['B'].ld, p(e['C']), e['C'].ld, p(e['bias']), p(e['asum']),
                               s.accumulate, ws.data_ptr() if has_ws else None, ws_bytes, torch.cuda.current_stream().cuda_stream), 'dpn_sgemm')
    torch.cuda.synchronize()
    return d, e, ws, (has_ws, ws_bytes, splits, kps)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('s', G.SGEMM, ids=lambda s: s.name)
def test_sgemm_integer_operands_are_bit_exact_at_every_split_count(s, tt, pad):
    """dpn_sgemm, kind A: a single pass without a workspace (K = 1 .. 1030, with and without accumulate), the split path (K >= 1024 and fewer
    than 256 tiles) with bias, asum and accumulate together, a workspace sized for exactly the wanted split count, one byte less (fewer
    splits), zero bytes behind a non-null pointer (one split), and K = 1023 / 256 tiles just outside the split condition: all torch.equal to
    fp64.  The workspace shows the split count the host chose: splits * (M N + M) floats written when it splits, none otherwise, and never a
    byte past the size it was given."""
    d, e, ws, (has_ws, ws_bytes, splits, kps) = _run_sgemm(s, 'A', tt, pad)
    ref = G.reference_sgemm(s, tt, d)
    assert torch.equal(e['C'].window(), _f32(ref['C'])), s.name
    assert e['C'].guards_kept()
    if s.asum:
        assert torch.equal(e['asum'].window()[0], _f32(ref['asum'])) and e['asum'].guards_kept(), s.name
    if has_ws:
        w = ws.cpu().numpy()
        used = G.sgemm_ws_bytes(s.M, s.N, splits) if splits > 1 else 0
        if splits > 1 and not s.asum:
            used = splits * s.M * s.N * 4
        assert used <= ws_bytes and (w[used:] == _WS_FILL).all(), (s.name, 'workspace written past the %d bytes of %d splits' % (used, splits))
        if splits > 1:                       # integer partial sums never have the fill pattern's bits
            assert (w[:used].view(np.uint32) != 0xA5A5A5A5).all(), (s.name, 'fewer than %d splits were written' % splits)


@pytest.mark.parametrize('tt', TTS)
@pytest.mark.parametrize('s', G.SGEMM_KIND_C, ids=lambda s: s.name)
def test_sgemm_random_operands_have_fp32_class_error(s, tt):
    d, e, _, _ = _run_sgemm(s, 'C', tt, True)
    ref = G.reference_sgemm(s, tt, d)
    err = np.abs(e['C'].window().numpy().astype(np.float64) - ref['C'])
    bound = G.kind_c_bound(s.K, ref['absprod'], ref['C'])
    assert (err <= bound).all(), (s.name, float((err / bound).max()))
    assert (np.abs(e['asum'].window()[0].numpy().astype(np.float64) - ref['asum']) <= (s.K + 16) * G.U * ref['asum_abs']).all()
    assert e['C'].guards_kept() and e['asum'].guards_kept()


@pytest.mark.parametrize('s', [G.S(33, 17, 1030, ws=None), G.S(159, 256, 7215, accumulate=1, ws='exact')], ids=lambda s: s.name)
def test_sgemm_is_deterministic_on_random_operands(s):
    d = G.build_sgemm(s, 'C', (1, 0), True)
    runs = [_run_sgemm(s, 'C', (1, 0), True, d)[1] for _ in range(2)]
    assert torch.equal(runs[0]['C'].full, runs[1]['C'].full) and torch.equal(runs[0]['asum'].full, runs[1]['asum'].full)
    assert not torch.isnan(runs[0]['C'].window()).any()


# ---------------------------------------------------------------------------------------------- dpn_sgemm_ln
@pytest.mark.parametrize('tb', [0, 1])
@pytest.mark.parametrize('N', G.LN_N)
@pytest.mark.parametrize('M', G.LN_M)
@pytest.mark.parametrize('mode', [1, 2])
def test_sgemm_ln_both_modes_against_fp64(mode, M, N, tb):
    """dpn_sgemm_ln at ragged M and N with ldb / ldc padding against fp64, at the tolerances of test_layernorm_folded_into_gemm_both_modes
    taken against the fp64 values; rows >= M of y, xhat, rstd and partial keep the sentinel and the last row block of partial sums only the
    rows that exist (the rows after them are NaN)."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.linear import _launch_ln
    d = G.build_ln(mode, M, N, tb, True)
    e = {k: _D(b) for k, b in d.items()}
    if mode == 1:
        _launch_ln(1, M, N, e['x'].view, e['r'].view, e['gamma'].view, e['beta'].view, None, e['y'].view, e['xhat'].view, e['rstd'].view, None,
                   e['B'].view, tb, e['B'].ld, e['C'].view, e['C'].ld, bias=e['bias'].view, epi=L.EPI_GELU, aux_out=e['pre'].view)
    else:
        _launch_ln(2, M, N, e['x'].view, e['r'].view, e['gamma'].view, None, e['rstd_in'].view, e['y'].view, None, None, e['partial'].view,
                   e['B'].view, tb, e['B'].ld, e['C'].view, e['C'].ld, bias=e['bias'].view)
    torch.cuda.synchronize()
    ref = G.reference_ln(mode, M, N, tb, d)
    for k, (rtol, atol) in G.LN_TOL[mode].items():
        got = e[k].window().numpy()
        assert G.within(got, ref[k], rtol, atol), (k, float(np.abs(got - ref[k]).max()))
        assert e[k].guards_kept(), k


# ---------------------------------------------------------------------------------------------- dpn_sum_parts
@pytest.mark.parametrize('zero_tail', [0, 1, 300])
@pytest.mark.parametrize('count', [1, 255, 256, 257])
@pytest.mark.parametrize('n_parts', [1, 2, 16])
def test_sum_parts_sums_zeroes_the_tail_and_writes_nothing_else(n_parts, count, zero_tail):
    from deepphysinet_amd import _lib as L
    rng = np.random.default_rng([n_parts, count, zero_tail])
    parts = _D(G.input_buf(rng.integers(-4, 5, size=(n_parts, count)).astype(np.float32), False))
    out = _D(G.output_buf(1, count + zero_tail, True))
    L.check(L.load().dpn_sum_parts(parts.view.data_ptr(), n_parts, count, zero_tail, out.view.data_ptr(), torch.cuda.current_stream().cuda_stream),
            'dpn_sum_parts')
    got = out.window()[0]
    assert torch.equal(got[:count], _f32(parts.buf.win.astype(np.float64).sum(0)))
    assert torch.equal(got[count:], torch.zeros(zero_tail)) and out.guards_kept()


# ---------------------------------------------------------------------------------------------- linear / linear_multi
def _ints(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-4, 5, size=shape).astype(np.float32))


def _linear_vs_fp64(x, ws, bs, seed):
    """linear / linear_multi on integer-valued tensors: outputs and all gradients torch.equal to fp64 autograd cast to fp32."""
    import torch.nn.functional as F
    from deepphysinet_amd.linear import linear, linear_multi
    gys = [_ints((x.shape[0], w.shape[0]), seed + 10 + i) for i, w in enumerate(ws)]
    leaves64 = [t.double().requires_grad_(True) for t in [x] + ws + bs]
    x64, w64, b64 = leaves64[0], leaves64[1:1 + len(ws)], leaves64[1 + len(ws):]
    y64 = [F.linear(x64, w, b) for w, b in zip(w64, b64)]
    torch.autograd.backward(y64, [g.double() for g in gys])
    leaves = [t.to(_dev()).requires_grad_(True) for t in [x] + ws + bs]
    xd, wd, bd = leaves[0], leaves[1:1 + len(ws)], leaves[1 + len(ws):]
    ys = [linear(xd, wd[0], bd[0])] if len(ws) == 1 else list(linear_multi(xd, wd, bd))
    torch.autograd.backward(ys, [g.to(_dev()) for g in gys])
    for y, r in zip(ys, y64):
        assert r.detach().abs().max() < 2 ** 24 and torch.equal(y.detach().cpu(), r.detach().float())
    for i, (t, r) in enumerate(zip(leaves, leaves64)):
        assert r.grad.abs().max() < 2 ** 24 and torch.equal(t.grad.cpu(), r.grad.float()), 'gradient of leaf %d' % i


def test_linear_forward_split_k_route_is_exact():
    from deepphysinet_amd.linear import _long_k
    assert _long_k(33, 17, 1030)
    _linear_vs_fp64(_ints((33, 1030), 1), [_ints((17, 1030), 2)], [_ints((17,), 3)], 100)


def test_linear_input_gradient_split_k_route_is_exact():
    from deepphysinet_amd.linear import _long_k
    assert _long_k(33, 40, 1056) and not _long_k(33, 1056, 40)
    _linear_vs_fp64(_ints((33, 40), 4), [_ints((1056, 40), 5)], [_ints((1056,), 6)], 200)


def test_linear_row_sliced_weight_gradient_route_is_exact(monkeypatch):
    """n = 1100 >= 1024 rows: encoder_ops._wgrad cuts the reduction into S = min(16, ceil(n / 1024)) = 2 slices of 550 rows, which run as two
    problems of one launch, and joins them with dpn_sum_parts.  The launches are recorded, so a moved threshold cannot turn this into a test
    of the unsliced route."""
    import deepphysinet_amd.linear as lin
    n, N, K = 1100, 24, 40
    S = min(16, (n + 1023) // 1024)
    rows = (n + S - 1) // S
    assert n >= 1024 and (S, rows) == (2, 550)
    launched, launch = [], lin._launch

    def recording(problems, *a, **kw):
        launched.append([(q.M, q.N, q.K, q.ta, q.tb) for q in problems])
        return launch(problems, *a, **kw)

    monkeypatch.setattr(lin, '_launch', recording)
    _linear_vs_fp64(_ints((n, K), 7), [_ints((N, K), 8)], [_ints((N,), 9)], 300)
    assert [(N, K, rows, 1, 0)] * S in launched, launched


def test_linear_multi_three_weights_is_exact():
    _linear_vs_fp64(_ints((33, 40), 10), [_ints((24, 40), 11 + i) for i in range(3)], [_ints((24,), 14 + i) for i in range(3)], 400)


# ---------------------------------------------------------------------------------------------- refusals
def _small_problem(**kw):
    """A valid 3 x 5 x 4 problem on sentinel-filled outputs; kw overrides fields of the DpnGemmProblem afterwards."""
    from deepphysinet_amd.linear import _problem
    dev = _dev()
    t = dict(A=torch.ones(3, 4, device=dev), B=torch.ones(4, 5, device=dev), aux=torch.ones(3, 5, device=dev),
             C=torch.full((3, 5), float(G.SENTINEL), device=dev), asum=torch.full((3,), float(G.SENTINEL), device=dev))
    nterms = kw.pop('nterms', 1)
    q = _problem(3, 5, 4, [(t['A'], 4, t['B'], 5)] * nterms, t['C'], 5, 0, 0, asum=t['asum'] if kw.pop('with_asum', False) else None,
                 epi=kw.pop('epi', 0), aux=t['aux'] if kw.pop('with_aux', False) else None)
    for k, v in kw.items():
        if k in ('A', 'B', 'k_term'):
            getattr(q, k)[0] = v
        else:
            setattr(q, k, v)
    return q, t


def _untouched(t):
    return bool((t.cpu().numpy().view(np.uint32) == G.SENTINEL_BITS).all())


def _thirteen_terms():
    made = [_small_problem(nterms=12)]
    made[0][0].nterms = 13                  # a DpnGemmProblem holds 12 terms: only the count can say 13
    return made


_REFUSED_PROBLEMS = {
    '27_problems': lambda: [_small_problem() for _ in range(27)],
    '13_terms_in_a_problem': _thirteen_terms,
    '33_terms_in_a_launch': lambda: [_small_problem(nterms=11) for _ in range(3)],
    'asum_with_two_terms': lambda: [_small_problem(nterms=2, with_asum=True)],
    'epi_2_without_aux': lambda: [_small_problem(epi=2)],
    'epi_3_without_aux': lambda: [_small_problem(epi=3)],
    'epi_4': lambda: [_small_problem(epi=4, with_aux=True)],
    'M_0': lambda: [_small_problem(M=0)],
    'N_negative': lambda: [_small_problem(N=-1)],
    'K_0': lambda: [_small_problem(K=0)],
    'k_term_negative_and_K_0': lambda: [_small_problem(K=0, k_term=-3)],
    'null_C': lambda: [_small_problem(C=None)],
    'null_A': lambda: [_small_problem(A=None)],
    'null_B': lambda: [_small_problem(B=None)],
}


@pytest.mark.parametrize('what', sorted(_REFUSED_PROBLEMS))
def test_batch_refuses_bad_arguments_and_touches_nothing(what):
    from deepphysinet_amd.linear import _launch
    made = _REFUSED_PROBLEMS[what]()
    if what == '33_terms_in_a_launch':
        assert sum(q.nterms for q, _ in made) == 33
    with pytest.raises(RuntimeError, match='dpn_sgemm_batch failed with code -1'):
        _launch([q for q, _ in made])
    torch.cuda.synchronize()
    assert all(_untouched(t['C']) and _untouched(t['asum']) for _, t in made)


@pytest.mark.parametrize('what', ['11_jobs', 'job_with_0_blocks'])
def test_batch_jobs_refuses_bad_jobs_and_touches_nothing(what):
    from deepphysinet_amd.linear import _launch
    dev = _dev()
    q, t = _small_problem()
    partial = torch.ones(2, 512, device=dev)
    outs = [torch.full((256,), float(G.SENTINEL), device=dev) for _ in range(22)]
    n = 11 if what == '11_jobs' else 2
    jobs = [(partial, 0, outs[2 * i], outs[2 * i + 1], 0 if (what != '11_jobs' and i == 1) else 2) for i in range(n)]
    with pytest.raises(RuntimeError, match='dpn_sgemm_batch_jobs failed with code -1'):
        _launch([q], jobs)
    torch.cuda.synchronize()
    assert _untouched(t['C']) and all(_untouched(o) for o in outs)


@pytest.mark.parametrize('what', ['null_A', 'null_B', 'null_C', 'M_0', 'N_0', 'K_0'])
def test_sgemm_refuses_bad_arguments_and_touches_nothing(what):
    from deepphysinet_amd import _lib as L
    dev = _dev()
    A, B, C = torch.ones(3, 4, device=dev), torch.ones(4, 5, device=dev), torch.full((3, 5), float(G.SENTINEL), device=dev)
    a = dict(M=3, N=5, K=4, A=A.data_ptr(), B=B.data_ptr(), C=C.data_ptr())
    k, v = what.split('_')
    a[v if k == 'null' else k] = None if k == 'null' else 0
    with pytest.raises(RuntimeError, match='dpn_sgemm failed with code -1'):
        L.check(L.load().dpn_sgemm(0, 0, a['M'], a['N'], a['K'], a['A'], 4, a['B'], 5, a['C'], 5, None, None, 0, None, 0,
                                   torch.cuda.current_stream().cuda_stream), 'dpn_sgemm')
    torch.cuda.synchronize()
    assert _untouched(C)


@pytest.mark.parametrize('what', ['mode_3', 'mode_2_without_partial'])
def test_sgemm_ln_refuses_bad_arguments_and_touches_nothing(what):
    from deepphysinet_amd.linear import _launch_ln
    d = G.build_ln(2, 33, 33, 0, True)
    e = {k: _D(b) for k, b in d.items()}
    with pytest.raises(RuntimeError, match='dpn_sgemm_ln failed with code -1'):
        _launch_ln(3 if what == 'mode_3' else 2, 33, 33, e['x'].view, e['r'].view, e['gamma'].view, None, e['rstd_in'].view, e['y'].view, None, None,
                   e['partial'].view if what == 'mode_3' else None, e['B'].view, 0, e['B'].ld, e['C'].view, e['C'].ld)
    torch.cuda.synchronize()
    assert all(_untouched(e[k].full) for k in ('y', 'C', 'partial'))
