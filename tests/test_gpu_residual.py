"""GPU (MI355X): the residual and loss family of csrc/dpn_residual.hip through its C ABI against the fp64 autograd reference of
tests/residual_cases.py -- dpn_residual_points, dpn_residual, dpn_residual_weighted, dpn_step_residual + dpn_step_finish_batch,
dpn_residual_finish[_batch] on given rows, dpn_smooth_l1, dpn_contract_gpe, every refusal and run-to-run determinism.

Pass conditions: every residual, block row, cotangent entry and loss inside GPU_FACTOR x the recorded K x 2^-24 x its own elementwise scale
(residual_cases.py; no point is left out of any comparison); the finish, SmoothL1 and contraction kernels inside bounds from their operation
counts; every array a window of an owned arena whose guards keep their bits (SENTINEL where the kernel writes, NaN around what it only reads).
Every case is launched once and its result shared.

The kernels' own worst |error| / (2^-24 scale) per kind, printed at the end of the module (measured on an MI355X; the plain fp32 torch evaluation
needs res 2.68, row 1.45, g_out 2.65, g_jxi 3.76, recorded as K = 3.5, 2.0, 3.5, 5.0, and the bars here are 4 K):
    dpn_residual_points     res 2.15
    dpn_residual            row 1.14   g_out 2.55   g_jxi 3.39
    dpn_residual_weighted   row 0.97   g_out 2.49   g_jxi 3.65
    dpn_step_residual       row 1.18   g_out 2.40   g_jxi 2.54   margin rows' PDE + data cotangent: 0.47 of its bar
    finished losses         at most 0.19 of their bars (the bars add every point's worst case, the errors add like a random walk)
No case exposed a kernel error.
"""
import ctypes

import numpy as np
import pytest
import torch

import residual_cases as R

pytestmark = pytest.mark.gpu

_RATIOS = {}


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


def _lib():
    from deepphysinet_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    print('\nresidual family, largest |error| / (2^-24 scale): ' + ', '.join('%s %.2f' % (k, v) for k, v in sorted(_RATIOS.items())))


def _note(prefix, r):
    for k, x in r.items():
        _RATIOS[prefix + k] = max(_RATIOS.get(prefix + k, 0.0), x)


def _physics(inp):
    L, _ = _lib()
    ph, tb = L.DpnPhysics(), inp.table
    for k in range(6):
        ph.mean[k], ph.std[k] = tb.mean[k], tb.std[k]
        ph.clip_lo[k], ph.clip_hi[k], ph.clip_on[k] = tb.lo[k], tb.hi[k], int(tb.clip_on[k])
        ph.factor[k], ph.sq_on[k], ph.sq_add[k] = tb.factor[k], int(tb.sq_on[k]), tb.sq_add[k]
    ph.criterion, ph.beta, ph.reduce_sum = R.CRIT_CODE[inp.crit], inp.beta, int(inp.reduce_sum)
    return ph


def _geo():
    L, _ = _lib()
    g = R.GEO
    return L.DpnGeometry(g['dx'], g['dy'], g['lon_m1'], g['lat_m1'], g['pred_t_span'])


class _Mem:
    """The arenas of one launch on the device: 'rd' fp32 read-only (NaN around the windows), 'ri' int32 read-only (0 around them: a stray read
    indexes bin_w[0], never past it), 'wr' fp32 written (SENTINEL), 'wd' fp64 written (SENTINEL64), 'rdd' fp64 read-only (NaN)."""
    KINDS = dict(rd=(np.float32, np.nan), ri=(np.int32, 0), wr=(np.float32, R.SENTINEL), wd=(np.float64, R.SENTINEL64), rdd=(np.float64, np.nan))

    def __init__(self, **arenas):
        dev = _dev()
        self.a = {kind: R.Arena(self.KINDS[kind][0], self.KINDS[kind][1], items) for kind, items in arenas.items() if items}
        self.d = {kind: torch.from_numpy(a.full).to(dev) for kind, a in self.a.items()}
        assert all(t.data_ptr() % 16 == 0 for t in self.d.values())
        self.where = {name: kind for kind, a in self.a.items() for name in a.offsets}

    def ptr(self, name):
        if name is None or name not in self.where:
            return None
        kind = self.where[name]
        return ctypes.c_void_p(self.d[kind].data_ptr() + self.a[kind].byte_offset(name))

    def fetch(self):
        torch.cuda.synchronize()
        host = {kind: t.cpu().numpy() for kind, t in self.d.items()}
        out = {name: self.a[kind].window(host[kind], name) for name, kind in self.where.items()}
        out['guards'] = {kind: (self.a[kind].outside_kept(host[kind]) if kind in ('wr', 'wd') else self.a[kind].untouched(host[kind])) for kind in self.a}
        out['untouched'] = {kind: self.a[kind].untouched(host[kind]) for kind in self.a}
        return out

    def window_untouched(self, got, name):
        kind = self.where[name]
        return R.bits_equal(got[name], self.a[kind].window(self.a[kind].full, name))


def _read_items(inp, labels=None):
    items = dict(out_n=inp.out_n, jac_n=inp.jac_n, f=inp.f)
    for k in ('gl', 'gtot', 'w', 'bin_w'):
        if getattr(inp, k) is not None:
            items[k] = getattr(inp, k)
    if labels is not None:
        items['labels'] = labels
    return items


def _sent(shape, dtype=np.float32):
    return np.full(shape, R.SENTINEL if dtype == np.float32 else R.SENTINEL64, dtype)


def _residual_mem(inp, row_cols=6, nblk=None, labels=None):
    n = inp.n
    return _Mem(rd=_read_items(inp, labels), ri=dict(bin=inp.bin) if inp.bin is not None else None,
                wr=dict(g_out=_sent((n, 6)), g_jxi=_sent((n, 6, 3)), losses=_sent(7), res=_sent((n, 6))),
                wd=dict(rows=_sent((nblk or R.blocks(n), row_cols), np.float64)))


def _launch_residual(mem, inp, entry, out='both', **bad):
    """dpn_residual / dpn_residual_weighted on the windows of `mem`.  bad: argument name -> None (a NULL pointer) or a replacement value."""
    L, lib = _lib()
    a = {k: mem.ptr(k) for k in ('out_n', 'jac_n', 'f', 'gl', 'gtot', 'rows', 'g_out', 'g_jxi', 'w', 'bin', 'bin_w')}
    if out == 'loss':
        a['g_out'] = a['g_jxi'] = None
    if out == 'cot':
        a['rows'] = None
    ph, geo = _physics(inp), _geo()
    a.update(n=inp.n, geo=ctypes.byref(geo), phys=ctypes.byref(ph))
    for k, v in bad.items():
        if k in ('criterion', 'beta'):
            setattr(ph, k, v)
        else:
            a[k] = v
    args = (a['out_n'], a['jac_n'], a['f'], a['n'], a['geo'], a['phys'], a['gl'], a['gtot'], a['rows'], a['g_out'], a['g_jxi'])
    if entry == 'weighted':
        return lib.dpn_residual_weighted(*args, a['w'], a['bin'], a['bin_w'], _stream())
    return lib.dpn_residual(*args, _stream())


def _finish(mem, inp, n=None, n_fields=1, batch=False, **bad):
    L, lib = _lib()
    ph = _physics(inp)
    a = dict(rows=mem.ptr('rows'), losses=mem.ptr('losses'), phys=ctypes.byref(ph), n=inp.n if n is None else n, n_fields=n_fields)
    a.update(bad)
    if not batch:
        return lib.dpn_residual_finish(a['rows'], a['n'], a['phys'], a['losses'], _stream())
    return lib.dpn_residual_finish_batch(a['rows'], a['n'], a['n_fields'], a['phys'], a['losses'], _stream())


_RESULTS = {}


def _result(name):
    """(return codes, fetched state, arenas) of a points / residual / weighted case: launched once, shared."""
    if name not in _RESULTS:
        L, lib = _lib()
        case = R.case_by_name(name)
        inp, _ = R.built(name)
        mem = _residual_mem(inp)
        if case.kind == 'points':
            ph, geo = _physics(inp), _geo()
            rc = [lib.dpn_residual_points(mem.ptr('out_n'), mem.ptr('jac_n'), mem.ptr('f'), inp.n, ctypes.byref(geo), ctypes.byref(ph), mem.ptr('res'), _stream())]
        else:
            rc = [_launch_residual(mem, inp, case.kind, case.out)]
            if case.out != 'cot' and rc[0] == 0:
                rc.append(_finish(mem, inp))
        _RESULTS[name] = (rc, mem.fetch(), mem)
    return _RESULTS[name]


def _assert_guards(got, what):
    for kind, kept in got['guards'].items():
        assert kept, '%s: a store outside the windows of the %s arena (or into a read-only one)' % (what, kind)


def _assert_bars(prefix, inp, ref, got, what):
    m = R.measure(inp, ref, got)
    _note(prefix, m)
    print('%s: %s' % (what, ', '.join('%s %.2f' % kv for kv in sorted(m.items()))))
    for k, x in m.items():
        assert x <= R.GPU_FACTOR * R.K_RECORDED[k], (what, k, x)


def _assert_losses(inp, ref, losses, what):
    bars, total_bar = R.loss_bars(inp, ref, R.GPU_FACTOR * R.K_RECORDED['res'])
    err = np.abs(losses[:6].astype(np.float64) - ref.ev.losses)
    print('%s: loss error / bar %s' % (what, np.array2string(err / np.maximum(bars, 1e-300), precision=3)))
    assert (err <= bars).all(), (what, err / bars)
    assert abs(float(losses[6]) - ref.ev.total) <= total_bar, (what, float(losses[6]), ref.ev.total)
    assert R.bits_equal(np.float32(losses[6]), R.total_in_order(losses[:6])), (what, 'the total is not its six terms added in the stated order')


# ---------------------------------------------------------------------------------------------- 1. dpn_residual_points
@pytest.mark.parametrize('name', R.cases_of('points'))
def test_residual_points_against_fp64(name):
    inp, ref = R.built(name)
    rc, got, mem = _result(name)
    assert rc == [0]
    _assert_guards(got, name)
    _assert_bars('points ', inp, ref, dict(res=got['res'].astype(np.float64)), name)
    for k in ('g_out', 'g_jxi', 'losses', 'rows'):
        assert mem.window_untouched(got, k), (name, k)


# ---------------------------------------------------------------------------------------------- 2, 3. dpn_residual, dpn_residual_weighted
@pytest.mark.parametrize('name', R.cases_of('residual', 'weighted'))
def test_residual_rows_losses_and_cotangents_against_fp64(name):
    """Block rows, the finished losses and both cotangents; the weighted entry against the reference with the weights in it.  With g_out NULL
    the cotangent windows keep their sentinel, with loss_sums NULL the rows do."""
    case = R.case_by_name(name)
    inp, ref = R.built(name)
    rc, got, mem = _result(name)
    assert all(x == 0 for x in rc), rc
    _assert_guards(got, name)
    out = {}
    if case.out != 'cot':
        out['rows'] = got['rows']
        _assert_losses(inp, ref, got['losses'], name)
    else:
        assert mem.window_untouched(got, 'rows') and mem.window_untouched(got, 'losses'), name
    if case.out != 'loss':
        out.update(g_out=got['g_out'].astype(np.float64), g_jxi=got['g_jxi'].astype(np.float64))
    else:
        assert mem.window_untouched(got, 'g_out') and mem.window_untouched(got, 'g_jxi'), name
    assert mem.window_untouched(got, 'res')
    _assert_bars(case.kind + ' ', inp, ref, out, name)
    if inp.exact and case.out == 'both':                         # the all-zero-Jacobian rows: five residuals exactly 0, their slopes and cotangents exact zeros
        z = slice(inp.n - R.N_EXACT_ZERO, None)
        assert not got['g_jxi'][z].any(), name
        assert not got['g_out'][z, :2].any(), name


# ---------------------------------------------------------------------------------------------- 4. dpn_step_residual + dpn_step_finish_batch
_STEP = {}


def _step_result(name):
    if name not in _STEP:
        L, lib = _lib()
        case = R.case_by_name(name)
        ni, n, B = case.n_inter, case.n, case.B
        nb = R.blocks(ni) + R.blocks(n - ni)
        assert lib.dpn_step_rows_doubles(ni, n) == 7 * nb
        fields, rcs = [], []
        all_rows = np.zeros((B, nb, 7))
        for b in range(B):
            inp, labels, sref = R.built_step(name, b)
            mem = _residual_mem(inp, row_cols=7, nblk=nb, labels=labels)
            ph, geo = _physics(inp), _geo()
            rcs.append(lib.dpn_step_residual(mem.ptr('out_n'), mem.ptr('jac_n'), mem.ptr('f'), mem.ptr('labels'), ni, n, ctypes.byref(geo), ctypes.byref(ph),
                                             R.STEP_BETA, R.f32(R.MARGIN_FACTOR / (6.0 * (n - ni))), mem.ptr('gtot'), mem.ptr('rows'), mem.ptr('g_out'),
                                             mem.ptr('g_jxi'), _stream()))
            got = mem.fetch()
            all_rows[b] = got['rows']
            fields.append((inp, labels, sref, got))
        fin = _Mem(rdd=dict(rows=all_rows), wr=dict(losses=_sent((B, 16))))
        ph = _physics(fields[0][0])
        rcs.append(lib.dpn_step_finish_batch(fin.ptr('rows'), ni, n, B, ctypes.byref(ph), R.MARGIN_FACTOR, fin.ptr('losses'), _stream()))
        _STEP[name] = (rcs, fields, fin.fetch())
    return _STEP[name]


@pytest.mark.parametrize('name', R.cases_of('step'))
def test_step_residual_and_finish_against_fp64(name):
    """Per field: both groups' rows and six losses, the data column and loss, the 16-float row with its totals in the stated order, the PDE
    cotangents on interior rows and PDE + data cotangents on margin rows."""
    case = R.case_by_name(name)
    ni, n = case.n_inter, case.n
    nb_i = R.blocks(ni)
    rcs, fields, fin = _step_result(name)
    assert all(x == 0 for x in rcs), rcs
    _assert_guards(fin, name)
    K = {k: R.GPU_FACTOR * v for k, v in R.K_RECORDED.items()}
    for b, (inp, labels, sref, got) in enumerate(fields):
        what = '%s field %d' % (name, b)
        _assert_guards(got, what)
        rows, row16 = got['rows'], fin['losses'][b]
        assert not rows[:nb_i, 6].any(), (what, 'an interior block wrote a data sum')
        derr = np.abs(rows[nb_i:, 6] - sref.data_rows)
        assert (derr <= sref.data_row_bar).all(), (what, derr / sref.data_row_bar)
        for g, (sl, off) in enumerate(((slice(0, ni), 0), (slice(ni, None), 7))):
            ginp, gref = inp.rows(sl), sref.groups[g]
            grows = rows[:nb_i, :6] if g == 0 else rows[nb_i:, :6]
            g_out = got['g_out'][sl].astype(np.float64)
            if g == 1:                                            # margin rows: the data cotangent sits behind the PDE one, one rounded addition
                want = gref.ev.g_out + sref.g_data
                x = R.ratio(g_out - want, gref.g_out_scale * K['g_out'] + sref.g_data_bar / R.U + np.abs(want))
                _note('step ', {'g_out + data (of its bar)': x})
                assert x <= 1.0, (what, x)
                m = R.measure(ginp, gref, dict(rows=grows, g_jxi=got['g_jxi'][sl].astype(np.float64)))
                _note('step ', m)
                for k, x in m.items():
                    assert x <= K[k], (what, k, x)
            else:
                _assert_bars('step ', ginp, gref, dict(rows=grows, g_out=g_out, g_jxi=got['g_jxi'][sl].astype(np.float64)), what)
            _assert_losses(ginp, gref, row16[off:off + 7], '%s group %d' % (what, g))
        assert abs(float(row16[14]) - sref.data) <= sref.data_bar, (what, float(row16[14]), sref.data)
        f = np.float32
        assert R.bits_equal(f(row16[15]), f(f(row16[14] + row16[6]) + row16[13])), (what, 'the step total is not (data + interior) + margin')


# ---------------------------------------------------------------------------------------------- 5. the finish kernels on given rows
@pytest.mark.parametrize('reduce_sum', [False, True])
@pytest.mark.parametrize('n_fields', R.FINISH_FIELDS)
@pytest.mark.parametrize('nblk', R.FINISH_BLOCKS)
def test_finish_on_given_rows(nblk, n_fields, reduce_sum):
    """Synthetic fp64 rows over 1e-20 .. 1e+20 against math.fsum, the two stated roundings and the total in the reference's order."""
    rows = R.finish_rows(nblk, n_fields)
    n = (nblk - 1) * 256 + (1 if nblk % 2 else 256)
    inp = R.Inputs(R.TABLES['custom' if nblk == 65 else 'shipped'], 'mse', 0.0, reduce_sum, np.zeros((1, 6), np.float32), np.zeros((1, 6, 3), np.float32),
                   np.zeros(1, np.float32))
    mem = _Mem(rdd=dict(rows=rows), wr=dict(losses=_sent((n_fields, 7))))
    assert _finish(mem, inp, n=n, n_fields=n_fields, batch=n_fields > 1 or nblk == 64) == 0
    got = mem.fetch()
    _assert_guards(got, (nblk, n_fields))
    for b in range(n_fields):
        l, bars, total, total_bar = R.finish_reference(rows[b], n, inp.table.factor, reduce_sum)
        err = np.abs(got['losses'][b, :6].astype(np.float64) - l)
        assert (err <= bars).all(), (nblk, b, err / bars)
        assert abs(float(got['losses'][b, 6]) - total) <= total_bar
        assert R.bits_equal(np.float32(got['losses'][b, 6]), R.total_in_order(got['losses'][b, :6]))


# ---------------------------------------------------------------------------------------------- 6. dpn_smooth_l1
def _smooth_l1_inputs(n, beta):
    rng = np.random.default_rng([n, int(beta * 1000)])
    out_n = rng.standard_normal((n, 6)).astype(np.float32)
    labels = (out_n.astype(np.float64) + rng.uniform(-3.0, 3.0, size=(n, 6)) * beta).astype(np.float32)
    special = [0.0, beta, -beta, np.float32(beta) * np.float32(0.5), 2 * beta][:min(5, 6 * n)]       # d = 0 and |d| = beta exactly: zero labels
    out_n.ravel()[:len(special)] = special
    labels.ravel()[:len(special)] = 0.0
    return out_n, labels


@pytest.mark.parametrize('mode', ['loss', 'cot', 'both', 'accumulate', 'accumulate_dev'])
@pytest.mark.parametrize('beta', [0.1, 1.0])
@pytest.mark.parametrize('n', [1, 42, 43, 256, 257])
def test_smooth_l1_against_fp64(n, beta, mode):
    """Block sums and the cotangent against fp64 F.smooth_l1_loss and its autograd: at most five fp32 operations per element, the block sum in
    fp64; accumulate adds onto a non-zero g_out with one more rounding; scale_dev multiplies the scale."""
    L, lib = _lib()
    beta = R.f32(beta)
    out_n, labels = _smooth_l1_inputs(n, beta)
    rng = np.random.default_rng(n)
    g0 = rng.standard_normal((n, 6)).astype(np.float32) if mode.startswith('accumulate') else _sent((n, 6))
    sdev = np.array([0.7], np.float32)
    scale = R.f32(1e6 / (6.0 * n))
    nblk = R.blocks(6 * n)
    mem = _Mem(rd=dict(out_n=out_n, labels=labels, sdev=sdev), wr=dict(g_out=g0), wd=dict(sums=_sent(nblk, np.float64)))
    rc = lib.dpn_smooth_l1(mem.ptr('out_n'), mem.ptr('labels'), n, beta, scale, None if mode == 'cot' else mem.ptr('sums'), None if mode == 'loss' else mem.ptr('g_out'),
                           int(mode.startswith('accumulate')), mem.ptr('sdev') if mode == 'accumulate_dev' else None, _stream())
    assert rc == 0
    got = mem.fetch()
    _assert_guards(got, (n, beta, mode))
    l, slope, bar = R.smooth_l1_reference(out_n, labels, beta)
    if mode == 'cot':
        assert mem.window_untouched(got, 'sums')
    else:
        ref = R.block_sums(np.stack([l.ravel(), bar.ravel()], 1))
        err = np.abs(got['sums'] - ref[:, 0])
        assert (err <= ref[:, 1] + 300 * 2.0 ** -53 * ref[:, 0]).all(), (n, beta, mode, err / ref[:, 1])
    if mode == 'loss':
        assert mem.window_untouched(got, 'g_out')
    else:
        gv = scale * (float(sdev[0]) if mode == 'accumulate_dev' else 1.0) * slope
        want = gv + (g0.astype(np.float64) if mode.startswith('accumulate') else 0.0)
        err = np.abs(got['g_out'].astype(np.float64) - want)
        gbar = R.U * (4 * np.abs(gv) + (np.abs(want) if mode.startswith('accumulate') else 0.0)) * 1.001
        assert (err <= gbar).all(), (n, beta, mode, float((err / np.maximum(gbar, 1e-300)).max()))
        k = min(3, 6 * n)                                         # d = 0: slope 0; |d| = beta: the linear side, +-1 -- scale * (+-1) is exact, so the
        if mode != 'accumulate_dev':                              # entry is `want` rounded once (scale * scale_dev rounds once more)
            assert R.bits_equal(got['g_out'].ravel()[:k], np.float32(want.ravel()[:k]))
        else:
            assert R.bits_equal(got['g_out'].ravel()[:1], g0.ravel()[:1])


# ---------------------------------------------------------------------------------------------- 7. dpn_contract_gpe
@pytest.mark.parametrize('n', [1, 3, 257])
def test_contract_gpe_against_fp64_einsum(n):
    L, lib = _lib()
    rng = np.random.default_rng(n)
    g_out = (rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-3, 3, size=(n, 6))).astype(np.float32)
    gpe = rng.standard_normal((n, 6, R.KPE)).astype(np.float32)
    mem = _Mem(rd=dict(g_out=g_out, gpe=gpe), wr=dict(g_pe=_sent((n, R.KPE))))
    assert lib.dpn_contract_gpe(mem.ptr('g_out'), mem.ptr('gpe'), n, mem.ptr('g_pe'), _stream()) == 0
    got = mem.fetch()
    _assert_guards(got, n)
    want = np.einsum('nk,nkc->nc', g_out.astype(np.float64), gpe.astype(np.float64))
    bar = 7 * R.U * np.einsum('nk,nkc->nc', np.abs(g_out.astype(np.float64)), np.abs(gpe.astype(np.float64)))
    err = np.abs(got['g_pe'].astype(np.float64) - want)
    assert (err <= bar).all(), float((err / bar).max())


# ---------------------------------------------------------------------------------------------- 8. refusals
_NULLS = ('out_n', 'jac_n', 'f', 'geo', 'phys')
_COMMON = [dict(**{k: None}) for k in _NULLS] + [dict(n=0), dict(n=-3), dict(g_jxi=None), dict(criterion=3), dict(criterion=-1),
                                                  dict(criterion=2, beta=0.0), dict(criterion=2, beta=-0.5)]


def _ids(bads):
    return ['-'.join('%s=%s' % kv for kv in b.items()) for b in bads]


def _refused(mem, rc):
    got = mem.fetch()
    assert rc == -1
    assert all(got['untouched'].values()), got['untouched']


@pytest.mark.parametrize('bad', _COMMON, ids=_ids(_COMMON))
def test_residual_refusals(bad):
    inp, _ = R.built('res_shipped_mse_257')
    mem = _residual_mem(inp)
    _refused(mem, _launch_residual(mem, inp, 'residual', **bad))


_WEIGHTED = _COMMON + [dict(w=None, bin=None, bin_w=None), dict(bin=None), dict(bin_w=None), dict(w=None, bin_w=None)]


@pytest.mark.parametrize('bad', _WEIGHTED, ids=_ids(_WEIGHTED))
def test_residual_weighted_refusals(bad):
    inp, _ = R.built('wt_both_mse_257')
    mem = _residual_mem(inp)
    _refused(mem, _launch_residual(mem, inp, 'weighted', **bad))


_POINTS = [dict(**{k: None}) for k in _NULLS + ('res',)] + [dict(n=0), dict(n=-1)]


@pytest.mark.parametrize('bad', _POINTS, ids=_ids(_POINTS))
def test_residual_points_refusals(bad):
    L, lib = _lib()
    inp, _ = R.built('points_shipped_257')
    mem = _residual_mem(inp)
    ph, geo = _physics(inp), _geo()
    a = dict(out_n=mem.ptr('out_n'), jac_n=mem.ptr('jac_n'), f=mem.ptr('f'), n=inp.n, geo=ctypes.byref(geo), phys=ctypes.byref(ph), res=mem.ptr('res'))
    a.update(bad)
    _refused(mem, lib.dpn_residual_points(a['out_n'], a['jac_n'], a['f'], a['n'], a['geo'], a['phys'], a['res'], _stream()))


_FINISH = [dict(rows=None), dict(phys=None), dict(losses=None), dict(n=0), dict(n=-5), dict(batch=True, n_fields=0), dict(batch=True, n_fields=-1)]


@pytest.mark.parametrize('batch', [False, True])
@pytest.mark.parametrize('bad', _FINISH, ids=_ids(_FINISH))
def test_residual_finish_refusals(bad, batch):
    inp, _ = R.built('res_shipped_mse_257')
    mem = _Mem(rdd=dict(rows=R.finish_rows(2, 1)[0]), wr=dict(losses=_sent(7)))
    _refused(mem, _finish(mem, inp, **dict(dict(batch=batch), **bad)))


_STEP_BAD = [dict(**{k: None}) for k in _NULLS + ('labels', 'gtot', 'rows', 'g_jxi')] + \
    [dict(n_inter=0), dict(n_inter=-1), dict(n_inter=512), dict(n_inter=513), dict(criterion=3), dict(criterion=2, beta=0.0), dict(data_beta=0.0),
     dict(data_beta=-1.0)]


@pytest.mark.parametrize('bad', _STEP_BAD, ids=_ids(_STEP_BAD))
def test_step_residual_refusals(bad):
    L, lib = _lib()
    name = 'step_255_257_B1'
    case = R.case_by_name(name)
    inp, labels, _ = R.built_step(name, 0)
    ni, n = case.n_inter, case.n
    assert n == 512                                               # the bad n_inter values: 0, -1, n, n + 1
    mem = _residual_mem(inp, row_cols=7, nblk=R.blocks(ni) + R.blocks(n - ni), labels=labels)
    ph, geo = _physics(inp), _geo()
    a = {k: mem.ptr(k) for k in ('out_n', 'jac_n', 'f', 'labels', 'gtot', 'rows', 'g_out', 'g_jxi')}
    a.update(n_inter=ni, geo=ctypes.byref(geo), phys=ctypes.byref(ph), data_beta=R.STEP_BETA)
    for k, v in bad.items():
        if k in ('criterion', 'beta'):
            setattr(ph, k, v)
        else:
            a[k] = v
    _refused(mem, lib.dpn_step_residual(a['out_n'], a['jac_n'], a['f'], a['labels'], a['n_inter'], n, a['geo'], a['phys'], a['data_beta'], 1.0, a['gtot'],
                                        a['rows'], a['g_out'], a['g_jxi'], _stream()))
    assert lib.dpn_step_rows_doubles(0, n) == 0 and lib.dpn_step_rows_doubles(n, n) == 0


_STEP_FIN_BAD = [dict(rows=None), dict(phys=None), dict(losses=None), dict(n_inter=0), dict(n_inter=512), dict(n_fields=0)]


@pytest.mark.parametrize('bad', _STEP_FIN_BAD, ids=_ids(_STEP_FIN_BAD))
def test_step_finish_refusals(bad):
    L, lib = _lib()
    inp, _ = R.built('res_shipped_mse_257')
    n, ni = 512, 255
    mem = _Mem(rdd=dict(rows=R.finish_rows(3, 1, cols=7)[0]), wr=dict(losses=_sent(16)))
    ph = _physics(inp)
    a = dict(rows=mem.ptr('rows'), n_inter=ni, n_fields=1, phys=ctypes.byref(ph), losses=mem.ptr('losses'))
    a.update(bad)
    _refused(mem, lib.dpn_step_finish_batch(a['rows'], a['n_inter'], n, a['n_fields'], a['phys'], R.MARGIN_FACTOR, a['losses'], _stream()))


_SL1_BAD = [dict(out_n=None), dict(labels=None), dict(n=0), dict(n=-2)]


@pytest.mark.parametrize('bad', _SL1_BAD, ids=_ids(_SL1_BAD))
def test_smooth_l1_refusals(bad):
    L, lib = _lib()
    out_n, labels = _smooth_l1_inputs(43, R.f32(0.1))
    mem = _Mem(rd=dict(out_n=out_n, labels=labels), wr=dict(g_out=_sent((43, 6))), wd=dict(sums=_sent(2, np.float64)))
    a = dict(out_n=mem.ptr('out_n'), labels=mem.ptr('labels'), n=43)
    a.update(bad)
    _refused(mem, lib.dpn_smooth_l1(a['out_n'], a['labels'], a['n'], R.f32(0.1), 1.0, mem.ptr('sums'), mem.ptr('g_out'), 0, None, _stream()))


_GPE_BAD = [dict(g_out=None), dict(gpe=None), dict(g_pe=None), dict(n=0), dict(n=-1)]


@pytest.mark.parametrize('bad', _GPE_BAD, ids=_ids(_GPE_BAD))
def test_contract_gpe_refusals(bad):
    L, lib = _lib()
    mem = _Mem(rd=dict(g_out=np.ones((3, 6), np.float32), gpe=np.ones((3, 6, R.KPE), np.float32)), wr=dict(g_pe=_sent((3, R.KPE))))
    a = dict(g_out=mem.ptr('g_out'), gpe=mem.ptr('gpe'), g_pe=mem.ptr('g_pe'), n=3)
    a.update(bad)
    _refused(mem, lib.dpn_contract_gpe(a['g_out'], a['gpe'], a['n'], a['g_pe'], _stream()))


# ---------------------------------------------------------------------------------------------- 9. determinism
def test_two_runs_are_bitwise_equal():
    """The file header promises fixed-order reductions: a second launch of the n = 1037 case on fresh arenas gives the same bits."""
    name = 'res_shipped_mse_1037'
    inp, _ = R.built(name)
    first = _result(name)[1]
    mem = _residual_mem(inp)
    assert _launch_residual(mem, inp, 'residual') == 0 and _finish(mem, inp) == 0
    second = mem.fetch()
    for k in ('rows', 'losses', 'g_out', 'g_jxi'):
        assert R.bits_equal(first[k], second[k]), k
