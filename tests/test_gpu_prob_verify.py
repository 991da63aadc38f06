"""GPU (MI355X): probabilistic verification of ensembles -- dpn_pverify_stage / dpn_pverify_case / dpn_pverify_pool / dpn_pverify_finish through
ProbVerifyState, PackedField.pverify_stage, InterfacePhysics.verify_ensemble_at, run_inference_interface's `verify.members` key and infer.py
--verify_members (hi+lo mode).

Yardsticks: deepphysinet_amd.prob_verification's numpy restatement of the four kernels (bit for bit: all are compiled without contraction), fed with
what dpn_fields_out and dpn_diagnostics_out write for the same out_n (the forecast) and for coord_data in its place (the baseline); the exact tables
and the bound of tests/prob_verify_cases.py; predict_points per member and case plus fp64 numpy on the stacked values; verify_at at M = 1.  Model,
field, sampler, stations and the five members are those of tests/test_gpu_ensemble.py, the helpers those of tests/test_gpu_verify.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prob_verify_cases as PC
from tests import verify_cases as VC
from tests.test_gpu_diagnostics import _inputs, _loop_model, _physics_cases
from tests.test_gpu_ensemble import _kernel_inputs, _members, _single_rows
from tests.test_gpu_parity import _dev
from tests.test_gpu_verify import CANARY, IDS, _arr, _baseline_rows, _coord_data, _report_file, _reports, _same, _thresholds, _with_speed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = list(range(8)) + [3]                                      # all eight ids, T repeated
PIDS = [IDS[c] for c in COLS]
N_ALL, C_ALL, M_ALL = 1037, 3, 64
_cache = {}


def _case_inputs(case):
    """(name, ph, clip, out_n [C][M] and coord_data [C][M] tensors [1 037, 6], x, b [C, M, 1 037, 9]) of a physics case: for every case and member
    random normalised rows -- drawn with a seed from the five members' own out_n and coord_data rows, plus a twentieth of a standard deviation of
    noise -- and the forecast and baseline values dpn_fields_out / dpn_diagnostics_out write for them in the order of PIDS.  Seeded faults: the last
    point of member 0 of case 0 is NaN on both sides (a station outside the cube), point 2 of member 1 of case 1 has one NaN baseline entry."""
    key = ('inputs', case)
    if key not in _cache:
        name, ph, clip = _physics_cases(_inputs())[case]
        pool_o = torch.cat([o for o, _, _ in _kernel_inputs()]).cpu()
        pool_c = torch.cat(list(_coord_data())).cpu()
        _, j, f = _kernel_inputs()[0]
        zero = torch.zeros_like(j)
        outs, cds = [], []
        xs, bs = (np.zeros((C_ALL, M_ALL, N_ALL, len(COLS)), dtype=np.float32) for _ in range(2))
        for c in range(C_ALL):
            outs.append([])
            cds.append([])
            for m in range(M_ALL):
                g = torch.Generator().manual_seed(1000 * c + m)
                o = pool_o[torch.randint(0, pool_o.shape[0], (N_ALL,), generator=g)] + 0.05 * torch.randn((N_ALL, 6), generator=g)
                cd = pool_c[torch.randint(0, pool_c.shape[0], (N_ALL,), generator=g)] + 0.05 * torch.randn((N_ALL, 6), generator=g)
                if (c, m) == (0, 0):
                    o[-1], cd[-1] = float('nan'), float('nan')
                if (c, m) == (1, 1):
                    cd[2, 2] = float('nan')
                o, cd = o.to(_dev()).contiguous(), cd.to(_dev()).contiguous()
                xs[c, m] = _single_rows(o, zero, f, ph, clip)[:, PIDS]
                bs[c, m] = _single_rows(cd, zero, f, ph, clip)[:, PIDS]
                outs[c].append(o)
                cds[c].append(cd)
        _cache[key] = (name, ph, clip, outs, cds, xs, bs)
    return _cache[key]


def _obs(x, seed):
    """Reports [C, n, P] for the forecast members x [C, M, n, P]: member 0 plus a biased noise, a tenth missing, one infinite (tests/test_gpu_verify.
    _reports); where there is a second point, one report that equals a member exactly."""
    o = np.stack([_reports(x[c, :1], seed=seed + c)[0] for c in range(x.shape[0])])
    if o.shape[1] > 1:
        o[0, 1, 3] = x[0, 0, 1, 3]
    return o


def _host(state):
    """The arrays of a ProbVerifyState on the host, by the restatement's names (rel [E, 2, 2, M + 1, N]; an empty array without thresholds)."""
    out = {k: v.cpu().numpy() for k, v in state.arrays().items() if v is not None}
    out.setdefault('rel', np.zeros((0, 2, 2, state.members + 1, state.n_total), dtype=np.int32))
    return out


def _assert_state(state, want, what):
    got = _host(state)
    for key in want:
        assert _same(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())


def _assert_rows(rows, want, what):
    for key, w in want.items():
        if rows.get(key) is None:
            assert w.shape[1] == 0, (what, key)
            continue
        assert _same(rows[key].cpu().numpy(), w), (what, key)


def _same_values(got, want):
    """Bit for bit where the value is a number, NaN where it is NaN."""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) and \
        _same(np.where(np.isnan(want), np.float32(0), got), np.where(np.isnan(want), np.float32(0), want))


def _upload_obs(o):
    return torch.from_numpy(np.ascontiguousarray(o)).to(_dev())


# ------------------------------------------------------------------------------------------------ 1. the kernels against their restatement
@pytest.mark.parametrize('n', [1, 63, 65, 255, 257, N_ALL])
def test_kernels_are_the_restatement_bit_for_bit(n):
    """M = 1, 2, 5, 64 members, three cases folded one after the other: the planes after every case's stages equal dpn_fields_out's /
    dpn_diagnostics_out's rows bit for bit, the state after every case, the pooled states and every finish output equal the restatement bit for bit.
    Nine columns (T twice), four thresholds (above and below, one value that occurs), NaN rows, a NaN baseline entry, missing and infinite reports."""
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.point_path import ProbVerifyState
    name, ph, clip, outs, cds, x_all, b_all = _case_inputs([1, 63, 65, 255, 257, N_ALL].index(n) % 3)
    lo = {1: 0, 63: 2, 255: 2}.get(n, N_ALL - n)                           # from point 2 (the NaN baseline entry), or the last n (the NaN row); all: both
    x, b = x_all[:, :, lo:lo + n], b_all[:, :, lo:lo + n]
    o = _obs(x, seed=n)
    thr = _thresholds([3, 6], x[0])
    groups = {'thirds': np.arange(n) % 3 if n >= 3 else np.zeros(n, dtype=np.int64), 'all': np.zeros(n, dtype=np.int64), 'gaps': (np.arange(n) % 2) * 4}
    if n <= 257:
        groups['own, reversed'] = np.arange(n)[::-1].copy()
    for M in (1, 2, 5, 64):
        st = ProbVerifyState(n, PIDS, *thr, M, _dev())
        want = PV.prob_verify_state_zeros(n, len(PIDS), len(thr[0]), M)
        pf, pb = PV.planes_zeros(n, len(PIDS), M)
        for c in range(C_ALL):
            for m in range(M):
                st.stage(outs[c][m][lo:lo + n], cds[c][m][lo:lo + n], ph, m, 0, clip)
                PV.pverify_stage_reference(pf, pb, x[c, m], b[c, m], m)
            assert _same_values(st.plane_f.cpu().numpy(), pf) and _same_values(st.plane_b.cpu().numpy(), pb), (name, M, c)
            st.case(_upload_obs(o[c]))
            PV.pverify_case_reference(want, pf, pb, o[c], *thr)
            _assert_state(st, want, (name, M, c))
        _assert_rows(st.finish(), PV.pverify_finish_reference(want, thr[0]), (name, M, 'points'))
        if lo + n == N_ALL and n > 1:                                      # the NaN row: case 0 is not counted there, cases 1 and 2 are
            assert st.n[:, -1].max().item() <= 2
        for gname, g in groups.items():
            plan = PV.pool_plan(g)
            pooled = st.pool(*plan)
            want_pool = PV.pverify_pool_reference(want, *plan, thr[0])
            _assert_state(pooled, want_pool, (name, M, gname))
            _assert_rows(pooled.finish(), PV.pverify_finish_reference(want_pool, thr[0]), (name, M, gname))
    # no thresholds, one column: rel and the threshold destinations are absent
    st = ProbVerifyState(n, [31], [], [], [], 2, _dev())
    want = PV.prob_verify_state_zeros(n, 1, 0, 2)
    pf, pb = PV.planes_zeros(n, 1, 2)
    for m in range(2):
        st.stage(outs[2][m][lo:lo + n], cds[2][m][lo:lo + n], ph, m, 0, clip)
        PV.pverify_stage_reference(pf, pb, x[2, m][:, 3:4], b[2, m][:, 3:4], m)
    st.case(_upload_obs(o[2][:, 3:4]))
    PV.pverify_case_reference(want, pf, pb, o[2][:, 3:4])
    _assert_state(st, want, 'no thresholds')
    rows = st.finish()
    assert rows['brier'] is None and rows['rel_n'] is None
    _assert_rows(rows, PV.pverify_finish_reference(want), 'no thresholds')


def _fold_table(case):
    """A hand-written table of tests/prob_verify_cases.py through dpn_pverify_case: its members written into the planes, the restatement beside."""
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.point_path import ProbVerifyState
    x, b, o, thr = case['x'], case['b'], case['o'], case['thr']
    C, M, n, P = x.shape
    st = ProbVerifyState(n, [31] * P, *thr, M, _dev())
    host = PV.prob_verify_state_zeros(n, P, len(thr[0]), M)
    for c in range(C):
        pf, pb = (np.ascontiguousarray(v[c].transpose(0, 2, 1)) for v in (x, b))
        st.plane_f.copy_(torch.from_numpy(pf))
        st.plane_b.copy_(torch.from_numpy(pb))
        st.case(_upload_obs(o[c]))
        PV.pverify_case_reference(host, pf, pb, o[c], *thr)
    return host, st


def test_the_hand_written_tables_on_the_device():
    """Every table folded by the case kernel, pooled and finished on the device: the restatement's bits, and the exact scores within the bound (the
    integer outputs exactly) -- ties, strict thresholds, NaN members, an event that never and one that always happens, an empty group, segments of
    65, 0, 1 and 64 points."""
    from deepphysinet_amd import prob_verification as PV
    for name, case in PC.tables().items():
        host, st = _fold_table(case)
        thr_col = case['thr'][0]
        _assert_state(st, host, (name, 'points'))
        rows = st.finish()
        _assert_rows(rows, PV.pverify_finish_reference(host, thr_col), (name, 'points'))
        dev = PC.deviation({k: v.cpu().numpy() for k, v in rows.items() if v is not None}, PC.exact_of(name, False))
        plan = PV.pool_plan(case['groups'], PC.n_groups(case))
        pooled = st.pool(*plan)
        want = PV.pverify_pool_reference(host, *plan, thr_col)
        _assert_state(pooled, want, (name, 'pooled'))
        prow = pooled.finish()
        _assert_rows(prow, PV.pverify_finish_reference(want, thr_col), (name, 'pooled'))
        pdev = PC.deviation({k: v.cpu().numpy() for k, v in prow.items() if v is not None}, PC.exact_of(name, True))
        print('%s on the device against the exact table: points %.3e, pooled %.3e (bound %.3e)' % (name, dev, pdev, PC.BOUND))
        assert dev <= PC.BOUND and pdev <= PC.BOUND, (name, dev, pdev)


def test_pool_segments_of_0_1_63_64_65_and_4097_points():
    """A random state uploaded (counts, sums of both signs, histograms, reliability tables), pooled over the interleaved groups of
    tests/verify_cases.py -- 1, 0, 63, 64, 65, 129 and 4 097 points -- and finished: the restatement's bits."""
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.point_path import ProbVerifyState
    groups = VC.layout_groups()
    n, P, M, thr = groups.size, 2, 3, ([0, 1, 1], [1.0, 2.0, 3.0], [0, 0, 1])
    g = np.random.default_rng(11)
    host = PV.prob_verify_state_zeros(n, P, 3, M)
    host['n'][:] = g.integers(0, 9, host['n'].shape)
    for k in PV.STATE_F64:
        host[k][:] = g.standard_normal(host[k].shape) * 10.0 ** g.integers(-3, 4, host[k].shape)
    host['sum_d2'][:], host['sum_var'][:], host['sum_crps'][:] = np.abs(host['sum_d2']), np.abs(host['sum_var']), np.abs(host['sum_crps'])
    host['rank'][:] = g.integers(0, 5, host['rank'].shape)
    host['rel'][:, :, 0] = g.integers(0, 6, host['rel'][:, :, 0].shape)
    host['rel'][:, :, 1] = g.integers(0, 6, host['rel'][:, :, 1].shape) % (host['rel'][:, :, 0] + 1)
    st = ProbVerifyState(n, [31] * P, *thr, M, _dev())
    for key, v in st.arrays().items():
        v.copy_(torch.from_numpy(host[key]))
    plan = PV.pool_plan(groups)
    assert np.diff(plan[1]).tolist() == [1, 0, 63, 64, 65, 129, 4097]
    pooled = st.pool(*plan)
    want = PV.pverify_pool_reference(host, *plan, thr[0])
    _assert_state(pooled, want, 'segments')
    _assert_rows(pooled.finish(), PV.pverify_finish_reference(want, thr[0]), 'segments')
    _assert_rows(st.finish(), PV.pverify_finish_reference(host, thr[0]), 'points')
    assert pooled.plane_f is None and pooled.n[:, 1].tolist() == [0, 0] and bool(torch.isnan(pooled.finish()['crps'][1]).all())


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_two_runs_and_three_chunkings_give_the_same_bits():
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.point_path import ProbVerifyState
    name, ph, clip, outs, cds, x, b = _case_inputs(1)
    n, M = N_ALL, 5
    o = _obs(x, seed=9)
    thr = _thresholds([3, 6], x[0])
    obs = [_upload_obs(o[c]) for c in range(C_ALL)]
    plan = PV.pool_plan(np.arange(n) % 7)
    results = []
    for chunk in (n, n, 256, 100, 37):
        st = ProbVerifyState(n, PIDS, *thr, M, _dev())
        for c in range(C_ALL):
            for m in range(M):
                for first in range(0, n, chunk):
                    k = min(chunk, n - first)
                    st.stage(outs[c][m][first:first + k], cds[c][m][first:first + k], ph, m, first, clip)
            for first in range(0, n, chunk):
                st.case(obs[c][first:first + min(chunk, n - first)], first)
        pooled = st.pool(*plan)
        results.append((_host(st), _host(pooled), {k: v.cpu().numpy() for k, v in pooled.finish().items()}))
    for other in results[1:]:
        for a, c in zip(results[0], other):
            for key in a:
                assert _same(a[key], c[key]), key
    assert int(results[0][0]['n'].sum()) > 0
    st.clear()
    assert not bool(st.buffer.any())                                       # one memset clears the whole state


# ------------------------------------------------------------------------------------------------ 3. refusals
def _fill(shape, dt):
    return torch.full(shape, CANARY, dtype=torch.uint8, device=_dev()).repeat_interleave(torch.empty((), dtype=dt).element_size()).view(dt).view(shape)


def _raw_state(n_total, P, E, M):
    """A canary-filled state as plain tensors by DpnPVerifyState's names."""
    from deepphysinet_amd import prob_verification as PV
    st = {'n': _fill((P, n_total), torch.int32), 'rank': _fill((2, P, M + 1, n_total), torch.int32),
          'rel': _fill((max(E, 1), 2, 2, M + 1, n_total), torch.int32)}
    st.update({k: _fill((2, P, n_total), torch.float64) for k in PV.STATE_F64})
    return st


def _c_state(st, drop=()):
    from deepphysinet_amd import prob_verification as PV
    from deepphysinet_amd.point_path import _ptr
    return PV.DpnPVerifyState(*[None if k in drop else _ptr(st[k]) for k in PV.STATE_FIELDS])


def _stage(planes, out_n, cd, n, ph, clip=0, ids=(31, 25), member=0, n_members=3, first=0, n_total=None, no_f=False, no_b=False):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    return L.load().dpn_pverify_stage(_ptr(out_n), _ptr(cd), n, None if ph is None else ctypes.byref(ph), clip, _arr(ids, ctypes.c_int32),
                                      0 if ids is None else len(ids), member, n_members, first, planes[0].shape[2] if n_total is None else n_total,
                                      None if no_f else _ptr(planes[0]), None if no_b else _ptr(planes[1]), _stream())


def _case(st, planes, obs, n, n_products=2, thr_col=(0, 1), thr_val=(280.0, 0.5), thr_side=(1, 0), n_thr=None, n_members=3, first=0, n_total=None,
          drop=(), no_state=False, no_f=False, no_b=False):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    return L.load().dpn_pverify_case(None if no_f else _ptr(planes[0]), None if no_b else _ptr(planes[1]), _ptr(obs), n, n_products,
                                     _arr(thr_col, ctypes.c_int32), _arr(thr_val, ctypes.c_float), _arr(thr_side, ctypes.c_int32),
                                     (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, n_members, first,
                                     st['n'].shape[1] if n_total is None else n_total, None if no_state else ctypes.byref(_c_state(st, drop)), _stream())


def _pool(src, dst, order, seg_dev, seg_host, n_points=None, n_groups=None, n_products=2, thr_col=(0, 1), n_thr=None, n_members=3, drop_src=(),
          drop_dst=(), no_src=False, no_dst=False):
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.point_path import _ptr, _stream
    host = None if seg_host is None else (ctypes.c_int64 * len(seg_host))(*seg_host)
    return L.load().dpn_pverify_pool(None if no_src else ctypes.byref(_c_state(src, drop_src)), src['n'].shape[1] if n_points is None else n_points,
                                     _ptr(order), _ptr(seg_dev), host, dst['n'].shape[1] if n_groups is None else n_groups, n_products,
                                     _arr(thr_col, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, n_members,
                                     None if no_dst else ctypes.byref(_c_state(dst, drop_dst)), _stream())


def _finish(st, rows, first=0, n=None, n_total=None, n_products=2, thr_col=(0, 1), n_thr=None, n_members=3, drop=(), no_state=False, no_rows=False):
    from deepphysinet_amd import _lib as L, prob_verification as PV
    from deepphysinet_amd.point_path import _ptr, _stream
    table = L.DpnPVerifyOut(*[None if k in drop else _ptr(rows[k]) for k in PV.OUT_FIELDS])
    N = st['n'].shape[1]
    return L.load().dpn_pverify_finish(None if no_state else ctypes.byref(_c_state(st, drop)), N if n_total is None else n_total, n_products,
                                       _arr(thr_col, ctypes.c_int32), (0 if thr_col is None else len(thr_col)) if n_thr is None else n_thr, n_members,
                                       first, N if n is None else n, None if no_rows else ctypes.byref(table), _stream())


def _untouched(tensors):
    return all(bool((v.contiguous().view(torch.uint8) == CANARY).all()) for v in tensors.values() if v is not None)


def test_entry_points_refuse_bad_arguments_and_write_nothing():
    from deepphysinet_amd import prob_verification as PV
    I = _inputs()
    n, M = 300, 3
    ph = I['cfg'].physics()
    out_n, cd = _kernel_inputs()[0][0][:n].contiguous(), _coord_data()[0][:n].contiguous()
    obs = torch.zeros((n, 2), dtype=torch.float32, device=_dev())
    st = _raw_state(n, 2, 2, M)
    planes = (_fill((M, 2, n), torch.float32), _fill((M, 2, n), torch.float32))
    nan, inf = float('nan'), float('inf')
    ok = dict(out_n=out_n, cd=cd, n=n, ph=ph)
    cases = [dict(out_n=None), dict(cd=None), dict(ph=None), dict(ids=None), dict(no_f=True), dict(no_b=True), dict(n=0), dict(n=-3), dict(first=-1),
             dict(first=1), dict(n_total=n - 1), dict(n_total=0), dict(ids=[]), dict(ids=[31] * 17), dict(ids=[31, 18]), dict(ids=[27, 25]), dict(ids=[31, 34]),
             dict(ids=[-1, 25]), dict(member=-1), dict(member=3), dict(member=64, n_members=64), dict(n_members=0), dict(n_members=65, member=1),
             dict(n_members=-1)]
    for case in cases:
        assert _stage(planes, **{**ok, **case}) == -1, sorted(case)
    cases = [dict(obs=None), dict(no_f=True), dict(no_b=True), dict(no_state=True), dict(n=0), dict(n=-3), dict(first=-1), dict(first=1),
             dict(n_total=n - 1), dict(n_total=0), dict(n_products=0), dict(n_products=17), dict(n_members=0), dict(n_members=65), dict(n_thr=17),
             dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=[-1, 1]), dict(thr_side=[1, 2]), dict(thr_side=[-1, 0]), dict(thr_val=[280.0, nan]),
             dict(thr_val=[inf, 0.5]), dict(thr_val=[280.0, -inf]), dict(thr_col=None, n_thr=2), dict(thr_val=None, n_thr=2),
             dict(thr_side=None, n_thr=2)] + [dict(drop=(k,)) for k in PV.STATE_FIELDS]
    for case in cases:
        assert _case(st, planes, **{**dict(obs=obs, n=n), **case}) == -1, sorted(case)
    rows = {k: _fill((n, 2), torch.int32 if k == 'count' else torch.float32) for k in ('count',) + PV.SCORES + PV.THRESHOLD_SCORES}
    rows.update({k: _fill((n, 2, M + 1), torch.int32) for k in PV.HISTS + PV.DIAGRAMS})
    cases = [dict(no_state=True), dict(no_rows=True), dict(n=0), dict(n=-1), dict(first=-1), dict(first=1), dict(n_total=n - 1), dict(n_total=0),
             dict(n_products=0), dict(n_products=17), dict(n_members=0), dict(n_members=65), dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 2]),
             dict(thr_col=[-1, 0]), dict(thr_col=None, n_thr=2)] + [dict(drop=(k,)) for k in PV.STATE_FIELDS + PV.OUT_FIELDS]
    for case in cases:
        assert _finish(st, rows, **case) == -1, sorted(case)
    G = 3
    dst = _raw_state(G, 2, 2, M)
    order = torch.arange(n, dtype=torch.int32, device=_dev())
    seg = [0, 100, 100, n]
    seg_dev = torch.tensor(seg, dtype=torch.int64, device=_dev())
    good = dict(order=order, seg_dev=seg_dev, seg_host=seg)
    cases = [dict(order=None), dict(seg_dev=None), dict(seg_host=None), dict(no_src=True), dict(no_dst=True), dict(n_points=0), dict(n_points=-1),
             dict(n_groups=0), dict(n_groups=-2), dict(seg_host=[1, 100, 100, n]), dict(seg_host=[0, 100, 99, n]), dict(seg_host=[0, 100, 100, n - 1]),
             dict(seg_host=[0, 100, 100, n + 1]), dict(seg_host=[0, n + 5, 100, n]), dict(n_products=0), dict(n_products=17), dict(n_members=0),
             dict(n_members=65), dict(n_thr=17), dict(n_thr=-1), dict(thr_col=[0, 2]), dict(thr_col=None, n_thr=2)] + \
            [dict(drop_src=(k,)) for k in PV.STATE_FIELDS] + [dict(drop_dst=(k,)) for k in PV.STATE_FIELDS]
    for case in cases:
        assert _pool(st, dst, **{**good, **case}) == -1, sorted(case)
    torch.cuda.synchronize()
    assert _untouched(st) and _untouched(dst) and _untouched(rows) and _untouched(dict(f=planes[0], b=planes[1]))
    # and the same arguments, accepted (without thresholds rel and the threshold destinations may be NULL)
    for key in st:
        st[key].zero_()
    for m in range(M):
        assert _stage(planes, **ok, member=m) == 0
    assert _case(st, planes, obs, n) == 0 and _case(st, planes, obs, n) == 0 and _finish(st, rows) == 0 and _pool(st, dst, **good) == 0
    assert _case(st, planes, obs, n, thr_col=[], thr_val=[], thr_side=[], drop=('rel',)) == 0
    assert _finish(st, rows, thr_col=[], drop=('rel',) + PV.THRESHOLD_SCORES + PV.DIAGRAMS) == 0
    assert _pool(st, dst, **good, thr_col=[], drop_src=('rel',), drop_dst=('rel',)) == 0
    torch.cuda.synchronize()
    assert bool((st['n'] == 3).all()) and dst['n'][:, 1].tolist() == [0, 0] and dst['n'][:, 2].tolist() == [600, 600]
    assert bool((rows['count'] == 3).all()) and bool((rows['rank_hist'].sum(dim=2) == 3).all())


# ------------------------------------------------------------------------------------------------ 4. the composed route
def _numpy_scores(x, b, o, thr, groups=None):
    """fp64 numpy on stacked values x, b [C, M, N, P] and o [C, N, P]: the tables per point (or per group, the pairs pooled) -- the CRPS from its
    definition per pair, the Brier score from the pairs themselves, the ROC area as the Mann-Whitney count over the reliability table."""
    C, M, N, P = x.shape
    groups = np.arange(N) if groups is None else np.asarray(groups)
    G, E = int(groups.max()) + 1, len(thr[0])
    ok = np.isfinite(o) & np.isfinite(x).all(axis=1) & np.isfinite(b).all(axis=1)                # [C, N, P]
    gi = np.broadcast_to(groups[None, :, None], ok.shape)
    pj = np.broadcast_to(np.arange(P)[None, None, :], ok.shape)

    def pooled(q):
        r = np.zeros((G, P))
        np.add.at(r, (gi[ok], pj[ok]), q[ok])
        return r

    out = {'count': pooled(np.ones(ok.shape)).astype(np.int32)}
    Nd = out['count'].astype(np.float64)
    O = np.where(ok, o, 0).astype(np.float64)
    sums = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for pre, v in (('', x), ('base_', b)):
            V = np.where(ok[:, None], v, 0).astype(np.float64)
            a = np.abs(V - O[:, None]).mean(axis=1)
            g = sum(np.abs(V[:, i] - V[:, k]) for i in range(M) for k in range(i + 1, M)) if M > 1 else np.zeros_like(a)
            d = V.mean(axis=1) - O
            s_crps, s_fair = pooled(a - g / (M * M)), pooled(a - g / (M * (M - 1)) if M > 1 else a)
            s_d, s_d2, s_var = pooled(d), pooled(d * d), pooled(V.var(axis=1, ddof=1) if M > 1 else np.zeros_like(a))
            sums[pre] = (s_crps, s_fair)
            rmse = np.sqrt(s_d2 / Nd)
            out[pre + 'crps'], out[pre + 'fair_crps'], out[pre + 'bias'], out[pre + 'rmse'] = s_crps / Nd, s_fair / Nd, s_d / Nd, rmse
            out[pre + 'spread'] = np.sqrt(s_var / Nd)
            out[pre + 'spread_skill'] = np.where((M > 1) & (rmse != 0), np.sqrt((M + 1) / M * s_var / Nd) / rmse, np.nan)
            with np.errstate(invalid='ignore'):
                bins = (v < o[:, None]).sum(axis=1) + (v == o[:, None]).sum(axis=1) // 2
            hist = np.zeros((G, P, M + 1), dtype=np.int32)
            np.add.at(hist, (gi[ok], pj[ok], bins[ok]), 1)
            out[pre + 'rank_hist'] = hist
        for k, key in enumerate(('crpss', 'fair_crpss')):
            out[key] = np.where((Nd > 0) & (sums['base_'][k] != 0), 1.0 - sums[''][k] / sums['base_'][k], np.nan)
        for key in PC.THRESHOLD_SCORES:
            out[key] = np.full((G, E), np.nan)
        for key in ('rel_n', 'rel_o', 'base_rel_n', 'base_rel_o'):
            out[key] = np.zeros((G, E, M + 1), dtype=np.int32)
        p = np.arange(M + 1) / M
        for e, (j, val, side) in enumerate(zip(*thr)):
            ev = (lambda z: z > np.float32(val)) if side == 0 else (lambda z: z < np.float32(val))
            sel, Ne = ok[:, :, j], Nd[:, j]
            with np.errstate(invalid='ignore'):
                eo = ev(o[:, :, j])
            for pre, v in (('', x), ('base_', b)):
                with np.errstate(invalid='ignore'):
                    k = ev(v[:, :, :, j]).sum(axis=1)                                            # [C, N]
                rel_n, rel_o = out[pre + 'rel_n'][:, e], out[pre + 'rel_o'][:, e]
                np.add.at(rel_n, (gi[:, :, 0][sel], k[sel]), 1)
                np.add.at(rel_o, (gi[:, :, 0][sel & eo], k[sel & eo]), 1)
                sq = np.zeros(G)
                np.add.at(sq, gi[:, :, 0][sel], ((k / M - eo) ** 2)[sel])
                nk, okk = rel_n.astype(np.float64), rel_o.astype(np.float64)
                events = okk.sum(axis=1)
                obar = events / Ne
                f = okk / nk
                brier, unc = sq / Ne, obar * (1.0 - obar)
                out[pre + 'brier'][:, e] = brier
                out[pre + 'reliability'][:, e] = np.nansum(nk * (p - f) ** 2, axis=1) / Ne
                out[pre + 'resolution'][:, e] = np.nansum(nk * (f - obar[:, None]) ** 2, axis=1) / Ne
                out['uncertainty'][:, e] = unc
                out[pre + 'bss'][:, e] = np.where(unc != 0, 1.0 - brier / unc, np.nan)
                non = nk - okk
                below = np.cumsum(non, axis=1) - non                                             # the non-events at lower levels
                wins = (okk * (below + 0.5 * non)).sum(axis=1)
                out[pre + 'roc_area'][:, e] = np.where((events > 0) & (Ne - events > 0), wins / (events * (Ne - events)), np.nan)
    return out


def _assert_table(table, want, what):
    """The integer outputs exactly; the float scores NaN where the numpy route's are and within the bound measured on the CPU elsewhere.  The
    numpy route adds its fp64 terms in another order than the device; over at most 3 x 1 037 terms that moves a sum by some 1e-13 relative, far
    inside the bound, so no larger margin is taken."""
    worst = 0.0
    for key, w in want.items():
        g = table[key].cpu().numpy()
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        if key in PC.INT_KEYS:
            assert np.array_equal(g, w), (what, key)
            continue
        g = g.astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, key)
        fin = ~np.isnan(w)
        err = np.abs(g[fin] - w[fin])
        assert np.all(err <= PC.BOUND * np.abs(w[fin])), (what, key, float(np.max(err / np.maximum(np.abs(w[fin]), 1e-300))))
        nz = w[fin] != 0
        if nz.any():
            worst = max(worst, float(np.max(err[nz] / np.abs(w[fin][nz]))))
    return worst


def _model_cases():
    """(members, xi, yi, hr, names, x, b [3, 5, 1 037, 4] by case): the five members at the 1 037 stations of seed 0, three cases by rotating the
    member order; predict_points per member and dpn_fields_out on the sampler's coord_data, T, u, p and speed."""
    if 'model' not in _cache:
        I = _inputs()
        m = I['m']
        xi, yi, hr = I['stations']
        ph = I['cfg'].physics()
        mem = _members(5)
        xs = [_with_speed(m.predict_points(c['field_data'], c['sampler'], xi, yi, hr, c['forecast_h'], with_clip=False).cpu().numpy()) for c in mem]
        bs = [_with_speed(_baseline_rows(c['sampler'], xi, yi, hr, ph, False)) for c in mem]
        rot = [[(k + c) % 5 for k in range(5)] for c in range(3)]
        _cache['model'] = (mem, rot, xi, yi, hr, ['T', 'u', 'p', 'speed'], np.stack([[xs[k] for k in r] for r in rot]),
                           np.stack([[bs[k] for k in r] for r in rot]))
    return _cache['model']


def test_verify_ensemble_at_against_predict_points_and_numpy():
    I = _inputs()
    m = I['m']
    mem, rot, xi, yi, hr, names, x, b = _model_cases()
    N = xi.size
    o = np.stack([_reports(x[c, :1], seed=c)[0] for c in range(3)])
    by = {'station': np.arange(N) % 37, 'hour': np.floor(hr / 6.0).astype(np.int64), 'all': np.zeros(N, dtype=np.int64)}
    thresholds = {'T': [('below', float(np.nanmedian(x[..., 0]))), float(np.nanquantile(x[..., 0], 0.75))], 'speed': float(np.nanmedian(x[..., 3]))}
    thr = ([0, 0, 3], [float(np.float32(thresholds['T'][0][1])), float(np.float32(thresholds['T'][1])), float(np.float32(thresholds['speed']))], [1, 0, 0])
    cases = [dict(members=[mem[k] for k in rot[c]], obs=_upload_obs(o[c])) for c in range(3)]
    got = m.verify_ensemble_at(cases, xi, yi, hr, names, thresholds=thresholds, by=by)
    assert got['names'] == names and got['members'] == 5
    assert got['thresholds'] == [('T', 'below', thr[1][0]), ('T', 'above', thr[1][1]), ('speed', 'above', thr[1][2])]
    assert sorted(got) == sorted(['names', 'thresholds', 'members', 'point', 'station', 'hour', 'all'])
    for key, groups in [('point', None)] + list(by.items()):
        worst = _assert_table(got[key], _numpy_scores(x, b, o, thr, groups), key)
        print('%s: worst relative deviation %.3e (bound %.3e)' % (key, worst, PC.BOUND))
    assert got['point']['count'].shape == (N, 4) and got['station']['crps'].shape == (37, 4) and got['hour']['brier'].shape == (4, 3)
    assert got['all']['rank_hist'].shape == (1, 4, 6) and got['all']['rel_n'].shape == (1, 3, 6)
    assert int(got['all']['count'][0, 0]) == int(got['point']['count'][:, 0].sum()) > 2000
    assert int(got['all']['rank_hist'][0, 0].sum()) == int(got['all']['count'][0, 0]) == int(got['all']['rel_n'][0, 0].sum())
    # degrees: the same bits as the index units they convert to; a chunked walk: the same bits as the whole
    cfg = mem[0]['sampler'].cfg
    lon, lat = cfg.begin_lon + xi * cfg.out_res_deg, cfg.begin_lat + yi * cfg.out_res_deg
    index = m.verify_ensemble_at(cases, *mem[0]['sampler'].lonlat_to_index(lon, lat), hr, names, thresholds=thresholds, by=by)
    degrees = m.verify_ensemble_at(cases, lon, lat, hr, names, thresholds=thresholds, by=by, lonlat=True)
    m.chunk_size = lambda *a, **k: 300
    try:
        chunked = m.verify_ensemble_at(cases, *mem[0]['sampler'].lonlat_to_index(lon, lat), hr, names, thresholds=thresholds, by=by)
    finally:
        del m.chunk_size
    for other in (degrees, chunked):
        for key in ('point', 'station', 'hour', 'all'):
            for k, v in index[key].items():
                assert _same(v.cpu().numpy(), other[key][k].cpu().numpy()), (key, k)
    # a station outside the cube is refused on the host, before the first launch, as predict_points refuses it
    with pytest.raises(IndexError):
        m.verify_ensemble_at(cases, np.append(xi[:-1], 300.0), yi, hr, names)
    # with the clip: the same comparison, two members, one case
    xc = np.stack([_with_speed(m.predict_points(c['field_data'], c['sampler'], xi, yi, hr, c['forecast_h'], with_clip=True).cpu().numpy()) for c in mem[:2]])
    bc = np.stack([_with_speed(_baseline_rows(c['sampler'], xi, yi, hr, I['cfg'].physics(), True)) for c in mem[:2]])
    clipped = m.verify_ensemble_at([dict(members=mem[:2], obs=cases[0]['obs'])], xi, yi, hr, names, thresholds=thresholds, by={'all': by['all']}, with_clip=True)
    for key, groups in (('point', None), ('all', by['all'])):
        _assert_table(clipped[key], _numpy_scores(xc[None], bc[None], o[:1], thr, groups), ('clip', key))


def test_one_member_is_verify_at():
    """M = 1, one threshold: bias and rmse of the forecast and of the baseline are verify_at's to the fp32 digit, crps is its mae, and so pooled."""
    I = _inputs()
    m = I['m']
    mem, rot, xi, yi, hr, names, x, b = _model_cases()
    N = xi.size
    o = np.stack([_reports(x[c, :1], seed=c)[0] for c in range(3)])
    by = {'station': np.arange(N) % 37, 'all': np.zeros(N, dtype=np.int64)}
    thresholds = {'T': float(np.nanmedian(x[..., 0]))}
    single = [dict(mem[rot[c][0]], obs=_upload_obs(o[c])) for c in range(3)]
    det = m.verify_at(single, xi, yi, hr, names, thresholds=thresholds, by=by)
    ens = m.verify_ensemble_at([dict(members=[mem[rot[c][0]]], obs=single[c]['obs']) for c in range(3)], xi, yi, hr, names, thresholds=thresholds, by=by)
    assert ens['members'] == 1
    for key in ('point', 'station', 'all'):
        d, e = det[key], ens[key]
        assert torch.equal(d['count'], e['count'])
        for mine, theirs in (('bias', 'bias'), ('rmse', 'rmse'), ('crps', 'mae'), ('fair_crps', 'mae'), ('base_bias', 'base_bias'), ('base_rmse', 'base_rmse'),
                             ('base_crps', 'base_mae')):
            assert _same(e[mine].cpu().numpy(), d[theirs].cpu().numpy()), (key, mine)
        assert bool((e['spread'][e['count'] > 0] == 0).all()) and bool(torch.isnan(e['spread_skill']).all())
        assert e['rank_hist'].shape[-1] == 2 and torch.equal(e['rank_hist'].sum(dim=-1), e['count'])


# ------------------------------------------------------------------------------------------------ 5. loop and launcher
def test_loop_writes_the_tables_with_the_members_key(tmp_path):
    from deepphysinet_amd.prob_verification import OUT_FIELDS
    results = tmp_path / 'pverify'
    _report_file(tmp_path / 'reports.npz', M=2)
    m = _loop_model(tmp_path, write_source=True, result_path=str(results), export_variable=['T'])
    option = dict(products=['speed', 'T'], obs=str(tmp_path / 'reports.npz'), thresholds={'T': ('below', 280.0), 'speed': [3.0]},
                  by=['station', 'hour', 'all'], members=2)
    run = lambda **kw: m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', **kw)
    with pytest.raises(ValueError, match='4 samples are not a multiple of members = 3'):
        run(samples_per_epoch=4, verify=dict(option, members=3))
    with pytest.raises(ValueError, match='the reports hold 2 cases, the sample source 1 of 2 members'):
        run(samples_per_epoch=2, verify=option)
    assert not results.exists() or not os.listdir(results)                 # both refused before the first sample ran
    run(samples_per_epoch=4, verify=option)
    v = m.last_verification
    assert v['names'] == ['speed', 'T'] and v['members'] == 2 and v['thresholds'] == [('speed', 'above', 3.0), ('T', 'below', 280.0)]
    assert v['point']['crps'].shape == (20, 2) and v['station']['crps'].shape == (5, 2) and v['hour']['brier'].shape == (4, 2)
    assert v['all']['count'].shape == (1, 2) and v['all']['rank_hist'].shape == (1, 2, 3) and v['all']['rel_n'].shape == (1, 2, 3)
    count = v['point']['count'].cpu().numpy().reshape(4, 5, 2)             # point i = h * S + s
    assert count[1, 2].tolist() == [1, 1] and int(count.sum()) == 2 * 20 * 2 - 2 and bool(torch.isfinite(v['all']['crpss']).all())
    new = sorted(fn for fn in os.listdir(results) if '_pverify_' in fn)
    assert len(new) == 4 * len(OUT_FIELDS) and not [fn for fn in os.listdir(results) if '_verify_' in fn]
    stamp = sorted(os.listdir(results))[0][:-len('_T.npy')]                # the first sample's first time step
    for group in ('point', 'station', 'hour', 'all'):
        for key in OUT_FIELDS:
            assert np.array_equal(np.load(results / ('%s_pverify_%s_%s.npy' % (stamp, group, key))), v[group][key].cpu().numpy(), equal_nan=True), (group, key)


def test_the_launcher_runs_with_the_members_flag(tmp_path):
    _loop_model(tmp_path)
    _report_file(tmp_path / 'reports.npz', M=1)
    child = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--log_path', str(tmp_path / 'cli'),
                            '--synthetic', '--synthetic_samples', '2', '--verify', 'T,speed', '--verify_obs', str(tmp_path / 'reports.npz'),
                            '--verify_threshold', 'T:below:280', '--verify_by', 'station,all', '--verify_members', '2'],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    assert "verification T,speed of 2 members: point (20, 2), pairs counted 0..1, groupings ['station', 'all'], thresholds [('T', 'below', 280.0)]" \
        in child.stdout
    refused = subprocess.run([sys.executable, os.path.join(ROOT, 'infer.py'), '--checkpoint_path', str(tmp_path / 'ckpt'), '--synthetic', '--verify', 'T',
                              '--verify_obs', str(tmp_path / 'reports.npz'), '--verify_members', '2'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert refused.returncode != 0 and '1 samples are not a multiple of members = 2' in refused.stderr
