"""No GPU: the fused clip + Adam case table (tests/optim_cases.py) is what it claims, its bounds hold for a correct fp32 evaluation and bite
on a wrong one, and its definition is torch's clip_grad_norm_ + Adam.

Margins of the plain numpy fp32 model (optim_cases.model_fp32: no fused multiply-add, so more roundings than the kernel) over the whole
table, largest error / bound per quantity:  norm 0.08,  m 0.23,  v 0.10,  p 0.997.
The p bound is nearly used up by design: where |p| ~ 1 the rounding of the store of p (u |p'|, half an ulp at worst) is almost all of it.
"""
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as O

# largest ratios of the fp32 model over the table, rounded up: a model that needs more than this has changed
RECORDED_MARGIN = dict(norm=0.09, m=0.24, v=0.11, p=1.0)


# ---------------------------------------------------------------------------------------------- the table
def test_table_covers_every_edge_it_lists():
    numels = {n for c in O.CASES for n in c.numels}
    assert set(O.NUMEL_EDGES) <= numels
    for n in O.NUMEL_EDGES:                                   # every edge alone on both alignment paths
        assert {c.place for c in O.CASES if c.numels == (n,)} >= {'aligned', 'shifted'}, n
    counts = {len(c.numels) for c in O.CASES if c.gs == 1.0}
    assert set(O.PTR_COUNTS) | set(O.FLAT_COUNTS) <= counts
    for n in (72, 73, 145, 160, 161, 321):
        assert {c.place for c in O.CASES if len(c.numels) == n and c.gs == 1.0} >= {'aligned', 'shifted', 'mixed'}, n
    assert {c.t for c in O.CASES} == set(O.STEPS)
    assert {c.gs for c in O.CASES} == set(O.GS)
    assert {c.kind for c in O.CASES} == {'W', 'U', 'U0', 'E', 'Z', 'I'}
    assert {c.hyper for c in O.CASES} == set(O.HYPER)
    for kind in ('U', 'U0'):
        assert {c.t for c in O.CASES if c.kind == kind} >= set(O.STEPS), kind
    assert {c.t for c in O.CASES if c.kind == 'E'} >= {1, 1000}
    assert len(set(O.CASE_IDS)) == len(O.CASES)
    for a, b in O.I_PAIRS:
        ca, cb = O.case_by_name(a), O.case_by_name(b)
        assert (ca.gs, ca.gmul, cb.gs, cb.gmul) == (1.0, 1, 0.125, 8) and ca.numels == cb.numels and ca.place == cb.place


@pytest.mark.parametrize('n,table', [(72, 72), (73, 72), (145, 72), (160, 160), (161, 160), (321, 160)])
def test_long_lists_put_chunk_edges_in_the_first_and_the_last_table(n, table):
    s = O.long_list(n, table)
    assert len(s) == n
    starts = O.table_starts(n, table)
    first, last = s[:table], s[starts[-1]:]
    multi = lambda part: any(k > O.CHUNK and k % O.CHUNK for k in part)           # more than one chunk and a partial last chunk
    assert multi(first) and multi(last)
    assert any(k % O.CHUNK == 0 for k in first) and any(k < 8 for k in first)
    assert sum(1 for k in s if k <= 7) > n // 2                                   # mostly tiny tensors
    for b in starts[1:]:                                                          # a whole chunk ends a table, a multi-chunk tensor starts the next
        assert s[b - 1] == O.CHUNK and s[b] > 2 * O.CHUNK
    # chunks before the last table: what the t0 > 0 offsets of the host loop are made of, and more than the tensor count
    if len(starts) > 1:
        assert sum(O.chunks_of(k) for k in s[:starts[-1]]) > starts[-1]


def test_every_case_is_small():
    for c in O.CASES:
        assert 0 < sum(c.numels) <= O.MAX_CASE_ELEMENTS and min(c.numels) >= 1, c.name


def test_restated_host_sizes_match_the_library_and_the_layout():
    from deepphysinet_amd import _lib
    lib = _lib.load()
    for c in O.CASES:
        n = len(c.numels)
        arr = (ctypes.c_int64 * n)(*c.numels)
        assert lib.dpn_clip_adam_scratch_doubles(n, arr) == O.scratch_doubles(c.numels), c.name
        assert lib.dpn_clip_adam_flat_floats(n, arr) == O.flat_floats(c.numels), c.name
        off = O.flat_offsets(c.numels)
        assert off[0] == 0 and all(o % O.CHUNK == 0 for o in off) and off[-1] + O.chunks_of(c.numels[-1]) * O.CHUNK == O.flat_floats(c.numels)
        a = O.flat_arena([np.zeros(k, np.float32) for k in c.numels], c.numels)
        assert len(a.full) == O.flat_floats(c.numels) + 2 * O.GUARD and int(a.inside.sum()) == sum(c.numels)
    assert lib.dpn_clip_adam_scratch_doubles(0, None) == -1 and lib.dpn_clip_adam_flat_floats(0, None) == -1


@pytest.mark.parametrize('place', ['aligned', 'shifted', 'mixed'])
def test_placements_reach_the_paths_they_name(place):
    c = next(c for c in O.CASES if c.place == place and len(c.numels) == 161)
    for form in ('ptr', 'flat'):
        paths, shifts = O.path_of(c, form), O.shifts_of(c, form)
        if place == 'aligned':
            assert set(paths) == {'vector'}
        elif place == 'shifted':
            assert set(paths) == {'scalar'} and {s[1] for s in shifts} == {1, 2, 3}
        else:
            assert set(paths) == {'vector', 'scalar'}
            roles = 4 if form == 'ptr' else 2                # every role is the only unaligned one somewhere
            assert {tuple(bool(x) for x in s[:roles]) for s in shifts} >= {tuple(r == k for r in range(roles)) for k in range(roles)}
    inp, _ = O.built(c.name)
    a = O.Arena(inp.p, [s[0] for s in O.shifts_of(c, 'ptr')], O.SENTINEL)
    assert all((o - s[0]) % 4 == 0 for o, s in zip(a.offsets, O.shifts_of(c, 'ptr')))
    assert all(O.bits_equal(w, x) for w, x in zip(a.windows(a.full), inp.p)) and O.is_sentinel(a.full[~a.inside]) and a.outside_kept(a.full)
    gaps = np.diff([0] + [o for o in a.offsets]) - np.array([0] + a.numels[:-1])
    assert gaps.min() >= O.GUARD


def test_input_kinds_are_what_they_claim():
    for c in O.CASES:
        inp, ref = O.built(c.name)
        h = inp.hyper
        assert all(x.dtype == np.float32 and len(x) == n for xs in (inp.p, inp.g, inp.m, inp.v) for x, n in zip(xs, inp.numels))
        assert all(np.isfinite(x).all() for xs in (inp.p, inp.g, inp.m, inp.v) for x in xs) and all((v >= 0).all() for v in inp.v)
        if c.kind in ('U', 'U0'):
            assert max(np.abs(p).max() for p in inp.p) <= h['lr']
        if c.kind in ('U0', 'E'):
            assert not any(p.any() for p in inp.p)
        if c.kind == 'E':
            gc = np.concatenate([np.abs(g.astype(np.float64)) for g in inp.g]) * ref['coef']
            assert 0.099 * h['eps'] <= gc.min() and gc.max() <= 10.1 * h['eps'] and not any(m.any() for m in inp.m + inp.v)
        if c.kind == 'Z':
            assert h['wd'] == 0.0 and ref['norm'] > 0
            assert all(not (inp.g[i].any() or inp.m[i].any() or inp.v[i].any()) for i in range(1, len(inp.numels), 2))
        if c.kind == 'I':
            gi = np.concatenate(inp.g) / c.gmul
            assert (gi == np.round(gi)).all() and np.abs(gi).max() <= 4 and ref['S'] == float(int(ref['S'])) and ref['S'] < 2.0 ** 53
        if c.gnorm:
            assert abs(ref['norm'] / (c.gnorm * inp.gs) - 1) < 1e-6 and ref['coef'] < 0.75 * inp.gs        # the clip is active because of the 1e-6
        if c.hyper in ('test_active', 'test_active_wd0') and c.kind != 'E':
            assert ref['coef'] < inp.gs
        if c.hyper in ('test_inactive', 'shipped', 'shipped_wd0'):
            assert ref['coef'] == inp.gs


# ---------------------------------------------------------------------------------------------- the bounds hold ...
@pytest.mark.parametrize('name', O.CASE_IDS)
def test_fp32_model_is_inside_every_bound(name):
    inp, ref = O.built(name)
    got = O.model_fp32(inp)
    r = O.ratios(inp, ref, got)
    for k in ('norm', 'm', 'v', 'p'):
        assert r[k] <= RECORDED_MARGIN[k], (name, k, r[k])
    c = O.case_by_name(name)
    if c.kind == 'Z':
        for i in range(1, len(inp.numels), 2):
            assert O.bits_equal(got['p'][i], inp.p[i]) and O.bits_equal(got['m'][i], inp.m[i]) and O.bits_equal(got['v'][i], inp.v[i])
    if c.kind == 'I' and c.gs == 1.0:
        assert got['norm'] == float(np.float32(np.sqrt(ref['S'])))


@pytest.mark.parametrize('a,b', O.I_PAIRS)
def test_power_of_two_grad_scale_is_bit_identical_in_the_model(a, b):
    ia, ib = O.built(a)[0], O.built(b)[0]
    assert all(O.bits_equal(x, y) for k in 'pmv' for x, y in zip(getattr(ia, k), getattr(ib, k)))
    assert all(O.bits_equal(x * np.float32(8), y) for x, y in zip(ia.g, ib.g))
    ga, gb = O.model_fp32(ia), O.model_fp32(ib)
    assert ga['norm'] == gb['norm'] and all(O.bits_equal(x, y) for k in 'pmv' for x, y in zip(ga[k], gb[k]))


# ---------------------------------------------------------------------------------------------- ... and bite
# mistake -> [(case that catches it, tensors per launch, a quantity whose bound it exceeds)]
CAUGHT_BY = {
    'bc2_dropped': [('u_t1_test', 160, 'p'), ('u0_t10_shipped', 160, 'p')],
    't_plus_1': [('u_t2_test', 160, 'p'), ('u0_t10_shipped', 160, 'p')],
    't_minus_1': [('u_t3_offdefault', 160, 'p'), ('u0_t2_shipped', 160, 'p')],
    'eps_before_bc2': [('e_shipped_wd0_t1', 160, 'p'), ('u0_t2_shipped', 160, 'p'), ('u_t10_test', 160, 'p')],
    'eps_inside_sqrt': [('u0_t2_shipped', 160, 'p'), ('u_t10_test', 160, 'p'), ('u0_t100000_shipped', 160, 'p'), ('e_offdefault_t1000', 160, 'p')],
    'wd_before_clip': [('w_list145_active', 72, 'm'), ('u_t1000_gs3', 160, 'm')],
    'clip_1e-6_dropped': [('w_norm1e-6_tiny_clip', 160, 'm'), ('u_norm1e-6_tiny_clip', 160, 'p')],
    'gs_once': [('w_gs3_shipped', 160, 'm'), ('w_gs8_test_active', 160, 'm')],
    'norm_first_table': [('w_list73_aligned', 72, 'norm'), ('w_list161_aligned', 160, 'norm'), ('w_list321_active', 160, 'm')],
    'second_table_moments_from_zero': [('w_list161_aligned', 160, 'm'), ('w_list321_shifted', 160, 'v'), ('w_list73_mixed', 72, 'm')],
    'tail_chunk_skipped': [('w_single_2049_aligned', 160, 'm'), ('w_single_5_shifted', 160, 'norm'), ('w_list161_mixed', 160, 'p')],
    'v_not_squared': [('w_single_257_aligned', 160, 'v'), ('u_t2_test', 160, 'p')],
}


def test_every_seeded_mistake_has_a_catching_case():
    assert set(CAUGHT_BY) == set(O.MISTAKES)


@pytest.mark.parametrize('mistake,name,table,quantity', [(m, *c) for m in O.MISTAKES for c in CAUGHT_BY[m]])
def test_seeded_mistake_exceeds_a_bound(mistake, name, table, quantity):
    inp, ref = O.built(name)
    r = O.ratios(inp, ref, O.model_fp32(inp, mistake, table))
    assert r[quantity] > 1, (mistake, name, r)


# ---------------------------------------------------------------------------------------------- the definition is torch's
W_CASES = [c.name for c in O.CASES if c.kind == 'W']


@pytest.mark.parametrize('name', W_CASES)
def test_reference_is_torch_clip_grad_norm_and_adam_in_fp64(name):
    """clip_grad_norm_ + torch.optim.Adam on fp64 CPU tensors, hyper-parameters at their fp32 values, grad_scale applied to the gradients
    beforehand, the state preset to step t - 1.  torch adds 1e-6 as a double where the kernel's ABI has float32(1e-6): that difference,
    relative to the clip denominator, is allowed on top of 1e-12."""
    inp, ref = O.built(name)
    h = inp.hyper
    ps = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in inp.p]
    opt = torch.optim.Adam(ps, lr=h['lr'], betas=(h['b1'], h['b2']), eps=h['eps'], weight_decay=h['wd'])
    for p, g, m, v in zip(ps, inp.g, inp.m, inp.v):
        p.grad = torch.from_numpy(g.astype(np.float64) * inp.gs)
        opt.state[p] = {'step': torch.tensor(float(inp.t - 1)), 'exp_avg': torch.from_numpy(m.astype(np.float64)),
                        'exp_avg_sq': torch.from_numpy(v.astype(np.float64))}
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm=h['max_norm'])
    opt.step()
    tol = 1e-12 + 4 * abs(1e-6 - O.f32(1e-6)) / (ref['norm'] + 1e-6)
    assert abs(float(norm) - ref['norm']) <= 1e-14 * ref['norm']
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert float(st['step']) == inp.t
        m0, v0, ghat = np.abs(inp.m[i].astype(np.float64)), inp.v[i].astype(np.float64), ref['ghat'][i]
        assert (np.abs(st['exp_avg'].numpy() - ref['m'][i]) <= tol * (h['b1'] * m0 + (1 - h['b1']) * ghat)).all(), (name, i, 'm')
        assert (np.abs(st['exp_avg_sq'].numpy() - ref['v'][i]) <= 2 * tol * (h['b2'] * v0 + (1 - h['b2']) * ghat ** 2)).all(), (name, i, 'v')
        assert (np.abs(p.detach().numpy() - ref['p'][i]) <= tol * (np.abs(ref['p'][i]) + 4 * np.abs(ref['dp'][i]))).all(), (name, i, 'p')
