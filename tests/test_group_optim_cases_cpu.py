"""No GPU: the case table of clip + Adam with parameter groups (tests/group_optim_cases.py) is what it claims, the bounds it takes over from
tests/optim_cases.py hold for a correct fp32 evaluation of the grouped step and bite on a wrong one.

Margins of the plain numpy fp32 model (group_optim_cases.model_fp32: no fused multiply-add) over the whole table, largest error / bound:
norm 0.08,  m 0.27,  v 0.23,  p 0.994,  shadow 0.62.  The p bound is nearly used up by design, as in test_optim_cases_cpu.py.
"""
import numpy as np
import pytest

import group_optim_cases as G
import optim_cases as O

RECORDED_MARGIN = dict(norm=0.09, m=0.28, v=0.24, p=1.0, s=0.62)


# ---------------------------------------------------------------------------------------------- the table
def test_table_covers_what_the_issue_lists():
    by = {c.name: c for c in G.CASES}
    assert len(by) == len(G.CASES)
    short = [c for c in G.CASES if c.numels == G.SHORT and c.groups == (0, 1, 2, 0, 1, 2)]
    assert {c.place for c in short} == {'aligned', 'shifted', 'mixed'} and {c.t for c in short} >= {1, 2, 1000}
    assert {c.gs for c in short} == {1.0, 1.0 / 3} and {c.ema is None for c in short} == {True, False}
    assert {(c.ema or (0, 0, None))[2] for c in G.CASES} == {None, True, False}           # no EMA, with and without warm-up
    for n in (161, 321):                                       # a table boundary inside the list, groups i % 3, every placement
        cs = [c for c in G.CASES if c.numels == O.long_list(n, O.FLAT_TABLE) and c.groups == tuple(i % 3 for i in range(n))]
        assert {c.place for c in cs} >= {'aligned', 'shifted', 'mixed'}
        assert all(c.groups[O.FLAT_TABLE:] != c.groups[:n - O.FLAT_TABLE] for c in cs)     # reading group_of from 0 in the second table is wrong
    assert any(c.n_groups == 1 for c in G.CASES) and any(c.n_groups == 16 and set(c.groups) == set(range(16)) for c in G.CASES)
    assert any(c.n_groups > max(c.groups) + 1 or set(range(c.n_groups)) - set(c.groups) for c in G.CASES)       # a group without tensors
    assert any(r['lr'] == 0.0 for c in G.CASES for r in G.rows_of(c))
    for name, key in (('wd_only', ('wd',)), ('betas_only_t2', ('b1', 'b2')), ('eps_only_t1', ('eps',))):
        rows = G.rows_of(by[name])
        differing = {k for k in G.ROW_NAMES if len({r[k] for r in rows}) > 1}
        assert differing == set(key), (name, differing)
    for c in G.CASES:
        assert len(c.groups) == len(c.numels) and max(c.groups) < c.n_groups <= G.MAX_GROUPS
        assert 0 < sum(c.numels) <= O.MAX_CASE_ELEMENTS
        h = G.hyper_rows(c)
        assert h.shape == (c.n_groups, 8) and h.dtype == np.float32
        assert float(h[0, 5]) == G.rows_of(c)[0]['max_norm'] and float(h[0, 6]) == O.f32(c.gs)


def test_clip_cases_are_active_and_inactive_as_named():
    for c in G.CASES:
        ref = G.references(c.name)[0][1]
        gs = O.f32(c.gs)
        if c.kind == 'E':
            assert ref['coef'] == gs
        elif c.clip == 'active':
            assert ref['coef'] < gs, c.name
        else:
            assert ref['coef'] == gs, c.name
        # one global norm: every group's one-group reference carries the same sum of squares
        assert len({r['S'] for _, r in G.references(c.name)}) == 1


def test_reference_of_one_group_is_the_plain_reference():
    c = G.case_by_name('one_group_short')
    inp, _ = G.built(c.name)
    (one, ref), = G.references(c.name)
    plain = O.reference(inp)
    assert one.hyper == inp.hyper
    assert all(np.array_equal(a, b) for k in 'pmv' for a, b in zip(ref[k], plain[k])) and ref['norm'] == plain['norm']


# ---------------------------------------------------------------------------------------------- the bounds hold ...
@pytest.mark.parametrize('name', G.CASE_IDS)
def test_fp32_model_is_inside_every_bound(name):
    c = G.case_by_name(name)
    inp, s0 = G.built(name)
    got = G.model_fp32(c, inp, s0)
    r = G.ratios(c, got)
    for k in ('norm', 'm', 'v', 'p'):
        assert r[k] <= RECORDED_MARGIN[k], (name, k, r[k])
    if c.ema is not None:
        assert G.shadow_ratio(c, s0, got) <= RECORDED_MARGIN['s'], name
    for i, k in enumerate(c.groups):                          # lr = 0: the parameters of that group stay, bit for bit
        if G.rows_of(c)[k]['lr'] == 0.0:
            assert O.bits_equal(got['p'][i], inp.p[i]) and not O.bits_equal(got['m'][i], inp.m[i])


# ---------------------------------------------------------------------------------------------- ... and bite
# mistake -> [(case that catches it, a quantity whose bound it exceeds)]
CAUGHT_BY = {
    'row0_everywhere': [('short_aligned_t1_gs1_plain', 'p'), ('wd_only', 'm'), ('betas_only_t2', 'v'), ('eps_only_t1', 'p'), ('sixteen_short', 'p')],
    'norm_per_group': [('short_aligned_t1_gs3_ema', 'm'), ('list161_aligned', 'm'), ('wd_only', 'm')],
    'second_table_group_from_0': [('list161_aligned', 'p'), ('list161_shifted', 'm'), ('list321_mixed', 'v'), ('sixteen_list161_ema', 'p')],
    'bias_correction_row0': [('betas_only_t1', 'p'), ('betas_only_t2', 'p'), ('short_shifted_t2_gs1_emawarm', 'p')],
}


def test_every_seeded_mistake_has_a_catching_case():
    assert set(CAUGHT_BY) == set(G.MISTAKES)


@pytest.mark.parametrize('mistake,name,quantity', [(m, *c) for m in G.MISTAKES for c in CAUGHT_BY[m]])
def test_seeded_mistake_exceeds_a_bound(mistake, name, quantity):
    c = G.case_by_name(name)
    inp, s0 = G.built(name)
    r = G.ratios(c, G.model_fp32(c, inp, s0, mistake))
    assert r[quantity] > 1, (mistake, name, r)


def test_second_table_mistake_needs_a_second_table():
    c = G.case_by_name('short_aligned_t1_gs1_plain')
    inp, s0 = G.built(c.name)
    a, b = G.model_fp32(c, inp, s0), G.model_fp32(c, inp, s0, 'second_table_group_from_0')
    assert all(O.bits_equal(x, y) for k in 'pmv' for x, y in zip(a[k], b[k]))
