"""No GPU: the weight-EMA case table (tests/ema_cases.py) is what it claims, its bound holds for a correct fp32 evaluation and bites on a wrong
one, and the library, the header's binding and the optimiser's argument checks know the two new entry points.

Margin of the plain numpy fp32 model (ema_cases.model_fp32: product and sum rounded separately, one rounding more than the kernel's fma) over
the whole table: largest |s - s'| / bound 0.653 without warm-up, 0.408 with it (its four roundings of half an ulp each against the bound's
three whole ones: at most 2/3).
"""
import numpy as np
import pytest

import ema_cases as E
import optim_cases as O

RECORDED_MARGIN = 0.70            # largest ratio of the fp32 model over the table, rounded up: a model that needs more has changed


def _step(name):
    """(case, s0, p before, p after) with the numpy Adam model of optim_cases standing in for the kernel's p'."""
    case = E.case_by_name(name)
    inp, s0 = E.built(name)
    return case, s0, inp.p, _p_new(name)


_P_NEW = {}


def _p_new(name):
    if name not in _P_NEW:
        _P_NEW[name] = O.model_fp32(E.built(name)[0])['p']
    return _P_NEW[name]


# ---------------------------------------------------------------------------------------------- the table
def test_table_covers_what_it_lists():
    assert len(set(E.CASE_IDS)) == len(E.CASES)
    assert len(E.COMBOS) == 48 and {(c.t, c.base, c.warmup, c.decay) for c in E.CASES} == set(E.COMBOS)
    for n in E.NUMEL_EDGES:
        assert {c.place for c in E.CASES if c.numels == (n,)} == set(E.PLACES), n
    for n in E.LISTS:
        assert {c.place for c in E.CASES if c.numels == E.long_list(n, E.FLAT_TABLE)} >= set(E.PLACES), n
    assert {(c.t, c.base, c.warmup, c.decay) for c in E.CASES if c.name.startswith('combo_')} == set(E.COMBOS)
    assert {c.decay for c in E.CASES} == set(E.DECAYS) and {c.t for c in E.CASES} == set(E.STEPS) and {c.base for c in E.CASES} == set(E.BASES)
    for c in E.CASES:
        assert 0 < sum(c.numels) <= O.MAX_CASE_ELEMENTS and c.hyper in E.HYPER


def test_placements_reach_the_paths_they_name():
    """The shadow is the fifth role: off with everything else ('shifted'), alone ('mixed', sshift), or on 16 bytes next to p or g alone off."""
    for c in E.CASES:
        paths = E.path_of(c)
        sh, ss = E.shifts_of(c)
        assert 0 <= ss < 4 and len(sh) == len(c.numels)
        if c.place == 'aligned':
            assert ss == 0 and set(paths) == {'vector'}
        elif c.place == 'shifted':
            assert ss in (1, 2, 3) and set(paths) == {'scalar'} and all(s[0] and s[1] for s in sh)
        elif ss:
            assert set(paths) == {'scalar'} and not any(s[0] or s[1] for s in sh)          # the shadow ALONE sends every tensor down the scalar loop
    mixed = [c for c in E.CASES if c.place == 'mixed']
    assert any(c.sshift for c in mixed) and any(not c.sshift for c in mixed)
    lists = [c for c in mixed if len(c.numels) > 100 and not c.sshift]
    assert lists and all(set(E.path_of(c)) == {'vector', 'scalar'} for c in lists)
    assert any(c.sshift for c in mixed if len(c.numels) > 100)


def test_inputs_are_shared_and_plausible():
    for c in E.CASES:
        inp, s0 = E.built(c.name)
        assert E.built(c.name)[1] is s0
        assert all(s.dtype == np.float32 and len(s) == n and np.isfinite(s).all() for s, n in zip(s0, c.numels))
        assert any((s != p).any() for s, p in zip(s0, inp.p))


def test_decay_schedule():
    assert E.decay64(0.9999, 1, 0, True) == 2.0 / 11.0 and E.decay64(0.9999, 1, 5, True) == 7.0 / 16.0
    assert E.decay64(0.9, 1000, 0, True) == O.f32(0.9) and E.decay64(0.9, 1, 0, False) == O.f32(0.9)
    assert E.decay64(0.0, 1, 0, True) == 0.0
    # the ramp crosses 0.9 between te = 79 and 80 (80 / 89 < 0.9 <= 81 / 90), 0.9999 far beyond every step of the table
    assert E.decay64(0.9, 74, 5, True) == 80.0 / 89.0 and E.decay64(0.9, 75, 5, True) == O.f32(0.9)
    assert E.decay64(0.9999, 1000, 5, True) == 1006.0 / 1015.0


# ---------------------------------------------------------------------------------------------- the bound holds ...
@pytest.mark.parametrize('name', E.CASE_IDS)
def test_fp32_model_is_inside_the_bound(name):
    case, s0, p_old, p_new = _step(name)
    args = (case.decay, case.t, case.base, case.warmup)
    got = E.model_fp32(s0, p_old, p_new, *args)
    r = E.ratio(got, E.reference(s0, p_new, *args), E.bound(s0, p_new, *args))
    assert r <= RECORDED_MARGIN, (name, r)
    if case.decay == 0.0:
        assert all(O.bits_equal(g, p) for g, p in zip(got, p_new))


def test_recorded_margin_is_what_the_table_needs():
    worst = {True: 0.0, False: 0.0}
    for c in E.CASES:
        case, s0, p_old, p_new = _step(c.name)
        args = (case.decay, case.t, case.base, case.warmup)
        worst[c.warmup] = max(worst[c.warmup], E.ratio(E.model_fp32(s0, p_old, p_new, *args), E.reference(s0, p_new, *args), E.bound(s0, p_new, *args)))
    print('fp32 model, largest |s - s\'| / bound: without warm-up %.3f, with warm-up %.3f' % (worst[False], worst[True]))
    assert max(worst.values()) <= RECORDED_MARGIN and max(worst.values()) > 0.1        # the bound is neither broken nor slack by an order


def test_propagated_bound_damps_earlier_steps():
    b = [[np.array([1.0])], [np.array([2.0])], [np.array([4.0])]]
    out = E.propagated_bound(b, [0.5, 0.5, 0.5])
    assert out[0][0] == 1.0 * 0.25 + 2.0 * 0.5 + 4.0


# ---------------------------------------------------------------------------------------------- ... and bites
# mistake -> cases that catch it
CAUGHT_BY = {
    'decay_swapped': ['combo_t1000_b0_flat_d0.9', 'combo_t1_b0_flat_d0', 'combo_t1000_b5_warm_d0.9999', 'single_2049_aligned'],
    'p_before_update': ['combo_t1000_b0_flat_d0.9', 'combo_t2_b5_flat_d0', 'combo_t10_b0_warm_d0.9999'],
    'warmup_t_minus_1': ['combo_t1_b0_warm_d0.9', 'combo_t10_b5_warm_d0.9999', 'combo_t2_b0_warm_d0.9999'],
    'base_ignored': ['combo_t1_b5_warm_d0.9', 'combo_t10_b5_warm_d0.9999', 'combo_t2_b5_warm_d0.9'],
}


def test_every_seeded_mistake_has_a_catching_case():
    assert set(CAUGHT_BY) == set(E.MISTAKES)


@pytest.mark.parametrize('mistake,name', [(m, n) for m in E.MISTAKES for n in CAUGHT_BY[m]])
def test_seeded_mistake_exceeds_the_bound(mistake, name):
    case, s0, p_old, p_new = _step(name)
    args = (case.decay, case.t, case.base, case.warmup)
    r = E.ratio(E.model_fp32(s0, p_old, p_new, *args, mistake=mistake), E.reference(s0, p_new, *args), E.bound(s0, p_new, *args))
    assert r > 1, (mistake, name, r)


# ---------------------------------------------------------------------------------------------- the library and the optimiser, host side
def test_library_exports_and_host_side_refusals():
    """Both entry points resolve with the binding's prototypes; what they refuse on the host they refuse without a device (nothing is launched
    before the checks)."""
    import ctypes
    from deepphysinet_amd import _lib
    lib = _lib.load()
    assert len(_lib.EXPORTS['dpn_clip_adam_flat_ema'][1]) == len(_lib.EXPORTS['dpn_clip_adam_flat_dev'][1]) + 3
    one = (ctypes.c_int64 * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(16)
    assert lib.dpn_ema_swap(0, ptrs, one, ctypes.c_void_p(16), None) == -1
    assert lib.dpn_ema_swap(1, None, one, ctypes.c_void_p(16), None) == -1
    assert lib.dpn_ema_swap(1, ptrs, None, ctypes.c_void_p(16), None) == -1
    assert lib.dpn_ema_swap(1, ptrs, one, None, None) == -1
    assert lib.dpn_ema_swap(1, ptrs, (ctypes.c_int64 * 1)(0), ctypes.c_void_p(16), None) == -1
    assert lib.dpn_ema_swap(1, ptrs, (ctypes.c_int64 * 1)(2 ** 31), ctypes.c_void_p(16), None) == -1
    p16 = ctypes.c_void_p(16)
    assert lib.dpn_clip_adam_flat_ema(1, ptrs, ptrs, one, p16, p16, p16, p16, p16, None, None, None, 1, None) == -1       # no shadow
    assert lib.dpn_clip_adam_flat_ema(1, ptrs, ptrs, one, p16, p16, p16, p16, None, None, p16, None, 1, None) == -1       # no hyper
    assert lib.dpn_clip_adam_flat_ema(1, ptrs, ptrs, (ctypes.c_int64 * 1)(0), p16, p16, p16, p16, p16, None, p16, None, 1, None) == -1


def test_loop_option_and_flags_parse():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    assert m._ema_option({}) is None and m._ema_option({'ema_weights': None}) is None
    assert m._ema_option({'ema_weights': 0.99}) == dict(decay=0.99, warmup=True)
    assert m._ema_option({'ema_weights': dict(decay=0.5, warmup=False)}) == dict(decay=0.5, warmup=False)
    with pytest.raises(ValueError, match='unknown keys'):
        m._ema_option({'ema_weights': dict(decay=0.5, warm=False)})
    with pytest.raises(ValueError, match='decay is required'):
        m._ema_option({'ema_weights': dict(warmup=False)})
    m.train_cfg.setdefault('optimizer', {})['ema_weights'] = dict(decay=0.75)          # the configuration's route
    assert m._ema_option({}) == dict(decay=0.75, warmup=True) and m._ema_option({'ema_weights': None}) is None
    import infer
    import train
    assert train.parse.parse_args(['--ema', '0.9']).ema == 0.9 and train.parse.parse_args([]).ema is None
    assert infer.parse.parse_args(['--ema']).ema is True and infer.parse.parse_args([]).ema is False
