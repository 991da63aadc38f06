"""No GPU: the plan builder of the regional statistics and its refusals, the numpy restatement of dpn_region_accumulate / dpn_region_finish
(deepphysinet_amd/regions.py) against the hand-written tables of tests/regions_cases.py and against math.fsum, the seven seeded mistakes, the struct
layouts against gcc, the loop's new key and the launcher's flags.  The kernels:
tests/test_gpu_regions.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import regions_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the plan
def test_plan_of_a_label_plane_and_of_overlapping_masks():
    from deepphysinet_amd.regions import region_plan
    lab = np.array([[2, 0, -1, 0], [-1, 2, 3, 0], [0, -1, 2, -1]])                         # id 1 is an empty region, id 3 a region of one point
    p = region_plan(lab)
    assert p.n_regions == 4 and p.n_sel == 8 and p.shape == (3, 4) and p.n_candidates == 12
    assert p.order.tolist() == [1, 3, 7, 8, 0, 5, 10, 6]                                   # -1 dropped; grouped by region, ascending inside
    assert p.seg.tolist() == [0, 0, 0, 0, 2, 2, 2, 3] and p.seg.dtype == np.int32
    assert p.offs.tolist() == [0, 4, 4, 7, 8] and p.offs.dtype == np.int32
    assert p.wgt.tolist() == [1.0] * 8 and p.wgt.dtype == np.float32
    for r in range(4):                                                                      # offs and seg say the same
        assert (p.seg[p.offs[r]:p.offs[r + 1]] == r).all() and np.all(np.diff(p.order[p.offs[r]:p.offs[r + 1]]) > 0)
    assert region_plan(lab, n_regions=6).offs.tolist() == [0, 4, 4, 7, 8, 8, 8]             # trailing empty regions
    assert region_plan(torch.from_numpy(lab)).order.tolist() == p.order.tolist()
    w = np.arange(12, dtype=np.float64).reshape(3, 4) / 4
    assert region_plan(lab, w).wgt.tolist() == [0.25, 0.75, 1.75, 2.0, 0.0, 1.25, 2.5, 1.5]
    # masks may overlap: a point in k regions is listed k times
    a, b, c = lab >= 2, lab == 0, np.zeros_like(lab, dtype=bool)
    m = region_plan([a, b, c, a], w)
    assert m.n_regions == 4 and m.order.tolist() == [0, 5, 6, 10, 1, 3, 7, 8, 0, 5, 6, 10] and m.offs.tolist() == [0, 4, 8, 8, 12]
    assert m.seg.tolist() == [0] * 4 + [1] * 4 + [3] * 4 and m.wgt.tolist() == [0.0, 1.25, 1.5, 2.5, 0.25, 0.75, 1.75, 2.0, 0.0, 1.25, 1.5, 2.5]
    assert region_plan(np.stack([a, b, c, a])).order.tolist() == m.order.tolist()
    # where: entries -> (ix, iy); -1 stays
    assert m.where(np.array([[3, -1], [4, 11]])).tolist() == [[[2, 2], [-1, -1]], [[1, 0], [2, 2]]]


def test_plan_of_station_groups_and_area_weights():
    from deepphysinet_amd.regions import area_weights, region_plan, row_latitudes
    from deepphysinet_amd.sampler import SamplerConfig
    p = region_plan(groups=[1, -1, 0, 1, 1], weights=[1, 2, 3, 4, 0.5])
    assert p.shape is None and p.order.tolist() == [2, 0, 3, 4] and p.seg.tolist() == [0, 1, 1, 1] and p.offs.tolist() == [0, 1, 4]
    assert p.wgt.tolist() == [3.0, 1.0, 4.0, 0.5] and p.where(np.array([0, -1, 3])).tolist() == [2, -1, 4]
    cfg = SamplerConfig()
    lat = row_latitudes(cfg, np.arange(145))
    assert lat[0] == 18.0 and lat[-1] == 54.0 and lat.dtype == np.float64
    xi, yi = np.array([3.0, 200.5]), np.array([0.0, 77.25])
    assert np.array_equal(row_latitudes(cfg, yi), cfg.begin_lat + yi * cfg.out_res_deg)    # the inverse of lonlat_to_index
    lab = np.zeros((145, 257), dtype=np.int64)
    area = region_plan(lab, 'area', lat)
    want = np.cos(np.deg2rad(lat.astype(np.float64))).astype(np.float32)                    # float32(cos(latitude)), formed in fp64
    assert area.wgt.dtype == np.float32 and np.array_equal(area.wgt.reshape(145, 257), np.repeat(want[:, None], 257, axis=1))
    assert np.array_equal(area_weights([0.0, 60.0, 90.0]), np.array([1.0, np.cos(np.pi / 3), np.cos(np.pi / 2)]).astype(np.float32))
    st = region_plan(groups=[0, 0], weights='area', lat_deg=[30.0, 45.0])
    assert np.array_equal(st.wgt, area_weights([30.0, 45.0]))


def test_plan_refusals():
    from deepphysinet_amd.regions import n_slots, region_plan
    lab = np.array([[0, 1], [-1, 1]])
    bad = [dict(), dict(regions=lab, groups=[0, 1]), dict(regions=np.array([[0, -2]])), dict(regions=lab.astype(np.float64)), dict(regions=lab, n_regions=1),
           dict(regions=np.full((2, 2), -1)), dict(regions=np.zeros((2, 2, 2), dtype=np.int64)), dict(regions=np.zeros((0, 2), dtype=np.int64)),
           dict(regions=[]), dict(regions=[lab == 0, (lab == 1)[:1]]), dict(regions=[lab == 0, lab]), dict(regions=[lab == 7, lab == 8]),
           dict(regions=[lab == 0], n_regions=2), dict(groups=[]), dict(groups=[[0, 1]]), dict(groups=[-1, -1]), dict(groups=[0.5, 1.0]),
           dict(regions=lab, weights='volume'), dict(regions=lab, weights='area'), dict(regions=lab, weights='area', lat_deg=[10.0]),
           dict(regions=lab, weights='area', lat_deg=[10.0, 91.0]), dict(regions=lab, weights='area', lat_deg=[10.0, np.nan]),
           dict(regions=lab, weights=np.ones((2, 3))), dict(regions=lab, weights=np.ones(4)), dict(regions=lab, weights=np.array([['a', 'b'], ['c', 'd']])),
           dict(groups=[0, 1], weights=[1.0])]
    for w in (-1.0, -1e-30, np.nan, np.inf, 1e39):                                          # (1e39 is not finite in float32)
        plane = np.ones((2, 2))
        plane[1, 0] = w                                                                     # even where the point is in no region
        bad.append(dict(regions=lab, weights=plane))
        bad.append(dict(groups=[0, 0], weights=[1.0, w]))
    for kw in bad:
        with pytest.raises(ValueError):
            region_plan(**kw)
    p = region_plan(lab)
    assert n_slots(p, 1) == 1 + 2 and n_slots(p, 43) == 3 + 86                              # ceil(129 / 64) + 43 * 2
    for nt in (0, -1, 2 ** 31 // 3 + 1):                                                    # nt * n_sel must stay below 2^31
        with pytest.raises(ValueError):
            n_slots(p, nt)
    assert n_slots(p, 2 ** 31 // 3) > 0


# ------------------------------------------------------------------------------------------------ 2. the restatement
@pytest.mark.parametrize('case', RC.cases(), ids=lambda c: c['name'])
def test_restatement_reproduces_the_hand_written_tables(case):
    from deepphysinet_amd.regions import regions_reference
    got = regions_reference(case['values'], case['plan'], case['nt'], case['thr_col'], case['thr_val'])
    assert RC.mismatches(case, got) == []
    loop = RC.loop_regions(case['values'], case['plan'], case['nt'], case['thr_col'], case['thr_val'])      # the loop the mistakes are seeded in
    assert RC.mismatches(case, loop) == []
    for key in RC.KEYS:
        assert RC.same(got[key], loop[key]), key
    assert RC.same(got['partials']['count'], loop['partial_count'])


@pytest.mark.parametrize('mistake', RC.MISTAKES)
def test_every_seeded_mistake_is_caught_by_a_hand_written_case(mistake):
    caught = [c['name'] for c in RC.cases() if RC.mismatches(c, RC.loop_regions(c['values'], c['plan'], c['nt'], c['thr_col'], c['thr_val'], mistake=mistake))]
    print('%s: caught by %s' % (mistake, caught))
    assert caught, mistake


def test_restatement_checks_its_arguments_and_partials_have_the_state_layout():
    from deepphysinet_amd.regions import region_plan, regions_reference
    p = region_plan(groups=[0, 1, 1])
    v = np.ones((6, 2), dtype=np.float32)
    out = regions_reference(v, p, 2, [1], [0.5])
    S = 1 + 2 * 2
    assert {k: (a.shape, a.dtype) for k, a in out['partials'].items()} == dict(
        w=((2, S), np.float64), wx=((2, S), np.float64), count=((2, S), np.int32), vmin=((2, S), np.float32), vmax=((2, S), np.float32),
        imin=((2, S), np.int32), imax=((2, S), np.int32), wexc=((1, S), np.float64))
    assert out['frac'].shape == (2, 2, 1) and out['mean'].shape == (2, 2, 2) and out['where_min'].dtype == np.int32
    for kw in (dict(values=v[:5]), dict(values=np.ones((6, 17))), dict(values=np.ones(6)), dict(thr_col=[2], thr_val=[0.0]), dict(thr_col=[0], thr_val=[]),
               dict(thr_col=[0] * 17, thr_val=[0.0] * 17), dict(nt=0)):
        with pytest.raises(ValueError):
            regions_reference(**{**dict(values=v, plan=p, nt=2), **kw})


@pytest.mark.parametrize('n_sel,nt,R', [(257, 3, 3), (1037, 2, 40), (5000, 1, 1)])
def test_mean_is_within_the_bound_of_sequential_fp64_summation(n_sel, nt, R):
    """|mean - fsum mean| <= 2^-24 |mean| + 2 N 2^-52 sum|w x| / W: one float32 rounding of the result, and the error of N sequential fp64 additions
    of exact products in numerator and denominator (each addition 2^-53 relative to a partial sum that sum|w x|, respectively W, bounds; numerator,
    denominator and the division together stay below the factor 2 N)."""
    from deepphysinet_amd.regions import region_plan, regions_reference
    g = np.random.default_rng(n_sel)
    groups = np.sort(g.integers(0, R, size=n_sel))
    w = g.uniform(0.5, 1.0, size=n_sel).astype(np.float32)
    w[g.integers(0, n_sel, size=n_sel // 10)] = 0
    plan = region_plan(groups=groups, weights=w, n_regions=R)
    v = (g.normal(size=(nt * n_sel, 2)) * np.array([15.0, 1e-4]) + np.array([280.0, 0.0])).astype(np.float32)
    v[g.integers(0, nt * n_sel, size=7), 0] = np.nan
    ref = regions_reference(v, plan, nt)
    for col in range(2):
        for c, (mean, bound) in enumerate(RC.fsum_bound(v, plan, nt, col)):
            got = float(ref['mean'].reshape(-1, 2)[c, col])
            assert mean is not None and 0 < bound and abs(got - mean) <= bound, (col, c, got, mean, bound)


# ------------------------------------------------------------------------------------------------ 3. the C interface, as far as no device is needed
def test_region_structs_have_the_c_compilers_layout(tmp_path):
    from deepphysinet_amd import _lib
    names = ['DpnRegionPlan', 'DpnRegionState', 'DpnRegionOut']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {',
             '  printf("group %d %d %d\\n", DPN_REG_GROUP, DPN_REG_MAX_COLUMNS, DPN_REG_MAX_THRESHOLDS);']
    want = {}
    for n in names:
        st = getattr(_lib, n)
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (n, n))
        want[n] = ctypes.sizeof(st)
        for f in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (n, f[0], n, f[0]))
            want['%s.%s' % (n, f[0])] = getattr(st, f[0]).offset
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split()[1:] == [str(v) for v in (_lib.REG_GROUP, _lib.REG_MAX_COLUMNS, _lib.REG_MAX_THRESHOLDS)]
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out[1:]}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


# ------------------------------------------------------------------------------------------------ 4. the interface, the loop's key and the launcher
def test_interface_refuses_a_bad_request_before_anything_runs():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import Lattice, SamplerConfig
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    lat = Lattice(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 3, 2)
    s = type('S', (), dict(cfg=SamplerConfig()))()                                           # nothing below reaches the sampler's cube
    lab = np.zeros((3, 4), dtype=np.int64)
    with pytest.raises(KeyError, match='gust'):
        m.regional_lattice(None, s, lat, None, lab, ['speed', 'gust'])
    with pytest.raises(ValueError, match='17 products'):
        m.regional_lattice(None, s, lat, None, lab, ['speed'] * 17)
    with pytest.raises(ValueError, match='vorticity'):
        m.regional_lattice(None, s, lat, None, lab, ['speed'], thresholds={'vorticity': [0.0]})
    with pytest.raises(ValueError, match='17'):
        m.regional_lattice(None, s, lat, None, lab, ['speed'], thresholds={'speed': list(range(17))})
    with pytest.raises(ValueError, match=r'\(4, 3\)'):
        m.regional_lattice(None, s, lat, None, lab.T, ['speed'])                             # a label plane that is not (ny, nx)
    with pytest.raises(ValueError, match='negative'):
        m.regional_lattice(None, s, lat, None, lab, ['speed'], weights=-np.ones((3, 4)))
    with pytest.raises(ValueError, match='2 groups for 3 stations'):
        m.regional_at(None, s, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0], None, [0, 0], ['speed'])
    with pytest.raises(ValueError, match='hours'):
        m.regional_at(None, s, [1.0], [1.0], [[0.0, 1.0]], None, [0], ['speed'])
    with pytest.raises(KeyError, match='gust'):
        m.regional_at(None, s, [1.0], [1.0], [0.0], None, [0], ['gust'])


def test_run_inference_interface_checks_the_regions_key_before_the_checkpoint(tmp_path):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg']['log'].update(write_source=False)
    lab = np.zeros((145, 257), dtype=np.int64)
    np.save(tmp_path / 'labels.npy', lab)
    np.save(tmp_path / 'small.npy', lab[:10])
    np.save(tmp_path / 'weights.npy', -np.ones((145, 257)))
    cfg['inference_cfg']['regions'] = dict(products=['speed', 'gust'], labels=lab)
    torch.manual_seed(0)
    m = builder_models(**cfg)
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    with pytest.raises(KeyError, match='gust'):                          # no checkpoint exists at that path: the name is refused first
        m.run_inference_interface(**nothing)
    for bad in (dict(products=['speed']), dict(products=['speed'], labels=lab, thresholds={'T': [280.0]}), dict(products=['speed'], labels=lab, colour='red'),
                dict(products=['speed'], labels=lab, weights='volume'), dict(products=['speed'], labels=lab, weights=str(tmp_path / 'weights.npy')),
                dict(products=['speed'], labels=lab.astype(np.float32)), dict(products=['speed'], labels=lab, thresholds={'speed': [float('inf')]})):
        m.inference_cfg['regions'] = bad
        with pytest.raises(ValueError):
            m.run_inference_interface(**nothing)
    for good in (dict(products=['speed', 'T'], labels=str(tmp_path / 'labels.npy'), weights='area', thresholds={'T': [273.15]}),
                 dict(products=['speed'], labels=str(tmp_path / 'small.npy'))):                # (its shape is the first sample's to refuse)
        m.inference_cfg['regions'] = good
        with pytest.raises(NotImplementedError):                         # now the missing checkpoint is what stops it
            m.run_inference_interface(**nothing)
    m.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    assert m.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None and m.last_regions is None


def test_infer_launcher_flags_reach_the_regions_key():
    import infer
    args = infer.parse.parse_args([])
    assert args.regions is None and args.region_threshold == [] and infer.regions_option(args) is None
    args = infer.parse.parse_args(['--regions', 'speed,T', '--region_labels', 'a.npy', '--synthetic'])
    assert infer.regions_option(args) == dict(products=['speed', 'T'], labels='a.npy', weights=None, thresholds={})
    args = infer.parse.parse_args(['--regions', 'vorticity,T', '--region_labels', 'a.npy', '--region_weights', 'area', '--region_threshold', 'T:273.15,300',
                                   '--region_threshold', 'vorticity:1e-5'])
    assert infer.regions_option(args) == dict(products=['vorticity', 'T'], labels='a.npy', weights='area', thresholds={'T': [273.15, 300.0], 'vorticity': [1e-5]})
    assert infer.regions_option(infer.parse.parse_args(['--regions', 'T', '--region_labels', 'a.npy', '--region_weights', 'w.npy']))['weights'] == 'w.npy'
    for bad in (['--regions', 'speed'], ['--region_labels', 'a.npy'], ['--region_weights', 'area'], ['--region_threshold', 'speed:10'],
                ['--regions', 'speed', '--region_labels', 'a.npy', '--region_threshold', 'speed'],
                ['--regions', 'speed', '--region_labels', 'a.npy', '--region_threshold', ':3']):
        with pytest.raises(SystemExit):
            infer.regions_option(infer.parse.parse_args(bad))
    src = open(os.path.join(ROOT, 'infer.py')).read()
    assert "['regions'] = regions_option(args)" in src                    # ... and the launcher puts it into inference_cfg
    assert infer.ensemble_option(infer.parse.parse_args(['--ensemble', 'T', '--ensemble_threshold', 'T:280'])) == dict(products=['T'], thresholds={'T': [280.0]})
