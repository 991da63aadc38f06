"""GPU (MI355X): the inference run with all eight product keys in ONE call -- InterfacePhysics.run_inference_interface through its public surface only
(hi+lo mode).  The launcher tests of the products switch on one key each; here every key is on at once: the files it writes (names written out
literally from the patterns of the products' paragraphs, bytes against the `last_*` results), every key alone against the all-keys run (no product
disturbs another; "equal" is bit for bit, which NaN-holding tables need and torch.equal cannot give), and the order of the launches.

Two synthetic samples, nt = 3 (dt = 12 h in the 24 h window), the 145 x 257 lattice; sample 1's first stamp is sample 0's last, as with every dt
that divides the window."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S0 = ['2022-03-25_00_00_00', '2022-03-25_12_00_00', '2022-03-26_00_00_00']           # the stamps of sample 0
S1 = ['2022-03-26_00_00_00', '2022-03-26_12_00_00', '2022-03-27_00_00_00']           # ... and of sample 1, the last one
LAST = ('last_diagnostics', 'last_trajectories', 'last_ensemble', 'last_verification', 'last_grid_verification', 'last_regions', 'last_extremes',
        'last_spells')
VERIFY_SCORES = ('count', 'bias', 'mae', 'rmse', 'max_abs_error', 'corr', 'base_bias', 'base_mae', 'base_rmse', 'skill', 'pod', 'far', 'csi', 'fbias', 'ets',
                 'base_pod', 'base_far', 'base_csi', 'base_fbias', 'base_ets')
PVERIFY_SCORES = ('count', 'crps', 'fair_crps', 'bias', 'rmse', 'spread', 'spread_skill', 'base_crps', 'base_fair_crps', 'base_bias', 'base_rmse',
                  'base_spread', 'base_spread_skill', 'crpss', 'fair_crpss', 'rank_hist', 'base_rank_hist', 'brier', 'reliability', 'resolution', 'bss',
                  'roc_area', 'base_brier', 'base_reliability', 'base_resolution', 'base_bss', 'base_roc_area', 'uncertainty', 'rel_n', 'rel_o',
                  'base_rel_n', 'base_rel_o')
NBHD_SCORES = ('fss', 'base_fss', 'windows', 'freq_f', 'freq_b', 'freq_o', 'fbias', 'base_fbias', 'useful', 'count', 'skilful_scale', 'base_skilful_scale')
REGION_KEYS = ('mean', 'total', 'weight', 'min', 'max', 'where_min', 'where_max', 'count')
EXTREME_KEYS = ('value', 'hour', 'lo', 'hi', 'status')
SPELL_KEYS = ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess', 'crossings', 'status')
TRAJ_WORDS = ('positions', 'hours', 'status', 'steps', 'fields')
GROUPS = ('point', 'station', 'hour', 'all')

# the files of the all-keys run, by key; 'variables' are written with every key
FILES = {
    'variables': ['%s_T.npy' % t for t in S0 + S1[1:]],
    'diagnostics': ['%s_%s.npy' % (t, n) for t in S0 + S1[1:] for n in ('vorticity', 'dT_dt')],
    'trajectories': ['%s_traj_%s.npy' % (t, w) for t in (S0[0], S1[0]) for w in TRAJ_WORDS],
    'ensemble': ['%s_ens_%s_%s.npy' % (t, k, n) for t in S0 for k in ('mean', 'spread', 'min', 'max', 'count') for n in ('speed', 'T')]
                + ['%s_ens_prob_speed_gt_3.npy' % t for t in S0],
    'verify': ['%s_verify_%s_%s.npy' % (S0[0], g, k) for g in GROUPS for k in VERIFY_SCORES],
    'verify_grid': ['%s_nbhd_%s_%s.npy' % (S0[0], g, k) for g in ('hour', 'all') for k in NBHD_SCORES],
    'regions': ['%s_region_%s_%s.npy' % (t, k, n) for t in (S0[0], S1[0]) for k in REGION_KEYS for n in ('speed', 'T')]
               + ['%s_region_frac_T_gt_280.npy' % t for t in (S0[0], S1[0])],
    'extremes': ['%s_extreme_%s_%s.npy' % (t, k, c) for t in (S0[0], S1[0]) for k in EXTREME_KEYS for c in ('T_max', 'speed_max')],
    'spells': ['%s_spell_%s_T_below_273.15.npy' % (t, k) for t in (S0[0], S1[0]) for k in SPELL_KEYS],
}

# the launches of the all-keys run as (entry point, consecutive calls), recorded before the run became a loop over the product table: per sample
# predict_lattice, diagnostic_lattice, trajectories, extreme_lattice, spell_lattice, regional_lattice; behind the loop ensemble_lattice, verify_at,
# verify_lattice
SPIED = ('dpn_fields_out', 'dpn_diagnostics_out', 'dpn_traj_stage', 'dpn_extreme_scan', 'dpn_spell_scan', 'dpn_region_accumulate', 'dpn_region_finish',
         'dpn_ensemble_accumulate', 'dpn_ensemble_finish', 'dpn_verify_accumulate', 'dpn_verify_pool', 'dpn_verify_finish', 'dpn_nbhd_stage', 'dpn_nbhd_fold',
         'dpn_nbhd_finish')
LAUNCHES = ([('dpn_fields_out', 1), ('dpn_diagnostics_out', 1), ('dpn_traj_stage', 13), ('dpn_extreme_scan', 5), ('dpn_spell_scan', 5),
             ('dpn_region_accumulate', 1), ('dpn_region_finish', 1)] * 2                                               # two samples
            + [('dpn_ensemble_accumulate', 2), ('dpn_ensemble_finish', 1)]
            + [('dpn_verify_accumulate', 2), ('dpn_verify_finish', 1)] + [('dpn_verify_pool', 1), ('dpn_verify_finish', 1)] * 3       # three groupings
            + [('dpn_nbhd_stage', 1), ('dpn_nbhd_fold', 1)] * 2 + [('dpn_nbhd_finish', 1)])                               # two cases


def _options(tmp_path, members=1):
    """The smallest requests that still exercise the name building, by key."""
    g = np.random.default_rng(31)
    lab = np.full((145, 257), -1, dtype=np.int64)
    lab[10:70, 20:120], lab[80:140, 130:250] = 0, 1
    np.save(tmp_path / 'labels.npy', lab)
    obs = dict(lon=np.array([80.5, 100.25, 120.0]), lat=np.array([22.0, 30.25, 45.5]), hours=np.array([0.0, 12.0]), names=np.array(['T']),
               obs=(g.standard_normal((2 // members, 2, 3, 1)) * 5.0 + 280.0).astype(np.float32))
    analysis = dict(names=np.array(['T']), hours=np.array([0.0, 12.0]), analysis=(g.standard_normal((2, 2, 1, 145, 257)) * 5.0 + 280.0).astype(np.float32))
    return {
        'diagnostics': ['vorticity', 'dT_dt'],
        'trajectories': dict(lonlat=[(100.5, 30.25), (110.0, 35.0)], start=0.0, hours=3.0, step=1.0),
        'ensemble': dict(products=['speed', 'T'], thresholds={'speed': [3.0]}),
        'verify': dict(products=['T'], obs=obs, thresholds={'T': ('below', 280.0)}, by=['station', 'hour', 'all'], **({'members': members} if members > 1 else {})),
        'verify_grid': dict(products=['T'], analysis=analysis, thresholds={'T': ('below', 280.0)}, scales=[1, 3]),
        'regions': dict(products=['speed', 'T'], labels=str(tmp_path / 'labels.npy'), weights='area', thresholds={'T': [280.0]}),
        'extremes': dict(columns=['T:max', 'speed:max'], window=(0.0, 24.0), scan_hours=6.0, refine=2),
        'spells': dict(columns=['T:below:273.15'], window=(0.0, 24.0), scan_hours=6.0, refine=2),
    }


def _model(tmp_path, results, options):
    """The launcher tests' model (seed 4, with_clip, a checkpoint of its own weights) with the product keys of `options` set."""
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    cfg = ncep_config()
    cfg['inference_cfg'].update(img_size=(145, 257), refine=1, dt=43200)
    cfg['inference_cfg']['log'].update(write_source=True, result_path=str(results), export_variable=['T'])
    for key, opt in options.items():
        if key == 'diagnostics':
            cfg['inference_cfg']['log']['export_diagnostic'] = opt
        else:
            cfg['inference_cfg'][key] = opt
    torch.manual_seed(4)
    m = builder_models(**cfg)
    m.with_clip = True
    if not (tmp_path / 'ckpt' / 'physics_latest.pth').exists():
        (tmp_path / 'ckpt').mkdir()
        m.save_model(str(tmp_path / 'ckpt'), epoch=0, global_step=1, prefix='physics')
    return m


class _Spy:
    """Records calls of the products' entry points on the loaded library (the spy of tests/test_gpu_regions.py)."""

    def __init__(self):
        from deepphysinet_amd import _lib as L
        self.lib, self.calls = L.load(), []
        self.inner = {name: getattr(self.lib, name) for name in SPIED}

    def __enter__(self):
        for name, fn in self.inner.items():
            setattr(self.lib, name, lambda *a, _n=name, _f=fn: (self.calls.append(_n), _f(*a))[1])
        return self

    def __exit__(self, *exc):
        for name, fn in self.inner.items():
            setattr(self.lib, name, fn)

    def runs(self):
        """The calls as (name, consecutive repeats)."""
        out = []
        for name in self.calls:
            if out and out[-1][0] == name:
                out[-1] = (name, out[-1][1] + 1)
            else:
                out.append((name, 1))
        return out


def _run(m, tmp_path):
    return m.run_inference_interface(checkpoint_path=str(tmp_path / 'ckpt'), samples='synthetic', samples_per_epoch=2)


def _host(v):
    """A result with its tensors as host arrays (dicts, lists and tuples walked; names, thresholds and None as they are)."""
    if torch.is_tensor(v):
        return v.cpu().numpy()
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    return type(v)(_host(x) for x in v) if isinstance(v, (list, tuple)) else v


def _same(a, b):
    """Bit for bit: arrays by dtype, shape and bytes; containers member by member."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _bytes(path):
    with open(path, 'rb') as f:
        return f.read()


@pytest.fixture(scope='module')
def everything(tmp_path_factory):
    """The all-keys run, once: its folder, model, returned maps, `last_*` on the host and recorded launches."""
    tmp_path = tmp_path_factory.mktemp('inference_run')
    m = _model(tmp_path, tmp_path / 'all', _options(tmp_path))
    with _Spy() as spy:
        maps = _run(m, tmp_path)
    return dict(tmp_path=tmp_path, out=tmp_path / 'all', m=m, maps=maps, last={k: _host(getattr(m, k)) for k in LAST}, launches=spy.runs())


def test_all_keys_in_one_run_write_their_files_from_their_results(everything):
    from deepphysinet_amd.sampler import SyntheticSamples
    out, m, last = everything['out'], everything['m'], everything['last']
    assert sorted(os.listdir(out)) == sorted(fn for names in FILES.values() for fn in names)
    load = lambda *parts: np.load(out / ('_'.join(parts) + '.npy'))
    maps = everything['maps']
    host = maps.cpu().numpy()
    d, tr, e, v, gv, r = (last[k] for k in LAST[:6])
    for it, t in enumerate(S1):                                            # the last sample's maps, every time step
        assert _same(load(t, 'T'), host[it, 3])
        for j, name in enumerate(('vorticity', 'dT_dt')):
            assert d['names'] == ['vorticity', 'dT_dt'] and _same(load(t, name), d['maps'][it, j]), (t, name)
    for word, key in zip(TRAJ_WORDS, ('positions', 'hours', 'status', 'steps_done', 'fields')):
        assert _same(load(S1[0], 'traj', word), tr[key]), word
    assert tr['positions'].shape == (4, 2, 2) and tr['fields'].shape == (4, 2, 6)
    for it, t in enumerate(S0):                                            # the first sample's stamps
        for j, name in enumerate(('speed', 'T')):
            for key in ('mean', 'spread', 'min', 'max', 'count'):
                assert _same(load(t, 'ens', key, name), e[key][it, j]), (t, key, name)
        assert _same(load(t, 'ens_prob_speed_gt_3'), e['prob'][it, 0])
    for group in GROUPS:
        for key in VERIFY_SCORES:
            assert _same(load(S0[0], 'verify', group, key), v[group][key]), (group, key)
    assert v['point']['bias'].shape == (6, 1) and v['station']['bias'].shape == (3, 1) and v['hour']['pod'].shape == (2, 1) and v['all']['count'].shape == (1, 1)
    for group in ('hour', 'all'):
        for key in NBHD_SCORES:
            assert _same(load(S0[0], 'nbhd', group, key), gv[group][key]), (group, key)
    assert gv['hour']['fss'].shape == (2, 1, 2) and gv['all']['fss'].shape == (1, 2)
    for j, name in enumerate(('speed', 'T')):
        for key in REGION_KEYS:
            a = load(S1[0], 'region', key, name)
            assert a.shape == ((3, 2, 2) if key.startswith('where') else (3, 2)) and _same(a, np.ascontiguousarray(r[key][:, :, j])), (key, name)
    assert _same(load(S1[0], 'region_frac_T_gt_280'), np.ascontiguousarray(r['frac'][:, :, 0]))
    for keys, word, result, columns in ((EXTREME_KEYS, 'extreme', last['last_extremes'], ('T_max', 'speed_max')),
                                        (SPELL_KEYS, 'spell', last['last_spells'], ('T_below_273.15',))):
        assert [k for k in result if k != 'names'] == list(keys)
        for key in keys:
            for j, column in enumerate(columns):
                a = load(S1[0], word, key, column)
                assert a.shape == (145, 257) and _same(a, result[key][j]), (word, key, column)
    # the returned maps are predict_lattice's of the last sample, called directly
    syn = SyntheticSamples(maps.device, n_margin=128, n_inter=128, leads=2)
    b = syn[1]
    lattice = syn.sampler.lattice(refine=1, hours=(0.0, 12.0, 3))
    assert maps.shape == (3, 6, 145, 257) and torch.equal(m.predict_lattice(b['field_data'], syn.sampler, lattice, b['forecast_h'], with_clip=True), maps)


def test_every_key_alone_gives_the_files_and_results_of_the_all_keys_run(everything):
    tmp_path, out = everything['tmp_path'], everything['out']
    options = _options(tmp_path)
    attribute = dict(zip(('diagnostics', 'trajectories', 'ensemble', 'verify', 'verify_grid', 'regions', 'extremes', 'spells'), LAST))
    for key, opt in options.items():
        alone = tmp_path / ('only_' + key)
        m = _model(tmp_path, alone, {key: opt})
        maps = _run(m, tmp_path)
        assert torch.equal(maps, everything['maps']), key
        assert sorted(os.listdir(alone)) == sorted(FILES['variables'] + FILES[key]), key
        for fn in os.listdir(alone):                                       # its files and the variables' files: the all-keys run's, byte for byte
            assert _bytes(alone / fn) == _bytes(out / fn), (key, fn)
        for k in LAST:
            if k == attribute[key]:
                assert _same(_host(getattr(m, k)), everything['last'][k]), key
            else:
                assert getattr(m, k) is None, (key, k)


def test_members_switch_verify_to_the_ensemble_scores(tmp_path):
    results = tmp_path / 'pverify'
    m = _model(tmp_path, results, {'verify': _options(tmp_path, members=2)['verify']})
    _run(m, tmp_path)
    v = _host(m.last_verification)
    assert v['members'] == 2 and v['names'] == ['T'] and v['thresholds'] == [('T', 'below', 280.0)]
    assert sorted(os.listdir(results)) == sorted(FILES['variables'] + ['%s_pverify_%s_%s.npy' % (S0[0], g, k) for g in GROUPS for k in PVERIFY_SCORES])
    for group in GROUPS:
        for key in PVERIFY_SCORES:
            assert _same(np.load(results / ('%s_pverify_%s_%s.npy' % (S0[0], group, key))), v[group][key]), (group, key)
    assert v['point']['crps'].shape == (6, 1) and v['all']['rank_hist'].shape == (1, 1, 3)


def test_the_launches_keep_their_order(everything):
    print('launches of the all-keys run:', everything['launches'])
    assert everything['launches'] == LAUNCHES
