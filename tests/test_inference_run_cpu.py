"""No GPU: the inference run as a loop over one table of products (deepphysinet_amd/interface/inference_run.py) -- the order of the refusals before
the checkpoint is read and the empty run with every key set, through InterfacePhysics.run_inference_interface alone; the table itself; and the
products' file functions on small fabricated results, names and shapes written out literally from the patterns of the products' paragraphs."""
import numpy as np
import pytest
import torch

H, S, P = 2, 3, 1
ORDER = ('diagnostics', 'trajectories', 'ensemble', 'verify', 'verify_grid', 'regions', 'extremes', 'spells')
LAST = ('last_diagnostics', 'last_trajectories', 'last_ensemble', 'last_verification', 'last_grid_verification', 'last_regions', 'last_extremes',
        'last_spells')


def _valid():
    """Every product key set validly: inference_cfg's part and log's part."""
    obs = dict(lon=np.array([80.5, 100.25, 120.0]), lat=np.array([22.0, 30.25, 45.5]), hours=np.array([0.0, 12.0]), names=np.array(['T']),
               obs=np.full((1, H, S, P), 280.0, dtype=np.float32))
    analysis = dict(names=np.array(['T']), hours=np.array([0.0, 12.0]), analysis=np.full((1, H, P, 145, 257), 280.0, dtype=np.float32))
    lab = np.zeros((145, 257), dtype=np.int64)
    lab[:, 128:] = 1
    return dict(trajectories=dict(lonlat=[(100.5, 30.25), (110.0, 35.0)], start=0.0, hours=3.0, step=1.0),
                ensemble=dict(products=['speed', 'T'], thresholds={'speed': [3.0]}),
                verify=dict(products=['T'], obs=obs, thresholds={'T': ('below', 280.0)}, by=['station', 'hour', 'all']),
                verify_grid=dict(products=['T'], analysis=analysis, thresholds={'T': ('below', 280.0)}, scales=[1, 3]),
                regions=dict(products=['speed', 'T'], labels=lab, weights='area', thresholds={'T': [280.0]}),
                extremes=dict(columns=['T:max', 'speed:max'], window=(0.0, 24.0), scan_hours=6.0, refine=2),
                spells=dict(columns=['T:below:273.15'], window=(0.0, 24.0), scan_hours=6.0, refine=2)), dict(export_diagnostic=['vorticity', 'dT_dt'])


# how to make each station of the refusal order bad, and what it then raises: (part, key, value or a change of the valid option, exception, match)
BAD = (('cfg', 'img_size', 'wide', NotImplementedError, r'^$'),
       ('log', 'result_path', '', ValueError, 'log.write_source needs log.result_path'),
       ('log', 'export_variable', ['T', 'gust_a'], KeyError, 'gust_a'),
       ('log', 'export_diagnostic', ['vorticity', 'gust_d'], KeyError, 'gust_d'),
       ('cfg', 'trajectories', dict(method='nope'), None, 'nope'),
       ('cfg', 'ensemble', dict(products=['speed', 'gust_e']), KeyError, 'gust_e'),
       ('cfg', 'verify', dict(products=['T', 'gust_v']), KeyError, 'gust_v'),
       ('cfg', 'verify_grid', dict(products=['T', 'gust_g']), KeyError, 'gust_g'),
       ('cfg', 'regions', dict(products=['speed', 'gust_r']), KeyError, 'gust_r'),
       ('cfg', 'extremes', dict(columns=['T:max', 'gust_x:max']), KeyError, 'gust_x'),
       ('cfg', 'spells', dict(columns=['gust_s:below:1.0']), KeyError, 'gust_s'))


@pytest.fixture(scope='module')
def model():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(0)
    return builder_models(**ncep_config())


def _configure(m, tmp_path, bad=()):
    """m.inference_cfg with all eight keys valid, then the stations `bad` of BAD made bad."""
    from deepphysinet_amd.configs import ncep_config
    cfg, log = _valid()
    ic = ncep_config()['inference_cfg']
    ic.update(cfg)
    ic['log'].update(log, write_source=True, result_path=str(tmp_path / 'never_made'), export_variable=['T'])
    for part, key, value, _, _ in bad:
        where = ic if part == 'cfg' else ic['log']
        where[key] = dict(where[key], **value) if isinstance(value, dict) else value
    m.inference_cfg = ic


def test_refusals_come_in_the_order_of_the_table_and_before_the_checkpoint(model, tmp_path):
    from deepphysinet_amd.trajectory import stage_table
    with pytest.raises(Exception) as unknown_method:
        stage_table('nope')
    nothing = dict(checkpoint_path=str(tmp_path / 'nothing_here'), device='cpu', samples=[])
    for first, second in zip(BAD[:-1], BAD[1:]):                            # both bad: the earlier one is what is refused
        _configure(model, tmp_path, (first, second))
        kind = first[3] or unknown_method.type
        with pytest.raises(kind, match=first[4]) as refused:
            model.run_inference_interface(**nothing)
        assert type(refused.value) is kind and second[4] not in str(refused.value), (first[1], second[1])
    _configure(model, tmp_path, BAD[-1:])                                   # the last station alone
    with pytest.raises(KeyError, match='gust_s'):
        model.run_inference_interface(**nothing)
    _configure(model, tmp_path)                                             # all valid: now the missing checkpoint is what stops it
    with pytest.raises(NotImplementedError, match='nothing_here'):
        model.run_inference_interface(**nothing)
    assert not (tmp_path / 'never_made').exists()


def test_all_keys_with_an_empty_source_run_through(model, tmp_path):
    model.save_model(str(tmp_path), epoch=0, global_step=1, prefix='physics')
    _configure(model, tmp_path)
    model.inference_cfg['log']['write_source'] = False
    for name in LAST:
        setattr(model, name, 'stale')
    assert model.run_inference_interface(checkpoint_path=str(tmp_path), device='cpu', samples=[]) is None
    assert [getattr(model, name) for name in LAST] == [None] * 8


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_names_the_eight_products_in_the_order_of_the_run(model):
    from deepphysinet_amd.interface.inference_run import PRODUCTS
    assert tuple(p.key for p in PRODUCTS) == ORDER and tuple(p.last for p in PRODUCTS) == LAST
    assert [p.path for p in PRODUCTS] == [('log', 'export_diagnostic')] + [(key,) for key in ORDER[1:]]
    assert [p.key for p in PRODUCTS if p.keyword] == ['verify', 'verify_grid'] == [p.key for p in PRODUCTS if p.count_check]
    assert [p.key for p in PRODUCTS if p.behind] == ['ensemble', 'verify', 'verify_grid']
    assert [p.key for p in sorted(PRODUCTS, key=lambda p: p.launch)] == ['diagnostics', 'trajectories', 'extremes', 'spells', 'regions', 'ensemble', 'verify',
                                                                        'verify_grid']       # the launches: the regions behind the time windows
    for p in PRODUCTS:
        assert p.request(model, None) is None and p.request(model, type(_valid()[0].get(p.key, []))()) is None, p.key      # absent, and empty
        assert p.last[len('last_'):] in p.doc or p.key in p.doc


def test_a_fresh_model_has_every_result_attribute():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    assert [getattr(m, name, 'missing') for name in LAST] == [None] * 8


def test_requests_prepare_what_the_calls_take(model):
    from deepphysinet_amd.interface.inference_run import PRODUCTS
    cfg, log = _valid()
    req = {p.key: p.request(model, log['export_diagnostic'] if p.key == 'diagnostics' else cfg[p.key]) for p in PRODUCTS}
    assert req['diagnostics'] == ['vorticity', 'dT_dt']
    assert req['trajectories']['method'] == 'rk4' and req['trajectories']['lon'] == [100.5, 110.0] and req['trajectories']['lat'] == [30.25, 35.0]
    assert req['ensemble'] == dict(products=['speed', 'T'], thresholds={'speed': [3.0]})
    assert req['verify']['members'] == 1 and req['verify']['reports']['obs'].shape == (1, H, S, P) and req['verify']['points'][0].shape == (H * S,)
    assert list(req['verify']['points'][3]) == ['station', 'hour', 'all']
    assert req['verify_grid']['scales'] == [1, 3] and req['verify_grid']['held']['analysis'].shape == (1, H, P, 145, 257)
    assert req['regions']['weights'] == 'area' and req['regions']['labels'].shape == (145, 257)
    assert req['extremes']['lonlat'] is None and req['spells']['refine'] == 2
    stations = PRODUCTS[6].request(model, dict(cfg['extremes'], lonlat=[(100.5, 30.25), (110.0, 35.0)]))
    assert stations['lonlat'] == [[100.5, 110.0], [30.25, 35.0]]
    # the count checks: verify_grid's and verify's texts
    by_key = {p.key: p for p in PRODUCTS}
    by_key['verify'].count_check(req['verify'], []), by_key['verify'].count_check(req['verify'], [0]), by_key['verify_grid'].count_check(req['verify_grid'], [])
    with pytest.raises(ValueError, match='the reports hold 1 cases, the sample source 2$'):
        by_key['verify'].count_check(req['verify'], [0, 1])
    with pytest.raises(ValueError, match='3 samples are not a multiple of members = 2'):
        by_key['verify'].count_check(dict(req['verify'], members=2), [0, 1, 2])
    with pytest.raises(ValueError, match='the reports hold 1 cases, the sample source 2 of 2 members'):
        by_key['verify'].count_check(dict(req['verify'], members=2), [0, 1, 2, 3])
    with pytest.raises(ValueError, match='0 samples are not|the reports hold 1 cases, the sample source 0 of 2 members'):
        by_key['verify'].count_check(dict(req['verify'], members=2), [])
    with pytest.raises(ValueError, match='the analysis holds 1 cases, the sample source 2'):
        by_key['verify_grid'].count_check(req['verify_grid'], [0, 1])


# ------------------------------------------------------------------------------------------------ the file functions
def _t(*shape, dtype=torch.float32):
    n = int(np.prod(shape))
    return torch.arange(n, dtype=torch.float64).reshape(shape).to(dtype)


def _files(key, request, result):
    """[(name, array)] of product `key` with the stamps S0, S1, ... by time step."""
    from deepphysinet_amd.interface.inference_run import PRODUCTS
    p = {p.key: p for p in PRODUCTS}[key]
    out = list(p.files(request, result, lambda it=0: 'S%d' % it))
    assert all(isinstance(a, np.ndarray) for _, a in out)
    return out


def _check(files, expected):
    """expected: [(name, the tensor or array it holds)], in order."""
    assert [name for name, _ in files] == [name for name, _ in expected]
    for (name, a), (_, want) in zip(files, expected):
        want = want.numpy() if torch.is_tensor(want) else want
        assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want), name


def test_files_of_diagnostics_trajectories_and_ensemble():
    maps = _t(2, 2, 3, 4)
    files = _files('diagnostics', ['vorticity', 'dT_dt'], dict(names=['vorticity', 'dT_dt'], maps=maps))
    _check(files, [('S0_vorticity.npy', maps[0, 0]), ('S0_dT_dt.npy', maps[0, 1]), ('S1_vorticity.npy', maps[1, 0]), ('S1_dT_dt.npy', maps[1, 1])])
    assert files[0][1].shape == (3, 4)
    tr = dict(positions=_t(4, 2, 2, dtype=torch.float64), hours=_t(4, dtype=torch.float64), status=_t(2, dtype=torch.int32),
              steps_done=_t(2, dtype=torch.int32), fields=_t(4, 2, 6), lonlat=True)
    _check(_files('trajectories', {}, tr), [('S0_traj_positions.npy', tr['positions']), ('S0_traj_hours.npy', tr['hours']), ('S0_traj_status.npy', tr['status']),
                                             ('S0_traj_steps.npy', tr['steps_done']), ('S0_traj_fields.npy', tr['fields'])])
    e = dict(mean=_t(2, 2, 3, 4), spread=_t(2, 2, 3, 4) + 1, min=_t(2, 2, 3, 4) + 2, max=_t(2, 2, 3, 4) + 3, count=_t(2, 2, 3, 4, dtype=torch.int32),
             prob=_t(2, 2, 3, 4) + 4, names=['speed', 'T'], thresholds=[('speed', 3.0), ('T', 273.15)])
    expected = []
    for it in (0, 1):
        for j, name in enumerate(('speed', 'T')):
            expected += [('S%d_ens_%s_%s.npy' % (it, key, name), e[key][it, j]) for key in ('mean', 'spread', 'min', 'max', 'count')]
        expected += [('S%d_ens_prob_speed_gt_3.npy' % it, e['prob'][it, 0]), ('S%d_ens_prob_T_gt_273.15.npy' % it, e['prob'][it, 1])]
    _check(_files('ensemble', {}, e), expected)
    assert expected[0][0] == 'S0_ens_mean_speed.npy' and expected[-3][0] == 'S1_ens_count_T.npy'
    assert [n for n, _ in _files('ensemble', {}, dict(e, prob=None, thresholds=[]))] == [n for n, _ in expected if '_prob_' not in n]


def test_files_of_the_two_verifications():
    groups = {'station': np.arange(6) % 3, 'all': np.zeros(6, dtype=np.int64)}
    points = (np.zeros(6), np.zeros(6), np.zeros(6), groups)
    table = lambda G: dict(count=_t(G, 1, dtype=torch.int32), crps=_t(G, 1), brier=None, rank_hist=_t(G, 1, 3, dtype=torch.int32))
    v = dict(names=['T'], thresholds=[], members=2, point=table(6), station=table(3), all=table(1))
    want = [('S0_%s_%s_%s.npy' % ('%s', g, k), v[g][k]) for g in ('point', 'station', 'all') for k in ('count', 'crps', 'rank_hist')]      # None: no file
    _check(_files('verify', dict(members=2, points=points), v), [(n % 'pverify', a) for n, a in want])
    _check(_files('verify', dict(members=1, points=points), v), [(n % 'verify', a) for n, a in want])
    assert want[0][0] % 'pverify' == 'S0_pverify_point_count.npy' and want[-1][0] % 'verify' == 'S0_verify_all_rank_hist.npy'
    gv = dict(names=['T'], scales=[1, 3], hour=dict(fss=_t(2, 1, 2), count=_t(2, 1, dtype=torch.int64)), all=dict(fss=_t(1, 2), count=_t(1, dtype=torch.int64)))
    _check(_files('verify_grid', {}, gv), [('S0_nbhd_hour_fss.npy', gv['hour']['fss']), ('S0_nbhd_hour_count.npy', gv['hour']['count']),
                                           ('S0_nbhd_all_fss.npy', gv['all']['fss']), ('S0_nbhd_all_count.npy', gv['all']['count'])])


def test_files_of_regions_and_of_the_time_windows():
    keys = ('mean', 'total', 'weight', 'min', 'max', 'where_min', 'where_max', 'count')
    r = {k: _t(3, 2, 2, 2, dtype=torch.int32) if k.startswith('where') else _t(3, 2, 2, dtype=torch.int32 if k == 'count' else torch.float32) for k in keys}
    r.update(frac=_t(3, 2, 2), names=['speed', 'T'], thresholds=[('T', 280.0), ('T', 273.15)])
    expected = [('S0_region_%s_%s.npy' % (k, name), r[k][:, :, j].numpy()) for k in keys for j, name in enumerate(('speed', 'T'))]
    expected += [('S0_region_frac_T_gt_280.npy', r['frac'][:, :, 0].numpy()), ('S0_region_frac_T_gt_273.15.npy', r['frac'][:, :, 1].numpy())]
    files = _files('regions', {}, r)
    _check(files, expected)
    assert files[0][0] == 'S0_region_mean_speed.npy' and files[0][1].shape == (3, 2) and dict(files)['S0_region_where_max_T.npy'].shape == (3, 2, 2)
    for key, word, results, columns, suffixes in (('extremes', 'extreme', ('value', 'hour', 'lo', 'hi', 'status'), ['T:max', 'speed:max'], ('T_max', 'speed_max')),
                                                  ('spells', 'spell', ('hours', 'first', 'last', 'first_lo', 'last_hi', 'excess', 'crossings', 'status'),
                                                   ['T:below:273.15', 'speed:above:15'], ('T_below_273.15', 'speed_above_15'))):
        at = dict({k: _t(3, 2, dtype=torch.int32 if k in ('status', 'crossings') else torch.float64) for k in results}, names=columns)      # stations: [N, C]
        _check(_files(key, dict(lonlat=[[100.5], [30.25]]), at), [('S0_%s_%s.npy' % (word, k), at[k]) for k in results])
        on = dict({k: _t(2, 3, 4) for k in results}, names=columns)                                                                          # maps: [C, ny, nx]
        _check(_files(key, dict(lonlat=None), on), [('S0_%s_%s_%s.npy' % (word, k, s), on[k][j]) for k in results for j, s in enumerate(suffixes)])
    assert _files('spells', dict(lonlat=None), on)[1][0] == 'S0_spell_hours_speed_above_15.npy' and _files('spells', dict(lonlat=[[1.0], [2.0]]), at)[0][0] == 'S0_spell_hours.npy'
