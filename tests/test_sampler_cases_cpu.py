"""CPU: the host models, the oracle wrapper and the bars of tests/sampler_cases.py, before tests/test_gpu_sampler_cases.py holds the kernels to them.
  * Philox-4x32-10 against the Random123 known answers; u53 and below at their edges;
  * the scipy oracle is finite at every fine node of every geometry (no case is ever skipped for NaN);
  * the numpy fp64 model of sample_point meets every bar against the oracle on every geometry and cube, nodes and stations;
  * each seeded mistake breaks a condition on at least one case -- among them today's exact inside test, which loses the last row and column of
    the 0.1 / 0.3 and 0.1 / 0.7 degree geometries."""
import numpy as np
import pytest

import sampler_cases as C

RATIOS = {}


def test_philox_known_answers():
    for counter, key, want in C.PHILOX_KNOWN_ANSWERS:
        assert C.philox4x32_10(counter, key) == want, (counter, key)


def test_u53_and_below_edges():
    assert C.u53(0, 0) == 0.0 and C.u53(C.MASK32, C.MASK32) == 1.0 - 2.0 ** -53
    assert C.u53(0, 1 << 11) == 2.0 ** -53 and C.u53(0, (1 << 11) - 1) == 0.0          # the low 11 bits of lo are dropped
    assert C.u53(1, 0) == 2.0 ** -32 and C.u53(1 << 31, 0) == 0.5
    assert C.u53(0x6627e8d5, 0xe169c58d) == float((0x6627e8d5 << 21) ^ (0xe169c58d >> 11)) / 2.0 ** 53
    for n in (1, 2, 10, 25, 257):
        assert C.below(0, n) == 0 and C.below(C.MASK32, n) == n - 1
        edges = [((k << 32) + n - 1) // n for k in range(1, n)]                          # the smallest word that gives k
        assert all(C.below(w, n) == k and C.below(w - 1, n) == k - 1 for k, w in enumerate(edges, start=1))


def test_draws_use_the_documented_counter_key_and_streams():
    g = C.GEO['r01_03']
    s = g.struct()
    raw = C.draws(C.INTERIOR, 0, 0, 0, 0, 3, g)
    assert raw[0, 0] == C.u53(0x6627e8d5, 0xe169c58d) * (s.lon - 1) and raw[0, 1] == C.u53(0xbc57ac4c, 0x9b00dbd8) * (s.lat - 1)
    seed, off = 2 ** 32 + 5, 2 ** 32 - 2
    raw = C.draws(C.MARGIN, seed, off, 0, 0, 4, g)
    for i in range(4):                                            # the carry into the high counter word falls inside the batch
        ctr = off + i
        w = C.philox4x32_10((ctr & C.MASK32, ctr >> 32, 0, 0), (5, 1))
        v = C.philox4x32_10((ctr & C.MASK32, ctr >> 32, 1, 0), (5, 1))
        assert tuple(raw[i]) == ((w[0] * 10) >> 32, (w[2] * 16) >> 32, (v[0] * 25) >> 32)
    assert np.array_equal(C.draws(C.MARGIN, 7, 5, 3, 2 ** 31, 8, g), C.draws(C.MARGIN, 7, 5 + 3 * 2 ** 31, 0, 0, 8, g))
    assert np.array_equal(C.draws(C.MARGIN, 7, 2 ** 64 - 2, 0, 0, 4, g)[2:], C.draws(C.MARGIN, 7, 0, 0, 0, 2, g))     # wraps modulo 2^64
    u = C.select_uniforms(seed, off, 0, 0, 4)
    for j in range(4):
        w = C.philox4x32_10(((off + j) & C.MASK32, (off + j) >> 32, 2, 0), (5, 1))
        assert u[j] == C.u53(w[0], w[1])


def test_margin_draws_of_the_small_geometry_reach_both_end_nodes_and_every_hour():
    """What the GPU test relies on when it compares 4096 MARGIN draws with the model instead of testing a distribution."""
    g = C.GEO['r01_03']
    raw = C.draws(C.MARGIN, 1, 0, 0, 0, 4096, g)
    assert set(raw[:, 0]) == set(range(g.lon)) and set(raw[:, 1]) == set(range(g.lat)) and set(raw[:, 2]) == set(range(g.t_hours + 1))


def test_geometry_table():
    names = [g.name for g in C.GEOMETRIES]
    assert names[0] == 'default' and len(set(names)) == len(names) == 8
    for g in C.GEOMETRIES:
        s = g.struct()
        assert (s.lon, s.lat, s.lon_in, s.lat_in, s.t_in, s.t_hours) == (g.lon, g.lat, g.lon_in, g.lat_in, g.t_in, g.t_hours)
        assert g.name == 'default' or g.n_nodes() <= 400
        assert float(np.float32(g.dx)) == g.dx and float(np.float32(g.dy)) == g.dy
        assert C.axis_allowance_holds(g), g.name
        # the fine grid spans the coarse cube on both axes (the last node lies on the cube's last face)
        assert abs((g.lon - 1) * g.out_res - (g.lon_in - 1) * g.in_res_x) < 1e-9 and abs((g.lat - 1) * g.out_res - (g.lat_in - 1) * g.in_res_y) < 1e-9
    m, a, e, t3 = C.GEO['minimal'].struct(), C.GEO['aniso'].struct(), C.GEO['equator'], C.GEO['t3'].struct()
    assert (m.lon_in, m.lat_in, m.t_in) == (2, 2, 2)
    assert a.cells_x != a.cells_y and a.dx != a.dy
    assert e.begin_lat < 0.0 < e.begin_lat + (e.lat - 1) * e.out_res
    assert t3.t_step_hours == 3.0 and t3.t_in == 4
    for n in C.NON_DYADIC:                                         # where the kernel's fx of the last node exceeds the last face
        s = C.GEO[n].struct()
        assert (s.lon - 1) * s.cells_x > s.lon_in - 1 or (s.lat - 1) * s.cells_y > s.lat_in - 1


@pytest.mark.parametrize('geo', C.GEOMETRIES, ids=lambda g: g.name)
def test_oracle_is_finite_at_every_fine_node(geo):
    """A condition, not a measurement: no geometry of the table may lose a node to the oracle's own bounds check."""
    xi, yi, ti = C.node_points(geo)
    cd = C.oracle_points(geo, C.cube(geo.name, 'normal'), xi, yi, ti)[4]
    assert cd.shape == (xi.size, 6) and np.isfinite(cd).all()
    assert (xi[-1], yi[-1], ti[-1]) == (geo.lon - 1, geo.lat - 1, geo.t_hours)


@pytest.mark.parametrize('kind', C.CUBES)
@pytest.mark.parametrize('geo', C.GEOMETRIES, ids=lambda g: g.name)
def test_model_meets_every_bar(geo, kind):
    cube = C.cube(geo.name, kind)
    xi, yi, ti = C.node_points(geo)
    res = C.check_points(geo, cube, xi, yi, ti, C.sample_model(geo, cube, xi, yi, ti))
    assert C.passes(res) and res['n_nan'] == 0, res
    RATIOS['%s %s nodes' % (geo.name, kind)] = (res['cd_ratio'], res['f_ratio'], res['n_differ'], res['n_compared'])
    xr, yr, tr, n_out = C.station_points(geo)
    got = C.sample_model(geo, cube, xr, yr, tr)
    res = C.check_points(geo, cube, xr, yr, tr, got)
    assert C.passes(res) and res['n_nan'] == 6 * n_out, res
    assert np.isnan(got[4][-n_out:]).all()
    RATIOS['%s %s stations' % (geo.name, kind)] = (res['cd_ratio'], res['f_ratio'], res['n_differ'], res['n_compared'])
    lx, ly, lt = C.lattice_positions(C.lattice_of(geo))
    res = C.check_points(geo, cube, lx, ly, lt, C.sample_model(geo, cube, lx, ly, lt))
    assert C.passes(res) and res['n_nan'] == 0, res
    RATIOS['%s %s lattice' % (geo.name, kind)] = (res['cd_ratio'], res['f_ratio'], res['n_differ'], res['n_compared'])
    # the two sides of the inside rule: 1e-10 of a cell beyond a face is on the face, 1e-8 beyond is NaN; the exact comparison loses the former
    pts = C.tolerance_points(geo)[0]
    pattern, ratio, differ = C.check_tolerance_points(geo, cube, C.sample_model(geo, cube, *pts)[4])
    assert pattern and ratio <= 1.0, (pattern, ratio)
    RATIOS['%s %s tolerance' % (geo.name, kind)] = (ratio, 0.0, differ, 6 * int(C.tolerance_points(geo)[1].sum()))
    assert not C.check_tolerance_points(geo, cube, C.sample_model(geo, cube, *pts, mistakes=('half_open',))[4])[0]


def test_the_clamp_is_the_identity_on_the_default_geometry():
    """Weights already in [0, 1] are used unchanged: with and without the tolerance the model gives the same bits at every node and station."""
    geo = C.GEO['default']
    cube = C.cube('default', 'normal')
    for pts in (C.node_points(geo), C.station_points(geo)[:3]):
        a, b = C.sample_model(geo, cube, *pts)[4], C.sample_model(geo, cube, *pts, mistakes=('half_open',))[4]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('name', C.NON_DYADIC)
def test_exact_inside_test_loses_the_last_row_and_column(name):
    """Putting back the exact comparison (the model's 'half_open' switch) makes the last-node checks fail on the cell ratios that are no binary
    fractions: the oracle is finite there, the model NaN."""
    geo = C.GEO[name]
    cube = C.cube(name, 'normal')
    xi, yi, ti = C.node_points(geo)
    cd = C.sample_model(geo, cube, xi, yi, ti, mistakes=('half_open',))[4]
    lost = np.isnan(cd).any(axis=1)
    assert lost[-1] and lost.any() and not np.isnan(C.sample_model(geo, cube, xi, yi, ti)[4]).any()
    edge = (xi == geo.lon - 1) | (yi == geo.lat - 1)
    assert not lost[~edge].any()
    if name == 'r01_03':
        assert lost[ti == 0].sum() == 25 and np.array_equal(lost, edge)              # 25 of the 160 nodes of a plane
    res = C.check_points(geo, cube, xi, yi, ti, C.sample_model(geo, cube, xi, yi, ti, mistakes=('half_open',)))
    assert not res['nan_match'] and not C.passes(res)


def _point_cases():
    for geo in C.GEOMETRIES:
        for kind in C.CUBES:
            yield geo, kind, 'nodes', C.node_points(geo)
            yield geo, kind, 'stations', C.station_points(geo)[:3]


@pytest.mark.parametrize('mistake', ('swap_xy_weights', 'time_unclamped', 'half_open'))
def test_seeded_value_mistakes_are_caught(mistake):
    caught = []
    for geo, kind, what, pts in _point_cases():
        if geo.name == 'default' and what == 'nodes' and kind == 'scaled':
            continue                                               # (the large case once is enough here)
        cube = C.cube(geo.name, kind)
        res = C.check_points(geo, cube, *pts, C.sample_model(geo, cube, *pts, mistakes=(mistake,)))
        if not C.passes(res):
            caught.append((geo.name, kind, what))
    assert caught, mistake
    if mistake == 'half_open':
        assert {c[0] for c in caught} == set(C.NON_DYADIC)


@pytest.mark.parametrize('mistake', ('drop_high_counter', 'one_stream', 'u53_no_low', 'below_modulo'))
def test_seeded_draw_mistakes_are_caught(mistake):
    """The draw cases of the GPU test: a generator with the mistake differs from the model on at least one of them."""
    g = C.GEO['r01_03']
    caught = []
    for mode in (C.INTERIOR, C.MARGIN):
        for seed in (0, 1, 2 ** 32 + 5, 2 ** 64 - 1):
            for off in (0, 2 ** 32 - 300, 2 ** 40 + 7):
                if not np.array_equal(C.draws(mode, seed, off, 0, 0, 600, g), C.draws(mode, seed, off, 0, 0, 600, g, mistakes=(mistake,))):
                    caught.append((mode, seed, off))
    assert caught, mistake
    if mistake == 'drop_high_counter':
        assert {c[2] for c in caught} == {2 ** 32 - 300, 2 ** 40 + 7}
        assert not np.array_equal(C.select_uniforms(1, 2 ** 32 - 100, 0, 0, 300), C.select_uniforms(1, 2 ** 32 - 100, 0, 0, 300, mistakes=(mistake,)))
    if mistake == 'u53_no_low':
        assert {c[0] for c in caught} == {C.INTERIOR}
        assert not np.array_equal(C.select_uniforms(1, 0, 0, 0, 300), C.select_uniforms(1, 0, 0, 0, 300, mistakes=(mistake,)))


def test_seeded_label_stride_mistake_is_caught():
    for name in ('r01_03', 'aniso'):
        geo = C.GEO[name]
        assert geo.lon != geo.lat
        xi, yi, ti = C.node_points(geo)
        want = C.SO.labels_at(C.labels(name), xi, yi, ti)
        assert np.array_equal(C.labels_model(geo, C.labels(name), xi, yi, ti), want)
        assert not np.array_equal(C.labels_model(geo, C.labels(name), xi, yi, ti, mistakes=('label_strides_swapped',)), want)


def test_denorm_model_and_its_placements():
    """denorm_model against oracle.grid_maps where that can say it (affine), against fp64 within one rounding per operation for the squared form;
    NaN passes the clip, +-inf lands on the bounds; the map-order mistake is caught."""
    out = C.denorm_inputs(15)
    t = C.PHYS_TABLES['affine']
    for clip in (False, True):
        want = C.SO.grid_maps(out, 5, 3, t['mean'], t['std'], t['clip_lo'], t['clip_hi'], clip)
        got = C.grid_maps_model(out, 5, 3, 'affine', clip)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for xx in range(5):
        for yy in range(3):
            assert np.array_equal(got[:, yy, xx].view(np.uint32), C.denorm_model(out[xx * 3 + yy], 'affine', True).view(np.uint32))
    out = C.denorm_inputs(600, 1)
    t = C.PHYS_TABLES['squared']
    for clip in (False, True):
        v = C.denorm_model(out, 'squared', clip)
        assert np.array_equal(np.isnan(v), np.isnan(out))
        for k in range(6):
            col = out[:, k].astype(np.float64)
            a = np.float32(t['std'][k]).astype(np.float64) * col + np.float64(np.float32(t['mean'][k]))
            if t['sq_on'][k]:
                a = a * a + np.float64(np.float32(t['sq_add'][k]))
            if clip and k >= 2:
                a = np.clip(a, np.float32(t['clip_lo'][k]), np.float32(t['clip_hi'][k]))
            fin = np.isfinite(col)
            scale = np.abs(col * t['std'][k]) + abs(t['mean'][k])
            scale = scale * scale + abs(t['sq_add'][k]) if t['sq_on'][k] else scale
            assert np.all(np.abs(v[fin, k] - a[fin]) <= 6 * 2.0 ** -24 * scale[fin]), (clip, k)
            inf = np.isinf(col)
            if clip and k >= 2:
                hi, lo = np.float32(t['clip_hi'][k]), np.float32(t['clip_lo'][k])
                assert np.all(v[inf & (col > 0), k] == hi) and np.all(v[inf & (col < 0), k] == (hi if t['sq_on'][k] else lo))
            else:
                assert np.isinf(v[inf, k]).all()
        assert clip is False or ((v[:, 4] == np.float32(t['clip_hi'][4])).any() and (v[:, 4] == np.float32(t['clip_lo'][4])).sum() == 0)
    lat = C.lattice_of(C.GEO['r01_03'])
    out = C.denorm_inputs(42, 2)
    whole = C.fields_out_model(out, 'affine', True, lat, 0, np.full((2, 6, 3, 7), C.SENTINEL, np.float32))
    rows = C.fields_out_model(out, 'affine', True)
    assert np.array_equal(whole.transpose(0, 2, 3, 1).reshape(42, 6).view(np.uint32), rows.view(np.uint32))
    for first, n in C.LATTICE_CHUNKS:
        part = C.fields_out_model(out[first:first + n], 'affine', True, lat, first, np.full((2, 6, 3, 7), C.SENTINEL, np.float32))
        seen = part.transpose(0, 2, 3, 1).reshape(42, 6)
        assert np.array_equal(seen[first:first + n].view(np.uint32), rows[first:first + n].view(np.uint32))
        rest = np.delete(seen, np.arange(first, first + n), axis=0)
        assert (rest.view(np.uint32) == C.SENTINEL_BITS).all()
        bad = C.fields_out_model(out[first:first + n], 'affine', True, lat, first, np.full((2, 6, 3, 7), C.SENTINEL, np.float32),
                                 mistakes=('map_order_swapped',))
        assert not np.array_equal(bad.view(np.uint32), part.view(np.uint32))


def test_every_seeded_mistake_has_a_test():
    assert set(C.MISTAKES) == {'drop_high_counter', 'one_stream', 'u53_no_low', 'below_modulo', 'swap_xy_weights', 'time_unclamped', 'half_open',
                               'label_strides_swapped', 'map_order_swapped'}


def test_zz_summary_of_error_to_bar_ratios():
    """Printed for the reviewer: how much of each bar the fp64 model uses against the scipy oracle (of the cases that ran in this process)."""
    print()
    for k in sorted(RATIOS):
        r = RATIOS[k]
        print('model error / bar   %-28s coord_data %.4f   f %.4f   differing %d of %d' % (k, r[0], r[1], r[2], r[3]))
        assert max(r[:2]) <= 1.0
