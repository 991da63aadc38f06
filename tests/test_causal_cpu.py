"""CPU: the host references of deepphysinet_amd.causal (what the GPU tests hold the kernels of csrc/dpn_causal.hip to), the option's value type, and the
build of the unit: it cross-compiles for gfx950, no kernel spills or uses scratch, and the entry points are exported as _lib.py declares them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ host references
def test_eps_zero_gives_all_ones_and_weights_start_at_one_and_never_increase():
    from deepphysinet_amd.causal import bin_weights_reference
    rng = np.random.default_rng(0)
    s, b = rng.random(500) * 1e6, rng.integers(0, 16, 500)
    for relative in (True, False):
        W, l, count = bin_weights_reference(s, b, 16, 0.0, relative)
        assert (W == 1.0).all() and count.sum() == 500
        for eps in (1e-7, 0.5, 5.0):
            W, l2, _ = bin_weights_reference(s, b, 16, eps, relative)
            assert W[0] == 1.0 and (np.diff(W) <= 0).all() and (W >= 0).all()
            np.testing.assert_array_equal(l2, l)                         # l is returned un-normalised in both modes


def test_hand_computed_four_bin_example():
    from deepphysinet_amd.causal import bin_weights_reference
    s, b = [1.0, 3.0, 4.0, 8.0, 0.5], [0, 0, 1, 2, 3]
    W, l, count = bin_weights_reference(s, b, 4, 0.25, relative=False)
    np.testing.assert_array_equal(l, [2.0, 4.0, 8.0, 0.5])
    np.testing.assert_array_equal(count, [2, 1, 1, 1])
    np.testing.assert_allclose(W, [1.0, np.exp(-0.5), np.exp(-1.5), np.exp(-3.5)], rtol=1e-15)
    # relative: l / mean(l) = l / 3.625
    W, l, count = bin_weights_reference(s, b, 4, 0.25, relative=True)
    np.testing.assert_array_equal(l, [2.0, 4.0, 8.0, 0.5])
    np.testing.assert_allclose(W, np.exp(-0.25 * np.array([0.0, 2.0, 6.0, 14.0]) / 3.625), rtol=1e-15)


def test_an_empty_bin_adds_nothing_and_repeats_its_predecessors_weight():
    from deepphysinet_amd.causal import bin_weights_reference
    for relative in (True, False):
        W, l, count = bin_weights_reference([2.0, 6.0], [0, 3], 5, 0.5, relative)
        np.testing.assert_array_equal(count, [1, 0, 0, 1, 0])
        assert l[1] == l[2] == l[4] == 0.0
        assert W[1] == W[2] == W[3] < W[0] == 1.0 and W[4] < W[3]
        norm = 4.0 if relative else 1.0                                   # the mean over the two non-empty bins
        np.testing.assert_allclose(W[4], np.exp(-0.5 * 8.0 / norm), rtol=1e-15)


def test_relative_mode_with_all_zero_losses_gives_all_ones():
    from deepphysinet_amd.causal import bin_weights_reference
    W, l, count = bin_weights_reference(np.zeros(10), np.arange(10) % 3, 3, 5.0, relative=True)
    assert (W == 1.0).all() and (l == 0.0).all()
    W, _, _ = bin_weights_reference([np.inf, 1.0], [0, 1], 2, 5.0, relative=True)      # a mean that is not finite
    assert (W == 1.0).all()


def test_bin_index_at_the_bounds_below_an_inner_edge_and_outside_the_range():
    from deepphysinet_amd.causal import bin_index
    edge = np.float32(21600.0)                                            # 86400 / 4
    below = np.nextafter(edge, np.float32(0.0))
    t = np.array([0.0, 86400.0, below, edge, -1.0, 1e9, 43200.0, np.nan], dtype=np.float32)
    np.testing.assert_array_equal(bin_index(t, 0.0, 86400.0, 4), [0, 3, 0, 1, 0, 3, 2, 0])
    assert bin_index(t, 0.0, 86400.0, 4).dtype == np.int32
    np.testing.assert_array_equal(bin_index(t[:7], 0.0, 86400.0, 1), [0] * 7)
    np.testing.assert_array_equal(bin_index([5.0, 6.0, 7.0], 5.0, 7.0, 64), [0, 32, 63])
    with pytest.raises(ValueError):
        bin_index(t, 1.0, 1.0, 4)
    with pytest.raises(ValueError):
        bin_index(t, 0.0, 1.0, 65)


def test_point_and_weighted_loss_references():
    from deepphysinet_amd.causal import CRIT_L1, CRIT_MSE, CRIT_SMOOTH_L1, point_loss_reference, weighted_losses_reference
    res = np.array([[1.0, -2.0, 0.05, 0.0, 3.0, -0.5], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]], dtype=np.float32)
    fac = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    np.testing.assert_allclose(point_loss_reference(res, fac), [1 + 8 + 3 * 0.0025 + 0 + 45 + 1.5, 0.25 * 21], rtol=1e-7)
    np.testing.assert_allclose(point_loss_reference(res, fac, CRIT_L1), [1 + 4 + 0.15 + 0 + 15 + 3, 0.5 * 21], rtol=1e-7)
    sl1 = point_loss_reference(res, fac, CRIT_SMOOTH_L1, 0.1)
    np.testing.assert_allclose(sl1[0], 0.95 + 2 * 1.95 + 3 * 0.0125 + 0 + 5 * 2.95 + 6 * 0.45, rtol=1e-6)
    ones = weighted_losses_reference(res, [1.0, 1.0], fac)
    np.testing.assert_allclose(ones, np.array(fac) * (res.astype(np.float64) ** 2).mean(0), rtol=1e-15)
    np.testing.assert_allclose(weighted_losses_reference(res, [0.5, 0.5], fac), 0.5 * ones, rtol=1e-15)
    np.testing.assert_allclose(weighted_losses_reference(res, [1.0, 0.0], fac, CRIT_MSE, 0.0, True), np.array(fac) * res[0].astype(np.float64) ** 2, rtol=1e-15)
    with pytest.raises(ValueError):
        weighted_losses_reference(res, [1.0], fac)


def test_causal_weights_checks_its_arguments():
    from deepphysinet_amd.causal import CausalWeights
    c = CausalWeights(eps=2)
    assert (c.eps, c.bins, c.relative, c.t_range) == (2.0, 16, True, None) and isinstance(c.eps, float)
    assert c.bounds(86400.0) == (0.0, 86400.0) and CausalWeights(1.0, t_range=(3, 9)).bounds(86400.0) == (3.0, 9.0)
    assert CausalWeights(0).eps == 0.0 and CausalWeights(1.0, bins=64).bins == 64
    for bad in (dict(eps=-1.0), dict(eps=float('nan')), dict(eps=float('inf')), dict(eps=1.0, bins=0), dict(eps=1.0, bins=65), dict(eps=1.0, bins=2.5),
                dict(eps=1.0, t_range=(1.0, 1.0)), dict(eps=1.0, t_range=(0.0, float('inf'))), dict(eps=1.0, t_range=(0.0,))):
        with pytest.raises(ValueError):
            CausalWeights(**bad)
    with pytest.raises(Exception):
        c.eps = 3.0                                                       # a value type: frozen


# ------------------------------------------------------------------------------------------------ build
def _hipcc():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    return hipcc


def test_causal_unit_cross_compiles_without_spills_or_scratch(tmp_path):
    from deepphysinet_amd.build import COMMON, UNITS
    unit = [u for u in UNITS if os.path.basename(u[0]) == 'dpn_causal.hip']
    assert len(unit) == 1 and unit[0][2] == 'dpn_causal.o' and UNITS[-1] is unit[0]            # appended: the other units keep their index
    residual = [u for u in UNITS if os.path.basename(u[0]) == 'dpn_residual.hip']             # holds the kernel that applies the weights
    assert len(residual) == 1
    texts = []
    for src, flags, obj in (unit[0], residual[0]):
        asm = str(tmp_path / (obj + '.s'))
        subprocess.run([_hipcc(), *[f for f in COMMON if f != '-fPIC'], *flags, '--cuda-device-only', '-S', '-I' + os.path.join(ROOT, 'include'), src,
                        '-o', asm], check=True, capture_output=True)
        texts.append(open(asm).read())
    found = [(re.findall(r'\.name:\s+(\S*dpn_causal_(?:bins|weights)_kernel\S*)', texts[0]), texts[0]),
             (re.findall(r'\.name:\s+(\S*dpn_residual_kernel\S*ResWArgs\S*)', texts[1]), texts[1])]
    assert [len(names) for names, _ in found] == [2, 1], found[0][0] + found[1][0]
    for name, text in ((name, text) for names, text in found for name in names):
        at = text.index('.name:           ' + name)                      # the kernel's metadata entry: from its `- .agpr_count` to the next one
        end = text.find('- .agpr_count', at)
        block = text[text.rindex('- .agpr_count', 0, at):end if end > 0 else len(text)]
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', block).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', block).group(1)) == 0, name           # no scratch
        assert int(re.search(r'\.wavefront_size:\s+(\d+)', block).group(1)) == 64, name
    for text in texts:
        assert 's_swappc_b64' not in text and 'scratch_' not in text
        assert not re.search(r'\b(global|flat|buffer|ds)_atomic|\bds_(add|max|min)_', text), 'the units must not use atomics'


def test_causal_entry_points_are_exported_and_match_the_binding():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.build import build_library
    _hipcc()
    lib = build_library()
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], check=True, capture_output=True, text=True).stdout
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name, n_args in (('dpn_causal_bins', 14), ('dpn_causal_weights', 8), ('dpn_residual_weighted', 15), ('dpn_causal_rows_doubles', 2)):
        assert re.search(r' T %s$' % name, syms, re.M), name
        assert name in L.EXPORTS and len(L.EXPORTS[name][1]) == n_args
        decl = re.search(r'^int(?:64_t)? %s\((.*?)\);' % name, header, re.M | re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', decl).split(',')) == n_args, name
    assert L.CAUSAL_MAX_BINS == 64 and '#define DPN_CAUSAL_MAX_BINS 64' in header
    # dpn_residual_weighted = dpn_residual's signature + (w, bin, bin_w) in front of the stream
    assert L.EXPORTS['dpn_residual_weighted'][1][:11] == L.EXPORTS['dpn_residual'][1][:11]
