"""No GPU: the teeth of tests/test_gpu_value_fp64.py.  Every case of tests/value_cases.py goes through emulate_value() -- the forward kernels' arithmetic
in fp32 torch on bf16 planes -- and the g_hxi passes through wgrad_cases.emulate(), in place of the GPU:
  * the faithful model is inside every condition of every stage (the largest ratio per stage is printed);
  * each seeded mistake (value_cases.SEEDS, and the two in the g_hxi seed) leaves a bound on its named case;
  * dx <-> dy in the chain rule changes NO bit on the NCEP geometry (dx == dy) and leaves the bounds on the unequal one: the gap this closes;
  * two points whose masks are another net's pass the count the older test holds the masks to, and fail the 'masks' condition;
  * forward_reference / deriv_reference under the fp64 model's own masks are kernel_model.phase_a;
  * the decoder of the stored Z0 rows reads the K-layout of csrc/dpn_layout.h at the offset of OperandView."""
import os
import subprocess

import pytest
import torch

import value_cases as VC
import wgrad_cases as WC
from oracle import kernel_model as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = VC.all_cases()
_passes = {}
_worst = {}

NAMED = VC.VCase('raw', 70, 'bf16x2', 1.0, 'odd', 'interior', 'derivs', None)          # the named case of every seeded mistake
NAMED_NCEP = NAMED._replace(geo='ncep')
NAMED_PLAIN = VC.VCase('raw', 70, 'bf16', 1.0, 'odd', 'interior', 'derivs', None)
# (layer 1 without one of its three products: pre1 is off by ~2^-9 of a random-sign sum -- the element-wise E_pre1 sees that where a mask bit turns with
#  it; two layers further down, the worst-case absolute-value bound on the field does not)
EXPECT = {'l1_no_lo_hi': ('masks', 'm1'),'gpe_no_hi_lo': ('stage', 'jac'), 'no_wd_wo': ('out', 'out'), 'no_wo_cvec': ('out', 'out'),
          'coord_as_ref': ('out', 'out'), 'dx_dy': ('chain', 'jac'), 'hess_one_division': ('stage', 'hess'), 'd3_from_pe': ('stage', 'd3'),
          'd2_swapped': ('stage', 'hess'), 'last_from_padding': ('stage', 'jac'), 'masks_next_net': ('masks', 'm1')}


def emulated(c, seeds=(None,)):
    key = (c, seeds)
    if key not in _passes:
        _passes[key] = VC.emulate_value(c, WC.oracle_weights(c.gain), VC.inputs(c), seeds=seeds)
    return _passes[key]


def checked(c, obs, stages=VC.STAGES):
    return VC.check_value(c, WC.oracle_weights(c.gain), obs['features'], obs, obs['ref6'], stages=stages)


@pytest.mark.parametrize('c', CASES, ids=VC.case_id)
def test_the_faithful_model_is_inside_every_condition(c):
    obs = emulated(c)[None]
    r = checked(c, obs)
    for key in sorted(r):
        print('%-6s %-5s %.3g' % (key[0], key[1], r[key]))
        if key != ('masks', 'bits'):
            _worst[key] = max(_worst.get(key, 0.0), r[key])
    want = {('masks', 'm1'), ('masks', 'm2'), ('masks', 'bits'), ('out', 'out')}
    if c.route == 'raw':
        want |= {(s, nm) for s in ('stage', 'chain') for nm in VC.DERIV_NAMES}
    assert set(r) == want
    bad = {k: v for k, v in VC.conditions(r).items() if not v <= 1.0}
    assert not bad, bad
    assert bool(obs['m1'].any()) and bool(obs['m2'].any()) and not bool(obs['m1'].all()) and not bool(obs['m2'].all())


def test_zz_largest_ratio_per_stage_of_the_faithful_model():
    for key in sorted(_worst):
        print('%-6s %-5s %.3g' % (key[0], key[1], _worst[key]))
    assert all(v <= 1.0 for v in _worst.values())


@pytest.mark.parametrize('c', [NAMED, NAMED._replace(gain=5.0, coords='beyond'), NAMED_PLAIN], ids=VC.case_id)
def test_every_seeded_mistake_leaves_its_bound(c):
    # plain bf16 (NAMED_PLAIN): no lo planes, the seven-GEMM form has neither fused term, and its worst-case bounds through several GEMMs -- 2^-8 of the
    # absolute-value sums per layer -- are wider than a swapped ref_data; what hangs on ONE stage (the derivative tail from the decoded T1, the masks) is
    # as sharp as in the hi+lo mode and is asked for
    hilo = c.prec == 'bf16x2'
    seeds = tuple(s for s in VC.SEEDS if hilo or s not in VC.HILO_SEEDS + VC.FUSED_SEEDS + ('coord_as_ref',))
    em = emulated(c, (None,) + seeds)
    assert not {k: v for k, v in VC.conditions(checked(c, em[None])).items() if not v <= 1.0}
    for seed in seeds:
        r = VC.conditions(checked(c, em[seed]))
        broken = sorted(k for k, v in r.items() if not v <= 1.0)
        print('%-18s %s' % (seed, ', '.join('%s/%s %.3g' % (k[0], k[1], r[k]) for k in broken)))
        expect = ('stage', 'jac') if seed == 'dx_dy' and not hilo else EXPECT[seed]
        assert expect in broken, (seed, 'passes its condition: the bound is too loose', r[expect])
        if hilo and EXPECT[seed][0] == 'stage' and seed != 'gpe_no_hi_lo':      # a mistake behind gpe: the statement that does not lean on T1 sees it as well
            assert ('chain', EXPECT[seed][1]) in broken, (seed, broken)


def test_dx_dy_swapped_is_invisible_on_the_ncep_geometry_and_caught_on_the_unequal_one():
    em = emulated(NAMED_NCEP, (None, 'dx_dy'))
    for nm in ('out',) + VC.DERIV_NAMES:
        assert torch.equal(em[None][nm], em['dx_dy'][nm]), nm                       # no bit changes: no tolerance could have seen it
    assert not {k: v for k, v in VC.conditions(checked(NAMED_NCEP, em['dx_dy'])).items() if not v <= 1.0}
    r = VC.conditions(checked(NAMED, emulated(NAMED, (None, 'dx_dy'))['dx_dy']))
    for stage in ('stage', 'chain'):
        for nm in VC.DERIV_NAMES:
            assert r[(stage, nm)] > 1.0, (stage, nm, r[(stage, nm)])
    assert r[('out', 'out')] <= 1.0 and r[('masks', 'm1')] <= 1.0


@pytest.mark.parametrize('n', [70, 1037])
def test_two_points_with_another_nets_masks_pass_the_count_and_fail_the_condition(n):
    c = NAMED._replace(n=n)
    em = emulated(c, (None, 'masks_next_net'))
    Ws, F = WC.oracle_weights(c.gain), em[None]['features']
    true = WC.masks_reference(Ws, F, VC.fused(c))
    for seed in (None, 'masks_next_net'):
        flipped = int(WC.flipped_points(true, (em[seed]['m1'], em[seed]['m2'])).sum())
        assert flipped <= max(3, n // 100), (seed, flipped)                        # the count test of tests/test_gpu_wgrad_fp64.py does not notice
    r = checked(c, em['masks_next_net'], stages=('masks',))
    assert r[('masks', 'm1')] > 1.0 and r[('masks', 'm2')] > 1.0, r
    r = checked(c, em[None], stages=('masks',))
    assert r[('masks', 'm1')] <= 1.0 and r[('masks', 'm2')] <= 1.0, r


@pytest.mark.parametrize('c', [NAMED, NAMED_PLAIN._replace(coords='beyond'), VC.VCase('raw', 65, 'bf16x2', 5.0, 'ncep', 'edges', 'fwd', None)], ids=VC.case_id)
def test_the_references_are_phase_a(c):
    """Under the fp64 model's own masks: fields and Jacobian of kernel_model.phase_a (which tests/test_kernel_model.py proves equal to the autograd
    oracle) to 1e-12 of each tensor's maximum, in both packed forms; hess and d3 are the same contraction with Features.d2pe / d3pe, which are checked
    against finite differences of pe along xi."""
    inp = VC.inputs(c)
    F = VC.features(c, inp)
    Ws = WC.oracle_weights(c.gain)
    ref6 = (inp['coord_data'] if inp['ref_data'] is None else inp['ref_data']).double()
    dx, dy, lon_m1, lat_m1, span = VC.GEOMETRIES[c.geo]
    gg = torch.tensor([lon_m1 * dx, lat_m1 * dy, span], dtype=torch.float64)
    for k in range(6):
        out, jxi, S = KM.phase_a(Ws[k], F.pe, F.dpe, F.pe6, ref6[:, k], 'fp64', fused=VC.fused(c))
        R = VC.forward_reference(c, Ws[k], F, S['m1'], S['m2'], ref6[:, k])
        assert float((R['out'] - out).abs().max()) <= 1e-12 * float(out.abs().max())
        assert torch.equal(R['pre1'] > 0, S['m1'] > 0) and int(((R['pre2'] > 0) != (S['m2'] > 0)).sum()) == 0
        D = VC.deriv_reference(c, Ws[k], F, S['t1'])
        assert float((D['jac'][0] - jxi / gg).abs().max()) <= 1e-12 * float((jxi / gg).abs().max())
        assert all(float(D[nm][1].min()) > 0 for nm in VC.DERIV_NAMES)
    # d2pe, d3pe: derivatives of pe along the angle's coordinate (central differences of sin / cos in fp64)
    ang = F.ang.double()
    f = F.fr.reshape(32, 2, 3)[None, :, 0, :]
    h = 1e-4
    pe_of = lambda a: torch.stack([torch.sin(a), torch.cos(a)], 2)
    d2 = (pe_of(ang + f * h) - 2 * pe_of(ang) + pe_of(ang - f * h)) / h ** 2
    d3 = (pe_of(ang + 2 * f * h) - 2 * pe_of(ang + f * h) + 2 * pe_of(ang - f * h) - pe_of(ang - 2 * f * h)) / (2 * h ** 3)
    assert float((F.d2pe - d2).abs().max()) <= 1e-4 * float(F.d2pe.abs().max())
    assert float((F.d3pe - d3).abs().max()) <= 1e-3 * float(F.d3pe.abs().max())


# ---------------------------------------------------------------------------------------------- g_hxi: dpn_bwd_points_derivs into the weight side
GH_STAGES = ('z0', 'stage1', 'saved', 'wgrad', 'finish', 'chain')


def gh_pass(n, kind, z0_seed=None, factor=1.0):
    key = ('gh', n, kind, z0_seed, factor)
    if key not in _passes:
        c = VC.gh_case(n)
        inp = VC.inputs(VC.GH_INPUTS._replace(n=n))
        g_out, g_jxi, g_hxi = VC.gh_cotangents(n, kind)
        g_hxi = g_hxi * factor
        em = WC.emulate(c, WC.oracle_weights(c.gain), inp['x'], inp['y'], inp['t'], inp['coord_data'], g_out, g_jxi, g_hxi=g_hxi, z0_seed=z0_seed,
                        geometry=VC.GEOMETRIES[VC.GH_INPUTS.geo])[None]
        _passes[key] = (c, em, g_out, g_jxi, g_hxi)
    return _passes[key]


@pytest.mark.parametrize('n', VC.GH_SIZES)
@pytest.mark.parametrize('kind', VC.GH_KINDS)
def test_the_faithful_model_with_g_hxi_is_inside_every_bound(n, kind):
    c, em, g_out, g_jxi, g_hxi = gh_pass(n, kind)
    r = WC.check(c, WC.oracle_weights(c.gain), em['features'], em, g_out, g_jxi, stages=GH_STAGES, g_hxi=g_hxi)
    for key in sorted(r):
        print('%-8s %-5s %.3g' % (key[0], key[1], r[key]))
    assert len(r) == 1 + 1 + 1 + len(WC.SUMS) + 2 * len(WC.NAMES)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    if kind == 'gh_only':           # reached through gH alone: gnet and every g-weighted sum are exact zeros, dw1 is not
        assert not bool(em['gnet'].any()) and not bool(em['sums']['S2'].any()) and not bool(em['sums']['mv'].any()) and bool(em['sums']['dw1'].any())


def test_g_hxi_times_a_power_of_two_scales_the_model_exactly():
    c, base, _, _, _ = gh_pass(70, 'gh_only')
    for f in (2.0 ** 8, 2.0 ** -8):
        got = gh_pass(70, 'gh_only', factor=f)[1]
        assert torch.equal(got['Z1'], base['Z1'] * f) and torch.equal(got['Z0'], base['Z0'] * f)
        for k in range(6):
            for nm in WC.NAMES:
                assert torch.equal(got['grads'][k][nm], base['grads'][k][nm] * f), (f, k, nm)


@pytest.mark.parametrize('z0_seed,expect', [('gh_fr', ('stage1', 'Z1')), ('z0_lo_no_gh', ('z0', 'Z0'))])
def test_a_mistake_in_the_g_hxi_seed_leaves_its_bound(z0_seed, expect):
    c, em, g_out, g_jxi, g_hxi = gh_pass(70, 'dense', z0_seed=z0_seed)
    r = WC.check(c, WC.oracle_weights(c.gain), em['features'], em, g_out, g_jxi, stages=GH_STAGES, g_hxi=g_hxi)
    broken = sorted(k for k, v in r.items() if not v <= 1.0)
    print(z0_seed, ', '.join('%s/%s %.3g' % (k[0], k[1], r[k]) for k in broken))
    assert expect in broken, (z0_seed, r[expect])
    assert ('z0', 'Z0') in broken and ('wgrad', 'dw1') in broken and ('chain', 'w1b1') in broken, broken       # the stored rows feed d w1 = T1^T Z0
    if z0_seed == 'z0_lo_no_gh':                                   # the multiplied Z0 is right: stage 1 cannot see a wrong STORED plane -- the 'z0' stage has to
        assert r[('stage1', 'Z1')] <= 1.0


Z0_ROWS = r'''
#include <cstdio>
#include "dpn_layout.h"
using namespace dpn;
int main() {
    // one 32-point tile of one plane of the stored Z0 (six column tiles): [kk 2][ct 6][lane 64][e 8] -> point, reference channel of the coordinate PE
    for (int kk = 0; kk < 2; ++kk)
        for (int ct = 0; ct < 6; ++ct)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int jj = lane & 31, h = lane >> 5;
                    std::printf("%d %d %d\n", ((kk * 6 + ct) * 64 + lane) * 8 + e, drow32(8 * kk + e, h), pe3_ch(2 * ct + (jj >> 4), (jj >> 3) & 1, jj & 7));
                }
    return 0;
}
'''


def test_the_stored_z0_decoder_reads_the_layout_of_dpn_layout_h(tmp_path):
    src = tmp_path / 'z0_rows.cpp'
    src.write_text(Z0_ROWS)
    exe = tmp_path / 'z0_rows'
    subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'deepphysinet_amd', 'csrc'), str(src), '-o', str(exe)], check=True)
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split('\n') if line]
    assert len(rows) == 2 * 6 * 64 * 8
    with open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_point_common.h')) as f:
        pc = f.read()
    # OperandView: Z0 behind the six nets' Z1 planes, [net][plane][tile32] pieces of ct_per_tile * 2048 bytes (kmat_ptr)
    for needle in ('const int64_t m256 = (int64_t)kNets * ns * n_pad * 512,', 'o.Z0 = KMat{b + m256, tiles32, 6};',
                   'return m.base + (((int64_t)net * ns + s) * m.tiles32 + tile32) * (m.ct_per_tile * 2048) + ((kk * m.ct_per_tile + ct) * 64 + lane) * 16;'):
        assert needle in pc, needle
    n, n_pad = 130, 256
    for prec, ns in (('bf16x2', 2), ('bf16', 1)):
        tiles = n_pad // 32
        img = torch.zeros(6, ns, tiles, 6 * 1024)                                   # bf16 elements, small integers: exact
        want = torch.zeros(6, ns, n, 192, dtype=torch.float64)
        for net in range(6):
            for s in range(ns):
                for tile in range(tiles):
                    for idx, point, ch in rows:
                        p = 32 * tile + point
                        if p < n:
                            v = float((net + 2 * s + 3 * p + 5 * ch) % 61 - 30)
                            img[net, s, tile, idx] = v
                            want[net, s, p, ch] = v
        z1_bytes = 6 * ns * n_pad * 512
        buf = torch.cat([torch.full((z1_bytes,), 0x7F, dtype=torch.uint8), (img.view(torch.int32) >> 16).to(torch.int16).reshape(-1).view(torch.uint8),
                         torch.full((4096,), 0x7F, dtype=torch.uint8)])
        z0, planes = VC.decode_z0_stored(buf, n, prec)
        assert torch.equal(planes, want) and torch.equal(z0, want.sum(1))
