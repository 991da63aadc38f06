"""No GPU: the teeth of tests/test_gpu_wgrad_fp64.py.  Every case of tests/wgrad_cases.py with n <= 1037 goes through emulate() -- the kernels'
arithmetic in fp32 torch, kernel_model.mm in the case's precision -- in place of the GPU:
  * the faithful emulation is inside every bound of every stage;
  * each seeded mistake (wgrad_cases.ALTERS) breaks a bound on at least one gradient tensor in every dense case;
  * the K-layout decoder's index map is the one of csrc/dpn_layout.h (a small g++ program prints the header's);
  * reference() with the fp64 model's own masks is kernel_model.phase_b inside pde_step(prec='fp64'), which tests/test_kernel_model.py
    proves equal to the autograd oracle;
  * the fp32 kernel model's ReLU masks differ from the fp64 ones at no more than the cap the GPU test holds the kernels' masks to."""
import os
import subprocess

import pytest
import torch

import wgrad_cases as WC
from oracle import dpn_oracle as O
from oracle import kernel_model as KM
from oracle.fill import synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = [c for c in WC.all_cases() if c.n <= 1037]
DENSE = [c for c in CPU_CASES if c.kind == 'dense']
_passes = {}


def alters_of(c):
    return tuple(a for a in WC.ALTERS if c.prec == 'bf16x2' or a not in WC.HILO_ALTERS)


def emulated(c):
    """{alter: pass} of case c, the faithful pass under None; dense cases carry their seeded mistakes (evaluated once, shared by the tests)."""
    if c not in _passes:
        inp = synthetic_inputs(c.n, tag='inter')
        g_out, g_jxi = WC.cotangents(c)
        pe_in = WC.pe_in_of(c.n) if c.route == 'pe_in' else None
        alters = (None,) + (alters_of(c) if c.kind == 'dense' else ())
        _passes[c] = (WC.emulate(c, WC.oracle_weights(c.gain), inp['x'], inp['y'], inp['t'], inp['coord_data'], g_out, g_jxi, pe_in=pe_in, alters=alters),
                      g_out, g_jxi)
    return _passes[c]


@pytest.mark.parametrize('c', CPU_CASES, ids=WC.case_id)
def test_the_faithful_emulation_is_inside_every_bound(c):
    em, g_out, g_jxi = emulated(c)
    r = WC.check(c, WC.oracle_weights(c.gain), em[None]['features'], em[None], g_out, g_jxi)
    assert len(r) == 1 + 1 + len(WC.SUMS) + 2 * len(WC.NAMES)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    if c.kind.startswith('onehot'):                        # a net without cotangents: exact zeros (what the GPU test asserts of the kernels)
        for k in range(6):
            if k != WC.HOT_NET:
                assert all(not bool(v.any()) for v in em[None]['grads'][k].values())
    if c.kind == 'gjxi':
        assert not bool(em[None]['gnet'].any())


def test_the_companion_is_the_same_expression_on_absolute_values():
    """|sum| <= companion sum and |gradient| <= finish() of the companions on |W|: what every bound is a multiple of."""
    c = WC.Case('raw', 70, 'bf16x2', 1.0, 'dense', 0.75)
    em, g_out, g_jxi = emulated(c)
    Ws, obs, F = WC.oracle_weights(c.gain), em[None], em[None]['features']
    g_all, gj_all = WC.scaled(c, g_out, g_jxi)
    for k in range(6):
        m1, m2 = obs['m1'][k].double(), obs['m2'][k].double()
        val, _, comp = WC.wgrad_reference(c, F, m2, obs['T1'][k], obs['Z1'][k], g_all[k], gj_all[k])
        for nm in WC.SUMS:
            assert bool((val[nm].abs() <= comp[nm] * (1 + 1e-12)).all()) and float(comp[nm].max()) > 0, nm
        ref = WC.reference(Ws[k], (m1, m2), F.pe, F.dpe, F.pe6, g_out[:, k], g_jxi[:, k], c.scale, t1=obs['T1'][k], z1=obs['Z1'][k])
        ca = WC.companion(Ws[k], comp)
        for nm in WC.NAMES:
            assert bool((ref[nm].reshape(ca[nm].shape).abs() <= ca[nm] * (1 + 1e-12)).all()), nm


@pytest.mark.parametrize('c', DENSE, ids=WC.case_id)
def test_every_seeded_mistake_breaks_a_bound_on_a_gradient_tensor(c):
    em, g_out, g_jxi = emulated(c)
    Ws = WC.oracle_weights(c.gain)
    for alter in alters_of(c):
        if alter in WC.NULL_ALTERS:
            # M2 is a 0 / 1 matrix: its lo plane is identically zero, the kernel issues no M2_lo . Z1_hi product and leaving it out changes no bit.
            # The mistake is seeded all the same and shown to be void; the product that HAS a lo.hi term (dw1 = T1^T Z0) carries 'dw1_no_lo_hi'.
            for k in range(6):
                for nm in WC.NAMES:
                    assert torch.equal(em[alter]['grads'][k][nm], em[None]['grads'][k][nm]), (alter, k, nm)
            continue
        r = WC.check(c, Ws, em[alter]['features'], em[alter], g_out, g_jxi, stages=('chain', 'finish'))
        broken = sorted(k for k, v in r.items() if not v <= 1.0)
        assert broken, (alter, 'passes every bound: the bounds are too loose', max(r.values()))
        # the mistakes in front of the finish stage must show in the gradients against the oracle's phase_b ('chain'), not only in the sums
        assert any(k[0] == 'chain' for k in broken), (alter, broken)


LAYOUT_TABLE = r'''
#include <cstdio>
#include "dpn_layout.h"
using namespace dpn;
int main() {
    // every bf16 element of one 32-point tile of a KMat with ct column tiles: [kk 2][ct][lane 64][e 8] -> point, slot, and what the slot means
    for (int ctn = 6; ctn <= 8; ctn += 2)
        for (int kk = 0; kk < 2; ++kk)
            for (int ct = 0; ct < ctn; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int jj = lane & 31, h = lane >> 5;
                        const int ks = 2 * ct + (jj >> 4), sh = (jj >> 3) & 1, se = jj & 7;
                        std::printf("%d %d %d %d %d %d\n", ctn, ((kk * ctn + ct) * 64 + lane) * 8 + e, drow32(8 * kk + e, h), chain_ch(ks, sh, se),
                                    ctn == 6 ? pe3_ch(ks, sh, se) : -1, ctn == 6 ? pe6_ch(ks, sh, se) : -1);
                    }
    return 0;
}
'''


def test_the_decoder_reads_the_k_layout_of_dpn_layout_h(tmp_path):
    src = tmp_path / 'kmat_table.cpp'
    src.write_text(LAYOUT_TABLE)
    exe = tmp_path / 'kmat_table'
    subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'deepphysinet_amd', 'csrc'), str(src), '-o', str(exe)], check=True)
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split('\n') if line]
    assert len(rows) == (6 + 8) * 2 * 64 * 8
    for ctn in (6, 8):
        tab = [r for r in rows if r[0] == ctn]
        # a two-tile buffer: plane 0 holds the element's point (0 .. 63, the second tile's from 32), plane 1 its channel (256 columns) or coordinate
        # feature (192), plane 2 its data feature -- small integers, exact in bf16
        per_tile = ctn * 1024                                                   # bf16 elements of one tile of one plane
        planes = 2 if ctn == 8 else 3
        buf = torch.zeros(planes, 2, per_tile)
        for _, idx, point, ch, p3, p6 in tab:
            for tile in range(2):
                buf[0, tile, idx] = 32 * tile + point
                buf[1, tile, idx] = ch if ctn == 8 else p3
                if ctn == 6:
                    buf[2, tile, idx] = p6
        raw = (buf.view(torch.int32) >> 16).to(torch.int16).reshape(-1).view(torch.uint8)
        dec = WC.kmat_decode(raw, 0, 1, planes, 64, ctn)[0]                     # [plane, 64 points, 32 ctn slots]
        assert torch.equal(dec[0], torch.arange(64, dtype=torch.float64)[:, None].expand(64, 32 * ctn))
        assert torch.equal(dec[1], (WC.CH_OF_SLOT if ctn == 8 else WC.PE3_OF_SLOT).double()[None, :].expand(64, 32 * ctn))
        if ctn == 6:                                                            # the data features' slots (the PE6 table, S2's columns)
            assert torch.equal(dec[2], WC.PE6_OF_SLOT.double()[None, :].expand(64, 32 * ctn))
        # and the encoder used below is the decoder's inverse
        x = torch.randint(-8, 8, (64, 32 * ctn)).double()
        assert torch.equal(WC.kmat_decode(WC.kmat_encode(x, ctn), 0, 1, 1, 64, ctn)[0, 0], x)
    for perm, inv in ((WC.CH_OF_SLOT, WC.SLOT_OF_CH), (WC.PE3_OF_SLOT, WC.SLOT_OF_PE3), (WC.PE6_OF_SLOT, WC.SLOT_OF_PE6)):
        assert torch.equal(perm[inv], torch.arange(perm.numel()))


def test_the_decoders_constants_are_the_kernels():
    csrc = os.path.join(ROOT, 'deepphysinet_amd', 'csrc')
    with open(os.path.join(csrc, 'dpn_wgrad.hip')) as f:
        wg = f.read()
    with open(os.path.join(csrc, 'dpn_point_common.h')) as f:
        pc = f.read()
    for needle in ('constexpr int kPartFloats = 65536 + 49152 * 2 + 7 * 256;', 'return prod == 1 ? 0 : prod == 2 ? 65536 : 114688;',
                   'constexpr int kPartVec = 163840;', 'constexpr int kMaxSplits = 20;',
                   'part[kPartVec + 2 * 256 + rr] = v;', 'part[kPartVec + 3 * 256 + rr] = v;', 'part[kPartVec + 4 * 256] = gs;',
                   'const int qo = kPartVec + (PROD == 1 ? 5 : 6) * 256;', 'out->partials = ((int64_t)out->k_splits * kNets * kPartFloats + kFinishScratchFloats) * 4;',
                   # the finish writes d bd, d evec and column 256 of d w2b2 from ONE value: the GPU test holds them bitwise equal
                   'else { Gd.w2b2[o * Gd.ld_w2b2 + 256] = v; Gd.evec[o] = v; Gd.bd[o] = v; }'):
        assert needle in wg, needle
    for needle in ('o.gnet = reinterpret_cast<float*>(b + m256 + m192 + t192);', 'o.gj = reinterpret_cast<float*>(b + m256 + t192);',
                   'static inline int64_t pad_points(int64_t n) { return ((n + 127) / 128) * 128; }'):
        assert needle in pc, needle
    assert WC.PART_FLOATS == 165632 and WC.MAX_SPLITS == 20


def test_the_reference_is_the_oracles_phase_b():
    """pde_step(prec='fp64') with the fp64 model's own masks and residual cotangents, net by net, to 1e-12 of each tensor's maximum; finish() -- the
    finish stage's reference -- is the same algebra behind the sums."""
    dt = torch.float64
    geo = O.Geometry()
    st = O.make_state(dtype=dt)
    inp = {k: v.to(dt) for k, v in synthetic_inputs(96, tag='inter').items()}
    res = KM.pde_step(st, inp['x'], inp['y'], inp['t'], inp['f'], inp['field_data'], inp['coord_data'], inp['forecast_h'], geo, prec='fp64')
    scale = torch.tensor([1.0 / geo.dx / (geo.lon - 1), 1.0 / geo.dy / (geo.lat - 1), 1.0 / geo.pred_t_span], dtype=dt)
    xi = torch.cat([inp['x'] / geo.dx / (geo.lon - 1), inp['y'] / geo.dy / (geo.lat - 1), inp['t'] / geo.pred_t_span], 1)
    pe, dpe = KM.pe_and_tangent(xi)
    pe6 = O.sine_cos_pe(inp['coord_data'], 16)
    Ws, Ss, jx = [], [], []
    for k, net in enumerate(O.NETS):
        W = KM.net_weights(st, net, res['meta_out'], inp['forecast_h'])
        W = dict(W, wo=W['wo'].reshape(-1))
        _, jxi, S = KM.phase_a(W, pe, dpe, pe6, inp['coord_data'][:, k], 'fp64', fused=True)
        Ws.append(W), Ss.append(S), jx.append(jxi)
    _, gout, gjn, _, _ = KM.residuals(res['out_n'], torch.stack(jx, 1) * scale, inp['f'])
    for k in range(6):
        g, gj = gout[:, k], gjn[:, k] * scale
        mine = WC.reference(Ws[k], (Ss[k]['m1'], Ss[k]['m2']), pe, dpe, pe6, g, gj, 1.0)
        Z1 = Ss[k]['m1'] * ((g[:, None] * pe + (dpe * gj[:, None, None, :]).reshape(96, -1)) @ Ws[k]['w1b1'][:, :192].T + g[:, None] * Ws[k]['w1b1'][:, 192])
        g6 = g[:, None] * pe6
        m2 = Ss[k]['m2']
        sums = {'S1': m2.T @ Z1, 'S2': m2.T @ g6, 'dw1': Ss[k]['t1'].T @ (g[:, None] * pe + (dpe * gj[:, None, None, :]).reshape(96, -1)),
                'mv': m2.T @ g, 'db1': Ss[k]['t1'].T @ g, 'sg': g.sum(), 'q1': Z1.sum(0), 'q6': g6.sum(0)}
        fin = WC.finish(Ws[k], Ss[k]['u'], sums)
        for nm in WC.NAMES:
            ref = res['grads'][k][nm].reshape(mine[nm].shape)
            top = float(ref.abs().max())
            assert top > 0, nm
            assert float((mine[nm] - ref).abs().max()) <= 1e-12 * top, (k, nm)
            assert float((fin[nm].reshape(ref.shape) - ref).abs().max()) <= 1e-12 * top, (k, nm, 'finish')
    # ... and the oracle weights handed to the emulation are the fp32 tensors of the same state
    W32 = WC.oracle_weights(1.0)
    assert float((W32[0]['W1'] - Ws[0]['W1']).abs().max()) <= 2.0 ** -24 * float(Ws[0]['W1'].abs().max())


@pytest.mark.parametrize('n,gain', [(n, 1.0) for n in WC.SIZES] + [(70, 5.0), (1037, 5.0)])
def test_the_fp32_models_masks_stay_inside_the_cap(n, gain):
    """The GPU test holds the kernels' decoded masks to the fp64 masks with at most max(3, n // 100) differing points.  The cap is test_gpu_parity's;
    here: the fp32 kernel model on the same weights and inputs is inside it at both gains (so gain 5 needs no smaller substitute)."""
    inp = synthetic_inputs(n, tag='inter')
    c = WC.Case('raw', n, 'bf16x2', gain, 'dense', 0.75)
    F = WC.Features(inp['x'], inp['y'], inp['t'], inp['coord_data'])
    Ws = WC.oracle_weights(gain)
    true = WC.masks_reference(Ws, F, WC.fused_route(c))
    model = WC.masks_reference(Ws, F, WC.fused_route(c), dtype=torch.float32)
    flipped = int(WC.flipped_points(true, model).sum())
    print('n = %d, gain %g: %d points carry a mask bit that differs between the fp32 model and fp64' % (n, gain, flipped))
    assert flipped <= max(3, n // 100)


def test_the_device_sincos_model_is_as_accurate_as_its_header_says():
    """The measured term of the bounds: csrc/dpn_sincos.h quotes |err| ~ 1e-7 for |theta| up to a few hundred; the cases' angles stay below 16 x 6."""
    inp = synthetic_inputs(1037, tag='inter')
    F = WC.Features(inp['x'], inp['y'], inp['t'], inp['coord_data'])
    assert float(F.ang.abs().max()) <= 16.0 and float(F.ang6.abs().max()) < 100.0
    assert 0 < F.sc <= WC.MARGIN * 2.5e-7
