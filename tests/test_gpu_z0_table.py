"""GPU (MI355X): in the hi+lo mode on raw coordinates stage 1 no longer stores Z0 = g pe3 + gJ_c d pe3 / d xi_c per point and net.  It writes a per-point
fp32 table of the coordinate features, the coordinate cotangents gJ_c and a header (form word, frequencies) into the space Z0 occupied, and product 3
of dpn_wgrad_kernel<2> forms Z0 from them in LDS (csrc/dpn_point_common.h, OperandView; csrc/dpn_wgrad.hip, form_z0()).  Plain bf16, caller-encoded
coordinates and the second-derivative kernels keep the stored Z0 and product 3's stored-form body.

The weight side is driven through the C ABI as tools/wgrad_digest.py drives it (same inputs, same cotangents, scale 0.75); the helper below adds what
that tool's cases do not have: the second-derivative entry point with an all-zero g_hxi, a reused operand buffer, and a fill byte for it."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('wgrad_digest', os.path.join(ROOT, 'tools', 'wgrad_digest.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

SIZES = (1, 70, 1037, 5197)        # 127 padding points | ragged 64- and 32-point tiles, the small range plan | the full 42-range plan
_cache = {}


def _case(route, n, prec, operands=None, fill=0):
    """pack -> dpn_fwd_ref -> stage 1 -> dpn_wgrad -> dpn_wgrad_finish.  route 'raw': dpn_bwd_points_scaled (g_out, g_jxi) | 'deriv':
    dpn_bwd_points_derivs with the same cotangents and an all-zero g_hxi | 'pe_in': dpn_bwd_points on caller-encoded coordinates (g_out only).
    operands: a buffer to reuse as it is; otherwise a fresh one filled with the byte `fill`."""
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as P
    from oracle.fill import synthetic_inputs
    m = D._model(prec)
    dev = torch.device('cuda:0')
    g = {k: v.to(dev) for k, v in synthetic_inputs(n, tag='inter').items()}
    cfg = m.point_config()
    lib = L.load()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(g['field_data'], g['forecast_h'])
        heads, evec = heads.detach().contiguous(), evec.detach().contiguous()
        statics = [s.detach().contiguous() for s in statics]
    nets = P._net_ptrs(heads, evec, statics)
    x, y, t = (g[k].reshape(-1).contiguous() for k in ('x', 'y', 't'))
    cd = g['coord_data'].contiguous()
    geo, fr = cfg.geometry(), P._freqs(dev)
    ws = P._Workspace(n, cfg.prec, dev)
    pe_in = torch.sin(D._randn((n, 192), 4, dev) * 3.0).contiguous() if route == 'pe_in' else None
    g_out = D._randn((n, 6), 1, dev)
    g_jxi = D._randn((n, 6, 3), 2, dev) if route != 'pe_in' else None
    scale = torch.full((1,), D.G_SCALE, device=dev)
    s = P._stream()
    L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0 if pe_in is None else 1), P._ptr(ws.packed), s), 'pack')
    out = torch.empty(n, 6, device=dev)
    saved = torch.zeros(ws.sizes.saved, dtype=torch.uint8, device=dev)
    if operands is None:
        operands = torch.full((ws.sizes.operands,), fill, dtype=torch.uint8, device=dev)
    assert operands.numel() == ws.sizes.operands
    partials = torch.empty(ws.sizes.partials, dtype=torch.uint8, device=dev)
    xyt = (P._ptr(x), P._ptr(y), P._ptr(t)) if pe_in is None else (None, None, None)
    jac = torch.empty(n, 6, 3, device=dev) if pe_in is None else None
    L.check(lib.dpn_fwd_ref(*xyt, P._ptr(pe_in), P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac),
                            P._ptr(saved), s), 'fwd')
    bargs = (*xyt, P._ptr(pe_in), P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(g_out), P._ptr(g_jxi))
    if route == 'raw':
        L.check(lib.dpn_bwd_points_scaled(*bargs, P._ptr(scale), P._ptr(saved), P._ptr(operands), s), 'bwd')
    elif route == 'deriv':
        g_hxi = torch.zeros(n, 6, 3, device=dev)
        L.check(lib.dpn_bwd_points_derivs(*bargs, P._ptr(g_hxi), P._ptr(scale), P._ptr(saved), P._ptr(operands), s), 'bwd derivs')
    else:
        L.check(lib.dpn_bwd_points(*bargs, P._ptr(saved), P._ptr(operands), s), 'bwd')
    g_heads = torch.empty(256, P.HEADS_COLS, device=dev)
    g_evec = torch.empty(6, 256, device=dev)
    g_stat = [torch.empty(P.STATIC_SHAPES[i % 8], device=dev) for i in range(48)]
    L.check(lib.dpn_wgrad(n, cfg.prec, P._ptr(g_out), P._ptr(saved), P._ptr(operands), P._ptr(partials), s), 'wgrad')
    L.check(lib.dpn_wgrad_finish(nets, P._ptr(ws.packed), n, cfg.prec, P._ptr(partials), P._net_ptrs(g_heads, g_evec, g_stat, cls=L.DpnNetGradPtrs), s),
            'finish')
    torch.cuda.synchronize()
    res = {'operands': operands, 'g_heads': g_heads, 'g_evec': g_evec}
    for i, st in enumerate(g_stat):
        res['static_%02d' % i] = st
    return res, int(ws.sizes.n_pad)


def _zero_run(n):
    """the plain route on a zero-initialised operand buffer, hi+lo: shared by the tests below"""
    if n not in _cache:
        _cache[n] = _case('raw', n, 'bf16x2')
    return _cache[n]


def _grads(res):
    return {k: v for k, v in res.items() if k != 'operands'}


def _form_word(operands, n_pad, ns):
    off = 6 * ns * n_pad * 512 + 7 * ns * n_pad * 384 + 6 * n_pad * 4 + 256
    return int(operands[off:off + 4].view(torch.int32)[0])


@pytest.mark.parametrize('n', SIZES)
def test_both_product_3_bodies_agree(n):
    """The second-derivative stage-1 kernel with g_hxi = 0 forms gs = fmaf(-0 fr, fr, g) = g and STORES the same Z0 the plain route's table form has
    dpn_wgrad_kernel form: the stored-form body against the table body in one build, all 50 gradients bit for bit."""
    tab, n_pad = _zero_run(n)
    sto, _ = _case('deriv', n, 'bf16x2')
    assert _form_word(tab['operands'], n_pad, 2) == 1 and _form_word(sto['operands'], n_pad, 2) == 0
    a, b = _grads(tab), _grads(sto)
    assert len(a) == 50
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff
    assert int(a['g_heads'].count_nonzero()) > 0
    # the table form leaves the stored form's rows unwritten: table = net 0's planes, gJ = 72 B per point behind it, nothing else
    z0 = 6 * 2 * n_pad * 512
    assert int(tab['operands'][z0 + 768 * n_pad + 72 * n_pad:z0 + 6 * 768 * n_pad].count_nonzero()) == 0
    assert int(sto['operands'][z0 + 768 * n_pad + 72 * n_pad:z0 + 6 * 768 * n_pad].count_nonzero()) > 0


def test_the_form_word_follows_the_route():
    """One operand buffer, n = 70: caller-encoded coordinates (stored Z0), raw coordinates (table), and again: every stage-1 launch says which form it
    wrote, and dpn_wgrad computes the parent commit's gradients each time."""
    with open(D.FIXTURE) as f:
        fx = json.load(f)['cases']
    operands = None
    for route in ('pe_in', 'raw', 'pe_in', 'raw'):
        res, n_pad = _case(route, 70, 'bf16x2', operands=operands)
        operands = res['operands']
        assert _form_word(operands, n_pad, 2) == (1 if route == 'raw' else 0), route
        got, ref = D.digest(res, with_sample=False), fx[D.case_key(route, 70, 'bf16x2')]
        diff = [k for k in got if got[k] != ref[k]]
        assert len(got) == 50 and not diff, (route, diff)


@pytest.mark.parametrize('n', [1, 70])
def test_nan_poisoned_operand_buffer(n):
    """The step's operand buffer is torch.empty: a table row, a gJ entry or a header word that stage 1 left unwritten would reach the gradients (NaN x 0
    is NaN).  Every byte 0xFF (NaNs in every format in there) before stage 1: finite gradients, the zero-initialised run's bits."""
    ref, _ = _zero_run(n)
    res, _ = _case('raw', n, 'bf16x2', fill=0xFF)
    a, b = _grads(res), _grads(ref)
    bad = [k for k in a if not bool(torch.isfinite(a[k]).all())]
    assert not bad, bad
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff


def test_plain_bf16_keeps_the_stored_z0():
    res, n_pad = _case('raw', 70, 'bf16')
    z0 = res['operands'][6 * n_pad * 512:6 * n_pad * 512 + 6 * n_pad * 384]
    assert _form_word(res['operands'], n_pad, 1) == 0
    assert int(z0.count_nonzero()) > 0
    per_net = z0.view(6, -1)
    assert all(int(per_net[k].count_nonzero()) > 0 for k in range(6))        # every net's rows, not only what a table would occupy
