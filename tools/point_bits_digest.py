#!/usr/bin/env python
"""Digests of everything the point kernels write (dpn_fwd -> dpn_residual -> dpn_bwd_points, and the *_derivs entry points), for the library in DPN_LIB
(default: the product build).  tests/test_gpu_point_valu_bits.py holds the product build to the digests this tool printed for the commit in front of the
instruction-count work on the point kernels (profiles/valu_diet_ab.txt): equal, not close.

    DPN_LIB=<library of the commit to pin against> python tools/point_bits_digest.py      # on the GPU; prints the EXPECTED table of the test

Per case (route, n, precision): the SHA-256 of the bytes of the fields, the Jacobian (route 'deriv': also the second and third derivatives), the WHOLE
saved state and the WHOLE operand buffer, both zeroed before the launches (they have bytes no kernel writes).  Inputs are the oracle's closed-form fills
and CPU-generator random numbers: nothing depends on the device's random numbers."""
import ctypes
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location('wgrad_digest', os.path.join(ROOT, 'tools', 'wgrad_digest.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

SIZES = (1, 70, 129, 1037)         # 127 padding points | a ragged 64-point workgroup | one point in the third workgroup | ragged 32-point tile, 17 workgroups
PRECS = ('bf16x2', 'bf16')
DERIV_N = 70


def case_key(route, n, prec):
    return '%s/%d/%s' % (route, n, prec)


def all_cases():
    return [('plain', n, p) for n in SIZES for p in PRECS] + [('deriv', DERIV_N, p) for p in PRECS]


def run_case(route, n, prec):
    """route 'plain': dpn_fwd -> dpn_residual -> dpn_bwd_points; 'deriv': dpn_fwd_ref_derivs -> dpn_residual -> dpn_bwd_points_derivs with a random
    g_hxi and scale 0.75.  Returns the tensors that are digested."""
    import torch
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
    x, y, t, f = (g[k].reshape(-1).contiguous() for k in ('x', 'y', 't', 'f'))
    cd = g['coord_data'].contiguous()
    geo, ph, fr = cfg.geometry(), cfg.physics(), P._freqs(dev)
    ws = P._Workspace(n, cfg.prec, dev)
    s = P._stream()
    L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0), P._ptr(ws.packed), s), 'pack')
    out = torch.zeros(n, 6, device=dev)
    jac = torch.zeros(n, 6, 3, device=dev)
    saved = torch.zeros(ws.sizes.saved, dtype=torch.uint8, device=dev)
    operands = torch.zeros(ws.sizes.operands, dtype=torch.uint8, device=dev)
    g_out = torch.zeros(n, 6, device=dev)
    g_jxi = torch.zeros(n, 6, 3, device=dev)
    res = {'fields': out, 'jacobian': jac, 'saved': saved, 'operands': operands}
    xyt = (P._ptr(x), P._ptr(y), P._ptr(t))
    if route == 'plain':
        L.check(lib.dpn_fwd(*xyt, None, P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac), P._ptr(saved), s), 'fwd')
    else:
        hess = torch.zeros(n, 6, 3, device=dev)
        d3 = torch.zeros(n, 6, 3, device=dev)
        L.check(lib.dpn_fwd_ref_derivs(*xyt, None, P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac),
                                       P._ptr(hess), P._ptr(d3), P._ptr(saved), s), 'fwd derivs')
        res['hessian'], res['third'] = hess, d3
    L.check(lib.dpn_residual(P._ptr(out), P._ptr(jac), P._ptr(f), n, ctypes.byref(geo), ctypes.byref(ph), None, None, None, P._ptr(g_out), P._ptr(g_jxi), s),
            'residual')
    bargs = (*xyt, None, P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(g_out), P._ptr(g_jxi))
    if route == 'plain':
        L.check(lib.dpn_bwd_points(*bargs, P._ptr(saved), P._ptr(operands), s), 'bwd')
    else:
        g_hxi = D._randn((n, 6, 3), 3, dev)
        scale = torch.full((1,), D.G_SCALE, device=dev)
        L.check(lib.dpn_bwd_points_derivs(*bargs, P._ptr(g_hxi), P._ptr(scale), P._ptr(saved), P._ptr(operands), s), 'bwd derivs')
    torch.cuda.synchronize()
    return res


def digest(res):
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in res.items()}


def main():
    from deepphysinet_amd import _lib as L
    print('# library: %s' % os.path.basename(L.LIB_PATH))
    print('EXPECTED = {')
    for route, n, prec in all_cases():
        res = run_case(route, n, prec)
        d = digest(res)
        print('    %r: {' % case_key(route, n, prec))
        for k in sorted(d):
            print('        %r: %r,' % (k, d[k]))
        print('    },', flush=True)
        finite = all(bool(v.isfinite().all()) for k, v in res.items() if v.dtype.is_floating_point)
        nz = {k: int(v.count_nonzero()) for k, v in res.items()}
        print('    # finite %s, non-zero %s' % (finite, nz), flush=True)
    print('}')


if __name__ == '__main__':
    main()
