#!/usr/bin/env python
"""Digests of what the point backward's weight side computes (dpn_bwd_points* -> dpn_wgrad -> dpn_wgrad_finish), for the library in DPN_LIB (default:
the product build).  tests/test_gpu_wgrad_tables.py holds the product build to tests/golden/wgrad_tables_parent.json, which this tool writes:

    DPN_LIB=<library of the commit to pin against> python tools/wgrad_digest.py            # on the GPU; rewrites the fixture
    python tools/wgrad_digest.py --print                                                   # digests of the product build, nothing written

Per case (route, n, precision): the SHA-256 of the bytes of g_heads, g_evec and each of the 48 static gradients.  With --sample the n = 5197 cases also
get every 97th element of g_heads (float32 bit patterns, little-endian, one hex string) and its largest magnitude: what a build with another range
plan -- another summation order -- would be compared on.  The committed fixture has no sample (114 KB of hex that no assertion reads while the
plan is the fixture commit's).  Inputs are the oracle's closed-form fills and CPU-generator random cotangents, so they do not depend on the device's
random numbers."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'wgrad_tables_parent.json')
SIZES = (1, 70, 1037, 5197)
PRECS = ('bf16x2', 'bf16')
STRIDE = 97
G_SCALE = 0.75
_models = {}


def case_key(route, n, prec):
    return '%s/%d/%s' % (route, n, prec)


def all_cases():
    return [('raw', n, p) for n in SIZES for p in PRECS] + [('pe_in', 70, p) for p in PRECS]


def _model(prec, gain=1.0):
    import torch
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from oracle.fill import fill_state_dict_
    if (prec, gain) not in _models:
        m = builder_models(**ncep_config(), precision=prec)
        sd = m.physics_net.state_dict()
        fill_state_dict_(sd, gain=gain)
        m.physics_net.load_state_dict(sd)
        _models[(prec, gain)] = m.to(torch.device('cuda:0'))
    return _models[(prec, gain)]


def _randn(shape, seed, dev):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def run_case(route, n, prec, zero_cotangents=False, bwd_kernel=None, cotangents=None, scale=G_SCALE, gain=1.0, keep=False):
    """One pass pack -> dpn_fwd_ref -> dpn_bwd_points_scaled (route 'raw': raw coordinates, g_out and g_jxi, scale 0.75) or dpn_bwd_points (route
    'pe_in': caller-encoded coordinates, g_out only) -> dpn_wgrad -> dpn_wgrad_finish.  Returns {'operands', 'g_heads', 'g_evec', 'static_00' ..}.
    cotangents = (g_out [n, 6], g_jxi [n, 6, 3] or None), host or device tensors, in place of the seeded normal ones (route 'pe_in' takes g_out alone);
    scale: the scalar of dpn_bwd_points_scaled; gain: fill_state_dict_'s.  keep: the result also holds 'saved', 'partials' (zeroed before the launch:
    the ranges no product writes stay zero) and 'inputs' = what the launches were handed (heads, evec, statics, x, y, t, coord_data, pe_in, g_out,
    g_jxi, scale, geometry, k_splits = the point ranges of dpn_sizes) -- tests/test_gpu_wgrad_fp64.py compares the outputs with an fp64 evaluation of the same operation on them."""
    import torch
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as P
    from oracle.fill import synthetic_inputs
    m = _model(prec, gain)
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
    pe_in = None
    if route == 'pe_in':
        pe_in = torch.sin(_randn((n, 192), 4, dev) * 3.0).contiguous()               # any finite features in [-1, 1]
    g_out = _randn((n, 6), 1, dev)
    g_jxi = _randn((n, 6, 3), 2, dev) if route == 'raw' else None
    if cotangents is not None:
        g_out = cotangents[0].to(dev, torch.float32).contiguous()
        g_jxi = cotangents[1].to(dev, torch.float32).contiguous() if (route == 'raw' and cotangents[1] is not None) else None
    if zero_cotangents:
        g_out.zero_()
        if g_jxi is not None:
            g_jxi.zero_()
    scale = torch.full((1,), float(scale), device=dev)
    prev = os.environ.get('DPN_BWD_KERNEL')
    if bwd_kernel:
        os.environ['DPN_BWD_KERNEL'] = bwd_kernel
    try:
        L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0 if pe_in is None else 1), P._ptr(ws.packed), P._stream()), 'pack')
        out = torch.empty(n, 6, device=dev)
        saved = torch.zeros(ws.sizes.saved, dtype=torch.uint8, device=dev)            # (zeroed: the buffers have bytes no kernel writes)
        operands = torch.zeros(ws.sizes.operands, dtype=torch.uint8, device=dev)
        partials = (torch.zeros if keep else torch.empty)(ws.sizes.partials, dtype=torch.uint8, device=dev)
        xyt = (P._ptr(x), P._ptr(y), P._ptr(t)) if pe_in is None else (None, None, None)
        jac = torch.empty(n, 6, 3, device=dev) if pe_in is None else None
        L.check(lib.dpn_fwd_ref(*xyt, P._ptr(pe_in), P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac),
                                P._ptr(saved), P._stream()), 'fwd')
        bargs = (*xyt, P._ptr(pe_in), P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(g_out), P._ptr(g_jxi))
        if route == 'raw':
            L.check(lib.dpn_bwd_points_scaled(*bargs, P._ptr(scale), P._ptr(saved), P._ptr(operands), P._stream()), 'bwd')
        else:
            L.check(lib.dpn_bwd_points(*bargs, P._ptr(saved), P._ptr(operands), P._stream()), 'bwd')
        g_heads = torch.empty(256, P.HEADS_COLS, device=dev)
        g_evec = torch.empty(6, 256, device=dev)
        g_stat = [torch.empty(P.STATIC_SHAPES[i % 8], device=dev) for i in range(48)]
        L.check(lib.dpn_wgrad(n, cfg.prec, P._ptr(g_out), P._ptr(saved), P._ptr(operands), P._ptr(partials), P._stream()), 'wgrad')
        L.check(lib.dpn_wgrad_finish(nets, P._ptr(ws.packed), n, cfg.prec, P._ptr(partials), P._net_ptrs(g_heads, g_evec, g_stat, cls=L.DpnNetGradPtrs),
                                     P._stream()), 'finish')
        torch.cuda.synchronize()
    finally:
        if bwd_kernel:
            if prev is None:
                os.environ.pop('DPN_BWD_KERNEL', None)
            else:
                os.environ['DPN_BWD_KERNEL'] = prev
    res = {'operands': operands, 'g_heads': g_heads, 'g_evec': g_evec}
    for i, s in enumerate(g_stat):
        res['static_%02d' % i] = s
    if keep:
        res.update(saved=saved, partials=partials,
                   inputs=dict(heads=heads, evec=evec, statics=statics, x=x, y=y, t=t, coord_data=cd, pe_in=pe_in, g_out=g_out, g_jxi=g_jxi,
                               scale=scale, geometry=(geo.dx, geo.dy, geo.lon_m1, geo.lat_m1, geo.pred_t_span), k_splits=int(ws.sizes.k_splits)))
    return res


def digest(res, with_sample):
    d = {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in res.items() if k != 'operands'}
    if with_sample:
        d['g_heads_absmax'] = float(res['g_heads'].abs().max()).hex()
        d['g_heads_sample'] = res['g_heads'].detach().cpu().reshape(-1)[::STRIDE].contiguous().numpy().astype('<f4').tobytes().hex()
    return d


def write_fixture(out):
    """One line per case: the file stays a dozen lines long."""
    with open(FIXTURE, 'w') as f:
        f.write('{"library": %s, "stride": %d, "cases": {\n' % (json.dumps(out['library']), out['stride']))
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(out['cases'].items())))
        f.write('\n}}\n')


def main():
    from deepphysinet_amd import _lib as L
    out = {'library': os.path.basename(L.LIB_PATH), 'stride': STRIDE, 'cases': {}}
    for route, n, prec in all_cases():
        out['cases'][case_key(route, n, prec)] = digest(run_case(route, n, prec), with_sample=(n == 5197 and '--sample' in sys.argv))
        print(case_key(route, n, prec), out['cases'][case_key(route, n, prec)]['g_heads'][:16], flush=True)
    if '--print' in sys.argv:
        return
    write_fixture(out)
    print('wrote', FIXTURE)


if __name__ == '__main__':
    main()
