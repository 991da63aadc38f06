"""dpn_wgrad alone at the flagship size (37 265 points, eager launches back to back: three means over 100 launches each) for the library in DPN_LIB
(default: the product build) -- the plan sweeps of choose_plan (csrc/dpn_wgrad.hip), one process per build so that two builds can be alternated.

    python tools/variant_build.py NAME --unit=1 -DDPN_EXPERIMENT_SPLITS
    DPN_LIB=tools/_variants/libdpn_hip_NAME.so python tools/wgrad_time.py bf16x2 default 0,15,13,14 0,14,14,14

PLAN: 'default' (what choose_plan returns) or '0,a,b,c' = the ranges of S1, S2, dw1 through DPN_WGRAD_PLAN, which only a -DDPN_EXPERIMENT_SPLITS
build reads."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from bench import synth_batch
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as PP
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    prec = sys.argv[1]
    plans = sys.argv[2:]
    n = 257 * 145
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision=prec).to(dev)
    b = synth_batch(n, dev, seed=1)
    lib = L.load()
    cfg = m.point_config()

    def timed(fn, reps=100):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1) * 1e3 / reps)
        return best

    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(b['field_data'], b['forecast_h'])
    x_, y_, t_ = (PP._f32c(b[k]).reshape(-1) for k in ('x', 'y', 't'))
    cd_ = PP._f32c(b['coord_data'])
    st = [PP._f32c(s) for s in statics]
    nets = PP._net_ptrs(PP._f32c(heads), PP._f32c(evec), st)
    g_out = torch.randn(n, 6, device=dev) * 1e-3
    g_jxi = torch.randn(n, 6, 3, device=dev) * 1e-3
    geo = cfg.geometry()
    tag = os.path.basename(os.environ.get('DPN_LIB', 'product'))
    for plan in plans:
        if plan == 'default':
            os.environ.pop('DPN_WGRAD_PLAN', None)
        else:
            os.environ['DPN_WGRAD_PLAN'] = plan
        ws = PP._Workspace(n, cfg.prec, dev)
        PP._forward_points(cfg, ws, nets, x_, y_, t_, None, cd_, True, True)
        operands = torch.empty(ws.sizes.operands, dtype=torch.uint8, device=dev)
        partials = torch.empty(ws.sizes.partials, dtype=torch.uint8, device=dev)
        L.check(lib.dpn_bwd_points(PP._ptr(x_), PP._ptr(y_), PP._ptr(t_), None, PP._ptr(cd_), n, PP._ptr(PP._freqs(dev)), ctypes.byref(geo),
                                   PP._ptr(ws.packed), cfg.prec, PP._ptr(g_out), PP._ptr(g_jxi), PP._ptr(ws.saved), PP._ptr(operands), PP._stream()), 'bwd')
        us = timed(lambda: L.check(lib.dpn_wgrad(n, cfg.prec, PP._ptr(g_out), PP._ptr(ws.saved), PP._ptr(operands), PP._ptr(partials), PP._stream()), 'wgrad'))
        print('%-28s %-7s plan %-12s  %s us' % (tag, prec, plan, ' '.join('%7.1f' % u for u in us)), flush=True)
        del ws, operands, partials


if __name__ == '__main__':
    main()
