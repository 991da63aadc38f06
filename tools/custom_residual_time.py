"""Timing of one training step through the reference's composition on the HIP model (InterfacePhysics.fields_at -> inverse_norm -> the six
*_equation methods with their 28 gradient() calls -> loss.backward()) against the fused place_one_batch, and of the point kernels alone
(dpn_fwd_ref_derivs + dpn_bwd_points_derivs with the derivative outputs on, against dpn_fwd_ref + dpn_bwd_points_scaled).  Eager launches,
HIP events, median of the timed repetitions.

usage: python tools/custom_residual_time.py [reps] [points ...]        (default: 20 repetitions, 4096 and 20480 points)"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    from bench import synth_batch
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd import point_path as P
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sizes = [int(v) for v in sys.argv[2:]] or [4096, 20480]
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    lf = m.train_cfg['losses']['loss_factor']
    crit = torch.nn.MSELoss()
    for n in sizes:
        b = synth_batch(n, dev, seed=1)

        def fused():
            m.physics_net.zero_grad(set_to_none=True)
            m.place_one_batch(b['x'], b['y'], b['t'], b['f'], b['field_data'], b['coord_data'], b['forecast_h'], crit, lf, 0, 0, dev).backward()

        def composed():
            m.physics_net.zero_grad(set_to_none=True)
            x, y, t = (b[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
            u, v, p, T, q, rio = m.inverse_norm(*m.fields_at(x, y, t, b['field_data'], b['coord_data'], b['forecast_h']), m.obs_norm_cfg)
            f = b['f']
            loss = (m.montion_equation_u(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_u_factor'])
                    + m.montion_equation_v(x, y, t, u, v, p, rio, f, crit, factor=lf['motion_v_factor'])
                    + m.energy_equation(x, y, t, u, v, p, T, rio, q, crit, factor=lf['energy_factor'])
                    + m.continuous_equation(x, y, t, u, v, rio, crit, factor=lf['continuous_factor'])
                    + m.vapor_equation(x, y, t, u, v, p, T, q, crit, factor=lf['vapor_factor'])
                    + m.gas_equation(p, T, rio, q, crit, factor=lf['gas_factor']))
            loss.backward()

        t_fused, t_comp = _median_ms(fused, reps), _median_ms(composed, reps)
        # the point kernels alone, on the same packed weights and buffers
        lib = L.load()
        cfg = m.point_config()
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(b['field_data'], b['forecast_h'])
        st = [s.detach() for s in statics]
        nets = P._net_ptrs(heads, evec, st)
        ws = P._Workspace(n, cfg.prec, dev)
        L.check(lib.dpn_pack_weights_form(nets, cfg.prec, lib.dpn_fwd_form(cfg.prec, 0), P._ptr(ws.packed), P._stream()), 'pack')
        ws.alloc_saved()
        x, y, t = (b[k].reshape(-1).contiguous() for k in ('x', 'y', 't'))
        cd = b['coord_data'].contiguous()
        geo, fr = cfg.geometry(), P._freqs(dev)
        out = torch.empty(n, 6, device=dev)
        jac, hess, d3, g_jxi, g_hxi = (torch.randn(n, 6, 3, device=dev) for _ in range(5))
        g_out = torch.randn(n, 6, device=dev)
        operands = torch.empty(ws.sizes.operands, dtype=torch.uint8, device=dev)
        head = (P._ptr(x), P._ptr(y), P._ptr(t), None, P._ptr(cd), None, n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(out), P._ptr(jac))
        bhead = (P._ptr(x), P._ptr(y), P._ptr(t), None, P._ptr(cd), n, P._ptr(fr), ctypes.byref(geo), P._ptr(ws.packed), cfg.prec, P._ptr(g_out), P._ptr(g_jxi))
        fwd0 = lambda: L.check(lib.dpn_fwd_ref(*head, P._ptr(ws.saved), P._stream()), 'fwd')
        fwd1 = lambda: L.check(lib.dpn_fwd_ref_derivs(*head, P._ptr(hess), P._ptr(d3), P._ptr(ws.saved), P._stream()), 'fwd derivs')
        bwd0 = lambda: L.check(lib.dpn_bwd_points_scaled(*bhead, None, P._ptr(ws.saved), P._ptr(operands), P._stream()), 'bwd')
        bwd1 = lambda: L.check(lib.dpn_bwd_points_derivs(*bhead, P._ptr(g_hxi), None, P._ptr(ws.saved), P._ptr(operands), P._stream()), 'bwd derivs')
        k = [_median_ms(f_, reps) * 1e3 for f_ in (fwd0, fwd1, bwd0, bwd1)]
        print('%6d points: step place_one_batch %.3f ms | fields_at + reference composition %.3f ms (x%.2f) || point kernels: fwd %.1f -> %.1f us '
              '(+ 2nd / 3rd derivatives), bwd stage 1 %.1f -> %.1f us (+ g_hxi)' % (n, t_fused, t_comp, t_comp / t_fused, k[0], k[1], k[2], k[3]))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
