"""Cost of causal time weighting of the PDE losses, hi+lo mode, on the shipped batch (4 096 interior + 20 480 margin points): median and spread
(min .. max) of the timed repetitions after warm-up; the routes alternate in one process, so all see the same state of the box.

  (a) the training step captured in a graph, as it runs without the option: device time per replay;
  (b) the same with causal=CausalWeights(eps=1, bins=16): per group two more launches (bins, weights), the weighted residual kernel in both passes;
  (c) the three new launches alone on the interior group's fields: dpn_causal_bins + dpn_causal_weights + dpn_residual_weighted (loss rows and unit
      cotangents), against the plain dpn_residual on the same fields, per call in a queue of 20.

usage: python tools/causal_time.py [reps]        (default 9 repetitions of 20 replays)"""
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v, unit='ms', scale=1.0):
    v = [x * scale for x in v]
    return '%.3f %s (min %.3f .. max %.3f, n = %d)' % (statistics.median(v), unit, min(v), max(v), len(v))


def _captured(m, batch, causal):
    """The training step captured after two warm-up steps on a side stream (as bench.py captures it)."""
    opt = m.build_optimizer()
    kw = {} if causal is None else {'causal': causal}
    step = lambda: m.training_step(batch, opt, with_pde=True, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(), step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def main():
    from deepphysinet_amd import _lib as L
    from deepphysinet_amd.causal import CausalWeights
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.point_path import _causal_group, _one, _ptr, _stream, pde_fields_and_jacobian
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    dev = torch.device('cuda:0')
    causal = CausalWeights(eps=1.0, bins=16)
    batch = SyntheticSamples(dev, leads=4, seed=1)[0]
    graphs = {}
    for name, opt in (('option off', None), ('causal eps 1, 16 bins', causal)):
        torch.manual_seed(1)
        graphs[name] = _captured(builder_models(**ncep_config(), precision='bf16x2').to(dev), batch, opt)
    times = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            times[k].append(_timed(lambda: [g.replay() for _ in range(20)]) / 20)
    n = batch['inter_x'].shape[0]
    print('captured training_step, %d interior + %d margin points, per replay in a queue of 20:' % (n, batch['margin_x'].shape[0]))
    for k in graphs:
        print('  %-24s %s' % (k, _stats(times[k])))
    # (c) the new launches alone
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    cfg = m.point_config()
    lib = L.load()
    with torch.no_grad():
        heads, evec, statics = m.physics_net.field_weights(batch['field_data'], batch['forecast_h'])
        x, y, t, f = (batch['inter_' + k].reshape(-1).contiguous() for k in 'xytf')
        out_n, jac_n = pde_fields_and_jacobian(cfg, x, y, t, batch['inter_data'], heads, evec, statics)
    geo, ph = cfg.geometry(), cfg.physics()
    sums = torch.empty(((n + 255) // 256) * 6, dtype=torch.float64, device=dev)
    g_out, g_jxi = torch.empty((n, 6), device=dev), torch.empty((n, 6, 3), device=dev)
    args = (_ptr(out_n), _ptr(jac_n), _ptr(f), n, ctypes.byref(geo), ctypes.byref(ph), None, _ptr(_one(dev)), _ptr(sums), _ptr(g_out), _ptr(g_jxi))

    def plain():
        L.check(lib.dpn_residual(*args, _stream()), 'dpn_residual')

    def weighted():
        bin_, w32, _ = _causal_group(cfg, causal, out_n, jac_n, f, t, 0, n)
        L.check(lib.dpn_residual_weighted(*args, None, _ptr(bin_), _ptr(w32), _stream()), 'dpn_residual_weighted')
    for name, fn in (('dpn_residual', plain), ('bins + weights + dpn_residual_weighted', weighted)):
        fn(), fn()
        ts = [_timed(lambda: [fn() for _ in range(20)]) / 20 for _ in range(reps)]
        print('%d interior points, %-40s per call in a queue of 20: %s' % (n, name, _stats(ts, 'us', 1e3)))


if __name__ == '__main__':
    main()
