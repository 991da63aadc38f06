#!/usr/bin/env python
"""Times the L-BFGS refinement on one MI355X at the flagship point counts (4 096 interior + 20 480 margin points):

  * one closure (InterfacePhysics.loss_and_gradients plus the loss read-back),
  * FusedLBFGS.step at history_size m and `--iters` iterations,
  * torch.optim.LBFGS(line_search_fn='strong_wolfe') with the same settings driving the same closure,

and reports for both the optimiser's OWN time per iteration, (step - evaluations x closure) / iterations, in `--rounds` rounds that alternate the two
routes (DESIGN.md section 7's criterion: the slowest round of the new route against the fastest round of torch's), and the launches of one FusedLBFGS
iteration by entry point.  Every round starts from the same weights.  Prints one JSON line.

    python tools/lbfgs_time.py [--m 10] [--iters 20] [--rounds 5] [--inter 4096] [--margin 20480]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inter', type=int, default=4096)
    ap.add_argument('--margin', type=int, default=20480)
    args = ap.parse_args()
    from deepphysinet_amd import _lib, grad_arena
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.lbfgs import FusedLBFGS
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_

    dev = torch.device('cuda:0')
    m = builder_models(**ncep_config(), precision='bf16x2')
    scaled_init_(m.physics_net, seed=1)
    m = m.to(dev)
    batch = SyntheticSamples(dev, n_margin=args.margin, n_inter=args.inter, leads=1, seed=3)[0]
    params = list(m.physics_net.parameters())
    start = [p.detach().clone() for p in params]
    settings = dict(lr=1.0, max_iter=args.iters, max_eval=100 * args.iters, history_size=args.m, tolerance_grad=0.0, tolerance_change=0.0)

    def restore():
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        grad_arena.param_epoch[0] += 1

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    fused = FusedLBFGS(params, **settings)
    evals = [0]

    def closure():
        evals[0] += 1
        return m.loss_and_gradients(batch, fused, with_pde=True)[0]

    for _ in range(3):                                  # warm-up: allocations, the encoder's caches
        float(closure())
    closure_ms = min(timed(lambda: float(closure()))[0] for _ in range(10))

    def run_fused():
        restore()
        evals[0] = 0
        ms, _ = timed(lambda: fused.step(closure))
        last = fused.last
        return dict(ms=ms, iters=last['iters'], evals=last['evals'], status=last['status'], f0=last['f0'], f=last['f'],
                    own_ms_per_iter=(ms - last['evals'] * closure_ms) / max(last['iters'], 1))

    def run_torch():
        restore()
        opt = torch.optim.LBFGS(params, line_search_fn='strong_wolfe', **settings)
        evals[0] = 0
        f = []

        def torch_closure():
            grad_arena.param_epoch[0] += 1              # torch moved the parameters: caches keyed on the epoch must miss, as after FusedLBFGS.move
            loss = closure()
            fused.gather_gradients()
            f.append(float(loss))
            return loss
        ms, _ = timed(lambda: opt.step(torch_closure))
        st = opt.state[params[0]]
        return dict(ms=ms, iters=st['n_iter'], evals=st['func_evals'], f0=f[0], f=min(f),
                    own_ms_per_iter=(ms - st['func_evals'] * closure_ms) / max(st['n_iter'], 1))

    run_fused(), run_torch()                            # one unrecorded round of each
    rounds = [dict(fused=run_fused(), torch=run_torch()) for _ in range(args.rounds)]

    # the launches of one iteration: entry points called between two dpn_lbfgs_direction calls, with history full
    lib, names, calls = _lib.load(), [k for k in _lib.EXPORTS if k.startswith('dpn_lbfgs_') and k != 'dpn_lbfgs_scratch_doubles'], []
    inner = {k: getattr(lib, k) for k in names}
    for k in names:
        setattr(lib, k, (lambda name: lambda *a: (calls.append(name), inner[name](*a))[1])(k))
    try:
        run_fused()
    finally:
        for k in names:
            setattr(lib, k, inner[k])
    cut = [i for i, k in enumerate(calls) if k == 'dpn_lbfgs_gram']
    one = calls[cut[-2]:cut[-1]] if len(cut) >= 2 else calls
    tables = -(-len(params) // 160)
    per_entry = {'dpn_lbfgs_gram': tables + 1, 'dpn_lbfgs_direction': 1 + tables, 'dpn_lbfgs_save': tables, 'dpn_lbfgs_move': tables,
                 'dpn_lbfgs_gtd': tables + 1, 'dpn_lbfgs_push': tables + 1}
    slow_fused = max(r['fused']['own_ms_per_iter'] for r in rounds)
    fast_torch = min(r['torch']['own_ms_per_iter'] for r in rounds)
    print(json.dumps(dict(points=[args.inter, args.margin], history_size=args.m, closure_ms=closure_ms, rounds=rounds,
                          slowest_fused_own_ms_per_iter=slow_fused, fastest_torch_own_ms_per_iter=fast_torch, criterion_met=bool(slow_fused < fast_torch),
                          calls_last_iteration=one, kernel_launches_last_iteration=sum(per_entry[k] for k in one))))


if __name__ == '__main__':
    main()
