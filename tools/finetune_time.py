"""What fine-tuning costs and saves on one box and one build (hi+lo mode), at the reference's 4 096 interior + 20 480 margin points:

  legs   (a) every parameter trainable, one parameter group -- the step of before;
         (b) every parameter trainable, three groups (hyper-network heads | biases and LayerNorm | the rest) that all carry leg (a)'s values: the
             update launch looks up its tensor's group row (dpn_clip_adam_flat_groups) and the weights take leg (a)'s trajectory bit for bit, so
             (b) - (a) is the cost of the lookup alone;
         (b2) the same three groups as one would configure them: heads at lr / 10, biases and LayerNorm without weight decay.  The weights take
             another trajectory, and the step's kernels are not data-blind: (b2) - (b) is what the VALUES cost, not the groups;
         (c) the encoder frozen (freeze=['meta_net.*']), one group over the 84 tensors left: the encoder's whole backward does not run.
  eager      InterfacePhysics.training_step (data + interior PDE + margin PDE, backward, clip + Adam), wall time per step over blocks of 50 steps
             that end in a device synchronise;
  captured   StagedPdeStep's stages + the optimiser step in ONE graph over the same 24 576 points, device time per replay in a queue of 100;
  optimiser  the optimiser's launches inside that captured step, between device-clock stamps (the cost of a pair of stamps is measured in the same
             replay and subtracted).
All legs live in one process and alternate round by round after a pre-warm of one second, so they see the same state of the box; every figure is the
median over the rounds with its spread (min .. max).

usage: python tools/finetune_time.py [rounds] [--baseline-only] [--root DIR] [--json PATH]
       (default 7 rounds; --baseline-only: leg (a) alone; --root: import deepphysinet_amd from another checkout, for example the parent commit's, which
       has no groups and no freeze(): implies --baseline-only; --json: also write the figures there)"""
import json
import os
import socket
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
PKG_ROOT = os.path.abspath(argv[argv.index('--root') + 1]) if '--root' in argv else ROOT
sys.path.insert(0, ROOT)              # bench.synth_batch, tools.ema_time
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, PKG_ROOT)
N_INTER, N_MARGIN = 4096, 20480
MATCH = (['*_net.coord_*_fc.*', '*_net.fore_h_fc.*'], ['*.bias', '*norm*'])
LEGS = {'a: all trainable, 1 group': {},
        'b: 3 groups, same values': dict(param_groups=[dict(match=MATCH[0]), dict(match=MATCH[1])]),
        'b2: 3 groups, lr / 10, wd 0': dict(param_groups=[dict(match=MATCH[0], lr=1e-5), dict(match=MATCH[1], weight_decay=0.0)]),
        'c: encoder frozen': dict(freeze=['meta_net.*'])}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v), raw=[round(x, 5) for x in v])


def _text(s, unit):
    return '%.4f %s (min %.4f .. max %.4f, n = %d)' % (s['median'], unit, s['min'], s['max'], s['n'])


def _model(tune, dev):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    return m, m.build_optimizer(max_norm=2.5e7, **tune)


def _captured(tune, batch, dev, stamps=None):
    from deepphysinet_amd.interface.interface_physics import StagedPdeStep
    m, opt = _model(tune, dev)
    st = StagedPdeStep(m, opt, batch)

    def step():
        for stage in st.stages:
            stage()
        if stamps is not None:
            stamps.stamp(), stamps.stamp(), stamps.stamp()
        opt.step()
        if stamps is not None:
            stamps.stamp()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(), step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g, (m, opt, st)


def main():
    from bench import synth_batch
    from ema_time import _Stamps
    from deepphysinet_amd import grad_arena
    from deepphysinet_amd.sampler import SyntheticSamples
    rounds = int(argv[0]) if argv and argv[0].isdigit() else 7
    legs = dict(list(LEGS.items())[:1]) if ('--baseline-only' in argv or PKG_ROOT != ROOT) else LEGS
    dev = torch.device('cuda:0')
    out = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0), package=PKG_ROOT, points=dict(interior=N_INTER, margin=N_MARGIN),
               rounds=rounds, legs={k: {} for k in legs})
    print('host %s, device %s, package %s' % (out['host'], out['device'], PKG_ROOT))
    # ---- eager training_step (before anything is captured: a captured fused step makes the encoder cache distrust its keys, grad_arena)
    sample = SyntheticSamples(dev, n_margin=N_MARGIN, n_inter=N_INTER, leads=1, seed=0)[0]
    eager = {k: _model(tune, dev) for k, tune in legs.items()}
    run = lambda m, opt: [m.training_step(sample, opt, with_pde=True) for _ in range(50)]
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:                     # pre-warm: the clocks ramp over the first tens of milliseconds
        for m, opt in eager.values():
            m.training_step(sample, opt, with_pde=True)
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (m, opt) in eager.items():
            times[k].append(_timed(lambda: run(m, opt)) / 50)
    print('eager training_step, %d + %d points, wall time per step in blocks of 50, legs alternating, %d rounds:' % (N_INTER, N_MARGIN, rounds))
    for k in legs:
        out['legs'][k]['eager_ms'] = _summary(times[k])
        out['legs'][k]['tensors'] = len(eager[k][1].params)
        out['legs'][k]['groups'] = len(eager[k][1].param_groups)
        print('  %-28s %s' % (k, _text(out['legs'][k]['eager_ms'], 'ms')))
    del eager
    # ---- the captured staged step
    batch = synth_batch(N_INTER + N_MARGIN, dev, seed=1)
    was = grad_arena.captured_step[0]
    graphs, keep = {}, []
    for k, tune in legs.items():
        graphs[k], alive = _captured(tune, batch, dev)
        keep.append(alive)
        out['legs'][k]['stages'] = len(alive[2].stages)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(_timed(lambda: [g.replay() for _ in range(100)]) / 100)
    print('captured StagedPdeStep + optimiser step, %d points, per replay in a queue of 100, legs alternating, %d rounds:' % (batch['x'].numel(), rounds))
    for k in graphs:
        out['legs'][k]['captured_ms'] = _summary(times[k])
        print('  %-28s %s' % (k, _text(out['legs'][k]['captured_ms'], 'ms')))
    # ---- the optimiser's launches inside the step
    inst = {}
    for k, tune in legs.items():
        st = _Stamps(dev)
        g, alive = _captured(tune, batch, dev, stamps=st)
        keep.append(alive)
        inst[k] = (g, st)
    for g, st in inst.values():
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        st.cursor.zero_()
    for _ in range(rounds):
        for g, st in inst.values():
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
    print('clip + Adam launches (gradient norm, reduction, update) inside the captured step, device clock, %d replays:' % (20 * rounds))
    for k, (g, st) in inst.items():
        pair, opt = st.intervals()
        s = _summary(opt)
        s.pop('raw')
        out['legs'][k]['optimizer_us'] = dict(s, stamp_pair_us=statistics.median(pair))
        print('  %-28s %s; a pair of stamps %.2f us' % (k, _text(s, 'us'), statistics.median(pair)))
    grad_arena.captured_step[0] = was
    names = list(legs)
    if len(names) > 1:
        print('differences of the medians against leg (a):')
        for what, unit, key in (('eager', 'ms', 'eager_ms'), ('captured', 'ms', 'captured_ms'), ('optimiser', 'us', 'optimizer_us')):
            ma = out['legs'][names[0]][key]['median']
            for k in names[1:]:
                d = out['legs'][k][key]['median'] - ma
                print('  %-10s %-30s %+.4f %s (%+.2f %%)' % (what, k, d, unit, d / ma * 100))
                out.setdefault('differences', {}).setdefault(key, {})[k] = dict(minus_a=d, percent=d / ma * 100)
    if '--json' in argv:
        path = argv[argv.index('--json') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote %s' % path)


if __name__ == '__main__':
    main()
