"""Cost of the step guard inside the fused clip + Adam step (FusedClipAdam(skip_nonfinite / spike_factor)), hi+lo mode, on the captured training
step at 4 096 + 20 480 points: zero_grad + place_one_batch + backward + clip + Adam captured in one graph, as bench.py captures it.

  (a) the captured step in three variants -- without the guard (the parent's launches: the optimiser never reaches the new entry point), with
      skip_nonfinite, with the spike rule (spike_factor 10) -- device time per replay in a queue of 100; all graphs live in one process and the legs
      alternate round by round, so they see the same state of the box; median and spread (min .. max) of the rounds after a pre-warm of one second
      of replays;
  (b) the optimiser's launches inside those steps (gradient norm, its reduction, the update), between two device-clock stamps queued around
      opt.step() in a second, instrumented capture of each step; the cost of a pair of stamps is measured in the same replay and subtracted.  A
      fourth leg here trains on a field sample that holds a NaN: every step is refused, its update launch returns early -- the cost of a skipped step.

usage: python tools/guard_time.py [rounds]          (default 7 rounds)
       python tools/guard_time.py --trace-leg K    (leg K = 0, 1, 2 alone: capture, pre-warm, 300 replays; for a run of its own under
                                                    `rocprofv3 --kernel-trace --stats -- python tools/guard_time.py --trace-leg K`)"""
import os
import socket
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
sys.path.insert(0, ROOT)              # bench.synth_batch
POINTS = 4096 + 20480
LEGS = [('without the guard', {}), ('skip_nonfinite', dict(skip_nonfinite=True)),
        ('spike rule (factor 10)', dict(spike_factor=10.0, spike_warmup=100, spike_patience=5))]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v, unit='ms'):
    return '%.4f %s (min %.4f .. max %.4f, n = %d)' % (statistics.median(v), unit, min(v), max(v), len(v))


class _Stamps:
    """Device-clock stamps (dpn_clock_stamp: a one-thread kernel appending wall_clock64 to a ring) queued inside a captured step."""

    def __init__(self, dev, cap=1 << 14):
        import ctypes
        from deepphysinet_amd import _lib as L
        self.L, self.cap = L, cap
        self.ring = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        khz = ctypes.c_int(0)
        L.check(L.load().dpn_clock_rate_khz(ctypes.byref(khz)), 'dpn_clock_rate_khz')
        self.khz = khz.value

    def stamp(self):
        import ctypes
        self.L.check(self.L.load().dpn_clock_stamp(ctypes.c_void_p(self.ring.data_ptr()), ctypes.c_void_p(self.cursor.data_ptr()), self.cap,
                                                   torch.cuda.current_stream().cuda_stream), 'dpn_clock_stamp')

    def intervals(self):
        """[replays][4] stamps -> (pair us, optimiser us minus the pair) per replay."""
        n = int(self.cursor.item())
        t = self.ring[:n - n % 4].cpu().view(-1, 4).double() * (1e3 / self.khz)
        pair, opt = (t[:, 1] - t[:, 0]), (t[:, 3] - t[:, 2])
        return pair.tolist(), (opt - pair).tolist()


def _captured(guard_kw, batch, dev, stamps=None):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    opt = m.build_optimizer(max_norm=2.5e7, **guard_kw)
    lf = m.train_cfg['losses']['loss_factor']
    crit = torch.nn.MSELoss()
    one = torch.ones((), dtype=torch.float32, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = m.place_one_batch(batch['x'], batch['y'], batch['t'], batch['f'], batch['field_data'], batch['coord_data'], batch['forecast_h'],
                                 crit, lf, 0, 0, dev)
        loss.backward(one)
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
    return g, (m, opt)


def trace_leg(k):
    from bench import synth_batch
    dev = torch.device('cuda:0')
    g, alive = _captured(LEGS[k][1], synth_batch(POINTS, dev, seed=1), dev)
    for _ in range(300):
        g.replay()
    torch.cuda.synchronize()
    print('leg %d (%s): 300 replays' % (k, LEGS[k][0]))


def main():
    from bench import synth_batch
    if '--trace-leg' in argv:
        return trace_leg(int(argv[argv.index('--trace-leg') + 1]))
    rounds = int(argv[0]) if argv and argv[0].isdigit() else 7
    dev = torch.device('cuda:0')
    batch = synth_batch(POINTS, dev, seed=1)
    print('host %s, device %s' % (socket.gethostname(), torch.cuda.get_device_name(0)))
    graphs, keep = {}, []
    for name, kw in LEGS:
        graphs[name], alive = _captured(kw, batch, dev)
        keep.append(alive)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:                     # pre-warm: the clocks ramp over the first tens of milliseconds
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(_timed(lambda: [g.replay() for _ in range(100)]) / 100)
    print('captured step, %d points, per replay in a queue of 100, legs alternating, %d rounds:' % (batch['x'].numel(), rounds))
    base = statistics.median(times[LEGS[0][0]])
    for k in graphs:
        print('  %-36s %s' % (k, _stats(times[k])))
        print('  %-36s raw %s' % ('', ' '.join('%.4f' % v for v in times[k])))
        if k != LEGS[0][0]:
            d = statistics.median(times[k]) - base
            print('  %-36s difference of the medians %+.2f us (%+.2f %%)' % ('', d * 1e3, d / base * 100))
    for (name, _), (_, opt) in zip(LEGS[1:], keep[1:]):
        st = opt.guard_stats()
        print('  %-36s guard: %d calls, skipped_nonfinite %d, skipped_spike %d' % (name, int(opt.step_count), st['skipped_nonfinite'], st['skipped_spike']))
    # (b) the optimiser's launches inside the step; the last leg: every step refused
    bad = dict(batch, field_data=batch['field_data'].clone())
    bad['field_data'].view(-1)[0] = float('nan')
    inst = {}
    for name, kw, b in [(n, kw, batch) for n, kw in LEGS] + [('skip_nonfinite, every step skipped', dict(skip_nonfinite=True), bad)]:
        st = _Stamps(dev)
        g, alive = _captured(kw, b, dev, stamps=st)
        keep.append(alive)
        inst[name] = (g, st)
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
    med = {}
    for k, (g, st) in inst.items():
        pair, opt = st.intervals()
        med[k] = statistics.median(opt)
        print('  %-36s %s; a pair of stamps %.2f us' % (k, _stats(opt, 'us'), statistics.median(pair)))
    for k in list(med)[1:]:
        print('  %-36s difference of the medians to the leg without the guard %+.2f us' % (k, med[k] - med[LEGS[0][0]]))
    st = keep[-1][1].guard_stats()
    print('  the skipped leg: %d calls, skipped_nonfinite %d' % (int(keep[-1][1].step_count), st['skipped_nonfinite']))


if __name__ == '__main__':
    main()
