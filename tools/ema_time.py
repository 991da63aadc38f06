"""Cost of the weight EMA fused into the Adam launch (FusedClipAdam(ema_decay=...)), hi+lo mode, on the flagship step: one field sample,
37 265 points, zero_grad + place_one_batch + backward + clip + Adam captured in one graph, as bench.py captures it.

  (a) the captured step without the option and with ema_decay = 0.999 (warm-up on): device time per replay in a queue of 100; both graphs live in one
      process and the legs alternate round by round, so both see the same state of the box; median and spread (min .. max) of the rounds after a
      pre-warm of one second of replays;
  (b) the optimiser's launches inside those steps (gradient norm, its reduction, the update), between two device-clock stamps queued around
      opt.step() in a second, instrumented capture of each step; the cost of a pair of stamps is measured in the same replay and subtracted.  The
      first two launches are the same code in both legs: the difference is the update launch's.

usage: python tools/ema_time.py [rounds] [--off-only] [--root DIR]
       (default 7 rounds; --off-only: the leg without the option alone; --root: import deepphysinet_amd from another checkout, for example the parent
       commit's, which has no EMA: implies --off-only)"""
import os
import socket
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
PKG_ROOT = os.path.abspath(argv[argv.index('--root') + 1]) if '--root' in argv else ROOT
sys.path.insert(0, ROOT)              # bench.synth_batch
sys.path.insert(0, PKG_ROOT)
DECAY = 0.999


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


def _captured(ema, batch, dev, stamps=None):
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    opt = m.build_optimizer(max_norm=2.5e7, **({'ema_decay': DECAY, 'ema_warmup': True} if ema else {}))
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


def main():
    from bench import synth_batch
    rounds = int(argv[0]) if argv and argv[0].isdigit() else 7
    off_only = '--off-only' in argv or PKG_ROOT != ROOT
    dev = torch.device('cuda:0')
    batch = synth_batch(257 * 145, dev, seed=1)
    legs = [('option off', False)] + ([] if off_only else [('ema_decay %g, warm-up' % DECAY, True)])
    print('host %s, device %s, package %s' % (socket.gethostname(), torch.cuda.get_device_name(0), PKG_ROOT))
    graphs, keep = {}, []
    for name, ema in legs:
        graphs[name], alive = _captured(ema, batch, dev)
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
    for k in graphs:
        print('  %-28s %s' % (k, _stats(times[k])))
        print('  %-28s raw %s' % ('', ' '.join('%.4f' % v for v in times[k])))
    if len(legs) == 2:
        a, b = (statistics.median(times[k]) for k in graphs)
        print('  difference of the medians     %+.2f us (%+.2f %%)' % ((b - a) * 1e3, (b - a) / a * 100))
    # (b) the optimiser's launches inside the step
    inst = {}
    for name, ema in legs:
        st = _Stamps(dev)
        g, alive = _captured(ema, batch, dev, stamps=st)
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
        print('  %-28s %s; a pair of stamps %.2f us' % (k, _stats(opt, 'us'), statistics.median(pair)))
    if len(legs) == 2:
        a, b = (med[k] for k in inst)
        print('  difference of the medians     %+.2f us: the update launch with the shadow (two more streams of %.1f MB)'
              % (b - a, keep[1][1]._ema_flat.numel() * 4 / 1e6))


if __name__ == '__main__':
    main()
