"""Cost of loss balancing by gradient norms, hi+lo mode, on the shipped batch (4 096 interior + 20 480 margin points):
median and spread (min .. max) of the timed repetitions after warm-up; the routes alternate in one process, so all see the same state of the box.
The option is not implemented for captured steps, so every route is the eager training step, timed per step in a queue of 20.

  (a) the training step as it runs without the option;
  (b) the step with the option on a step that does not refresh (every = 10^9 after the first): one dpn_balance_combine launch per direction, and
      the per-term cotangents instead of the total's;
  (c) the step with every = 1, i.e. each step a refresh: K forward + backward passes, K dpn_balance_sumsq and one dpn_balance_update on top of (b),
      at K = 7 ('equations') and at K = 3 ('parts').

usage: python tools/balance_time.py [reps]        (default 9 repetitions of 20 steps)"""
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


def _stats(v):
    return '%.3f ms (min %.3f .. max %.3f, n = %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    from deepphysinet_amd.balance import LossBalance
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    dev = torch.device('cuda:0')
    batch = SyntheticSamples(dev, leads=4, seed=1)[0]
    routes = {}
    for name, bal in (('(a) option off', None), ('(b) option on, no refresh', LossBalance(every=10 ** 9)),
                      ('(c) refresh every step, K = 7', LossBalance(every=1, groups='equations')),
                      ('(c) refresh every step, K = 3', LossBalance(every=1, groups='parts'))):
        torch.manual_seed(1)
        m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
        opt = m.build_optimizer()
        kw = {} if bal is None else {'balance': bal}
        routes[name] = (lambda m=m, opt=opt, kw=kw: m.training_step(batch, opt, with_pde=True, **kw))
        routes[name](), routes[name]()                      # warm-up (the first step of (b) is its one refresh)
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, step in routes.items():
            times[k].append(_timed(lambda: [step() for _ in range(20)]) / 20)
    print('eager training_step, %d interior + %d margin points, per step in a queue of 20:' % (batch['inter_x'].shape[0], batch['margin_x'].shape[0]))
    for k in routes:
        print('  %-32s %s' % (k, _stats(times[k])))
    a, b = statistics.median(times['(a) option off']), statistics.median(times['(b) option on, no refresh'])
    for k in ('(c) refresh every step, K = 7', '(c) refresh every step, K = 3'):
        c = statistics.median(times[k])
        print('  %s: one refresh costs %.3f ms; at every = 100 the option adds %.3f ms per step (%.1f %% of (a))'
              % (k[4:], c - b, (b - a) + (c - b) / 100.0, 100.0 * ((b - a) + (c - b) / 100.0) / a))


if __name__ == '__main__':
    main()
