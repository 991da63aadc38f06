#!/usr/bin/env python
"""One optimiser step on B samples (InterfacePhysics.training_step_batch) against B calls of training_step on the same samples.

    python tools/lead_step_time.py                      # B = 4 samples of 256 + 1024 points
    python tools/lead_step_time.py --full               # 61 x (4096 + 20480) and 8 x (4096 + 20480): BASELINE configs[2]'s size
    python tools/lead_step_time.py --batch 8 --n_inter 4096 --n_margin 20480 --steps 5

Per size one worker process measures both legs (same process, same box, legs alternating round by round; device events around whole steps,
the median over the rounds) and prints one JSON line: ms per sample, points per second, torch.cuda.max_memory_allocated of each leg.  The driver
(this process: it never touches the GPU) starts the workers one after the other, each under its own `timeout`, and stops at the first one that does
not exit cleanly: nothing more is started on a device that has faulted or hung."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, ROOT)
    import socket
    import torch
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    from deepphysinet_amd.utils.init import scaled_init_
    dev = torch.device('cuda:0')
    m = builder_models(**ncep_config(), precision=args.precision)
    scaled_init_(m.physics_net, seed=1)
    m.to(dev)
    opt = m.build_optimizer()
    src = SyntheticSamples(dev, n_margin=args.n_margin, n_inter=args.n_inter, leads=args.batch)
    samples = [src[i] for i in range(args.batch)]

    def batched():
        m.training_step_batch(samples, opt, with_pde=True)

    def looped():
        for b in samples:
            m.training_step(b, opt, with_pde=True)

    legs = {'batch': batched, 'loop': looped}
    times, peak = {k: [] for k in legs}, {}
    for name, fn in legs.items():                        # warm-up, and each leg's peak memory on its own
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
    for _ in range(args.steps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    pts = args.n_inter + args.n_margin
    row = {'box': socket.gethostname(), 'device': torch.cuda.get_device_name(0), 'precision': args.precision, 'B': args.batch, 'n_inter': args.n_inter,
           'n_margin': args.n_margin, 'steps': args.steps, 'warmup': args.warmup}
    for name in legs:
        t = sorted(times[name])
        med = t[len(t) // 2]
        row[name] = {'ms_per_sample': med / args.batch, 'ms_min': t[0] / args.batch, 'ms_max': t[-1] / args.batch,
                     'points_per_s': pts * args.batch / (med * 1e-3), 'max_memory_allocated': peak[name]}
    row['loop_over_batch'] = row['loop']['ms_per_sample'] / row['batch']['ms_per_sample']
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--n_inter', type=int, default=256)
    ap.add_argument('--n_margin', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--precision', default='bf16x2')
    ap.add_argument('--full', action='store_true', help='61 and 8 samples of 4096 + 20480 points instead of --batch / --n_inter / --n_margin')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per worker')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    sizes = [(61, 4096, 20480), (8, 4096, 20480)] if args.full else [(args.batch, args.n_inter, args.n_margin)]
    for B, n_i, n_m in sizes:
        cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--worker', '--batch', str(B), '--n_inter', str(n_i),
               '--n_margin', str(n_m), '--steps', str(args.steps), '--warmup', str(args.warmup), '--precision', args.precision]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                      # a fault, an abort or the time limit: nothing more runs on this device
            raise SystemExit('lead_step_time: %d x (%d + %d) ended with status %d; stopping here' % (B, n_i, n_m, rc))


if __name__ == '__main__':
    main()
