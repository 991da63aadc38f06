#!/usr/bin/env python
"""Benchmark of the physics-informed training step on MI355X (one process per GPU).

    python bench.py [--gpus N --steps 200 --warmup 20] [--prec bf16] [--leads 61]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
`python bench.py --gpus N` without a torchrun environment starts the N ranks itself (a child `torch.distributed.run`, before this
process has touched a GPU) and exits with the child's code.

Workload (BASELINE.json configs[1], SURVEY.md 8d "cfg2"): one field sample on the 0.25 degree grid (257 x 145 =
37 265 collocation points, every grid node, t drawn per point), all six primitive-equation residual losses.
One step = place_one_batch (encoder + hyper-network heads + fused HIP forward/Jacobian + residuals) + backward to
all 155 parameter tensors + clip_grad_norm_(2.5e7) + Adam step, captured in one hipGraph; inputs are resident in HBM.
With N > 1 every rank runs its own field sample (weak scaling, as the reference's DistributedSampler does); the step is cut into three
hipGraphs where a bucket of gradients is complete (point backward | heads backward | encoder backward) and each bucket's RCCL
all-reduce -- in place on a slice of the optimiser's flat gradient buffer -- is queued behind its graph, so it runs under the rest of
the backward pass; the fused optimiser follows the last bucket.
Default precision: bf16x2 (hi+lo split bf16 MFMA operands), the mode whose PDE losses are parity-tested at 1e-4; plain bf16 operands
(--prec bf16) are reported under `other_precision_mode`.
--leads B: BASELINE configs[2], B field samples x 37 265 points in one step (place_lead_batch).

Protocol of a plain run: `warmup` replays, a pre-warm to a steady clock (untimed, --no-prewarm skips it), the state from right after
the capture restored, then ONE timed block of `steps` replays, bracketed by barrier + synchronize; `ms_per_step` is that block / `steps`, the MAX over the ranks.
The timed steps therefore start from the same parameters and optimiser state from run to run, however many replays the clock took to settle, and
`--dump-outputs DIR` writes what the last of them computed (loss, gradient norm, every gradient and updated parameter as DIR/<name>.npy, float32).
Protocol of `--full`: `first_block_ms` (the `warmup` + `steps` replays straight after the capture), a pre-warm to a steady clock, then `--blocks`
(10) blocks of `steps` replays; `ms_per_step` is the median block, every block time the MAX over the ranks; then every extra listed below.
Lead batches start every block from a restored state and check that it stayed finite (a draw of the fields that hits the reference formula's NaN
is discarded).
N > 1 over RCCL: the measurement runs as segment graphs + host-issued all-reduces; with --full and DPN_BENCH_TRY_FORMS=1 the one-graph form (all-reduces
captured) is tried at the END and reported if faster -- a stall of that trial keeps the finished line (exit code 14).  Environment: DPN_BENCH_WATCHDOG_S (300), DPN_PG_TIMEOUT_S (600),
DPN_BENCH_TRIAL_WATCHDOG_S (90), DPN_BENCH_TRY_FORMS=1 (the end-of-run trial: opt-in), DPN_BENCH_CAPTURE_COLLECTIVES=0|1 (pin the form), DPN_BENCH_RCCL_ONE_RANK=1 /
DPN_BENCH_ONE_DEVICE=1 + DPN_BENCH_BACKEND=gloo (exercise the N > 1 code path on a one-GPU box), DPN_BENCH_SPLIT_STEP=1.

Prints ONE JSON line on rank 0: the contract keys, `config`, `switches` (every DPN_* variable and non-default frozen switch) and `collective`
(devices, buckets); with --full also `roofline` (the fused forward + Jacobian kernel, MFMA-bound; duration from device-clock stamp
nodes around its launch INSIDE the replayed step graph, `roofline.in_step`; `kernel_ms_eager_pair` = a HIP event pair around eager launches),
`roofline_hbm_kernel` (dpn_wgrad_kernel, backward stage 1), `pde_losses` (the six scalars of the workload), `collective` per-rank times, exposed
all-reduce time and step-form trial, `other_precision_mode`, `lead_batch_full` (61 fields in one step), `lead_batch_probe` (8 fields),
`cpu_baseline` (the oracle on the host cores, reference schedule + shared-derivative variant).
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

TRIAL_STALL_EXIT = 14        # exit code of a rank whose opt-in end-of-run one-graph trial stalled (the segment form's line has been printed by rank 0)

ALG_FLOP_FWD_JAC = 11_218_944          # algorithmic FLOP per collocation point, fwd + Jacobian
ALG_FLOP_STEP = 31_887_360             # fwd + Jacobian + bwd
EXEC_MAC_FWD = 278_528                 # MACs per point per net issued by dpn_fwd_tiles_kernel: five GEMMs (w1, A = W1 w2, B = W1 Wd, A^T, w1^T; csrc/dpn_layout.h)
EXEC_MAC_FWD_RING = 409_600            # ... by the ring kernel dpn_fwd_kernel (plain bf16): the seven GEMMs of variable_net.py:49-87
EXEC_MAC_BWD1 = 49_152                 # backward stage 1: w1 Z0 (192 x 256) per point per net (round 5: the Z products are gone, csrc dpn_finish_gside_kernel)
MFMA_PEAK_BF16 = 2.5e15                # dense bf16 MFMA peak, MI355X_MICROARCH.md
HBM_PEAK = 8.0e12                      # HBM3E, MI355X_MICROARCH.md
# HBM bytes per launch of the two roofline kernels come from the rocprofv3 PMC passes committed in profiles/ (bench.py cannot run PMC
# passes on itself): profiles/pmc_traffic.json, written by tools/pmc_traffic.py from the FETCH_SIZE / WRITE_SIZE passes of
# tools/refresh_profiles.sh (2 x FETCH_SIZE + WRITE_SIZE, the guide's gfx950 correction), keyed "<kernel>|<prec>|<points>".
PMC_TRAFFIC_FILE = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')


def pmc_traffic(kernel, prec, points):
    try:
        with open(PMC_TRAFFIC_FILE) as fh:
            tab = json.load(fh)
    except (OSError, ValueError):
        return None, None
    e = tab.get('%s|%s|%d' % (kernel, prec, points))
    return (e['bytes'], e.get('source')) if e else (None, None)


def synth_batch(n_points, device, seed, lon=257, lat=145, dx=27000.0, dy=27000.0):
    """SURVEY.md 8(d) synthetic inputs; points = grid nodes in row-major order (all of them when n_points = lon*lat)."""
    g = torch.Generator().manual_seed(seed)
    field = torch.randn(1, 159, 2405, generator=g)
    field[:, 155:, :] = torch.rand(1, 4, 2405, generator=g)
    idx = torch.arange(n_points) % (lon * lat)
    x = (idx % lon).float() * dx
    y = (idx // lon).float() * dy
    t = torch.randint(0, 25, (n_points,), generator=g).float() * 3600.0
    f = 2.0 * 7.29e-5 * torch.sin((18.0 + y / dy * 0.25) * torch.pi / 180.0)
    cd = torch.randn(n_points, 6, generator=g)
    fh = torch.full((1, 1, 1), 24.0 / 360.0)
    b = dict(field_data=field, forecast_h=fh, x=x.reshape(-1, 1), y=y.reshape(-1, 1), t=t.reshape(-1, 1), f=f.reshape(-1, 1).float(),
             coord_data=cd)
    return {k: v.to(device) for k, v in b.items()}


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def dump_outputs(path, loss, opt, net):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy in float32 -- the loss, the global gradient norm of the clip,
    every parameter's gradient (grad.<name>) and every parameter as the optimiser left it (param.<name>): 2 x 5.6 M values, 45 MB."""
    import numpy as np
    names = {id(p): n for n, p in net.named_parameters()}
    arrays = {'loss': loss, 'grad_norm': opt.grad_norm}
    for p, g in zip(opt.params, opt._slots):               # the flat buffer's view of each gradient: what the step's backward wrote
        arrays['grad.' + names[id(p)]] = g
        arrays['param.' + names[id(p)]] = p
    total = sum(v.numel() * 4 for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit('bench.py --dump-outputs: %d bytes of outputs exceed the %d-byte limit' % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + '.npy'), v.detach().float().cpu().numpy())


def cpu_baseline(sample_points, seed, share_derivatives=False):
    """The CPU oracle (reference-faithful: 28 autograd.grad calls + double backward; or, share_derivatives, the 18 distinct derivatives
    taken once) on a bounded sample of the same workload."""
    from oracle import dpn_oracle as O
    torch.manual_seed(seed)
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    m = builder_models(**ncep_config())
    st = {k: v.detach().clone().requires_grad_(v.is_floating_point() and not k.endswith('.pe')) for k, v in m.physics_net.state_dict().items()}
    b = synth_batch(sample_points, 'cpu', seed)
    geo = O.Geometry()
    names = O.param_names(st)
    best = None
    for it in range(4):                        # 1 warm-up + best of 3
        x, y, t = (b[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
        t0 = time.perf_counter()
        tot = O.place_one_batch(st, x, y, t, b['f'], b['field_data'], b['coord_data'], b['forecast_h'], geo, share_derivatives=share_derivatives)
        torch.autograd.grad(tot, [st[n] for n in names])
        dt = time.perf_counter() - t0
        if it > 0:
            best = dt if best is None else min(best, dt)
    return sample_points / best, best


def sample_power(work, seconds=2.0):
    """Median shader clock and socket power (rocm-smi) while `work()` keeps the GPU busy for `seconds`: the MFMA-heavy point kernels run AT the
    socket's power cap, where the clock -- and with it the MFMA peak a kernel can be priced against -- is what the power management leaves
    (profiles/round4_point_kernel_clocks.txt).  None when rocm-smi is not there or says nothing."""
    import shutil, statistics, subprocess, threading
    smi = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(smi):
        return None
    rows, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            try:
                d = json.loads(subprocess.run([smi, '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=10).stdout)
                c = d[sorted(d)[0]]
                clk = [v for k, v in c.items() if k.startswith('sclk clock speed')]
                pw = [v for k, v in c.items() if 'Power (W)' in k]
                rows.append((float(str(clk[0]).strip('()Mhz')), float(pw[0])))
            except Exception:       # noqa
                pass
            time.sleep(0.05)
    th = threading.Thread(target=sampler, daemon=True)
    th.start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        work()
        torch.cuda.synchronize()
    stop.set()
    th.join(timeout=15)
    rows = rows[1:] if len(rows) > 3 else rows           # the first sample may predate the load
    if not rows:
        return None
    return {'sclk_mhz': statistics.median(r[0] for r in rows), 'socket_w': statistics.median(r[1] for r in rows), 'samples': len(rows),
            'source': 'rocm-smi --showclocks --showpower, median over %.1f s of back-to-back work' % seconds}


def launch_ranks(n, argv):
    """`python bench.py --gpus N` outside torchrun: start the N ranks as a CHILD torch.distributed.run and hand back its exit code.  The
    parent may already have touched the GPU runtime (on ROCm torch.cuda.device_count() can fall through to hipGetDeviceCount), so it only
    ever SPAWNS a child -- it must never exec another program in its own process (that takes the machine down on this pool)."""
    import socket
    import subprocess
    one_device = os.environ.get('DPN_BENCH_ONE_DEVICE') == '1'
    have = torch.cuda.device_count()
    if have < (1 if one_device else n):
        print('bench.py --gpus %d: only %d GPU(s) visible on this node' % (n, have), file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')          # dmabuf IPC: RCCL across processes needs it on this pool
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--points', type=int, default=257 * 145)
    ap.add_argument('--leads', type=int, default=1, help='field samples per step (BASELINE configs[2]: 61); default 1 = configs[1]')
    ap.add_argument('--prec', default=os.environ.get('DPN_PREC', 'bf16x2'), choices=['bf16', 'bf16x2'],
                    help='bf16x2 (default): the parity-grade mode (PDE losses within 1e-4 of the fp32 reference); bf16: plain bf16 operands')
    ap.add_argument('--no-graph', action='store_true', help='do not capture the step in a hipGraph')
    ap.add_argument('--full', action='store_true', help='the long run: the headline timed as the median of --blocks blocks, then the rooflines, power samples, '
                                                        'the other precision mode, the configs[2] legs, the PDE losses and the CPU baseline (off: the headline only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last of them computed as DIR/<name>.npy (float32): loss, grad_norm, grad.<parameter>, '
                         'param.<parameter> (updated); a plain run gives the same inputs to that step on every run')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--cpu-sample', type=int, default=0, help='points of the CPU baseline sample (0 = the workload itself: all --points)')
    ap.add_argument('--cpu-threads', type=int, default=0, help='threads for the CPU baseline (0 = min(32, cores))')
    ap.add_argument('--no-alt', action='store_true', help='with --full: skip the short run of the other precision mode')
    ap.add_argument('--no-power', action='store_true', help='with --full: skip the rocm-smi clock / socket power samples (about 5 s)')
    ap.add_argument('--blocks', type=int, default=10, help='with --full: timed blocks of --steps replays each; ms_per_step is the median block')
    ap.add_argument('--no-prewarm', action='store_true', help='skip the untimed replays that bring the clock to a steady state (their number depends on timing: '
                                                              'a --full run that must do a fixed number of optimiser steps -- tests comparing two runs -- switches them off)')
    ap.add_argument('--no-lead-probe', action='store_true', help='with --full: skip the configs[2] legs: the full-size 61-lead batch (scaled and default initialisation, '
                                                                 '15 steps each) and the 8-lead probe (about 6 s of GPU work in all)')
    ap.add_argument('--init', default=None, choices=['default', 'scaled'],
                    help='weight initialisation: default = PyTorch\'s (what configs[1] is measured on since round 1), scaled = ~1/sqrt(fan_in) uniform '
                         '(deepphysinet_amd/utils/init.py: raw outputs O(1), inside the clip bounds).  Unset: default for one field, scaled for --leads > 1 '
                         '(61 random fields on default-initialised weights run into the reference formula\'s NaN within tens of steps)')
    ap.add_argument('--encoder-fp8', nargs='?', const='mx', default=None, choices=['mx', '1'],
                    help='BASELINE configs[4]: the encoder layers\' forward GEMMs on fp8 (OCP e4m3) MFMA, bf16x2 Jacobian path; OFF by default -- it moves '
                         'the PDE losses by 1e-2 ... 2e-1 (tests/test_gpu_parity.py::test_config4_fp8_encoder_workload) and buys no time.  '
                         'mx (the default form): block-scaled v_mfma_scale_f32_32x32x64_f8f6f4, one E8M0 scale per 32 k; "1": the shelved non-scaled form with '
                         'per-row scales (needs the experiment library: python -m deepphysinet_amd.build --experiments)')
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit('--gpus must be >= 1')
    env_world = os.environ.get('WORLD_SIZE')
    if env_world is None and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit('bench.py --gpus %d was started with WORLD_SIZE=%s: the launcher and the flag disagree' % (args.gpus, env_world))

    if args.encoder_fp8:
        os.environ['DPN_ENCODER_FP8'] = args.encoder_fp8      # read by deepphysinet_amd.encoder_ops at call time
    from deepphysinet_amd import distributed as D
    # DPN_BENCH_BACKEND=gloo + DPN_BENCH_ONE_DEVICE=1: exercise the N > 1 code path with every rank on GPU 0 (test boxes have one GPU)
    # DPN_BENCH_RCCL_ONE_RANK=1: a one-rank RCCL group + the N > 1 step shape (segment graphs, bucket all-reduces): the real collective
    # calls, their interplay with hipGraph capture and replay, on a single-GPU box
    one_rank_rccl = os.environ.get('DPN_BENCH_RCCL_ONE_RANK') == '1' and args.gpus == 1
    rank, world, local = D.init_from_env(os.environ.get('DPN_BENCH_BACKEND'), force=one_rank_rccl)
    if os.environ.get('DPN_BENCH_ONE_DEVICE') == '1':
        local = 0
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (no CPU fallback for the point path)')
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)

    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models

    weights_init = ['default']                    # 'default': PyTorch's initialisation (configs[1], rounds 1-5); 'scaled': deepphysinet_amd.utils.init (lead batches)

    def build(prec):
        torch.manual_seed(1)                      # identical random-init weights on every rank
        m = builder_models(**ncep_config(), precision=prec)
        if weights_init[0] == 'scaled':
            from deepphysinet_amd.utils.init import scaled_init_
            scaled_init_(m.physics_net, seed=1)    # raw outputs O(1): every physical value starts inside its clip bounds (the module's header says why)
        m = m.to(dev)
        # clip_grad_norm_(2.5e7) + Adam(lr 1e-4, weight_decay 1e-4), cfg:151-155; flat gradient buffer in backward-completion order
        opt = m.build_optimizer(max_norm=2.5e7)
        return m, opt

    batch = synth_batch(args.points, dev, seed=1 + rank)
    lead_batches = {}

    def make_leads(n_leads, shift=0):              # configs[2]: distinct field samples / lead times, one step
        many = [synth_batch(args.points, dev, seed=1000 * (1 + rank) + b + 100000 * shift) for b in range(n_leads)]
        lb = {k: torch.stack([m_[k].reshape(-1) for m_ in many]) for k in ('x', 'y', 't', 'f')}
        lb['coord_data'] = torch.stack([m_['coord_data'] for m_ in many])
        lb['field_data'] = torch.cat([m_['field_data'] for m_ in many], dim=0)
        lb['forecast_h'] = torch.arange(n_leads, device=dev, dtype=torch.float32).mul_(24.0 / 360.0).view(-1, 1, 1)
        lead_batches[n_leads] = lb
        return lb
    lead = make_leads(args.leads) if args.leads > 1 else None
    crit = torch.nn.MSELoss()
    step_loss = [None]                             # the loss of the last step run through make_step's one-graph form
    # N > 1 (or DPN_BENCH_SPLIT_STEP=1 on one GPU, to time the same code path): three graph segments with a bucket all-reduce behind each
    split_step = world > 1 or one_rank_rccl or os.environ.get('DPN_BENCH_SPLIT_STEP') == '1'
    # DPN_BENCH_CAPTURE_COLLECTIVES=1: capture the bucket all-reduces inside ONE graph with the segments (opt-in: measured with a one-rank
    # RCCL group on the single-GPU test box, profiles/; the default keeps the collectives host-issued between the segment graphs)
    one_graph_collectives = os.environ.get('DPN_BENCH_CAPTURE_COLLECTIVES') == '1' and split_step and (world > 1 or one_rank_rccl)

    def make_step(m, opt, n_leads):
        """One GPU: [whole] = zero_grad + place_one_batch + backward + clip + Adam, one callable (one hipGraph).
        N > 1: the StagedPdeStep segments (each its own hipGraph) with the bucket all-reduce queued behind each, then the optimiser."""
        lf = m.train_cfg['losses']['loss_factor']
        one = torch.ones((), dtype=torch.float32, device=dev)

        def whole():
            opt.zero_grad(set_to_none=True)
            if n_leads > 1:
                lb = lead_batches[n_leads]
                loss, _ = m.place_lead_batch(lb['x'], lb['y'], lb['t'], lb['f'], lb['field_data'], lb['coord_data'],
                                             lb['forecast_h'], crit, lf)
            else:
                loss = m.place_one_batch(batch['x'], batch['y'], batch['t'], batch['f'], batch['field_data'], batch['coord_data'],
                                         batch['forecast_h'], crit, lf, 0, 0, dev)
            loss.backward(one)                         # persistent seed: no ones_like fill per step
            opt.step()                                 # global-norm clip (2.5e7) + Adam in the HIP library
            step_loss[0] = loss.detach()               # (captured: the graph's output, which every replay rewrites; detached, so that no
                                                       # autograd graph of an earlier step stays alive into the capture)
            return loss

        if not split_step:
            return [whole], None
        from deepphysinet_amd.interface.interface_physics import StagedPdeStep
        staged = StagedPdeStep(m, opt, lead_batches[n_leads] if n_leads > 1 else batch, lf, lead_batch=n_leads > 1)
        return list(staged.stages) + [opt.step], staged

    def run(prec, steps, warmup, use_graph, leads=None, blocks=None, steady=None, plain=False):
        """Build model + optimiser, capture the step, measure.  plain: `warmup` replays, the pre-warm of 2., the state from right after the capture
        restored, then ONE timed block of `steps` replays.  Otherwise (--full and its extra legs) the protocol of VERDICT r4 item 3:
          1. `first_block`: `warmup` untimed steps, then `steps` timed ones, straight after the capture -- what rounds 1-4 reported.  The GPU has
             been idle through the capture; its clock ramps over the first tens of milliseconds, so a 20-step block is taken ON
             the ramp.
          2. pre-warm: the captured step replayed untimed until at least 0.5 s have passed AND two consecutive 20-replay blocks agree within 1 %
             (at most 4 s): `prewarm_s`, `prewarm_replays`.
          3. `blocks` timed blocks of `steps` replays each, every block bracketed by barrier + synchronize; per block the MAX over ranks;
             `ms_per_step` = the median block / steps.
        Returns a dict."""
        nonlocal sync
        n_leads = args.leads if leads is None else leads
        blocks = args.blocks if blocks is None else blocks
        steady = (not args.no_prewarm) if steady is None else steady
        m, opt = build(prec)
        if world > 1:
            D.broadcast_parameters(m.physics_net)      # DDP's wrap-time broadcast (the seeds already agree; this makes it a fact)
        sync = D.GradientAllReduce(opt, single_rank_too=one_rank_rccl) if (world > 1 or one_rank_rccl) else None
        if dog is not None:
            dog.sync = sync
            dog.beat('model built')
        coll['gradient_buckets_mb'] = [round((b - a) * 4 / 2 ** 20, 2) for a, b in opt.bucket_bounds]
        segments, staged = make_step(m, opt, n_leads)
        n_reduce = len(segments) - 1 if split_step else 0     # segment i completes the layout buckets staged.stage_buckets[i]; the last segment is the optimiser
        rec = {'capture_error': None, 'step_form': None, 'n_segments': len(segments)}

        def eager():
            for i, seg in enumerate(segments):
                seg()
                if sync is not None and i < n_reduce:
                    sync.reduce_bucket(*staged.stage_buckets[i])
                    if i == n_reduce - 1:
                        sync.wait()

        def capture_one_graph():
            # the whole step INCLUDING its bucket all-reduces as one hipGraph (RCCL kernels are capturable; ProcessGroupNCCL forks its
            # communication stream off the capture stream, so each all-reduce becomes a parallel branch behind its segment and joins in
            # front of the optimiser): one replay per step instead of four replays + three host-issued collectives
            D.quiesce_for_capture()           # the process group's watchdog must have reaped every eager collective before its stream is captured
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                for i, seg in enumerate(segments):
                    seg()
                    if i < n_reduce:
                        sync.reduce_bucket(*staged.stage_buckets[i])
                        if i == n_reduce - 1:
                            sync.wait()
            return [g]

        def capture_segments():
            graphs, pool = [], None
            for seg in segments:              # one capture stream (torch's default) and one memory pool for all segments:
                g = torch.cuda.CUDAGraph()    # the autograd graph built in segment 0 is walked in segments 1 and 2
                # thread_local: the process group's watchdog thread queries events while we capture
                with torch.cuda.graph(g, pool=pool, capture_error_mode='thread_local' if sync is not None else 'global'):
                    seg()
                pool = g.pool()
                graphs.append(g)
            return graphs

        def replayer(graphs, wait_events=None):
            if len(graphs) == 1:
                return graphs[0].replay

            def fn():
                for i, g in enumerate(graphs):
                    g.replay()
                    if sync is not None and i < n_reduce:
                        sync.reduce_bucket(*staged.stage_buckets[i])         # queued behind segment i, runs under segments i+1..
                        if i == n_reduce - 1:
                            sync.wait(wait_events)    # the optimiser segment waits for every bucket
            return fn

        def all_agree(ok):
            """Every rank must take the same step form (a rank replaying one graph with captured collectives against a rank issuing them from
            the host would deadlock): the AND of the ranks' flags."""
            if world == 1:
                return bool(ok)
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev if torch.distributed.get_backend() == 'nccl' else 'cpu')
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            return bool(int(flag.item()))

        # Lead batches (configs[2]): 61 random fields on default-initialised weights start at losses of 1e13 and the trajectory is chaotic -- after some
        # tens of optimiser steps one field's vapour term is NaN (the reference's own formula is) and every later step would be timed on
        # NaN operands (which run FASTER: constant bit patterns toggle less).  So every block of a lead-batch run starts from the same state (parameters,
        # Adam moments, step counter as they were after the capture), restored OUTSIDE the timed bracket, and is checked to have stayed finite.
        snap = None
        every_block_restored = n_leads > 1         # plain runs of one field restore the snapshot in front of the timed block only
        blocks_finite = []
        local_times = []                           # this rank's own clock per block (block_time returns the MAX over the ranks)

        def take_snapshot():
            return ([p_.detach().clone() for p_ in opt.params], opt._m_flat.clone(), opt._v_flat.clone(), opt.step_count.clone())

        def restore_snapshot():
            with torch.no_grad():
                for p_, s_ in zip(opt.params, snap[0]):
                    p_.copy_(s_)
                opt._m_flat.copy_(snap[1])
                opt._v_flat.copy_(snap[2])
                opt.step_count.copy_(snap[3])

        def block_time(fn, k, restore=False):
            if dog is not None:
                dog.beat('a block of %d steps' % k)
            if snap is not None and (every_block_restored or restore):
                restore_snapshot()
            if world > 1:
                torch.distributed.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            torch.cuda.synchronize()
            if world > 1:
                torch.distributed.barrier()
            dt_ = time.perf_counter() - t0
            local_times.append(dt_)
            if world > 1:
                # every decision taken on a block time (leave the pre-warm loop, stop timing blocks) must be the SAME on all ranks -- a rank that
                # runs one block more than its peers waits in a collective nobody else enters: the MAX over the ranks is what everybody sees
                t_ = torch.tensor([dt_], dtype=torch.float64, device=dev if torch.distributed.get_backend() == 'nccl' else 'cpu')
                torch.distributed.all_reduce(t_, op=torch.distributed.ReduceOp.MAX)
                dt_ = float(t_.item())
            if every_block_restored:
                # (the first moments are enough: a non-finite gradient at any step of the block stays in m = b1 m + (1 - b1) g, and finite moments
                # cannot produce a non-finite parameter -- one reduction instead of one per parameter tensor)
                blocks_finite.append(bool(torch.isfinite(opt._m_flat).all()))
            return dt_

        graphs = None
        if use_graph:
            try:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(2):
                        eager()
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                graphs = capture_one_graph() if one_graph_collectives else capture_segments()
                rec['step_form'] = 'one graph, collectives captured' if one_graph_collectives else ('%d segment graphs, collectives issued from the host' % len(graphs) if split_step else 'one graph')
            except Exception as e:                 # noqa
                rec['capture_error'] = '%s: %s' % (type(e).__name__, str(e)[:400])
                if rank == 0:
                    print('[bench] hipGraph capture failed (%s); running eager' % rec['capture_error'], file=sys.stderr)
                graphs = None
                torch.cuda.synchronize()
                m, opt = build(prec)
                sync = D.GradientAllReduce(opt, single_rank_too=one_rank_rccl) if (world > 1 or one_rank_rccl) else None
                segments, staged = make_step(m, opt, n_leads)
            if world > 1 and not all_agree(graphs is not None):          # one rank failed to capture: everybody runs eager
                graphs = None
                rec['capture_error'] = rec['capture_error'] or 'another rank failed to capture'
                # the rank whose capture failed rebuilt its model from the seed while its peers kept parameters that had taken the two
                # eager steps above -- the ranks would average gradients of different parameters for the rest of the run.  Everybody starts again
                # from rank 0's parameters and a fresh optimiser state, and the stall watchdog follows the gradient synchroniser that is in use.
                torch.cuda.synchronize()
                m, opt = build(prec)
                sync = D.GradientAllReduce(opt, single_rank_too=one_rank_rccl)
                D.broadcast_parameters(m.physics_net)
                segments, staged = make_step(m, opt, n_leads)
                if dog is not None:
                    dog.sync = sync
        fn = eager if graphs is None else replayer(graphs)
        if n_leads > 1 or plain:
            torch.cuda.synchronize()
            snap = take_snapshot()
        # 1. the first block, cold (rounds 1-4's protocol; a plain run times no block here)
        for _ in range(warmup):
            fn()
        if snap is not None:                       # (the warm-up replays belong to no block: the first block starts from the snapshot like every other)
            torch.cuda.synchronize()
        first = None if plain else block_time(fn, steps)
        # 2. pre-warm to a steady clock
        prewarm_s, prewarm_replays = 0.0, 0
        if steady:
            last = None
            pw = min(20, steps) if every_block_restored else 20
            while prewarm_s < 4.0:
                dt_ = block_time(fn, pw) * (20.0 / pw)
                prewarm_s += dt_ * pw / 20.0
                prewarm_replays += pw
                if last is not None and prewarm_s >= 0.5 and abs(dt_ - last) <= 0.01 * last:
                    break
                last = dt_
        # 3. the timed blocks (plain: one, from the snapshot -- its inputs do not depend on how many replays the pre-warm took)
        times = []
        if plain:
            times.append(block_time(fn, steps, restore=True))
        else:
            while len(times) < blocks and (len(times) < min(3, blocks) or sum(times) < 8.0):
                times.append(block_time(fn, steps))
        per_rank = None
        if world > 1 and not plain:                # (first / times are already the MAX over the ranks, block by block)
            own = local_times[-len(times):]        # the timed blocks as this rank's clock saw them
            every = [None] * world
            torch.distributed.all_gather_object(every, sorted(own)[len(own) // 2] / steps * 1e3)
            per_rank = {'ms_per_step': [round(v, 4) for v in every], 'min': min(every), 'max': max(every), 'slowest_rank': int(max(range(world), key=lambda r: every[r])),
                        'fastest_rank': int(min(range(world), key=lambda r: every[r]))}
        med = sorted(times)[len(times) // 2]
        rec.update({'model': m, 'optimizer': opt, 'dt': med, 'graphed': graphs is not None, 'fn': fn, 'first_block_s': first, 'block_s': times,
                    'prewarm_s': prewarm_s, 'prewarm_replays': prewarm_replays, 'per_rank': per_rank, 'staged': staged, 'graphs': graphs,
                    'n_reduce': n_reduce, 'replayer': replayer, 'blocks_finite': blocks_finite if every_block_restored else None,
                    'recapture': (lambda: capture_one_graph() if (split_step and len(graphs) == 1) else capture_segments()) if graphs is not None else None,
                    'capture_one_graph': capture_one_graph, 'block_time': block_time, 'all_agree': all_agree, 'local_times': local_times, 'sync': sync})
        return rec

    def in_step_kernel_times(rec, reps=40):
        """Durations of the three point kernels INSIDE the replayed step: a second capture of the same step with two device-clock stamps (one-thread
        kernels writing wall_clock64, point_path.KernelClock) around each of dpn_fwd / dpn_bwd_points / dpn_wgrad, replayed 10 + `reps` times back to
        back behind the timed region.  (HIP event records inside a capture are dependencies, not timers, and torch refuses external events on ROCm;
        an event pair around an eager launch measures the kernel in another clock / cache state than the step's: it read 370-419 us where rocprofv3
        shows 353 us for the launches of the step.)  The stamp pair's own cost is measured in the same replay and subtracted.  One GPU only."""
        if rec.get('recapture') is None or world > 1 or args.leads != 1:
            return None
        from deepphysinet_amd import point_path as PP
        try:
            PP.clock = PP.KernelClock(dev)
            try:
                probe_graphs = rec['recapture']()
            finally:
                clk, PP.clock = PP.clock, None
            pf = rec['replayer'](probe_graphs)
            for _ in range(10):
                pf()
            torch.cuda.synchronize()
            clk.reset()
            for _ in range(reps):
                pf()
            torch.cuda.synchronize()
            d = clk.durations()
            del probe_graphs
            if not all(k in d for k in ('fwd', 'bwd', 'wgrad')):
                return {'error': 'stamps incomplete: %s' % sorted(d)}
            med = lambda v: sorted(v)[len(v) // 2]
            return {'replays': reps, 'clock_khz': clk.khz,
                    'fwd_us': sum(d['fwd']) / reps, 'bwd_us': sum(d['bwd']) / reps, 'wgrad_us': sum(d['wgrad']) / reps,
                    'fwd_us_median': med(d['fwd']), 'fwd_us_min': min(d['fwd']), 'fwd_us_max': max(d['fwd']),
                    'stamp_pair_us': sum(d['pair']) / reps if 'pair' in d else None}
        except Exception as e:                     # noqa
            PP.clock = None
            torch.cuda.synchronize()
            return {'error': '%s: %s' % (type(e).__name__, str(e)[:300])}

    def collective_info():
        """Who took part: backend, world size, every rank's device (index, PCI bus id, name) gathered over the process group itself, and the
        RCCL version -- so that a scaling record shows N ranks on N distinct GPUs, not N ranks somewhere."""
        pr = torch.cuda.get_device_properties(dev)
        bus = getattr(pr, 'pci_bus_id', None)
        mine = {'rank': rank, 'local_rank': local, 'device_index': dev.index, 'name': pr.name,
                'pci': ('%04x:%02x:%02x' % (getattr(pr, 'pci_domain_id', 0), bus, getattr(pr, 'pci_device_id', 0))) if bus is not None else None,
                'uuid': str(getattr(pr, 'uuid', '')) or None, 'pid': os.getpid()}
        every = [mine]
        backend = None
        if torch.distributed.is_initialized():
            backend = torch.distributed.get_backend()
            every = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(every, mine)
        try:
            ver = '.'.join(str(v) for v in torch.cuda.nccl.version())
        except Exception:                          # noqa
            ver = None
        return {'backend': backend, 'backend_is': 'RCCL (torch backend "nccl" on ROCm)' if backend == 'nccl' else backend, 'world': world,
                'rccl_version': ver, 'devices': every, 'distinct_devices': len({(d['pci'], d['uuid'], d['device_index']) for d in every}),
                'gradient_buckets_mb': None, 'reduce_op': 'AVG in place on the flat gradient buffer, one all-reduce per backward segment',
                'HSA_ENABLE_IPC_MODE_LEGACY': D.ipc_mode()}

    sync = None
    coll = collective_info()
    # N > 1: a rank that stops making progress ends the job with its rank and the bucket it last queued named (exit code 13)
    dog = D.Watchdog(float(os.environ.get('DPN_BENCH_WATCHDOG_S', '300')), rank) if world > 1 else None
    from deepphysinet_amd import config as C
    weights_init[0] = args.init or ('scaled' if args.leads > 1 else 'default')
    rec = run(args.prec, args.steps, args.warmup, not args.no_graph, plain=not args.full)
    # Lead batches: 61 random fields on default-initialised weights is an ill-conditioned start (losses of 4e13, half the points on clip bounds) and within the
    # first few optimiser steps the reference's own vapour formula can produce a NaN at one of the 2.3 M points (q_s = 0.622 e_s / (p - 0.378 e_s) with an
    # exactly cancelling denominator, interface_physics.py:165-185) -- whether it does is a matter of the last bits.  A run whose blocks did
    # not all stay finite is not a measurement (NaN operands run faster): draw the fields again (another seed, the same distribution) and say so.
    lead_attempts = []
    while (args.leads > 1 and world == 1 and rec.get('blocks_finite') is not None and not all(rec['blocks_finite']) and len(lead_attempts) < 4):
        lead_attempts.append({'seed_shift': len(lead_attempts), 'blocks_finite': '%d of %d' % (sum(rec['blocks_finite']), len(rec['blocks_finite']))})
        rec.clear()
        torch.cuda.empty_cache()
        from deepphysinet_amd.encoder_ops import reset_enc_status
        reset_enc_status()                         # (sticky, set by the discarded attempt's non-finite weights)
        lead = make_leads(args.leads, shift=len(lead_attempts))
        rec = run(args.prec, args.steps, args.warmup, not args.no_graph, plain=not args.full)
    if dog is not None:
        dog.stop()                                 # the timed region is over: what follows (rooflines on rank 0, the final barrier) has no collectives in flight
    m, dt, graphed, step_fn = rec['model'], rec['dt'], rec['graphed'], rec['fn']
    if args.dump_outputs and rank == 0:            # NOW, like the PDE losses below: nothing may run the step again in front of it
        dump_outputs(args.dump_outputs, rec['staged'].loss if rec['staged'] is not None else step_loss[0], rec['optimizer'], m.physics_net)
    pde_losses_out = finite_out = None             # evaluated NOW: nothing below may add optimiser steps in front of them
    if rank == 0 and args.leads == 1 and args.full:
        with torch.no_grad():                      # the six scaled PDE-loss scalars of the timed workload (SURVEY 8d asks for them next to the rate)
            terms = m.pde_loss_terms(batch['x'], batch['y'], batch['t'], batch['f'], batch['field_data'], batch['coord_data'], batch['forecast_h'])
        pde_losses_out = dict(zip(('motion_u', 'motion_v', 'continuous', 'energy', 'vapor', 'gas'), [float(v) for v in terms.cpu()]))

    if rank == 0 and args.leads > 1 and args.full:  # configs[2]: the six scalars averaged over the fields, and whether the run stayed finite
        with torch.no_grad():
            _, terms = m.place_lead_batch(lead['x'], lead['y'], lead['t'], lead['f'], lead['field_data'], lead['coord_data'], lead['forecast_h'], crit,
                                          m.train_cfg['losses']['loss_factor'])
        tm = terms.float().mean(dim=0).cpu()
        pde_losses_out = dict(zip(('motion_u', 'motion_v', 'continuous', 'energy', 'vapor', 'gas'), [float(v) for v in tm]))
        finite_out = bool(all(bool(torch.isfinite(p_).all()) for p_ in m.physics_net.parameters()))

    ms_per_step = dt / args.steps * 1e3
    pts_per_s = args.points * args.leads * world * args.steps / dt
    n_segments = len(rec['graphs']) if rec['graphs'] else (rec.get('n_segments', 4) if split_step else 1)

    out = {
        'metric': 'collocation-points/sec (fwd+PDE-Jacobian+bwd)', 'value': pts_per_s, 'unit': 'points/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_per_step, 'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': 'bf16 MFMA operands, fp32 accumulate' if args.prec == 'bf16' else 'bf16x2 (hi+lo split bf16 MFMA operands), fp32 accumulate',
        'data': 'synthetic',
        'config': {'workload': (('configs[1]' if world == 1 else 'configs[3] (configs[1] per GPU, data-parallel over %d GPUs, RCCL bucket all-reduces under the backward)' % world) +
                                ': 0.25deg grid 257x145 = %d collocation points/GPU/step, one field sample per GPU, six PDE residual losses, '
                                'encoder+hyper-net+fwd+Jacobian+bwd+clip+Adam; fixed collocation batch, sampler outside the timed graph' % args.points) if args.leads == 1 else
                               (('configs[2]' if world == 1 else 'configs[3] (configs[2] per GPU, data-parallel over %d GPUs, RCCL bucket all-reduces under the backward)' % world) +
                                ': %d forecast-lead field samples x %d collocation points per GPU per step (one batched encoder pass, '
                                'point kernels field after field), six PDE residual losses, fwd+Jacobian+bwd+clip+Adam; fixed collocation batch, sampler outside the timed graph' % (args.leads, args.points)),
                   'leads': args.leads, 'weights_init': weights_init[0],
                   'collocation_batch': 'one fixed synthetic batch per rank, replayed every step; the on-device sampler (SURVEY 8 f1) is OUTSIDE the timed graph '
                                        '(tools/reference_step.py times it inside)',
                   'points_per_gpu': args.points, 'precision_mode': args.prec, 'hip_graph': graphed, 'parallelism': 'dp%d' % world,
                   'step_segments': n_segments,           # N > 1: two backward segments (lead batches: three) + the optimiser, or one graph with the collectives captured
                   'step_form': rec['step_form'], 'collectives_in_graph': bool(split_step and graphed and n_segments == 1),
                   'graph_branches': list(C.FROZEN.branches)},
        # ms_per_step is the MEDIAN of `timed_blocks` blocks of `steps` replays each (a plain run: one block), taken after the clock has settled
        # (`prewarm_*`); with --full the first block -- `warmup` + `steps` replays straight after the capture, the protocol of rounds 1-4 -- is
        # reported beside it
        'timed_seconds': sum(rec['block_s']), 'timed_blocks': len(rec['block_s']),
        'block_ms_per_step': [round(b_ / args.steps * 1e3, 5) for b_ in rec['block_s']],
        'prewarm_s': round(rec['prewarm_s'], 3), 'prewarm_replays': rec['prewarm_replays'],
        'algorithmic_tflops_step': pts_per_s * ALG_FLOP_STEP / 1e12,
        'collective': coll,
        'switches': C.snapshot(),                   # every DPN_* variable of the environment + the frozen switches that differ from their defaults
    }
    if rec['first_block_s'] is not None:
        out['first_block_ms'] = rec['first_block_s'] / args.steps * 1e3
    if pde_losses_out is not None:
        out['pde_losses'] = pde_losses_out
    if finite_out is not None:
        out['parameters_finite'] = finite_out
    if rec.get('blocks_finite') is not None:
        # lead batches: every block (first, pre-warm, timed) starts from the state after the capture and must end finite; a block that went NaN makes the
        # measurement invalid (NaN operands run faster)
        out['config']['state_restored_before_every_block'] = True
        out['config']['field_seed_shift'] = len(lead_attempts)
        if lead_attempts:
            out['discarded_attempts'] = lead_attempts       # earlier draws of the 61 fields whose trajectory hit the NaN inside a block
        out['blocks_finite'] = all(rec['blocks_finite'])
        if not out['blocks_finite']:
            out['warning'] = 'INVALID: %d of %d blocks ended with non-finite parameters' % (sum(1 for b_ in rec['blocks_finite'] if not b_), len(rec['blocks_finite']))
    if rec['capture_error']:
        out['capture_error'] = rec['capture_error']
    if rec.get('step_form_trial'):
        coll['step_form_trial'] = rec['step_form_trial']
    if rec['per_rank']:
        coll['per_rank'] = rec['per_rank']
    if args.full and sync is not None and rec['graphs'] is not None and len(rec['graphs']) > 1:
        # how long the optimiser segment actually WAITS for each bucket's all-reduce (an event pair around every wait, 20 replays): the part of
        # the collectives that the backward segments did not hide
        evs = []
        probe = rec['replayer'](rec['graphs'], wait_events=evs)
        for _ in range(20):
            probe()
        torch.cuda.synchronize()
        nb = max(1, rec['n_reduce'])
        per = [[] for _ in range(nb)]
        for i, (e0, e1) in enumerate(evs):
            per[i % nb].append(e0.elapsed_time(e1) * 1e3)
        coll['exposed_us'] = [round(sorted(v)[len(v) // 2], 1) if v else None for v in per]
        coll['exposed_us_note'] = 'median over 20 replays of the time the optimiser segment waits for bucket i (HIP events around each wait)'
    if args.encoder_fp8:
        out['config']['encoder_fp8'] = 'mx (E8M0 scale per 32 k, v_mfma_scale_f32_32x32x64_f8f6f4)' if args.encoder_fp8 == 'mx' else 'per-row scales, v_mfma_f32_32x32x16_fp8_fp8'
        out['dtype'] += '; encoder forward GEMMs fp8 e4m3 MFMA (configs[4])'

    def kernel_rooflines(m, prec, in_step=None):
        """`roofline` (dpn_fwd_kernel, MFMA-bound: the dominant kernel) and `roofline_hbm_kernel` (dpn_wgrad_kernel) of the workload in
        precision mode `prec`.  Durations: `in_step` (in_step_kernel_times: device-clock stamps around the launches inside the replayed step graph)
        when it is there; beside it (`kernel_ms_eager_pair`), and alone when the step was not captured, a HIP event pair around every launch inside a
        pre-queued eager replay of the point path."""
        import ctypes
        from deepphysinet_amd import _lib as L
        from deepphysinet_amd import point_path as PP
        cfg = m.point_config()
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(batch['field_data'], batch['forecast_h'])
            x_, y_, t_ = (PP._f32c(batch[k]).reshape(-1) for k in ('x', 'y', 't'))
            cd_ = PP._f32c(batch['coord_data'])
            st = [PP._f32c(s) for s in statics]
            ws = PP._Workspace(args.points, cfg.prec, dev)
            nets = PP._net_ptrs(PP._f32c(heads), PP._f32c(evec), st)
            PP._forward_points(cfg, ws, nets, x_, y_, t_, None, cd_, True, True)       # packs weights, allocates saved
            lib = L.load()
            out_n = torch.empty((args.points, 6), device=dev)
            jac_n = torch.empty((args.points, 6, 3), device=dev)
            geo = cfg.geometry()

            def launch():
                L.check(lib.dpn_fwd(PP._ptr(x_), PP._ptr(y_), PP._ptr(t_), None, PP._ptr(cd_), args.points, PP._ptr(PP._freqs(dev)),
                                    ctypes.byref(geo), PP._ptr(ws.packed), cfg.prec, PP._ptr(out_n), PP._ptr(jac_n), PP._ptr(ws.saved),
                                    PP._stream()), 'dpn_fwd')
            reps = 20
            # ---- the HBM-bound kernel of the path: dpn_wgrad (points-reduction GEMMs; every saved / cotangent operand is read once)
            f_ = PP._f32c(batch['f']).reshape(-1)
            ph = cfg.physics()
            g_out = torch.empty((args.points, 6), device=dev)
            g_jxi = torch.empty((args.points, 6, 3), device=dev)
            operands = torch.empty(ws.sizes.operands, dtype=torch.uint8, device=dev)
            partials = torch.empty(ws.sizes.partials, dtype=torch.uint8, device=dev)
            L.check(lib.dpn_residual(PP._ptr(out_n), PP._ptr(jac_n), PP._ptr(f_), args.points, ctypes.byref(geo), ctypes.byref(ph), None, None, None,
                                     PP._ptr(g_out), PP._ptr(g_jxi), PP._stream()), 'dpn_residual')

            def launch_b():
                L.check(lib.dpn_bwd_points(PP._ptr(x_), PP._ptr(y_), PP._ptr(t_), None, PP._ptr(cd_), args.points, PP._ptr(PP._freqs(dev)),
                                           ctypes.byref(geo), PP._ptr(ws.packed), cfg.prec, PP._ptr(g_out), PP._ptr(g_jxi), PP._ptr(ws.saved),
                                           PP._ptr(operands), PP._stream()), 'dpn_bwd_points')
            launch_b()

            def launch_w():
                L.check(lib.dpn_wgrad(args.points, cfg.prec, PP._ptr(g_out), PP._ptr(ws.saved), PP._ptr(operands), PP._ptr(partials), PP._stream()),
                        'dpn_wgrad')
            # Kernel durations: an event pair around EVERY launch of the kernel, inside a pre-queued replay of the point path
            # (spin -> fwd -> bwd -> wgrad: the order and duty cycle of the step).  The queue is filled ahead of the GPU (the kernels take
            # 150-600 us, a launch costs the host ~10 us), so no interval contains host latency, and the MFMA-heavy kernel is not run
            # back to back in a loop of its own, which holds the chip at its power limit and reads a few % slower than the same kernel
            # does inside the step (rocprofv3 shows both populations, profiles/).
            # the encoder / optimiser part of the step is ~0.6 ms of light kernels: a spin of that length stands in for it (calibrated here)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            torch.cuda._sleep(1000000)
            c1.record()
            torch.cuda.synchronize()
            spin = max(1, int(1000000 * 0.6 / max(c0.elapsed_time(c1), 1e-3)))
            for _ in range(3):
                launch()
                launch_b()
                launch_w()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
            for e0, e1, e2, e3 in ev:
                torch.cuda._sleep(spin)
                e0.record()
                launch()
                e1.record()
                launch_b()
                e2.record()
                launch_w()
                e3.record()
            torch.cuda.synchronize()
            k_ms = sum(e[0].elapsed_time(e[1]) for e in ev) / reps
            b_ms = sum(e[1].elapsed_time(e[2]) for e in ev) / reps
            w_ms = sum(e[2].elapsed_time(e[3]) for e in ev) / reps
            eager_ms = (k_ms, b_ms, w_ms)
            if in_step and 'fwd_us' in in_step:
                k_ms, b_ms, w_ms = in_step['fwd_us'] * 1e-3, in_step['bwd_us'] * 1e-3, in_step['wgrad_us'] * 1e-3
            sustained = None
            if not args.no_power:
                def soak():
                    for _ in range(40):
                        launch()
                sustained = sample_power(soak, 2.5)
        ach = args.points * ALG_FLOP_FWD_JAC / (k_ms * 1e-3)
        ns = 2 if prec == 'bf16x2' else 1
        nsplit = 3 if prec == 'bf16x2' else 1
        traffic, source = pmc_traffic('dpn_fwd_tiles_kernel' if ns == 2 else 'dpn_fwd_kernel', prec, args.points)
        fwd_name = 'dpn_fwd_kernel<1>'
        if ns == 2:
            fwd_name = 'dpn_fwd_tiles_kernel<2>'
        roof = {'bound': 'mfma', 'kernel': fwd_name,
                'achieved': ach / 1e12, 'peak': MFMA_PEAK_BF16 / 1e12, 'unit': 'TFLOP/s', 'frac': ach / MFMA_PEAK_BF16,
                'traffic': traffic, 'traffic_source': source, 'kernel_ms': k_ms,
                'kernel_ms_source': ('device-clock stamps around the launch inside the replayed step graph, mean of %d replays' % in_step['replays'])
                                    if in_step and 'fwd_us' in in_step else 'HIP event pair around each launch, pre-queued eager replay of the point path',
                'kernel_ms_eager_pair': eager_ms[0], 'in_step': in_step,
                'algorithmic_flop_per_point': ALG_FLOP_FWD_JAC,
                'algorithmic_bytes': args.points * 136,          # 40 B in + 96 B out per point: the kernel is MFMA-bound
                'executed_mfma_tflops': args.points * 6 * (EXEC_MAC_FWD if ns == 2 else EXEC_MAC_FWD_RING) * 2 * nsplit / (k_ms * 1e-3) / 1e12,
                'executed_mfma_frac_of_peak': args.points * 6 * (EXEC_MAC_FWD if ns == 2 else EXEC_MAC_FWD_RING) * 2 * nsplit / (k_ms * 1e-3) / MFMA_PEAK_BF16}
        if sustained is not None:
            # the kernel alone, back to back: the clock the socket's power cap leaves it, and the dense peak AT that clock (peak above = 2.4 GHz)
            sustained['peak_at_this_clock_tflops'] = MFMA_PEAK_BF16 / 1e12 * sustained['sclk_mhz'] / 2400.0
            roof['kernel_back_to_back'] = sustained
        # operands of the three products per point per net: M2 (0/1 bf16, one plane: 512 B) + Z1 (512 B x ns), M2 + [pe6 table], T1 (512 B x ns) + Z0
        # (384 B x ns); the pe6 table is per POINT (384 B x ns, shared by the six nets: read from HBM once, then from the memory-side cache).  Neither v
        # (affine in m2), nor Z (linear in Z1, G6, g), nor G6 = g pe6 (formed in registers from the table) is an operand
        w_bytes = ws.sizes.n_pad * 6 * (2 * 512 + (512 + 512 + 384) * ns) + ws.sizes.n_pad * 384 * ns
        roof_hbm = {'bound': 'hbm', 'kernel': 'dpn_wgrad_kernel<%d>' % ns,
                    'achieved': w_bytes / (w_ms * 1e-3) / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                    'frac': w_bytes / (w_ms * 1e-3) / HBM_PEAK, 'kernel_ms': w_ms, 'kernel_ms_eager_pair': eager_ms[2], 'algorithmic_bytes': w_bytes,
                    'traffic': pmc_traffic('dpn_wgrad_kernel', prec, args.points)[0], 'bwd_points_kernel_ms': b_ms}
        # backward stage 1 (dpn_bwd_tiles_kernel / dpn_bwd_kernel): per point and net it writes the K-layout rows of Z1 (256 columns) and Z0 (192 columns),
        # hi (+ lo) bf16, per point the pe6 table (192 columns), and reads 40 B of cotangents
        b_bytes = ws.sizes.n_pad * 6 * (512 + 384) * ns + ws.sizes.n_pad * 384 * ns
        b_traffic = pmc_traffic('dpn_bwd_tiles_kernel' if ns == 2 else 'dpn_bwd_kernel', prec, args.points)[0]
        roof_hbm['bwd_stage1_kernel'] = {'bound': 'hbm', 'kernel': 'dpn_bwd_tiles_kernel<2>' if ns == 2 else 'dpn_bwd_kernel<1>',
                                         'achieved': b_bytes / (b_ms * 1e-3) / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                                         'frac': b_bytes / (b_ms * 1e-3) / HBM_PEAK, 'kernel_ms': b_ms, 'kernel_ms_eager_pair': eager_ms[1],
                                         'algorithmic_bytes': b_bytes, 'traffic': b_traffic,
                                         'executed_mfma_frac_of_peak': args.points * 6 * EXEC_MAC_BWD1 * 2 * nsplit / (b_ms * 1e-3) / MFMA_PEAK_BF16}
        return roof, roof_hbm

    if rank == 0 and args.full:
        out['roofline'], out['roofline_hbm_kernel'] = kernel_rooflines(m, args.prec, in_step_kernel_times(rec))
        out['roofline']['step_frac_of_peak'] = pts_per_s / world * ALG_FLOP_STEP / MFMA_PEAK_BF16
        if not args.no_power and world == 1:
            def steps_():
                for _ in range(25):
                    step_fn()
            out['power'] = sample_power(steps_, 2.0)          # the whole step replayed back to back (after the timed region)
        if not args.no_alt and world == 1:
            alt = 'bf16x2' if args.prec == 'bf16' else 'bf16'
            del m, step_fn
            rec.clear()
            torch.cuda.empty_cache()
            st2 = max(5, args.steps // 3)
            rec2 = run(alt, st2, 3, not args.no_graph, blocks=3)
            m2, dt2 = rec2['model'], rec2['dt']
            out['other_precision_mode'] = {'mode': alt, 'value': args.points * args.leads * st2 / dt2, 'ms_per_step': dt2 / st2 * 1e3,
                                           'parity': 'PDE losses within 1e-4 of the fp32 reference' if alt == 'bf16x2' else
                                                     'plain bf16 operands: PDE losses within 5e-2 (measured 1e-3 ... 2e-2), not the parity-grade mode'}
            if args.leads == 1:
                r2, _ = kernel_rooflines(m2, alt, in_step_kernel_times(rec2))
                out['other_precision_mode']['roofline'] = {k: r2[k] for k in ('kernel', 'frac', 'kernel_ms', 'achieved', 'executed_mfma_frac_of_peak')}
            del m2
            rec2.clear()
        if not args.no_lead_probe and world == 1 and args.leads == 1:
            # BASELINE configs[2] at FULL size in the driver's line: 61 forecast-lead field samples x the same points in ONE captured step,
            # 3 blocks of 5 replays, every block from the state after the capture; field seed shift 0, no redraw.  `scaled` initialisation (utils/init.py) is
            # the measurement; the default-initialised variant (what `--leads 61` measured in rounds 3-5 after redraws) runs beside it and says whether it
            # stayed finite.
            rec.clear()
            torch.cuda.empty_cache()
            from deepphysinet_amd.encoder_ops import check_enc_status as _ces
            try:                                   # the status words are sticky and the legs below reset them: the headline run's verdict is taken first
                _ces()
            except RuntimeError as e:
                out['encoder_weights_in_range'] = False
                out['warning'] = (out.get('warning', '') + ' ' + str(e)).strip()
            full = {}
            for init_ in ('scaled', 'default'):
                keep_init, weights_init[0] = weights_init[0], init_
                try:
                    nlf = 61
                    make_leads(nlf)
                    recf = run(args.prec, 5, 2, not args.no_graph, leads=nlf, blocks=3, steady=False)
                    mf, dtf = recf['model'], recf['dt']
                    vf = args.points * nlf * 5 / dtf
                    full[init_] = {'leads': nlf, 'points_per_step': args.points * nlf, 'ms_per_step': dtf / 5 * 1e3, 'value': vf, 'unit': 'points/s', 'steps': 5,
                                   'blocks': len(recf['block_s']), 'block_ms_per_step': [round(b_ / 5 * 1e3, 3) for b_ in recf['block_s']], 'hip_graph': recf['graphed'],
                                   'weights_init': init_, 'field_seed_shift': 0, 'discarded_attempts': [],
                                   'blocks_finite': all(recf['blocks_finite']) if recf.get('blocks_finite') else None,
                                   'parameters_finite': bool(all(bool(torch.isfinite(p_).all()) for p_ in mf.physics_net.parameters())),
                                   'step_frac_of_peak': vf * ALG_FLOP_STEP / MFMA_PEAK_BF16}
                    if recf['capture_error']:
                        full[init_]['capture_error'] = recf['capture_error']
                    del mf
                    recf.clear()
                except Exception as e:             # noqa  (the legs beside the headline must never take the line down)
                    full[init_] = {'error': '%s: %s' % (type(e).__name__, str(e)[:300])}
                    torch.cuda.synchronize()
                finally:
                    weights_init[0] = keep_init
                    lead_batches.pop(61, None)
                    torch.cuda.empty_cache()
                    from deepphysinet_amd.encoder_ops import reset_enc_status
                    reset_enc_status()             # (sticky: a default-initialised lead batch that went non-finite must not mark the headline run)
            out['lead_batch_full'] = dict(full.get('scaled', {}), default_init_variant=full.get('default'),
                                          note='BASELINE configs[2]: 61 leads x %d points in one captured step; `bench.py --leads 61` is the long form of the same run' % args.points)
            # the same code path at 8 leads, kept for continuity with round 5's line
            nl = 8
            make_leads(nl)
            rec3 = run(args.prec, 3, 1, not args.no_graph, leads=nl, blocks=3, steady=False)
            m3, dt3 = rec3['model'], rec3['dt']
            v3 = args.points * nl * 3 / dt3
            out['lead_batch_probe'] = {'leads': nl, 'points_per_step': args.points * nl, 'ms_per_step': dt3 / 3 * 1e3, 'value': v3, 'unit': 'points/s',
                                       'steps': 3, 'blocks': len(rec3['block_s']), 'hip_graph': rec3['graphed'],
                                       'parameters_finite': bool(all(bool(torch.isfinite(p_).all()) for p_ in m3.physics_net.parameters())),
                                       'blocks_finite': all(rec3['blocks_finite']) if rec3.get('blocks_finite') else None,
                                       'step_frac_of_peak': v3 * ALG_FLOP_STEP / MFMA_PEAK_BF16,
                                       'note': 'configs[2] itself (61 leads) is `bench.py --leads 61`; this probe is the same code path at 8 leads'}
            if rec3['capture_error']:
                out['lead_batch_probe']['capture_error'] = rec3['capture_error']
            del m3
            rec3.clear()
            lead_batches.pop(nl, None)
        if not args.no_cpu_baseline and world == 1:
            torch.set_num_threads(args.cpu_threads or min(32, os.cpu_count() or 1))   # more threads only add OpenMP overhead on these small ops
            cpu_model = None
            try:
                with open('/proc/cpuinfo') as fh:
                    cpu_model = next((ln.split(':', 1)[1].strip() for ln in fh if ln.startswith('model name')), None)
            except OSError:
                pass
            n_cpu = args.cpu_sample or args.points                # default: the identical step, all points of the workload
            v, secs = cpu_baseline(n_cpu, seed=1)
            v2, secs2 = cpu_baseline(n_cpu, seed=1, share_derivatives=True)
            out['cpu_baseline'] = {'value': v, 'unit': 'points/s', 'cores': torch.get_num_threads(), 'kind': 'port',
                                   'sample': 'oracle place_one_batch + backward (fp32, 28 autograd.grad calls) on %d of the %d points of the same '
                                             'synthetic field (%s); best of 3 after 1 warm-up, %.1f s per pass; host: %s, %d logical cores, %d threads used'
                                             % (n_cpu, args.points, 'the identical step' if n_cpu == args.points else 'a bounded sample', secs, cpu_model,
                                                os.cpu_count() or 0, torch.get_num_threads()),
                                   'host_cpu': cpu_model, 'host_logical_cores': os.cpu_count(),
                                   'shared_jacobian_variant': {'value': v2, 'seconds_per_pass': secs2,
                                                               'note': 'same oracle, the 18 distinct derivatives taken once (SURVEY 8d variant ii)'}}
    if rank == 0:
        from deepphysinet_amd.encoder_ops import check_enc_status
        try:
            check_enc_status()                     # an encoder weight left the range of the f16 hi+lo operand split during the run (or went non-finite)?
            out['encoder_weights_in_range'] = out.get('encoder_weights_in_range', True)
        except RuntimeError as e:
            out['encoder_weights_in_range'] = False
            out['warning'] = (out.get('warning', '') + ' ' + str(e)).strip()

    # ---- N > 1 over RCCL: "segment graphs + host-issued collectives" (measured above: the form that needs nothing of RCCL but ordinary stream-ordered
    # collectives) against "ONE graph with the collectives captured" (the two swap places from box to box on a one-rank group and
    # nobody has timed them on xGMI).  Tried LAST, with the finished line of the segment form in hand: a capture error keeps the segment form; a STALL of
    # the captured collectives (RCCL kernels replayed from a graph across N processes have never run here) makes every rank's watchdog print what it
    # has -- rank 0 the finished line, `step_form_trial.error` saying where it stalled -- and end the process with exit code 14 (TRIAL_STALL_EXIT: non-zero, so that
    # torchrun and the driver see a wedged collective; the printed line is the valid segment-form measurement).  If the one-graph form is
    # more than 1 % faster over 20 replays, the ten blocks are timed again in it and the line reports it (the segment form's numbers stay in
    # `collective.step_form_trial`).  DPN_BENCH_CAPTURE_COLLECTIVES=0/1 pins the form.  OPT-IN (DPN_BENCH_TRY_FORMS=1) since the end of round 5: a capture that
    # contains collectives can take the whole process down from ProcessGroupNCCL's watchdog thread (distributed.quiesce_for_capture: found, reproduced and
    # worked around here), and nothing of that kind may stand between an 8-GPU run and its line.
    stash = {'line': None, 'printed': False, 'lock': threading.Lock()}
    tdog = None
    want_trial = (args.full and rec.get('graphed') and split_step and not one_graph_collectives and os.environ.get('DPN_BENCH_CAPTURE_COLLECTIVES') is None
                  and rec.get('sync') is not None and torch.distributed.get_backend() == 'nccl' and rec.get('graphs') is not None and len(rec['graphs']) > 1
                  and os.environ.get('DPN_BENCH_TRY_FORMS', '0') == '1')
    if os.environ.get('DPN_BENCH_TRY_FORMS', '0') == '1' and not want_trial and rank == 0:
        # asked for and not run must be visible in the line (the default single-rank flow has released the measured step for the other-precision
        # and lead-batch runs by now: pass --no-alt --no-lead-probe with DPN_BENCH_RCCL_ONE_RANK=1)
        coll['step_form_trial'] = {'skipped': 'the measured step is no longer held (--no-alt --no-lead-probe keep it) or it was not a captured multi-segment RCCL step'
                                   if args.full else 'the trial runs with --full only'}
    if want_trial:
        trial = {'segments_ms': None, 'one_graph_ms': None, 'error': None, 'segment_form_result': None}
        phase = ['start']
        torch.distributed.barrier()                # rank 0 comes from the roofline measurements: the trial's clock starts when everybody is here
        if rank == 0:
            trial['error'] = 'stalled'             # what the stashed line says if it is ever printed
            coll['step_form_trial'] = trial
            stash['line'] = json.dumps(out)
            trial['error'] = None

        def on_stall(msg):
            with stash['lock']:                    # the main thread prints under the same lock: exactly one line leaves the process
                if rank == 0 and not stash['printed']:
                    line = json.loads(stash['line'])
                    line['collective']['step_form_trial']['error'] = 'stalled in: %s -- the segment form\'s line is reported (exit code %d)' % (phase[0], TRIAL_STALL_EXIT)
                    print(json.dumps(line), flush=True)
                    stash['printed'] = True
            print('[bench] rank %d: the one-graph trial stalled (%s); the segment form\'s result stands' % (rank, phase[0]), file=sys.stderr, flush=True)
            os._exit(TRIAL_STALL_EXIT)             # NON-ZERO: a launcher must be able to tell a wedged collective from a clean run; the line printed above is still the valid segment-form measurement
        tdog = D.Watchdog(float(os.environ.get('DPN_BENCH_TRIAL_WATCHDOG_S', '90')), rank, sync=rec['sync'], on_stall=on_stall)
        fn_seg, block_time, all_agree = rec['fn'], rec['block_time'], rec['all_agree']
        one = None
        try:
            phase[0] = 'capture of the step with its all-reduces'
            tdog.beat(phase[0])
            if os.environ.get('DPN_BENCH_TRIAL_TEST_STALL') == 'capture':
                time.sleep(1e6)
            one = rec['capture_one_graph']()
        except Exception as e:                     # noqa
            trial['error'] = '%s: %s' % (type(e).__name__, str(e)[:300])
            torch.cuda.synchronize()
        phase[0] = 'agreement of the ranks on the capture'
        tdog.beat(phase[0])
        if all_agree(one is not None):
            f2 = rec['replayer'](one)
            phase[0] = 'first replays of the one-graph form'
            tdog.beat(phase[0])
            if os.environ.get('DPN_BENCH_TRIAL_TEST_STALL') == 'replay':
                time.sleep(1e6)
            for f_ in (fn_seg, f2):
                for _ in range(5):
                    f_()
            torch.cuda.synchronize()
            phase[0] = 'timing 20 replays of each form'
            tdog.beat(phase[0])
            t_seg, t_one = block_time(fn_seg, 20), block_time(f2, 20)
            trial['segments_ms'], trial['one_graph_ms'] = t_seg / 20 * 1e3, t_one / 20 * 1e3
            if t_one < 0.99 * t_seg:
                phase[0] = 'timing the blocks in the one-graph form'
                n0 = len(rec['local_times'])
                times2 = []
                for _ in range(max(1, len(rec['block_s']))):
                    tdog.beat(phase[0])
                    times2.append(block_time(f2, args.steps))
                med2 = sorted(times2)[len(times2) // 2]
                own = rec['local_times'][n0:]
                every = [None] * world
                torch.distributed.all_gather_object(every, sorted(own)[len(own) // 2] / args.steps * 1e3)
                if rank == 0:
                    trial['segment_form_result'] = {'ms_per_step': out['ms_per_step'], 'value': out['value'], 'block_ms_per_step': out['block_ms_per_step']}
                    scale = (dt / args.steps) / (med2 / args.steps)
                    out['ms_per_step'] = med2 / args.steps * 1e3
                    out['value'] = args.points * args.leads * world * args.steps / med2
                    out['timed_seconds'], out['timed_blocks'] = sum(times2), len(times2)
                    out['block_ms_per_step'] = [round(b_ / args.steps * 1e3, 5) for b_ in times2]
                    out['algorithmic_tflops_step'] = out['value'] * ALG_FLOP_STEP / 1e12
                    out['roofline']['step_frac_of_peak'] *= scale
                    out['config'].update(step_form='one graph, collectives captured (chosen by the trial at the end of the run)', step_segments=1, collectives_in_graph=True)
                    coll['per_rank'] = {'ms_per_step': [round(v, 4) for v in every], 'min': min(every), 'max': max(every),
                                        'slowest_rank': int(max(range(world), key=lambda r: every[r])), 'fastest_rank': int(min(range(world), key=lambda r: every[r]))}
                    coll.pop('exposed_us', None)
                    coll.pop('exposed_us_note', None)
            elif rank == 0:
                out['config']['step_form'] += ' (kept by the trial at the end of the run)'
        elif trial['error'] is None:
            trial['error'] = 'another rank failed to capture the collectives'
        phase[0] = 'the final barrier'
        tdog.beat(phase[0])
    if rank == 0:
        with stash['lock']:
            if not stash['printed']:
                print(json.dumps(out), flush=True)
                stash['printed'] = True
        if not out['encoder_weights_in_range'] and args.leads == 1:
            raise SystemExit('bench.py: ' + out['warning'])          # the line above is printed for the record; the run is not a measurement
    if world > 1 or one_rank_rccl:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if tdog is not None:
        tdog.stop()


if __name__ == '__main__':
    main()
