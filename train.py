#!/usr/bin/env python
"""Launcher with the reference's three flags (reference train.py:17-19, :34-48): --config_file, --checkpoint_path, --log_path.

    python train.py [--config_file cfg.py] [--checkpoint_path DIR] [--log_path DIR] [--dist] [--max_steps N] [--synthetic] [--valid_synthetic]
                    [--adaptive_interior] [--causal_weights EPS] [--balance_losses EVERY] [--lead_batch K] [--ema DECAY]
                    [--skip_nonfinite] [--spike_factor F [--spike_warmup N] [--spike_patience N]]
                    [--freeze PATTERN]... [--param_group 'PATTERN[,PATTERN...]:lr=...,weight_decay=...']...
                    [--lbfgs_from EPOCH [--lbfgs_history M] [--lbfgs_iters N]]

The reference reads the config with mmcv.Config.fromfile (absent here, and moved to mmengine in the pinned mmcv: SURVEY section 0, defect
3), builds the interface with `builder_models(**cfg['config'])` and calls `run_train_interface(checkpoint_path=..., log_path=...)`.  The
same happens here: a python config file that defines `config = dict(...)` is exec'd (the format of configs/DeepPhysiNet_NCEP_cfg.py);
without --config_file the built-in copy of that config (deepphysinet_amd.configs.ncep_config) is used.  The reference's PhysicsDataset
reads GeoTIFF / xarray files that do not exist offline (out of scope); a config that names no `samples`
source therefore FAILS like the reference without its files, unless --synthetic asks for random field samples and batches from the
on-device CollocationSampler (smoke runs: the checkpoints are trained on noise).  --dist selects run_train_interface_dist (torchrun).
Fine-tuning: --checkpoint_path naming an existing checkpoint, with --freeze / --param_group (fnmatch patterns on state-dict names)."""
import argparse
import os
import runpy
import shutil

import torch

from deepphysinet_amd.configs import ncep_config
from deepphysinet_amd.interface import builder_models

parse = argparse.ArgumentParser()
parse.add_argument('--config_file', default=None, type=str)
parse.add_argument('--checkpoint_path', default=None, type=str)
parse.add_argument('--log_path', default=None, type=str)
parse.add_argument('--dist', action='store_true', help='data-parallel loop (run_train_interface_dist); start with torchrun')
parse.add_argument('--max_steps', default=None, type=int)
parse.add_argument('--synthetic', action='store_true', help="samples='synthetic': random field samples and on-device collocation batches "
                   '(the reference dataset is file I/O that does not exist offline); without it a config with no `samples` source fails, '
                   'as the reference does without its data files')
parse.add_argument('--valid_synthetic', action='store_true', help="valid_samples='synthetic': a validation source of random field samples drawn from "
                   'another seed than --synthetic; at every log step the loop then evaluates one of them and writes the training / validation lines '
                   'to log_<date>.txt and metrics.jsonl under --log_path')
parse.add_argument('--adaptive_interior', action='store_true', help='once the PDE losses are on, redraw every step\'s interior collocation points where '
                   'the residuals are large (adaptive_interior=dict(pool_factor=8, k=1, c=1, every=1)); the sampler is the samples source\'s own '
                   '(--synthetic has one)')
parse.add_argument('--causal_weights', default=None, type=float, metavar='EPS', help='once the PDE losses are on, weight every step\'s PDE losses by causal '
                   'time weights W_k = exp(-EPS * sum of the earlier time bins\' losses, relative to their mean) (causal_weights=dict(eps=EPS, bins=16, '
                   'relative=True)); validation stays unweighted')
parse.add_argument('--balance_losses', default=None, type=int, metavar='EVERY', help='once the PDE losses are on, weight the data loss and the six equations '
                   'by weights balanced by the norms of their parameter gradients, refreshed on every EVERY-th step (balance_losses=dict(every=EVERY, '
                   'momentum=0.9, groups=\'equations\')); validation stays unweighted')
parse.add_argument('--lead_batch', default=None, type=int, metavar='K', help='K consecutive samples of the epoch (for example forecast leads) per optimiser '
                   'step: one batched encoder pass, the point kernels sample after sample, the loss their mean (lead_batch=K; 1 or unset: one sample '
                   'per step); not together with --causal_weights / --balance_losses')
parse.add_argument('--ema', default=None, type=float, metavar='DECAY', help='keep an exponential moving average of the weights inside the optimiser step '
                   '(ema_weights=dict(decay=DECAY, warmup=True)): validation runs on it and the checkpoints carry it as model_ema (infer.py --ema)')
parse.add_argument('--skip_nonfinite', action='store_true', help='skip, on the device, every optimiser step whose total gradient norm is NaN or +-inf: '
                   'parameters, moments and the weight EMA stay bit for bit as they were (step_guard=True)')
parse.add_argument('--spike_factor', default=None, type=float, metavar='F', help='also skip a step whose gradient norm exceeds F times the running mean of '
                   'the applied steps\' norms (step_guard=dict(spike_factor=F, ...); implies --skip_nonfinite)')
parse.add_argument('--spike_warmup', default=None, type=int, metavar='N', help='applied steps before the spike rule starts (default 100)')
parse.add_argument('--spike_patience', default=None, type=int, metavar='N', help='spikes in a row after which the guard is overruled and the running mean '
                   'starts again (default 5)')


def step_guard_arg(args):
    """The `step_guard` option of the loops from the four flags: None, True, or a dict of the spike settings."""
    if args.spike_factor is None:
        if args.spike_warmup is not None or args.spike_patience is not None:
            raise SystemExit('--spike_warmup / --spike_patience need --spike_factor')
        return True if args.skip_nonfinite else None
    opt = dict(spike_factor=args.spike_factor)
    if args.spike_warmup is not None:
        opt['spike_warmup'] = args.spike_warmup
    if args.spike_patience is not None:
        opt['spike_patience'] = args.spike_patience
    return opt


parse.add_argument('--lbfgs_from', default=None, type=int, metavar='EPOCH', help='from this epoch on the loop drops Adam and refines with L-BFGS and a '
                   'strong-Wolfe line search on the flat buffers, one FusedLBFGS.step per loop step (lbfgs=dict(start_epoch=EPOCH, ...)); not together '
                   'with --adaptive_interior, --causal_weights, --balance_losses, --ema, --skip_nonfinite / --spike_factor or --dist')
parse.add_argument('--lbfgs_history', default=None, type=int, metavar='M', help='curvature pairs kept, 1 .. 32 (default 10)')
parse.add_argument('--lbfgs_iters', default=None, type=int, metavar='N', help='L-BFGS iterations per loop step (default 20)')


def lbfgs_arg(args):
    """The `lbfgs` option of the loops from the three flags: None, or dict(start_epoch, [history_size], [max_iter])."""
    if args.lbfgs_from is None:
        if args.lbfgs_history is not None or args.lbfgs_iters is not None:
            raise SystemExit('--lbfgs_history / --lbfgs_iters need --lbfgs_from')
        return None
    opt = dict(start_epoch=args.lbfgs_from)
    if args.lbfgs_history is not None:
        opt['history_size'] = args.lbfgs_history
    if args.lbfgs_iters is not None:
        opt['max_iter'] = args.lbfgs_iters
    return opt


def param_group_arg(text):
    """'PATTERN[,PATTERN...]:key=value[,key=value...]' -> dict(match=[patterns], key=value, ...) for the `param_groups` option.  Keys: lr, eps,
    weight_decay (a number each) and betas (two numbers joined by '/': betas=0.9/0.999)."""
    pats, sep, rest = text.partition(':')
    match = [p for p in (q.strip() for q in pats.split(',')) if p]
    if not sep or not match:
        raise argparse.ArgumentTypeError("expected 'PATTERN[,PATTERN...]:key=value[,key=value...]', got %r" % text)
    group = dict(match=match)
    for item in (q.strip() for q in rest.split(',')):
        if not item:
            continue
        key, eq, val = item.partition('=')
        key = key.strip()
        try:
            if key not in ('lr', 'eps', 'weight_decay', 'betas') or not eq:
                raise ValueError
            group[key] = tuple(float(v) for v in val.split('/')) if key == 'betas' else float(val)
            if key == 'betas' and len(group[key]) != 2:
                raise ValueError
        except ValueError:
            raise argparse.ArgumentTypeError('%r: expected lr=, eps=, weight_decay= (a number) or betas=B1/B2 in %r' % (item, text))
    return group


parse.add_argument('--freeze', action='append', default=None, metavar='PATTERN', help='fine-tuning: freeze the parameters whose state-dict name matches '
                   "the fnmatch pattern ('meta_net.*': the whole grid encoder, whose backward then does not run); repeatable (freeze=[...])")
parse.add_argument('--param_group', action='append', default=None, type=param_group_arg, metavar='PATTERNS:KEY=VALUE,...', help='fine-tuning: a parameter '
                   "group with hyper-parameters of its own, e.g. '*_net.coord_*_fc.*:lr=1e-5' or '*.bias,*norm*:weight_decay=0'; repeatable, earlier "
                   'groups win, the rest keeps the config\'s values (param_groups=[...])')


def load_config(path):
    if path is None:
        return ncep_config()
    ns = runpy.run_path(path)
    if 'config' not in ns:
        raise SystemExit('%s does not define `config`' % path)
    cfg = dict(ns['config'])
    cfg.setdefault('name', 'InterfacePhysics')
    return cfg


if __name__ == '__main__':
    args = parse.parse_args()
    print(args)
    cfg = load_config(args.config_file)
    model = builder_models(**cfg)
    if args.checkpoint_path is not None:
        os.makedirs(args.checkpoint_path, exist_ok=True)
        if args.config_file is not None:                  # the reference copies the config next to the checkpoints (train.py:44)
            shutil.copy(args.config_file, os.path.join(args.checkpoint_path, os.path.basename(args.config_file)))
    kwargs = dict(checkpoint_path=args.checkpoint_path, log_path=args.log_path)
    if args.max_steps is not None:
        kwargs['max_steps'] = args.max_steps
    if args.synthetic:
        kwargs['samples'] = 'synthetic'
    if args.valid_synthetic:
        kwargs['valid_samples'] = 'synthetic'
    if args.adaptive_interior:
        kwargs['adaptive_interior'] = dict(pool_factor=8, k=1.0, c=1.0, every=1)
    if args.causal_weights is not None:
        kwargs['causal_weights'] = dict(eps=args.causal_weights, bins=16, relative=True)
    if args.balance_losses is not None:
        kwargs['balance_losses'] = dict(every=args.balance_losses, momentum=0.9, groups='equations')
    if args.lead_batch is not None:
        kwargs['lead_batch'] = args.lead_batch
    if args.ema is not None:
        kwargs['ema_weights'] = dict(decay=args.ema, warmup=True)
    if step_guard_arg(args) is not None:
        kwargs['step_guard'] = step_guard_arg(args)
    if lbfgs_arg(args) is not None:
        kwargs['lbfgs'] = lbfgs_arg(args)
    if args.freeze:
        kwargs['freeze'] = args.freeze
    if args.param_group:
        kwargs['param_groups'] = args.param_group
    run = model.run_train_interface_dist if args.dist else model.run_train_interface
    out = run(**kwargs)
    lrs = out['lr'] if isinstance(out['lr'], list) else [out['lr']]
    print('done: epoch %d, global_step %d, lr %s' % (out['epoch'], out['global_step'], ' '.join('%.3e' % v for v in lrs)))
    if out.get('last_validation') is not None:
        print('last validation: valid loss %.6g at step %d' % (float(out['last_validation']['valid_loss']), out['last_validation']['global_step']))
