#!/usr/bin/env python
"""Inference launcher next to train.py, with the same three flags: --config_file, --checkpoint_path, --log_path.

    python infer.py [--config_file cfg.py] [--checkpoint_path DIR] [--log_path DIR] [--synthetic] [--ema]

Builds the interface from the config (train.py's loader), loads `physics_latest.pth` from --checkpoint_path (or inference_cfg.checkpoints) and
calls `run_inference_interface`: every field sample is evaluated on the lattice inference_cfg.img_size (x `refine`) at every inference_cfg.dt
seconds of its window, and with log.write_source the maps go to --log_path (or inference_cfg.log.result_path) as one .npy per time step and
exported variable.  The reference's dataset is file I/O that does not exist offline: a config that names no `samples` source fails, unless
--synthetic asks for a random field sample (smoke runs: the maps are noise).  --ema evaluates the checkpoint's averaged weights (`model_ema`, written by
train.py --ema) in place of the raw ones; a checkpoint without them is a KeyError."""
import argparse

import torch

from deepphysinet_amd.interface import builder_models
from train import load_config

parse = argparse.ArgumentParser()
parse.add_argument('--config_file', default=None, type=str)
parse.add_argument('--checkpoint_path', default=None, type=str)
parse.add_argument('--log_path', default=None, type=str)
parse.add_argument('--synthetic', action='store_true', help="samples='synthetic': a random field sample over a random coarse cube")
parse.add_argument('--ema', action='store_true', help="weights='ema': the checkpoint's averaged weights (model_ema) in place of the raw ones")

if __name__ == '__main__':
    args = parse.parse_args()
    print(args)
    cfg = load_config(args.config_file)
    if args.log_path is not None:
        cfg.setdefault('inference_cfg', {}).setdefault('log', {})['result_path'] = args.log_path
    model = builder_models(**cfg)
    kwargs = dict(checkpoint_path=args.checkpoint_path)
    if args.synthetic:
        kwargs['samples'] = 'synthetic'
    if args.ema:
        kwargs['weights'] = 'ema'
    maps = model.run_inference_interface(**kwargs)
    if maps is None:
        print('done: no samples')
    else:
        print('done: maps %s, finite %s' % (tuple(maps.shape), bool(torch.isfinite(maps).all())))
