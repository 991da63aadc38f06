#!/usr/bin/env python
"""Inference launcher next to train.py, with the same three flags: --config_file, --checkpoint_path, --log_path.

    python infer.py [--config_file cfg.py] [--checkpoint_path DIR] [--log_path DIR] [--synthetic [--synthetic_samples N]] [--ema] [--diagnostics name[,name...]]
                    [--trajectories LON,LAT[;LON,LAT...] --traj_start H --traj_hours D --traj_step S [--traj_method rk4]]
                    [--ensemble name[,name...] [--ensemble_threshold NAME:V[,V...]]...]
                    [--extremes T:max,T:min,speed:max --extreme_window H0,H1 [--extreme_scan S] [--extreme_refine R]]
                    [--spells T:below:273.15,speed:above:15 --spell_window H0,H1 [--spell_scan S] [--spell_refine R]]
                    [--regions name[,name...] --region_labels FILE.npy [--region_weights area|FILE.npy] [--region_threshold NAME:V[,V...]]...]
                    [--verify name[,name...] --verify_obs FILE.npz [--verify_threshold NAME:[above|below:]V[,V...]]... [--verify_by station,hour,all]
                     [--verify_members K]]
                    [--verify_grid name[,name...] --verify_analysis FILE.npz --verify_grid_threshold NAME:[above|below:]V[,V...]...
                     [--verify_scales 1,3,5,9,17,33]]

Builds the interface from the config (train.py's loader), loads `physics_latest.pth` from --checkpoint_path (or inference_cfg.checkpoints) and
calls `run_inference_interface`: every field sample is evaluated on the lattice inference_cfg.img_size (x `refine`) at every inference_cfg.dt
seconds of its window, and with log.write_source the maps go to --log_path (or inference_cfg.log.result_path) as one .npy per time step and
exported variable.  The reference's dataset is file I/O that does not exist offline: a config that names no `samples` source fails, unless
--synthetic asks for a random field sample (smoke runs: the maps are noise).  --ema evaluates the checkpoint's averaged weights (`model_ema`, written by
train.py --ema) in place of the raw ones; a checkpoint without them is a KeyError.  --diagnostics vorticity,dT_dt sets
inference_cfg.log.export_diagnostic: derived products of the Jacobian (deepphysinet_amd.diagnostics.PRODUCTS), one more .npy per time step and name.
--trajectories 100.5,30.25;110,35 --traj_start 24 --traj_hours -24 --traj_step 0.25 sets inference_cfg.trajectories: parcels started at those places
(degrees east, north) at hour 24 of each sample's window and followed backward for a day in 15-minute RK4 steps through the network's own wind
(InterfacePhysics.trajectories); positions, hours, status, step counts and the six fields along the paths are written as <time>_traj_*.npy.
--ensemble speed,T --ensemble_threshold speed:10,15 sets inference_cfg.ensemble: after the per-sample maps, all samples are taken as the members of an
ensemble (InterfacePhysics.ensemble_lattice) and the mean, spread, min, max and count of every named product (deepphysinet_amd.ensemble.ENSEMBLE_PRODUCTS)
and the probability of exceeding each threshold are written as <time>_ens_*.npy.
--extremes T:max,T:min,speed:max --extreme_window 0,24 sets inference_cfg.extremes: per sample the maximum / minimum of the named products over those
hours of its window and the hour they occur at (or, PRODUCT:mean, the window mean), found by a scan every --extreme_scan hours and --extreme_refine
rounds of bisection on the network's own d/dt (InterfacePhysics.extreme_lattice), written as <time>_extreme_<value|hour|lo|hi|status>_*.npy maps.
--spells T:below:273.15,speed:above:15 --spell_window 0,24 sets inference_cfg.spells: per sample how long the named products stay strictly below / above
the thresholds over those hours of its window, the hour of the first entry and of the last exit, the crossings and the degree-hours, found by a scan
every --spell_scan hours and --spell_refine rounds of bisection on the sign of value - threshold (InterfacePhysics.spell_lattice), written as
<time>_spell_<hours|first|last|first_lo|last_hi|excess|crossings|status>_*.npy maps.
--regions vorticity,speed,T --region_labels catchments.npy --region_weights area --region_threshold T:273.15 sets inference_cfg.regions: per sample and
time step the area-weighted mean, total, minimum and maximum (and where they sit) of the named products over every region of the label plane, and the
share of each region above the thresholds (InterfacePhysics.regional_lattice: only the points inside a region are evaluated), written as
<time>_region_*.npy tables [time steps, regions].
--verify T,speed --verify_obs reports.npz --verify_threshold T:below:273.15 --verify_by station,hour,all sets inference_cfg.verify: after the per-sample
maps, all samples are taken as the cases of a verification (InterfacePhysics.verify_at) against the station reports of the file -- lon [S], lat [S],
hours [H], names [P], obs [M, H, S, P], M the samples in the source's order, NaN where there is no report -- and bias, MAE, RMSE, correlation, the same
for the interpolated coarse forecast, the skill against it and the contingency scores of every threshold are written per point, per station, per hour
and over everything as <time>_verify_*.npy tables.  Without --verify_obs there is nothing to verify against (synthetic samples come with no reports).
--verify_members K (default 1) takes K consecutive samples as the members of one case (obs then [M / K, H, S, P]) and scores the ensemble as a
distribution (InterfacePhysics.verify_ensemble_at): CRPS, rank histogram, spread against skill, and per threshold the Brier score with its
decomposition, the reliability diagram and the ROC area, for the model and the interpolated coarse forecast, as <time>_pverify_*.npy tables.
--verify_grid T,speed --verify_analysis analysis.npz --verify_grid_threshold T:below:273.15 --verify_grid_threshold speed:15 --verify_scales 1,3,5,9,17,33
sets inference_cfg.verify_grid: after the per-sample maps, all samples are taken as the cases of a neighbourhood verification on the fine grid
(InterfacePhysics.verify_lattice) against the gridded analysis of the file -- names [P], hours [H], analysis [M, H, P, ny, nx] on the fine grid's nodes,
NaN where there is none -- and the fractions skill score of the model and of the interpolated coarse forecast at every window width (in nodes, odd),
the event frequencies, the frequency biases and the smallest skilful scale are written per hour and over all hours as <time>_nbhd_*.npy tables."""
import argparse

import torch

from deepphysinet_amd.interface import builder_models
from train import load_config

parse = argparse.ArgumentParser()
parse.add_argument('--config_file', default=None, type=str)
parse.add_argument('--checkpoint_path', default=None, type=str)
parse.add_argument('--log_path', default=None, type=str)
parse.add_argument('--synthetic', action='store_true', help="samples='synthetic': a random field sample over a random coarse cube")
parse.add_argument('--synthetic_samples', default=1, type=int, help='N: that many random field samples (the members and cases of --verify_members)')
parse.add_argument('--ema', action='store_true', help="weights='ema': the checkpoint's averaged weights (model_ema) in place of the raw ones")
parse.add_argument('--diagnostics', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='name[,name...]: inference_cfg.log.export_diagnostic, derived products (deepphysinet_amd.diagnostics.PRODUCTS) written next to the variables')
parse.add_argument('--trajectories', default=None, type=lambda s: [tuple(float(v) for v in p.split(',')) for p in s.split(';') if p],
                   help='LON,LAT[;LON,LAT...]: inference_cfg.trajectories, start places of parcel trajectories in degrees east, north')
parse.add_argument('--traj_start', default=0.0, type=float, help='start hour inside the sample window')
parse.add_argument('--traj_hours', default=None, type=float, help='duration in hours; negative: back-trajectories')
parse.add_argument('--traj_step', default=0.25, type=float, help='step in hours')
parse.add_argument('--traj_method', default='rk4', type=str, help='euler | midpoint | rk4')
parse.add_argument('--ensemble', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='name[,name...]: inference_cfg.ensemble.products, statistics over all samples as ensemble members (deepphysinet_amd.ensemble.ENSEMBLE_PRODUCTS)')
parse.add_argument('--ensemble_threshold', default=[], action='append', type=str,
                   help='NAME:V[,V...] (repeatable): inference_cfg.ensemble.thresholds, the probability that product NAME exceeds V')
parse.add_argument('--extremes', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='PRODUCT:SENSE[,...]: inference_cfg.extremes.columns, e.g. T:max,T:min,speed:max,q:mean (deepphysinet_amd.extremes)')
parse.add_argument('--extreme_window', default=None, type=lambda s: tuple(float(v) for v in s.split(',')),
                   help='H0,H1: the hours of the sample window the extremes are taken over')
parse.add_argument('--extreme_scan', default=1.0, type=float, help='hours between the scan nodes')
parse.add_argument('--extreme_refine', default=10, type=int, help='bisection rounds after the scan (0..32)')
parse.add_argument('--spells', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='PRODUCT:SIDE:THRESHOLD[,...]: inference_cfg.spells.columns, e.g. T:below:273.15,speed:above:15 (deepphysinet_amd.spells)')
parse.add_argument('--spell_window', default=None, type=lambda s: tuple(float(v) for v in s.split(',')),
                   help='H0,H1: the hours of the sample window the spells are looked for in')
parse.add_argument('--spell_scan', default=1.0, type=float, help='hours between the scan nodes')
parse.add_argument('--spell_refine', default=10, type=int, help='bisection rounds after the scan (0..32)')
parse.add_argument('--regions', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='name[,name...]: inference_cfg.regions.products, statistics per region and time step (deepphysinet_amd.ensemble.ENSEMBLE_PRODUCTS)')
parse.add_argument('--region_labels', default=None, type=str, help='FILE.npy: the int label plane [lat, lon] of the regions, -1 = in no region')
parse.add_argument('--region_weights', default=None, type=str, help="area (the cosine of the row's latitude) or FILE.npy, a plane of weights; default: ones")
parse.add_argument('--region_threshold', default=[], action='append', type=str,
                   help='NAME:V[,V...] (repeatable): inference_cfg.regions.thresholds, the share of the region where product NAME exceeds V')
parse.add_argument('--verify', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='name[,name...]: inference_cfg.verify.products, scores against reports (deepphysinet_amd.verification.VERIFY_PRODUCTS)')
parse.add_argument('--verify_obs', default=None, type=str, help='FILE.npz: lon [S], lat [S], hours [H], names [P], obs [M, H, S, P] (NaN: no report)')
parse.add_argument('--verify_threshold', default=[], action='append', type=str,
                   help='NAME:V[,V...] | NAME:above:V[,V...] | NAME:below:V[,V...] (repeatable): inference_cfg.verify.thresholds, the events that are scored')
parse.add_argument('--verify_members', default=1, type=int,
                   help='K: inference_cfg.verify.members, K consecutive samples are the members of one case (probabilistic scores; reports [M / K, H, S, P])')
parse.add_argument('--verify_by', default=['station', 'hour', 'all'], type=lambda s: [n for n in s.split(',') if n],
                   help='station,hour,all: inference_cfg.verify.by, the groupings the point scores are pooled over')
parse.add_argument('--verify_grid', default=None, type=lambda s: [n for n in s.split(',') if n],
                   help='name[,name...]: inference_cfg.verify_grid.products, fractions skill scores against a gridded analysis (VERIFY_PRODUCTS)')
parse.add_argument('--verify_analysis', default=None, type=str, help='FILE.npz: names [P], hours [H], analysis [M, H, P, ny, nx] on the fine grid (NaN: none)')
parse.add_argument('--verify_grid_threshold', default=[], action='append', type=str,
                   help='NAME:V[,V...] | NAME:above:V[,V...] | NAME:below:V[,V...] (repeatable): inference_cfg.verify_grid.thresholds, at least one')
parse.add_argument('--verify_scales', default=None, type=lambda s: [int(v) for v in s.split(',') if v],
                   help='W[,W...]: inference_cfg.verify_grid.scales, odd window widths in nodes, ascending (default 1,3,5,9,17,33)')


def _window_option(args, key, word):
    """inference_cfg[key] of --<key> / --<word>_window / --<word>_scan / --<word>_refine, or None without --<key>."""
    columns, window = getattr(args, key), getattr(args, word + '_window')
    if not columns:
        if window is not None:
            parse.error('--%s_window needs --%s' % (word, key))
        return None
    if window is None or len(window) != 2:
        parse.error('--%s needs --%s_window H0,H1' % (key, word))
    return dict(columns=list(columns), window=tuple(window), scan_hours=getattr(args, word + '_scan'), refine=getattr(args, word + '_refine'))


def extremes_option(args):
    """inference_cfg['extremes'] of --extremes / --extreme_window: dict(columns=[...], window=(H0, H1), scan_hours=S, refine=R), or None without
    --extremes."""
    return _window_option(args, 'extremes', 'extreme')


def spells_option(args):
    """inference_cfg['spells'] of --spells / --spell_window: dict(columns=[...], window=(H0, H1), scan_hours=S, refine=R), or None without --spells."""
    return _window_option(args, 'spells', 'spell')


def ensemble_option(args):
    """inference_cfg['ensemble'] of --ensemble / --ensemble_threshold: dict(products=[...], thresholds={name: [values]}), or None without --ensemble."""
    if not args.ensemble:
        if args.ensemble_threshold:
            parse.error('--ensemble_threshold needs --ensemble')
        return None
    return dict(products=list(args.ensemble), thresholds=_thresholds(args.ensemble_threshold, '--ensemble_threshold'))


def _thresholds(items, flag):
    """{name: [values]} of the repeated NAME:V[,V...] items of `flag`."""
    thresholds = {}
    for item in items:
        name, sep, values = item.partition(':')
        if not sep or not name or not values:
            parse.error('%s takes NAME:V[,V...], got %r' % (flag, item))
        thresholds.setdefault(name, []).extend(float(v) for v in values.split(',') if v)
    return thresholds


def regions_option(args):
    """inference_cfg['regions'] of --regions / --region_labels / --region_weights / --region_threshold: dict(products=[...], labels=FILE.npy,
    weights=None | 'area' | FILE.npy, thresholds={name: [values]}), or None without --regions."""
    if not args.regions:
        if args.region_labels or args.region_weights or args.region_threshold:
            parse.error('--region_labels, --region_weights and --region_threshold need --regions')
        return None
    if not args.region_labels:
        parse.error('--regions needs --region_labels FILE.npy')
    return dict(products=list(args.regions), labels=args.region_labels, weights=args.region_weights,
                thresholds=_thresholds(args.region_threshold, '--region_threshold'))


def _sided_thresholds(items, flag):
    """{name: [('above' | 'below', value), ...]} of the NAME:[above|below:]V[,V...] items of `flag`."""
    thresholds = {}
    for item in items:
        parts = item.split(':')
        if len(parts) == 2:
            parts = [parts[0], 'above', parts[1]]
        if len(parts) != 3 or not parts[0] or parts[1] not in ('above', 'below') or not parts[2]:
            parse.error('%s takes NAME:V[,V...], NAME:above:V[,V...] or NAME:below:V[,V...], got %r' % (flag, item))
        thresholds.setdefault(parts[0], []).extend((parts[1], float(v)) for v in parts[2].split(',') if v)
    return thresholds


def verify_grid_option(args):
    """inference_cfg['verify_grid'] of --verify_grid / --verify_analysis / --verify_grid_threshold / --verify_scales: dict(products=[...],
    analysis=FILE.npz, thresholds={name: [('above' | 'below', value), ...]}, scales=[...]), or None without --verify_grid."""
    if not args.verify_grid:
        if args.verify_analysis or args.verify_grid_threshold or args.verify_scales:
            parse.error('--verify_analysis, --verify_grid_threshold and --verify_scales need --verify_grid')
        return None
    if not args.verify_analysis:
        parse.error('--verify_grid needs --verify_analysis FILE.npz (names, hours, analysis [M, H, P, ny, nx]): there is nothing to verify against '
                    'without an analysis, and --synthetic samples come with none')
    if not args.verify_grid_threshold:
        parse.error('--verify_grid needs at least one --verify_grid_threshold NAME:[above|below:]V[,V...]: the fractions skill score is a score of events')
    option = dict(products=list(args.verify_grid), analysis=args.verify_analysis,
                  thresholds=_sided_thresholds(args.verify_grid_threshold, '--verify_grid_threshold'))
    if args.verify_scales:
        option['scales'] = list(args.verify_scales)
    return option


def verify_option(args):
    """inference_cfg['verify'] of --verify / --verify_obs / --verify_threshold / --verify_by: dict(products=[...], obs=FILE.npz, thresholds={name:
    [values and ('below', value) pairs]}, by=[...]), or None without --verify."""
    if not args.verify:
        if args.verify_obs or args.verify_threshold or args.verify_members != 1:
            parse.error('--verify_obs, --verify_threshold and --verify_members need --verify')
        return None
    if not args.verify_obs:
        parse.error('--verify needs --verify_obs FILE.npz (lon, lat, hours, names, obs [M, H, S, P]): there is nothing to verify against without '
                    'reports, and --synthetic samples come with none')
    thresholds = _sided_thresholds(args.verify_threshold, '--verify_threshold')
    option = dict(products=list(args.verify), obs=args.verify_obs, thresholds=thresholds, by=list(args.verify_by))
    if args.verify_members != 1:
        option['members'] = args.verify_members
    return option


if __name__ == '__main__':
    args = parse.parse_args()
    print(args)
    cfg = load_config(args.config_file)
    if args.log_path is not None:
        cfg.setdefault('inference_cfg', {}).setdefault('log', {})['result_path'] = args.log_path
    if args.diagnostics:
        cfg.setdefault('inference_cfg', {}).setdefault('log', {})['export_diagnostic'] = args.diagnostics
    if args.trajectories:
        if args.traj_hours is None or any(len(p) != 2 for p in args.trajectories):
            parse.error('--trajectories takes LON,LAT pairs and needs --traj_hours')
        cfg.setdefault('inference_cfg', {})['trajectories'] = dict(lonlat=args.trajectories, start=args.traj_start, hours=args.traj_hours,
                                                                   step=args.traj_step, method=args.traj_method)
    if ensemble_option(args):
        cfg.setdefault('inference_cfg', {})['ensemble'] = ensemble_option(args)
    if extremes_option(args):
        cfg.setdefault('inference_cfg', {})['extremes'] = extremes_option(args)
    if spells_option(args):
        cfg.setdefault('inference_cfg', {})['spells'] = spells_option(args)
    if regions_option(args):
        cfg.setdefault('inference_cfg', {})['regions'] = regions_option(args)
    if verify_option(args):
        cfg.setdefault('inference_cfg', {})['verify'] = verify_option(args)
    if verify_grid_option(args):
        cfg.setdefault('inference_cfg', {})['verify_grid'] = verify_grid_option(args)
    model = builder_models(**cfg)
    kwargs = dict(checkpoint_path=args.checkpoint_path)
    if args.synthetic:
        kwargs['samples'] = 'synthetic'
        if args.synthetic_samples != 1:
            kwargs['samples_per_epoch'] = args.synthetic_samples
    if args.ema:
        kwargs['weights'] = 'ema'
    maps = model.run_inference_interface(**kwargs)
    if maps is None:
        print('done: no samples')
    else:
        print('done: maps %s, finite %s' % (tuple(maps.shape), bool(torch.isfinite(maps).all())))
    if model.last_diagnostics is not None:
        d = model.last_diagnostics
        print('diagnostics %s: maps %s, finite %s' % (','.join(d['names']), tuple(d['maps'].shape), bool(torch.isfinite(d['maps']).all())))
    if model.last_trajectories is not None:
        tr = model.last_trajectories
        print('trajectories: positions %s, steps done %s, status %s' % (tuple(tr['positions'].shape), tr['steps_done'].tolist(), tr['status'].tolist()))
    if model.last_ensemble is not None:
        e = model.last_ensemble
        print('ensemble %s: mean %s, members counted %d..%d, thresholds %s' % (','.join(e['names']), tuple(e['mean'].shape), int(e['count'].min()),
                                                                             int(e['count'].max()), e['thresholds']))
    if model.last_extremes is not None:
        x = model.last_extremes
        print('extremes %s: value %s, status %s' % (','.join(x['names']), tuple(x['value'].shape), sorted(set(x['status'].reshape(-1).tolist()))))
    if model.last_spells is not None:
        x = model.last_spells
        print('spells %s: hours %s, status %s' % (','.join(x['names']), tuple(x['hours'].shape), sorted(set(x['status'].reshape(-1).tolist()))))
    if model.last_regions is not None:
        r = model.last_regions
        print('regions %s: mean %s, points counted %d..%d, thresholds %s' % (','.join(r['names']), tuple(r['mean'].shape), int(r['count'].min()),
                                                                           int(r['count'].max()), r['thresholds']))
    if model.last_verification is not None:
        v = model.last_verification
        print('verification %s%s: point %s, pairs counted %d..%d, groupings %s, thresholds %s'
              % (','.join(v['names']), ' of %d members' % v['members'] if 'members' in v else '', tuple(v['point']['bias'].shape),
                 int(v['point']['count'].min()), int(v['point']['count'].max()), [k for k in v if k not in ('names', 'thresholds', 'members', 'point')],
                 v['thresholds']))
    if model.last_grid_verification is not None:
        v = model.last_grid_verification
        print('neighbourhood verification %s: fss %s, scales %s, nodes counted %d..%d, thresholds %s'
              % (','.join(v['names']), tuple(v['hour']['fss'].shape), v['scales'], int(v['hour']['count'].min()), int(v['hour']['count'].max()),
                 v['thresholds']))
