"""Timing of the validation pass, hi+lo mode, eager launches, a host clock around work that ends in a device synchronise, median and spread
(min .. max) of the timed repetitions after warm-up; the two routes alternate in one process, so both see the same state of the box.

  (a) the route there was before: data_loss + two place_one_batch under no_grad, then inverse_norm / MSELoss per variable in torch
      (three point passes on overlapping points, three encoder passes);
  (b) validation_step: one point pass without saved state, the label statistics from one kernel;
on the shipped batch (4 096 interior + 20 480 margin points), and over a validation set of 61 samples: 61 x (a) against validate().

usage: python tools/validation_time.py [reps] [samples]        (default 7 repetitions, 61 samples)"""
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
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(v):
    return '%.2f ms (min %.2f .. max %.2f, n = %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import SyntheticSamples
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 61
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    m = builder_models(**ncep_config(), precision='bf16x2').to(dev)
    lf = m.train_cfg['losses']['loss_factor']
    src = SyntheticSamples(dev, leads=n_samples, seed=1)
    samples = [src[i] for i in range(n_samples)]
    crit, mse = torch.nn.MSELoss(), torch.nn.MSELoss()

    def old_route(b):
        with torch.no_grad():
            out = {'margin_loss': m.data_loss(b['margin_x'], b['margin_y'], b['margin_t'], b['field_data'], b['margin_input_data'], b['margin_data'],
                                              b['forecast_h'], lf['margin_factor'])}
            out['inter_pde_loss'] = m.place_one_batch(b['inter_x'], b['inter_y'], b['inter_t'], b['inter_f'], b['field_data'], b['inter_data'],
                                                      b['forecast_h'], crit, lf, 0, 0, dev)
            out['margin_pde_loss'] = m.place_one_batch(b['margin_x'], b['margin_y'], b['margin_t'], b['margin_f'], b['field_data'],
                                                       b['margin_input_data'], b['forecast_h'], crit, lf, 0, 0, dev, prefix='margin')
            fields = m.physics_net.forward_xyt(b['field_data'], b['margin_x'], b['margin_y'], b['margin_t'], b['margin_input_data'], b['forecast_h'])
            keep, m.with_clip = m.with_clip, False
            pred = m.inverse_norm(*fields, m.obs_norm_cfg)
            lab = m.inverse_norm(*(b['margin_data'][:, k:k + 1] for k in range(6)), m.obs_norm_cfg)
            m.with_clip = keep
            out['mse'] = torch.stack([mse(p, l) for p, l in zip(pred, lab)])
            out['valid_loss'] = out['margin_loss'] + out['inter_pde_loss'] + out['margin_pde_loss']
        return out

    b0 = samples[0]
    for _ in range(2):
        a, c = old_route(b0), m.validation_step(b0)
    got = torch.tensor([c['variables'][v]['mse'] for v in ('u', 'v', 'p', 'T', 'q', 'rio')], dtype=torch.float64)
    print('one sample, %d + %d points: valid loss old %.6g new %.6g; per-variable MSE max rel. difference %.2e'
          % (b0['inter_x'].shape[0], b0['margin_x'].shape[0], float(a['valid_loss']), float(c['valid_loss']),
             float(((a['mse'].double().cpu() - got).abs() / got).max())))
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(_timed(lambda: old_route(b0))[0])
        t_new.append(_timed(lambda: m.validation_step(b0))[0])
    print('  (a) data_loss + 2 x place_one_batch + inverse_norm / MSELoss: %s' % _stats(t_old))
    print('  (b) validation_step:                                         %s' % _stats(t_new))
    sweep_old = lambda: [old_route(b) for b in samples]
    sweep_new = lambda: m.validate(samples)
    sweep_old(), sweep_new()
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(_timed(sweep_old)[0])
        t_new.append(_timed(sweep_new)[0])
    print('%d samples (validate: groups of %d):' % (n_samples, m.lead_batch_size(b0['inter_x'].shape[0] + b0['margin_x'].shape[0], n_samples)))
    print('  (a) %d x the old route: %s' % (n_samples, _stats(t_old)))
    print('  (b) validate:            %s' % _stats(t_new))


if __name__ == '__main__':
    main()
