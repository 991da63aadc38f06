"""Fixture F14 (tests/golden/f14_validation.npz): the validation branch of the reference's training loop, run by the reference's own objects.

    python tests/golden/make_golden_validation.py

Like make_golden.py this imports the reference where it exists (make_golden.load_reference: third-party stand-ins, the reference's modules
unmodified, oracle/fill.py's closed-form parameters) and commits only what it computed.  The order of operations is that of
interface/interface_physics.py:629-719: with_clip = True; encoding_coord + physics_net.forward on the margin points; the prediction criterion
(builder_loss(**prediction_loss)) times margin_factor; with the PDE losses place_one_batch on the interior points, then on the margin points (the
twelve terms are caught from the `summary` object it reports them to); valid loss = their sum in that order; inverse_norm of the margin
predictions and of their labels; builder_loss(name='MSELoss') per variable.

Inputs are NOT stored: synthetic_inputs(256, tag='inter') and synthetic_inputs(256, tag='margin', margin=True), the points of F5 / F8 / F13.
Recorded (scalars only): with and without the PDE losses in fp32 -- margin_loss, inter_pde_loss, margin_pde_loss, valid_loss, terms [2, 6],
mse [6], mse_noclip [6] --; both sets of MSEs from an fp64 run of the same objects; max |out_n| of the margin predictions per variable (fp32 run).

The reference's inverse_norm ignores its own `with_clip` argument and clips P, T, q, rho whenever self.with_clip is set (:256-259), which :629
has just done: the loop's six MSEs are therefore CLIPPED ones (`mse`, `mse_fp64`), and on these inputs the bounds do bind (`clip_binds` counts
the values on a bound; q's labels fall below 1e-6).  The same calls with self.with_clip = False -- what the call at :706-713 reads like, and the
default of this project's validation_step -- are recorded next to them (`mse_noclip`, `mse_noclip_fp64`); only q differs (1.6 %).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

N_POINTS = 256
TERMS = ('montion_u_loss', 'montion_v_loss', 'continous_loss', 'energy_loss', 'vapor_loss', 'gas_loss')    # the order of this project's terms [6]


class _Summary:
    """Stands in for the tensorboard writer: keeps what place_one_batch reports."""

    def __init__(self):
        self.scalars = {}

    def add_scalar(self, name, value, step):
        self.scalars[name] = float(value)


def run_validation(m, cfg, builder_loss, inter, margin, with_pde, dtype):
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    inter, margin = {k: c(v) for k, v in inter.items()}, {k: c(v) for k, v in margin.items()}
    tc = cfg.config['train_cfg']
    pde_criterion = builder_loss(**tc['losses']['pde_loss'])
    prediction_criterion = builder_loss(**tc['losses']['prediction_loss'])
    variable_criterion = builder_loss(name='MSELoss')
    loss_factor = tc['losses']['loss_factor']
    summary = _Summary()
    m.with_clip = True                                                                       # :629
    field_data, forecast_h = margin['field_data'], margin['forecast_h']
    margin_input = m.encoding_coord(margin['x'], margin['y'], margin['t'], m.pred_t_span)   # :655
    fields = m.physics_net.forward(field_data, margin_input, margin['coord_data'], forecast_h)
    margin_loss = prediction_criterion(torch.cat(fields, dim=1), margin['labels']).float()
    margin_loss = margin_loss * loss_factor['margin_factor']
    loss_dict = {'margin_loss': margin_loss}
    if with_pde:
        x, y, t = (inter[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
        inter_loss = m.place_one_batch(x, y, t, inter['f'], field_data, inter['coord_data'], forecast_h, pde_criterion, loss_factor,
                                       1, 0, 'cpu', summary, 'inter', log_step=100).detach()
        mx, my, mt = (margin[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
        margin_pde_loss = m.place_one_batch(mx, my, mt, margin['f'], field_data, margin['coord_data'], forecast_h, pde_criterion, loss_factor,
                                            1, 0, 'cpu', summary, 'margin', log_step=100).detach()
        loss_dict['inter_pde_loss'] = inter_loss.detach()
        loss_dict['margin_pde_loss'] = margin_pde_loss.detach()
    valid_loss = 0
    for key, v in loss_dict.items():
        valid_loss = valid_loss + v.detach()
    lab = margin['labels']
    mses = {}
    for key, clip in (('mse', True), ('mse_noclip', False)):        # 'mse': the loop as it is (with_clip still True from :629)
        m.with_clip = clip
        pred = m.inverse_norm(*(f_.detach() for f_ in fields), m.obs_norm_cfg)
        label = m.inverse_norm(lab[:, 0:1], lab[:, 1:2], lab[:, 2:3], lab[:, 3:4], lab[:, 4:5], lab[:, 5:6], m.obs_norm_cfg)
        mses[key] = np.array([float(variable_criterion(p_, l_).detach()) for p_, l_ in zip(pred, label)], np.float64)
    m.with_clip = True
    pred = m.inverse_norm(*(f_.detach() for f_ in fields), m.obs_norm_cfg)
    label = m.inverse_norm(lab[:, 0:1], lab[:, 1:2], lab[:, 2:3], lab[:, 3:4], lab[:, 4:5], lab[:, 5:6], m.obs_norm_cfg)
    # does a clip bound bind on either side?  (P, T, q, rho only)
    binds = 0
    for k, name in enumerate(('u10', 'v10', 'pres', 't2', 'q2', 'rio')):
        if k >= 2:
            lo, hi = m.obs_norm_cfg[name]['bound']
            for v in (pred[k], label[k]):
                binds += int(((v <= lo) | (v >= hi)).sum())
    rec = {'margin_loss': float(margin_loss.detach()), 'valid_loss': float(valid_loss)}
    rec.update(mses)
    if with_pde:
        rec['inter_pde_loss'], rec['margin_pde_loss'] = float(loss_dict['inter_pde_loss']), float(loss_dict['margin_pde_loss'])
        rec['terms'] = np.array([[summary.scalars['%s/%s' % (g, t_)] for t_ in TERMS] for g in ('inter', 'margin')], np.float64)
    out_abs = np.array([float(f_.detach().abs().max()) for f_ in fields], np.float64)
    return rec, out_abs, binds


def main():
    from make_golden import load_reference
    from oracle.fill import fill_state_dict_, synthetic_inputs
    torch.manual_seed(0)
    torch.set_num_threads(8)
    m, cfg = load_reference()
    from DeepPhysiNet.losses.builder import builder_loss            # load_reference() put the reference on sys.path
    m.eval()
    sd = m.physics_net.state_dict()
    fill_state_dict_(sd)
    m.physics_net.load_state_dict(sd, strict=True)
    inter = synthetic_inputs(N_POINTS, tag='inter')
    margin = synthetic_inputs(N_POINTS, tag='margin', margin=True)
    out = {'n_points': np.array(N_POINTS, np.int64)}
    binds_total = 0
    for with_pde in (True, False):
        rec, out_abs, binds = run_validation(m, cfg, builder_loss, inter, margin, with_pde, torch.float32)
        binds_total += binds
        for k, v in rec.items():
            out['pde%d.%s' % (int(with_pde), k)] = np.asarray(v, np.float64)
        if with_pde:
            out['out_n_abs_max'] = out_abs
    m.double()
    m.pe.double()
    rec64, _, binds = run_validation(m, cfg, builder_loss, inter, margin, False, torch.float64)
    out['mse_fp64'], out['mse_noclip_fp64'] = rec64['mse'], rec64['mse_noclip']
    out['clip_binds'] = np.array(binds_total + binds, np.int64)
    np.savez_compressed(os.path.join(HERE, 'f14_validation.npz'), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == '__main__':
    main()
