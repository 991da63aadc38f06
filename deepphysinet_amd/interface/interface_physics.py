"""InterfacePhysics: the reference's training-interface surface for the physics-informed step
(interface/interface_physics.py:32-332 and the step bodies :443-515 / :990-1065).

Hot methods (`place_one_batch`, `data_loss`, `training_step`) run the fused HIP point path.  The six
`*_equation` methods and `gradient` keep the reference's signatures and formulas as plain torch expressions, for
callers that hold autograd-connected fields of their own.  File I/O, visualisation and the epoch loops of the
reference are out of scope.
"""
import contextlib
import os
import shutil
import types

import numpy as np
import torch
import torch.nn as nn

from ..balance import LossBalance
from ..causal import CausalWeights
from ..diagnostics import product_ids
from ..ensemble import check_thresholds, ensemble_ids
from ..trajectory import check_request, domain_of
from .. import extremes as X
from .. import spells as SP
from .. import regions as RG
from .. import verification as VF
from .. import prob_verification as PV
from .. import neighbourhood as NB
from ..losses.builder import builder_loss
from ..model.physics_net import PhysicsNet
from ..guard import StepGuard
from ..lbfgs import FusedLBFGS
from ..optim import GROUP_KEYS, FusedClipAdam, resolve_param_groups
from ..point_path import (balance_sumsq, balance_update, balanced_total, data_losses_batch, eval_step, eval_step_batch, grid_maps, label_errors, ParcelState,
                          EnsembleState, ExtremeState, LOSS_ORDER, NbhdState, OBS_ORDER, PackedField, ProbVerifyState, RegionState, SpellState, VerifyState, pde_losses, pde_losses_batch, point_buffers, point_fields, point_sizes,
                          PointConfig, require_gpu, smooth_l1_data_loss, step_losses, step_losses_batch)
from ..sampler import SyntheticSamples
from ..staged_backward import StagedBackward
from ..utils.position_encoding import SineCosPE
from .. import _lib as L, encoder_ops, grad_arena, validation as V
from .inference_run import PRODUCTS, run_inference


def _loop_option(kwargs, train_cfg, name, section, known, true_is_empty, instance_of, build):
    """An option of the training loops: the keyword `name`, or train_cfg[section][name].  None / False: off (None); an instance of `instance_of`
    passes through; True: {} where true_is_empty; a dict of `known` keys -> build(dict)."""
    opt = kwargs.get(name, (train_cfg.get(section) or {}).get(name))
    if opt is None or opt is False:
        return None
    if instance_of is not None and isinstance(opt, instance_of):
        return opt
    if opt is True and true_is_empty:
        opt = {}
    unknown = set(opt) - set(known)
    if unknown:
        raise ValueError('%s: unknown keys %s (known: %s)' % (name, sorted(unknown), ', '.join(known)))
    return build(opt)


def _to_device(batch, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _chunks(total, chunk):
    """(first, n) of the chunks of `total` points, `chunk` at a time, the last one shorter."""
    for first in range(0, total, chunk):
        yield first, min(chunk, total - first)


class InterfacePhysics(nn.Module):
    def __init__(self, meta_cfg: dict, net_cfg: dict, obs_norm_cfg: dict, variable_cfg: dict, train_cfg: dict, test_cfg=None,
                 inference_cfg: dict = None, precision='bf16x2', **kwargs):
        super().__init__()
        self.net_cfg, self.obs_norm_cfg, self.variable_cfg = net_cfg, obs_norm_cfg, variable_cfg
        self.train_cfg, self.test_cfg, self.inference_cfg = train_cfg, test_cfg, inference_cfg
        self.physics_net = PhysicsNet(meta_cfg, net_cfg)
        self.pe = SineCosPE(3, include_input=False)
        img_size = self.train_cfg['img_size']
        if isinstance(img_size, (int, float)):
            self.lat_size, self.lon_size = img_size, img_size
        elif isinstance(img_size, (list, tuple)) and len(img_size) == 2:
            self.lat_size, self.lon_size = img_size
        else:
            raise NotImplementedError
        # attributes the reference only sets inside its training loops (:339-342, :412-418, :438)
        self.dx = float(train_cfg.get('dx', 27000.0))
        self.dy = float(train_cfg.get('dy', 27000.0))
        self.dt = 3600.0 * float(train_cfg.get('lable_time_step', 1))
        td = train_cfg.get('train_data', {})
        self.pred_t_span = float(td.get('input_time_step', 6)) * float(td.get('input_time_step_nums', 4)) * 3600.0
        self.with_clip = True
        self.precision = L.PREC_NAMES[precision]
        self._cfg_cache = None
        self.loss_balance_state = None          # training_step(balance=...): {'groups', 'lam' (fp32 [K], device), 'step', 'diag' (device or None)}
        for p in PRODUCTS:                      # run_inference_interface: where each product's result of the last run stays (inference_run.PRODUCTS)
            setattr(self, p.last, None)

    # ------------------------------------------------------------------ configuration of the HIP path
    def point_config(self, loss_factor=None, criterion=None) -> PointConfig:
        crit_kind, crit_beta, crit_sum = self._check_pde_criterion(criterion if criterion is not None else self.train_cfg['losses'].get('pde_loss', {'name': 'MSELoss'}))
        # inverse_norm (:232-262) per variable as (out * std + mean) [squared and shifted] + optional clip: mean_norm v * nf[1] + nf[0]; min_max
        # v * (nf[1] - nf[0]) + nf[0], with a third factor (v * (nf[1] - nf[0]) + nf[0]) ** 2 + nf[2] (:244-247); use_norm False: the identity and no
        # clip (the reference clips inside its `if use_norm`: bounds of +-FLT_MAX never bind)
        mean, std, clipv, sq = [], [], [], []
        for k in OBS_ORDER:
            c = self.obs_norm_cfg[k]
            if not c.get('use_norm', True):
                mean.append(0.0), std.append(1.0), clipv.append(False), sq.append(None)
                continue
            nf = c['norm_factor']
            if c.get('norm_type', 'mean_norm').lower() == 'min_max':
                mean.append(float(nf[0])), std.append(float(nf[1]) - float(nf[0]))
                sq.append(None if len(nf) == 2 else float(nf[2]))
            else:
                mean.append(float(nf[0])), std.append(float(nf[1])), sq.append(None)
            clipv.append(True)
        lf = loss_factor or self.train_cfg['losses']['loss_factor']
        big = 3.4028234663852886e38
        bound = lambda k, i: (float(self.obs_norm_cfg[k]['bound'][i]) if ('bound' in self.obs_norm_cfg[k] and self.obs_norm_cfg[k].get('use_norm', True))
                              else (-big, big)[i])
        bounds = tuple((bound(k, 0), bound(k, 1)) for k in OBS_ORDER)        # part of the key: a changed clip bound alone must rebuild the configuration
        key = (self.dx, self.dy, self.lon_size, self.lat_size, self.pred_t_span, bool(self.with_clip), self.precision,
               tuple(float(lf[k]) for k in LOSS_ORDER), tuple(mean), tuple(std), tuple(clipv), crit_kind, crit_beta, tuple(sq), crit_sum, bounds)
        if self._cfg_cache is None or self._cfg_cache[0] != key:
            cfg = PointConfig(dx=self.dx, dy=self.dy, lon_size=self.lon_size, lat_size=self.lat_size, pred_t_span=self.pred_t_span,
                              mean=tuple(mean), std=tuple(std),
                              clip_lo=tuple(bound(k, 0) for k in OBS_ORDER), clip_hi=tuple(bound(k, 1) for k in OBS_ORDER),
                              with_clip=bool(self.with_clip), clip_vars=tuple(clipv), factors=key[7], prec=self.precision,
                              criterion=crit_kind, beta=crit_beta, sq_add=tuple(sq), reduce_sum=crit_sum)
            self._cfg_cache = (key, cfg)
        self.physics_net.point_cfg = self._cfg_cache[1]
        return self._cfg_cache[1]

    # ------------------------------------------------------------------ checkpoints (:53-88)
    def save_model(self, checkpoint_path, epoch, global_step, prefix='physics', **kwargs):
        checkpoint_file = os.path.join(checkpoint_path, '%s_%d.pth' % (prefix, epoch))
        state_dict = {'model': self.physics_net.state_dict(), 'epoch': epoch, 'gobal_step': global_step}
        state_dict.update(kwargs)
        lb = self.loss_balance_state
        if lb is not None:                                   # the loss-balancing weights and their step counter (training_step(balance=...))
            state_dict['loss_balance'] = {'groups': lb['groups'], 'lam': lb['lam'].detach().cpu().clone(), 'step': int(lb['step'])}
        torch.save(state_dict, checkpoint_file)
        shutil.copy(checkpoint_file, os.path.join(checkpoint_path, '%s_latest.pth' % prefix))

    def load_model(self, checkpoint_path, current_epoch=None, prefix='downscale', map_location='cpu'):
        if os.path.isfile(checkpoint_path):
            model_file = checkpoint_path
        elif current_epoch is None:
            model_file = os.path.join(checkpoint_path, '%s_latest.pth' % prefix)
        else:
            model_file = os.path.join(checkpoint_path, '%s_%d.pth' % (prefix, current_epoch))
        if not os.path.exists(model_file):
            print('warning:%s does not exist!' % model_file)
            return None, 0, 0
        state_dict = torch.load(model_file, map_location=map_location)
        glob_step = state_dict.pop('gobal_step', 0)
        epoch = state_dict.pop('epoch', 0)
        lb = state_dict.get('loss_balance')
        if lb is not None:                                   # (a checkpoint without the key leaves the state as it is)
            self.loss_balance_state = {'groups': lb['groups'], 'lam': lb['lam'].to(dtype=torch.float32).contiguous(), 'step': int(lb['step']), 'diag': None}
        # checkpoints written under DDP carry a 'module.' prefix (:1397 via :56); accept both
        if 'model' in state_dict and any(k.startswith('module.') for k in state_dict['model']):
            state_dict['model'] = {k[len('module.'):] if k.startswith('module.') else k: v for k, v in state_dict['model'].items()}
        return state_dict, epoch + 1, glob_step

    # ------------------------------------------------------------------ generic torch expressions (reference formulas)
    def gradient(self, y, x):
        return torch.autograd.grad(y, x, grad_outputs=torch.ones_like(y), create_graph=True, only_inputs=True, allow_unused=False)[0]

    def montion_equation_u(self, x, y, t, u, v, p, rio, f, loss, factor=1e-6):
        lhs = self.gradient(u, t) + u * self.gradient(u, x) + v * self.gradient(u, y) + self.gradient(p, x) / rio
        return loss(lhs, f * v).float() * factor

    def montion_equation_v(self, x, y, t, u, v, p, rio, f, loss, factor=1e-6):
        lhs = self.gradient(v, t) + u * self.gradient(v, x) + v * self.gradient(v, y) + self.gradient(p, y) / rio
        return loss(lhs, -f * u).float() * factor

    def continuous_equation(self, x, y, t, u, v, rio, loss, factor=1e-6):
        lhs = (self.gradient(rio, t) + u * self.gradient(rio, x) + v * self.gradient(rio, y)
               + rio * self.gradient(u, x) + rio * self.gradient(v, y))
        return loss(lhs, torch.zeros_like(lhs).float()).float() * factor

    def _advect(self, a, x, y, t, u, v):
        return self.gradient(a, t) + u * self.gradient(a, x) + v * self.gradient(a, y)

    def energy_equation(self, x, y, t, u, v, p, T, rio, q, loss, factor=1e-6, c_p=1005, L=2.5e6):
        lhs = c_p * self._advect(T, x, y, t, u, v) + (-self._advect(p, x, y, t, u, v) / (rio + 1e-6)) + L * self._advect(q, x, y, t, u, v)
        return loss(lhs, torch.zeros_like(lhs).float()).float() * factor

    def get_qs(self, p, T):
        tc = T - 273.15
        e_s = 6.112 * torch.exp(17.67 * tc / (tc + 243.5)) * 100
        return 0.622 * e_s / (p - 0.378 * e_s)

    def vapor_equation(self, x, y, t, u, v, p, T, q, loss, factor=1e-5, c_p=1005, L=2.5e6, R_v=461.5, R_d=287):
        omega = self._advect(p, x, y, t, u, v)
        q_adv = self._advect(q, x, y, t, u, v)
        q_s = torch.maximum(self.get_qs(p, T).detach(), torch.full_like(p, 1e-6))
        delta = ((omega < 0) & (q >= q_s)).to(p.dtype).detach()
        R = (1 + 0.608 * q) * R_d
        Fv = (((L * R - c_p * R_v * T) / (c_p * R_v + T * T + L * L * q_s)) * q_s * T).detach()
        lhs = -omega * delta * Fv / (p + 1e-6) + q_adv
        return loss(lhs, torch.zeros_like(lhs).float()).float() * factor

    def gas_equation(self, p, T, rio, q, loss, factor=1e-5, R_d=287):
        return loss(p, rio * (1 + 0.608 * q) * R_d * T).float() * factor

    def inverse_norm(self, u, v, P, T, q, rio, obs_norm_cfg, with_clip=False):
        """:232-262 -- like the reference, clipping follows self.with_clip and never applies to u, v."""
        out = []
        for k, (val, name) in enumerate(zip((u, v, P, T, q, rio), OBS_ORDER)):
            c = obs_norm_cfg[name]
            if c['use_norm']:
                nf = c['norm_factor']
                if c['norm_type'].lower() == 'min_max':                 # :242-249 (unused by the shipped config)
                    val = val * (nf[1] - nf[0]) + nf[0]
                    if len(nf) != 2:
                        val = val ** 2 + nf[2]
                else:
                    val = val * nf[1] + nf[0]
                if k >= 2 and self.with_clip:
                    val = torch.clip(val, c['bound'][0], c['bound'][1])
            out.append(val)
        return tuple(out)

    def calc_rio(self, p, T, q, R_d=287):
        return ((1 + 0.608 * q) * R_d * T / p).detach()

    def encoding_coord(self, x, y, t, pred_t_span):
        x = x / self.dx / (self.lon_size - 1)
        y = y / self.dy / (self.lat_size - 1)
        t = t / pred_t_span
        pts = torch.stack([x, y, t], dim=1) if x.dim() == 1 else torch.cat([x, y, t], dim=1)
        return self.pe(pts)

    # ------------------------------------------------------------------ fused HIP path
    def _check_pde_criterion(self, criterion):
        """The PDE criterion (`builder_loss(**train_cfg.losses.pde_loss)`, :384; every equation calls it as loss(residual, 0), :104 ... :179) as the
        fused residual kernel's (kind, beta, reduce_sum).  What the reference's losses/builder.py can build for it is implemented: MSELoss (cfg:137),
        L1Loss -- reduction "mean" or "sum" --, WeightSmoothL1Loss(beta); given as a module or as the config's dict."""
        from ..losses import WeightSmoothL1Loss
        red = {'mean': False, 'sum': True}
        if isinstance(criterion, dict):
            name = criterion.get('name', 'MSELoss')
            extra = set(criterion) - {'name'}
            if name in ('MSELoss', 'L1Loss') and extra <= {'reduction'} and criterion.get('reduction', 'mean') in red:
                return (L.CRIT_MSE if name == 'MSELoss' else L.CRIT_L1), 0.0, red[criterion.get('reduction', 'mean')]
            if name == 'WeightSmoothL1Loss' and extra <= {'beta'} and float(criterion.get('beta', 0.1)) > 0.0:
                return L.CRIT_SMOOTH_L1, float(criterion.get('beta', 0.1)), False
        elif isinstance(criterion, (nn.MSELoss, nn.L1Loss)) and criterion.reduction in red:
            return (L.CRIT_MSE if isinstance(criterion, nn.MSELoss) else L.CRIT_L1), 0.0, red[criterion.reduction]
        elif isinstance(criterion, WeightSmoothL1Loss) and criterion.beta > 0:
            return L.CRIT_SMOOTH_L1, float(criterion.beta), False
        elif isinstance(criterion, nn.SmoothL1Loss) and criterion.reduction in red and criterion.beta > 0:
            return L.CRIT_SMOOTH_L1, float(criterion.beta), red[criterion.reduction]
        raise NotImplementedError('the fused residual kernel implements the PDE criteria of the reference\'s loss builder -- nn.MSELoss (cfg:137), nn.L1Loss, '
                                  'WeightSmoothL1Loss(beta > 0), reduction "mean" or "sum"; got %r' % (criterion,))

    def pde_loss_terms(self, x, y, t, f, field_data, input_data, forecast_h, loss_factor=None, use_cache=False, with_total=False, criterion=None, *,
                       point_weights=None, causal=None):
        """The six scaled residual losses as a [6] tensor (motion_u, motion_v, continuous, energy, vapor, gas).  point_weights [N] or [N, 1]: constant
        per-point weights (importance weights, a region's down-weighting, a 0/1 mask; the mean stays over all N points); causal: a
        causal.CausalWeights, causal time weights over the points' t (point_path.pde_losses)."""
        cfg = self.point_config(loss_factor, criterion)
        heads, evec, statics = self.physics_net.field_weights(field_data, forecast_h, use_cache=use_cache)
        return pde_losses(cfg, x, y, t, f, input_data, heads, evec, statics, with_total=with_total, point_weights=point_weights, causal=causal)

    def place_one_batch(self, x, y, t, f, field_data, input_data, forecast_h, criterion, loss_factor, global_step, local_rank, device,
                        summary=None, prefix='inter', log_step=100, use_cache=False, *, point_weights=None, causal=None):
        """:271-320.  Same arguments and return value; the fields, the Jacobian, the residuals and their backward run in HIP.  point_weights, causal:
        as pde_loss_terms."""
        f, x, y, t = f.to(device), x.to(device), y.to(device), t.to(device)
        # train_loss = mu + mv + en + co + va + ga in the reference's order of additions (:301), formed inside the residual kernel
        terms, train_loss = self.pde_loss_terms(x, y, t, f, field_data, input_data, forecast_h, loss_factor, use_cache=use_cache,
                                                with_total=True, criterion=criterion, point_weights=point_weights, causal=causal)
        if summary is not None and global_step % log_step == 1 and local_rank == 0:
            names = ('montion_u_loss', 'montion_v_loss', 'continous_loss', 'energy_loss', 'vapor_loss', 'gas_loss')
            vals = terms.detach().cpu().tolist()
            summary.add_scalar('%s/total_loss' % prefix, float(train_loss.detach()), global_step)
            for n_, v_ in zip(names, vals):
                summary.add_scalar('%s/%s' % (prefix, n_), v_, global_step)
            print('%s:' % prefix + ','.join('%s:%f' % (n_, v_) for n_, v_ in zip(names, vals)))
        return train_loss.float()

    def place_lead_batch(self, x, y, t, f, field_data, input_data, forecast_h, criterion, loss_factor, reduction='mean'):
        """BASELINE configs[2]: B field samples (e.g. the 61 forecast leads, physics_dataset.py:173-174) in ONE step.  x, y, t, f: [B, N];
        field_data [B, 159, 2405]; input_data [B, N, 6]; forecast_h [B, 1, 1].  Equals place_one_batch applied to every sample
        (:271-320), the B totals averaged ('mean') or added ('sum'); the encoder runs once over all B samples and the point kernels
        field after field.  Returns (loss, terms [B, 6])."""
        cfg = self.point_config(loss_factor, criterion)
        heads, evec, statics = self.physics_net.field_weights(field_data, forecast_h)
        B = field_data.shape[0]
        heads, evec = heads.reshape(B, 256, -1), evec.reshape(B, 6, 256)
        terms, totals = pde_losses_batch(cfg, x, y, t, f, input_data, heads, evec, statics)
        loss = totals.sum() if reduction == 'sum' else totals.mean()
        return loss.float(), terms

    def data_loss(self, x, y, t, field_data, input_data, labels, forecast_h, margin_factor=None, beta=0.1, use_cache=False):
        """Data ("margin") loss of the step body (:464-474): mean SmoothL1(beta) over [N,6] times margin_factor."""
        self.point_config()
        if margin_factor is None:
            margin_factor = self.train_cfg['losses']['loss_factor']['margin_factor']
        fields = self.physics_net.forward_xyt(field_data, x, y, t, input_data, forecast_h, use_cache=use_cache)
        return smooth_l1_data_loss(torch.cat(fields, dim=1), labels, beta=beta, factor=1.0).float() * margin_factor

    def fields_at(self, x, y, t, field_data, input_data, forecast_h, use_cache=False):
        """The six [N,1] normalised fields (u, v, P, T, q, rho) at raw coordinates, differentiable w.r.t. the weights and w.r.t. x, y, t up to
        the order a second-order residual needs (PhysicsNet.forward_coords).  The reference's own composition trains on it unchanged:
        fields_at -> inverse_norm -> the *_equation methods with their gradient() calls -> loss.backward(); so does a residual of one's own,
        e.g. u_xx = gradient(gradient(u, x), x)."""
        self.point_config()
        return self.physics_net.forward_coords(field_data, x, y, t, input_data, forecast_h, use_cache=use_cache)

    @torch.no_grad()
    def predict_grid(self, field_data, x, y, t, input_data, forecast_h, with_clip=False, use_cache=False):
        """Full-grid evaluation of the visualisation branch (:536-591): the six fields at all lon*lat nodes, given in the
        reference's node order (x outer, y inner; e.g. CollocationSampler.full_grid), de-normalised (the reference switches
        the clip off there, :533) and scattered into maps [6, lat, lon] (u, v, P, T, q, rho) on the device."""
        cfg = self.point_config()
        n = self.lon_size * self.lat_size
        if x.numel() != n:
            raise ValueError('predict_grid needs all %d x %d nodes (got %d points)' % (self.lon_size, self.lat_size, x.numel()))
        heads, evec, statics = self.physics_net.field_weights(field_data, forecast_h, use_cache=use_cache)
        out_n = point_fields(cfg, input_data, heads, evec, statics, x=x, y=y, t=t)
        return grid_maps(cfg, out_n, self.lon_size, self.lat_size, with_clip)

    # ------------------------------------------------------------------ inference at stations and on lattices
    INFER_BUDGET_BYTES = 256 << 20      # per-point buffers of one chunk of a lattice evaluation (the packed weights and the output maps come on top)
    FIELD_POINT_BYTES = 4 * (4 + 6 + 6)                 # x, y, t, f | coord_data | out_n
    RESIDUAL_POINT_BYTES = 4 * (4 + 6 + 6 + 18 + 6)     # ... | Jacobian | residual rows
    DIAG_POINT_BYTES = 4 * (4 + 6 + 6 + 18)             # ... | Jacobian (the products go straight into the output maps)

    @staticmethod
    def chunk_size(n_points, chunk_points=None, point_bytes=FIELD_POINT_BYTES, prec=L.PREC_BF16X2):
        """Points per chunk of a lattice evaluation: a multiple of the point kernels' padding unit (dpn_sizes: 128 points), so that a chunked and an
        unchunked run form identical tiles; a given size is rounded down to it (and up to one unit), the default is what INFER_BUDGET_BYTES of
        per-point buffers hold.  A lattice that is smaller is one chunk."""
        unit = point_sizes(1, prec)[0]
        want = InterfacePhysics._within_budget(point_bytes) if chunk_points is None else int(chunk_points)
        if want < 1:
            raise ValueError('chunk_points must be positive, got %r' % (chunk_points,))
        chunk = max(unit, want // unit * unit)
        return int(n_points) if chunk >= n_points else chunk

    @staticmethod
    def _within_budget(item_bytes):
        """How many items of item_bytes each INFER_BUDGET_BYTES holds: the rule of chunk_size and lead_batch_size."""
        return InterfacePhysics.INFER_BUDGET_BYTES // int(item_bytes)

    def _inference_weights(self, field_data, forecast_h, n_chunk):
        """encode_field, field_weights and the weight packing, once per call (the field cache is not consulted and not written)."""
        require_gpu(field_data, 'field_data', 'inference')
        cfg = self.point_config()
        heads, evec, statics = self.physics_net.field_weights(field_data, forecast_h, use_cache=False)
        return PackedField(cfg, heads, evec, statics, n_chunk)

    def _station_inputs(self, sampler, x_idx, y_idx, hours, lonlat):
        x, y, t, cd, f = (sampler.at_lonlat if lonlat else sampler.at_positions)(x_idx, y_idx, hours)
        return x, y, t, cd, f.reshape(-1)

    @torch.no_grad()
    def predict_points(self, field_data, sampler, x_idx, y_idx, hours, forecast_h, with_clip=False, lonlat=False):
        """The six physical fields [N, 6] (u, v, P, T, q, rho) at N stations: positions in fine-grid index units (lonlat: degrees east / north)
        and hours, all fractional (CollocationSampler.at_positions / at_lonlat interpolate the coarse cube there)."""
        x, y, t, cd, _ = self._station_inputs(sampler, x_idx, y_idx, hours, lonlat)
        rows = torch.empty((x.shape[0], 6), dtype=torch.float32, device=x.device)
        self._inference_weights(field_data, forecast_h, x.shape[0]).fields(x, y, t, cd, with_clip, rows=rows)
        return rows

    def _lattice_chunks(self, sampler, lattice, chunk):
        """(first, n, x, y, t, f, coord_data) for the chunks of a lattice; the five buffers are allocated once and reused."""
        bufs = point_buffers(chunk, sampler.cube.device)
        for first, n in _chunks(lattice.n_points, chunk):
            yield (first, n) + sampler.sample_at(n, lattice=lattice, first=first, out=bufs)

    @torch.no_grad()
    def predict_lattice(self, field_data, sampler, lattice, forecast_h, with_clip=False, chunk_points=None):
        """The six physical fields on a lattice (CollocationSampler.lattice) as maps [nt, 6, ny, nx].  The encoder, the hyper-network heads and the
        weight packing run once; the lattice is then walked in chunks (chunk_size) of dpn_sample_at -> fields-only forward -> dpn_fields_out, every
        chunk writing its places of the one preallocated output.  NaN where the lattice leaves the coarse cube."""
        chunk = self.chunk_size(lattice.n_points, chunk_points, self.FIELD_POINT_BYTES, self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk)
        maps = torch.empty((lattice.nt, 6, lattice.ny, lattice.nx), dtype=torch.float32, device=field_data.device)
        for first, n, x, y, t, _, cd in self._lattice_chunks(sampler, lattice, chunk):
            field.fields(x, y, t, cd, with_clip, maps=maps, lattice=lattice, first=first)
        return maps

    def _residual_factors(self, residual_factors, device):
        if not residual_factors:
            return None
        lf = self.train_cfg['losses']['loss_factor'] if residual_factors is True else residual_factors
        return torch.tensor([float(lf[k]) for k in LOSS_ORDER], dtype=torch.float64).float().to(device)

    @torch.no_grad()
    def residuals_at(self, field_data, sampler, x_idx, y_idx, hours, forecast_h, lonlat=False, residual_factors=False):
        """Where the network's output violates its equations: the six signed residuals lhs - rhs [N, 6] (motion-u, motion-v, continuity, energy,
        vapour, gas) at N stations, de-normalised and clipped as the training loss does it (self.with_clip).  loss_factor_i * mean(res_i ** 2) is the
        MSE loss term of the same points.  residual_factors: True multiplies column i by the configuration's loss factor, a dict by its own."""
        x, y, t, cd, f = self._station_inputs(sampler, x_idx, y_idx, hours, lonlat)
        n = x.shape[0]
        field = self._inference_weights(field_data, forecast_h, n)
        res = torch.empty((n, 6), dtype=torch.float32, device=x.device)
        field.residuals(x, y, t, f, cd, res)
        fac = self._residual_factors(residual_factors, res.device)
        return res if fac is None else res * fac

    @torch.no_grad()
    def residual_lattice(self, field_data, sampler, lattice, forecast_h, residual_factors=False, chunk_points=None):
        """residuals_at on a lattice, as maps [nt, 6, ny, nx]; chunked as predict_lattice is."""
        chunk = self.chunk_size(lattice.n_points, chunk_points, self.RESIDUAL_POINT_BYTES, self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk)
        rows = torch.empty((lattice.n_points, 6), dtype=torch.float32, device=field_data.device)
        for first, n, x, y, t, f, cd in self._lattice_chunks(sampler, lattice, chunk):
            field.residuals(x, y, t, f, cd, rows[first:first + n])
        fac = self._residual_factors(residual_factors, rows.device)
        if fac is not None:
            rows *= fac
        return rows.view(lattice.nt, lattice.ny, lattice.nx, 6).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def diagnostics_at(self, field_data, sampler, x_idx, y_idx, hours, forecast_h, products, with_clip=False, lonlat=False):
        """Derived diagnostics [N, P] at N stations (positions as predict_points takes them): `products`, a sequence of names of
        deepphysinet_amd.diagnostics.PRODUCTS -- the 18 derivatives du_dx .. drho_dt of the physical fields with respect to x (m), y (m), t (s),
        vorticity, abs_vorticity, divergence, omega (Dp/Dt), t_advection, q_advection, q_flux_divergence, speed, rel_humidity, deformation --, formed
        on the device from the Jacobian the forward kernel computes (dpn_diagnostics_out).  Evaluated without the clip, as predict_points is by
        default; with_clip applies the training clip of P, T, q, rho (a clipped variable has zero derivatives where it is clipped)."""
        ids = product_ids(products)
        x, y, t, cd, f = self._station_inputs(sampler, x_idx, y_idx, hours, lonlat)
        rows = torch.empty((x.shape[0], len(ids)), dtype=torch.float32, device=x.device)
        self._inference_weights(field_data, forecast_h, x.shape[0]).diagnostics(x, y, t, f, cd, ids, with_clip, rows=rows)
        return rows

    @torch.no_grad()
    def diagnostic_lattice(self, field_data, sampler, lattice, forecast_h, products, with_clip=False, chunk_points=None):
        """diagnostics_at on a lattice, as maps [nt, P, ny, nx]; chunked as predict_lattice is (every chunk writes its places of the one output).  NaN
        where the lattice leaves the coarse cube."""
        ids = product_ids(products)
        chunk = self.chunk_size(lattice.n_points, chunk_points, self.DIAG_POINT_BYTES, self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk)
        maps = torch.empty((lattice.nt, len(ids), lattice.ny, lattice.nx), dtype=torch.float32, device=field_data.device)
        for first, n, x, y, t, f, cd in self._lattice_chunks(sampler, lattice, chunk):
            field.diagnostics(x, y, t, f, cd, ids, with_clip, maps=maps, lattice=lattice, first=first)
        return maps

    # ------------------------------------------------------------------ ensemble statistics over field samples
    ENS_POINT_BYTES = DIAG_POINT_BYTES                  # a chunk's per-point buffers, as diagnostics (the state of ALL points stays resident, on top)
    _ENS_SHARED = ('lat_size', 'lon_size', 'dx', 'dy', 'input_time_step', 'input_time_step_nums')
    _ENS_SHARED_LONLAT = ('begin_lon', 'begin_lat', 'out_res_deg')

    def _ensemble_request(self, members, products, thresholds, lonlat=False):
        """The checks of ensemble_at / ensemble_lattice, all before the first launch: names (KeyError), thresholds (ValueError), at least one member,
        and members that share the fine grid and the hour window (lonlat: origin and resolution too).  -> members (a list), names, an EnsembleState
        factory, the (name, value) list of the thresholds."""
        names = list(products)
        ids = ensemble_ids(names)
        thr_col, thr_val = check_thresholds(names, thresholds)
        members = list(members)
        if not members:
            raise ValueError('ensemble: no members (a sequence of dicts with field_data, forecast_h and sampler)')
        self._check_shared_window(members, lonlat, 'ensemble member', 'members')
        dev = members[0]['sampler'].cube.device
        return members, names, (lambda n_total: EnsembleState(n_total, ids, thr_col, thr_val, dev)), [(names[c], v) for c, v in zip(thr_col, thr_val)]

    def _check_shared_window(self, members, lonlat, word, plural):
        """ValueError unless the samplers of `members` share the fine grid and the hour window (lonlat: origin and resolution too) with the first."""
        ref = members[0]['sampler'].cfg
        for m, mem in enumerate(members[1:], start=1):
            for name in self._ENS_SHARED + (self._ENS_SHARED_LONLAT if lonlat else ()):
                if getattr(mem['sampler'].cfg, name) != getattr(ref, name):
                    raise ValueError('%s %d: %s = %r, but %s 0 has %r; the %s must share the fine grid and the hour window'
                                     % (word, m, name, getattr(mem['sampler'].cfg, name), word.split()[-1], getattr(ref, name), plural))

    @staticmethod
    def _ensemble_outputs(shape_of, P, E, dev):
        out = {k: torch.empty(shape_of(P), dtype=torch.float32, device=dev) for k in ('mean', 'spread', 'min', 'max')}
        out['count'] = torch.empty(shape_of(P), dtype=torch.int32, device=dev)
        out['prob'] = torch.empty(shape_of(E), dtype=torch.float32, device=dev) if E else None
        return out

    @torch.no_grad()
    def ensemble_at(self, members, x_idx, y_idx, hours, products, thresholds=None, with_clip=False, lonlat=False):
        """Statistics over the members of an ensemble at N stations.  members: a sequence of dicts with field_data, forecast_h and sampler (what
        _inference_samples yields) -- the forecasts of different initialisation dates that cover one window (a lagged ensemble), or perturbed members --
        which share the fine grid and the hour window; positions and hours (as predict_points takes them) are read in each member's own window.
        products: names of deepphysinet_amd.ensemble.ENSEMBLE_PRODUCTS (the diagnostics and u, v, p, T, q, rho); thresholds: dict name -> value(s), at
        most 16 in all.  The members are the outer loop: encoder, heads and packing run once per member and one PackedField is alive at a time; each
        member's values are folded into a state that stays on the device (dpn_ensemble_accumulate: Welford in fp64), and after the last member one
        dpn_ensemble_finish per chunk writes the results, with no host synchronisation in between.  A member whose value is not finite at a point
        is skipped there, in that column.  Returns {'names', 'mean', 'spread' (sample standard deviation, NaN below two members), 'min', 'max' [N, P]
        fp32, 'count' [N, P] int32, 'thresholds' [(name, value)], 'prob' [N, E] (the share of the counted members above the threshold, strictly; None
        without thresholds)}, on the device."""
        members, names, new_state, thr = self._ensemble_request(members, products, thresholds, lonlat)
        s0 = members[0]['sampler']
        if lonlat:
            x_idx, y_idx = s0.lonlat_to_index(x_idx, y_idx)
        xr, yr, tr = s0.check_positions(x_idx, y_idx, hours)
        N, dev = xr.shape[0], s0.cube.device
        chunk = self.chunk_size(N, None, self.ENS_POINT_BYTES, self.precision)
        state = new_state(N)
        bufs = point_buffers(chunk, dev)
        for mem in members:
            field = self._inference_weights(mem['field_data'].to(dev), mem['forecast_h'].to(dev), chunk)
            for first, n in _chunks(N, chunk):
                x, y, t, f, cd = mem['sampler'].sample_at(n, xr[first:first + n], yr[first:first + n], tr[first:first + n], out=bufs)
                field.ensemble_accumulate(x, y, t, f, cd, state, first, with_clip)
            del field                                                     # before the next member packs its own
        out = self._ensemble_outputs(lambda c: (N, c), len(names), len(thr), dev)
        for first, n in _chunks(N, chunk):
            state.finish(first, n, rows={k: None if v is None else v[first:first + n] for k, v in out.items()})
        return dict(out, names=names, thresholds=thr)

    @torch.no_grad()
    def ensemble_lattice(self, members, lattice, products, thresholds=None, with_clip=False, chunk_points=None):
        """ensemble_at on a lattice: the statistics as maps [nt, P, ny, nx] and the probabilities as maps [nt, E, ny, nx]; chunked as predict_lattice is,
        inside the loop over the members (per point the members arrive in their given order whatever the chunking, so chunk_points does not change a
        bit of the result).  count is 0 and the rest NaN where the lattice leaves every member's coarse cube."""
        members, names, new_state, thr = self._ensemble_request(members, products, thresholds)
        total, dev = lattice.n_points, members[0]['sampler'].cube.device
        chunk = self.chunk_size(total, chunk_points, self.ENS_POINT_BYTES, self.precision)
        state = new_state(total)
        for mem in members:
            field = self._inference_weights(mem['field_data'].to(dev), mem['forecast_h'].to(dev), chunk)
            for first, n, x, y, t, f, cd in self._lattice_chunks(mem['sampler'], lattice, chunk):
                field.ensemble_accumulate(x, y, t, f, cd, state, first, with_clip)
            del field                                                     # before the next member packs its own
        out = self._ensemble_outputs(lambda c: (lattice.nt, c, lattice.ny, lattice.nx), len(names), len(thr), dev)
        for first, n in _chunks(total, chunk):
            state.finish(first, n, maps=out, lattice=lattice)
        return dict(out, names=names, thresholds=thr)

    # ------------------------------------------------------------------ verification against observations
    @staticmethod
    def _verify_request(products, thresholds, by_names=None, members=None, word='verify'):
        """What a request of verify_at (word 'verify') or verify_ensemble_at ('verify_ensemble') names: the products (KeyError), at most 16 of
        them, the thresholds, the grouping names -- none may be a key of the result's own -- and 1 <= M <= 64 where `members` is given
        (ValueError).  -> names, ids, (thr_col, thr_val, thr_side)."""
        names = list(products)
        ids = VF.verify_ids(names)
        if len(ids) > VF.MAX_COLUMNS:
            raise ValueError('%s: %d products; at most %d in one request' % (word, len(ids), VF.MAX_COLUMNS))
        thr = VF.check_thresholds(names, thresholds)
        for name in by_names or ():
            if name in (VF.RESULT_KEYS if word == 'verify' else PV.RESULT_KEYS):
                raise ValueError("%s: a grouping may not be called %r (the result's own keys)" % (word, name))
        if members is not None:
            PV.check_members(members)
        return names, ids, thr

    def _verify_setup(self, word, sources, cases, x_idx, y_idx, hours, lonlat, by, n_columns, new_state):
        """What verify_at and verify_ensemble_at (`word`) do between the request and the first launch.  sources: every dict with a sampler, in
        order (the cases, or the members of all cases) -- they must share the window; positions and hours are converted (lonlat) and checked in the
        first one's; every case's obs must be an fp32 [N, n_columns] tensor on the device; every grouping of `by` becomes a pool plan; then the
        chunk size, the state (new_state(N, device)), the chunk's buffers and the plans on the device, so that nothing waits for the device between
        the launches.  -> xr, yr, tr, device, state, plans, bufs, chunk."""
        self._check_shared_window(sources, lonlat, *(('verification case', 'cases') if word == 'verify' else ('ensemble member', 'members')))
        s0 = sources[0]['sampler']
        if lonlat:
            x_idx, y_idx = s0.lonlat_to_index(x_idx, y_idx)
        xr, yr, tr = s0.check_positions(x_idx, y_idx, hours)
        N, dev = xr.shape[0], s0.cube.device
        for c, case in enumerate(cases):
            obs = case.get('obs')
            if not torch.is_tensor(obs) or tuple(obs.shape) != (N, n_columns) or obs.dtype != torch.float32 or obs.device != dev:
                raise ValueError('verification case %d: obs must be an fp32 tensor [%d, %d] on %s, got %s'
                                 % (c, N, n_columns, dev, (tuple(obs.shape), obs.dtype, obs.device) if torch.is_tensor(obs) else type(obs).__name__))
        plans = {}
        for name, groups in dict(by or {}).items():
            g = groups.detach().cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)
            if g.shape != (N,):
                raise ValueError('%s: by[%r] must hold one group id per point, [%d], got %s' % (word, name, N, g.shape))
            plans[name] = VF.pool_plan(g)
        chunk = self.chunk_size(N, None, self.FIELD_POINT_BYTES + 4 * n_columns, self.precision)
        state = new_state(N, dev)
        bufs = point_buffers(chunk, dev)
        return xr, yr, tr, dev, state, {name: state.upload_plan(*plan) for name, plan in plans.items()}, bufs, chunk

    @staticmethod
    def _verify_result(state, plans, names, thr, members=None):
        """The dict both calls return: names, the thresholds as (name, 'above' | 'below', value), members where given, the table of the points
        (`finish`) and, in `plans`' order, that of every grouping (`pool`, then `finish`)."""
        side = {VF.ABOVE: 'above', VF.BELOW: 'below'}
        out = dict(names=names, thresholds=[(names[c], side[s], v) for c, v, s in zip(*thr)])
        if members is not None:
            out['members'] = members
        out['point'] = state.finish()
        for name, plan in plans.items():
            out[name] = state.pool(plan=plan).finish()
        return out

    @torch.no_grad()
    def verify_at(self, cases, x_idx, y_idx, hours, products, thresholds=None, by=None, with_clip=False, lonlat=False):
        """Was the forecast right: scores of the model and of its baseline against reports at N points (station, hour), over a sequence of cases.
        cases: dicts with field_data, forecast_h and sampler (what _inference_samples yields) -- one forecast date each, sharing the fine grid and the
        hour window -- plus obs, an [N, P] fp32 tensor on the device of the reports in physical units, NaN where there is none; positions and hours as
        predict_points takes them, read in each case's own window.  products: names of deepphysinet_amd.verification.VERIFY_PRODUCTS (u, v, p, T, q,
        rho, speed, rel_humidity), at most 16; thresholds: dict name -> value(s) (the event is strictly above) or name -> ('below', value(s)), at most
        16 in all; by: dict name -> int group id >= 0 per point [N], e.g. {'station': .., 'hour': .., 'all': zeros}.
        The baseline is the interpolated coarse forecast the network was built to improve on: the sampler's coord_data at the point, de-normalised
        by the same code as the forecast (with_clip applies to both, never to the reports).  The cases are the outer loop: encoder, heads and
        packing run once per case and one PackedField is alive at a time; every case is folded into a state that stays on the device
        (dpn_verify_accumulate: fp64, no atomics), the groupings are pooled from it in one fixed order (dpn_verify_pool) and dpn_verify_finish writes
        the scores, with no host synchronisation before the results.  A (point, column) of a case counts only where forecast, baseline and report are
        all finite.  Returns {'names', 'thresholds' [(name, 'above' | 'below', value)], 'point': table} and, for every entry of `by`, name: table;
        a table is a dict of count [G, P] int32, bias, mae, rmse, max_abs_error, corr, base_bias, base_mae, base_rmse, skill (1 - MSE / MSE of the
        baseline) [G, P] fp32 and pod, far, csi, fbias, ets, base_pod .. base_ets [G, E] fp32 (None without thresholds), on the device; NaN where a
        score is not defined.  KeyError: an unknown name; ValueError: a bad threshold, no case, an obs that is not [N, P] fp32 on the device, a
        negative group id, more than 16 columns -- all before the first launch."""
        names, ids, thr = self._verify_request(products, thresholds, by)
        cases = list(cases)
        if not cases:
            raise ValueError('verify: no cases (a sequence of dicts with field_data, forecast_h, sampler and obs)')
        xr, yr, tr, dev, state, plans, bufs, chunk = self._verify_setup('verify', cases, cases, x_idx, y_idx, hours, lonlat, by, len(ids),
                                                                        lambda N, dev: VerifyState(N, ids, *thr, dev))
        for case in cases:
            field = self._inference_weights(case['field_data'].to(dev), case['forecast_h'].to(dev), chunk)
            obs = case['obs'].contiguous()
            for first, n in _chunks(state.n_total, chunk):
                x, y, t, _, cd = case['sampler'].sample_at(n, xr[first:first + n], yr[first:first + n], tr[first:first + n], out=bufs)
                field.verify_accumulate(x, y, t, cd, obs[first:first + n], state, first, with_clip)
            del field                                                     # before the next case packs its own
        return self._verify_result(state, plans, names, thr)

    # ------------------------------------------------------------------ probabilistic verification of ensembles
    @torch.no_grad()
    def verify_ensemble_at(self, cases, x_idx, y_idx, hours, products, thresholds=None, by=None, with_clip=False, lonlat=False):
        """Were the ensemble's probabilities any good: probabilistic scores of the model's ensemble and of the baseline's against reports at N points
        (station, hour), over a sequence of cases.  cases: dicts with members -- a sequence of M dicts with field_data, forecast_h and sampler, as
        ensemble_at takes them; every case has the same M, 1..64 -- and obs, an [N, P] fp32 tensor on the device as verify_at takes it (NaN: no
        report).  All samplers share the fine grid and the hour window.  products, thresholds, by, with_clip, lonlat as verify_at takes them; the
        baseline ensemble is the members' interpolated coarse forecasts (coord_data).
        The cases are the outer loop and the members the inner: encoder, heads and packing run once per member and one PackedField is alive at a
        time; a member's forecast and baseline values are staged into two planes that stay on the device (dpn_pverify_stage), after a case's last
        member one dpn_pverify_case per chunk folds the case into the resident state (fp64, no atomics), after the last case the groupings are
        pooled in one fixed order (dpn_pverify_pool) and dpn_pverify_finish writes the scores, with no host synchronisation before the results.  A
        (point, column) of a case counts only where all M forecast values, all M baseline values and the report are finite.
        Returns {'names', 'thresholds' [(name, 'above' | 'below', value)], 'members': M, 'point': table} and, for every entry of `by`, name: table;
        a table is a dict by deepphysinet_amd.prob_verification.OUT_FIELDS: count [G, P] int32; crps, fair_crps, bias and rmse of the ensemble
        mean, spread, spread_skill, their base_ forms, crpss, fair_crpss [G, P] fp32; rank_hist, base_rank_hist [G, P, M + 1] int32; brier,
        reliability, resolution, bss, roc_area, their base_ forms and uncertainty [G, E] fp32; rel_n, rel_o, base_rel_n, base_rel_o [G, E, M + 1]
        int32 (the threshold entries None without thresholds), on the device; NaN where a score is not defined.  KeyError: an unknown name;
        ValueError: a bad threshold, no case, unequal member counts, more than 64 members, an obs that is not [N, P] fp32 on the device, a negative
        group id, a grouping named like a result key, a state past 2^31 - 1 elements -- all before the first launch."""
        names, ids, thr = self._verify_request(products, thresholds, by, word='verify_ensemble')
        cases = [dict(case, members=list(case['members'])) for case in cases]
        if not cases:
            raise ValueError('verify_ensemble: no cases (a sequence of dicts with members and obs)')
        M = len(cases[0]['members'])
        for c, case in enumerate(cases):
            if len(case['members']) != M:
                raise ValueError('verify_ensemble: case %d has %d members, case 0 has %d; all cases must have the same number' % (c, len(case['members']), M))
        if M < 1:
            raise ValueError('verify_ensemble: a case has no members (a sequence of dicts with field_data, forecast_h and sampler)')
        PV.check_members(M)
        members = [mem for case in cases for mem in case['members']]
        xr, yr, tr, dev, state, plans, bufs, chunk = self._verify_setup(    # (the state refuses an array past 2^31 - 1 elements)
            'verify_ensemble', members, cases, x_idx, y_idx, hours, lonlat, by, len(ids), lambda N, dev: ProbVerifyState(N, ids, *thr, M, dev))
        for case in cases:
            for m, mem in enumerate(case['members']):
                field = self._inference_weights(mem['field_data'].to(dev), mem['forecast_h'].to(dev), chunk)
                for first, n in _chunks(state.n_total, chunk):
                    x, y, t, _, cd = mem['sampler'].sample_at(n, xr[first:first + n], yr[first:first + n], tr[first:first + n], out=bufs)
                    field.pverify_stage(x, y, t, cd, state, m, first, with_clip)
                del field                                                 # before the next member packs its own
            obs = case['obs'].contiguous()
            for first, n in _chunks(state.n_total, chunk):
                state.case(obs[first:first + n], first)
        return self._verify_result(state, plans, names, thr, members=M)

    # ------------------------------------------------------------------ neighbourhood verification on lattices
    @torch.no_grad()
    def verify_lattice(self, cases, lattice, products, thresholds, scales, with_clip=False, chunk_points=None):
        """From which spatial scale on is the forecast useful: the fractions skill score (FSS) of the model and of its baseline against gridded
        analyses on a lattice, over square windows of growing width, over a sequence of cases.  cases: dicts with field_data, forecast_h and
        sampler (what _inference_samples yields) -- one forecast date each, sharing the fine grid and the hour window -- plus analysis, an
        [nt, P, ny, nx] fp32 tensor on the device of the analysis at the lattice's own nodes (the layout of diagnostic_lattice's output), in
        physical units, NaN where there is none.  products: names of deepphysinet_amd.verification.VERIFY_PRODUCTS; thresholds: as verify_at
        takes them, at least one (the FSS is a score of events); scales: the window widths in lattice nodes, odd, strictly ascending, at most 8
        (neighbourhood.check_scales), e.g. (1, 3, 5, 9, 17, 33).
        The baseline is the interpolated coarse forecast (coord_data), de-normalised by the same code as the forecast; with_clip applies to
        both, never to the analysis.  The cases are the outer loop and one PackedField is alive at a time: a case's lattice is walked in chunks
        (dpn_sample_at -> fields-only forward -> dpn_nbhd_stage, which writes the event masks), then dpn_nbhd_fold builds an integer
        summed-area table per (hour, threshold), forms the window fractions of every scale from four corners per node and folds their squares
        in one fixed order, without atomics, into a state that stays on the device; dpn_nbhd_finish writes the tables.  No host
        synchronisation before the result; chunk_points changes no bit of it.  A node of a column counts only where forecast, baseline and
        analysis are all finite; a window is clamped to the lattice and its fractions are taken over its valid nodes.
        Returns {'names', 'thresholds' [(name, 'above' | 'below', value)], 'scales' (the widths), 'hour': table, 'all': table}; a table is a
        dict by deepphysinet_amd.neighbourhood.OUT_FIELDS: fss, base_fss fp32 and windows int64 [nt, E, K]; freq_f, freq_b, freq_o, fbias,
        base_fbias, useful (0.5 + freq_o / 2) fp32, count int64 and skilful_scale, base_skilful_scale int32 (the first scale index whose FSS
        reaches useful, or -1) [nt, E] -- in 'all' without the leading nt --, on the device; NaN where a score is not defined.  KeyError: an
        unknown name; ValueError: bad thresholds or none, bad scales, no case, an analysis that is not [nt, P, ny, nx] fp32 on the device,
        windows that are not shared, a lattice of 2^31 nodes or more -- all before the first launch."""
        names, ids, thr = self._verify_request(products, thresholds, word='verify_lattice')
        if not thr[0]:
            raise ValueError('verify_lattice: no threshold; the fractions skill score is a score of events (thresholds={name: value, ..})')
        radius = NB.check_scales(scales)
        cases = list(cases)
        if not cases:
            raise ValueError('verify_lattice: no cases (a sequence of dicts with field_data, forecast_h, sampler and analysis)')
        self._check_shared_window(cases, False, 'verification case', 'cases')
        dev = cases[0]['sampler'].cube.device
        shape = (int(lattice.nt), len(ids), int(lattice.ny), int(lattice.nx))
        for c, case in enumerate(cases):
            an = case.get('analysis')
            if not torch.is_tensor(an) or tuple(an.shape) != shape or an.dtype != torch.float32 or an.device != dev:
                raise ValueError('verification case %d: analysis must be an fp32 tensor %s on %s, got %s'
                                 % (c, list(shape), dev, (tuple(an.shape), an.dtype, an.device) if torch.is_tensor(an) else type(an).__name__))
        if lattice.n_points >= 2 ** 31:
            raise ValueError('verify_lattice: a lattice of %d nodes; fewer than 2^31' % lattice.n_points)
        chunk = self.chunk_size(lattice.n_points, chunk_points, self.FIELD_POINT_BYTES, self.precision)
        state = NbhdState(lattice, ids, *thr, radius, dev, self.INFER_BUDGET_BYTES)
        for case in cases:
            field = self._inference_weights(case['field_data'].to(dev), case['forecast_h'].to(dev), chunk)
            analysis = case['analysis'].contiguous()
            for first, n, x, y, t, _, cd in self._lattice_chunks(case['sampler'], lattice, chunk):
                field.nbhd_stage(x, y, t, cd, analysis, state, first, with_clip)
            del field                                                     # before the next case packs its own
            state.fold()
        side = {VF.ABOVE: 'above', VF.BELOW: 'below'}
        return dict(state.finish(), names=names, thresholds=[(names[c], side[s], v) for c, v, s in zip(*thr)], scales=[2 * r + 1 for r in radius])

    # ------------------------------------------------------------------ regional statistics in space
    @staticmethod
    def _region_request(products, thresholds):
        """The name and threshold checks of regional_at / regional_lattice: names (KeyError), at most 16 of them and the thresholds (ValueError)."""
        names = list(products)
        ids = ensemble_ids(names)
        if len(ids) > RG.MAX_COLUMNS:
            raise ValueError('regions: %d products; at most %d in one request' % (len(ids), RG.MAX_COLUMNS))
        thr_col, thr_val = check_thresholds(names, thresholds)
        return names, ids, thr_col, thr_val

    def _region_run(self, field_data, sampler, forecast_h, plan, xs, ys, hours, request, with_clip, chunk_points):
        """The walk of a regional request: the flat, time-major point list (positions xs, ys [n_sel] of the plan's entries at every hour of `hours`
        [nt], fp64 on the host) goes through the station route of dpn_sample_at chunk by chunk -- sample_at -> forward -> region_accumulate --, then
        one finish.  Encoder, heads and packing run once; nothing is read back in between."""
        require_gpu(field_data, 'field_data', 'regions')
        names, ids, thr_col, thr_val = request
        nt, n_sel, dev = hours.size, plan.n_sel, field_data.device
        state = RegionState(plan, nt, ids, thr_col, thr_val, dev)              # (refuses nt * n_sel >= 2^31)
        total = nt * n_sel
        chunk = self.chunk_size(total, chunk_points, self.DIAG_POINT_BYTES, self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk)
        xr, yr = (torch.from_numpy(np.ascontiguousarray(np.tile(v, nt), dtype=np.float64)).to(dev) for v in (xs, ys))
        tr = torch.from_numpy(np.ascontiguousarray(np.repeat(hours, n_sel), dtype=np.float64)).to(dev)
        bufs = point_buffers(chunk, dev)
        for first, n in _chunks(total, chunk):
            x, y, t, f, cd = sampler.sample_at(n, xr[first:first + n], yr[first:first + n], tr[first:first + n], out=bufs)
            field.region_accumulate(x, y, t, f, cd, state, first, with_clip)
        out = state.finish()
        order = torch.from_numpy(plan.order).to(dev)
        for key in ('where_min', 'where_max'):                                # entries of the plan -> station indices or (ix, iy); -1 stays
            j = out[key].long()
            at = torch.where(j >= 0, order[j.clamp(min=0)], j)
            if plan.shape is not None:
                nx = plan.shape[1]
                at = torch.where((j >= 0).unsqueeze(-1), torch.stack([at % nx, at // nx], dim=-1), j.unsqueeze(-1))
            out[key] = at
        return dict(out, names=names, thresholds=[(names[c], v) for c, v in zip(thr_col, thr_val)])

    @torch.no_grad()
    def regional_lattice(self, field_data, sampler, lattice, forecast_h, regions, products, weights=None, thresholds=None, with_clip=False,
                         chunk_points=None):
        """A number per area and hour: the area-weighted mean of a product over a catchment, the peak wind inside a polygon and where it sits, the
        share of a district below freezing -- without building the maps.  regions: an int label plane [ny, nx] over the lattice's positions (-1: in
        no region, ids 0..R - 1) or a list of R boolean masks, which may overlap.  products: up to 16 names of
        deepphysinet_amd.ensemble.ENSEMBLE_PRODUCTS; weights: None (ones), 'area' (float32(cos(latitude of the row))) or a non-negative finite plane
        [ny, nx]; thresholds: dict name -> value(s), at most 16 in all.  Only the positions inside a region are evaluated, at every time node of the
        lattice; a request without a product that reads the Jacobian runs the fields-only forward.  The reduction is deterministic (no atomics, one
        fixed order: deepphysinet_amd.regions), so two runs and any chunk_points give the same bits.  Returns {'names', 'thresholds' [(name, value)],
        'mean' (the weighted mean), 'total' (sum of weight * value), 'weight' (the counted weight), 'min', 'max' [nt, R, P] fp32, 'count' [nt, R, P]
        int32, 'where_min', 'where_max' [nt, R, P, 2] int64 (ix, iy on the lattice; -1 without a counted point), 'frac' [nt, R, E] fp32 (the share
        of the counted weight strictly above the threshold; None without thresholds)}, on the device.  A point whose value is not finite (outside
        the coarse cube) or whose weight is 0 is skipped in that column; a cell without a counted point has count 0, weight 0 and NaN elsewhere.
        KeyError: an unknown name; ValueError: labels that are not (ny, nx), a bad weight or threshold -- all before the first launch."""
        request = self._region_request(products, thresholds)
        shape = (lattice.ny, lattice.nx)
        X_, Y_, T_ = lattice.positions()
        plane = lattice.ny * lattice.nx
        lat_deg = RG.row_latitudes(sampler.cfg, Y_[:plane:lattice.nx]) if isinstance(weights, str) else None
        if torch.is_tensor(weights):
            weights = weights.detach().cpu().numpy()
        plan = RG.region_plan(regions, weights, lat_deg)
        if plan.shape != shape:
            raise ValueError('regional_lattice: the regions are planes of shape %s, the lattice is (ny, nx) = %s' % (plan.shape, shape))
        return self._region_run(field_data, sampler, forecast_h, plan, X_[:plane][plan.order], Y_[:plane][plan.order], T_[::plane], request, with_clip,
                                chunk_points)

    @torch.no_grad()
    def regional_at(self, field_data, sampler, x_idx, y_idx, hours, forecast_h, groups, products, weights=None, thresholds=None, with_clip=False,
                    lonlat=False):
        """regional_lattice for N stations in groups: positions as predict_points takes them (lonlat: degrees east / north), hours the 1-d list of
        the nt time nodes shared by all stations, groups [N] int (-1: in none), weights None, 'area' (the cosine of the station's latitude) or [N].
        The outputs are [nt, R, P] ([nt, R, E]), where_min / where_max [nt, R, P] the station index."""
        request = self._region_request(products, thresholds)
        hours = np.ascontiguousarray(np.atleast_1d(hours.detach().cpu().numpy() if torch.is_tensor(hours) else np.asarray(hours)), dtype=np.float64)
        if hours.ndim != 1 or hours.size == 0:
            raise ValueError('regional_at: hours is the 1-d list of the time nodes shared by all stations, got shape %s' % (hours.shape,))
        x_idx, y_idx = (np.atleast_1d(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)).reshape(-1) for v in (x_idx, y_idx))
        if lonlat:
            x_idx, y_idx = sampler.lonlat_to_index(x_idx, y_idx)
        if x_idx.size != y_idx.size:
            raise ValueError('regional_at: x_idx and y_idx must have the same length')
        if torch.is_tensor(weights):
            weights = weights.detach().cpu().numpy()
        plan = RG.region_plan(groups=groups, weights=weights, lat_deg=RG.row_latitudes(sampler.cfg, y_idx) if isinstance(weights, str) else None)
        if plan.n_candidates != x_idx.size:
            raise ValueError('regional_at: %d groups for %d stations' % (plan.n_candidates, x_idx.size))
        for h in (hours.min(), hours.max()):                                  # every station at the first and the last hour: IndexError outside
            sampler.check_positions(x_idx, y_idx, np.full(x_idx.size, h))
        return self._region_run(field_data, sampler, forecast_h, plan, x_idx[plan.order], y_idx[plan.order], hours, request, with_clip, None)

    @torch.no_grad()
    def trajectories(self, field_data, sampler, x_idx, y_idx, hours, forecast_h, duration_hours, step_hours, method='rk4', lonlat=False,
                     with_fields=False, with_clip=False, chunk_points=None):
        """Where the air at N places comes from or goes to: parcels started at positions x_idx, y_idx (fine-grid index units; lonlat: degrees east /
        north) at the one hour `hours`, carried by the network's own wind (u, v of predict_points, evaluated at the parcel, never interpolated from
        a grid) for K = round(|duration_hours| / |step_hours|) steps of `method` ('euler', 'midpoint', 'rk4': deepphysinet_amd.trajectory.METHODS).
        duration_hours < 0 integrates backward in time (back-trajectories).  The encoder, the heads and the weight packing run once and the start
        positions are checked on the host once; every stage is then two launches (the fields-only forward and dpn_traj_stage), with no host
        synchronisation until the results are read.  More parcels than chunk_size allows (chunk_points) are integrated chunk by chunk.
        Returns {'positions' [K + 1, N, 2] fp64 (index units, or degrees when lonlat), 'hours' [K + 1], 'status' [N] int32 (0 alive, 1 left the fine
        grid, 2 left the hour window, 3 non-finite wind), 'steps_done' [N] int32, and with_fields 'fields' [K + 1, N, 6]: the six fields along the
        path (with_clip as predict_points takes it)}, on the device but `hours`.  A parcel that leaves keeps NaN from that step on.
        The integration stays inside ONE field sample's hour window [0, input_time_step * input_time_step_nums]: all parcels share the clock, and
        when it reaches either end of the window every parcel still alive stops there with status 2.  `hours` must be one scalar (ValueError);
        fields at arbitrary (position, hour) sets are predict_points'."""
        require_gpu(field_data, 'field_data', 'trajectories')
        if lonlat:
            x_idx, y_idx = sampler.lonlat_to_index(x_idx, y_idx)
        xs, ys, t0, h, K, stages, inv_wsum = check_request(x_idx, y_idx, hours, duration_hours, step_hours, method, domain_of(sampler._s))
        N, dev = xs.size, field_data.device
        chunk = self.chunk_size(N, chunk_points, self.FIELD_POINT_BYTES + 48 + (K + 1) * (16 + (24 if with_fields else 0)), self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk)
        positions = torch.empty((K + 1, N, 2), dtype=torch.float64, device=dev)
        fields = torch.empty((K + 1, N, 6), dtype=torch.float32, device=dev) if with_fields else None
        status, steps_done = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
        hrs = [t0]
        for _ in range(K):
            hrs.append(hrs[-1] + h)                    # the running sum: hour k is bit for bit the hour the k-th path point's forward was sampled at
        xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
        for first, n in _chunks(N, chunk):
            parcels = ParcelState(sampler, xd[first:first + n].contiguous(), yd[first:first + n].contiguous(), t0, K + 1)
            rows = torch.empty((K + 1, n, 6), dtype=torch.float32, device=dev) if with_fields else None
            for k in range(K):
                for stage in stages:
                    field.trajectory_stage(sampler, parcels, stage, hrs[k], h, inv_wsum, k, rows, with_clip)
            if with_fields:                            # the last path point's fields: one more forward, nothing moves
                field.trajectory_stage(sampler, parcels, stages[0], hrs[K], h, inv_wsum, K, rows, with_clip, record_only=True)
                fields[:, first:first + n] = rows
            positions[:, first:first + n] = parcels.path
            status[first:first + n], steps_done[first:first + n] = parcels.status, parcels.steps_done
        if lonlat:
            c = sampler.cfg
            positions = torch.stack([c.begin_lon + positions[..., 0] * c.out_res_deg, c.begin_lat + positions[..., 1] * c.out_res_deg], dim=-1)
        out = {'positions': positions, 'hours': torch.tensor(hrs, dtype=torch.float64), 'status': status, 'steps_done': steps_done}
        if with_fields:
            out['fields'] = fields
        return out

    # ------------------------------------------------------------------ time-window products: window extremes and means, threshold spells
    def _window_request(self, check_request, word, field_data, sampler, columns, window, scan_hours, refine):
        """The request of a time-window product, checked against the sample's own window of hours before anything is launched."""
        require_gpu(field_data, 'field_data', word)
        c = sampler.cfg
        return check_request(columns, window, scan_hours, refine, c.input_time_step * c.input_time_step_nums)

    @staticmethod
    def _window_stations(sampler, x_idx, y_idx, lonlat, t0):
        """Stations as predict_points takes them -> checked fp64 xr, yr on the device (t0: the hour they are first sampled at)."""
        x_idx, y_idx = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64) for v in (x_idx, y_idx))
        if lonlat:
            x_idx, y_idx = sampler.lonlat_to_index(x_idx, y_idx)
        return sampler.check_positions(x_idx, y_idx, np.full(np.shape(np.atleast_1d(x_idx)), t0))[:2]

    @staticmethod
    def _window_lattice(lattice, device):
        """The positions of a lattice with nt == 1 -> fp64 xd, yd on the device, in point order."""
        xs, ys, _ = lattice.positions()
        return tuple(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device) for v in (xs, ys))

    def _window_run(self, State, field_data, sampler, xd, yd, req, forecast_h, with_clip, chunk_points):
        """The walk of a time-window product over N points xd, yd (fp64 on the device, checked), State its state class (ExtremeState, SpellState):
        per chunk the K + 1 scan nodes, the state's rounds and its finish; the results of all points as [C, N] tensors."""
        N = xd.shape[0]
        chunk = self.chunk_size(N, chunk_points, State.point_bytes(req), self.precision)
        field = self._inference_weights(field_data, forecast_h, chunk * max(State.probe_rows(req), 1))
        out = None
        for first, n in _chunks(N, chunk):
            state = State(sampler, xd[first:first + n], yd[first:first + n], req)
            for k in range(req.K + 1):
                field.window_scan(sampler, state, k, with_clip)
            for rnd in range(State.rounds(req)):
                field.window_refine(sampler, state, rnd, with_clip)
            state.finish()
            results = state.results()
            if out is None:                            # the outputs take their types from the state's own arrays
                out = {key: torch.empty((v.shape[0], N), dtype=v.dtype, device=v.device) for key, v in results.items()}
            for key, v in results.items():
                out[key][:, first:first + n] = v
        return out

    @torch.no_grad()
    def extremes_at(self, field_data, sampler, x_idx, y_idx, window, forecast_h, columns, scan_hours=1.0, refine=10, with_clip=False, lonlat=False,
                    chunk_points=None):
        """Daily maximum and minimum, peak wind and their hours, window means: per station and column of `columns` ('T:max', 'T:min', 'speed:max',
        'q:mean', ...: product one of u, v, p, T, q, rho, speed; sense max, min or mean; deepphysinet_amd.extremes) the extreme of the product over the
        hours window = (t0, t1) of the sample's window and the hour it occurs at, found on the network's own d/dt: a scan of the K + 1 nodes t0 +
        k * scan_hours (one fields-only forward each), then `refine` + 1 forwards with the Jacobian at one probe per station and max / min column --
        round 0 probes the best scan node and chooses the side, every later round halves the bracket, so the hour is resolved to scan_hours /
        2**refine.  The mean is the trapezoid sum of the scan nodes in fp64.  Positions as predict_points takes them (lonlat: degrees east / north).
        The encoder, the heads and the weight packing run once; more stations than chunk_size allows (chunk_points) go chunk by chunk; no host
        synchronisation until the results are read.  Returns {'names', 'value' [N, C] fp32, 'hour' [N, C] fp64 (NaN for a mean), 'lo', 'hi' [N, C] fp64
        (the final bracket), 'status' [N, C] int32: 0 an interior extreme (or a mean), 1 a scan value was not finite (everything NaN), 2 a probe was
        not finite (the best so far stands), 3 / 4 the extreme sits at the window's start / end with the slope pointing outward}, on the device.  The
        result is never worse than the best scan node, and a (value, hour) pair always comes from one evaluation."""
        req = self._window_request(X.check_request, 'extremes', field_data, sampler, columns, window, scan_hours, refine)
        xr, yr = self._window_stations(sampler, x_idx, y_idx, lonlat, req.t0)
        out = self._window_run(ExtremeState, field_data, sampler, xr, yr, req, forecast_h, with_clip, chunk_points)
        return dict({k: v.t().contiguous() for k, v in out.items()}, names=req.names)

    @torch.no_grad()
    def extreme_lattice(self, field_data, sampler, lattice, window, forecast_h, columns, scan_hours=1.0, refine=10, with_clip=False, chunk_points=None):
        """extremes_at on the positions of a lattice with nt == 1 (ValueError otherwise: `window` gives the times), as maps [C, ny, nx]: 'value',
        'hour', 'lo', 'hi', 'status'.  Points outside the coarse cube have status 1 and NaN everywhere."""
        req = self._window_request(X.check_request, 'extremes', field_data, sampler, columns, window, scan_hours, refine)
        if lattice.nt != 1:
            raise ValueError('extreme_lattice: the lattice gives the positions (nt == 1, got %d); `window` gives the times' % lattice.nt)
        xd, yd = self._window_lattice(lattice, field_data.device)
        out = self._window_run(ExtremeState, field_data, sampler, xd, yd, req, forecast_h, with_clip, chunk_points)
        return dict({k: v.view(len(req.ids), lattice.ny, lattice.nx) for k, v in out.items()}, names=req.names)

    @torch.no_grad()
    def spells_at(self, field_data, sampler, x_idx, y_idx, window, forecast_h, columns, scan_hours=1.0, refine=10, with_clip=False, lonlat=False,
                  chunk_points=None):
        """Frost hours, hours of strong wind, the hour a station first drops below freezing: per station and column of `columns`
        ('T:below:273.15', 'speed:above:15', ...: product one of u, v, p, T, q, rho, speed; side above or below; the threshold in the product's unit;
        deepphysinet_amd.spells) how long the product is strictly above (below) the threshold over the hours window = (t0, t1) of the sample's
        window, from when until when.  A scan of the K + 1 nodes t0 + k * scan_hours (one fields-only forward each) brackets the first entry and
        the last exit; `refine` fields-only forwards at two probes per station and column halve both brackets on the sign of value - threshold, so
        'first' and 'last' are resolved to scan_hours / 2**refine.  Positions as predict_points takes them (lonlat: degrees east / north).  The
        encoder, the heads and the weight packing run once; more stations than chunk_size allows (chunk_points) go chunk by chunk; no host
        synchronisation until the results are read.  Returns {'names', 'hours' [N, C] fp64 (the time in: the scan's piecewise-linear estimate with
        its first entry and last exit replaced by the refined ones), 'first', 'last' [N, C] fp64 (hours at which the network was evaluated and found
        in; t0 / t1 when the spell holds there; NaN when it never does), 'first_lo', 'last_hi' [N, C] fp64 (the other ends of the brackets: found
        out), 'excess' [N, C] fp64 (the integral of the margin over the time in, unit x hours -- degree-hours; the scan's clipped trapezoid, which
        the refinement does not change), 'crossings' [N, C] int32 (entries and exits the scan saw), 'status' [N, C] int32, bits: 1 a scan value was
        not finite (everything NaN), 2 a probe was not finite (the brackets stand), 4 never in, 8 in at t0, 16 in at t1}, on the device.  A spell
        shorter than a scan step that lies between two nodes is not seen."""
        req = self._window_request(SP.check_request, 'spells', field_data, sampler, columns, window, scan_hours, refine)
        xr, yr = self._window_stations(sampler, x_idx, y_idx, lonlat, req.t0)
        out = self._window_run(SpellState, field_data, sampler, xr, yr, req, forecast_h, with_clip, chunk_points)
        return dict({k: v.t().contiguous() for k, v in out.items()}, names=req.names)

    @torch.no_grad()
    def spell_lattice(self, field_data, sampler, lattice, window, forecast_h, columns, scan_hours=1.0, refine=10, with_clip=False, chunk_points=None):
        """spells_at on the positions of a lattice with nt == 1 (ValueError otherwise: `window` gives the times), as maps [C, ny, nx]: 'hours',
        'first', 'last', 'first_lo', 'last_hi', 'excess', 'crossings', 'status'.  Points outside the coarse cube have status 1 and NaN everywhere."""
        req = self._window_request(SP.check_request, 'spells', field_data, sampler, columns, window, scan_hours, refine)
        if lattice.nt != 1:
            raise ValueError('spell_lattice: the lattice gives the positions (nt == 1, got %d); `window` gives the times' % lattice.nt)
        xd, yd = self._window_lattice(lattice, field_data.device)
        out = self._window_run(SpellState, field_data, sampler, xd, yd, req, forecast_h, with_clip, chunk_points)
        return dict({k: v.view(len(req.ids), lattice.ny, lattice.nx) for k, v in out.items()}, names=req.names)

    @torch.no_grad()
    def adaptive_interior(self, batch: dict, sampler, pool_factor=8, k=1.0, c=1.0):
        """The batch with its interior collocation points redrawn where the current network violates its equations most (residual-based adaptive
        sampling, Wu et al. 2023): pool_factor * n uniform interior draws of `sampler` are scored by the six residuals of the batch's field
        (score = sum_e loss_factor_e * res_e ** 2, the summand of the PDE loss), and n of them are drawn with probability ~ score ** k /
        mean(score ** k) + c (CollocationSampler.get_inter_data_adaptive).  Returns a copy of the dict with inter_x, inter_y, inter_t, inter_f,
        inter_data replaced (same shapes and dtypes); everything else is the same objects.  One encoder forward and one fields + Jacobian pass over
        the pool, without autograd; parameters, .grad, optimiser state and the field cache are left alone."""
        require_gpu(batch['field_data'], 'field_data', 'adaptive_interior')
        n = int(batch['inter_x'].shape[0])
        pool = int(pool_factor) * n
        if pool < n or pool < 1:
            raise ValueError('adaptive_interior: pool_factor must be an integer >= 1, got %r' % (pool_factor,))
        lf = self.train_cfg['losses']['loss_factor']
        meta_out = self.physics_net.encode_field(batch['field_data'], batch['forecast_h'])
        heads, evec, statics = self.physics_net.field_weights(batch['field_data'], batch['forecast_h'], meta_out=meta_out)
        field = PackedField(self.point_config(lf), heads, evec, statics, pool)
        x, y, t, cd, f = sampler.get_inter_data_adaptive(field, [float(lf[name]) for name in LOSS_ORDER], n=n, pool=pool, k=k, c=c)
        self.physics_net.clear_field_cache()
        out = dict(batch)
        for key, v in (('inter_x', x), ('inter_y', y), ('inter_t', t), ('inter_f', f), ('inter_data', cd)):
            out[key] = v.reshape(batch[key].shape).to(batch[key].dtype)
        return out

    def _adaptive_option(self, kwargs):
        """The loops' `adaptive_interior` option (keyword, or train_cfg['train_data']['adaptive_interior']): None (off), or a dict of pool_factor, k, c,
        every (refresh on every every-th step, counted from the first) and sampler."""
        def build(opt):
            opt = dict({'pool_factor': 8, 'k': 1.0, 'c': 1.0, 'every': 1, 'sampler': None}, **opt)
            if int(opt['every']) < 1:
                raise ValueError('adaptive_interior: every must be >= 1, got %r' % (opt['every'],))
            return opt
        return _loop_option(kwargs, self.train_cfg, 'adaptive_interior', 'train_data', ('pool_factor', 'k', 'c', 'every', 'sampler'), True, None, build)

    def _causal_option(self, kwargs):
        """The loops' `causal_weights` option (keyword, or train_cfg['losses']['causal_weights']): None (off), or a dict of eps, bins, relative ->
        a causal.CausalWeights."""
        def build(opt):
            if 'eps' not in opt:
                raise ValueError('causal_weights: eps is required')
            return CausalWeights(**opt)
        return _loop_option(kwargs, self.train_cfg, 'causal_weights', 'losses', ('eps', 'bins', 'relative'), False, CausalWeights, build)

    def _ema_option(self, kwargs):
        """The loops' `ema_weights` option (keyword, or train_cfg['optimizer']['ema_weights']): None (off), a decay, or a dict of decay, warmup ->
        dict(decay, warmup) for FusedClipAdam(ema_decay, ema_warmup)."""
        opt = kwargs.get('ema_weights', (self.train_cfg.get('optimizer') or {}).get('ema_weights'))
        if isinstance(opt, (int, float)) and not isinstance(opt, bool):
            opt = {'decay': opt}
        def build(o):
            if 'decay' not in o:
                raise ValueError('ema_weights: decay is required')
            return dict(decay=float(o['decay']), warmup=bool(o.get('warmup', True)))
        return _loop_option({'ema_weights': opt}, {}, 'ema_weights', 'optimizer', ('decay', 'warmup'), False, None, build)

    def _step_guard_option(self, kwargs):
        """The loops' `step_guard` option (keyword, or train_cfg['optimizer']['step_guard']): None (off), True (skip a step whose gradient norm is
        non-finite), a guard.StepGuard, or a dict of spike_factor, spike_decay, spike_warmup, spike_patience (the spike rule on top) -> a
        guard.StepGuard with the C ABI's argument rules."""
        return _loop_option(kwargs, self.train_cfg, 'step_guard', 'optimizer', StepGuard.KEYS, True, StepGuard, lambda opt: StepGuard(**opt))

    LBFGS_KEYS = ('start_epoch', 'history_size', 'max_iter', 'max_eval', 'lr', 'tolerance_grad', 'tolerance_change', 'history')

    def _lbfgs_option(self, kwargs):
        """The loops' `lbfgs` option (keyword, or train_cfg['optimizer']['lbfgs']): None (off), or a dict of start_epoch (required) and FusedLBFGS's
        history_size, max_iter, max_eval, lr, tolerance_grad, tolerance_change, history.  From start_epoch on the loop refines with L-BFGS."""
        def build(opt):
            if 'start_epoch' not in opt:
                raise ValueError('lbfgs: start_epoch is required')
            if isinstance(opt['start_epoch'], bool) or int(opt['start_epoch']) != opt['start_epoch'] or int(opt['start_epoch']) < 0:
                raise ValueError('lbfgs: start_epoch must be an integer >= 0, got %r' % (opt['start_epoch'],))
            return dict(opt, start_epoch=int(opt['start_epoch']))
        return _loop_option(kwargs, self.train_cfg, 'lbfgs', 'optimizer', self.LBFGS_KEYS, False, None, build)

    def _lbfgs_refusals(self, kwargs, dist_mode):
        """ValueError before training starts for what cannot run beside the L-BFGS phase."""
        if dist_mode:
            raise ValueError('lbfgs: run_train_interface_dist refuses the option: the line search decides on the loss, which would have to be reduced '
                             'across the ranks as well as the gradients (data-parallel L-BFGS is not implemented)')
        section = {'adaptive_interior': 'train_data', 'causal_weights': 'losses', 'balance_losses': 'losses', 'ema_weights': 'optimizer',
                   'step_guard': 'optimizer'}
        on = [n for n, sec in section.items() if kwargs.get(n, (self.train_cfg.get(sec) or {}).get(n)) not in (None, False)]
        if on:
            raise ValueError('lbfgs together with %s: with adaptive_interior, causal_weights or balance_losses the objective changes between the '
                             'evaluations of one line search; ema_weights and step_guard live in the fused clip + Adam launch' % ' and '.join(on))

    @staticmethod
    def _step_guard_log(optimizer, prev):
        """At a log step (the loop synchronises there anyway): the guard's counters as the extra keys of the log line and the metrics row, and the
        (calls, skipped) pair the next log step compares with.  RuntimeError when every call since the previous log step was skipped: training is
        stuck, and a run that silently does nothing is worse than one that stops."""
        st = optimizer.guard_stats()
        calls, skipped = int(optimizer.step_count), st['skipped_nonfinite'] + st['skipped_spike']
        if calls > prev[0] and skipped - prev[1] == calls - prev[0]:
            raise RuntimeError('step_guard: all %d optimiser steps since the previous log step were skipped (in total skipped_nonfinite %d, '
                               'skipped_spike %d of %d calls; last norm %r, running norm %r): training is stuck'
                               % (calls - prev[0], st['skipped_nonfinite'], st['skipped_spike'], calls, st['last'], st['running']))
        row = {'skipped_nonfinite': st['skipped_nonfinite'], 'skipped_spike': st['skipped_spike'], 'running_norm': st['running']}
        return row, (calls, skipped)

    def _lead_batch_option(self, kwargs):
        """The loops' `lead_batch` option (keyword, or train_cfg['train_data']['lead_batch']): samples per optimiser step, 1 when unset.  Refused
        together with a causal_weights / balance_losses option that is set (implemented for one sample per step): the loops ask at their start."""
        k = kwargs.get('lead_batch', (self.train_cfg.get('train_data') or {}).get('lead_batch'))
        k = 1 if k is None else int(k)
        if k < 1:
            raise ValueError('lead_batch must be >= 1, got %d' % k)
        on = [n for n in ('causal_weights', 'balance_losses') if kwargs.get(n, (self.train_cfg.get('losses') or {}).get(n)) not in (None, False)]
        if k > 1 and on:
            raise NotImplementedError('lead_batch=%d with %s: causal time weights and loss balancing are implemented for one sample per optimiser step '
                                      '(training_step), not for lead batches' % (k, ' and '.join(on)))
        return k

    def _balance_option(self, kwargs):
        """The loops' `balance_losses` option (keyword, or train_cfg['losses']['balance_losses']): None (off), a balance.LossBalance, or a dict of
        every, momentum, groups, lam_min, lam_max -> a balance.LossBalance."""
        return _loop_option(kwargs, self.train_cfg, 'balance_losses', 'losses', ('every', 'momentum', 'groups', 'lam_min', 'lam_max'), True, LossBalance,
                            lambda opt: LossBalance(**opt))

    def _balance_state(self, balance, device):
        """loss_balance_state for this option on this device: kept while the groups stay the same (a checkpoint's weights arrive on the host),
        otherwise lambda = 1 and the counter at 0."""
        st = self.loss_balance_state
        if st is None or st['groups'] != balance.groups or st['lam'].numel() != balance.n_terms:
            st = {'groups': balance.groups, 'lam': torch.ones(balance.n_terms, dtype=torch.float32, device=device), 'step': 0, 'diag': None}
        if st['lam'].device != device:
            st['lam'] = st['lam'].to(device)
        self.loss_balance_state = st
        return st

    def _balance_refresh(self, balance, state, b, lf, inter_w, causal, grad_sync):
        """One refresh of the balancing weights: for each term k the sum of squares of d (group k's terms) / d (all parameters), unweighted by lambda,
        then dpn_balance_update.  Every term takes a forward and a backward pass of its own: the encoder stack's backward node hands the token
        convolution's gradient on through state that one backward pass consumes, so one graph is not walked K times.  The
        gradients come back from torch.autograd.grad inside grad_arena.detached(): none reaches a .grad or the optimiser's flat buffer."""
        net = self.physics_net
        params = [p for p in net.parameters() if p.requires_grad]
        shapes = [p.shape for p in params]
        K, dev = balance.n_terms, b['field_data'].device
        sumsq = torch.empty(K, dtype=torch.float64, device=dev)
        cfg = self.point_config(lf)
        n_inter, pts = self._eval_inputs(b, True)
        with grad_arena.detached():
            for k in range(K):
                net.clear_field_cache()
                meta_out = net.encode_field(b['field_data'], b['forecast_h'])
                heads, evec, statics = net.field_weights(b['field_data'], b['forecast_h'], meta_out=meta_out)
                it, _, mt, _, data = step_losses(cfg, n_inter, *pts, b['margin_data'], heads, evec, statics, beta=0.1, margin_factor=lf['margin_factor'],
                                                 inter_weights=inter_w, causal=causal)
                if k == 0:
                    term = data
                elif balance.groups == 'equations':
                    term = it[k - 1] + mt[k - 1]
                else:
                    term = (it, mt)[k - 1].sum()
                grads = torch.autograd.grad(term, params, allow_unused=True)
                balance_sumsq(grads, shapes, sumsq[k:k + 1])
                del grads, term, it, mt, data, heads, evec, statics, meta_out
        net.clear_field_cache()
        if grad_sync is not None and grad_sync.active():
            # every rank must hold the same lambda: the K sums are averaged over the ranks (one collective of 8 K bytes per refresh)
            import torch.distributed as dist
            from ..distributed import _all_reduce_mean
            _all_reduce_mean(sumsq, dist.get_world_size(grad_sync.group), grad_sync.group, False)
        if state['diag'] is None or state['diag'].device != dev:
            state['diag'] = torch.zeros(3 * K + 2, dtype=torch.float64, device=dev)
        balance_update(sumsq, state['lam'], balance, state['diag'])

    def _balance_log(self, on=True):
        """{'balance_lambda': [K], 'balance_norm': [K]} of the last balanced step (lambda, and the gradient norms n_k of the last refresh), or {}.
        Reads device memory: for log steps, where the loop synchronises anyway."""
        st = self.loss_balance_state
        if not on or st is None or st['step'] == 0 or st['diag'] is None:
            return {}
        K = st['lam'].numel()
        return {'balance_lambda': st['lam'].tolist(), 'balance_norm': st['diag'][:K].tolist()}

    def _balance_log_text(self, on=True):
        row = self._balance_log(on)
        if not row:
            return ''
        return ' lambda %s grad_norm %s' % (' '.join('%.4g' % v for v in row['balance_lambda']), ' '.join('%.4g' % v for v in row['balance_norm']))

    def _adaptive_sampler(self, opt, batch, kwargs):
        """The sampler that draws the pool: the option's own, the batch's 'sampler' entry, or the sample source's `.sampler` attribute."""
        for s in (opt.get('sampler'), batch.get('sampler'), getattr(self._train_source(kwargs), 'sampler', None)):
            if s is not None:
                return s
        raise RuntimeError("adaptive_interior needs the CollocationSampler that draws the pool: give it as adaptive_interior['sampler'], as the batch's "
                           "'sampler' entry, or as the `.sampler` attribute of the samples source (SyntheticSamples has one)")

    def training_step(self, batch: dict, optimizer, with_pde=True, max_norm=2.5e7, grad_sync=None, *, causal=None, balance=None):
        """One step body (:443-515 / :990-1065): data loss on the margin points, PDE losses on interior and margin points,
        backward, clip_grad_norm_(2.5e7), optimizer step.  `batch` holds device tensors: field_data [1,159,2405],
        forecast_h [1,1,1], margin_{x,y,t,f} [N,1], margin_data [N,6], margin_input_data [N,6], inter_{x,y,t,f} [M,1],
        inter_data [M,6].  The encoder runs once (the reference runs it three times on identical inputs).
        causal (a causal.CausalWeights; with the PDE losses only): causal time weights on the interior and on the margin PDE losses, each group with
        bins and weights of its own; `self.last_causal` then holds {'inter': diag, 'margin': diag} as device tensors (no synchronisation here), and
        None after a step without the option.  An optional batch entry inter_w [M] or [M, 1]: constant weights of the interior points' PDE losses.
        The data loss is never weighted.
        balance (a balance.LossBalance; with the PDE losses and device tensors only): the step minimises sum_k lambda_k * (term k) instead of the plain
        sum, lambda in `self.loss_balance_state['lam']` (fp32 [K] on the device, ones at first); on every balance.every-th call, counted from the
        first, lambda is refreshed from the norms of the terms' parameter gradients before the step's own passes (_balance_refresh; `diag` of the
        state: dpn_balance_update's row, a device tensor).  The returned loss is the balanced total, `parts` stay the unweighted three.  A
        data-parallel step with the option takes the plain backward + grad_sync(parameters); grad_sync must then be a
        distributed.GradientAllReduce (TypeError otherwise): the refresh averages the K sums of squares over its process group.  A refresh takes
        at most 4096 trainable parameter tensors (DPN_BALANCE_MAX_TENSORS; a PhysicsNet has 155)."""
        lf = self.train_cfg['losses']['loss_factor']
        self.last_causal = None
        inter_w = batch.get('inter_w') if with_pde else None
        if not with_pde:
            causal = balance = None
        bal_state = self._balance_prepare(balance, batch, grad_sync, lf, inter_w, causal)
        self.physics_net.clear_field_cache()
        fwd = self._step_forward(batch, with_pde, lf, inter_w, causal, keep_embedding=grad_sync is not None)
        if bal_state is not None:
            train_loss = balanced_total(fwd.inter_terms, fwd.margin_terms, fwd.data, bal_state['lam'], balance.groups)      # one launch; its backward: one
        else:
            train_loss = 0
            for v in fwd.parts.values():
                train_loss = train_loss + v
        optimizer.zero_grad()
        if getattr(self, '_seed', None) is None or self._seed.device != train_loss.device:
            self._seed = torch.ones((), dtype=train_loss.dtype, device=train_loss.device)      # persistent backward seed: no fill per step
        buckets = self._can_stage(optimizer, grad_sync, fwd.heads is not None and bal_state is None)
        if buckets is not None:
            # data-parallel step: the backward pass is cut where buckets of gradients are complete (staged_backward) and their all-reduce is queued at
            # once, so it travels under the rest of the backward (what DistributedDataParallel's bucket hooks do in the reference, :903-907, :1056).
            # Statics + heads are ONE all-reduce (the heads' backward is two launches: a collective of its own costs more than the 40 us it could start
            # earlier), encoder + embedding another: the fused stack's weight-gradient launch completes both, any other encoder leaves no x0 to cut at
            back = StagedBackward(buckets, optimizer)
            back.points(train_loss, fwd.heads, fwd.evec, fwd.statics, fwd.meta_out, getattr(self.physics_net.meta_net.model, 'last_embedding', None),
                        self._seed)
            back.heads_cut()
            grad_sync.reduce_bucket(0, 2)
            back.encoder()
            back.embedding()
            grad_sync.reduce_bucket(2, 4)
            grad_sync.wait()
            self.physics_net.clear_field_cache()
        else:
            train_loss.backward(self._seed)
            self.physics_net.clear_field_cache()
            if grad_sync is not None:
                grad_sync(self.physics_net.parameters())
        if isinstance(optimizer, FusedClipAdam):                  # clip + Adam in one HIP pass
            optimizer.max_norm = float(max_norm)
            gnorm = optimizer.step()
        else:
            gnorm = torch.nn.utils.clip_grad_norm_(self.physics_net.parameters(), max_norm=max_norm)
            optimizer.step()
        return train_loss.detach(), {k: v.detach() for k, v in fwd.parts.items()}, gnorm

    def _lead_forward(self, batches, with_pde, what):
        """The forward of one step on B samples (training_step_batch, loss_and_gradients): its checks, the batched encoder pass, the point kernels
        sample after sample.  (terms, sample_parts, totals) as training_step_batch returns them, totals still attached to the graph."""
        batches = list(batches)
        if not batches:
            raise ValueError('%s: no samples' % what)
        if any('inter_w' in b for b in batches):
            raise NotImplementedError('%s: per-point weights (inter_w) are implemented for one sample per step (training_step), not '
                                      'for lead batches' % what)
        shape = lambda b: (b['inter_x'].shape[0] if with_pde else 0, b['margin_x'].shape[0])
        if any(shape(b) != shape(batches[0]) for b in batches[1:]):
            raise ValueError('%s: the samples of one step must have equal point counts, got (interior, margin) = %s'
                             % (what, sorted({shape(b) for b in batches})))
        for b in batches:
            require_gpu(b['field_data'], 'field_data', what)
        lf = self.train_cfg['losses']['loss_factor']
        self.last_causal = None
        B = len(batches)
        net = self.physics_net
        net.clear_field_cache()
        cfg = self.point_config(lf)
        field = torch.cat([b['field_data'] for b in batches], dim=0)
        fh = torch.cat([b['forecast_h'] for b in batches], dim=0)
        meta_out = net.encode_field(field, fh)
        heads, evec, statics = net.field_weights(field, fh, meta_out=meta_out)
        heads, evec = heads.reshape(B, 256, -1), evec.reshape(B, 6, 256)
        inputs = [self._eval_inputs(b, with_pde) for b in batches]
        pts = tuple(torch.stack([p[1][c] for p in inputs], dim=0) for c in range(5))
        labels = torch.stack([b['margin_data'] for b in batches], dim=0)
        if with_pde:
            terms, sample_parts, totals = step_losses_batch(cfg, inputs[0][0], *pts, labels, heads, evec, statics, beta=0.1,
                                                            margin_factor=lf['margin_factor'])
        else:
            totals = data_losses_batch(cfg, pts[0], pts[1], pts[2], pts[4], labels, heads, evec, statics, beta=0.1, margin_factor=lf['margin_factor'])
            terms, sample_parts = None, totals.detach().reshape(B, 1)
        return terms, sample_parts, totals

    def loss_and_gradients(self, batch_or_batches, optimizer, with_pde=True):
        """The forward and the backward of training_step (a batch dict) or of training_step_batch (a list of them), ending BEFORE the optimiser
        call: (loss, parts) with the gradients left in the optimiser's arena (`optimizer.flat_gradients()` for the fused optimisers) -- the closure
        of FusedLBFGS.step.  The same launches in the same order as those steps make without causal weights, balancing and grad_sync, so the loss and
        the gradients are bit for bit theirs.  An `inter_w` entry (single sample) weights the interior points as in training_step."""
        if isinstance(batch_or_batches, (list, tuple)):
            terms, sample_parts, totals = self._lead_forward(batch_or_batches, with_pde, 'loss_and_gradients')
            train_loss = totals.mean()
            means = sample_parts.mean(dim=0)
            parts = {k: means[i] for i, k in enumerate(('margin_loss', 'inter_pde_loss', 'margin_pde_loss')[:means.numel()])}
        else:
            batch = batch_or_batches
            lf = self.train_cfg['losses']['loss_factor']
            self.last_causal = None
            self.physics_net.clear_field_cache()
            fwd = self._step_forward(batch, with_pde, lf, batch.get('inter_w') if with_pde else None, None, keep_embedding=False)
            train_loss = 0
            for v in fwd.parts.values():
                train_loss = train_loss + v
            parts = {k: v.detach() for k, v in fwd.parts.items()}
        optimizer.zero_grad()
        if getattr(self, '_seed', None) is None or self._seed.device != train_loss.device:
            self._seed = torch.ones((), dtype=train_loss.dtype, device=train_loss.device)
        train_loss.backward(self._seed)
        self.physics_net.clear_field_cache()
        if hasattr(optimizer, 'gather_gradients'):        # what autograd summed outside the arena (a lead batch's samples) is copied in, as step() does
            optimizer.gather_gradients()
        return train_loss.detach(), parts

    def training_step_batch(self, batches, optimizer, with_pde=True, max_norm=2.5e7, grad_sync=None):
        """ONE optimiser step on B samples: `batches` is a list of B training_step batch dicts (device tensors) with equal point counts -- for example B
        forecast leads.  The encoder, the hyper-network heads and the weight packing run once for all B (the lead-batch launches); the point kernels
        run sample after sample, each sample's backward right behind its forward (point_path.step_losses_batch).  loss = the mean of the B samples'
        totals, each total training_step's (data + interior PDE) + margin PDE: the mean keeps the gradient scale of a single-sample step, so max_norm
        and the learning rate keep their meaning.  Then backward, grad_sync(parameters) when given (the plain backward, as a balanced
        data-parallel step takes it: there is no staged backward for this step), clip + Adam as training_step ends.  with_pde False: the data loss
        alone (point_path.data_losses_batch).  Returns (loss, parts, gnorm, per_sample): parts = the means over the samples of margin_loss,
        inter_pde_loss, margin_pde_loss; per_sample = {'terms' [B, 2, 6], 'parts' [B, 3], 'totals' [B]} on the device (without the PDE losses terms
        is None, parts [B, 1]); nothing is read back.  Point weights (an `inter_w` entry: NotImplementedError), causal weights and loss balancing are
        implemented for one sample per step only (training_step).  A list of one sample runs the same path with B = 1."""
        net = self.physics_net
        terms, sample_parts, totals = self._lead_forward(batches, with_pde, 'training_step_batch')
        train_loss = totals.mean()
        optimizer.zero_grad()
        if getattr(self, '_seed', None) is None or self._seed.device != train_loss.device:
            self._seed = torch.ones((), dtype=train_loss.dtype, device=train_loss.device)
        train_loss.backward(self._seed)
        net.clear_field_cache()
        if grad_sync is not None:
            grad_sync(net.parameters())
        if isinstance(optimizer, FusedClipAdam):                  # clip + Adam in one HIP pass
            optimizer.max_norm = float(max_norm)
            gnorm = optimizer.step()
        else:
            gnorm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=max_norm)
            optimizer.step()
        means = sample_parts.mean(dim=0)
        parts = {k: means[i] for i, k in enumerate(('margin_loss', 'inter_pde_loss', 'margin_pde_loss')[:means.numel()])}
        return train_loss.detach(), parts, gnorm, {'terms': terms, 'parts': sample_parts, 'totals': totals.detach()}

    @staticmethod
    def _lead_groups(samples, k):
        """The loops' lead_batch grouping: consecutive samples of a stream, k at a time; a group is cut early where the point counts (interior, margin)
        change and at the end of the stream, so a shorter last group is a smaller B.  Yields lists of samples; consumes the stream lazily."""
        k = int(k)
        if k < 1:
            raise ValueError('lead_batch must be >= 1, got %d' % k)
        shape = lambda b: (b['inter_x'].shape[0], b['margin_x'].shape[0])
        group = []
        for smp in samples:
            if group and (len(group) == k or shape(smp) != shape(group[0])):
                yield group
                group = []
            group.append(smp)
        if group:
            yield group

    def _balance_prepare(self, balance, batch, grad_sync, lf, inter_w, causal):
        """training_step's balance option: its checks, the refresh on every balance.every-th call and the counter; the state, or None without."""
        if balance is None:
            return None
        if not isinstance(balance, LossBalance):
            raise TypeError('training_step: balance must be a deepphysinet_amd.balance.LossBalance, got %r' % (balance,))
        if grad_sync is not None and not (hasattr(grad_sync, 'active') and hasattr(grad_sync, 'group')):
            # a plain callable could average the gradients but not the K sums of squares: the ranks' lambda would drift apart unnoticed
            raise TypeError('training_step: balance with grad_sync needs a distributed.GradientAllReduce (its process group carries the average '
                            'of the K sums of squares that keeps lambda equal on every rank), got %r' % (grad_sync,))
        if not batch['field_data'].is_cuda:
            raise ValueError('training_step: balance needs the HIP point path (device tensors); field_data is on %s' % batch['field_data'].device)
        state = self._balance_state(balance, batch['field_data'].device)
        if state['step'] % balance.every == 0:
            self._balance_refresh(balance, state, batch, lf, inter_w, causal, grad_sync)
        state['step'] += 1
        return state

    def _step_forward(self, b, with_pde, lf, inter_w, causal, keep_embedding):
        """training_step's forward: `parts`, the unweighted losses in the order they are added; from the HIP path also inter_terms, margin_terms,
        data, and heads, evec, statics, meta_out, where a staged backward cuts (heads None: the per-op path ran)."""
        out = types.SimpleNamespace(heads=None)
        if with_pde and b['field_data'].is_cuda:
            # one point pass for everything: [interior | margin] points, PDE means per group, SmoothL1 on the margin rows; the margin
            # forward serves both of its losses and all points share one backward (point_path._StepLossFn)
            cfg = self.point_config(lf)
            out.meta_out = self.physics_net.encode_field(b['field_data'], b['forecast_h'], keep_embedding=keep_embedding)
            out.heads, out.evec, out.statics = self.physics_net.field_weights(b['field_data'], b['forecast_h'], meta_out=out.meta_out)
            n_inter, pts = self._eval_inputs(b, True)
            diag = [] if causal is not None else None
            out.inter_terms, inter_total, out.margin_terms, margin_total, out.data = step_losses(
                cfg, n_inter, *pts, b['margin_data'], out.heads, out.evec, out.statics, beta=0.1, margin_factor=lf['margin_factor'],
                inter_weights=inter_w, causal=causal, diag=diag)
            if causal is not None:
                self.last_causal = {'inter': diag[0], 'margin': diag[1]}
            out.parts = {'margin_loss': out.data, 'inter_pde_loss': inter_total.float(), 'margin_pde_loss': margin_total.float()}
            return out
        loss = self.data_loss(b['margin_x'], b['margin_y'], b['margin_t'], b['field_data'], b['margin_input_data'], b['margin_data'],
                              b['forecast_h'], lf['margin_factor'], use_cache=True)
        out.parts = {'margin_loss': loss}
        if with_pde:
            crit, dev = nn.MSELoss(), b['field_data'].device
            out.parts['inter_pde_loss'] = self.place_one_batch(b['inter_x'], b['inter_y'], b['inter_t'], b['inter_f'], b['field_data'], b['inter_data'],
                                                               b['forecast_h'], crit, lf, 0, 0, dev, use_cache=True, point_weights=inter_w, causal=causal)
            out.parts['margin_pde_loss'] = self.place_one_batch(b['margin_x'], b['margin_y'], b['margin_t'], b['margin_f'], b['field_data'],
                                                                b['margin_input_data'], b['forecast_h'], crit, lf, 0, 0, dev, prefix='margin',
                                                                use_cache=True, causal=causal)
        return out

    def _can_stage(self, optimizer, grad_sync, hip_unbalanced):
        """The four gradient buckets if training_step may take the staged backward, else None (the plain backward + grad_sync(parameters)): the HIP
        forward without balancing, an active bucket reducer bound to THIS optimiser, whose flat buffer is laid out in the four buckets of
        gradient_buckets() filtered to the trainable parameters -- a bucket may be empty, with the encoder frozen the last two are (not: an
        optimiser built without `layout`, a reducer of another or no optimiser, an optimiser that holds other parameters than the trainable ones)."""
        if not (hip_unbalanced and grad_sync is not None and hasattr(grad_sync, 'reduce_bucket') and grad_sync.active()
                and isinstance(optimizer, FusedClipAdam)):
            return None
        buckets = [[p for p in b_ if p.requires_grad] for b_ in self.physics_net.gradient_buckets()]      # = PhysicsNet.trainable_buckets()
        ok = (getattr(grad_sync, 'opt', None) is optimizer and len(getattr(optimizer, 'bucket_bounds', ())) == 4
              and getattr(optimizer, 'layout_ids', None) == [[id(p) for p in b_] for b_ in buckets])
        return buckets if ok else None

    # ------------------------------------------------------------------ validation (:518-530, :629-745)
    def variable_errors(self, out_n, labels, with_clip=False):
        """The six per-variable errors of normalised predictions out_n [N, 6] against labels [N, 6] in physical units (:518-530: inverse_norm
        of both sides, nn.MSELoss per variable), from ONE pass over the data (dpn_label_errors): {v: {mse, rmse, mae, bias, max_abs}} for
        v in u, v, p, T, q, rio; `mse` is the reference's margin_<v>_loss.  with_clip applies the clip bounds of P, T, q, rho to both sides."""
        stats = label_errors(self.point_config(), out_n, labels, beta=0.1, with_clip=with_clip)
        return V.metrics_from_stats(V.stats_row(stats[0], out_n.shape[0]))['variables']

    def _eval_inputs(self, b, with_pde):
        """(n_inter, (x, y, t, f, coord_data)) of the step body from a training batch (training_step, eval_step): [interior | margin] rows with
        the PDE losses, the margin rows alone without."""
        flat = lambda v: v.reshape(v.shape[0], -1)
        if not with_pde:
            return 0, tuple(flat(b[k]) for k in ('margin_x', 'margin_y', 'margin_t', 'margin_f', 'margin_input_data'))
        cat = lambda a_, b_: torch.cat([flat(a_), flat(b_)], dim=0)
        return b['inter_x'].shape[0], (cat(b['inter_x'], b['margin_x']), cat(b['inter_y'], b['margin_y']), cat(b['inter_t'], b['margin_t']),
                                       cat(b['inter_f'], b['margin_f']), cat(b['inter_data'], b['margin_input_data']))

    def _validation_dict(self, losses, stats, n_margin, with_pde, forecast_h=None):
        """One sample's result from eval_step's outputs (device tensors; nothing is synchronised here except the statistics' copy to the host)."""
        mf = self.train_cfg['losses']['loss_factor']['margin_factor']
        # the training step's own expression (_StepLossFn.forward / data_loss): one rounding to fp32, then the factor
        out = {'margin_loss': (stats[0] / (6.0 * n_margin)).float() * mf}
        if with_pde:
            out['inter_pde_loss'], out['margin_pde_loss'] = losses[0, 6].float(), losses[1, 6].float()
            out['terms'] = losses[:, :6]
        else:
            out['terms'] = None
        valid = 0
        for k in ('margin_loss', 'inter_pde_loss', 'margin_pde_loss'):          # the order training_step adds them in
            if k in out:
                valid = valid + out[k]
        out['valid_loss'] = valid
        row = V.stats_row(stats, n_margin, {k: out[k] for k in V.LOSS_KEYS if k in out})
        out['variables'] = V.metrics_from_stats(row)['variables']
        out['stats'] = row
        if forecast_h is not None:
            out['forecast_h'] = float(forecast_h.reshape(-1)[0])
        return out

    @torch.no_grad()
    def validation_step(self, batch: dict, with_pde=True, with_clip=False):
        """The validation branch of the reference's loop (:629-719) on one sample -- the batch dict of training_step --: the three losses of the
        step body without an update, and the per-variable errors of the margin predictions in physical units.  Returns a dict: valid_loss,
        margin_loss, (with_pde) inter_pde_loss, margin_pde_loss, terms [2, 6] (interior | margin; None without with_pde) as device tensors;
        variables {u, v, p, T, q, rio: {mse, rmse, mae, bias, max_abs}} (mse = the reference's margin_<v>_loss); stats (the fp64 row
        validation.merge_stats pools); forecast_h.  One point pass over [interior | margin] with no saved state (point_path.eval_step); the PDE
        residuals clip as training_step's do (self.with_clip; the loops set it before every step, :629), the per-variable errors only on request
        (with_clip).
        Touches no .grad, no optimiser state and not the field cache."""
        b = batch
        require_gpu(b['field_data'], 'field_data', 'validation_step')
        cfg = self.point_config(self.train_cfg['losses']['loss_factor'])
        heads, evec, statics = self.physics_net.field_weights(b['field_data'], b['forecast_h'], use_cache=False)
        n_inter, pts = self._eval_inputs(b, with_pde)
        losses, stats = eval_step(cfg, n_inter, *pts, b['margin_data'], heads, evec, statics, beta=0.1, with_pde=with_pde, with_clip=with_clip)
        return self._validation_dict(losses, stats, b['margin_data'].shape[0], with_pde, b['forecast_h'])

    VALID_POINT_BYTES = 4 * (4 + 6 + 6 + 18) + 4 * 6      # x, y, t, f | coord_data | out_n | Jacobian of every point, + the margin labels

    def lead_batch_size(self, n_points, n_samples):
        """Samples per group of `validate`: as many as INFER_BUDGET_BYTES (256 MiB, the rule of chunk_size) hold of per-point buffers
        (VALID_POINT_BYTES each) plus one packed weight block per sample; at least 1, at most the number of samples."""
        per = int(n_points) * self.VALID_POINT_BYTES + point_sizes(n_points, self.precision)[1]
        return max(1, min(int(n_samples), self._within_budget(per)))

    @torch.no_grad()
    def validate(self, samples, with_pde=True, lead_batch=None, with_clip=False):
        """validation_step over a whole validation set, `lead_batch` samples at a time: the encoder, the hyper-network heads and the weight
        packing run once per group through the lead-batch launches (point_path.eval_step_batch), the point pass sample after sample.  Samples
        of a group must have equal point counts (a group is cut where they change).  Returns {'samples': [validation_step's dict per sample,
        in order], 'pooled': validation.metrics_from_stats of the merged rows (+ 'stats', the merged row)}: pooling adds sums and counts and
        maximises maxima, it never averages RMSEs.  lead_batch None: lead_batch_size (the 256 MiB rule)."""
        samples = list(samples)
        if not samples:
            raise ValueError('validate: no samples')
        cfg = self.point_config(self.train_cfg['losses']['loss_factor'])
        dev = next(self.physics_net.parameters()).device
        shape = lambda b: (b['inter_x'].shape[0], b['margin_x'].shape[0])
        rows, i = [], 0
        while i < len(samples):
            n_i, n_m = shape(samples[i])
            want = self.lead_batch_size((n_i if with_pde else 0) + n_m, len(samples)) if lead_batch is None else max(1, int(lead_batch))
            j = i + 1
            while j < len(samples) and j - i < want and shape(samples[j]) == (n_i, n_m):
                j += 1
            group = [_to_device(b, dev) for b in samples[i:j]]
            require_gpu(group[0]['field_data'], 'field_data', 'validate')
            if len(group) == 1:
                rows.append(self.validation_step(group[0], with_pde=with_pde, with_clip=with_clip))
            else:
                field = torch.cat([b['field_data'] for b in group], dim=0)
                fh = torch.cat([b['forecast_h'] for b in group], dim=0)
                B = len(group)
                heads, evec, statics = self.physics_net.field_weights(field, fh, use_cache=False)
                heads, evec = heads.reshape(B, 256, -1), evec.reshape(B, 6, 256)
                parts = [self._eval_inputs(b, with_pde) for b in group]
                pts = tuple(torch.stack([p[1][c] for p in parts], dim=0) for c in range(5))
                labels = torch.stack([b['margin_data'] for b in group], dim=0)
                losses, stats = eval_step_batch(cfg, parts[0][0], *pts, labels, heads, evec, statics, beta=0.1, with_pde=with_pde, with_clip=with_clip)
                for k_, b in enumerate(group):
                    rows.append(self._validation_dict(None if losses is None else losses[k_], stats[k_], n_m, with_pde, b['forecast_h']))
            i = j
        merged = V.merge_stats([r['stats'] for r in rows])
        pooled = V.metrics_from_stats(merged)
        pooled['stats'] = merged
        return {'samples': rows, 'pooled': pooled}

    def _valid_samples(self, kwargs):
        """The validation source of the training loops, resolved like `samples` (_train_samples): keyword `valid_samples` or
        train_cfg['valid_data']['samples']; a sequence, a callable valid_samples() -> sequence, or 'synthetic' (a SyntheticSamples drawn from
        another seed than the training source's).  None configured: None -- the loop then runs without validation, as it always did."""
        src = kwargs.get('valid_samples', (self.train_cfg.get('valid_data') or {}).get('samples'))
        if src is None:
            return None
        if isinstance(src, str):
            if src != 'synthetic':
                raise ValueError("valid_samples=%r: the only named source is 'synthetic'" % src)
            if getattr(self, '_synthetic_valid', None) is None:
                td = self.train_cfg.get('train_data', {})
                dev = next(self.physics_net.parameters()).device
                # seed 1: other fields, other cubes and other collocation draws than the training source's (seed 0)
                self._synthetic_valid = SyntheticSamples(dev, n_margin=td.get('label_batch_size', 20480), n_inter=td.get('batch_size_inter', 4096),
                                                         leads=int(kwargs.get('valid_samples_per_epoch', kwargs.get('samples_per_epoch', 61))),
                                                         seed=1, lat=self.lat_size, lon=self.lon_size)
            return self._synthetic_valid
        src = src() if callable(src) else src
        if not (hasattr(src, '__len__') and hasattr(src, '__getitem__')):
            src = list(src)
        return src

    # ------------------------------------------------------------------ training loops (:334-846, :848-1404; step body only)
    def _set_trainable(self, patterns, on, what):
        import fnmatch
        named = list(self.physics_net.named_parameters())
        names = [k for k, _ in named]
        hit = set()
        for pat in ([patterns] if isinstance(patterns, str) else list(patterns)):
            found = fnmatch.filter(names, pat)
            if not found:
                raise ValueError('%s: the pattern %r matches no parameter name' % (what, pat))
            hit |= set(found)
        changed = [k for k, p in named if k in hit and p.requires_grad != on]
        if not on and not any(p.requires_grad for k, p in named if k not in hit):
            raise ValueError('freeze: no trainable parameter is left')
        for k, p in named:
            if k in hit:
                p.requires_grad_(on)
        return changed

    def freeze(self, patterns):
        """requires_grad_(False) on every parameter of the PhysicsNet whose state-dict name matches one of the fnmatch patterns ('meta_net.*',
        '*_net.coord_*_fc.*', '*.bias'); returns the names it changed.  For callers with their own loop: freeze, THEN build_optimizer (the
        optimiser holds the trainable parameters only; one built before does not follow).  The steps skip what a frozen part does not need -- with
        'meta_net.*' the whole encoder backward.  ValueError: a pattern that matches nothing, nothing trainable left."""
        return self._set_trainable(patterns, False, 'freeze')

    def unfreeze(self, patterns):
        """The reverse of freeze; returns the names it changed.  Build a new optimiser afterwards and load_state_dict the old one's state if wanted."""
        return self._set_trainable(patterns, True, 'unfreeze')

    def build_optimizer(self, **overrides):
        """Fused clip + Adam over the PhysicsNet with the config's optimiser settings (cfg:151-155; `initial_lr` as :394 sets it), its flat
        gradient buffer laid out in backward-completion order (PhysicsNet.gradient_buckets).  The config's `ema_weights` entry is a loop option
        (_ema_option), not an optimiser keyword: it becomes ema_decay / ema_warmup unless the overrides name those themselves.  Likewise
        `step_guard` (config key or override; _step_guard_option): it becomes skip_nonfinite and the four spike keywords of FusedClipAdam.
        Fine-tuning (config keys or overrides): `freeze` = [fnmatch patterns on state-dict names] sets requires_grad_(False) on what they match;
        `param_groups` = [dict(match=[patterns], lr=..., weight_decay=..., betas=..., eps=...), ...] -- earlier groups win, the unmatched trainable
        parameters form the last group with the config's own values (optim.resolve_param_groups).  The optimiser then holds the trainable parameters
        only, in gradient_buckets() order with the frozen ones left out (a bucket may be empty), every group with its `initial_lr` and the `names` of
        its parameters.  Neither key set, nothing frozen: the one-group optimiser of before, built by the same call."""
        oc = dict(self.train_cfg.get('optimizer', {}))
        name = oc.pop('name', 'Adam')
        if name != 'Adam':
            raise NotImplementedError('the fused optimiser implements Adam (cfg:151-155); got %r' % name)
        if oc.pop('ema_weights', None) is not None and 'ema_decay' not in overrides:
            ema = self._ema_option({})
            if ema is not None:
                oc.update(ema_decay=ema['decay'], ema_warmup=ema['warmup'])
        oc.update(overrides)
        guard = self._step_guard_option({'step_guard': oc.pop('step_guard', None)})
        if guard is not None:
            oc.update(skip_nonfinite=True, **guard.as_dict())
        freeze, groups = oc.pop('freeze', None), oc.pop('param_groups', None)
        net = self.physics_net
        if freeze:
            self.freeze(freeze)
        if not groups and all(p.requires_grad for p in net.parameters()):
            opt = FusedClipAdam(net.parameters(), layout=net.gradient_buckets(), **oc)
        else:
            _, resolved = resolve_param_groups(net.named_parameters(), None, groups, {k: oc[k] for k in GROUP_KEYS if k in oc})
            opt = FusedClipAdam(resolved, layout=net.trainable_buckets(), **oc)
        for g in opt.param_groups:
            g.setdefault('initial_lr', g['lr'])
        if opt.ema_decay is not None:
            opt.bind_module(self.physics_net)                            # load_ema / ema_state_dict go by this module's parameter names
        return opt

    def _build_lr_schedule(self, optimizer, current_epoch):
        sc = dict(self.train_cfg.get('lr_schedule') or {})
        if not sc:
            return None
        name = sc.pop('name', 'CosineAnnealingLR')
        sc.pop('verbose', None)                       # cfg:160-165 passes verbose=True, which torch >= 2.7 rejects (defect 4)
        return getattr(torch.optim.lr_scheduler, name)(optimizer, last_epoch=current_epoch - 1, **sc)

    def _train_source(self, kwargs):
        """The training samples source as given (keyword `samples`, or train_cfg['train_data']['samples']); 'synthetic': the SyntheticSamples
        _train_samples made for it (None before it did)."""
        src = kwargs.get('samples', (self.train_cfg.get('train_data') or {}).get('samples'))
        return getattr(self, '_synthetic_samples', None) if src == 'synthetic' else src

    def _train_samples(self, kwargs, epoch):
        src = kwargs.get('samples', self.train_cfg.get('train_data', {}).get('samples'))
        if src is None:
            # the reference's PhysicsDataset reads GeoTIFF / xarray files (dataset/physics_dataset.py: file I/O outside this build, SURVEY.md
            # section 2 row 10) and fails when they are missing; so does this loop.  Synthetic data is an explicit choice.
            raise RuntimeError("run_train_interface: no `samples` source (a sequence / callable of training batches, as keyword or as "
                               "train_cfg['train_data']['samples']).  samples='synthetic' (train.py --synthetic) draws random field samples "
                               "and on-device collocation batches instead -- noise, for smoke runs only")
        if isinstance(src, str):
            if src != 'synthetic':
                raise ValueError("samples=%r: the only named source is 'synthetic'" % src)
            if getattr(self, '_synthetic_samples', None) is None:
                td = self.train_cfg.get('train_data', {})
                dev = next(self.physics_net.parameters()).device
                self._synthetic_samples = SyntheticSamples(dev, n_margin=td.get('label_batch_size', 20480), n_inter=td.get('batch_size_inter', 4096),
                                                           leads=int(kwargs.get('samples_per_epoch', 61)), lat=self.lat_size, lon=self.lon_size)
                print("run_train_interface: samples='synthetic' -- random field samples (%d per epoch) and on-device collocation batches; "
                      "the checkpoints of this run are trained on noise" % len(self._synthetic_samples))
            return self._synthetic_samples
        return src(epoch) if callable(src) else src

    @staticmethod
    def _shard_samples(samples, rank, world, shuffle_seed=None):
        """DistributedSampler semantics (:936, drop_last=False): every rank takes ceil(n / world) samples of the epoch -- rank r the samples
        r, r + world, ... -- and the tail wraps around to the epoch's first samples, so that all ranks run the same number of steps (and
        of all-reduces).  A sequence is indexed (a rank touches only its own samples); any other iterable is consumed round by round.
        shuffle_seed (sequences only): the order is `torch.randperm(n)` drawn from a generator seeded with it, as DistributedSampler(shuffle=True,
        seed=0) does; the reference never calls `set_epoch`, so every epoch walks the SAME seed-0 permutation (torch/utils/data/distributed.py)."""
        if hasattr(samples, '__len__') and hasattr(samples, '__getitem__'):
            n = len(samples)
            if n == 0:
                return
            if shuffle_seed is not None:
                g = torch.Generator()
                g.manual_seed(int(shuffle_seed))
                order = torch.randperm(n, generator=g).tolist()
            else:
                order = list(range(n))
            if world == 1:
                for i in order:
                    yield samples[i]
                return
            for k in range(-(-n // world)):
                yield samples[order[(rank + k * world) % n]]
            return
        if world == 1:
            yield from samples
            return
        head, buf = [], []
        for smp in samples:
            if len(head) < world:
                head.append(smp)
            buf.append(smp)
            if len(buf) == world:
                yield buf[rank]
                buf = []
        if buf:                                          # incomplete last round: padded with the epoch's first samples
            k = 0
            while len(buf) < world:
                buf.append(head[k % len(head)])
                k += 1
            yield buf[rank]

    def _epoch_samples(self, kwargs, epoch, rank, world, dist_mode=False):
        """The epoch's samples of this rank.  `samples` may be a callable samples(epoch) -> all samples, sharded here like DistributedSampler.
        The distributed loop shuffles an indexable source the way the reference's sampler does (:936: DistributedSampler's defaults = a seed-0
        permutation, the same every epoch because `set_epoch` is never called); keyword `shuffle=False` keeps the given order, `shuffle_seed`
        changes the seed.  The single-process loop takes the samples in the given order (the reference's DataLoader(shuffle=True), :419, draws an
        unseeded permutation per epoch: shuffle in the source if wanted).  Iterables that cannot be indexed are consumed in their own order.
        With samples_per_rank=True (keyword, or attribute `samples.per_rank = True`) the callable is samples(epoch, rank, world) -> this rank's
        samples only (nothing is drawn for the other ranks)."""
        src = self._train_source(kwargs)
        per_rank = kwargs.get('samples_per_rank', getattr(src, 'per_rank', False))
        if callable(src) and per_rank:                   # explicit protocol (keyword samples_per_rank=True or attribute samples.per_rank)
            return src(epoch, rank, world)
        seed = int(kwargs.get('shuffle_seed', 0)) if (dist_mode and kwargs.get('shuffle', True)) else None
        return self._shard_samples(self._train_samples(kwargs, epoch), rank, world, shuffle_seed=seed)

    def _run_train(self, dist_mode, **kwargs):
        tc = self.train_cfg
        # samples per optimiser step (1: not one call differs below); refused here, before anything is built, together with the single-sample options
        lead_batch = self._lead_batch_option(kwargs)
        lbfgs = self._lbfgs_option(kwargs)                              # None: not one call differs below
        if lbfgs is not None:
            self._lbfgs_refusals(kwargs, dist_mode)
        self.last_lbfgs = None
        num_epoch = int(kwargs.get('num_epoch', tc['num_epoch']))
        self.dx, self.dy = float(tc['dx']), float(tc['dy'])
        time_step = tc.get('lable_time_step', 1)
        self.dt = float(60 * 60 * time_step)
        checkpoint_path = kwargs.get('checkpoint_path') or tc.get('checkpoints', {}).get('checkpoints_path')
        save_step = int(tc.get('checkpoints', {}).get('save_step', 1))
        log_step = int(tc.get('log', {}).get('log_step', 100))
        pde_start = int(kwargs.get('pde_start_step', 2000))              # :436-441: PDE losses switch on at global_step >= 2000
        max_steps = kwargs.get('max_steps')
        with_pde_cfg = bool(tc.get('with_pde', True)) if dist_mode else True      # only the _dist loop reads train_cfg['with_pde'] (:857)
        rank, world, sync = 0, 1, None
        if dist_mode:
            from .. import distributed as D
            rank, world, local = D.init_from_env(kwargs.get('backend'))
            device = torch.device('cuda', local if kwargs.get('device') is None else kwargs['device'])
            torch.cuda.set_device(device)
        else:
            device = torch.device(kwargs.get('device', tc.get('device', 'cuda:0')))
        self.physics_net.to(device)
        self.pe.to(device)
        if checkpoint_path and rank == 0:
            os.makedirs(checkpoint_path, exist_ok=True)
        loss_factor = tc['losses']['loss_factor']
        state_dict, current_epoch, global_step = (None, 0, 0)
        if checkpoint_path:
            state_dict, current_epoch, global_step = self.load_model(checkpoint_path, prefix='physics', map_location=device)
        if state_dict is not None:
            if rank == 0:
                print('resume from epoch %d global_step %d' % (current_epoch, global_step))
            self.physics_net.load_state_dict(state_dict['model'], strict=True)
        ema = self._ema_option(kwargs)                                  # None: the optimiser, the launches, the rows and the checkpoints of before
        tune = {k: kwargs[k] for k in ('freeze', 'param_groups') if kwargs.get(k)}      # fine-tuning: keywords win over train_cfg['optimizer']
        guard = self._step_guard_option(kwargs)                         # None: likewise
        if guard is not None:
            tune['step_guard'] = guard
        optimizer = self.build_optimizer(**tune) if ema is None else self.build_optimizer(ema_decay=ema['decay'], ema_warmup=ema['warmup'], **tune)
        if guard is not None and not (isinstance(optimizer, FusedClipAdam) and optimizer.step_guard is not None):
            raise ValueError('step_guard: the guard lives inside the fused clip + Adam step (FusedClipAdam); the optimiser built here is %s'
                             % type(optimizer).__name__)
        guard_seen = (int(optimizer.step_count), 0) if guard is not None else None      # (calls, skipped) at the previous log step
        self.last_step_guard = None
        if dist_mode:
            D.broadcast_parameters(self.physics_net)                    # DistributedDataParallel does this at wrap time (:903-907)
            sync = D.GradientAllReduce(optimizer)
        if ema is not None:
            if state_dict is not None and 'model_ema' in state_dict and 'ema' in state_dict:
                # a resumed run: the saved average, not the raw weights, and the warm-up goes on where it was
                optimizer.load_ema(state_dict['model_ema'], int(state_dict['ema']['updates']))
            elif dist_mode:
                optimizer.reset_ema()                                   # the shadow was filled before the broadcast
        lr_schedule = self._build_lr_schedule(optimizer, current_epoch)
        self.physics_net.train()
        last = None
        # validation (:629-745): only with a source; without one nothing below runs and the loop is what it was
        valid_src = self._valid_samples(kwargs)
        vlog = self._ValidationLoop(self, valid_src, kwargs.get('log_path'), rank, world, num_epoch, device) if valid_src is not None else None
        if vlog is not None and ema is not None:
            vlog.ema_optimizer = optimizer                              # both validation events run on the averaged weights
        adaptive = self._adaptive_option(kwargs)                        # None: not one extra call below
        causal = self._causal_option(kwargs)                            # None: the step's launches of before
        balance = self._balance_option(kwargs)                          # None: likewise
        if balance is None:
            self.loss_balance_state = None                              # (a checkpoint's weights are not carried into a run without the option)
        seen = global_step                                              # samples this rank has trained on (the log line's fps)
        for epoch in range(current_epoch, num_epoch):
            if lbfgs is not None and epoch >= lbfgs['start_epoch'] and not isinstance(optimizer, FusedLBFGS):
                # the refinement phase: Adam is dropped (its arena registration with it), L-BFGS takes over the same trainable parameters
                grad_arena.unregister(optimizer)
                optimizer.zero_grad()
                optimizer = FusedLBFGS([p for p in self.physics_net.parameters() if p.requires_grad],
                                       **{k: v for k, v in lbfgs.items() if k != 'start_epoch'})
                lr_schedule = None                                      # (the schedule was Adam's)
                if rank == 0:
                    print('epoch %d: L-BFGS refinement (history %d, %d iterations per step)'
                          % (epoch, optimizer.defaults['history_size'], optimizer.defaults['max_iter']))
            stream = self._epoch_samples(kwargs, epoch, rank, world, dist_mode)   # DistributedSampler (:936): one field sample per rank per step
            if lead_batch > 1:                                          # ... or lead_batch consecutive ones of the rank's stream
                stream = self._lead_groups(stream, lead_batch)
            for batch_id, batch in enumerate(stream):
                with_pde = with_pde_cfg and global_step >= pde_start
                self.with_clip = True
                global_step += 1
                if lead_batch > 1:                                      # the log step's forecast_hours and train_vars: the group's first sample
                    group = [_to_device(b, device) for b in batch]
                    batch = group[0]
                else:
                    group, batch = None, _to_device(batch, device)
                seen += 1 if group is None else len(group)
                log_now = vlog is not None and global_step % log_step == 1
                if log_now:              # the training batch's six errors (:518-530) from the predictions the step is about to train on
                    train_vars = self.validation_step(batch, with_pde=False)['variables']
                if adaptive is not None and with_pde and (global_step - 1) % int(adaptive['every']) == 0:
                    # the interior points go where this step's network violates its equations most (adaptive_interior)
                    redraw = lambda b: self.adaptive_interior(b, self._adaptive_sampler(adaptive, b, kwargs), pool_factor=adaptive['pool_factor'],
                                                              k=adaptive['k'], c=adaptive['c'])
                    if group is not None:                               # sample by sample (the point counts, so the grouping, stay)
                        group = [redraw(b) for b in group]
                    batch = redraw(batch) if group is None else group[0]
                # (causal time weights, balanced terms: training_step drops both until the PDE losses are on)
                lbfgs_text = ''
                if isinstance(optimizer, FusedLBFGS):
                    # one L-BFGS call on this step's points: the closure is the step's forward and backward (loss_and_gradients)
                    held = {}

                    def closure():
                        held['loss'], held['parts'] = self.loss_and_gradients(batch if group is None else group, optimizer, with_pde=with_pde)
                        return held['loss']
                    optimizer.step(closure)
                    lb = optimizer.last
                    loss, parts, gnorm = torch.tensor(lb['f']), held['parts'], None
                    self.last_lbfgs = {'lbfgs_iters': lb['iters'], 'lbfgs_evals': lb['evals'], 'lbfgs_t': lb['t'], 'lbfgs_status': lb['status']}
                    lbfgs_text = ' lbfgs_iters %d lbfgs_evals %d lbfgs_t %.4g lbfgs_status %s' % (lb['iters'], lb['evals'], lb['t'], lb['status'])
                elif group is None:
                    loss, parts, gnorm = self.training_step(batch, optimizer, with_pde=with_pde, grad_sync=sync, causal=causal, balance=balance)
                else:
                    loss, parts, gnorm, _ = self.training_step_batch(group, optimizer, with_pde=with_pde, grad_sync=sync)
                last = {'loss': loss, 'parts': parts, 'grad_norm': gnorm}
                guard_text = ''
                if guard is not None and global_step % log_step == 1:   # read at log steps only; raises when every step since the last one was skipped
                    self.last_step_guard, guard_seen = self._step_guard_log(optimizer, guard_seen)
                    guard_text = ' skipped_nonfinite %d skipped_spike %d running_norm %.4g' % tuple(
                        self.last_step_guard[k] for k in ('skipped_nonfinite', 'skipped_spike', 'running_norm'))
                if rank == 0 and global_step % log_step == 1:
                    print('epoch %d step %d loss %.6g %s%s%s' % (epoch, global_step, float(loss),
                                                                  ' '.join('%s %.4g' % (k, float(v)) for k, v in parts.items()),
                                                                  self._balance_log_text(balance is not None and with_pde), guard_text + lbfgs_text))
                if global_step % log_step == 1:                       # (the loop synchronises here anyway: float(loss))
                    encoder_ops.check_enc_status()                                # an encoder weight outside the f16 hi+lo split's range raises HERE, named
                if log_now:
                    vlog.log_step_event(epoch, batch_id, global_step, batch, loss, parts, train_vars, with_pde, kwargs, seen)
                if max_steps is not None and global_step >= max_steps:
                    break
            if epoch % save_step == 0:
                if lr_schedule is not None:
                    lr_schedule.step()
                    optimizer.sync_hyper()
                encoder_ops.check_enc_status()
                if checkpoint_path and rank == 0:
                    extra = {} if ema is None else dict(model_ema=optimizer.ema_state_dict(self.physics_net),
                                                        ema=dict(decay=ema['decay'], warmup=ema['warmup'], updates=optimizer.ema_updates()))
                    self.save_model(checkpoint_path, epoch, global_step, prefix='physics', dx=self.dx, dy=self.dy, dt=self.dt,
                                    pred_x_span=self.dx * self.lon_size, pred_y_span=self.dy * self.lat_size, pred_t_span=self.pred_t_span,
                                    label_time_step=time_step, obs_norm_cfg=self.obs_norm_cfg, **extra)
            if vlog is not None and kwargs.get('validate_every_epoch', False):
                vlog.epoch_event(epoch, global_step, with_pde_cfg and global_step >= pde_start, kwargs)
            if max_steps is not None and global_step >= max_steps:
                break
        out = {'epoch': epoch if num_epoch > current_epoch else current_epoch, 'global_step': global_step, 'optimizer': optimizer,
               'lr': optimizer.param_groups[0]['lr'] if len(optimizer.param_groups) == 1 else [g['lr'] for g in optimizer.param_groups],
               'last': last}
        if vlog is not None:
            out['last_validation'], out['last_epoch_validation'] = vlog.last, vlog.last_epoch
        return out

    class _ValidationLoop:
        """What the training loops do at a log step once a validation source is set (:596-745): the training line, one validation sample taken
        round-robin (the reference's valid_iter, :630-634), the validation line; rank 0 writes, every rank evaluates its own shard."""

        def __init__(self, model, source, log_path, rank, world, num_epoch, device):
            import time
            self.m, self.src, self.rank, self.world, self.num_epoch, self.device = model, source, rank, world, num_epoch, device
            self.log = V.TrainLog(log_path) if (log_path and rank == 0) else None
            self.cursor, self.last, self.last_epoch = 0, None, None
            self.clock, self.t0, self.step0 = time.perf_counter, time.perf_counter(), 0
            self.hours = float((model.train_cfg.get('train_data') or {}).get('forecast_time_period', 360))
            self.ema_optimizer = None                  # the loops' ema_weights option: the optimiser whose averaged weights validation runs on

        def _weights(self):
            """(context the validation runs in, extra keys of its row): the averaged weights and "weights": "ema", or nothing."""
            if self.ema_optimizer is None:
                return contextlib.nullcontext(), {}
            return self.ema_optimizer.ema_weights(), {'weights': 'ema'}

        def _all_ranks(self, row):
            """The rows of all ranks merged in rank order: ONE collective on one small fp64 tensor (gathered, so that the maxima travel with it)."""
            if self.world == 1:
                return row
            import torch.distributed as dist
            mine = row.to(self.device)
            rows = [torch.empty_like(mine) for _ in range(self.world)]
            dist.all_gather(rows, mine)
            return V.merge_stats([r.cpu() for r in rows])

        def log_step_event(self, epoch, batch_id, global_step, batch, loss, parts, train_vars, with_pde, kwargs, seen=None):
            m = self.m
            now = self.clock()
            seen = global_step if seen is None else seen                                       # (lead_batch: several samples per step)
            fps = (seen - self.step0) * self.world / max(now - self.t0, 1e-9)                 # samples per second since the last log line
            src_train = m._train_source(kwargs)
            n_batches = -(-len(src_train) // self.world) if hasattr(src_train, '__len__') else 0
            vb = _to_device(self.src[(self.cursor * self.world + self.rank) % len(self.src)], self.device)     # round-robin; rank r its own stride
            self.cursor += 1
            m.with_clip = True                                                                 # :629
            was_training = m.physics_net.training
            m.physics_net.eval()                                                               # :516 (no layer here depends on it)
            weights, tag = self._weights()
            with weights:
                res = m.validation_step(vb, with_pde=with_pde)
            m.physics_net.train(was_training)
            res['pooled'] = V.metrics_from_stats(self._all_ranks(res['stats']))
            res['global_step'] = global_step
            self.last = res
            if self.log is not None:
                f_train = int(round(float(batch['forecast_h'].reshape(-1)[0]) * self.hours))
                f_valid = int(round(res['forecast_h'] * self.hours))
                vparts = {k: res[k] for k in ('margin_loss', 'inter_pde_loss', 'margin_pde_loss') if k in res}
                self.log.line(V.format_train_line(epoch, self.num_epoch, batch_id, n_batches, global_step, loss, parts, f_train, fps))
                self.log.line(V.format_valid_line(epoch, self.num_epoch, batch_id, n_batches, global_step, res['valid_loss'], vparts, f_valid, fps))
                extra = {}
                lc = getattr(m, 'last_causal', None)
                if lc is not None:                           # the interior group's causal weights of this step (the loop synchronises here anyway)
                    bins = (lc['inter'].numel() - 2) // 3
                    extra = {'causal_min_w': float(lc['inter'][3 * bins]), 'causal_w': lc['inter'][:bins].tolist()}
                extra.update(m._balance_log(with_pde))       # the K balancing weights and gradient norms (likewise read here only)
                extra.update(getattr(m, 'last_step_guard', None) or {})       # the step guard's counters and running norm (likewise)
                extra.update(getattr(m, 'last_lbfgs', None) or {})            # the L-BFGS phase: iterations, evaluations, step length, status
                self.log.event('training', epoch=epoch, global_step=global_step, train_loss=loss, forecast_hours=f_train, fps=fps, variables=train_vars,
                               **parts, **extra)
                self.log.event('validation', epoch=epoch, global_step=global_step, forecast_hours=f_valid, fps=fps,
                               **{k: v for k, v in res.items() if k != 'global_step'}, **tag)
            self.t0, self.step0 = self.clock(), seen

        def epoch_event(self, epoch, global_step, with_pde, kwargs):
            """validate_every_epoch: the whole source (this rank's shard of it, unshuffled), pooled over the ranks."""
            m = self.m
            shard = list(m._shard_samples(self.src, self.rank, self.world))
            m.with_clip = True
            weights, tag = self._weights()
            with weights:
                res = m.validate(shard, with_pde=with_pde, lead_batch=kwargs.get('valid_lead_batch'))
            pooled = V.metrics_from_stats(self._all_ranks(res['pooled']['stats']))
            self.last_epoch = {'epoch': epoch, 'global_step': global_step, 'samples': res['samples'], 'pooled': pooled}
            if self.log is not None:
                self.log.event('validation_epoch', epoch=epoch, global_step=global_step, pooled=pooled,
                               samples=[{'forecast_h': r['forecast_h'], 'valid_loss': r['valid_loss'], 'variables': r['variables']} for r in res['samples']],
                               **tag)

    def run_train_interface(self, **kwargs):
        """The single-GPU training loop (:334-846) reduced to what is on the path: per-step body (:443-515) = training_step, PDE losses on
        from global_step >= 2000, CosineAnnealingLR stepped and a checkpoint written once per epoch (:831-845), resume from
        `physics_latest.pth` (:389-397).  kwargs of the reference: checkpoint_path, log_path (written only with a validation source: the
        reference's two lines per log step in log_<date>.txt and metrics.jsonl; no tensorboard / JPEG output here);
        added: samples (see _train_samples), valid_samples (see _valid_samples; none: no validation, the loop of before), validate_every_epoch,
        valid_lead_batch, num_epoch, max_steps, pde_start_step, device, adaptive_interior (None, or dict(pool_factor, k, c, every, sampler): once
        the PDE losses are on, every every-th step's interior points are redrawn by adaptive_interior before the step; unset: the loop of before),
        causal_weights (None, or dict(eps, bins, relative): once the PDE losses are on, every step's PDE losses carry causal time weights; the
        log-step row of metrics.jsonl gains causal_min_w and causal_w, the interior group's weights; validation stays unweighted),
        balance_losses (None, a balance.LossBalance, or dict(every, momentum, groups, lam_min, lam_max): once the PDE losses are on, the step
        minimises the terms under weights balanced by their gradient norms, refreshed on every every-th such step; the log line and the log-step row
        of metrics.jsonl gain balance_lambda and balance_norm, K values each; checkpoints carry the weights and the counter under 'loss_balance';
        validation stays unweighted),
        lead_batch (k: k consecutive samples of the epoch's -- per-rank -- stream per optimiser step, training_step_batch; a group is cut early where
        the point counts change and at the end of the epoch; global_step counts optimiser steps, the log line's fps counts samples, its forecast
        hours and train_vars are the group's first sample's; adaptive_interior redraws sample by sample; together with causal_weights or
        balance_losses: NotImplementedError at loop start; unset or 1: the loop of before),
        ema_weights (None, a decay, or dict(decay, warmup): the optimiser keeps an exponential moving average of the weights inside its update
        launch; both validation events run on it and their rows carry "weights": "ema" (train_vars stay on the raw weights), checkpoints gain
        `model_ema` -- a state dict of the PhysicsNet -- and `ema` = dict(decay, warmup, updates), and a resumed run takes the average and its
        update count from them; unset: the loop of before),
        step_guard (None, True, a guard.StepGuard, or dict(spike_factor, spike_decay, spike_warmup, spike_patience): the fused optimiser step refuses,
        on the device, an update whose total gradient norm is NaN / +-inf -- with a spike_factor also one above spike_factor times the running mean
        of the applied steps' norms; a refused step leaves parameters, moments and the weight EMA bit for bit as they were, for the single-sample
        step and the lead_batch step alike (a bad sample skips the whole step); the log line and the log-step row of metrics.jsonl gain
        skipped_nonfinite, skipped_spike and running_norm, read at log steps only; RuntimeError when every step since the previous log step was
        skipped; ValueError at loop start with an optimiser that is not a FusedClipAdam; the guard's state rides in the optimiser's state dict --
        the loops' checkpoints hold no optimiser state, today as before; a loss that is non-finite while all gradients are finite is not seen;
        unset: the loop of before),
        lbfgs (None, or dict(start_epoch, history_size, max_iter, max_eval, lr, tolerance_grad, tolerance_change, history): from epoch start_epoch on
        the loop drops the Adam optimiser and refines with lbfgs.FusedLBFGS over the same trainable parameters (frozen ones stay frozen), ONE
        FusedLBFGS.step per loop step on that step's points -- single samples and lead_batch groups alike; the learning-rate schedule ends with Adam;
        the log line and the log-step row of metrics.jsonl gain lbfgs_iters, lbfgs_evals, lbfgs_t and lbfgs_status; ValueError before training starts
        together with adaptive_interior, causal_weights, balance_losses (the objective would change between the evaluations of a line search),
        ema_weights or step_guard (they live in the Adam launch); unset: the loop of before),
        freeze ([fnmatch patterns on state-dict names]) and param_groups ([dict(match=[patterns], lr=..., weight_decay=..., betas=..., eps=...)]):
        fine-tuning, as train_cfg['optimizer'] takes them (build_optimizer) -- with checkpoint_path naming an existing checkpoint the run starts from
        its weights, frozen parameters stay bit-identical, the checkpoints written still hold the full model (and a complete model_ema), and the
        result's `lr` is a list, one per group, when there are several.
        With a validation source the result carries `last_validation`."""
        return self._run_train(False, **kwargs)

    def run_train_interface_dist(self, **kwargs):
        """The data-parallel loop (:848-1404): one process per GPU (start it with torchrun; torch.distributed is initialised from the
        environment, which the reference never does -- SURVEY section 0, defect 2), rank r takes every world-th sample
        (DistributedSampler, :936), gradients are averaged by distributed.GradientAllReduce on the optimiser's flat gradient buffer
        (replaces the DistributedDataParallel wrap :903-907), rank 0 writes the checkpoints.  Validation: every rank evaluates its own samples
        of the source, the statistics rows are gathered once (validation.merge_stats), rank 0 logs.
        lead_batch: every rank groups its OWN stream, and every optimiser step is a collective -- all ranks must form the same number of groups per
        epoch.  They do when all samples of the epoch have the same point counts (the sharding hands every rank the same number of samples; groups
        are then cut by count alone).  A source whose point counts vary from sample to sample can cut the ranks' streams differently, and the
        rank with more groups would wait in its all-reduce for ever: give such a source to this loop only with lead_batch unset.
        step_guard: the gradients are all-reduced before the norm is taken and the guard's state evolves from the norm alone, so every rank forms
        the same verdict and the ranks stay in step without a collective of the guard's own.  This has not been run with more than one rank.
        lbfgs: refused (ValueError): the line search would need the loss reduced across the ranks as well."""
        return self._run_train(True, **kwargs)

    # ------------------------------------------------------------------ inference loop (:1407-1530)
    @staticmethod
    def gather_key_from_state(k, state_dict: dict, default):
        """:1532-1536 -- a checkpoint's own value of `k` when it carries one."""
        return state_dict[k] if k in state_dict else default

    def _inference_samples(self, kwargs):
        """The field samples of run_inference_interface, from the source _run_train takes its own from (`samples=` keyword or
        inference_cfg['samples']; 'synthetic' = infer.py --synthetic).  Each sample: a dict with field_data [1,159,2405], forecast_h [1,1,1] and
        `sampler`, the CollocationSampler over that sample's coarse cube."""
        src = kwargs.get('samples', (self.inference_cfg or {}).get('samples'))
        if src is None:
            raise RuntimeError("run_inference_interface: no `samples` source (a sequence / callable of dicts with field_data, forecast_h and sampler, as "
                               "keyword or as inference_cfg['samples']).  samples='synthetic' (infer.py --synthetic) evaluates random field samples -- "
                               "noise, for smoke runs only")
        if isinstance(src, str):
            if src != 'synthetic':
                raise ValueError("samples=%r: the only named source is 'synthetic'" % src)
            dev = next(self.physics_net.parameters()).device
            syn = SyntheticSamples(dev, n_margin=128, n_inter=128, leads=int(kwargs.get('samples_per_epoch', 1)), lat=self.lat_size, lon=self.lon_size)
            print("run_inference_interface: samples='synthetic' -- random field samples (%d): the maps are noise" % len(syn))
            return [dict(field_data=b['field_data'], forecast_h=b['forecast_h'], sampler=syn.sampler) for b in (syn[i] for i in range(len(syn)))]
        return src() if callable(src) else src

    def run_inference_interface(self, **kwargs):
        """The reference's inference loop (:1407-1530; there it cannot run: it calls the network with one argument, :1483): load `physics_latest.pth`
        (strictly; obs_norm_cfg and pred_t_span come from the checkpoint when it carries them, :1450-1452), then for every field sample evaluate the
        lattice `img_size` over the training domain (x `refine`) at every `dt` seconds inside the sample's window in ONE predict_lattice call; with
        log.write_source one `<time>_<variable>.npy` [lat, lon] per time step and exported variable goes to log.result_path (start_time only labels
        the files).  Returns the maps [nt, 6, ny, nx] of the last sample (None without samples).  kwargs: checkpoint_path, samples, device, with_clip,
        weights ('ema': the checkpoint's averaged weights `model_ema` in place of `model`; KeyError when it carries none).
        The product keys, each read, checked and refused before the checkpoint is read, each with a `last_*` attribute that is None again at the start
        of every run (inference_run.PRODUCTS, in its order; every entry carries its paragraph): log.export_diagnostic, inference_cfg.trajectories,
        .ensemble, .verify (or the keyword verify=), .verify_grid (or the keyword verify_grid=), .regions, .extremes, .spells.
        Plotting (log.with_vis: Basemap) is not built."""
        return run_inference(self, **kwargs)


class StagedPdeStep:
    """place_one_batch (or, lead_batch, place_lead_batch) + backward, cut where a bucket of gradients is complete
    (PhysicsNet.gradient_buckets), so that a data-parallel caller can start that bucket's all-reduce while the rest of the backward pass runs
    (BASELINE configs[3]: "bucketed overlap with backward"; the reference gets the same from DistributedDataParallel's bucket hooks,
    interface_physics.py:903-907,:1056):
        stages[0]  zero_grad, encoder + heads forward, point forward / residuals, point backward,
                   hyper-network heads backward                     -> layout buckets 0 and 1 (48 static tensors, the heads): stage_buckets[0] = (0, 2)
        stages[1]  encoder layers + norm + projection backward       -> layout bucket 2: stage_buckets[1] = (2, 3)
        stages[2]  data embedding backward (the token convolution's 7.4 MB gradient: the last to complete, it travels alone so that the
                   other 6.4 MB of the encoder start one launch earlier) -> layout bucket 3: stage_buckets[2] = (3, 4)
    One field on the fused encoder (round 6): stages[1] and stages[2] are ONE stage and buckets 2, 3 one all-reduce -- the token convolution's gradient is
    written by the encoder stack's own weight-gradient launch, so both buckets complete together (encoder_ops.embed_wgrad_rides_with_stack).
    Fine-tuning with the encoder frozen (no trainable parameter in buckets 2 and 3): meta_out requires no grad, the encoder's and the embedding's backward do
    not run and there is ONE stage -- stages == (stage_points_and_heads,), stage_buckets == ((0, 2),).  `buckets` are gradient_buckets() filtered to the
    trainable parameters (PhysicsNet.trainable_buckets), the layout of the optimiser build_optimizer makes after freeze().
    The cuts are staged_backward.StagedBackward's (training_step takes the same); the forward is this class's.
    Each stage is a plain callable (capturable in a hipGraph of its own, on one capture stream and one memory pool); after stage i the caller
    queues `grad_sync.reduce_bucket(*stage_buckets[i])`.  (Round 2 cut the heads' backward off as a stage of its own: three collectives and
    four graph segments cost 1.80 -> 2.00 ms with a one-rank RCCL group; the heads' backward is two launches, so the statics' all-reduce
    loses ~40 us of head start and still has the whole encoder backward, 0.3 ms, to travel under.)
    batch: place_one_batch's tensors (x, y, t, f, field_data, coord_data, forecast_h); with lead_batch they carry a leading B (field_data
    [B, 159, 2405], x .. f [B, N], coord_data [B, N, 6], forecast_h [B, 1, 1]) and the loss is the mean of the B field totals."""

    def __init__(self, interface, optimizer, batch, loss_factor=None, lead_batch=False, balance=None):
        if balance is not None:
            raise NotImplementedError('StagedPdeStep: loss balancing (balance=) is implemented for InterfacePhysics.training_step only, not for the '
                                      'staged or captured step, nor for lead batches')
        self.m, self.opt, self.b = interface, optimizer, batch
        self.lf = loss_factor or interface.train_cfg['losses']['loss_factor']
        self.lead_batch = bool(lead_batch)
        self.buckets, self.loss = interface.physics_net.trainable_buckets(), None       # (frozen parameters left out: a bucket may be empty)
        self.stages = (self.stage_points_and_heads, self.stage_encoder, self.stage_embedding)
        self.stage_buckets = ((0, 2), (2, 3), (3, 4))
        self.encoder_frozen = not (self.buckets[2] or self.buckets[3])
        if self.encoder_frozen:
            # fine-tuning on a frozen encoder: meta_out requires no grad, the encoder and embedding cuts vanish with their launches (the attention
            # backward, dpn_enc_bwd, the weight-gradient launch with the token convolution's 7.4 MB, the heads' g_meta problems) -- ONE stage
            self.stages = (self.stage_points_and_heads,)
            self.stage_buckets = ((0, 2),)
        elif not self.lead_batch and encoder_ops.embed_wgrad_rides_with_stack(1):
            # Round 6: one field on the fused encoder -- the token convolution's weight gradient is a problem of the stack's ONE weight-gradient launch,
            # the embedding's own backward launches nothing: buckets 2 and 3 complete together.  Two all-reduces behind each other (and a graph
            # segment that is empty) were 73 us of exposed tail on a one-rank RCCL group (gap 21 + 10 + gap 17 + 8 + gap 17); one is gap + 16 + gap.
            self.stages = (self.stage_points_and_heads, self.stage_encoder_and_embedding)
            self.stage_buckets = ((0, 2), (2, 4))
        self._seed, self.back = None, StagedBackward(self.buckets, optimizer)      # (the cuts themselves: shared with training_step)

    def stage_points(self):
        m, b = self.m, self.b
        net = m.physics_net
        self.opt.zero_grad(set_to_none=True)
        cfg = m.point_config(self.lf)
        meta_out = net.encode_field(b['field_data'], b['forecast_h'], keep_embedding=True)
        x0 = getattr(net.meta_net.model, 'last_embedding', None)             # the cut between stages 1 and 2 (None: the encoder ran unfused)
        object.__setattr__(net.meta_net.model, 'last_embedding', None)       # (self.back holds it from here on)
        heads, evec, statics = net.field_weights(b['field_data'], b['forecast_h'], meta_out=meta_out)
        if self.lead_batch:
            B = b['field_data'].shape[0]
            heads, evec = heads.reshape(B, 256, -1), evec.reshape(B, 6, 256)
            _, totals = pde_losses_batch(cfg, b['x'], b['y'], b['t'], b['f'], b['coord_data'], heads, evec, statics)
            total = totals.mean().float()
        else:
            _, total = pde_losses(cfg, b['x'], b['y'], b['t'], b['f'], b['coord_data'], heads, evec, statics, with_total=True)
        if self._seed is None:
            self._seed = torch.ones((), dtype=total.dtype, device=total.device)
        self.back.points(total, heads, evec, statics, meta_out, x0, self._seed)
        self.loss = total.detach()
        return self.loss

    def stage_points_and_heads(self):
        loss = self.stage_points()
        self.stage_heads()
        if self.encoder_frozen:
            self.stage_embedding()               # the last stage: nothing left to differentiate, release what the cuts hold
        return loss

    def stage_heads(self):
        self.back.heads_cut()

    def stage_encoder(self):
        self.back.encoder()

    def stage_encoder_and_embedding(self):
        self.stage_encoder()
        self.stage_embedding()

    def stage_embedding(self):
        self.back.embedding()                    # (the rare gradient that did not land in its slot was copied there: FusedClipAdam.place_gradients)
        self.m.physics_net.clear_field_cache()
