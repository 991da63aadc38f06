"""CPU: the parts of the validation pass that need no device -- fixture F14 against the oracle, the merge of the sufficient statistics, the log
lines, how the training loops resolve a validation source, and the C surface of the label-evaluation kernel."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import dpn_oracle as O
from oracle.fill import synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = O.Geometry()


# ------------------------------------------------------------------------------------------------ 1. F14 against the oracle
@pytest.mark.parametrize('with_pde', [True, False])
def test_f14_oracle_reproduces_the_reference_validation(golden_dir, with_pde):
    """data_loss, place_one_batch(return_parts=True), inverse_norm and a mean square, composed in the order of interface_physics.py:629-719, fp32.
    Tolerances of tests/test_oracle_golden.py for the same kinds of quantity: F5's for the PDE terms (2e-5) and totals (1e-5), F6's for the data
    loss (1e-6) and for the per-variable MSEs.  The oracle with the clip OFF reproduces `mse_noclip`; the reference's loop itself clips (its
    inverse_norm reads self.with_clip, not its argument): the oracle with the clip ON reproduces `mse`."""
    d = np.load(os.path.join(golden_dir, 'f14_validation.npz'))
    pre = 'pde%d.' % int(with_pde)
    n = int(d['n_points'])
    st = O.make_state()
    inter, margin = synthetic_inputs(n, tag='inter'), synthetic_inputs(n, tag='margin', margin=True)
    with torch.no_grad():
        dl = O.data_loss(st, margin['x'], margin['y'], margin['t'], margin['field_data'], margin['coord_data'], margin['labels'], margin['forecast_h'], GEO)
    assert abs(float(dl) - float(d[pre + 'margin_loss'])) <= 1e-6 * float(d[pre + 'margin_loss'])
    valid = dl.float()
    if with_pde:
        for gi, (inp, key) in enumerate(((inter, 'inter_pde_loss'), (margin, 'margin_pde_loss'))):
            x, y, t = (inp[k].clone().requires_grad_(True) for k in ('x', 'y', 't'))
            total, parts, _, _ = O.place_one_batch(st, x, y, t, inp['f'], margin['field_data'], inp['coord_data'], margin['forecast_h'], GEO, return_parts=True)
            mine = np.array([float(p.detach()) for p in parts])
            assert np.all(np.abs(mine - d[pre + 'terms'][gi]) <= 2e-5 * np.abs(d[pre + 'terms'][gi])), (mine, d[pre + 'terms'][gi])
            assert abs(float(total.detach()) - float(d[pre + key])) <= 1e-5 * float(d[pre + key])
            valid = valid + total.detach().float()
    else:
        assert pre + 'terms' not in d.files
    assert abs(float(valid) - float(d[pre + 'valid_loss'])) <= 1e-6 * float(d[pre + 'valid_loss'])
    with torch.no_grad():
        fn = O.physics_net_forward(st, margin['field_data'], O.encoding_coord(margin['x'], margin['y'], margin['t'], GEO), margin['coord_data'],
                                   margin['forecast_h'])
        lab = [margin['labels'][:, k:k + 1] for k in range(6)]
        for clip, key in ((False, 'mse_noclip'), (True, 'mse')):
            mse = np.array([float(((a - b) ** 2).mean()) for a, b in zip(O.inverse_norm(fn, with_clip=clip), O.inverse_norm(lab, with_clip=clip))])
            assert np.all(np.abs(mse - d[pre + key]) <= 1e-6 * d[pre + key]), (key, mse, d[pre + key])
        out_abs = np.array([float(f_.abs().max()) for f_ in fn])
    assert np.all(np.abs(out_abs - d['out_n_abs_max']) <= 2e-6 * d['out_n_abs_max'])
    # the fixture's own fp32 / fp64 pair: the arithmetic of the errors is a 1e-5-class effect at most, and the clip binds on these inputs
    assert np.all(np.abs(d[pre + 'mse'] - d['mse_fp64']) <= 1e-5 * d['mse_fp64']) and int(d['clip_binds']) > 0
    assert np.all(np.abs(d[pre + 'mse_noclip'] - d['mse_noclip_fp64']) <= 1e-5 * d['mse_noclip_fp64'])


# ------------------------------------------------------------------------------------------------ 2. the merge
def _shard_row(pred, lab):
    from deepphysinet_amd import validation as V
    d = (pred - lab).double()
    k = torch.cat([torch.zeros(1, dtype=torch.float64), (d * d).sum(0), d.abs().sum(0), d.sum(0), d.abs().max(0).values])
    return V.stats_row(k, pred.shape[0], {'valid_loss': float(d.abs().mean())})


def test_merged_shards_equal_the_concatenation():
    from deepphysinet_amd import validation as V
    g = torch.Generator().manual_seed(0)
    sizes = (1000, 17, 300)                                     # unbalanced
    scale = (1.0, 30.0, 0.1)
    pred = [torch.randn(n, 6, generator=g, dtype=torch.float64) * s for n, s in zip(sizes, scale)]
    lab = [torch.randn(n, 6, generator=g, dtype=torch.float64) for n in sizes]
    rows = [_shard_row(p, l) for p, l in zip(pred, lab)]
    merged = V.merge_stats(rows)
    whole = _shard_row(torch.cat(pred), torch.cat(lab))
    assert torch.equal(merged[19:27], torch.cat([whole[19:25], torch.tensor([1317.0, 3.0])]))          # maxima and counts exactly
    assert torch.allclose(merged[:19], whole[:19], rtol=1e-13, atol=0.0) or float((merged[1:13] - whole[1:13]).abs().max() / whole[1:13].max()) < 1e-13
    assert float((merged[13:19] - whole[13:19]).abs().max()) <= 1e-13 * float(whole[7:13].max())       # sum d: relative to sum |d|
    assert torch.equal(V.merge_stats(torch.stack(rows)), merged)                                       # [R, ROW] form
    assert torch.equal(V.merge_stats([rows[0]]), rows[0])
    pooled = V.metrics_from_stats(merged)
    direct = torch.cat(pred) - torch.cat(lab)
    for k, v in enumerate(V.VARIABLES):
        assert abs(pooled['variables'][v]['rmse'] - float((direct[:, k] ** 2).mean().sqrt())) <= 1e-12 * pooled['variables'][v]['rmse']
        assert abs(pooled['variables'][v]['bias'] - float(direct[:, k].mean())) <= 1e-12 * float(direct[:, k].abs().mean())
        assert pooled['variables'][v]['max_abs'] == float(direct[:, k].abs().max())
    assert pooled['n_points'] == 1317 and pooled['n_samples'] == 3
    # pooling is not the mean of the shards' RMSEs
    mean_of_rmse = np.mean([V.metrics_from_stats(r)['variables']['u']['rmse'] for r in rows])
    assert abs(mean_of_rmse - pooled['variables']['u']['rmse']) > 0.5 * pooled['variables']['u']['rmse']
    # the losses pool as means over the samples
    assert abs(pooled['valid_loss'] - np.mean([float(r[27]) for r in rows])) < 1e-12
    with pytest.raises(ValueError):
        V.merge_stats([])


# ------------------------------------------------------------------------------------------------ 3. the log lines
NUM = r'-?\d+\.\d{6}'
HEAD = r'epoch:\d+/\d+,batch:\d+/\d+,iter:\d+/\d+,'
# interface_physics.py:609-618 ('grad' only when the caller has the reference's sum of gradient norms) and :720-733
TRAIN_LINE = re.compile(HEAD + r'train loss:%s,(\w+:%s,)+forecast:\d{3}h,(grad:%s,)?fps:%s' % (NUM, NUM, NUM, NUM))
VALID_LINE = re.compile(HEAD + r'valid loss:%s,(\w+:%s,)+forecast:\d{3}h,fps:%s' % (NUM, NUM, NUM))


def test_log_lines_follow_the_reference_format(tmp_path):
    from deepphysinet_amd import validation as V
    parts = {'margin_loss': torch.tensor(3527295.25), 'inter_pde_loss': torch.tensor(1251.2457), 'margin_pde_loss': torch.tensor(1094.0197)}
    tl = V.format_train_line(3, 200, 17, 61, 201, torch.tensor(3529640.5), parts, 24, 12.5)
    vl = V.format_valid_line(3, 200, 17, 61, 201, 3529640.5, {'margin_loss': 1.0}, 336, 12.5)
    assert TRAIN_LINE.fullmatch(tl) and VALID_LINE.fullmatch(vl), (tl, vl)
    # the reference's own expressions, spelled out once
    ref = 'epoch:%d/%d,batch:%d/%d,iter:%d/%d,' % (3, 200, 17, 61, 201, 61 * 200) + '%s:%f,' % ('train loss', 3529640.5)
    for k, v in parts.items():
        ref += '%s:%f,' % (k, v.item())
    ref += '%s:%03dh,' % ('forecast', 24) + '%s:%f,%s:%f' % ('grad', 7.0, 'fps', 12.5)
    assert V.format_train_line(3, 200, 17, 61, 201, 3529640.5, parts, 24, 12.5, grad=7.0) == ref
    assert tl == ref.replace('grad:7.000000,', '')
    assert vl == 'epoch:3/200,batch:17/61,iter:201/12200,valid loss:3529640.500000,margin_loss:1.000000,forecast:336h,fps:12.500000'
    log = V.TrainLog(str(tmp_path / 'logs'))
    log.line(tl), log.line(vl)
    result = {'valid_loss': torch.tensor(2.0), 'margin_loss': torch.tensor(1.5), 'inter_pde_loss': torch.tensor(0.25), 'margin_pde_loss': torch.tensor(0.25),
              'terms': torch.ones(2, 6), 'variables': {v: {'mse': 1.0, 'rmse': 1.0, 'mae': 1.0, 'bias': 0.0, 'max_abs': 2.0} for v in V.VARIABLES},
              'stats': torch.zeros(V.ROW, dtype=torch.float64), 'forecast_h': 0.5}
    log.event('validation', epoch=0, global_step=1, **result)
    log.event('validation', epoch=0, global_step=3, **dict(result, terms=None))
    assert re.fullmatch(r'log_\d{4}-\d\d-\d\d_\d\d_\d\d_\d\d\.txt', os.path.basename(log.text_path))
    assert open(log.text_path).read().splitlines() == [tl, vl]
    events = [json.loads(l) for l in open(log.json_path)]
    assert len(events) == 2 and set(result) <= set(events[0]) and events[0]['terms'] == [[1.0] * 6] * 2 and events[1]['terms'] is None
    assert events[0]['variables']['q']['max_abs'] == 2.0 and events[0]['event'] == 'validation'


# ------------------------------------------------------------------------------------------------ 4. source resolution
def _interface():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    return builder_models(**ncep_config(), precision='bf16x2')


def test_validation_source_resolution():
    m = _interface()
    assert m._valid_samples({}) is None                                     # none configured: no validation, not an error
    with pytest.raises(ValueError, match='synthetic'):
        m._valid_samples({'valid_samples': 'era5'})
    seq = [{'a': 1}, {'a': 2}]
    assert m._valid_samples({'valid_samples': seq}) is seq
    assert m._valid_samples({'valid_samples': lambda: iter(seq)}) == seq   # a callable; an iterable is materialised (the loop indexes it round-robin)
    m.train_cfg['valid_data'] = {'samples': seq}
    assert m._valid_samples({}) is seq and m._valid_samples({'valid_samples': None}) is None


def test_loop_without_a_source_never_validates(monkeypatch):
    """No source -> the old path: validation_step / validate are never called and no log object is made (stubs that raise).  The loop is driven on the
    CPU up to its first training step, which is where a run without a GPU ends (RuntimeError of the point path) -- after the source was resolved."""
    from deepphysinet_amd import validation as V
    m = _interface()
    called = []
    monkeypatch.setattr(m, 'validation_step', lambda *a, **k: called.append('validation_step'))
    monkeypatch.setattr(m, 'validate', lambda *a, **k: called.append('validate'))
    monkeypatch.setattr(V, 'TrainLog', lambda *a, **k: called.append('TrainLog'))
    monkeypatch.setattr(m, 'training_step', lambda batch, opt, **k: (torch.tensor(1.0), {'margin_loss': torch.tensor(1.0)}, torch.tensor(0.0)))

    def _optimizer(**k):
        opt = torch.optim.SGD(m.physics_net.parameters(), lr=1e-3)
        opt.sync_hyper = lambda: None                                        # the fused optimiser's hook behind lr_schedule.step()
        return opt
    monkeypatch.setattr(m, 'build_optimizer', _optimizer)
    from deepphysinet_amd import encoder_ops
    monkeypatch.setattr(encoder_ops, 'check_enc_status', lambda: None)
    batches = [{'forecast_h': torch.zeros(1, 1, 1)}] * 3
    out = m.run_train_interface(samples=batches, device='cpu', num_epoch=1, log_path='/nonexistent/never/made')
    assert out['global_step'] == 3 and called == [] and 'last_validation' not in out
    # with a source the very same loop does call it (and the stub's answer is what comes back)
    m.train_cfg.setdefault('log', {})['log_step'] = 2
    stub = {'variables': {}, 'stats': torch.zeros(V.ROW, dtype=torch.float64), 'valid_loss': torch.tensor(0.0), 'forecast_h': 0.0}
    stub['stats'][25] = 1.0
    monkeypatch.setattr(m, 'validation_step', lambda *a, **k: (called.append('validation_step'), dict(stub))[1])
    out = m.run_train_interface(samples=batches, valid_samples=batches, device='cpu', num_epoch=1)
    assert called == ['validation_step'] * 4 and out['last_validation']['global_step'] == 3        # steps 1 and 3: training batch + validation sample


def test_validation_needs_device_tensors():
    m = _interface()
    b = {'field_data': torch.zeros(1, 159, 2405), 'forecast_h': torch.zeros(1, 1, 1)}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.validation_step(b)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.validate([dict(b, inter_x=torch.zeros(4, 1), margin_x=torch.zeros(4, 1))])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.variable_errors(torch.zeros(4, 6), torch.zeros(4, 6))
    with pytest.raises(ValueError):
        m.validate([])


# ------------------------------------------------------------------------------------------------ 5. the C surface
def test_label_errors_symbols_and_argument_checks():
    import ctypes
    from deepphysinet_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    for name in ('dpn_label_errors', 'dpn_label_errors_finish', 'dpn_label_errors_blocks'):
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r'^\s*(?:int|int64_t)\s+%s\s*\(' % name, header, flags=re.M), name
    assert int(re.search(r'#define DPN_EVAL_STATS (\d+)', header).group(1)) == L.EVAL_STATS == 25
    assert [lib.dpn_label_errors_blocks(n) for n in (0, 1, 512, 513, 1037, 20480)] == [0, 1, 1, 2, 3, 40]
    ph = L.DpnPhysics()
    buf = ctypes.c_void_p(4096)
    assert lib.dpn_label_errors(None, buf, 4, 1, ctypes.byref(ph), 0.1, 0, buf, None) == -1          # argument checks come before any launch
    assert lib.dpn_label_errors(buf, buf, 0, 1, ctypes.byref(ph), 0.1, 0, buf, None) == -1
    assert lib.dpn_label_errors(buf, buf, 4, 0, ctypes.byref(ph), 0.1, 0, buf, None) == -1
    assert lib.dpn_label_errors(buf, buf, 4, 1, ctypes.byref(ph), 0.0, 0, buf, None) == -1
    assert lib.dpn_label_errors(ctypes.c_void_p(4100), buf, 4, 1, ctypes.byref(ph), 0.1, 0, buf, None) == -1       # not 8-byte aligned
    assert lib.dpn_label_errors_finish(None, 4, 1, buf, None) == -1
    src = open(os.path.join(ROOT, 'deepphysinet_amd', 'build.py')).read()
    assert 'dpn_eval.hip' in src
