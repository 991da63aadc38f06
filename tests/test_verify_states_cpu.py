"""The two verification states through their shared base (point_path._ScoreState) and the shared request checks (InterfacePhysics._verify_request
and the preparation behind it), on the CPU: the byte layout of the one buffer against the formula written out here, and the full text of every
refusal that test_verify_cpu.py and test_prob_verify_cpu.py provoke, so that the shared `word` cannot turn `verify_ensemble:` into `verify:`."""
import numpy as np
import pytest
import torch

from deepphysinet_amd import prob_verification as PV
from deepphysinet_amd import verification as VF
from deepphysinet_amd.point_path import ProbVerifyState, VerifyState

N, P, M = 3, 1, 2                                                         # odd N: a 4-byte array in front of a double would misalign it


def _documented(kind, E):
    """(name, dtype, shape) of every array by include/dpn_hip.h, in the struct's order."""
    if kind == 'verify':
        rows = [('n', torch.int32, (P, N))] + [(k, torch.float64, (P, N)) for k in VF.STATE_F64]
        return rows + [('max_ad', torch.float32, (P, N)), ('cont', torch.int32, (E, 6, N))]
    rows = [('n', torch.int32, (P, N))] + [(k, torch.float64, (2, P, N)) for k in PV.STATE_F64]
    return rows + [('rank', torch.int32, (2, P, M + 1, N)), ('rel', torch.int32, (E, 2, 2, M + 1, N))]


def _state(kind, E, **kw):
    thr = ([0], [280.0], [VF.ABOVE]) if E else ([], [], [])
    return VerifyState(N, [31], *thr, 'cpu') if kind == 'verify' else ProbVerifyState(N, [31], *thr, M, 'cpu', **kw)


@pytest.mark.parametrize('kind,E', [('verify', 1), ('verify', 0), ('verify_ensemble', 1), ('verify_ensemble', 0)])
def test_one_buffer_doubles_first_no_gaps(kind, E):
    st = _state(kind, E)
    doc = _documented(kind, E)
    fields = VF.STATE_FIELDS if kind == 'verify' else PV.STATE_FIELDS
    arrays = st.arrays()
    assert tuple(arrays) == fields == tuple(r[0] for r in doc)
    bytes_of = {torch.float64: 8, torch.int32: 4, torch.float32: 4}
    at = 0
    for name, dtype, shape in [r for r in doc if r[1] == torch.float64] + [r for r in doc if r[1] != torch.float64]:
        view = arrays[name]
        if name == fields[-1] and E == 0:
            assert view is None
            continue
        assert view.dtype == dtype and tuple(view.shape) == shape and view.is_contiguous(), name
        assert view.data_ptr() - st.buffer.data_ptr() == at, (name, at)
        assert dtype != torch.float64 or at % 8 == 0, name
        at += bytes_of[dtype] * int(np.prod(shape))
    assert st.buffer.dtype == torch.uint8 and st.buffer.numel() == at
    assert not st.buffer.any()
    for view in arrays.values():
        if view is not None:
            view.fill_(1)
    assert all(bool((v == 1).all()) for v in arrays.values() if v is not None)        # (no view overlaps another)
    st.clear()
    assert not st.buffer.any() and all(not v.any() for v in arrays.values() if v is not None)


def test_a_pooled_state_is_of_its_class_and_stages_nothing():
    for kind in ('verify', 'verify_ensemble'):
        st = _state(kind, 1)
        out = st._like(5)                                                 # what `pool` launches into
        assert type(out) is type(st) and out.n_total == 5 and out.n.shape == (P, 5)
        assert (out.ids, out.thr_col, out.thr_val, out.thr_side) == (st.ids, st.thr_col, st.thr_val, st.thr_side)
    assert st.plane_f.shape == st.plane_b.shape == (M, P, N) and out.plane_f is None and out.plane_b is None and out.members == M
    assert _state('verify_ensemble', 0, planes=False).plane_f is None


# ------------------------------------------------------------------------------------------------ the refusals, word for word
def _model_and_cases():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    from deepphysinet_amd.sampler import CollocationSampler, SamplerConfig
    torch.manual_seed(0)
    m = builder_models(**ncep_config())
    stub = lambda cfg: type('S', (), dict(cfg=cfg, cube=torch.zeros(1), check_positions=CollocationSampler.check_positions,
                                          lonlat_to_index=CollocationSampler.lonlat_to_index))()       # nothing below reaches a kernel
    mem = dict(field_data=None, forecast_h=None, sampler=stub(SamplerConfig()))
    other = dict(mem, sampler=stub(SamplerConfig(input_time_step_nums=3)))
    return m, mem, other


def provocations():
    """(key, callable) of every ValueError / KeyError that the two CPU modules provoke from the request check, the two entry points, the two
    state constructors and upload_plan."""
    from deepphysinet_amd.interface.interface_physics import InterfacePhysics
    out = []
    for word in ('verify', 'verify_ensemble'):
        req = lambda *a, word=word: InterfacePhysics._verify_request(*a, word=word)
        out += [((word, 'request', '17 products'), lambda req=req: req(['T'] * 17, None)),
                ((word, 'request', 'vorticity'), lambda req=req: req(['T', 'vorticity'], None)),
                ((word, 'request', 'threshold on speed'), lambda req=req: req(['T'], {'speed': 1.0}))]
        for name in ('point', 'names', 'thresholds') + (('members',) if word == 'verify_ensemble' else ()):
            out.append(((word, 'request', 'grouping ' + name), lambda req=req, name=name: req(['T'], None, ['station', name])))
    for bad in (0, 65, -1, 2.5):
        out.append((('verify_ensemble', 'request', 'members %r' % bad),
                    lambda bad=bad: InterfacePhysics._verify_request(['T'], None, None, bad, word='verify_ensemble')))
    m, mem, other = _model_and_cases()
    obs = torch.zeros((3, 1), dtype=torch.float32)
    xi, yi, hr = [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0, 2.0]
    for word, call, case, odd in (('verify', m.verify_at, dict(mem, obs=obs), dict(other, obs=obs)),
                                  ('verify_ensemble', m.verify_ensemble_at, dict(members=[mem, mem], obs=obs), dict(members=[mem, other], obs=obs))):
        at = lambda cases, products=('T',), call=call, **kw: call(cases, xi, yi, hr, list(products), **kw)
        out += [((word, 'at', 'gust'), lambda at=at, case=case: at([case], ['gust'])),
                ((word, 'at', 'inf'), lambda at=at, case=case: at([case], thresholds={'T': float('inf')})),
                ((word, 'at', 'no cases'), lambda at=at: at([])),
                ((word, 'at', '17 products'), lambda at=at, case=case: at([case], ['T'] * 17)),
                ((word, 'at', 'window'), lambda at=at, case=case, odd=odd: at([case, odd])),
                ((word, 'at', 'case 1 obs'), lambda at=at, case=case: at([case, dict(case, obs=None)])),
                ((word, 'at', 'negative'), lambda at=at, case=case: at([case], by={'station': [0, -1, 1]})),
                ((word, 'at', 'by hour'), lambda at=at, case=case: at([case], by={'hour': [0, 1]})),
                ((word, 'at', 'grouping'), lambda at=at, case=case, word=word: at([case], by={'names' if word == 'verify' else 'members': [0, 0, 0]}))]
        for i, bad in enumerate((obs[:2], obs.double(), obs.numpy(), None, torch.zeros((3, 2)))):
            out.append(((word, 'at', 'obs %d' % i), lambda at=at, case=case, bad=bad: at([dict(case, obs=bad)])))
    case = dict(members=[mem, mem], obs=obs)
    ens = lambda cases: m.verify_ensemble_at(cases, xi, yi, hr, ['T'])
    out += [(('verify_ensemble', 'at', 'unequal'), lambda: ens([case, dict(case, members=[mem] * 3)])),
            (('verify_ensemble', 'at', 'no members'), lambda: ens([dict(case, members=[])])),
            (('verify_ensemble', 'at', '65 members'), lambda: ens([dict(case, members=[mem] * 65)]))]
    for i, args in enumerate(((0, [31], [], [], []), (4, [], [], [], []), (4, [31] * 17, [], [], []), (4, [31], [0] * 17, [1.0] * 17, [0] * 17),
                              (4, [31], [0], [], [0]), (4, [31], [0], [1.0], []))):
        out.append((('verify', 'state', i), lambda args=args: VerifyState(*args, device='cpu')))
        out.append((('verify_ensemble', 'state', i), lambda args=args: ProbVerifyState(*args, 3, device='cpu')))
    for i, members in enumerate((0, 65)):
        out.append((('verify_ensemble', 'state', 'members %d' % members), lambda members=members: ProbVerifyState(4, [31], [], [], [], members, device='cpu')))
    for i, (n, p, e, mm) in enumerate(((2 ** 22, 16, 0, 64), (2 ** 24, 1, 16, 1), (2 ** 26, 1, 0, 64), (2 ** 31, 1, 0, 1))):
        out.append((('verify_ensemble', 'state', 'size %d' % i),
                    lambda n=n, p=p, e=e, mm=mm: ProbVerifyState(n, [31] * p, [0] * e, [1.0] * e, [0] * e, mm, device='cpu')))
    for word in ('verify', 'verify_ensemble'):
        out.append(((word, 'plan', 'order'), lambda word=word: _state(word, 0, **({} if word == 'verify' else {'planes': False})).upload_plan([0, 1], [0, 2])))
        out.append(((word, 'plan', 'seg_start'), lambda word=word: _state(word, 0, **({} if word == 'verify' else {'planes': False})).upload_plan([0, 1, 2], [3])))
    return out


# recorded on the commit before the two requests and the two states were merged; (exception, str(exception)) by provocation
PINNED = {('verify', 'request', '17 products'): ('ValueError', 'verify: 17 products; at most 16 in one request'),
 ('verify', 'request', 'vorticity'): ('KeyError', '"verification product \'vorticity\': one of u, v, p, T, q, rho, speed, rel_humidity"'),
 ('verify', 'request', 'threshold on speed'): ('ValueError', "threshold on 'speed', which is not among the requested products ['T']"),
 ('verify', 'request', 'grouping point'): ('ValueError', "verify: a grouping may not be called 'point' (the result's own keys)"),
 ('verify', 'request', 'grouping names'): ('ValueError', "verify: a grouping may not be called 'names' (the result's own keys)"),
 ('verify', 'request', 'grouping thresholds'): ('ValueError', "verify: a grouping may not be called 'thresholds' (the result's own keys)"),
 ('verify_ensemble', 'request', '17 products'): ('ValueError', 'verify_ensemble: 17 products; at most 16 in one request'),
 ('verify_ensemble', 'request', 'vorticity'): ('KeyError', '"verification product \'vorticity\': one of u, v, p, T, q, rho, speed, rel_humidity"'),
 ('verify_ensemble', 'request', 'threshold on speed'): ('ValueError', "threshold on 'speed', which is not among the requested products ['T']"),
 ('verify_ensemble', 'request', 'grouping point'): ('ValueError', "verify_ensemble: a grouping may not be called 'point' (the result's own keys)"),
 ('verify_ensemble', 'request', 'grouping names'): ('ValueError', "verify_ensemble: a grouping may not be called 'names' (the result's own keys)"),
 ('verify_ensemble', 'request', 'grouping thresholds'): ('ValueError', "verify_ensemble: a grouping may not be called 'thresholds' (the result's own keys)"),
 ('verify_ensemble', 'request', 'grouping members'): ('ValueError', "verify_ensemble: a grouping may not be called 'members' (the result's own keys)"),
 ('verify_ensemble', 'request', 'members 0'): ('ValueError', 'verify_ensemble: 0 members per case; 1 to 64'),
 ('verify_ensemble', 'request', 'members 65'): ('ValueError', 'verify_ensemble: 65 members per case; 1 to 64'),
 ('verify_ensemble', 'request', 'members -1'): ('ValueError', 'verify_ensemble: -1 members per case; 1 to 64'),
 ('verify_ensemble', 'request', 'members 2.5'): ('ValueError', 'verify_ensemble: 2.5 members per case; 1 to 64'),
 ('verify', 'at', 'gust'): ('KeyError', '"verification product \'gust\': one of u, v, p, T, q, rho, speed, rel_humidity"'),
 ('verify', 'at', 'inf'): ('ValueError', "threshold %r on 'T' is not finite" % np.float64('inf')),
 ('verify', 'at', 'no cases'): ('ValueError', 'verify: no cases (a sequence of dicts with field_data, forecast_h, sampler and obs)'),
 ('verify', 'at', '17 products'): ('ValueError', 'verify: 17 products; at most 16 in one request'),
 ('verify', 'at', 'window'): ('ValueError', 'verification case 1: input_time_step_nums = 3, but case 0 has 4; the cases must share the fine grid and the hour window'),
 ('verify', 'at', 'case 1 obs'): ('ValueError', 'verification case 1: obs must be an fp32 tensor [3, 1] on cpu, got NoneType'),
 ('verify', 'at', 'negative'): ('ValueError', 'pool_plan: a group id is negative (-1)'),
 ('verify', 'at', 'by hour'): ('ValueError', "verify: by['hour'] must hold one group id per point, [3], got (2,)"),
 ('verify', 'at', 'grouping'): ('ValueError', "verify: a grouping may not be called 'names' (the result's own keys)"),
 ('verify', 'at', 'obs 0'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((2, 1), torch.float32, device(type='cpu'))"),
 ('verify', 'at', 'obs 1'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((3, 1), torch.float64, device(type='cpu'))"),
 ('verify', 'at', 'obs 2'): ('ValueError', 'verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ndarray'),
 ('verify', 'at', 'obs 3'): ('ValueError', 'verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got NoneType'),
 ('verify', 'at', 'obs 4'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((3, 2), torch.float32, device(type='cpu'))"),
 ('verify_ensemble', 'at', 'gust'): ('KeyError', '"verification product \'gust\': one of u, v, p, T, q, rho, speed, rel_humidity"'),
 ('verify_ensemble', 'at', 'inf'): ('ValueError', "threshold %r on 'T' is not finite" % np.float64('inf')),
 ('verify_ensemble', 'at', 'no cases'): ('ValueError', 'verify_ensemble: no cases (a sequence of dicts with members and obs)'),
 ('verify_ensemble', 'at', '17 products'): ('ValueError', 'verify_ensemble: 17 products; at most 16 in one request'),
 ('verify_ensemble', 'at', 'window'): ('ValueError', 'ensemble member 3: input_time_step_nums = 3, but member 0 has 4; the members must share the fine grid and the hour window'),
 ('verify_ensemble', 'at', 'case 1 obs'): ('ValueError', 'verification case 1: obs must be an fp32 tensor [3, 1] on cpu, got NoneType'),
 ('verify_ensemble', 'at', 'negative'): ('ValueError', 'pool_plan: a group id is negative (-1)'),
 ('verify_ensemble', 'at', 'by hour'): ('ValueError', "verify_ensemble: by['hour'] must hold one group id per point, [3], got (2,)"),
 ('verify_ensemble', 'at', 'grouping'): ('ValueError', "verify_ensemble: a grouping may not be called 'members' (the result's own keys)"),
 ('verify_ensemble', 'at', 'obs 0'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((2, 1), torch.float32, device(type='cpu'))"),
 ('verify_ensemble', 'at', 'obs 1'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((3, 1), torch.float64, device(type='cpu'))"),
 ('verify_ensemble', 'at', 'obs 2'): ('ValueError', 'verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ndarray'),
 ('verify_ensemble', 'at', 'obs 3'): ('ValueError', 'verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got NoneType'),
 ('verify_ensemble', 'at', 'obs 4'): ('ValueError', "verification case 0: obs must be an fp32 tensor [3, 1] on cpu, got ((3, 2), torch.float32, device(type='cpu'))"),
 ('verify_ensemble', 'at', 'unequal'): ('ValueError', 'verify_ensemble: case 1 has 3 members, case 0 has 2; all cases must have the same number'),
 ('verify_ensemble', 'at', 'no members'): ('ValueError', 'verify_ensemble: a case has no members (a sequence of dicts with field_data, forecast_h and sampler)'),
 ('verify_ensemble', 'at', '65 members'): ('ValueError', 'verify_ensemble: 65 members per case; 1 to 64'),
 ('verify', 'state', 0): ('ValueError', 'VerifyState: 0 points, 1 products (1..16), 0 thresholds (0..16)'),
 ('verify_ensemble', 'state', 0): ('ValueError', 'ProbVerifyState: 0 points, 1 products (1..16), 0 thresholds (0..16)'),
 ('verify', 'state', 1): ('ValueError', 'VerifyState: 4 points, 0 products (1..16), 0 thresholds (0..16)'),
 ('verify_ensemble', 'state', 1): ('ValueError', 'ProbVerifyState: 4 points, 0 products (1..16), 0 thresholds (0..16)'),
 ('verify', 'state', 2): ('ValueError', 'VerifyState: 4 points, 17 products (1..16), 0 thresholds (0..16)'),
 ('verify_ensemble', 'state', 2): ('ValueError', 'ProbVerifyState: 4 points, 17 products (1..16), 0 thresholds (0..16)'),
 ('verify', 'state', 3): ('ValueError', 'VerifyState: 4 points, 1 products (1..16), 17 thresholds (0..16)'),
 ('verify_ensemble', 'state', 3): ('ValueError', 'ProbVerifyState: 4 points, 1 products (1..16), 17 thresholds (0..16)'),
 ('verify', 'state', 4): ('ValueError', 'VerifyState: 4 points, 1 products (1..16), 1 thresholds (0..16)'),
 ('verify_ensemble', 'state', 4): ('ValueError', 'ProbVerifyState: 1 threshold columns, 0 values, 1 sides'),
 ('verify', 'state', 5): ('ValueError', 'VerifyState: 4 points, 1 products (1..16), 1 thresholds (0..16)'),
 ('verify_ensemble', 'state', 5): ('ValueError', 'ProbVerifyState: 1 threshold columns, 1 values, 0 sides'),
 ('verify_ensemble', 'state', 'members 0'): ('ValueError', 'verify_ensemble: 0 members per case; 1 to 64'),
 ('verify_ensemble', 'state', 'members 65'): ('ValueError', 'verify_ensemble: 65 members per case; 1 to 64'),
 ('verify_ensemble', 'state', 'size 0'): ('ValueError', 'ProbVerifyState: 4194304 points, 16 products, 0 thresholds, 64 members: rank would hold 8724152320 elements, more than 2^31 - 1'),
 ('verify_ensemble', 'state', 'size 1'): ('ValueError', 'ProbVerifyState: 16777216 points, 1 products, 16 thresholds, 1 members: rel would hold 2147483648 elements, more than 2^31 - 1'),
 ('verify_ensemble', 'state', 'size 2'): ('ValueError', 'ProbVerifyState: 67108864 points, 1 products, 0 thresholds, 64 members: rank would hold 8724152320 elements, more than 2^31 - 1'),
 ('verify_ensemble', 'state', 'size 3'): ('ValueError', 'ProbVerifyState: 2147483648 points, 1 products, 0 thresholds, 1 members: n would hold 2147483648 elements, more than 2^31 - 1'),
 ('verify', 'plan', 'order'): ('ValueError', 'VerifyState.pool: order [3] and seg_start [G + 1], got (2,) and (2,)'),
 ('verify', 'plan', 'seg_start'): ('ValueError', 'VerifyState.pool: order [3] and seg_start [G + 1], got (3,) and (1,)'),
 ('verify_ensemble', 'plan', 'order'): ('ValueError', 'ProbVerifyState.pool: order [3] and seg_start [G + 1], got (2,) and (2,)'),
 ('verify_ensemble', 'plan', 'seg_start'): ('ValueError', 'ProbVerifyState.pool: order [3] and seg_start [G + 1], got (3,) and (1,)')}


def test_every_refusal_keeps_its_text():
    table = provocations()
    assert [k for k, _ in table] == list(PINNED)
    for key, call in table:
        with pytest.raises((ValueError, KeyError)) as err:
            call()
        assert (type(err.value).__name__, str(err.value)) == PINNED[key], key
