"""The value side of the point path -- what dpn_fwd, dpn_fwd_ref, dpn_fwd_ref_nets and dpn_fwd_ref_derivs return (fields, Jacobian, second and third
coordinate derivatives, the two ReLU masks) and what dpn_bwd_points_derivs with g_hxi feeds into the weight side -- against fp64, stage by stage, each
stage from the GPU's OWN saved masks and, where named, its own decoded T1 (tests/value_cases.py holds the cases, references and bounds;
tests/test_value_cases_cpu.py shows on the CPU that a faithful model of the kernels stays inside them and that each of a list of seeded mistakes leaves
them).  One pass per case at the C ABI (tools/value_digest.run_case), one synchronisation, one read-back.  Every condition is element-wise; nothing is
normalised by a tensor's maximum and no point is removed.  Beside the bounds: the exact statements between the entry points, the sentinel rows behind
every output, NaN guards around every per-point input, and the refusals that return before a launch."""
import os
import sys

import pytest
import torch

import value_cases as VC
import wgrad_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'tools') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu

_ratios = {}            # case id -> {(stage, tensor): worst error-to-bound ratio}
_passes = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def gpu_pass(c):
    """One pass of case c, read back: (W, Features, obs as value_cases.check_value takes it, what the entry point adds to the fields)."""
    import value_digest as VD
    inp = VC.inputs(c)
    res = VD.run_case(c.route, c.n, c.prec, gain=c.gain, geometry=VC.GEOMETRIES[c.geo], coords=(inp['x'], inp['y'], inp['t']), coord_data=inp['coord_data'],
                      ref_data=inp['ref_data'], pe_in=inp['pe_in'], entry=c.entry, fwd_kernel=c.kernel)
    assert res['inputs']['form'] == int(VC.fused(c))
    assert all(res['tails'].values()), res['tails']             # the rows behind row n of out / jac / hess / d3 and the bytes behind saved: untouched
    assert res['guards']                                        # no input was written; a read outside them would have put a NaN into a result
    W = WC.weights_of(res['inputs']['heads'], res['inputs']['evec'], res['inputs']['statics'])
    T1, m1, m2 = WC.decode_saved(res['saved'], c.n, c.prec)
    obs = {'m1': m1, 'm2': m2, 'T1': T1, 'out': res['out'], 'jac': res['jac'], 'hess': res['hess'], 'd3': res['d3']}
    ref6 = inp['coord_data'] if inp['ref_data'] is None else inp['ref_data']
    return W, VC.features(c, inp), obs, ref6


@pytest.mark.parametrize('c', VC.all_cases(), ids=VC.case_id)
def test_every_stage_against_fp64_from_the_gpus_own_masks(c):
    W, F, obs, ref6 = gpu_pass(c)
    for nm in ('out',) + VC.DERIV_NAMES:
        want = nm == 'out' or (c.route == 'raw' and (nm == 'jac' or c.entry == 'derivs'))
        assert (obs[nm] is not None) == want and (obs[nm] is None or bool(torch.isfinite(obs[nm]).all())), nm
    r = VC.check_value(c, W, F, obs, ref6)
    _ratios[VC.case_id(c)] = VC.conditions(r)
    for key in sorted(r):
        print('%-6s %-5s %.3g' % (key[0], key[1], r[key]))
    bad = {k: v for k, v in VC.conditions(r).items() if not v <= 1.0}
    assert not bad, bad
    assert bool(obs['m1'].any()) and bool(obs['m2'].any()) and not bool(obs['m1'].all()) and not bool(obs['m2'].all())


# ---------------------------------------------------------------------------------------------- exact statements between the entry points
EXACT = [VC.VCase('raw', 70, 'bf16x2', 1.0, 'odd', 'edges', 'ref', None), VC.VCase('raw', 129, 'bf16', 1.0, 'odd', 'interior', 'ref', None)]


def launch(p, entry, **kw):
    """One forward launch of Pass p read back: {'out', 'jac', 'hess', 'd3', 'saved': host tensor or None}; the sentinels behind them are asserted."""
    f = p.forward(entry, **kw)
    assert f['rc'] == 0, (entry, f['rc'])
    torch.cuda.synchronize()
    out = {}
    for k in ('out', 'jac', 'hess', 'd3', 'saved'):
        if f[k] is None:
            out[k] = None
        else:
            out[k], tail = f[k].read()
            assert tail, (entry, k, 'the sentinel behind the output is damaged')
    return out


def make_pass(c, ref_seed=7):
    import value_digest as VD
    inp = VC.inputs(c)
    ref = torch.randn(c.n, 6, generator=torch.Generator().manual_seed(ref_seed))
    return VD.Pass(c.route, c.n, c.prec, gain=c.gain, geometry=VC.GEOMETRIES[c.geo], coords=(inp['x'], inp['y'], inp['t']), coord_data=inp['coord_data'],
                   ref_data=ref, pe_in=inp['pe_in'], fwd_kernel=c.kernel), inp


@pytest.mark.parametrize('c', EXACT, ids=VC.case_id)
def test_the_entry_points_agree_bit_for_bit(c):
    import value_digest as VD
    p, inp = make_pass(c)
    base = launch(p, 'ref')
    # ---- dpn_fwd is dpn_fwd_ref with ref_data = coord_data; another ref_data moves the fields alone
    own = launch(p, 'fwd')
    as_ref = launch(p, 'ref', ref_data=p.P._ptr(p.d['coord_data']))
    for k in ('out', 'jac', 'saved'):
        assert same(own[k], as_ref[k]), k
    assert same(base['jac'], own['jac']) and same(base['saved'], own['saved']) and not same(base['out'], own['out'])
    # ---- NULL jac_n, NULL saved: no bit of what is still written changes
    for want in (('saved',), ('jac',), ()):
        got = launch(p, 'ref', want=want)
        for k in ('out',) + want:
            assert same(got[k], base[k]), (want, k)
    # ---- dpn_fwd_ref_nets: the first n_nets columns are the full launch's, the others keep the sentinel
    for n_nets in (1, 3, 6):
        got = launch(p, 'nets', n_nets=n_nets)
        assert same(got['out'][:, :n_nets], base['out'][:, :n_nets]) and same(got['jac'].view(c.n, 6, 3)[:, :n_nets], base['jac'].view(c.n, 6, 3)[:, :n_nets]), n_nets
        assert bool((bits(got['out'][:, n_nets:]) == VD.SENTINEL).all()) and bool((bits(got['jac'].view(c.n, 6, 3)[:, n_nets:]) == VD.SENTINEL).all()), n_nets
        assert same(launch(p, 'nets', n_nets=n_nets, want=())['out'][:, :n_nets], base['out'][:, :n_nets])
    # ---- dpn_fwd_ref_derivs: hess_n alone, d3_n alone and both give the same bits, and leave fields, Jacobian and saved state as dpn_fwd_ref's
    both = launch(p, 'derivs')
    for want in (('jac', 'hess', 'saved'), ('jac', 'd3', 'saved'), ('jac', 'hess', 'd3')):
        got = launch(p, 'derivs', want=want)
        for k in ('out',) + want:
            assert same(got[k], both[k]), (want, k)
    for k in ('out', 'jac', 'saved'):
        assert same(both[k], base[k]), k
    assert p.guards_intact()


def test_caller_encoded_coordinates_agree_between_the_entry_points():
    c = VC.VCase('pe_in', 70, 'bf16x2', 1.0, 'ncep', 'interior', 'ref', None)
    p, inp = make_pass(c)
    base = launch(p, 'ref')
    assert base['jac'] is None
    as_ref = launch(p, 'ref', ref_data=p.P._ptr(p.d['coord_data']))
    own = launch(p, 'fwd')
    assert same(own['out'], as_ref['out']) and same(own['saved'], as_ref['saved']) and same(own['saved'], base['saved']) and not same(own['out'], base['out'])
    assert same(launch(p, 'ref', want=())['out'], base['out'])
    assert same(launch(p, 'nets', n_nets=3, want=())['out'][:, :3], base['out'][:, :3])
    assert p.guards_intact()


# ---------------------------------------------------------------------------------------------- refusals in front of the launch
def refusals(p):
    """(entry, keyword arguments of Pass.forward) of every wrong argument that is refused before anything is launched.  (pe_in handed to a derivative
    entry and hess_n without jac_n: tests/test_gpu_custom_residuals.py drives those.)"""
    out = []
    for entry in ('fwd', 'ref', 'nets', 'derivs'):
        for want in ((('jac', 'hess', 'd3', 'saved'), ('jac', 'saved')) if entry == 'derivs' else (('jac', 'saved'),)):       # derivs: its own check, and fwd_launch's
            out += [(entry, dict(want=want, n=0)), (entry, dict(want=want, n=-5)), (entry, dict(want=want, prec=0)), (entry, dict(want=want, prec=3))]
            out += [(entry, dict(want=want, **{k: None})) for k in ('packed', 'freqs', 'geo', 'coord_data', 'out_n', 'x', 'y', 't')]
    out += [('nets', dict(n_nets=0)), ('nets', dict(n_nets=7)), ('nets', dict(n_nets=-1))]
    return out


def test_wrong_arguments_are_refused_before_a_launch():
    c = VC.VCase('raw', 70, 'bf16x2', 1.0, 'odd', 'interior', 'ref', None)
    p, _ = make_pass(c)
    pending = []
    for entry, kw in refusals(p):
        f = p.forward(entry, **kw)
        assert f['rc'] == -1, (entry, kw, f['rc'])
        pending.append((entry, kw, f))
    torch.cuda.synchronize()
    for entry, kw, f in pending:
        for k in ('out', 'jac', 'hess', 'd3', 'saved'):
            assert f[k] is None or f[k].untouched(), (entry, kw, k)
    # caller-encoded coordinates: x, y, t may be NULL, the other refusals hold
    cp = VC.VCase('pe_in', 70, 'bf16', 1.0, 'ncep', 'interior', 'ref', None)
    pp, _ = make_pass(cp)
    pending = [(kw, pp.forward('ref', **kw)) for kw in (dict(n=0), dict(prec=3), dict(packed=None), dict(coord_data=None), dict(out_n=None), dict(geo=None))]
    assert all(f['rc'] == -1 for _, f in pending)
    torch.cuda.synchronize()
    assert all(f['out'].untouched() and f['saved'].untouched() for _, f in pending)
    assert launch(pp, 'ref')['out'] is not None and launch(p, 'ref')['out'] is not None          # the passes themselves were fit to run


# ---------------------------------------------------------------------------------------------- g_hxi: dpn_bwd_points_derivs into the weight side
GH_STAGES = ('z0', 'stage1', 'saved', 'wgrad', 'finish', 'chain')


def gh_pass(n, kind, factor=1.0):
    import value_digest as VD
    key = (n, kind, factor)
    if key not in _passes:
        c, vc = VC.gh_case(n), VC.GH_INPUTS._replace(n=n)
        inp = VC.inputs(vc)
        g_out, g_jxi, g_hxi = VC.gh_cotangents(n, kind)
        g_hxi = g_hxi * factor
        res = VD.run_case('raw', n, c.prec, gain=c.gain, geometry=VC.GEOMETRIES[vc.geo], coords=(inp['x'], inp['y'], inp['t']), coord_data=inp['coord_data'],
                          ref_data=inp['ref_data'], entry='derivs', cotangents=(g_out, g_jxi), g_hxi=g_hxi, scale=c.scale)
        assert all(res['tails'].values()) and res['guards'], res['tails']
        W = WC.weights_of(res['inputs']['heads'], res['inputs']['evec'], res['inputs']['statics'])
        T1, m1, m2 = WC.decode_saved(res['saved'], n, c.prec)
        Z1, gnet, _ = WC.decode_operands(res['operands'], n, c.prec, table=False)
        Z0, _ = VC.decode_z0_stored(res['operands'], n, c.prec)
        sums, sums_abs = WC.decode_partials(res['partials'], res['k_splits'])
        outs = [res['g_heads'], res['g_evec']] + res['statics']
        obs = {'m1': m1, 'm2': m2, 'T1': T1, 'Z1': Z1, 'Z0': Z0, 'gnet': gnet, 'sums': sums, 'sums_abs': sums_abs, 'grads': WC.weights_of(outs[0], outs[1], outs[2:])}
        _passes[key] = (c, W, VC.features(vc, inp), obs, outs, (g_out, g_jxi, g_hxi))
    return _passes[key]


@pytest.mark.parametrize('n', VC.GH_SIZES)
@pytest.mark.parametrize('kind', VC.GH_KINDS)
def test_the_weight_side_behind_g_hxi_against_fp64_stage_by_stage(n, kind):
    c, W, F, obs, outs, (g_out, g_jxi, g_hxi) = gh_pass(n, kind)
    s = torch.tensor(c.scale, dtype=torch.float32)
    want = torch.zeros(6, WC.pad_points(n))
    want[:, :n] = (s * g_out).t()
    assert torch.equal(obs['gnet'], want), 'gnet is not scale * g_out'
    r = WC.check(c, W, F, obs, g_out, g_jxi, stages=GH_STAGES, g_hxi=g_hxi)
    _ratios['g_hxi-%d-%s' % (n, kind)] = r
    for key in sorted(r):
        print('%-8s %-5s %.3g' % (key[0], key[1], r[key]))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    if kind == 'gh_only':           # reached through gH alone: gnet and every g-weighted sum are exact zeros, dw1 is not
        assert not bool(obs['gnet'].any()) and not bool(obs['sums']['S2'].any()) and not bool(obs['sums']['mv'].any()) and bool(obs['sums']['dw1'].any())


def test_g_hxi_times_a_power_of_two_scales_every_gradient_exactly():
    """g_hxi alone, times 2^8 and 2^-8: Z1, the stored Z0 and every gradient times exactly that factor (normal values, as in the weight side's
    linearity test: the dense stream's hi and lo parts stay normal at these factors)."""
    _, _, _, base, outs, _ = gh_pass(70, 'gh_only')
    assert all(bool(torch.isfinite(v).all()) for v in outs) and min(float(v.abs()[v != 0].min()) for v in outs if bool(v.any())) * 2.0 ** -8 > 2.0 ** -100
    for f in (2.0 ** 8, 2.0 ** -8):
        _, _, _, got, gouts, _ = gh_pass(70, 'gh_only', factor=f)
        assert torch.equal(got['Z1'], base['Z1'] * f) and torch.equal(got['Z0'], base['Z0'] * f)
        for i, (a, b) in enumerate(zip(gouts, outs)):
            assert torch.equal(a, b * f), (f, i)


def test_zz_summary_of_error_to_bound_ratios():
    """The worst error-to-bound ratio per stage and tensor over the cases above that ran in this process (the table of DESIGN.md section 5, 'value side';
    profiles/value_fp64_ratios.txt is this output on an MI355X)."""
    worst = {}
    for cid, r in _ratios.items():
        side = 'g_hxi' if cid.startswith('g_hxi') else 'value'
        for key, v in r.items():
            key = (side,) + key
            if key not in worst or v > worst[key][0]:
                worst[key] = (v, cid)
    print('\nside   stage    tensor  worst |error| / bound   case  (%d cases)' % len(_ratios))
    order = {s: i for i, s in enumerate(VC.STAGES + GH_STAGES)}
    for key in sorted(worst, key=lambda k: (k[0] != 'value', order[k[1]], k[2])):
        print('%-6s %-8s %-6s  %-8.3g               %s' % (key[0], key[1], key[2], worst[key][0], worst[key][1]))
    assert all(v[0] <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v[0] <= 1.0}
