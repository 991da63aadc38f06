"""GPU (MI355X): the fused clip + Adam family -- dpn_clip_adam, dpn_clip_adam_flat, dpn_clip_adam_flat_dev -- through the C ABI against the
fp64 evaluation of its definition (tests/optim_cases.py), over the whole surface of the ABI: one to three tables of either layout, every chunk
edge, both alignment paths of dpn_gradnorm_kernel and dpn_adam_kernel, grad_scale, step counters up to 100 000, the eps regime, zeros, a NULL
out_norm and every refusal.

Pass conditions: p, m, v and out_norm inside the derived bounds of optim_cases.py (nothing measured); bit-exact identities between the three
forms, for power-of-two gradient scalings and for one list cut into 161 tensors; every p, g, m, v sits in a window of an owned arena whose
guards are a sentinel bit pattern (NaN around the read-only g), the padding of the flat moment buffers included.  Every (case, form) is
launched once and its result shared by the tests that need it.
"""
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as O

pytestmark = pytest.mark.gpu

STEP_GUARD = -559038737           # 0xDEADBEEF around the int step counter
_RATIOS = {}                      # largest error / bound per quantity over everything this module ran: printed, never asserted


def _dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    print('\noptim bound ratios (largest error / bound): ' + ', '.join('%s %.3f' % (k, v) for k, v in sorted(_RATIOS.items())))


def _note(r):
    for k, x in r.items():
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), x)


class _Run:
    """One step's state on the device: an arena per role (the flat forms: two flat moment buffers), scratch of exactly
    dpn_clip_adam_scratch_doubles doubles, the step counter and out_norm, each inside guards."""

    def __init__(self, inp, shifts, form):
        self.inp, self.form, self.n = inp, form, len(inp.numels)
        dev = _dev()
        self.P = O.Arena(inp.p, [s[0] for s in shifts], O.SENTINEL)
        self.G = O.Arena(inp.g, [s[1] for s in shifts], np.nan)
        if form == 'ptr':
            self.M = O.Arena(inp.m, [s[2] for s in shifts], O.SENTINEL)
            self.V = O.Arena(inp.v, [s[3] for s in shifts], O.SENTINEL)
        else:
            self.M, self.V = O.flat_arena(inp.m, inp.numels), O.flat_arena(inp.v, inp.numels)
        self.d = {k: torch.from_numpy(getattr(self, k).full).to(dev) for k in 'PGMV'}
        self.n_scratch = O.scratch_doubles(inp.numels)
        s64 = np.array([O.SENTINEL64_BITS], np.uint64).view(np.float64)[0]
        self.scratch0 = np.full(self.n_scratch + 2 * O.GUARD, s64, np.float64)
        self.step0 = np.full(9, STEP_GUARD, np.int32)
        self.step0[4] = inp.t - 1
        self.norm0 = np.full(2 * O.GUARD + 1, O.SENTINEL, np.float32)
        h = inp.hyper
        self.hyper = [h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], h['max_norm']]
        self.d.update(scratch=torch.from_numpy(self.scratch0).to(dev), step=torch.from_numpy(self.step0).to(dev),
                      norm=torch.from_numpy(self.norm0).to(dev), hyper=torch.tensor(self.hyper + [inp.gs], dtype=torch.float32, device=dev))
        assert all(t.data_ptr() % 16 == 0 for t in self.d.values())
        arr = lambda k, a: (ctypes.c_void_p * self.n)(*[self.d[k].data_ptr() + 4 * o for o in a.offsets])
        self.args = dict(params=arr('P', self.P), grads=arr('G', self.G), numel=(ctypes.c_int64 * self.n)(*inp.numels),
                         scratch=ctypes.c_void_p(self.d['scratch'].data_ptr() + 8 * O.GUARD), step=ctypes.c_void_p(self.d['step'].data_ptr() + 16),
                         norm=ctypes.c_void_p(self.d['norm'].data_ptr() + 4 * O.GUARD), hyper=ctypes.c_void_p(self.d['hyper'].data_ptr()))
        if form == 'ptr':
            self.args.update(m=arr('M', self.M), v=arr('V', self.V))
        else:
            self.args.update(m=ctypes.c_void_p(self.d['M'].data_ptr() + 4 * O.GUARD), v=ctypes.c_void_p(self.d['V'].data_ptr() + 4 * O.GUARD))

    def launch(self, n_tensors=None, **override):
        """The entry point of this form; override: argument name -> value (None: a NULL pointer)."""
        from deepphysinet_amd import _lib
        lib = _lib.load()
        a = dict(self.args, **override)
        n = self.n if n_tensors is None else n_tensors
        stream = torch.cuda.current_stream().cuda_stream
        if self.form == 'ptr':
            return lib.dpn_clip_adam(n, a['params'], a['grads'], a['m'], a['v'], a['numel'], a['scratch'], a['step'], *self.hyper, a['norm'], stream)
        if self.form == 'flat':
            return lib.dpn_clip_adam_flat(n, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], *self.hyper, a['norm'], stream)
        return lib.dpn_clip_adam_flat_dev(n, a['params'], a['grads'], a['numel'], a['m'], a['v'], a['scratch'], a['step'], a['hyper'], a['norm'], stream)

    def set_gradients(self, g):
        full = self.G.full.copy()
        for o, x in zip(self.G.offsets, g):
            full[o:o + len(x)] = x
        self.G.full = full
        self.d['G'].copy_(torch.from_numpy(full))

    def fetch(self):
        torch.cuda.synchronize()
        host = {k: self.d[k].cpu().numpy() for k in ('P', 'G', 'M', 'V', 'scratch', 'step', 'norm')}
        scratch_bits, s0 = host['scratch'].view(np.uint64), self.scratch0.view(np.uint64)
        return dict(p=[w.copy() for w in self.P.windows(host['P'])], m=[w.copy() for w in self.M.windows(host['M'])],
                    v=[w.copy() for w in self.V.windows(host['V'])], norm=float(host['norm'][O.GUARD]), norm_bits=host['norm'][O.GUARD:O.GUARD + 1].copy(),
                    step=int(host['step'][4]),
                    guards=dict(p=self.P.outside_kept(host['P']), m=self.M.outside_kept(host['M']), v=self.V.outside_kept(host['V']),
                                g=O.bits_equal(host['G'], self.G.full),
                                scratch=bool((scratch_bits[:O.GUARD] == s0[:O.GUARD]).all() and (scratch_bits[-O.GUARD:] == s0[-O.GUARD:]).all()),
                                step=bool((np.delete(host['step'], 4) == STEP_GUARD).all()),
                                norm=O.is_sentinel(np.delete(host['norm'], O.GUARD))),
                    untouched=dict(p=O.bits_equal(host['P'], self.P.full), m=O.bits_equal(host['M'], self.M.full), v=O.bits_equal(host['V'], self.V.full),
                                   scratch=bool((scratch_bits == s0).all()), step=bool((host['step'] == self.step0).all()),
                                   norm=O.is_sentinel(host['norm'])))


_RESULTS = {}


def _result(name, form):
    """(rc, fetched state) of a case in a form: launched once, shared, never written to."""
    if (name, form) not in _RESULTS:
        case = O.case_by_name(name)
        run = _Run(O.built(name)[0], O.shifts_of(case, form), form)
        rc = run.launch()
        _RESULTS[(name, form)] = (rc, run.fetch())
    return _RESULTS[(name, form)]


def _assert_guards(got, what):
    for k, kept in got['guards'].items():
        assert kept, '%s: a store outside the windows of %s (or into the read-only gradients)' % (what, k)


def _assert_inside_bounds(inp, ref, got, what):
    r = O.ratios(inp, ref, got)
    _note(r)
    for k in ('norm', 'm', 'v', 'p'):
        assert r[k] <= 1.0, (what, k, r)


def _same(a, b, what, norm=True):
    for k in 'pmv':
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert O.bits_equal(x, y), (what, k, 'tensor', i)
    if norm:
        assert O.bits_equal(a['norm_bits'], b['norm_bits']), (what, 'out_norm', a['norm'], b['norm'])


ALL = [pytest.param(c.name, f, id='%s-%s' % (c.name, f)) for c in O.CASES for f in c.forms]


# ---------------------------------------------------------------------------------------------- the table against fp64
@pytest.mark.parametrize('name,form', ALL)
def test_entry_point_is_inside_the_fp64_bounds(name, form):
    """p, m, v and out_norm inside the derived bounds, the step counter bumped once whatever the number of tables, every guard, the flat
    padding and the gradients bit-identical to what was uploaded."""
    case = O.case_by_name(name)
    inp, ref = O.built(name)
    rc, got = _result(name, form)
    assert rc == 0
    assert got['step'] == inp.t
    _assert_guards(got, (name, form))
    _assert_inside_bounds(inp, ref, got, (name, form))
    if case.kind == 'Z':                                      # 0 / (0 + eps): zero tensors among nonzero ones come back as they went in
        for i in range(1, len(inp.numels), 2):
            assert O.bits_equal(got['p'][i], inp.p[i]) and O.bits_equal(got['m'][i], inp.m[i]) and O.bits_equal(got['v'][i], inp.v[i]), (name, i)
    if case.kind == 'I' and case.gs == 1.0:                   # an exact sum of squares in any order: the correctly rounded norm
        assert got['norm'] == float(np.float32(np.sqrt(ref['S']))), (name, got['norm'])


# ---------------------------------------------------------------------------------------------- identities between the forms
GS1 = [c.name for c in O.CASES if c.gs == 1.0]


@pytest.mark.parametrize('name', GS1)
def test_flat_by_value_equals_flat_dev_with_unit_grad_scale(name):
    _same(_result(name, 'flat')[1], _result(name, 'dev')[1], name)


@pytest.mark.parametrize('name', [n for n in GS1 if O.case_by_name(n).place != 'mixed'])
def test_pointer_form_equals_flat_form(name):
    """Same windows for p and g, the moments in per-tensor windows against the flat buffers.  Only where both forms take the same path of
    dpn_adam_kernel for every tensor: the 16-byte loop and the scalar loop are separate code that a compiler may contract differently, and the
    'mixed' placement moves m or v alone, which sends the pointer form down the scalar loop and the flat form down the other."""
    case = O.case_by_name(name)
    assert O.path_of(case, 'ptr') == O.path_of(case, 'flat')
    _same(_result(name, 'ptr')[1], _result(name, 'flat')[1], name)


@pytest.mark.parametrize('a,b', O.I_PAIRS)
def test_gradients_times_8_with_grad_scale_one_eighth_are_bit_identical(a, b):
    """Every scaling is a power of two: the _dev form gives the same p, m, v and out_norm bits."""
    _same(_result(a, 'dev')[1], _result(b, 'dev')[1], (a, b))


@pytest.mark.parametrize('form', O.FORMS)
@pytest.mark.parametrize('name', ['w_list161_aligned', 'i_list161'])
def test_list_cut_into_161_tensors_equals_one_tensor(name, form):
    """The same numbers as ONE tensor in ONE table.  The W case runs with the clip inactive, so coef is exactly 1 whatever the order the squares
    were added in and every element must agree; out_norm is compared where the sum of squares is exact (kind I)."""
    case = O.case_by_name(name)
    inp, ref = O.built(name)
    assert case.kind == 'I' or ref['coef'] == 1.0
    cat = lambda xs: [np.concatenate(xs)]
    one = O.Inputs((sum(inp.numels),), cat(inp.p), cat(inp.g), cat(inp.m), cat(inp.v), inp.hyper, inp.gs, inp.t)
    run = _Run(one, [(0, 0, 0, 0)], form)
    assert run.launch() == 0
    got = run.fetch()
    _assert_guards(got, (name, form, 'one tensor'))
    split = _result(name, form)[1]
    _same({k: cat(split[k]) for k in 'pmv'} | dict(norm_bits=split['norm_bits'], norm=split['norm']), got, (name, form), norm=case.kind == 'I')


# ---------------------------------------------------------------------------------------------- out_norm_dev = NULL, two steps
@pytest.mark.parametrize('form', O.FORMS)
def test_null_out_norm_changes_nothing_else(form):
    name = 'w_list161_shifted'
    run = _Run(O.built(name)[0], O.shifts_of(O.case_by_name(name), form), form)
    assert run.launch(norm=None) == 0
    got = run.fetch()
    assert got['untouched']['norm'] and got['step'] == O.built(name)[0].t
    _assert_guards(got, (name, form))
    _same(got, _result(name, form)[1], (name, form), norm=False)


@pytest.mark.parametrize('place', ['aligned', 'shifted'])
@pytest.mark.parametrize('form', O.FORMS)
def test_two_consecutive_steps_on_one_state(form, place):
    """t = 1 then 2 with new gradients: the second launch must read the moments (nontemporal stores) and parameters the first one wrote.  The
    second reference step starts from the fp32 state the first launch left, so each step is held to the one-step bounds."""
    name = 'u_t1_test' if place == 'aligned' else 'u_t1_offdefault'
    case = O.case_by_name(name)
    assert case.t == 1 and case.place == place
    inp, ref = O.built(name)
    run = _Run(inp, O.shifts_of(case, form), form)
    assert run.launch() == 0
    first = run.fetch()
    _assert_inside_bounds(inp, ref, first, (name, form, 'step 1'))
    rng = np.random.default_rng(7)
    g2 = [(g * rng.uniform(0.5, 2.0, size=len(g)) * rng.choice([-1.0, 1.0], size=len(g))).astype(np.float32) for g in inp.g]
    run.set_gradients(g2)
    assert run.launch() == 0
    second = run.fetch()
    inp2 = O.Inputs(inp.numels, first['p'], g2, first['m'], first['v'], inp.hyper, inp.gs, 2)
    assert second['step'] == 2
    _assert_guards(second, (name, form, 'step 2'))
    _assert_inside_bounds(inp2, O.reference(inp2), second, (name, form, 'step 2'))


# ---------------------------------------------------------------------------------------------- refusals
def _refusals():
    out = []
    for form in O.FORMS:
        moments = ('m', 'v')
        for arg in ('params', 'grads', 'numel', 'scratch', 'step') + moments + (('hyper',) if form == 'dev' else ()):
            out.append(pytest.param(form, 'null_' + arg, id='%s-null_%s' % (form, arg)))
        for why in ('n_tensors_0', 'numel_0_first', 'numel_0_last_table', 'numel_2^31_first', 'numel_2^31_last_table'):
            out.append(pytest.param(form, why, id='%s-%s' % (form, why)))
    return out


@pytest.mark.parametrize('form,why', _refusals())
def test_refusal_returns_minus_one_and_writes_nothing(form, why):
    """-1, and after it every buffer -- parameters, moments, scratch, out_norm and the step counter -- holds the bits that were uploaded.  A bad
    size in the LAST table is refused before the launches of the tables in front of it."""
    name = 'w_list73_aligned' if form == 'ptr' else 'w_list161_aligned'
    case = O.case_by_name(name)
    run = _Run(O.built(name)[0], O.shifts_of(case, form), form)
    if why.startswith('null_'):
        rc = run.launch(**{why[5:]: None})
    elif why == 'n_tensors_0':
        rc = run.launch(n_tensors=0)
    else:
        numel = list(case.numels)
        assert len(O.table_starts(len(numel), O.PTR_TABLE if form == 'ptr' else O.FLAT_TABLE)) == 2
        numel[0 if why.endswith('first') else -1] = 0 if why.startswith('numel_0') else 2 ** 31       # a host-side value only: nothing is launched
        rc = run.launch(numel=(ctypes.c_int64 * len(numel))(*numel))
    got = run.fetch()
    assert rc == -1
    assert all(got['untouched'].values()) and got['guards']['g'], (form, why, got['untouched'])
    assert got['step'] == case.t - 1


# ---------------------------------------------------------------------------------------------- the host path training takes
def test_fused_clip_adam_optimizer_on_an_update_resolved_case():
    """FusedClipAdam (dpn_clip_adam_flat_dev on its own flat buffers) with step_count preset to 999 and grad_scale = 1/3."""
    from deepphysinet_amd.optim import FusedClipAdam
    name = 'u_t1000_gs3'
    case = O.case_by_name(name)
    inp, ref = O.built(name)
    assert case.kind == 'U' and inp.t == 1000 and inp.gs == O.f32(1.0 / 3)
    dev, h = _dev(), inp.hyper
    params = [torch.from_numpy(p).to(dev).requires_grad_(True) for p in inp.p]
    opt = FusedClipAdam(params, lr=h['lr'], betas=(h['b1'], h['b2']), eps=h['eps'], weight_decay=h['wd'], max_norm=h['max_norm'])
    opt.step_count.fill_(999)
    opt.grad_scale = 1.0 / 3
    for p, g, m, v, em, ev in zip(params, inp.g, inp.m, inp.v, opt.exp_avg, opt.exp_avg_sq):
        p.grad = torch.from_numpy(g).to(dev)
        em.copy_(torch.from_numpy(m)); ev.copy_(torch.from_numpy(v))
    norm = opt.step()
    torch.cuda.synchronize()
    got = dict(p=[p.detach().cpu().numpy() for p in params], m=[m.cpu().numpy() for m in opt.exp_avg], v=[v.cpu().numpy() for v in opt.exp_avg_sq],
               norm=float(norm))
    assert int(opt.step_count) == 1000
    _assert_inside_bounds(inp, ref, got, name)
    assert all(O.bits_equal(p.grad.cpu().numpy(), g) for p, g in zip(params, inp.g))
    flat_m = opt._m_flat.cpu().numpy()                       # the padding of the optimiser's own flat buffers stays zero
    inside = np.zeros(len(flat_m), bool)
    for o, k in zip(O.flat_offsets(inp.numels), inp.numels):
        inside[o:o + k] = True
    assert not flat_m[~inside].any() and not opt._v_flat.cpu().numpy()[~inside].any()
