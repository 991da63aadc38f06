"""No GPU: the host side of the L-BFGS refinement (deepphysinet_amd/lbfgs.py) -- the small-space recursion against the classical two-loop recursion,
the strong-Wolfe search on 1-D functions, the whole loop against torch.optim.LBFGS, the seeded mistakes, the state struct's layout against gcc, the
refusals of the C ABI and of the host class that need no device, the option's way through the loops and train.py's flags, and the build wiring."""
import ctypes
import math
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import lbfgs_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def LB():
    from deepphysinet_amd import lbfgs
    return lbfgs


# ---------------------------------------------------------------------------------------------- small-space recursion
def classical_two_loop(S, Y, g):
    """The textbook recursion on the vectors themselves (pairs oldest first), fp64: d = -H g."""
    q = g.copy()
    k = len(S)
    al = [0.0] * k
    for i in range(k - 1, -1, -1):
        al[i] = float(S[i] @ q) / float(S[i] @ Y[i])
        q = q - al[i] * Y[i]
    r = q * (float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])) if k else q
    for i in range(k):
        be = float(Y[i] @ r) / float(S[i] @ Y[i])
        r = r + S[i] * (al[i] - be)
    return -r


def spd_pairs(n, k, cond, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, min(n, 64))))
    lam = np.logspace(0, math.log10(cond), Q.shape[1])
    A = lambda v: v + Q @ ((lam - 1.0) * (Q.T @ v))                  # SPD, eigenvalues in [1, cond]
    S = [rng.standard_normal(n) for _ in range(k)]
    return S, [A(s) for s in S], rng.standard_normal(n)


def small_space(S, Y, g, m, newest, mistake=None, pending=0):
    """The pairs (oldest first) laid into a ring of m slots whose newest pair sits in slot `newest`; coefficients + direction in fp64."""
    lb = LB()
    k = len(S)
    st = dict(lb.zero_state(), count=k, newest=newest, pending=pending)
    vec = [None] * (2 * m + 1)
    for i in range(k):
        sl = (newest - (k - 1 - i)) % m
        vec[sl], vec[m + sl] = S[i], Y[i]
    vec[2 * m] = g
    G = np.zeros((2 * m + 1, 2 * m + 1))
    for a in range(2 * m + 1):
        for b in range(2 * m + 1):
            if vec[a] is not None and vec[b] is not None:
                G[a, b] = float(vec[a] @ vec[b])
    delta, st2 = lb.coefficients(G, st, m, mistake)
    order = lb.basis_order(st2, m, mistake)
    return lb.direction([vec[b] for b in order], delta[order], np.float64), delta, st2, G


@pytest.mark.parametrize('cond', (10.0, 1e4))
@pytest.mark.parametrize('n', (50, 4096))
@pytest.mark.parametrize('k', (1, 3, 10, 20))
def test_small_space_recursion_is_the_classical_two_loop(n, k, cond):
    """Relative 2-norm difference <= 1e-12 (observed here: at most 2e-15 over these cases), also with the ring wrapped (newest slot in the middle)."""
    S, Y, g = spd_pairs(n, k, cond, 1000 * k + n)
    want = classical_two_loop(S, Y, g)
    for m, newest in ((k, k - 1), (k, k // 2), (k + 2, 0)):
        got, delta, st, G = small_space(S, Y, g, m, newest)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= 1e-12, (m, newest, rel)
        assert abs(st['gtd'] - float(g @ want)) <= 1e-10 * abs(float(g @ want))
        assert abs(st['dnorm'] - np.linalg.norm(want)) <= 1e-10 * np.linalg.norm(want)
        assert st['iters'] == 1 and st['skipped'] == 0 and st['count'] == k


def test_no_pair_gives_steepest_descent_and_a_refused_pair_steps_the_ring_back():
    lb = LB()
    S, Y, g = spd_pairs(64, 3, 10.0, 5)
    got, delta, st, _ = small_space([], [], g, 3, 0)
    assert np.array_equal(got, -g) and st['gamma'] == 1.0 and st['gtd'] == -float(g @ g)
    # the newest pair pending with s.y <= 1e-10: the direction is the one of the two older pairs
    Yb = Y[:2] + [-Y[2]]
    want = classical_two_loop(S[:2], Y[:2], g)
    got, delta, st, _ = small_space(S, Yb, g, 3, 1, pending=1)
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    assert (st['count'], st['newest'], st['skipped'], st['pending']) == (2, 0, 1, 0)
    # ... a positive s.y just under the threshold too, and a standing pair stays
    tiny = [S[2] * 0 + 0.999e-5 / math.sqrt(64.0)]
    _, _, st, G = small_space(S[:2] + tiny, Y[:2] + tiny, g, 3, 2, pending=1)
    assert G[2, 5] <= 1e-10 and st['skipped'] == 1
    _, _, st, _ = small_space(S, Y, g, 3, 2, pending=1)
    assert st['skipped'] == 0 and st['count'] == 3 and st['pending'] == 0


# ---------------------------------------------------------------------------------------------- strong Wolfe
def wolfe_holds(f, df, f0, g0, t, c1=1e-4, c2=0.9):
    return f(t) <= f0 + c1 * t * g0 and abs(df(t)) <= -c2 * g0


LINE_FUNCTIONS = {
    'quadratic': (lambda t: (t - 2.0) ** 2, lambda t: 2.0 * (t - 2.0)),
    'quartic': (lambda t: (t - 1.0) ** 4 + 0.1 * t * t - 0.3 * t, lambda t: 4.0 * (t - 1.0) ** 3 + 0.2 * t - 0.3),
    'steep_then_flat': (lambda t: math.exp(-5.0 * t) + 0.01 * t * t, lambda t: -5.0 * math.exp(-5.0 * t) + 0.02 * t),
    'cosine': (lambda t: -math.sin(t) + 0.05 * t * t, lambda t: -math.cos(t) + 0.1 * t),
}


@pytest.mark.parametrize('name', sorted(LINE_FUNCTIONS))
@pytest.mark.parametrize('t0', (1e-3, 1.0, 40.0))
def test_strong_wolfe_returns_a_point_that_satisfies_both_conditions(name, t0):
    f, df = LINE_FUNCTIONS[name]
    t, ft, gt, evals, status = LB().strong_wolfe(lambda t: (f(t), df(t)), f(0.0), df(0.0), t0)
    assert status in LB().LS_STATUS
    if status == 'wolfe':
        assert wolfe_holds(f, df, f(0.0), df(0.0), t) and ft == f(t) and gt == df(t)
    else:                                               # the status says why not; the decrease condition holds all the same
        assert status in ('bracket_small', 'max_ls') and f(t) <= f(0.0) + 1e-4 * t * df(0.0)
    assert 1 <= evals <= 26
    assert status == 'wolfe'                            # (all twelve do reach a Wolfe point)


@pytest.mark.parametrize('bad', (float('inf'), float('nan')))
def test_strong_wolfe_treats_a_non_finite_trial_as_overshoot(bad):
    """phi is not finite beyond the radius 0.7; the minimum of the finite part lies at 0.5."""
    f = lambda t: (t - 0.5) ** 2 if t <= 0.7 else bad
    df = lambda t: 2.0 * (t - 0.5) if t <= 0.7 else bad
    seen = []

    def phi(t):
        seen.append(t)
        return f(t), df(t)
    for t0 in (1.0, 64.0):
        t, ft, gt, evals, status = LB().strong_wolfe(phi, f(0.0), df(0.0), t0)
        assert 0.0 < t <= 0.7 and math.isfinite(ft) and ft < f(0.0) and status == 'wolfe'
    # the slope alone not finite counts too
    t, ft, gt, evals, status = LB().strong_wolfe(lambda t: ((t - 0.5) ** 2, 2.0 * (t - 0.5) if t <= 0.7 else bad), 0.25, -1.0, 1.0)
    assert 0.0 < t <= 0.7 and status == 'wolfe'


def test_strong_wolfe_fails_with_t_zero_when_nothing_finite_lowers_f():
    lb = LB()
    t, ft, gt, evals, status = lb.strong_wolfe(lambda t: (float('inf'), float('nan')), 1.0, -1.0, 1.0)
    assert (t, ft, gt, status) == (0.0, 1.0, -1.0, 'ls_failed') and evals == 26
    # a slope that lies (the function rises although gtd0 < 0): no trial satisfies the decrease condition
    t, ft, gt, evals, status = lb.strong_wolfe(lambda t: (1.0 + t, 1.0), 1.0, -1.0, 1.0)
    assert t == 0.0 and status == 'ls_failed'


# ---------------------------------------------------------------------------------------------- the loop against torch
def rosenbrock_pairs(x):
    x = np.asarray(x, np.float64)
    a, b = x[::2], x[1::2]
    g = np.zeros_like(x)
    g[::2] = -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[1::2] = 200.0 * (b - a * a)
    return float(np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2)), g


def rosenbrock_chain(x):
    x = np.asarray(x, np.float64)
    a, b = x[:-1], x[1:]
    g = np.zeros_like(x)
    g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[1:] += 200.0 * (b - a * a)
    return float(np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2)), g


QUAD = np.logspace(0, 2, 64)


def quadratic(x):
    x = np.asarray(x, np.float64)
    return float(0.5 * np.sum(QUAD * x * x)), QUAD * x


def torch_form(name, x):
    if name == 'rosenbrock2':
        return (100.0 * (x[1::2] - x[::2] ** 2) ** 2 + (1.0 - x[::2]) ** 2).sum()
    if name == 'rosenbrock10':
        return (100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2).sum()
    return 0.5 * (torch.from_numpy(QUAD) * x * x).sum()


PROBLEMS = {'rosenbrock2': (rosenbrock_pairs, np.array([-1.2, 1.0])), 'rosenbrock10': (rosenbrock_chain, np.array([-1.2, 1.0] * 5)),
            'quadratic64': (quadratic, np.cos(np.arange(64.0)) + 1.5)}


def run_torch(name, **opts):
    x = torch.tensor(PROBLEMS[name][1], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([x], line_search_fn='strong_wolfe', **opts)
    losses = []

    def closure():
        opt.zero_grad()
        loss = torch_form(name, x)
        loss.backward()
        losses.append(float(loss.detach()))
        return loss
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        opt.step(closure)
    with torch.no_grad():
        final = float(torch_form(name, x))
    return losses, final, opt.state[x]['func_evals']


def run_ours(name, mistake=None, **opts):
    trace = []
    fun, x0 = PROBLEMS[name]
    x, last = LB().lbfgs_reference(fun, x0, dtype=np.float64, mistake=mistake, trace=trace, **opts)
    return [last['f0']] + [f for _, f in trace], last


def worst_relative(mine, theirs):
    k = min(len(mine), len(theirs))
    return max(abs(a - b) / abs(b) for a, b in zip(mine[:k], theirs[:k])), k


FIVE = dict(lr=1.0, max_iter=5, max_eval=1000, history_size=3, tolerance_grad=1e-9, tolerance_change=1e-14)


@pytest.mark.parametrize('name', ('rosenbrock2', 'quadratic64'))
def test_first_five_iterations_agree_with_torch(name):
    """Every closure evaluation of the first five iterations (history_size 3, so the ring wraps at the fourth pair) gives torch's loss to 1e-6
    relative.  The two differ in summation order only.  Observed on the CPU: rosenbrock2 5.1e-16 (7 evaluations), quadratic64 1.1e-15 (8 evaluations) -- rounding; an algorithmic
    difference shows as 1e-2 (the seeded mistakes below)."""
    theirs, _, evals = run_torch(name, **FIVE)
    mine, last = run_ours(name, **FIVE)
    rel, k = worst_relative(mine, theirs)
    print('%s: %d evaluations, worst relative difference %.3g' % (name, k, rel))
    assert len(mine) == len(theirs) == evals == last['evals'] and last['iters'] == 5
    assert rel <= 1e-6
    assert rel <= 1e-9, 'more than rounding: an algorithmic difference to be found'


FULL = dict(lr=1.0, max_iter=500, max_eval=100000, history_size=10, tolerance_grad=1e-9, tolerance_change=1e-14)


@pytest.mark.parametrize('name', ('rosenbrock2', 'rosenbrock10'))
def test_full_runs_reach_the_minimum_within_twice_torchs_evaluations(name):
    """torch on the CPU: rosenbrock2 45 evaluations, f = 6.8e-17; rosenbrock10 (the chained form from (-1.2, 1) x 5) 91 evaluations, f = 5.7e-15.
    Observed here: 45 evaluations, 36 iterations, f = 6.8e-17; 91 evaluations, 78 iterations, f = 6.0e-15 (tolerance_grad 1e-9, tolerance_change
    1e-14: with torch's defaults both implementations stop near 1e-10 on the change rule)."""
    theirs, final, evals = run_torch(name, **FULL)
    mine, last = run_ours(name, **FULL)
    print('%s: torch %d evaluations f = %.3g; here %d evaluations, %d iterations, f = %.3g, %s' % (name, evals, final, last['evals'], last['iters'],
                                                                                                    last['f'], last['status']))
    assert final < 1e-10
    assert last['f'] < 1e-10 and last['evals'] <= 2 * evals
    assert last['status'] in ('tolerance_change', 'tolerance_grad')


# ---------------------------------------------------------------------------------------------- seeded mistakes
def caught_by_torch(mistake):
    for name in ('rosenbrock2', 'quadratic64'):
        theirs, _, _ = run_torch(name, **FIVE)
        mine, last = run_ours(name, mistake=mistake, **FIVE)
        if len(mine) != len(theirs) or worst_relative(mine, theirs)[0] > 1e-6:
            return True
    return False


def caught_by_classical(mistake):
    S, Y, g = spd_pairs(50, 3, 1e4, 3050)
    want = classical_two_loop(S, Y, g)
    got = small_space(S, Y, g, 3, 1, mistake)[0]                     # a wrapped ring
    return np.linalg.norm(got - want) > 1e-12 * np.linalg.norm(want)


def caught_by_refused_pair(mistake):
    S, Y, g = spd_pairs(64, 3, 10.0, 5)
    want = classical_two_loop(S[:2], Y[:2], g)
    got, _, st, _ = small_space(S, Y[:2] + [-Y[2]], g, 3, 1, mistake, pending=1)
    return st['skipped'] != 1 or np.linalg.norm(got - want) > 1e-12 * np.linalg.norm(want)


CAUGHT_BY = {'no_gamma_scale': (caught_by_classical, caught_by_torch), 'ring_order': (caught_by_classical, caught_by_torch),
             'skip_ignored': (caught_by_refused_pair,), 'move_incremental': (caught_by_torch,), 'alpha_sign': (caught_by_classical, caught_by_torch),
             'stale_g_prev': (caught_by_torch,)}


def test_every_seeded_mistake_is_caught():
    lb = LB()
    assert set(CAUGHT_BY) == set(lb.MISTAKES)
    assert {'no_gamma_scale', 'ring_order', 'skip_ignored', 'move_incremental', 'alpha_sign', 'stale_g_prev'} <= set(lb.MISTAKES)
    for mistake, checks in CAUGHT_BY.items():
        for check in checks:
            assert check(mistake), (mistake, check.__name__)
    for check in (caught_by_classical, caught_by_torch, caught_by_refused_pair):
        assert not check(None), check.__name__


# ---------------------------------------------------------------------------------------------- restatements on the case table
@pytest.mark.parametrize('name', ('small', 'chunks'))
def test_gram_restatement_is_within_the_fp64_bound_of_the_exact_sums(name):
    """gram_partials + gram_reduce against math.fsum of the fp64 products: |error| <= 2 N 2^-53 sum |a_i| |b_i|, the bound for fp64 accumulation of
    exact products; and the table is laid out as the header says."""
    lb = LB()
    tl, m = LC.tensor_list(name), 3
    lay = lb.Layout(tl.numels)
    assert lay.total == LC.total_floats(tl.numels)
    seq = LC.push_sequence(tl.numels, m, m + 2, 11)
    S, Y = np.zeros((m, lay.total), np.float32), np.zeros((m, lay.total), np.float32)
    g_prev, st, G = lay.pack(seq[0].g), lb.zero_state(), np.zeros((2 * m + 1) ** 2)
    for p in seq[1:]:
        g = lay.pack(p.g)
        st = lb.push(g, g_prev, lay.pack(p.d), p.t, S, Y, st, m, lay.mask)
        G, st = lb.gram_reduce(lb.gram_partials(S, Y, g, lay, m, st), G, m, st)
        _, st = lb.coefficients(G, st, m)
    vec = lambda b: g if b == 2 * m else (S[b] if b < m else Y[b - m])
    N = sum(tl.numels)
    for a in lb.basis_order(st, m):
        for b in lb.basis_order(st, m):
            x, y = vec(a)[lay.mask].astype(np.float64), vec(b)[lay.mask].astype(np.float64)
            exact = math.fsum((x * y).tolist())
            assert abs(G[a, b] - exact) <= 2 * N * 2.0 ** -53 * math.fsum(np.abs(x * y).tolist()), (a, b)
    assert st['g_l1'] == pytest.approx(math.fsum(np.abs(g[lay.mask].astype(np.float64)).tolist()), rel=1e-12)
    assert st['g_inf'] == float(np.abs(g[lay.mask]).max()) and st['count'] == m


def test_move_restores_x0_bit_for_bit_and_push_leaves_the_padding():
    lb = LB()
    lay = lb.Layout((3, 2049))
    x0 = lay.pack([np.array([-0.0, 1.0, 2.0], np.float32), np.linspace(-1, 1, 2049).astype(np.float32)])
    d = lay.pack([np.array([np.inf, 1.0, -2.0], np.float32), np.ones(2049, np.float32)])
    assert np.array_equal(lb.move(x0, d, 0.0).view(np.uint32), x0.view(np.uint32))
    assert np.array_equal(lb.move(x0, d, 0.5)[1:3], np.float32([1.5, 1.0]))
    S, Y = np.full((2, lay.total), 7, np.float32), np.full((2, lay.total), 7, np.float32)
    g, g_prev = lay.pack([np.ones(3, np.float32), np.ones(2049, np.float32)]), np.full(lay.total, 5, np.float32)
    st = lb.push(g, g_prev, d, 0.25, S, Y, lb.zero_state(), 2, lay.mask)
    assert (st['count'], st['newest'], st['pending']) == (1, 1, 1)
    assert np.all(S[1][~lay.mask] == 7) and np.all(Y[1][~lay.mask] == 7) and np.all(g_prev[~lay.mask] == 5) and np.all(S[0] == 7)
    assert np.array_equal(Y[1][lay.mask], np.full(2052, -4, np.float32)) and np.array_equal(g_prev[lay.mask], g[lay.mask])


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU
def test_state_struct_has_the_c_compilers_layout(tmp_path):
    from deepphysinet_amd import _lib
    st = _lib.DpnLbfgsState
    assert tuple(f[0] for f in st._fields_) == LB().FIELDS and ctypes.sizeof(st) == 72
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpn_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(DpnLbfgsState));']
    lines += ['  printf("%s %%zu\\n", offsetof(DpnLbfgsState, %s));' % (f[0], f[0]) for f in st._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'lbfgs_layout.c', tmp_path / 'lbfgs_layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    want = dict({f[0]: getattr(st, f[0]).offset for f in st._fields_}, size=ctypes.sizeof(st))
    assert got == want
    assert want['gamma'] == 24 and want['gg'] == 64                     # what FusedLBFGS.lbfgs_state reads as fp64 words 3 .. 8


ENTRIES = ('dpn_lbfgs_scratch_doubles', 'dpn_lbfgs_save', 'dpn_lbfgs_move', 'dpn_lbfgs_push', 'dpn_lbfgs_gram', 'dpn_lbfgs_gtd', 'dpn_lbfgs_direction')


def test_symbols_are_declared_exported_and_bound_and_the_inc_is_built_in():
    from deepphysinet_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'^(int|int64_t)\s+%s\s*\(' % name, header, flags=re.M) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert 'typedef struct DpnLbfgsState' in header
    inc = os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_lbfgs.inc')
    assert inc in build.DEPS
    optim = open(os.path.join(ROOT, 'deepphysinet_amd', 'csrc', 'dpn_optim.hip')).read()
    assert optim.rstrip().endswith('#include "dpn_lbfgs.inc"')
    assert len(build.MORE_UNITS) == 1 and not any('lbfgs' in u[0] for u in build.ALL_UNITS)
    assert 'atomic' not in re.sub(r'//.*', '', open(inc).read()).lower()


def test_scratch_size_and_its_refusals():
    from deepphysinet_amd import _lib
    lib = _lib.load()
    for tl in LC.TENSOR_LISTS:
        arr = (ctypes.c_int64 * len(tl.numels))(*tl.numels)
        for m in (1, 3, 32):
            assert lib.dpn_lbfgs_scratch_doubles(len(tl.numels), arr, m) == (3 * (2 * m + 1) + 2) * LC.total_floats(tl.numels) // LC.CHUNK
    one = (ctypes.c_int64 * 1)(5)
    assert lib.dpn_lbfgs_scratch_doubles(0, one, 3) == -1 and lib.dpn_lbfgs_scratch_doubles(1, None, 3) == -1
    assert lib.dpn_lbfgs_scratch_doubles(1, one, 0) == -1 and lib.dpn_lbfgs_scratch_doubles(1, one, 33) == -1


def refusal_calls(a):
    """{why: (entry, args)} from a dict `a` of valid arguments (n, params, numel, the flat buffers x0, d, g, gp, S, Y, scratch, G, delta, out, state,
    m): every entry with every pointer NULL in turn, n_tensors 0, a bad numel, m out of range, a step length that is not finite."""
    f = ctypes.c_float
    calls = {'save': ('dpn_lbfgs_save', ['n', 'params', 'numel', 'x0']),
             'move': ('dpn_lbfgs_move', ['n', 'params', 'numel', 'x0', 'd', ('t', f(0.5))]),
             'push': ('dpn_lbfgs_push', ['n', 'params', 'numel', 'g', 'gp', 'd', ('t', f(0.5)), 'S', 'Y', 'm', 'state']),
             'gram': ('dpn_lbfgs_gram', ['n', 'params', 'numel', 'S', 'Y', 'g', 'm', 'state', 'scratch', 'G']),
             'gtd': ('dpn_lbfgs_gtd', ['n', 'params', 'numel', 'g', 'd', 'scratch', 'out']),
             'direction': ('dpn_lbfgs_direction', ['n', 'params', 'numel', 'S', 'Y', 'g', 'm', 'state', 'G', 'delta', 'd'])}
    out = {}
    for short, (entry, names) in calls.items():
        def args(**override):
            vals = []
            for nm in names:
                key, val = nm if isinstance(nm, tuple) else (nm, a[nm])
                vals.append(override.get(key, val))
            return (entry, tuple(vals) + (None,))
        for nm in names:
            key = nm[0] if isinstance(nm, tuple) else nm
            if key not in ('n', 'm', 't'):
                out['%s_null_%s' % (short, key)] = args(**{key: None})
        out['%s_n_0' % short] = args(n=0)
        out['%s_numel_0' % short] = args(numel=(ctypes.c_int64 * 2)(5, 0))
        out['%s_numel_2^31' % short] = args(numel=(ctypes.c_int64 * 2)(5, 2 ** 31))
        if 'm' in names:
            out['%s_m_0' % short], out['%s_m_33' % short] = args(m=0), args(m=33)
        if short in ('move', 'push'):
            out['%s_t_nan' % short], out['%s_t_inf' % short] = args(t=f(float('nan'))), args(t=f(float('inf')))
    return out


def fake_arguments():
    fake = ctypes.c_void_p(4096)
    return dict(n=2, params=(ctypes.c_void_p * 2)(4096, 8192), numel=(ctypes.c_int64 * 2)(5, 7), m=3,
                **{k: fake for k in ('x0', 'd', 'g', 'gp', 'S', 'Y', 'scratch', 'G', 'delta', 'out', 'state')})


REFUSALS = sorted(refusal_calls(fake_arguments()))


@pytest.mark.parametrize('why', REFUSALS)
def test_refusals_return_minus_one_before_anything_is_launched(why):
    """Made-up addresses: a refusal launches nothing and dereferences no device pointer, so it is safe without a GPU."""
    from deepphysinet_amd import _lib
    entry, args = refusal_calls(fake_arguments())[why]
    assert getattr(_lib.load(), entry)(*args) == -1


# ---------------------------------------------------------------------------------------------- the host class and the loops' option
def test_fused_lbfgs_refuses_what_it_cannot_run():
    lb = LB()
    cpu = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(RuntimeError, match='fp32 HIP parameters'):
        lb.FusedLBFGS(cpu)
    with pytest.raises(RuntimeError, match='fp32 HIP parameters'):
        lb.FusedLBFGS([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match='ema_decay'):
        lb.FusedLBFGS(cpu, ema_decay=0.999)
    with pytest.raises(ValueError, match='agree in every option'):
        lb.FusedLBFGS([dict(params=cpu), dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=0.5)])
    for bad in (dict(history_size=0), dict(history_size=33), dict(history_size=2.5), dict(history='forget'), dict(max_iter=0), dict(lr=0.0),
                dict(lr=float('inf'))):
        with pytest.raises(ValueError):
            lb.FusedLBFGS(cpu, **bad)


def _interface():
    from deepphysinet_amd.configs import ncep_config
    from deepphysinet_amd.interface import builder_models
    return builder_models(**ncep_config())


def test_loop_option_and_its_refusals():
    m = _interface()
    assert m._lbfgs_option({}) is None and m._lbfgs_option({'lbfgs': False}) is None
    assert m._lbfgs_option({'lbfgs': dict(start_epoch=2, history_size=5)}) == dict(start_epoch=2, history_size=5)
    m.train_cfg.setdefault('optimizer', {})['lbfgs'] = dict(start_epoch=1, max_iter=4)
    assert m._lbfgs_option({}) == dict(start_epoch=1, max_iter=4)
    assert m._lbfgs_option({'lbfgs': dict(start_epoch=3)}) == dict(start_epoch=3)          # the keyword wins
    for bad in (dict(history_size=5), dict(start_epoch=-1), dict(start_epoch=1.5), dict(start_epoch=1, clip=3.0)):
        with pytest.raises(ValueError):
            m._lbfgs_option({'lbfgs': bad})
    opt = dict(lbfgs=dict(start_epoch=0), samples=[], num_epoch=1, device='cpu')
    for other in (dict(adaptive_interior=True), dict(causal_weights=dict(eps=1.0)), dict(balance_losses=True), dict(ema_weights=0.999),
                  dict(step_guard=True)):
        with pytest.raises(ValueError, match='lbfgs together with %s' % next(iter(other))):
            m.run_train_interface(**opt, **other)
    with pytest.raises(ValueError, match='reduced\\s+across the ranks'):
        m.run_train_interface_dist(**opt)
    m.train_cfg['optimizer']['step_guard'] = True                                            # from the configuration too
    with pytest.raises(ValueError, match='lbfgs together with step_guard'):
        m.run_train_interface(**opt)


def test_train_py_flags_reach_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_launcher_lbfgs', os.path.join(ROOT, 'train.py'))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    arg = lambda *a: train.lbfgs_arg(train.parse.parse_args(list(a)))
    assert arg() is None
    assert arg('--lbfgs_from', '3') == dict(start_epoch=3)
    assert arg('--lbfgs_from', '0', '--lbfgs_history', '20', '--lbfgs_iters', '8') == dict(start_epoch=0, history_size=20, max_iter=8)
    with pytest.raises(SystemExit):
        arg('--lbfgs_history', '5')
    m = _interface()
    assert m._lbfgs_option({'lbfgs': arg('--lbfgs_from', '1', '--lbfgs_iters', '2')}) == dict(start_epoch=1, max_iter=2)
