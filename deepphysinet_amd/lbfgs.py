"""L-BFGS refinement on the optimiser's flat buffers with a strong-Wolfe line search (the second half of the usual recipe for physics-informed
networks: Adam first, then L-BFGS on a fixed collocation set).

The kernels (csrc/dpn_lbfgs.inc; the contract is the comment of include/dpn_hip.h) restate L-BFGS so that an iteration reads the history twice:
one pass takes every inner product the two-loop recursion needs (the Gram matrix over the basis {stored s, stored y, g}), one thread runs the
recursion on that small matrix in fp64, one more pass forms d = sum_j delta_j b_j ("vector-free" L-BFGS).  The restatement is exact.

This module holds
  * the numpy restatements the GPU tests hold the kernels to, operation for operation: `gram_partials` / `gram_reduce` (thread, lane and wave order
    of the Gram pass), `coefficients` (the scalar fp64 recursion and the rule for accepting a pair), `direction`, `move`, `push`;
  * `strong_wolfe`, the bracketing / cubic-interpolation / zoom search of torch.optim.LBFGS on Python floats, with one rule torch lacks: a trial
    whose loss or slope is not finite counts as overshoot (it becomes the bracket's upper end, the next trial bisects), and a search without a
    finite accepted point returns t = 0 with status `ls_failed`;
  * `minimise`, the ONE iteration loop, written against a small backend interface, and its two backends: numpy vectors (`lbfgs_reference`) and the
    device (`FusedLBFGS`).  What the two compute differs only in who runs the kernels' arithmetic;
  * `MISTAKES`, seeded errors the CPU tests must catch (the pattern of guard.MISTAKES).

Deviations from torch.optim.LBFGS(line_search_fn='strong_wolfe'), all deliberate:
  * the change rule is t * ||d||_2 <= tolerance_change where torch takes the infinity norm of t d: ||d||_2 falls out of the Gram matrix
    (sqrt(delta^T G delta)), the infinity norm would cost a reduction of its own.  The line search's bracket-width test uses the same norm;
  * the curvature pair of an iteration is stored right after its line search, not at the start of the next iteration, and a pair refused by
    s.y > 1e-10 in a FULL ring costs the slot it overwrote (count m -> m - 1) where torch keeps m older pairs;
  * a line search that ends on a point other than the last one evaluated re-evaluates the closure there (one more evaluation, rare) instead of
    keeping copies of the gradient at both bracket ends;
  * no clip: a clipped gradient breaks the curvature pairs.
"""
import ctypes
import math

import numpy as np
import torch

from .optim import FusedClipAdam

CHUNK = 2048             # every tensor is padded to whole 2048-element chunks (dpn_clip_adam_flat_floats)
MAX_M = 32               # kLbfgsMaxM
PAIR_MIN = 1e-10         # the newest pair stands when s.y > 1e-10 (torch's rule)
FIELDS = ('count', 'newest', 'iters', 'skipped', 'pending', 'reserved', 'gamma', 'gtd', 'dnorm', 'g_l1', 'g_inf', 'gg')
INT_FIELDS = FIELDS[:6]
MISTAKES = ('no_gamma_scale', 'ring_order', 'skip_ignored', 'move_incremental', 'alpha_sign', 'stale_g_prev')
LS_STATUS = ('wolfe', 'bracket_small', 'max_ls', 'ls_failed')


# ------------------------------------------------------------------------------------------------ layout and state
def zero_state():
    """DpnLbfgsState as the caller hands it over: all zero."""
    return dict({k: 0 for k in INT_FIELDS}, **{k: 0.0 for k in FIELDS[6:]})


class Layout:
    """The flat layout of a tensor list: tensor i at offsets[i] = CHUNK * (chunks of the tensors before it); `mask` marks the tensors' elements."""

    def __init__(self, numels):
        self.numels = [int(n) for n in numels]
        self.offsets, off = [], 0
        for n in self.numels:
            self.offsets.append(off)
            off += -(-n // CHUNK) * CHUNK
        self.total, self.chunks = off, off // CHUNK
        self.mask = np.zeros(off, bool)
        for o, n in zip(self.offsets, self.numels):
            self.mask[o:o + n] = True

    def pack(self, tensors, dtype=None, fill=0):
        dtype = np.asarray(tensors[0]).dtype if dtype is None else dtype
        flat = np.full(self.total, fill, dtype)
        for o, n, t in zip(self.offsets, self.numels, tensors):
            flat[o:o + n] = np.asarray(t).reshape(-1)
        return flat

    def unpack(self, flat):
        return [flat[o:o + n].copy() for o, n in zip(self.offsets, self.numels)]


def slot_of(i, state, m, mistake=None):
    """Ring slot of the pair of age rank i (0: the oldest stored, count - 1: the newest)."""
    count, nw = int(state['count']), int(state['newest'])
    if mistake == 'ring_order' and count == m and nw != m - 1 and i in (0, count - 1):
        i = count - 1 - i
    return (nw - (count - 1 - i) + m) % m


def basis_order(state, m, mistake=None):
    """The basis indices (by slot: s j = j, y j = m + j, g = 2m) in basis order: s oldest -> newest, y oldest -> newest, g."""
    slots = [slot_of(i, state, m, mistake) for i in range(int(state['count']))]
    return slots + [m + s for s in slots] + [2 * m]


# ------------------------------------------------------------------------------------------------ the kernels, restated
def _wave_sum(a):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ o]
    return a[..., 0]


def _wave_max(a):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = np.maximum(a, a[..., idx ^ o])
    return a[..., 0]


def _block(per_thread, is_max=False):
    """[..., 256] per-thread fp64 values -> the block's value: lanes by the xor butterfly, waves as (w0 + w1) + (w2 + w3)."""
    w = per_thread.reshape(per_thread.shape[:-1] + (4, 64))
    if is_max:
        w = _wave_max(w)
        return np.maximum(np.maximum(w[..., 0], w[..., 1]), np.maximum(w[..., 2], w[..., 3]))
    w = _wave_sum(w)
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _chunks64(flat, mask):
    """A flat fp32 vector as [chunks, 8, 256] fp64: element e of a chunk belongs to thread e % 256, its (e // 256)-th; padding counts as 0."""
    return np.where(mask, flat, 0).astype(np.float64).reshape(-1, 8, 256)


def _chunk_dot(a, b):
    acc = np.zeros((a.shape[0], 256))
    for k in range(8):
        acc = acc + a[:, k] * b[:, k]
    return _block(acc)


def gram_partials(S, Y, g, layout, m, state):
    """dpn_lbfgs_gram_kernel: partial[q][chunk], q = v (2m + 1) + b for v in (newest s, newest y, g) and the basis index b, then sum |g| (q = 3 (2m + 1))
    and max |g|; NaN where the kernel writes nothing (a slot without a pair).  S, Y: [m, total] fp32, g: [total] fp32, in the flat layout."""
    B, count, nw = 2 * m + 1, int(state['count']), int(state['newest'])
    out = np.full((3 * B + 2, layout.chunks), np.nan)
    g64 = _chunks64(g, layout.mask)
    zero = np.zeros_like(g64)
    new = (_chunks64(S[nw], layout.mask) if count else zero, _chunks64(Y[nw], layout.mask) if count else zero, g64)
    with np.errstate(all='ignore'):
        for b in basis_order(state, m):
            vb = g64 if b == 2 * m else _chunks64(S[b] if b < m else Y[b - m], layout.mask)
            for v in range(3):
                out[v * B + b] = _chunk_dot(new[v], vb)
        l1, mx = np.zeros((g64.shape[0], 256)), np.zeros((g64.shape[0], 256))
        for k in range(8):
            w = np.abs(g64[:, k])
            l1 = l1 + w
            mx = np.maximum(mx, w)
        out[3 * B], out[3 * B + 1] = _block(l1), _block(mx, True)
    return out


def reduce_row(row, is_max=False):
    """One block of a reduce launch: thread t takes partials t, t + 256, ... in index order, then the block's order."""
    pad = np.zeros(-(-len(row) // 256) * 256)
    pad[:len(row)] = row
    pad = pad.reshape(-1, 256)
    d = np.zeros(256)
    with np.errstate(all='ignore'):
        for r in pad:
            d = np.maximum(d, r) if is_max else d + r
        return float(_block(d, is_max))


def gram_reduce(partials, G, m, state):
    """dpn_lbfgs_gram_reduce_kernel: (G with the rows and columns of the three new vectors rewritten, state with g_l1, g_inf, gg)."""
    B, count, nw = 2 * m + 1, int(state['count']), int(state['newest'])
    G = np.array(G, np.float64).reshape(B, B).copy()
    st = dict(state)
    rows = ((nw, m + nw, 2 * m) if count else (None, None, 2 * m))
    for v, r in enumerate(rows):
        if r is None:
            continue
        for b in basis_order(state, m):
            G[r, b] = G[b, r] = reduce_row(partials[v * B + b])
    st['g_l1'], st['g_inf'], st['gg'] = reduce_row(partials[3 * B]), reduce_row(partials[3 * B + 1], True), float(G[2 * m, 2 * m])
    return G, st


def gtd_reference(a, b, layout):
    """dpn_lbfgs_gtd: a . b of two flat fp32 vectors in the Gram pass's order."""
    return reduce_row(_chunk_dot(_chunks64(a, layout.mask), _chunks64(b, layout.mask)))


def coefficients(G, state, m, mistake=None):
    """dpn_lbfgs_coef_kernel, scalar fp64 (Python floats round once per operation): (delta [2m + 1] by slot, the state after).  Judges a pending
    pair first: it stands when G[s_new, y_new] > 1e-10, otherwise the ring pointer steps back."""
    assert mistake is None or mistake in MISTAKES
    B = 2 * m + 1
    G = np.asarray(G, np.float64).reshape(B, B)
    st = dict(state)
    count, nw = int(st['count']), int(st['newest'])
    if st['pending']:
        if count > 0 and not (float(G[nw, m + nw]) > PAIR_MIN) and mistake != 'skip_ignored':
            st['skipped'] += 1
            nw = (nw - 1 + m) % m
            count -= 1
        st['pending'] = 0
    st['count'], st['newest'] = count, nw
    order = basis_order(st, m, mistake)
    slots = order[:count]
    dl = [0.0] * B
    dl[2 * m] = -1.0

    def dotcol(c):
        a = 0.0
        for b in order:
            a = a + dl[b] * float(G[b, c])
        return a

    al = [0.0] * count
    with np.errstate(all='ignore'):
        for i in range(count - 1, -1, -1):
            sl = slots[i]
            al[i] = _div(dotcol(sl), float(G[sl, m + sl]))
            dl[m + sl] = dl[m + sl] + al[i] if mistake == 'alpha_sign' else dl[m + sl] - al[i]
        gamma = 1.0
        if count > 0:
            top = slots[-1]
            gamma = _div(float(G[top, m + top]), float(G[m + top, m + top]))
            if mistake != 'no_gamma_scale':
                dl = [x * gamma for x in dl]
        for i in range(count):
            sl = slots[i]
            beta = _div(dotcol(m + sl), float(G[sl, m + sl]))
            up = al[i] - beta
            dl[sl] = dl[sl] + up
        gtd = dotcol(2 * m)
        dd = 0.0
        for b in order[:-1]:
            dd = dd + dl[b] * dotcol(b)
        dd = dd + dl[2 * m] * gtd
    st['iters'] += 1
    st['gamma'], st['gtd'], st['dnorm'] = gamma, gtd, (math.sqrt(dd) if dd > 0.0 else 0.0)
    return np.array(dl, np.float64), st


def _div(a, b):
    """IEEE division on Python floats (0 in the denominator gives inf / nan, as on the device)."""
    return float(np.float64(a) / np.float64(b))


def direction(basis, delta, dtype=np.float32):
    """dpn_lbfgs_direction_kernel: d = sum_j delta_j b_j per element in fp64, terms in the order given (the basis order), every product and every
    sum rounded once, the result rounded once to `dtype`."""
    acc = np.zeros(np.asarray(basis[0]).shape, np.float64)
    with np.errstate(all='ignore'):
        for b, c in zip(basis, delta):
            acc = acc + np.float64(c) * np.asarray(b, np.float64)
        return acc.astype(dtype)


def move(x0, d, t, x_prev=None, mistake=None):
    """dpn_lbfgs_move_kernel: fl(x0 + fl(t d)) in the vectors' own precision; t == 0 returns x0's words.  Every trial is formed from x0."""
    if t == 0:
        return x0.copy()
    base = x_prev if (mistake == 'move_incremental' and x_prev is not None) else x0
    with np.errstate(all='ignore'):
        td = x0.dtype.type(t) * d
        return base + td


def push(g, g_prev, d, t, S, Y, state, m, mask=None, mistake=None):
    """dpn_lbfgs_push: s = fl(t d), y = fl(g - g_prev) into slot (newest + 1) % m, g_prev = g, then the ring pointer.  In place on S, Y, g_prev
    (the padding, where `mask` is False, stays untouched); returns the state after."""
    st = dict(state)
    count, nw = int(st['count']), int(st['newest'])
    slot = (nw + 1) % m
    sel = slice(None) if mask is None else mask
    with np.errstate(all='ignore'):
        S[slot][sel] = (S.dtype.type(t) * d)[sel]
        Y[slot][sel] = (g - g_prev)[sel]
    if mistake != 'stale_g_prev':
        g_prev[sel] = g[sel]
    st.update(newest=slot, count=min(count + 1, m), pending=1)
    return st


# ------------------------------------------------------------------------------------------------ line search
def _cubic(x1, f1, g1, x2, f2, g2, bounds=None):
    """torch.optim.lbfgs._cubic_interpolate on floats: the minimiser of the cubic through two points with slopes, clamped to the bounds."""
    lo, hi = bounds if bounds is not None else ((x1, x2) if x1 <= x2 else (x2, x1))
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    sq = d1 * d1 - g1 * g2
    if sq >= 0:
        d2 = math.sqrt(sq)
        try:
            if x1 <= x2:
                pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
            else:
                pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
        except ZeroDivisionError:
            return (lo + hi) / 2.0
        if pos != pos:
            return (lo + hi) / 2.0
        return min(max(pos, lo), hi)
    return (lo + hi) / 2.0


def strong_wolfe(phi, f0, gtd0, t0, c1=1e-4, c2=0.9, max_ls=25, tolerance_change=1e-9, d_norm=1.0):
    """Strong-Wolfe line search on Python floats; phi(t) -> (f, gtd) evaluates the objective and its slope along the direction at step t.
    The bracketing, cubic-interpolation and zoom logic of torch.optim.LBFGS's search, plus: a trial whose f or gtd is not finite counts as
    overshoot -- it becomes the bracket's upper end (f = +inf) and the next trial bisects the bracket.
    Returns (t, f, gtd, evaluations, status): 'wolfe' (both conditions hold at t), 'bracket_small' (the bracket times d_norm fell under
    tolerance_change), 'max_ls' (the evaluations ran out) -- in both t is the bracket's lower end, which satisfies the decrease condition --
    or 'ls_failed' (no trial gave a finite point that lowers f: t = 0, f = f0, gtd = gtd0)."""
    inf = float('inf')

    def trial(t):
        f, g = phi(t)
        f, g = float(f), float(g)
        if not (math.isfinite(f) and math.isfinite(g)):
            return inf, float('nan')
        return f, g

    t = float(t0)
    f_new, gtd_new = trial(t)
    evals = 1
    t_prev, f_prev, gtd_prev = 0.0, float(f0), float(gtd0)
    done, ls_iter, bracket = False, 0, None
    while ls_iter < max_ls:
        if f_new > (f0 + c1 * t * gtd0) or (ls_iter > 1 and f_new >= f_prev):       # (a non-finite trial is +inf: it lands here)
            bracket, bracket_f, bracket_gtd = [t_prev, t], [f_prev, f_new], [gtd_prev, gtd_new]
            break
        if abs(gtd_new) <= -c2 * gtd0:
            bracket, bracket_f, bracket_gtd = [t], [f_new], [gtd_new]
            done = True
            break
        if gtd_new >= 0:
            bracket, bracket_f, bracket_gtd = [t_prev, t], [f_prev, f_new], [gtd_prev, gtd_new]
            break
        min_step, max_step = t + 0.01 * (t - t_prev), t * 10
        tmp = t
        t = _cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds=(min_step, max_step))
        t_prev, f_prev, gtd_prev = tmp, f_new, gtd_new
        f_new, gtd_new = trial(t)
        evals += 1
        ls_iter += 1
    if bracket is None:                                                              # max_ls reached while still extending
        bracket, bracket_f, bracket_gtd = [0.0, t], [float(f0), f_new], [float(gtd0), gtd_new]
    status = 'wolfe' if done else 'max_ls'
    insuf = False
    low, high = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
    while not done and ls_iter < max_ls:
        if abs(bracket[1] - bracket[0]) * d_norm < tolerance_change:
            status = 'bracket_small'
            break
        if math.isfinite(bracket_f[0]) and math.isfinite(bracket_f[1]):
            t = _cubic(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1])
        else:
            t = 0.5 * (bracket[0] + bracket[1])                                      # an end that overshot carries no cubic: bisect
        hi_t, lo_t = max(bracket), min(bracket)
        eps = 0.1 * (hi_t - lo_t)
        if min(hi_t - t, t - lo_t) < eps:
            if insuf or t >= hi_t or t <= lo_t:
                t = hi_t - eps if abs(t - hi_t) < abs(t - lo_t) else lo_t + eps
                insuf = False
            else:
                insuf = True
        else:
            insuf = False
        f_new, gtd_new = trial(t)
        evals += 1
        ls_iter += 1
        if f_new > (f0 + c1 * t * gtd0) or f_new >= bracket_f[low]:
            bracket[high], bracket_f[high], bracket_gtd[high] = t, f_new, gtd_new
            low, high = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
        else:
            if abs(gtd_new) <= -c2 * gtd0:
                done, status = True, 'wolfe'
            elif gtd_new * (bracket[high] - bracket[low]) >= 0:
                bracket[high], bracket_f[high], bracket_gtd[high] = bracket[low], bracket_f[low], bracket_gtd[low]
            bracket[low], bracket_f[low], bracket_gtd[low] = t, f_new, gtd_new
    if len(bracket) == 1:
        low = 0
    t, f, gtd = bracket[low], bracket_f[low], bracket_gtd[low]
    if t == 0.0 or not math.isfinite(f) or not f <= f0:
        return 0.0, float(f0), float(gtd0), evals, 'ls_failed'
    return t, f, gtd, evals, status


# ------------------------------------------------------------------------------------------------ the loop
def minimise(be, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9, c1=1e-4, c2=0.9, max_ls=25, trace=None):
    """One call of L-BFGS on the backend `be` (NumpyBackend or FusedLBFGS's device backend):
        be.evaluate() -> f      the closure at the current parameters, the gradient left in the backend's g
        be.refresh()            g_prev = g (the pairs of this call are differences under THIS call's objective)
        be.direction() -> dict  the Gram pass, the recursion, the direction pass; the state's scalars
        be.save() / be.move(t)  x0 = x;  x = fl(x0 + fl(t d))
        be.gtd() -> g . d       at the current point
        be.push(t)              the pair of the step t d just taken
        be.clear()              empty ring
    Returns dict(iters, evals, t, status, f0, f, skipped_pairs).  trace (a list): (t, f) of every line-search evaluation is appended."""
    max_eval = max_iter * 5 // 4 if max_eval is None else int(max_eval)
    f = float(be.evaluate())
    out = dict(iters=0, evals=1, t=0.0, status='max_iter', f0=f, f=f, skipped_pairs=0)
    if not math.isfinite(f):
        out['status'] = 'nonfinite_loss'
        return out
    be.refresh()
    while True:
        st = be.direction()
        out['skipped_pairs'] = int(st['skipped'])
        if not (math.isfinite(st['g_inf']) and math.isfinite(st['gtd']) and math.isfinite(st['dnorm'])):
            out['status'] = 'nonfinite_gradient'
            be.clear()
            break
        if st['g_inf'] <= tolerance_grad:
            out['status'] = 'tolerance_grad'
            break
        if st['gtd'] > -tolerance_change:
            out['status'] = 'tolerance_change'
            break
        t0 = (min(1.0, 1.0 / st['g_l1']) * lr) if int(st['count']) == 0 else lr         # torch's first step length, then lr
        be.save()
        seen = [None]

        def phi(t):
            be.move(t)
            ft = float(be.evaluate())
            gt = float(be.gtd())
            seen[0] = t
            if trace is not None:
                trace.append((t, ft))
            return ft, gt

        t, f_new, _, ls_evals, ls_status = strong_wolfe(phi, f, st['gtd'], t0, c1, c2, max_ls, tolerance_change, st['dnorm'])
        out['evals'] += ls_evals
        if ls_status == 'ls_failed':
            be.move(0.0)                                # x0, bit for bit
            be.clear()
            out.update(status='ls_failed', t=0.0)
            break
        if seen[0] != t:                                # the search ended on an earlier trial: its gradient is evaluated again
            be.move(t)
            f_new = float(be.evaluate())
            out['evals'] += 1
            if trace is not None:
                trace.append((t, f_new))
        be.push(t)
        f_prev, f = f, f_new
        out.update(iters=out['iters'] + 1, t=t, f=f)
        if out['iters'] >= max_iter:
            out['status'] = 'max_iter'
            break
        if out['evals'] >= max_eval:
            out['status'] = 'max_eval'
            break
        if t * st['dnorm'] <= tolerance_change or abs(f - f_prev) < tolerance_change:
            out['status'] = 'tolerance_change'
            break
    return out


class NumpyBackend:
    """The kernels' arithmetic on numpy vectors in the flat layout, fp32 (bit for bit the device's) or fp64 (the same operations, for comparisons
    with other implementations).  fun(x) -> (f, g), x and g as the caller gave x0: one 1-D array, or a list of arrays (one per tensor)."""

    def __init__(self, fun, x0, history_size=10, dtype=np.float32, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.fun, self.m, self.dtype, self.mistake = fun, int(history_size), np.dtype(dtype), mistake
        self.single = not isinstance(x0, (list, tuple))
        tensors = [np.asarray(x0)] if self.single else [np.asarray(t) for t in x0]
        self.shapes = [t.shape for t in tensors]
        self.layout = Layout([t.size for t in tensors])
        self.x = self.layout.pack(tensors, self.dtype)
        n = self.layout.total
        self.x0, self.g, self.g_prev, self.d = (np.zeros(n, self.dtype) for _ in range(4))
        self.S, self.Y = np.zeros((self.m, n), self.dtype), np.zeros((self.m, n), self.dtype)
        self.G = np.zeros((2 * self.m + 1, 2 * self.m + 1))
        self.state, self.delta, self.x_trial = zero_state(), None, None

    def params(self):
        parts = [p.reshape(s) for p, s in zip(self.layout.unpack(self.x), self.shapes)]
        return parts[0] if self.single else parts

    def evaluate(self):
        f, g = self.fun(self.params())
        self.g = self.layout.pack([np.asarray(g)] if self.single else [np.asarray(t) for t in g], self.dtype)
        return float(f)

    def refresh(self):
        self.g_prev = self.g.copy()

    def clear(self):
        self.state = zero_state()

    def direction(self):
        m, lay = self.m, self.layout
        if self.dtype == np.float32:
            self.G, st = gram_reduce(gram_partials(self.S, self.Y, self.g, lay, m, self.state), self.G, m, self.state)
        else:                                           # fp64 vectors: the same inner products, numpy's summation order
            st = dict(self.state)
            count, nw = int(st['count']), int(st['newest'])
            vec = lambda b: self.g if b == 2 * m else (self.S[b] if b < m else self.Y[b - m])
            for r in ((nw, m + nw, 2 * m) if count else (2 * m,)):
                for b in basis_order(st, m):
                    self.G[r, b] = self.G[b, r] = float(np.dot(vec(r), vec(b)))
            st.update(g_l1=float(np.abs(self.g).sum()), g_inf=float(np.abs(self.g).max()), gg=float(self.G[2 * m, 2 * m]))
        self.delta, self.state = coefficients(self.G, st, m, self.mistake)
        order = basis_order(self.state, m, self.mistake)
        vecs = [self.g if b == 2 * m else (self.S[b] if b < m else self.Y[b - m]) for b in order]
        self.d = np.where(lay.mask, direction(vecs, self.delta[order], self.dtype), self.d)
        return dict(self.state)

    def save(self):
        self.x0 = self.x.copy()
        self.x_trial = None

    def move(self, t):
        self.x = np.where(self.layout.mask, move(self.x0, self.d, t, self.x_trial, self.mistake), self.x)
        self.x_trial = self.x.copy()

    def gtd(self):
        if self.dtype == np.float32:
            return gtd_reference(self.g, self.d, self.layout)
        return float(np.dot(self.g, self.d))

    def push(self, t):
        self.state = push(self.g, self.g_prev, self.d, t, self.S, self.Y, self.state, self.m, self.layout.mask, self.mistake)


def lbfgs_reference(fun, x0, lr=1.0, max_iter=20, max_eval=None, history_size=10, tolerance_grad=1e-7, tolerance_change=1e-9, c1=1e-4, c2=0.9,
                    dtype=np.float64, mistake=None, trace=None):
    """The whole loop over numpy vectors, built from the pieces above: (x, last) with x shaped like x0 and last = minimise's dict."""
    be = NumpyBackend(fun, x0, history_size, dtype, mistake)
    last = minimise(be, lr, max_iter, max_eval, tolerance_grad, tolerance_change, c1, c2, trace=trace)
    return be.params(), last


# ------------------------------------------------------------------------------------------------ the device
class FusedLBFGS(torch.optim.Optimizer):
    """L-BFGS with a strong-Wolfe line search on the HIP kernels of csrc/dpn_lbfgs.inc, a torch.optim.Optimizer.

    It owns ONE flat fp32 gradient buffer (`_g_flat`, with `_leased`) registered with grad_arena exactly as FusedClipAdam's, so the gradients of this
    package's autograd nodes arrive in place; history S, Y [history_size, total], x0, g_prev and d in the same layout, the fp64 Gram matrix and the
    DpnLbfgsState on the device.  `step(closure)` runs `minimise`: per iteration the Gram pass and its reduce, the one-thread recursion and the
    direction pass (four launches that read the history twice), `save`, the line search (`move`, closure, one inner product per trial), `push`.
    The host reads the loss and g.d per evaluation and the state's scalars once per iteration, nothing else.
    `step_count` (device int32[1]) is bumped once per step() CALL, not per evaluation: a sampler bound to it keeps its points through a line search.
    history='reset' empties the ring at the start of every step() (a new collocation set is a new objective), 'keep' carries the pairs over.
    After a failed line search the parameters equal the iteration's x0 bit for bit and the ring is empty; parameters are never left at a trial
    whose loss was not finite.  No clip.  Refused: parameter groups whose options differ, ema_decay, a call inside a graph capture, CPU or non-fp32
    parameters.  state_dict carries the options and counters, not the history: a loaded optimiser starts with an empty ring."""

    OPTIONS = ('lr', 'max_iter', 'max_eval', 'history_size', 'tolerance_grad', 'tolerance_change', 'c1', 'c2', 'history')

    def __init__(self, params, lr=1.0, max_iter=20, max_eval=None, history_size=10, tolerance_grad=1e-7, tolerance_change=1e-9, c1=1e-4, c2=0.9,
                 history='reset', ema_decay=None):
        from . import _lib as L, grad_arena
        if ema_decay is not None:
            raise ValueError('FusedLBFGS: ema_decay is not supported (the weight EMA lives in the fused clip + Adam launch)')
        if history not in ('reset', 'keep'):
            raise ValueError("FusedLBFGS: history must be 'reset' or 'keep', got %r" % (history,))
        if isinstance(history_size, bool) or int(history_size) != history_size or not 1 <= int(history_size) <= MAX_M:
            raise ValueError('FusedLBFGS: history_size must be an integer in 1 .. %d, got %r' % (MAX_M, history_size))
        if int(max_iter) < 1 or (max_eval is not None and int(max_eval) < 1):
            raise ValueError('FusedLBFGS: max_iter and max_eval must be >= 1')
        if not (float(lr) > 0.0 and math.isfinite(float(lr))):
            raise ValueError('FusedLBFGS: lr must be a finite number > 0, got %r' % (lr,))
        defaults = dict(lr=float(lr), max_iter=int(max_iter), max_eval=None if max_eval is None else int(max_eval), history_size=int(history_size),
                        tolerance_grad=float(tolerance_grad), tolerance_change=float(tolerance_change), c1=float(c1), c2=float(c2), history=history)
        self._built = False
        super().__init__(params, defaults)
        self._built = True
        first = self.param_groups[0]
        for g in self.param_groups[1:]:
            differing = [k for k in self.OPTIONS if g[k] != first[k]]
            if differing:
                raise ValueError('FusedLBFGS: one line search moves every parameter: parameter groups must agree in every option, they differ in %s'
                                 % ', '.join(differing))
        self.params = [p for g in self.param_groups for p in g['params']]
        if not self.params or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in self.params):
            raise RuntimeError('FusedLBFGS needs contiguous fp32 HIP parameters (no CPU fallback)')
        dev, n, m = self.params[0].device, len(self.params), int(history_size)
        lib = L.load()
        self._numel = (ctypes.c_int64 * n)(*[p.numel() for p in self.params])
        self.layout = Layout([p.numel() for p in self.params])
        total = int(lib.dpn_clip_adam_flat_floats(n, self._numel))
        assert total == self.layout.total
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self._g_flat, self._x0, self._g_prev, self._d = f32(total), f32(total), f32(total), f32(total)
        self._S, self._Y = f32(m, total), f32(m, total)
        self._scratch = torch.zeros(int(lib.dpn_lbfgs_scratch_doubles(n, self._numel, m)), dtype=torch.float64, device=dev)
        self._G = torch.zeros((2 * m + 1) ** 2, dtype=torch.float64, device=dev)
        self._delta = torch.zeros(2 * m + 1, dtype=torch.float64, device=dev)
        self._gtd_out = torch.zeros(1, dtype=torch.float64, device=dev)
        self._state = torch.zeros(ctypes.sizeof(L.DpnLbfgsState) // 8, dtype=torch.int64, device=dev)     # DpnLbfgsState: 6 int32 + 6 fp64
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._offsets = list(self.layout.offsets)
        self._slots = [self._g_flat[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.params)]
        self._p = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.params])
        self._ptrs = [p.data_ptr() for p in self.params]
        self._leased = set()
        self.steps_done = 0                                         # host-side count of parameter rewrites (move calls)
        self.last = None
        self._closure = None
        grad_arena.register(self, self.params, self._offsets)

    def add_param_group(self, param_group):
        if getattr(self, '_built', False):
            raise NotImplementedError('FusedLBFGS.add_param_group: the flat buffers are laid out at construction; build a new optimiser')
        super().add_param_group(param_group)

    def __del__(self):
        try:
            from . import grad_arena
            grad_arena.unregister(self)
        except Exception:                                           # interpreter shutdown
            pass

    # the arena side is FusedClipAdam's own code (it reads self.params, _ptrs, _slots, _g_flat, _leased): pointers checked against the live tensors,
    # flat_gradients, gather_gradients, place_gradients, zero_grad
    _check_pointers = FusedClipAdam._check_pointers
    flat_gradients = FusedClipAdam.flat_gradients
    gather_gradients = FusedClipAdam.gather_gradients
    place_gradients = FusedClipAdam.place_gradients
    zero_grad = FusedClipAdam.zero_grad

    # ---- the kernels -------------------------------------------------------------------------------------------------------
    def _call(self, name, *args):
        from . import _lib as L
        ptr = lambda a: ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a
        L.check(getattr(L.load(), name)(len(self.params), self._p, self._numel, *[ptr(a) for a in args], torch.cuda.current_stream().cuda_stream), name)

    def lbfgs_state(self):
        """DpnLbfgsState as a dict (reads the device, so it synchronises)."""
        raw = self._state.cpu().numpy()
        ints, dbl = raw.view(np.int32), raw.view(np.float64)
        out = {k: int(ints[i]) for i, k in enumerate(INT_FIELDS)}
        out.update({k: float(dbl[3 + i]) for i, k in enumerate(FIELDS[6:])})
        return out

    # the backend interface of `minimise`
    def evaluate(self):
        with torch.enable_grad():
            loss = self._closure()
        self.gather_gradients()
        return float(loss)

    def refresh(self):
        self._g_prev.copy_(self._g_flat)

    def clear(self):
        self._state.zero_()

    def direction(self):
        m = self.defaults['history_size']
        self._call('dpn_lbfgs_gram', self._S, self._Y, self._g_flat, m, self._state, self._scratch, self._G)
        self._call('dpn_lbfgs_direction', self._S, self._Y, self._g_flat, m, self._state, self._G, self._delta, self._d)
        return self.lbfgs_state()

    def save(self):
        self._call('dpn_lbfgs_save', self._x0)

    def move(self, t):
        from . import grad_arena
        self._call('dpn_lbfgs_move', self._x0, self._d, ctypes.c_float(t))
        grad_arena.param_epoch[0] += 1                 # the parameters changed through raw pointers: caches keyed on the epoch miss
        self.steps_done += 1                           # (point_path's forward / backward stamps: a rewrite between the two passes is noticed)

    def gtd(self):
        self._call('dpn_lbfgs_gtd', self._g_flat, self._d, self._scratch, self._gtd_out)
        return float(self._gtd_out)

    def push(self, t):
        self._call('dpn_lbfgs_push', self._g_flat, self._g_prev, self._d, ctypes.c_float(t), self._S, self._Y, self.defaults['history_size'], self._state)

    # ---- step --------------------------------------------------------------------------------------------------------------
    def step(self, closure=None, trace=None):
        """One L-BFGS call: up to max_iter iterations / max_eval closure evaluations.  closure() zeroes the gradients, evaluates the loss, runs
        backward and returns the loss.  Returns the first loss (a float tensor's value as torch.optim.LBFGS returns orig_loss); `last` keeps
        dict(iters, evals, t, status, f0, f, skipped_pairs)."""
        if closure is None:
            raise RuntimeError('FusedLBFGS.step needs a closure that re-evaluates the model and returns the loss')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedLBFGS.step inside a graph capture: the line search reads losses on the host')
        self._check_pointers()
        o = self.param_groups[0]
        with torch.no_grad():
            self.step_count += 1
            if o['history'] == 'reset':
                self.clear()
            self._closure = closure
            try:
                self.last = minimise(self, o['lr'], o['max_iter'], o['max_eval'], o['tolerance_grad'], o['tolerance_change'], o['c1'], o['c2'],
                                     trace=trace)
            finally:
                self._closure = None
        return self.last['f0']

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd['lbfgs'] = dict(step_count=int(self.step_count), steps_done=self.steps_done, last=self.last)
        return sd

    def load_state_dict(self, state_dict):
        extra = state_dict.get('lbfgs')
        super().load_state_dict({k: v for k, v in state_dict.items() if k != 'lbfgs'})
        for g in self.param_groups:
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        if int(self.param_groups[0]['history_size']) != self.defaults['history_size']:
            raise ValueError('FusedLBFGS.load_state_dict: history_size %r, the ring buffers were laid out for %d'
                             % (self.param_groups[0]['history_size'], self.defaults['history_size']))
        self.clear()                                    # the history is not saved: an empty ring
        if extra is not None:
            self.step_count.fill_(int(extra.get('step_count', 0)))
            self.steps_done, self.last = int(extra.get('steps_done', 0)), extra.get('last')
