"""CPU: staged_backward.StagedBackward on a toy graph of four parameter buckets -- which buckets each cut places, that the placed
gradients are those of one plain backward pass, and that the object lets go of the graph.  Plain torch on CPU tensors: no HIP library.
"""
import torch

from deepphysinet_amd.staged_backward import StagedBackward


class _Placer:
    """Stands in for the optimiser: place_gradients records, in call order, which parameters it was given and their gradients."""

    def __init__(self):
        self.calls, self.grads = [], {}

    def place_gradients(self, params, grads):
        params, grads = list(params), list(grads)
        assert len(params) == len(grads)
        self.calls.append([id(p) for p in params])
        for p, g in zip(params, grads):
            assert id(p) not in self.grads, 'a parameter was placed twice'
            self.grads[id(p)] = g


def _graph():
    """x0 = f(bucket 3); meta_out = g(x0, bucket 2); heads, evec = h(meta_out, bucket 1); loss = k(heads, evec, bucket 0).  Built from a fixed
    seed: two calls give identical graphs."""
    gen = torch.Generator().manual_seed(3)
    new = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_(True)
    buckets = [[new(5), new(7, 5)], [new(5, 4), new(7, 4)], [new(4, 4), new(4)], [new(6, 4), new(4)]]
    field = torch.randn(3, 6, generator=gen, dtype=torch.float64)
    x0 = torch.tanh(field @ buckets[3][0]) + buckets[3][1]
    meta_out = torch.sin(x0 @ buckets[2][0]) * buckets[2][1]
    heads = buckets[1][0] @ meta_out.t()
    evec = buckets[1][1] @ meta_out.t()
    statics = buckets[0]
    loss = ((heads * statics[0][:, None]).sum() + (statics[1] @ heads * evec).sum()) ** 2
    return buckets, dict(loss=loss, heads=heads, evec=evec, statics=statics, meta_out=meta_out, x0=x0)


def _reference():
    buckets, t = _graph()
    flat = [p for b in buckets for p in b]
    return [list(g) for g in _split(torch.autograd.grad(t['loss'], flat), buckets)]


def _split(grads, buckets):
    out, k = [], 0
    for b in buckets:
        out.append(grads[k:k + len(b)])
        k += len(b)
    return out


def _run(x0_mode):
    """The four cuts, noting after each which buckets have been placed so far.  x0_mode: 'given', 'none', 'no_grad'."""
    buckets, t = _graph()
    if x0_mode != 'given':
        t['x0'] = None if x0_mode == 'none' else t['x0'].detach()        # (detached: the caller holds the values, not the graph's node)
    placer = _Placer()
    back = StagedBackward(buckets, placer)
    seed = torch.ones((), dtype=torch.float64)
    placed = lambda: [k for k, b in enumerate(buckets) if all(id(p) in placer.grads for p in b)]
    after = []
    back.points(t['loss'], t['heads'], t['evec'], t['statics'], t['meta_out'], t['x0'], seed)
    after.append(placed())
    back.heads_cut()
    after.append(placed())
    back.encoder()
    after.append(placed())
    held_x0 = back.x0 is not None
    back.embedding()
    after.append(placed())
    return buckets, placer, back, after, held_x0


def _assert_equals_plain_backward(buckets, placer, ref):
    for k, b in enumerate(buckets):
        for j, p in enumerate(b):
            assert torch.equal(placer.grads[id(p)], ref[k][j]), (k, j)


def _assert_released(back):
    assert all(getattr(back, name) is None for name in StagedBackward.HELD)
    assert {'heads', 'evec', 'meta_out', 'x0', 'g_heads', 'g_evec', 'g_meta', 'g_x0'} <= set(StagedBackward.HELD)


def test_with_x0_every_cut_places_its_buckets_and_the_gradients_are_the_plain_backwards():
    buckets, placer, back, after, held_x0 = _run('given')
    assert held_x0
    assert after == [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3]]
    assert placer.calls == [[id(p) for p in b] for b in buckets]             # one call per bucket, in layout order
    _assert_equals_plain_backward(buckets, placer, _reference())
    _assert_released(back)


def test_without_x0_the_encoder_cut_takes_the_embedding_along():
    buckets, placer, back, after, held_x0 = _run('none')
    assert not held_x0
    assert after == [[0], [0, 1], [0, 1, 2, 3], [0, 1, 2, 3]]                 # the embedding cut places nothing
    assert placer.calls == [[id(p) for p in buckets[0]], [id(p) for p in buckets[1]], [id(p) for p in buckets[2] + buckets[3]]]
    _assert_equals_plain_backward(buckets, placer, _reference())
    _assert_released(back)


def test_an_x0_that_does_not_require_grad_is_no_cut():
    buckets, placer, back, after, held_x0 = _run('no_grad')
    assert not held_x0
    assert after == [[0], [0, 1], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert placer.calls == [[id(p) for p in buckets[0]], [id(p) for p in buckets[1]], [id(p) for p in buckets[2] + buckets[3]]]
    _assert_equals_plain_backward(buckets, placer, _reference())
    _assert_released(back)
