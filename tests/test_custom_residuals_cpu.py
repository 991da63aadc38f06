"""CPU: the coordinate-differentiable point op (point_path.point_fields_xyt) -- the C entry points it calls are declared and exported, and its
autograd plumbing (the attach nodes that make out, J, H functions of x, y, t) gives what torch autograd gives on a plain expression with the
same structure.  The HIP core node is replaced here by a torch stand-in of that structure (each output a sum of one-coordinate terms); the
GPU file tests/test_gpu_custom_residuals.py checks the kernels themselves against the oracle."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('dpn_fwd_ref_derivs', 'dpn_bwd_points_derivs')


def test_derivative_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'dpn_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(dpn_\w+)\s*\(', header, flags=re.M))
    import __graft_entry__ as g
    g.build()
    from deepphysinet_amd import _lib
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def _stand_in_fields(a, b, x, y, t):
    """out[:, k] = sum_c a[k, c] sin(b[k, c] xi_c): one-coordinate terms, like the point nets (piecewise linear in per-coordinate features)."""
    xi = torch.stack([x.reshape(-1), y.reshape(-1), t.reshape(-1)], 1)                   # [N, 3]
    return (a[None] * torch.sin(b[None] * xi[:, None, :])).sum(2)                       # [N, 6]


class _StandInCore:
    """What _PointDerivsFn returns -- (out, J, H, D3) with the coordinates detached, differentiable w.r.t. the weights -- in torch."""

    @staticmethod
    def apply(cfg, x, y, t, coord_data, a, b):
        xi = torch.stack([x.reshape(-1), y.reshape(-1), t.reshape(-1)], 1)[:, None, :]
        s, c = torch.sin(b[None] * xi), torch.cos(b[None] * xi)
        out = (a[None] * s).sum(2)
        return out, a * b * c, -a * b * b * s, -a * b * b * b * c


@pytest.fixture
def stand_in(monkeypatch):
    from deepphysinet_amd import point_path
    monkeypatch.setattr(point_path, '_PointDerivsFn', _StandInCore)
    torch.manual_seed(0)
    n = 7
    a = torch.randn(6, 3, dtype=torch.float64, requires_grad=True)
    b = (torch.rand(6, 3, dtype=torch.float64) + 0.5).requires_grad_(True)
    x, y, t = (torch.rand(n, 1, dtype=torch.float64, requires_grad=True) for _ in range(3))
    return point_path, a, b, x, y, t


def _grad(v, w):
    return torch.autograd.grad(v, w, grad_outputs=torch.ones_like(v), create_graph=True, allow_unused=False)[0]


def _custom_loss(fields, x, y, t):
    u, T = fields[:, 0:1], fields[:, 3:4]
    res = u * _grad(u, x) + 0.3 * (_grad(_grad(u, x), x) + _grad(_grad(u, y), y)) + _grad(_grad(T, x), x) + _grad(_grad(T, y), y) \
        + _grad(_grad(u, t), t) + _grad(T, t)
    return (res ** 2).mean()


def test_attach_nodes_give_autograd_values_and_gradients(stand_in):
    pp, a, b, x, y, t = stand_in
    mine = pp.point_fields_xyt(None, x, y, t, None, a, b, [])
    ref = _stand_in_fields(a, b, x, y, t)
    assert torch.allclose(mine, ref)
    lm, lr = _custom_loss(mine, x, y, t), _custom_loss(ref, x, y, t)
    assert torch.allclose(lm, lr)
    gm = torch.autograd.grad(lm, [a, b, x, y, t])
    gr = torch.autograd.grad(lr, [a, b, x, y, t])
    for u, v in zip(gm, gr):
        assert torch.allclose(u, v, rtol=1e-10, atol=1e-12)


def test_mixed_partials_are_zero_and_third_order_is_the_limit(stand_in):
    pp, a, b, x, y, t = stand_in
    u = pp.point_fields_xyt(None, x, y, t, None, a, b, [])[:, 0:1]
    u_x = _grad(u, x)
    assert torch.equal(_grad(u_x, y), torch.zeros_like(x))
    u_xxx = _grad(_grad(u_x, x), x)
    assert torch.allclose(u_xxx, _grad(_grad(_grad(_stand_in_fields(a, b, x, y, t)[:, 0:1], x), x), x))
    with pytest.raises(RuntimeError, match='third derivative'):
        torch.autograd.grad(u_xxx.sum(), [a], retain_graph=True)
    with pytest.raises(RuntimeError, match='third derivative'):
        torch.autograd.grad(u_xxx.sum(), [x])
