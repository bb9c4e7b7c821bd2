"""CPU side of the bias gradient that rides in the weight-gradient GEMM:
``wgrad_matmul(..., bsum=db)`` never fuses on CPU tensors (returns False, ``db``
untouched), and the callers then produce the reference bias gradient."""
import torch

from flexflow_train_amd.ops import base as opbase
from flexflow_train_amd.ops import gemm as G


def _ctx(op, attrs):
    return opbase.OpContext(op_type=op, attrs=attrs, name=op.lower(), training=True)


def test_wgrad_matmul_on_cpu_leaves_bsum_alone():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(64, 16, generator=g), torch.randn(64, 24, generator=g)
    for beta in (0.0, 1.0):
        out0 = torch.randn(16, 24, generator=g)
        out = out0.clone()
        db = torch.arange(24, dtype=torch.float32) + 1.0
        fused = G.wgrad_matmul(_ctx("LINEAR", {}), a, b, out, beta, bsum=db)
        assert fused is False
        assert torch.equal(db, torch.arange(24, dtype=torch.float32) + 1.0)
        torch.testing.assert_close(out, a.t() @ b + beta * out0)
    assert G.wgrad_matmul(_ctx("LINEAR", {}), a, b, torch.zeros(16, 24), 0.0) is False


def test_linear_bias_gradient_on_cpu():
    g = torch.Generator().manual_seed(4)
    x, W, b = torch.randn(40, 16, generator=g), torch.randn(16, 24, generator=g), torch.randn(24, generator=g)
    dy = torch.randn(40, 24, generator=g)
    impl, ctx = opbase.get_impl("LINEAR"), _ctx("LINEAR", {"activation": "none"})
    _, saved = impl.forward(ctx, [x], [W, b])
    start = torch.arange(24, dtype=torch.float32)
    grads = [torch.zeros(16, 24), start.clone()]
    (dx,) = impl.backward(ctx, saved, [dy], grads, [True])
    torch.testing.assert_close(grads[1], start + dy.sum(0))
    torch.testing.assert_close(grads[0], x.t() @ dy)
    torch.testing.assert_close(dx, dy @ W.t())
    # no weight gradient wanted: the bias gradient is still complete
    grads = [None, start.clone()]
    impl.backward(ctx, saved, [dy], grads, [False])
    torch.testing.assert_close(grads[1], start + dy.sum(0))


def test_self_attention_bias_gradient_on_cpu():
    g = torch.Generator().manual_seed(5)
    E, H = 32, 4
    D = E // H
    x = torch.randn(2, 8, E, generator=g)
    W = (torch.randn(E * 3 * H * D + H * D * E, generator=g) * 0.3).view(-1, H)
    b_in = torch.randn(3 * H * D, generator=g) * 0.1
    dout = torch.randn(2, 8, E, generator=g)
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = _ctx("MULTIHEAD_ATTENTION", {"embed_dim": E, "num_heads": H, "kdim": 0, "vdim": 0, "causal": False})

    # autograd reference: the same operator's forward is differentiable on the CPU path's torch ops
    bp = b_in.clone().requires_grad_(True)
    (out,), _ = impl.forward(ctx, [x, x, x], [W, bp])
    out.backward(dout)
    want = bp.grad

    (out,), saved = impl.forward(ctx, [x, x, x], [W, b_in])
    start = torch.full((3 * H * D,), 0.5)
    grads = [torch.zeros_like(W), start.clone()]
    impl.backward(ctx, saved, [dout], grads, [True, False, False])
    torch.testing.assert_close(grads[1], start + want, rtol=1e-4, atol=1e-5)
