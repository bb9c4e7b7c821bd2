"""The bias gradient taken from the weight-gradient GEMM (``wgrad_matmul``'s
``bsum``) in the two operators that use it: a biased Linear without
activation and the self-attention QKV projection.

The decision is forced, not timed: ``gemm._BSUM_MODE`` "2" (every eligible
signature fused, unsplit) against "0" (never).  Every GEMM of the test runs on
gemmp variant 6 unsplit where it takes the shape (``_candidates`` reduced to
"w:1"), so the two runs
differ in the ``bsum`` switch alone: dW and dx must agree bit for bit, and the
bias gradients within twice ``bsum_bound`` (each run is within one bound of
the exact sum of the same bf16 values)."""
import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops import base as opbase
from flexflow_train_amd.ops import gemm as G
from test_wgrad_bsum_gpu import bsum_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def only_w1(monkeypatch):
    monkeypatch.setattr(G, "_CHOICE", {})
    monkeypatch.setattr(G, "_TIMES", {})
    # (the Linear's input-gradient GEMM has K = 264, which the 256x256-tile
    # family does not take: that one runs on the 128x128-tile kernel both times)
    monkeypatch.setattr(G, "_candidates",
                        lambda a, b, ta, tb, *r, **k: {"w:1": lambda *args: G._gt(*args, splits=1, variant=6)}
                        if K.gemmp_supported(a, b, ta, tb) else {"hip": G._hip})


def _linear():
    g = torch.Generator().manual_seed(11)
    T, I, O = 512, 256, 264
    x = torch.randn(T, I, generator=g).to(BF16).to(DEV)
    W = (torch.randn(I, O, generator=g) * 0.05).to(BF16).to(DEV)
    b = torch.randn(O, generator=g).to(BF16).to(DEV)
    dy = torch.randn(T, O, generator=g).to(BF16).to(DEV)
    impl = opbase.get_impl("LINEAR")
    ctx = opbase.OpContext(op_type="LINEAR", attrs={"activation": "none"}, name="fc", training=True)
    _, saved = impl.forward(ctx, [x], [W, b])

    def backward():
        grads = [torch.zeros(I, O, device=DEV, dtype=F32), torch.zeros(O, device=DEV, dtype=F32)]
        (dx,) = impl.backward(ctx, saved, [dy], grads, [True])
        return dx, grads[0], grads[1]
    return backward, T


def _attention():
    g = torch.Generator().manual_seed(12)
    B, S, H, D = 2, 128, 4, 64
    E = H * D
    x = torch.randn(B, S, E, generator=g).to(BF16).to(DEV)
    W = (torch.randn(E * 3 * H * D + H * D * E, generator=g) * 0.05).to(BF16).to(DEV).view(-1, H)
    b_in = (torch.randn(3 * H * D, generator=g) * 0.1).to(BF16).to(DEV)
    dout = torch.randn(B, S, E, generator=g).to(BF16).to(DEV)
    attrs = {"embed_dim": E, "num_heads": H, "kdim": 0, "vdim": 0, "causal": False}
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = opbase.OpContext(op_type="MULTIHEAD_ATTENTION", attrs=attrs, name="mha", training=True)
    _, saved = impl.forward(ctx, [x, x, x], [W, b_in])

    def backward():
        grads = [torch.zeros(W.shape, device=DEV, dtype=F32), torch.zeros(3 * H * D, device=DEV, dtype=F32)]
        dx = impl.backward(ctx, saved, [dout], grads, [True, False, False])[0]
        return dx, grads[0], grads[1]
    return backward, B * S


@pytest.fixture
def seen(monkeypatch):
    """The gradient matrix whose column sums are the bias gradient: operand b
    of the operator's ``wgrad_matmul`` call that carries ``bsum``."""
    from flexflow_train_amd.ops import attention, dense
    rec = {}

    def spy(ctx, a, b, out, beta, bsum=None):
        if bsum is not None:
            rec["g"] = b
        return G.wgrad_matmul(ctx, a, b, out, beta, bsum)
    monkeypatch.setattr(dense, "wgrad_matmul", spy)
    monkeypatch.setattr(attention, "wgrad_matmul", spy)
    return rec


def _within(db, g, T, times):
    """|db - exact| <= times * bsum_bound per column; exact = the fp64 sums of g."""
    g = g.double()
    bound = bsum_bound(T, 1, 1, g.abs().sum(0))
    worst = ((db.double() - g.sum(0)).abs() / (times * bound)).max().item()
    print(f"worst |db - exact| / ({times} bound) = {worst:.4f}")
    return worst <= 1.0


@pytest.mark.parametrize("make", [_linear, _attention], ids=["linear", "self_attention"])
def test_fused_and_separate_bias_gradient_agree(make, only_w1, seen, monkeypatch):
    backward, T = make()
    monkeypatch.setattr(G, "_BSUM_MODE", "0")
    backward()   # tunes (the single candidate) outside the counted runs
    before = K.STATS["colsum_act"]
    dx0, dW0, db0 = backward()
    assert K.STATS["colsum_act"] == before + 1
    monkeypatch.setattr(G, "_BSUM_MODE", "2")
    before = K.STATS["colsum_act"]
    dx1, dW1, db1 = backward()
    assert K.STATS["colsum_act"] == before, "the column-sum pass ran beside the fused bias gradient"
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    assert torch.equal(dW0.view(torch.int32), dW1.view(torch.int32))
    g = seen["g"]
    assert g.shape[0] == T and bool(torch.isfinite(db1).all())
    assert _within(db1, g, T, 1)
    bound = bsum_bound(T, 1, 1, g.double().abs().sum(0))
    assert bool(((db0.double() - db1.double()).abs() <= 2 * bound).all())


@pytest.mark.parametrize("make", [_linear, _attention], ids=["linear", "self_attention"])
def test_fused_bias_gradient_under_graph_capture(make, only_w1, seen, monkeypatch):
    backward, T = make()
    monkeypatch.setattr(G, "_BSUM_MODE", "2")
    backward()
    _, dW_e, db_e = backward()
    g = seen["g"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    before = K.STATS["colsum_act"]
    with torch.cuda.graph(graph):
        _, dW_g, db_g = backward()   # the gradient buffers are zeroed inside the graph
    assert K.STATS["colsum_act"] == before
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dW_e.view(torch.int32), dW_g.view(torch.int32))
    assert _within(db_g, g, T, 1)
    bound = bsum_bound(T, 1, 1, g.double().abs().sum(0))
    assert bool(((db_g.double() - db_e.double()).abs() <= 2 * bound).all())
