"""SWIGLU on the CPU: IR, the operator's torch fallback, the LLaMA spelling and the executor's gate / up fusion.

fp32 on the CPU; on a GPU machine the executor computes in bf16 on the device, which tests/test_swiglu_gpu.py covers.
"""
import pytest
import torch
import torch.nn.functional as F

from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.models.llama import LlamaConfig, build_llama
from flexflow_train_amd.ops import base as opbase

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="exercises the CPU paths")

F32 = C.DataType.FLOAT
TINY = dict(vocab_size=128, hidden_size=64, num_layers=2, num_heads=2, num_kv_heads=1, intermediate_size=128,
            sequence_length=16, batch_size=4)


def test_shape_inference_and_json_round_trip():
    op = C.OpAttrs("SWIGLU")
    x = C.TensorShape([3, 5, 64], F32)
    assert C.infer_output_shapes(op, [x, x])[0].dims == [3, 5, 64] and C.infer_weight_shapes(op, [x, x]) == []
    for other in ([3, 5, 32], [1, 5, 64], [5, 64]):   # no broadcasting
        with pytest.raises(ValueError, match="equal shapes"):
            C.infer_output_shapes(op, [x, C.TensorShape(other, F32)])
    P = C.ParallelTensorShape
    (o,) = C.infer_parallel_output_shapes(op, [P([4, 16, 64], [2, 1, 2], 1, 1, F32)] * 2)
    assert o.shard_degrees() == [2, 1, 2] and o.sum_degree == 1
    with pytest.raises(ValueError, match="shard degrees differ"):
        C.infer_parallel_output_shapes(op, [P([4, 16, 64], [2, 1, 2], 1, 1, F32), P([4, 16, 64], [2, 2, 1], 1, 1, F32)])
    with pytest.raises(ValueError, match="partial sums"):
        C.infer_parallel_output_shapes(op, [P([4, 16, 64], [1, 1, 1], 2, 1, F32)] * 2)
    m = FFModel(FFConfig())
    t = m.create_tensor([2, 6, 16], DataType.DT_FLOAT, name="x")
    m.swiglu(t, m.sigmoid(t, name="s"), name="gated")
    text = m.cg.to_json()
    assert C.ComputationGraph.from_json(text).to_json() == text and '"SWIGLU"' in text


def test_operator_matches_autograd():
    gen = torch.Generator().manual_seed(2)
    g, u, dy = (torch.randn(3, 5, 24, generator=gen) * s for s in (2.0, 1.0, 1.0))
    g[0, 0, :4] = torch.tensor([20.0, -20.0, 90.0, -90.0])
    impl = opbase.get_impl("SWIGLU")
    ctx = opbase.OpContext(op_type="SWIGLU", attrs={}, name="swiglu")
    (y,), saved = impl.forward(ctx, [g, u], [])
    dg, du = impl.backward(ctx, saved, [dy], [], [True, True])
    gr, ur = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ref = F.silu(gr) * ur
    ref.backward(dy)
    for got, want in ((y, ref.detach()), (dg, gr.grad), (du, ur.grad)):
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, want)


def _llama(swiglu_op, fuse):
    cfg = FFConfig()
    cfg.perform_fusion = fuse
    m = FFModel(cfg)
    build_llama(m, LlamaConfig(swiglu_op=swiglu_op, **TINY))
    m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    gen = torch.Generator().manual_seed(1)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=gen) * 0.05
                         + (1.0 if n.endswith("gamma") else 0.0))
    ids = torch.randint(0, 128, (4, 17), generator=gen, dtype=torch.int32)
    return ex, {"input_ids": ids[:, :16].contiguous()}, ids[:, 1:].long()


def _loss_and_grads(ex, feeds, labels):
    ex.forward(feeds, training=True)
    ex.backward(ex.compute_loss(labels))
    return torch.tensor(ex.perf_metrics().loss), {n: ex.get_parameter_grad(n).clone() for n in ex.parameter_names()}


@pytest.mark.parametrize("fuse", [False, True])
def test_llama_spellings_agree(fuse):
    """swiglu_op=True against the sigmoid / multiply / multiply chain from the same weights: the same
    loss and parameter gradients (the two differ only in fp32 rounding).  With perform_fusion, one
    FUSED_GATE_UP_SWIGLU step per layer stands in for the two projections and the SWIGLU."""
    a, feeds, labels = _llama(True, fuse)
    b, _, _ = _llama(False, fuse)
    kinds = [s.op_type for s in a.steps]
    assert kinds.count("FUSED_GATE_UP_SWIGLU") == (TINY["num_layers"] if fuse else 0)
    assert kinds.count("SWIGLU") == (0 if fuse else TINY["num_layers"])
    assert sorted(a.parameter_names()) == sorted(b.parameter_names())
    (la, ga), (lb, gb) = _loss_and_grads(a, feeds, labels), _loss_and_grads(b, feeds, labels)
    assert la > 1.0, "the loss was read"   # about ln(128) at these weights
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-6)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_second_reader_of_gate_keeps_the_steps_unfused():
    cfg = FFConfig()
    cfg.perform_fusion = True
    m = FFModel(cfg)
    x = m.create_tensor([4, 16], DataType.DT_FLOAT, name="x")
    gate = m.dense(x, 32, use_bias=False, name="gate")
    up = m.dense(x, 32, use_bias=False, name="up")
    m.add(m.swiglu(gate, up, name="gated"), gate, name="sum")
    m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    kinds = [s.op_type for s in m.executor.steps]
    assert kinds.count("LINEAR") == 2 and kinds.count("SWIGLU") == 1 and "FUSED_GATE_UP_SWIGLU" not in kinds
