"""Gated (SwiGLU) experts on the CPU: IR, the operator's torch path and the MoE LLaMA.

fp32 on the CPU; tests/test_moe_swiglu_gpu.py covers the device kernels.
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


def _experts(m, use_bias=False):
    x = m.create_tensor([32, 16], DataType.DT_FLOAT, name="x")
    vals, idx = m.top_k(m.softmax(m.dense(x, 4, name="router")), 2, True)
    return m.experts(x, idx, vals, 4, 24, out_dim=8, activation="swiglu", use_bias=use_bias, name="experts")


def test_shape_inference_refusal_and_json():
    op = C.OpAttrs("EXPERTS", num_experts=4, hidden_size=24, out_dim=8, activation="swiglu", use_bias=False)
    ins = [C.TensorShape([32, 16], F32), C.TensorShape([32, 2], C.DataType.INT32), C.TensorShape([32, 2], F32)]
    assert [w.dims for w in C.infer_weight_shapes(op, ins)] == [[4, 16, 48], [4, 24, 8]]      # w1 = [E, D, 2H]
    assert C.infer_output_shapes(op, ins)[0].dims == [32, 8]
    with pytest.raises(ValueError, match="swiglu.*use_bias"):
        _experts(FFModel(FFConfig()), use_bias=True)
    m = FFModel(FFConfig())
    _experts(m)
    text = m.cg.to_json()
    assert C.ComputationGraph.from_json(text).to_json() == text and '"swiglu"' in text


def test_operator_matches_fp64_autograd():
    g = torch.Generator().manual_seed(0)
    B, D, H, O, E, k = 40, 16, 24, 8, 4, 2
    ids = torch.stack([torch.randperm(E - 1, generator=g)[:k] for _ in range(B)]).to(torch.int32)   # expert 3 unused
    x, gate, dout = torch.randn(B, D, generator=g), torch.softmax(torch.randn(B, k, generator=g), -1), torch.randn(B, O, generator=g)
    w1, w2 = torch.randn(E, D, 2 * H, generator=g) * 0.2, torch.randn(E, H, O, generator=g) * 0.2
    impl = opbase.get_impl("EXPERTS")
    attrs = {"num_experts": E, "hidden_size": H, "out_dim": O, "activation": "swiglu", "use_bias": False}
    ctx = opbase.OpContext(op_type="EXPERTS", attrs=attrs, name="moe")
    (out,), saved = impl.forward(ctx, [x, ids, gate], [w1, w2])
    grads = [torch.zeros_like(w1), torch.zeros_like(w2)]
    dx, _, dgate = impl.backward(ctx, saved, [dout], grads, [True, False, True])
    xd, gd, w1d, w2d = (t.double().requires_grad_() for t in (x, gate, w1, w2))
    gu = torch.einsum("bd,bjdn->bjn", xd, w1d[ids.long()])                       # [B, k, 2H]
    y = torch.einsum("bjh,bjho->bjo", F.silu(gu[..., :H]) * gu[..., H:], w2d[ids.long()])
    ref = (y * gd.unsqueeze(-1)).sum(1)
    ref.backward(dout.double())
    for got, want in ((out, ref.detach()), (dx, xd.grad), (dgate, gd.grad), (grads[0], w1d.grad), (grads[1], w2d.grad)):
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)
    assert not grads[0][3].any() and not grads[1][3].any()
    with pytest.raises(ValueError, match="2H"):                                  # w1 of width H
        impl.forward(ctx, [x, ids, gate], [w1[:, :, :H].contiguous(), w2])
    with pytest.raises(ValueError, match="no biases"):
        impl.forward(opbase.OpContext(op_type="EXPERTS", attrs=dict(attrs, use_bias=True), name="moe"),
                     [x, ids, gate], [w1, torch.zeros(E, H), w2, torch.zeros(E, O)])


def _llama(**kw):
    m = FFModel(FFConfig())
    build_llama(m, LlamaConfig(**TINY, **kw))
    return m


def test_moe_llama_trains_and_default_is_unchanged():
    assert _llama(num_experts=0).cg.to_json() == _llama().cg.to_json()
    assert "EXPERTS" not in _llama().cg.to_json() and "router" not in _llama().cg.to_json()
    m = _llama(num_experts=4)
    assert m.cg.to_json().count('"EXPERTS"') == TINY["num_layers"] and "gate_proj" not in m.cg.to_json()
    m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    gen = torch.Generator().manual_seed(1)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=gen) * 0.05
                         + (1.0 if n.endswith("gamma") else 0.0))
    w1 = [n for n in ex.parameter_names() if "experts" in n and tuple(ex.get_parameter(n).shape) == (4, 64, 256)]
    assert len(w1) == TINY["num_layers"]
    router = next(n for n in sorted(ex.parameter_names()) if "layers0.router" in n)
    before = ex.get_parameter(router).clone()
    ids = torch.randint(0, 128, (4, 17), generator=gen, dtype=torch.int32)
    ex.train_step({"input_ids": ids[:, :16].contiguous()}, ids[:, 1:].long())
    loss = torch.tensor(ex.perf_metrics().loss)
    assert torch.isfinite(loss) and loss > 1.0                                    # about ln(128) at these weights
    assert not torch.equal(ex.get_parameter(router), before)
