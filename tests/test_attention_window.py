"""SDPA attribute ``window`` on the CPU: shape inference, serialisation, the fallback, a tiny LLaMA."""
import json
import math

import pytest
import torch

from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType
from flexflow_train_amd.models.llama import LlamaConfig, build_llama
from flexflow_train_amd.ops import base as opbase

TS, F32 = C.TensorShape, C.DataType.FLOAT
B, H, HKV, S, D = 2, 4, 2, 12, 8


def test_shape_inference_and_serialisation():
    ins = [TS([B, H, S, D], F32), TS([B, HKV, S, D], F32), TS([B, HKV, S, D], F32)]
    assert C.infer_output_shapes(C.OpAttrs("SDPA", causal=True, window=5), ins)[0].dims == [B, H, S, D]
    with pytest.raises(ValueError, match="window needs causal"):
        C.infer_output_shapes(C.OpAttrs("SDPA", window=5), ins)
    with pytest.raises(ValueError, match="window must be >= 1"):
        C.infer_output_shapes(C.OpAttrs("SDPA", causal=True, window=0), ins)
    texts = []
    for window in (None, 5):
        m = FFModel(FFConfig())
        q, k, v = (m.create_tensor([B, h, S, D], DataType.DT_FLOAT, name=n) for n, h in (("q", H), ("k", HKV), ("v", HKV)))
        m.scaled_dot_product_attention(q, k, v, causal=True, window=window, name="attn")
        texts.append(m.cg.to_json())
        assert C.ComputationGraph.from_json(texts[-1]).to_json() == texts[-1]
    assert "window" not in texts[0], "a model without a window serialises as before"
    (attrs,) = [l["op"]["attrs"] for l in json.loads(texts[1])["layers"] if l["op"]["op_type"] == "SDPA"]
    assert attrs["window"] == 5


@pytest.mark.parametrize("W", [1, 5, S])
def test_torch_fallback_matches_fp64(W):
    g = torch.Generator().manual_seed(3)
    q, do = torch.randn(B, H, S, D, generator=g), torch.randn(B, H, S, D, generator=g)
    k, v = torch.randn(B, HKV, S, D, generator=g), torch.randn(B, HKV, S, D, generator=g)
    impl = opbase.get_impl("SDPA")
    ctx = opbase.OpContext(op_type="SDPA", attrs=dict(causal=True, window=W), name="sdpa", training=True)
    (o,), saved = impl.forward(ctx, [q, k, v], [])
    grads = impl.backward(ctx, saved, [do], [], [True] * 3)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    d = torch.arange(S).view(S, 1) - torch.arange(S).view(1, S)   # q - k
    s = qd @ kd.repeat_interleave(H // HKV, dim=1).transpose(-1, -2) / math.sqrt(D)
    ref = torch.softmax(s.masked_fill((d < 0) | (d >= W), float("-inf")), -1) @ vd.repeat_interleave(H // HKV, dim=1)
    ref.backward(do.double())
    for got, want in zip((o, *grads), (ref.detach(), qd.grad, kd.grad, vd.grad)):
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5)


def test_llama_sliding_window_reaches_the_operator():
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 128, (2, 33), generator=g, dtype=torch.int32)
    feeds, labels = {"input_ids": ids[:, :32].contiguous()}, ids[:, 1:].long()
    loss = {}
    for W in (0, 8):
        m = FFModel(FFConfig())
        build_llama(m, LlamaConfig(vocab_size=128, hidden_size=64, num_layers=2, num_heads=2, num_kv_heads=1,
                                   intermediate_size=128, sequence_length=32, batch_size=2, sliding_window=W))
        m.compile(optimizer=AdamOptimizer(m, alpha=1e-3), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
        ex = m.executor
        assert [s.ctx.attrs.get("window", 0) for s in ex.steps if s.op_type == "SDPA"] == [W, W]
        pg = torch.Generator().manual_seed(2)
        for n in sorted(ex.parameter_names()):
            ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=pg) * 0.3
                             + (1.0 if n.endswith("gamma") else 0.0))
        before = {n: ex.get_parameter(n).clone() for n in ex.parameter_names()}
        probs = ex.forward(feeds, training=False, keep_outputs=True).float()
        loss[W] = float(-probs.gather(-1, labels.unsqueeze(-1)).log().mean())
        ex.train_step(feeds, labels)
        after = {n: ex.get_parameter(n) for n in before}
        assert all(torch.isfinite(t).all() for t in after.values())
        assert any(not torch.equal(after[n], before[n]) for n in before)
    assert math.isfinite(loss[8]) and abs(loss[8] - loss[0]) > 1e-6, loss
