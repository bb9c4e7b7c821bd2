"""RMS_NORM and ROPE on the CPU: shape inference and serialisation, the
operators' torch fallbacks against torch / Hugging Face references in fp64,
the EW_ADD -> RMS_NORM fusion, the LLaMA-style model against a plain torch
module, the torch.export / torch.fx importers, the strategy search and the
memory plan.
"""
import json
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights, string_to_ff
from flexflow_train_amd.models.llama import LlamaConfig, build_llama, llama_synthetic
from flexflow_train_amd.search import native

# fp32 on the CPU against fp64 references: on a GPU machine the executor computes in bf16 on the device,
# which tests/test_rmsnorm_rope_gpu.py covers
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="exercises the CPU paths")

F32 = C.DataType.FLOAT
P = C.ParallelTensorShape
TS = C.TensorShape
CPU_TOL = dict(rtol=1e-4, atol=1e-5)   # tests/test_fusions.py's CPU tolerance


# ------------------------------------------------------------------------ IR
def test_serial_shape_and_weight_inference():
    rms, plain = C.OpAttrs("RMS_NORM"), C.OpAttrs("RMS_NORM", elementwise_affine=False)
    x = TS([3, 5, 64], F32)
    assert C.infer_output_shapes(rms, [x])[0].dims == [3, 5, 64]
    assert [w.dims for w in C.infer_weight_shapes(rms, [x])] == [[64]] and C.weight_names(rms) == ["gamma"]
    assert C.infer_weight_shapes(plain, [x]) == [] and C.weight_names(plain) == []
    for sd, dims in ((-2, [2, 3, 130, 64]), (1, [2, 130, 3, 64]), (0, [7, 6])):
        rope = C.OpAttrs("ROPE", seq_dim=sd)
        assert C.infer_output_shapes(rope, [TS(dims, F32)])[0].dims == dims
        assert C.infer_weight_shapes(rope, [TS(dims, F32)]) == []
    bad = [(C.OpAttrs("ROPE"), [4, 7], "must be even"),
           (C.OpAttrs("ROPE", seq_dim=-1), [4, 8], "seq_dim cannot be the last dim"),
           (C.OpAttrs("ROPE", seq_dim=1), [4, 8], "seq_dim cannot be the last dim"),
           (C.OpAttrs("ROPE", seq_dim=5), [4, 8], "seq_dim out of range"),
           (C.OpAttrs("ROPE"), [8], "rank >= 2")]
    for op, dims, what in bad:
        with pytest.raises(ValueError, match=what):
            C.infer_output_shapes(op, [TS(dims, F32)])


def test_parallel_shape_inference():
    rms, rope = C.OpAttrs("RMS_NORM"), C.OpAttrs("ROPE", seq_dim=1)
    for b, h in ((1, 1), (2, 1), (1, 3), (2, 3)):
        x = P([4, 6, 16, 64], [b, h, 1, 1], 1, 1, F32)
        (o,) = C.infer_parallel_output_shapes(rms, [x])
        assert o.shard_degrees() == [b, h, 1, 1] and o.sum_degree == 1
        (g,) = C.infer_parallel_weight_shapes(rms, [x])
        # gamma is whole on every device: replicated over the batch / head degrees
        assert g.shard_degrees() == [1] and g.discard_copy_degree == b * h and g.sum_degree == 1
        # [B, S, H, D] with seq_dim = 1: batch and head degrees pass through
        y = P([4, 16, 6, 64], [b, 1, h, 1], 1, 1, F32)
        (o,) = C.infer_parallel_output_shapes(rope, [y])
        assert o.shard_degrees() == [b, 1, h, 1]
        assert C.infer_parallel_weight_shapes(rope, [y]) == []
    assert not C.is_valid_parallelization(rms, [P([4, 6, 16, 64], [1, 1, 1, 2], 1, 1, F32)])
    with pytest.raises(ValueError, match="normalized axis must be unpartitioned"):
        C.infer_parallel_output_shapes(rms, [P([4, 6, 16, 64], [1, 1, 1, 2], 1, 1, F32)])
    with pytest.raises(ValueError, match="partial-sum"):
        C.infer_parallel_output_shapes(rms, [P([4, 6, 16, 64], [1, 1, 1, 1], 2, 1, F32)])
    with pytest.raises(ValueError, match="position offset; sequence-parallel RoPE is out of scope"):
        C.infer_parallel_output_shapes(rope, [P([4, 16, 6, 64], [1, 2, 1, 1], 1, 1, F32)])
    with pytest.raises(ValueError, match="rotary dim .* must be unpartitioned"):
        C.infer_parallel_output_shapes(rope, [P([4, 16, 6, 64], [1, 1, 1, 2], 1, 1, F32)])
    with pytest.raises(ValueError, match="partial-sum"):
        C.infer_parallel_output_shapes(rope, [P([4, 16, 6, 64], [1, 1, 1, 1], 2, 1, F32)])


def test_json_round_trip_and_defaults():
    m = FFModel(FFConfig())
    x = m.create_tensor([2, 6, 4, 16], DataType.DT_FLOAT, name="x")
    m.rope(m.rms_norm(x, eps=1e-5, name="n"), theta=500000.0, seq_dim=1, interleaved=True, name="r")
    m.rope(m.rms_norm(x, elementwise_affine=False, name="n2"), name="r2")
    text = m.cg.to_json()
    again = C.ComputationGraph.from_json(text)
    assert again.to_json() == text and '"RMS_NORM"' in text and '"ROPE"' in text
    ops = {l["name"]: l["op"]["attrs"] for l in json.loads(text)["layers"] if l["op"]["op_type"] in ("RMS_NORM", "ROPE")}
    assert ops["n"]["eps"] == {"f": 1e-5} and ops["n"]["elementwise_affine"] is True
    assert ops["n2"]["eps"] == {"f": 1e-6} and ops["n2"]["elementwise_affine"] is False
    assert ops["r"] == {"theta": {"f": 500000.0}, "seq_dim": 1, "interleaved": True}
    assert ops["r2"] == {"theta": {"f": 10000.0}, "seq_dim": -2, "interleaved": False}
    assert [l.op_type for l in m.get_layers() if l.op_type in ("RMS_NORM", "ROPE")] == ["RMS_NORM", "ROPE"] * 2
    with pytest.raises(ValueError, match="seq_dim cannot be the last dim"):
        m.rope(x, seq_dim=3)


# ------------------------------------------------------------------ operators
def _op(op_type, attrs, inputs, weights, dy, wgrads):
    from flexflow_train_amd.ops import base as opbase
    impl = opbase.get_impl(op_type)
    ctx = opbase.OpContext(op_type=op_type, attrs=attrs, name=op_type.lower(), training=True)
    outs, saved = impl.forward(ctx, inputs, weights)
    grads = impl.backward(ctx, saved, [dy], wgrads, [True] * len(inputs))
    return outs[0], grads


@pytest.mark.parametrize("affine", [True, False])
def test_rms_norm_matches_torch_fp64(affine):
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(3, 5, 64, generator=g), torch.randn(3, 5, 64, generator=g)
    gamma = torch.randn(64, generator=g) if affine else None
    # through the model API: the executor runs the operator
    m = FFModel(FFConfig())
    xt = m.create_tensor([3, 5, 64], DataType.DT_FLOAT, name="x")
    m.rms_norm(xt, eps=1e-5, elementwise_affine=affine, name="n")
    m.compile(optimizer=SGDOptimizer(m, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    ex = m.executor
    assert sorted(ex.parameter_names()) == (["n.gamma"] if affine else [])
    if affine:
        assert torch.equal(ex.get_parameter("n.gamma"), torch.ones(64)), "gamma starts at one"
        ex.set_parameter("n.gamma", gamma)
    out = ex.forward({"x": x}, training=True)
    ex.backward(dy)
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True) if affine else None
    ref = F.rms_norm(xr, (64,), gr, 1e-5)
    ref.backward(dy.double())
    torch.testing.assert_close(out.double(), ref.detach(), rtol=1e-5, atol=1e-6)
    if affine:
        torch.testing.assert_close(ex.get_parameter_grad("n.gamma").double(), gr.grad, rtol=1e-5, atol=1e-5)
    # the input gradient, from the operator itself
    wg = [torch.zeros(64)] if affine else []
    y, (dx,) = _op("RMS_NORM", dict(eps=1e-5, elementwise_affine=affine), [x], [gamma] if affine else [], dy, wg)
    torch.testing.assert_close(y.double(), ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dx.double(), xr.grad, rtol=1e-5, atol=1e-6)
    if affine:
        torch.testing.assert_close(wg[0].double(), gr.grad, rtol=1e-5, atol=1e-5)


def _cos_sin64(S, D, theta=10000.0):
    inv = theta ** (-torch.arange(0, D // 2, dtype=torch.float64) * 2.0 / D)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cos(ang), torch.sin(ang)   # [S, D / 2]


def _rope_model(shape, seq_dim, interleaved=False):
    m = FFModel(FFConfig())
    xt = m.create_tensor(list(shape), DataType.DT_FLOAT, name="x")
    m.rope(xt, seq_dim=seq_dim, interleaved=interleaved, name="r")
    m.compile(optimizer=SGDOptimizer(m, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    return m.executor


@pytest.mark.parametrize("shape,seq_dim", [((2, 3, 130, 64), -2), ((2, 130, 3, 64), 1)])
def test_rope_matches_hugging_face(shape, seq_dim):
    hf = pytest.importorskip("transformers.models.llama.modeling_llama")
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    out = _rope_model(shape, seq_dim).forward({"x": x}, training=True)
    y, (dx,) = _op("ROPE", dict(seq_dim=seq_dim), [x], [], dy, [])
    assert torch.equal(out, y)
    c, s = _cos_sin64(130, 64)
    cos, sin = torch.cat([c, c], -1)[None], torch.cat([s, s], -1)[None]   # [1, S, D], fp64
    xr = x.double().requires_grad_(True)
    # apply_rotary_pos_emb broadcasts cos / sin over the heads dim: dim 1 of [B, H, S, D], dim 2 of [B, S, H, D]
    ref, _ = hf.apply_rotary_pos_emb(xr, xr, cos, sin, unsqueeze_dim=1 if seq_dim == -2 else 2)
    ref.backward(dy.double())
    # fp32 math on an fp32 table: a few fp32 roundings of values of size <= |x| sqrt(2)
    torch.testing.assert_close(y.double(), ref.detach(), rtol=0, atol=2e-6)
    torch.testing.assert_close(dx.double(), xr.grad, rtol=0, atol=2e-6)
    pos0 = (slice(None), slice(None), 0) if seq_dim == -2 else (slice(None), 0)
    assert torch.equal(y[pos0], x[pos0]), "position 0 is the identity, bit for bit"


def test_rope_interleaved_matches_fp64_reference():
    g = torch.Generator().manual_seed(5)
    shape = (2, 130, 3, 64)
    x, dy = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    y, (dx,) = _op("ROPE", dict(seq_dim=1, interleaved=True), [x], [], dy, [])
    out = _rope_model(shape, 1, True).forward({"x": x}, training=True)
    assert torch.equal(out, y)
    c, s = (t[None, :, None, :] for t in _cos_sin64(130, 64))
    xr = x.double().requires_grad_(True)
    a, b = xr[..., 0::2], xr[..., 1::2]
    ref = torch.stack([a * c - b * s, b * c + a * s], -1).flatten(-2)
    ref.backward(dy.double())
    torch.testing.assert_close(y.double(), ref.detach(), rtol=0, atol=2e-6)
    torch.testing.assert_close(dx.double(), xr.grad, rtol=0, atol=2e-6)
    assert torch.equal(y[:, 0], x[:, 0])


def test_rope_fallback_takes_other_rotary_dims():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 5, 24, generator=g)
    y, (dx,) = _op("ROPE", {}, [x], [], x, [])
    c, s = _cos_sin64(5, 24)
    a, b = x.double()[..., :12], x.double()[..., 12:]
    torch.testing.assert_close(y.double(), torch.cat([a * c - b * s, b * c + a * s], -1), rtol=0, atol=2e-6)


# -------------------------------------------------------- tiny LLaMA, fusion
TINY = dict(vocab_size=128, hidden_size=64, num_layers=2, num_heads=2, num_kv_heads=1, intermediate_size=128,
            sequence_length=16, batch_size=4)


def _llama(fuse, optimizer="adam"):
    cfg = FFConfig()
    cfg.perform_fusion = fuse
    m = FFModel(cfg)
    lc = LlamaConfig(**TINY)
    build_llama(m, lc)
    opt = AdamOptimizer(m, alpha=1e-3) if optimizer == "adam" else SGDOptimizer(m, lr=0.1)
    m.compile(optimizer=opt, loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              metrics=[MetricsType.METRICS_SPARSE_CATEGORICAL_CROSSENTROPY])
    ex = m.executor
    g = torch.Generator().manual_seed(1)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.05
                         + (1.0 if n.endswith("gamma") else 0.0))
    ids = torch.randint(0, 128, (4, 17), generator=g, dtype=torch.int32)
    return ex, {"input_ids": ids[:, :16].contiguous()}, ids[:, 1:].long()


def test_add_rms_norm_fusion_matches_unfused():
    a, feeds, labels = _llama(True)
    b, _, _ = _llama(False)
    fused = [s for s in a.steps if s.op_type == "FUSED_ADD_RMS_NORM"]
    # two residual adds per block, each followed by a norm (the last one by the final norm)
    assert len(fused) >= 4, [s.op_type for s in a.steps]
    # the sum of every add but the last is also the residual stream of the next add: emit_sum
    assert sum(1 for s in fused if s.ctx.extra.get("emit_sum")) == len(fused) - 1 >= 3
    assert all(len(s.outputs) == (2 if s.ctx.extra.get("emit_sum") else 1) for s in fused)
    assert not any(s.op_type == "EW_ADD" for s in a.steps), "every residual add is fused"
    assert not any(s.op_type == "FUSED_ADD_RMS_NORM" for s in b.steps)
    assert sum(1 for s in b.steps if s.op_type == "EW_ADD") == 4
    for _ in range(3):
        a.train_step(feeds, labels)
        b.train_step(feeds, labels)
    for n in a.parameter_names():
        torch.testing.assert_close(a.get_parameter(n), b.get_parameter(n), **CPU_TOL)


# ------------------------------------------------------- against plain torch
def _torch_rope(x, theta=10000.0):
    """[B, S, H, D], half-split, from an fp64-built table."""
    S, D = x.shape[1], x.shape[3]
    c, s = (t.to(x.dtype)[None, :, None, :] for t in _cos_sin64(S, D, theta))
    a, b = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


class Block(nn.Module):
    def __init__(self, E=64, H=2, Hkv=1, I=128, eps=1e-6, rope=True):
        super().__init__()
        self.H, self.Hkv, self.D, self.rope = H, Hkv, E // H, rope
        self.input_norm, self.post_attn_norm = nn.RMSNorm(E, eps=eps), nn.RMSNorm(E, eps=eps)
        self.q_proj = nn.Linear(E, E, bias=False)
        self.k_proj, self.v_proj = nn.Linear(E, Hkv * self.D, bias=False), nn.Linear(E, Hkv * self.D, bias=False)
        self.o_proj = nn.Linear(E, E, bias=False)
        self.gate_proj, self.up_proj = nn.Linear(E, I, bias=False), nn.Linear(E, I, bias=False)
        self.down_proj = nn.Linear(I, E, bias=False)

    def forward(self, x):
        h = self.input_norm(x)
        q = self.q_proj(h).reshape(4, 16, self.H, self.D)
        k = self.k_proj(h).reshape(4, 16, self.Hkv, self.D)
        v = self.v_proj(h).reshape(4, 16, self.Hkv, self.D)
        if self.rope:
            q, k = _torch_rope(q), _torch_rope(k)
        a = F.scaled_dot_product_attention(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
                                           is_causal=True, enable_gqa=True)
        x = x + self.o_proj(a.permute(0, 2, 1, 3).reshape(4, 16, self.H * self.D))
        h = self.post_attn_norm(x)
        return x + self.down_proj(F.silu(self.gate_proj(h)) * self.up_proj(h))


class TorchLlama(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed_tokens = nn.Embedding(128, 64)
        self.layers = nn.ModuleList([Block(), Block()])
        self.norm = nn.RMSNorm(64, eps=1e-6)
        self.lm_head = nn.Linear(64, 128, bias=False)

    def forward(self, ids):
        x = self.embed_tokens(ids)
        for blk in self.layers:
            x = blk(x)
        return self.lm_head(self.norm(x))


def test_llama_trains_like_plain_torch():
    ex, feeds, labels = _llama(True, optimizer="sgd")
    net = TorchLlama()
    sd = {}
    for n in ex.parameter_names():
        p = ex.get_parameter(n)
        layer, w = n.rsplit(".", 1)
        layer = layer.replace("layers0", "layers.0").replace("layers1", "layers.1")
        sd[layer + ".weight"] = p.t().contiguous() if w == "kernel" else p.clone()
    net.load_state_dict(sd)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    ids = feeds["input_ids"].long()
    for _ in range(3):
        ex.train_step(feeds, labels)
        opt.zero_grad()
        F.cross_entropy(net(ids).reshape(-1, 128), labels.reshape(-1)).backward()
        opt.step()
    moved = 0.0
    for k, want in net.state_dict().items():
        layer, _ = k.rsplit(".", 1)
        layer = layer.replace("layers.0", "layers0").replace("layers.1", "layers1")
        name = next(n for n in ex.parameter_names() if n.rsplit(".", 1)[0] == layer)
        got = ex.get_parameter(name)
        torch.testing.assert_close(got.t() if name.endswith("kernel") else got, want, **CPU_TOL)
        moved = max(moved, float((want - sd[k]).abs().max()))
    assert moved > 1e-3, "the steps changed the weights"


# ------------------------------------------------------------------ importers
def _import_block(path):
    torch.manual_seed(11)
    net = Block(rope=False)
    with torch.no_grad():
        for norm in (net.input_norm, net.post_attn_norm):
            norm.weight.add_(0.1 * torch.randn(64))
    ff = FFModel(FFConfig())
    x = ff.create_tensor([4, 16, 64], DataType.DT_FLOAT, name="x")
    pm = PyTorchModel(net)
    if path == "export":
        pm.graph = None
    else:
        assert pm.graph is not None, pm.trace_error
    (out,) = pm.torch_to_ff(ff, [x])
    ff.compile(optimizer=SGDOptimizer(ff, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    copy_weights(ff, pm.weights() if path == "fx" else None)
    return net, ff


@pytest.mark.parametrize("path", ["export", "fx"])
def test_import_yields_rms_norm_nodes(path):
    net, ff = _import_block(path)
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("RMS_NORM") == 2 and types.count("SDPA") == 1, types
    assert not {"POW", "MEAN", "RSQRT"} & set(types), types
    assert types.count("SIGMOID") == 1, "SiLU is multiply(x, sigmoid(x))"
    eps = [l["op"]["attrs"]["eps"] for l in json.loads(ff.cg.to_json())["layers"] if l["op"]["op_type"] == "RMS_NORM"]
    assert eps == [{"f": 1e-6}] * 2
    # trains to torch's weights: equal outputs and equal gradients of every parameter
    g = torch.Generator().manual_seed(12)
    inp, dout = torch.randn(4, 16, 64, generator=g), torch.randn(4, 16, 64, generator=g)
    ex = ff.executor
    out = ex.forward({"x": inp}, training=True)
    want = net(inp)
    torch.testing.assert_close(out.float(), want, rtol=1e-5, atol=1e-5)
    ex.backward(dout)
    want.backward(dout)
    names = list(ex.parameter_names())
    assert len(names) == 9
    for p in net.parameters():
        wt = p.detach().t() if p.dim() == 2 else p.detach()
        (n,) = [n for n in names if ex.get_parameter(n).shape == wt.shape and torch.equal(ex.get_parameter(n), wt)]
        gt = p.grad.t() if p.dim() == 2 else p.grad
        torch.testing.assert_close(ex.get_parameter_grad(n), gt, rtol=1e-4, atol=1e-5)


def test_functional_rms_norm_and_default_eps():
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.linspace(0.5, 1.5, 64))
            self.fc = nn.Linear(64, 8)

        def forward(self, x):
            return self.fc(F.silu(F.rms_norm(x, (64,), self.w)))

    for path in ("export", "fx"):
        net = Net()
        ff = FFModel(FFConfig())
        x = ff.create_tensor([4, 64], DataType.DT_FLOAT, name="x")
        pm = PyTorchModel(net)
        if path == "export":
            pm.graph = None
        else:
            assert pm.graph is not None, pm.trace_error
        pm.torch_to_ff(ff, [x])
        ff.compile(optimizer=SGDOptimizer(ff, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
        copy_weights(ff, pm.weights() if path == "fx" else None)
        (op,) = [l["op"]["attrs"] for l in json.loads(ff.cg.to_json())["layers"] if l["op"]["op_type"] == "RMS_NORM"]
        assert op["eps"] == {"f": float(torch.finfo(torch.float32).eps)}, "a missing eps is torch's default"
        inp = torch.randn(4, 64, generator=torch.Generator().manual_seed(2))
        torch.testing.assert_close(ff.executor.forward({"x": inp}, training=False).float(), net(inp), rtol=1e-5,
                                   atol=1e-5)


def test_ff_text_ir_round_trip():
    net = Block(rope=False)
    lines = PyTorchModel(net).torch_to_string()
    rms = [l for l in lines if "; RMS_NORM; " in l]
    assert len(rms) == 2 and all(l.endswith("RMS_NORM; 1e-06; 1") for l in rms), rms
    assert sum("; SIGMOID" in l for l in lines) == 1 and sum("; SDPA; " in l for l in lines) == 1
    ff = FFModel(FFConfig())
    (o,) = string_to_ff(lines, ff, [ff.create_tensor([4, 16, 64], DataType.DT_FLOAT, name="x")])
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("RMS_NORM") == 2 and types.count("SDPA") == 1 and types.count("SIGMOID") == 1
    assert list(o.dims) == [4, 16, 64]
    # written again from the text, the lines are the same
    ff2 = FFModel(FFConfig())
    (o2,) = string_to_ff(["x; ; n,; INPUT", "n; x,; out,; RMS_NORM; 0.001; 0", "out; n,; ; OUTPUT"], ff2,
                         [ff2.create_tensor([4, 64], DataType.DT_FLOAT, name="x")])
    (op,) = [l["op"]["attrs"] for l in json.loads(ff2.cg.to_json())["layers"] if l["op"]["op_type"] == "RMS_NORM"]
    assert op == {"eps": {"f": 0.001}, "elementwise_affine": False}


# ----------------------------------------------------------- search and plan
def _llama_graph():
    m = FFModel(FFConfig())
    build_llama(m, LlamaConfig(**dict(TINY, batch_size=8, num_heads=4, num_kv_heads=2)))
    return m


def test_strategy_search_and_memory_plan_over_llama():
    m = _llama_graph()
    cm = native.cost_model()
    world = 8   # one node of eight devices
    pcg, mapping, _ = C.lower_strategy(m.cg, C.data_parallel_strategy(m.cg, world), world)
    pcg.reinfer_shapes()
    for l in m.get_layers():
        if l.op_type in ("RMS_NORM", "ROPE"):
            assert pcg.shape(C.ValueRef(mapping[l.node], 0)).shard_degrees()[0] == world
    cfg = json.dumps({"world": world, "budget": 30, "time_limit": 20, "seed": 1})
    pcg2, rep = C.unity_search(C.data_parallel_pcg(m.cg, world), cm, cfg)[:2]
    rep = json.loads(rep)
    assert math.isfinite(rep["cost"]) and 0 < rep["cost"] <= rep["data_parallel_cost"] * 1.0000001
    pcg2.reinfer_shapes()
    plans = native.plan_memory(C.data_parallel_pcg(m.cg, world), world, with_blocks=True, act_elem_bytes=2.0,
                               executor_fusions=True)
    assert len(plans) == world and all(p["peak_live_bytes"] > p["weight_bytes"] > 0 for p in plans)
    # one device, with blocks: the norms' activations are in the plan
    one = C.data_parallel_pcg(m.cg, 1)
    (p,) = native.plan_memory(one, 1, with_blocks=True, act_elem_bytes=2.0, executor_fusions=True)
    assert any(one.layer_op(b["node"]).op_type == "RMS_NORM" for b in p["blocks"] if b["kind"] == 0)


def test_model_zoo_and_synthetic_batch():
    from flexflow_train_amd import models
    assert models.MODELS["llama"][1] is build_llama
    cfg = LlamaConfig(**TINY)
    import numpy as np
    feeds, labels = llama_synthetic(cfg, np.random.default_rng(0))
    assert feeds["input_ids"].shape == (4, 16) and labels.shape == (4, 16)


def test_other_executors_refuse_the_nodes():
    for build, what in ((lambda m, x: m.rms_norm(x, name="n"), "RMS_NORM .*node n"),
                        (lambda m, x: m.rope(x, name="r"), "ROPE .*node r")):
        cfg = FFConfig()
        cfg.local_execution = True
        m = FFModel(cfg)
        x = m.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")
        m.softmax(m.dense(build(m, x), 5, name="head"), name="sm")
        with pytest.raises(ValueError, match=what):
            C.LocalTrainingBacking(m.cg)
