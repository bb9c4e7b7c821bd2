"""The SDPA operator (scaled-dot-product attention without projections, with an
additive mask) on the CPU: the torch fallback against
F.scaled_dot_product_attention, shape inference, serialisation, the strategy
search, the torch.export / torch.fx importers and the executors that refuse it.
"""
import json
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights, string_to_ff
from flexflow_train_amd.ops import base as opbase

F32, I32, BOOL = C.DataType.FLOAT, C.DataType.INT32, C.DataType.BOOL
P = C.ParallelTensorShape
TS = C.TensorShape
B, H, SQ, SK, D = 2, 3, 10, 12, 8


# ------------------------------------------------------------------ operator
def _op(attrs, inputs, do):
    impl = opbase.get_impl("SDPA")
    ctx = opbase.OpContext(op_type="SDPA", attrs=attrs, name="sdpa", training=True)
    (o,), saved = impl.forward(ctx, inputs, [])
    grads = impl.backward(ctx, saved, [do], [], [True] * len(inputs))
    return o, grads


@pytest.mark.parametrize("case", ["none", "float", "float_b11k", "bool", "causal", "scale"])
def test_torch_fallback_matches_torch_sdpa(case):
    g = torch.Generator().manual_seed(3)
    sk = SQ if case == "causal" else SK
    q = torch.randn(B, H, SQ, D, generator=g)
    k, v = torch.randn(B, H, sk, D, generator=g), torch.randn(B, H, sk, D, generator=g)
    do = torch.randn(B, H, SQ, D, generator=g)
    mask, kw, attrs = None, {}, {}
    if case == "float":
        mask = torch.randn(1, H, SQ, sk, generator=g)
    elif case == "float_b11k":
        mask = torch.zeros(B, 1, 1, sk).masked_fill(torch.rand(B, 1, 1, sk, generator=g) < 0.3, float("-inf"))
        mask[..., 0] = 0.0
    elif case == "bool":
        mask = torch.rand(B, H, SQ, sk, generator=g) < 0.7
        mask[..., 0] = True
    elif case == "causal":
        kw, attrs = dict(is_causal=True), dict(causal=True)
    elif case == "scale":
        kw, attrs = dict(scale=0.37), dict(scale=0.37)
    if mask is not None:
        attrs["mask"] = True
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qr, kr, vr, attn_mask=mask, **kw)
    ref.backward(do)
    o, grads = _op(attrs, [q, k, v] + ([mask] if mask is not None else []), do)
    assert o.shape == (B, H, SQ, D) and len(grads) == (4 if mask is not None else 3)
    assert mask is None or grads[3] is None, "the mask gets no gradient"
    for got, want in zip((o, *grads[:3]), (ref, qr.grad, kr.grad, vr.grad)):
        torch.testing.assert_close(got, want.detach(), rtol=1e-5, atol=1e-5)


def test_fully_masked_row_gives_zeros():
    g = torch.Generator().manual_seed(4)
    q, k, v, do = (torch.randn(B, H, SQ, SQ, generator=g)[..., :D].contiguous() for _ in range(4))
    mask = torch.zeros(B, 1, SQ, SQ)
    mask[0, 0, 4] = float("-inf")
    o, grads = _op(dict(mask=True), [q, k, v, mask], do)
    assert not o[0, :, 4].any() and not grads[0][0, :, 4].any()
    assert all(torch.isfinite(t).all() for t in (o, *grads[:3]))


def test_operator_input_errors():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, SQ, D, generator=g)
    k = torch.randn(B, H, SK, D, generator=g)
    with pytest.raises(ValueError, match="causal needs Sq == Sk"):
        _op(dict(causal=True), [q, k, k], q)
    with pytest.raises(ValueError, match="causal cannot be combined"):
        _op(dict(causal=True, mask=True), [q, q, q, torch.zeros(1, 1, SQ, SQ)], q)
    with pytest.raises(ValueError, match="not broadcastable"):
        _op(dict(mask=True), [q, k, k, torch.zeros(B, 2, SQ, SK)], q)
    with pytest.raises(ValueError, match="float or bool"):
        _op(dict(mask=True), [q, k, k, torch.zeros(B, H, SQ, SK, dtype=torch.int32)], q)


# ----------------------------------------------------------- shape inference
def _shapes(sq=SQ, sk=SK):
    return [TS([B, H, sq, D], F32), TS([B, H, sk, D], F32), TS([B, H, sk, D], F32)]


def test_serial_shape_inference():
    op3, op4 = C.OpAttrs("SDPA"), C.OpAttrs("SDPA", mask=True)
    assert C.num_data_inputs(op3) == 3 and C.num_data_inputs(op4) == 4
    assert C.infer_output_shapes(op3, _shapes())[0].dims == [B, H, SQ, D]
    assert C.infer_weight_shapes(op3, _shapes()) == []
    for md in ([B, H, SQ, SK], [1, H, SQ, SK], [B, 1, 1, SK], [1, 1, SQ, SK], [1, 1, 1, 1]):
        assert C.infer_output_shapes(op4, _shapes() + [TS(md, F32)])[0].dims == [B, H, SQ, D]
    assert C.infer_output_shapes(C.OpAttrs("SDPA", causal=True), _shapes(SQ, SQ))[0].dims == [B, H, SQ, D]
    q, k, v = _shapes()
    bad = [(op3, [TS([B, SQ, D], F32), TS([B, SK, D], F32), TS([B, SK, D], F32)], "rank 4"),
           (op3, [q, TS([B + 1, H, SK, D], F32), v], "batch mismatch"),
           (op3, [q, TS([B, H + 1, SK, D], F32), TS([B, H + 1, SK, D], F32)], "head count mismatch"),
           (op3, [q, TS([B, H, SK, D + 1], F32), v], "head dim mismatch"),
           (op3, [q, k, TS([B, H, SK, D + 8], F32)], "v's last dim"),
           (op4, [q, k, v, TS([B, 2, SQ, SK], F32)], "1 or the full extent"),
           (op4, [q, k, v, TS([B, H, SQ, SK + 1], F32)], "1 or the full extent"),
           (op4, [q, k, v, TS([H, SQ, SK], F32)], "mask must be rank 4"),
           (op4, [q, k, v, TS([B, H, SQ, SK], I32)], "float dtype"),
           (op4, [q, k, v, TS([B, H, SQ, SK], BOOL)], "float dtype"),
           (C.OpAttrs("SDPA", causal=True, mask=True), _shapes(SQ, SQ) + [TS([1, 1, SQ, SQ], F32)],
            "causal cannot be combined with a mask"),
           (C.OpAttrs("SDPA", causal=True), [q, k, v], "causal needs Sq == Sk"),
           (op4, [q, k, v], "expected 4 inputs"),
           (op3, [q, k, v, TS([B, H, SQ, SK], F32)], "expected 3 inputs")]
    for op, ins, what in bad:
        with pytest.raises(ValueError, match=what):
            C.infer_output_shapes(op, ins)


def test_parallel_shape_inference():
    op3, op4 = C.OpAttrs("SDPA"), C.OpAttrs("SDPA", mask=True)

    def qkv(b, h, sdeg=1, ddeg=1):
        return [P([4, 6, SQ, D], [b, h, sdeg, ddeg], 1, 1, F32), P([4, 6, SK, D], [b, h, 1, 1], 1, 1, F32),
                P([4, 6, SK, D], [b, h, 1, 1], 1, 1, F32)]

    for b, h in ((1, 1), (2, 1), (1, 3), (2, 3), (4, 6)):
        (o,) = C.infer_parallel_output_shapes(op3, qkv(b, h))
        assert o.shard_degrees() == [b, h, 1, 1] and o.sum_degree == 1
        # a full mask dim follows q, a broadcast dim stays whole
        for md, deg in (([4, 6, SQ, SK], [b, h, 1, 1]), ([1, 6, SQ, SK], [1, h, 1, 1]),
                        ([4, 1, 1, SK], [b, 1, 1, 1]), ([1, 1, SQ, SK], [1, 1, 1, 1])):
            m = P(md, deg, 1, 1, F32)
            assert C.is_valid_parallelization(op4, qkv(b, h) + [m]), (b, h, md)
            assert C.infer_parallel_output_shapes(op4, qkv(b, h) + [m]) == [o]
    assert not C.is_valid_parallelization(op4, qkv(2, 3) + [P([4, 6, SQ, SK], [1, 3, 1, 1], 1, 1, F32)])
    assert not C.is_valid_parallelization(op4, qkv(2, 3) + [P([4, 6, SQ, SK], [2, 1, 1, 1], 1, 1, F32)])
    assert not C.is_valid_parallelization(op3, qkv(1, 1, sdeg=2)), "no sequence degree"
    assert not C.is_valid_parallelization(op3, qkv(1, 1, ddeg=2))
    bad = qkv(2, 1)
    bad[1] = P([4, 6, SK, D], [1, 1, 1, 1], 1, 1, F32)
    assert not C.is_valid_parallelization(op3, bad), "k's batch degree differs from q's"
    with pytest.raises(ValueError, match="sequence parallelism is not offered"):
        C.infer_parallel_output_shapes(op3, qkv(1, 1, sdeg=2))


# ------------------------------------------------- model, JSON, .ff, search
def _model(mask_dims=None, causal=False, cfg=None):
    m = FFModel(cfg or FFConfig())
    x = m.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")
    mask = m.create_tensor(mask_dims, DataType.DT_FLOAT, create_grad=False, name="mask") if mask_dims else None

    def heads(t):
        return m.transpose(m.reshape(t, [4, 6, 2, 8]), [0, 2, 1, 3])

    q, k, v = (heads(m.dense(x, 16, name=n)) for n in ("q", "k", "v"))
    a = m.scaled_dot_product_attention(q, k, v, mask=mask, causal=causal, dropout=0.0, scale=None, name="attn")
    a = m.reshape(m.transpose(a, [0, 2, 1, 3]), [4, 6, 16])
    m.softmax(m.dense(a, 5, name="head"), name="sm")
    return m


def test_ffmodel_builds_and_json_round_trips():
    for mask_dims, causal in ((None, False), (None, True), ([4, 1, 1, 6], False), ([1, 2, 6, 6], False)):
        m = _model(mask_dims, causal)
        (l,) = [l for l in m.get_layers() if l.op_type == "SDPA"]
        assert len(m.cg.layer_data_inputs(l.node)) == (4 if mask_dims else 3)
        assert m.cg.shape(C.ValueRef(l.node, 0)).dims == [4, 2, 6, 8]
        text = m.cg.to_json()
        again = C.ComputationGraph.from_json(text)
        assert again.to_json() == text and '"SDPA"' in text
    with pytest.raises(ValueError, match="causal cannot be combined with a mask"):
        _model([1, 1, 6, 6], True)


def test_model_trains_like_the_unfused_chain():
    """The same weights through SDPA and through batch_matmul / softmax / batch_matmul: one SGD step, equal weights."""
    def build(fused):
        m = FFModel(FFConfig())
        x = m.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")
        mask = m.create_tensor([4, 1, 1, 6], DataType.DT_FLOAT, create_grad=False, name="mask")
        q, k, v = (m.transpose(m.reshape(m.dense(x, 16, name=n), [4, 6, 2, 8]), [0, 2, 1, 3]) for n in "qkv")
        if fused:
            a = m.scaled_dot_product_attention(q, k, v, mask=mask, name="attn")
        else:
            s = m.scalar_multiply(m.batch_matmul(q, m.transpose(k, [0, 1, 3, 2])), 1.0 / math.sqrt(8))
            a = m.batch_matmul(m.softmax(m.add(s, mask), 3), v)
        a = m.reshape(m.transpose(a, [0, 2, 1, 3]), [4, 6, 16])
        m.softmax(m.dense(a, 5, name="head"), name="sm")
        m.compile(optimizer=SGDOptimizer(m, lr=0.5), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
        ex = m.executor
        g = torch.Generator().manual_seed(0)
        for n in sorted(ex.parameter_names()):
            ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.3)
        mk = torch.zeros(4, 1, 1, 6)
        mk[1, 0, 0, 4:] = -1e4   # finite: the unfused softmax has no zero-row rule
        mk[3, 0, 0, 2:] = -1e4
        ex.train_step({"x": torch.randn(4, 6, 16, generator=g), "mask": mk},
                      torch.randint(0, 5, (4, 6), generator=g, dtype=torch.int32))
        return {n: ex.get_parameter(n).double() for n in sorted(ex.parameter_names())}

    a, b = build(True), build(False)
    assert a.keys() == b.keys()
    for n in a:
        torch.testing.assert_close(a[n], b[n], rtol=1e-5, atol=1e-6)


def test_strategy_search_over_a_model_with_the_node():
    from flexflow_train_amd.search import native

    m = _model([4, 1, 1, 6])
    (l,) = [l for l in m.get_layers() if l.op_type == "SDPA"]
    cands = [json.loads(c) for c in C.candidate_configs(m.cg, l.node, 4)]
    assert cands and all(c["seq"] == 1 for c in cands), "sequence degree is not offered"
    assert any(c["batch"] == 4 for c in cands) and any(c["kind"] == "heads" and c["model"] == 2 for c in cands)
    cm = native.cost_model()
    cfg = json.dumps({"world": 4, "budget": 100, "time_limit": 20, "seed": 1})
    for pcg, rep in (C.graph_optimize(m.cg, cm, cfg)[:2], C.mcmc_search(m.cg, cm, cfg)[:2],
                     C.unity_search(C.data_parallel_pcg(m.cg, 4), cm, cfg)[:2]):
        rep = json.loads(rep)
        assert math.isfinite(rep["cost"]) and 0 < rep["cost"] <= rep["data_parallel_cost"] * 1.0000001
        pcg.reinfer_shapes()
    # data parallel: the mask's full batch dim gets q's degree, its broadcast dims stay whole
    pcg, mapping, _ = C.lower_strategy(m.cg, C.data_parallel_strategy(m.cg, 4), 4)
    degrees = [pcg.shape(v).shard_degrees() for v in pcg.layer_data_inputs(mapping[l.node])]
    assert degrees == [[4, 1, 1, 1]] * 4


def test_local_execution_refuses_the_node():
    cfg = FFConfig()
    cfg.local_execution = True
    m = _model(None, True, cfg)
    with pytest.raises(ValueError, match="SDPA node attn"):
        m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    with pytest.raises(ValueError, match="SDPA node attn"):
        C.LocalTrainingBacking(m.cg)


# ----------------------------------------------------------------- frontends
class Attn(nn.Module):
    """[4, 6, 16] -> two heads of 8 -> F.scaled_dot_product_attention -> [4, 6, 5]."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.q, self.k, self.v, self.out = nn.Linear(16, 16), nn.Linear(16, 16), nn.Linear(16, 16), nn.Linear(16, 5)
        g = torch.Generator().manual_seed(7)
        if kind == "bool_mask":
            keep = torch.rand(4, 1, 6, 6, generator=g) < 0.6
            keep[..., 0] = True
            self.register_buffer("mask", keep)
        elif kind == "param_bias":
            self.mask = nn.Parameter(torch.randn(1, 2, 6, 6, generator=g))

    def forward(self, x):
        q, k, v = (f(x).reshape(4, 6, 2, 8).permute(0, 2, 1, 3) for f in (self.q, self.k, self.v))
        if self.kind == "causal":
            a = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        else:
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=self.mask)
        return self.out(a.permute(0, 2, 1, 3).reshape(4, 6, 16))


def _import(kind, path):
    torch.manual_seed(11)
    net = Attn(kind).eval()
    ff = FFModel(FFConfig())
    x = ff.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")
    pm = PyTorchModel(net)
    if path == "export":
        pm.graph = None          # what an untraceable (Hugging Face) model takes
    (out,) = pm.torch_to_ff(ff, [x])
    ff.compile(optimizer=SGDOptimizer(ff, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    copy_weights(ff, pm.weights() if path == "fx" and pm.graph is not None else None)
    return net, ff, pm


def _check_against_torch(net, ff, extra=()):
    g = torch.Generator().manual_seed(12)
    inp, dout = torch.randn(4, 6, 16, generator=g), torch.randn(4, 6, 5, generator=g)
    ex = ff.executor
    out = ex.forward({"x": inp}, training=True)
    want = net(inp)
    torch.testing.assert_close(out.float(), want, rtol=1e-5, atol=1e-5)
    ex.backward(dout)
    want.backward(dout)
    kernels = [n for n in ex.parameter_names() if n.endswith(".kernel")]
    for lin in (net.q, net.k, net.v, net.out):
        # the importers name layers their own way: a layer is found by the weight it was given
        wt = lin.weight.detach().t()
        (kn,) = [n for n in kernels if ex.get_parameter(n).shape == wt.shape and torch.equal(ex.get_parameter(n), wt)]
        torch.testing.assert_close(ex.get_parameter_grad(kn), lin.weight.grad.t(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(ex.get_parameter_grad(kn[:-len("kernel")] + "bias"), lin.bias.grad, rtol=1e-5,
                                   atol=1e-5)


@pytest.mark.parametrize("path", ["export", "fx"])
@pytest.mark.parametrize("kind", ["causal", "bool_mask"])
def test_import_yields_one_sdpa_node(kind, path):
    net, ff, pm = _import(kind, path)
    assert (pm.graph is None) == (path == "export")
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("SDPA") == 1 and "SOFTMAX" not in types and "BATCHMATMUL" not in types, types
    (l,) = [l for l in ff.get_layers() if l.op_type == "SDPA"]
    assert len(ff.cg.layer_data_inputs(l.node)) == (3 if kind == "causal" else 4)
    assert ('"causal":true' in ff.cg.to_json().replace(" ", "")) == (kind == "causal")
    _check_against_torch(net, ff)


@pytest.mark.parametrize("path", ["export", "fx"])
def test_parameter_bias_keeps_the_unfused_lowering(path):
    net, ff, pm = _import("param_bias", path)
    assert pm.graph is None, "fx hands a mask that a parameter feeds to the torch.export path"
    types = [l.op_type for l in ff.get_layers()]
    assert "SDPA" not in types and "SOFTMAX" in types and types.count("BATCHMATMUL") == 2, types
    _check_against_torch(net, ff)


@pytest.mark.parametrize("path", ["export", "fx"])
def test_parameter_bias_gets_a_gradient(path):
    """The learned bias of the unfused lowering receives torch's gradient: it
    is a standalone weight that the mask add reads as a data input, and the
    executor moves that input gradient into the parameter's gradient."""
    net, ff, pm = _import("param_bias", path)
    _check_against_torch(net, ff)
    (wn,) = [n for n in ff.executor.parameter_names() if n.startswith("mask")]
    assert net.mask.grad.abs().sum() > 0
    got = ff.executor.get_parameter_grad(wn)
    print(f"bias gradient norm {float(got.norm()):.4g}, torch {float(net.mask.grad.norm()):.4g}")
    torch.testing.assert_close(got, net.mask.grad, rtol=1e-5, atol=1e-5)


def test_ff_text_ir_round_trip():
    net = Attn("causal").eval()
    lines = PyTorchModel(net).torch_to_string()
    (ln,) = [l for l in lines if "; SDPA; " in l]
    assert ln.endswith("SDPA; 1; 0.0; 0.0; 0")
    ff = FFModel(FFConfig())
    string_to_ff(lines, ff, [ff.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")])
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("SDPA") == 1 and "BATCHMATMUL" not in types
    # a tensor mask is the node's fourth input in the text IR
    ff2 = FFModel(FFConfig())
    q = ff2.create_tensor([2, 2, 6, 8], DataType.DT_FLOAT, name="q")
    mk = ff2.create_tensor([2, 1, 1, 6], DataType.DT_FLOAT, create_grad=False, name="mk")
    (o,) = string_to_ff(["q; ; a,; INPUT", "mk; ; a,; INPUT", "a; q,q,q,mk,; out,; SDPA; 0; 0.1; 0.25; 1",
                         "out; a,; ; OUTPUT"], ff2, [q, mk])
    (l,) = [l for l in ff2.get_layers() if l.op_type == "SDPA"]
    assert len(ff2.cg.layer_data_inputs(l.node)) == 4 and list(o.dims) == [2, 2, 6, 8]
    (op,) = [l["op"] for l in json.loads(ff2.cg.to_json())["layers"] if l["op"]["op_type"] == "SDPA"]
    assert op["attrs"]["scale"] == {"f": 0.25} and op["attrs"]["mask"] is True and not op["attrs"]["causal"]
    assert abs(op["attrs"]["dropout"]["f"] - 0.1) < 1e-12
    with pytest.raises(NotImplementedError, match="no tensor constants"):
        PyTorchModel(Attn("bool_mask").eval()).torch_to_string()
