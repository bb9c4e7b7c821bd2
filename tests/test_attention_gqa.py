"""Grouped-query attention (k / v with Hkv < H heads) in the SDPA operator on
the CPU: the torch fallback against F.scaled_dot_product_attention(enable_gqa=
True), shape inference, head sharding, serialisation, the memory plan, the
strategy search and the torch.export / torch.fx / torch.compile importers.
"""
import json
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import flexflow.torch as fft
from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights, string_to_ff
from flexflow_train_amd.ops import base as opbase
from flexflow_train_amd.search import native

F32 = C.DataType.FLOAT
P = C.ParallelTensorShape
TS = C.TensorShape
B, H, SQ, SK, D = 2, 6, 10, 12, 8


# ------------------------------------------------------------------ operator
def _op(attrs, inputs, do):
    impl = opbase.get_impl("SDPA")
    ctx = opbase.OpContext(op_type="SDPA", attrs=attrs, name="sdpa", training=True)
    (o,), saved = impl.forward(ctx, inputs, [])
    return o, impl.backward(ctx, saved, [do], [], [True] * len(inputs))


@pytest.mark.parametrize("case", ["none", "float", "causal", "mqa"])
def test_torch_fallback_matches_torch_enable_gqa(case):
    g = torch.Generator().manual_seed(3)
    sk = SQ if case == "causal" else SK
    hkv = 1 if case == "mqa" else 2
    q = torch.randn(B, H, SQ, D, generator=g)
    k, v = torch.randn(B, hkv, sk, D, generator=g), torch.randn(B, hkv, sk, D, generator=g)
    do = torch.randn(B, H, SQ, D, generator=g)
    mask, kw, attrs = None, {}, {}
    if case == "float":
        mask = torch.randn(1, H, SQ, sk, generator=g)
        attrs["mask"] = True
    elif case == "causal":
        kw, attrs = dict(is_causal=True), dict(causal=True)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qr, kr, vr, attn_mask=mask, enable_gqa=True, **kw)
    ref.backward(do)
    o, grads = _op(attrs, [q, k, v] + ([mask] if mask is not None else []), do)
    assert o.shape == (B, H, SQ, D) and grads[1].shape == k.shape and grads[2].shape == v.shape
    for got, want in zip((o, *grads[:3]), (ref, qr.grad, kr.grad, vr.grad)):
        torch.testing.assert_close(got, want.detach(), rtol=1e-5, atol=1e-5)


def test_operator_refuses_bad_head_counts():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, SQ, D, generator=g)
    k4, k2, k3 = (torch.randn(B, h, SK, D, generator=g) for h in (4, 2, 3))
    with pytest.raises(ValueError, match="not a multiple of 4 K / V heads"):
        _op({}, [q, k4, k4], q)
    with pytest.raises(ValueError, match="k has 2 heads and v has 3"):
        _op({}, [q, k2, k3], q)


# ----------------------------------------------------------- shape inference
def _shapes(hkv, hv=None, sk=SK):
    return [TS([B, H, SQ, D], F32), TS([B, hkv, sk, D], F32), TS([B, hkv if hv is None else hv, sk, D], F32)]


def test_serial_shape_inference():
    op3, op4 = C.OpAttrs("SDPA"), C.OpAttrs("SDPA", mask=True)
    for hkv in (1, 2, 3, 6):
        assert C.infer_output_shapes(op3, _shapes(hkv))[0].dims == [B, H, SQ, D]
        assert C.infer_output_shapes(C.OpAttrs("SDPA", causal=True), _shapes(hkv, sk=SQ))[0].dims == [B, H, SQ, D]
        # the mask's head dim is 1 or H, never Hkv
        for mh in (1, H):
            assert C.infer_output_shapes(op4, _shapes(hkv) + [TS([B, mh, SQ, SK], F32)])[0].dims == [B, H, SQ, D]
        if hkv not in (1, H):
            with pytest.raises(ValueError, match="1 or the full extent"):
                C.infer_output_shapes(op4, _shapes(hkv) + [TS([B, hkv, SQ, SK], F32)])
    for ins in (_shapes(4), _shapes(5), _shapes(12), _shapes(2, 3), _shapes(2, 6), _shapes(6, 2)):
        with pytest.raises(ValueError, match="head count mismatch"):
            C.infer_output_shapes(op3, ins)


def test_parallel_shape_inference_and_head_sharding():
    op3 = C.OpAttrs("SDPA")

    def qkv(b, h, hkv, hk_deg=None):
        hk_deg = h if hk_deg is None else hk_deg
        return [P([4, 12, SQ, D], [b, h, 1, 1], 1, 1, F32), P([4, hkv, SK, D], [b, hk_deg, 1, 1], 1, 1, F32),
                P([4, hkv, SK, D], [b, hk_deg, 1, 1], 1, 1, F32)]

    for hkv in (4, 6, 12):
        for h in (1, 2, 3, 4, 6):
            ok = hkv % h == 0      # the degree must divide Hkv: whole groups per shard
            assert C.is_valid_parallelization(op3, qkv(2, h, hkv)) == ok, (hkv, h)
            if ok:
                (o,) = C.infer_parallel_output_shapes(op3, qkv(2, h, hkv))
                assert o.shard_degrees() == [2, h, 1, 1]
    # k / v follow q's degree
    assert not C.is_valid_parallelization(op3, qkv(1, 2, 4, hk_deg=1))
    assert not C.is_valid_parallelization(op3, qkv(1, 2, 4, hk_deg=4))


def _model(hkv, mask_dims=None, causal=False, dropout=0.0, heads=4):
    """[4, 6, 32] -> q of `heads` heads, k / v of hkv heads of 8 -> SDPA -> [4, 6, 5]."""
    m = FFModel(FFConfig())
    x = m.create_tensor([4, 6, 32], DataType.DT_FLOAT, name="x")
    mask = m.create_tensor(mask_dims, DataType.DT_FLOAT, create_grad=False, name="mask") if mask_dims else None
    q, k, v = (m.transpose(m.reshape(m.dense(x, nh * 8, name=n), [4, 6, nh, 8]), [0, 2, 1, 3])
               for n, nh in (("q", heads), ("k", hkv), ("v", hkv)))
    a = m.scaled_dot_product_attention(q, k, v, mask=mask, causal=causal, dropout=dropout, name="attn")
    a = m.reshape(m.transpose(a, [0, 2, 1, 3]), [4, 6, heads * 8])
    m.softmax(m.dense(a, 5, name="head"), name="sm")
    return m


def test_heads_candidates_and_strategy_search():
    m = _model(2, [4, 1, 1, 6])
    (l,) = [l for l in m.get_layers() if l.op_type == "SDPA"]
    cands = [json.loads(c) for c in C.candidate_configs(m.cg, l.node, 4)]
    heads = sorted(c["model"] for c in cands if c["kind"] == "heads")
    assert heads and set(heads) == {2}, "a head degree must divide Hkv = 2 (4 divides H only)"
    # Hkv == H offers 4 as well
    m4 = _model(4)
    (l4,) = [l for l in m4.get_layers() if l.op_type == "SDPA"]
    assert {c["model"] for c in map(json.loads, C.candidate_configs(m4.cg, l4.node, 4)) if c["kind"] == "heads"} \
        == {2, 4}
    cm = native.cost_model()
    cfg = json.dumps({"world": 4, "budget": 100, "time_limit": 20, "seed": 1})
    for pcg, rep in (C.graph_optimize(m.cg, cm, cfg)[:2], C.mcmc_search(m.cg, cm, cfg)[:2],
                     C.unity_search(C.data_parallel_pcg(m.cg, 4), cm, cfg)[:2]):
        rep = json.loads(rep)
        assert math.isfinite(rep["cost"]) and 0 < rep["cost"] <= rep["data_parallel_cost"] * 1.0000001
        pcg.reinfer_shapes()     # the chosen strategy validates
    # data parallel: k / v and the mask's full batch dim get q's degree
    pcg, mapping, _ = C.lower_strategy(m.cg, C.data_parallel_strategy(m.cg, 4), 4)
    degrees = [pcg.shape(v).shard_degrees() for v in pcg.layer_data_inputs(mapping[l.node])]
    assert degrees == [[4, 1, 1, 1]] * 4


# ------------------------------------------------------ JSON, .ff, memory plan
def test_json_round_trip():
    for hkv, mask_dims, causal in ((1, None, True), (2, None, False), (2, [4, 4, 6, 6], False)):
        m = _model(hkv, mask_dims, causal)
        (l,) = [l for l in m.get_layers() if l.op_type == "SDPA"]
        ins = m.cg.layer_data_inputs(l.node)
        assert m.cg.shape(ins[1]).dims == [4, hkv, 6, 8] and m.cg.shape(C.ValueRef(l.node, 0)).dims == [4, 4, 6, 8]
        text = m.cg.to_json()
        again = C.ComputationGraph.from_json(text)
        assert again.to_json() == text and "kv_heads" not in text, "Hkv is read from the shapes"
    with pytest.raises(ValueError, match="head count mismatch"):
        _model(3)


def test_ff_text_ir_round_trip():
    net = GQAttn("causal").eval()
    lines = PyTorchModel(net).torch_to_string()
    (ln,) = [l for l in lines if "; SDPA; " in l]
    assert ln.endswith("SDPA; 1; 0.0; 0.0; 0"), "no new field in the text IR"
    ff = FFModel(FFConfig())
    string_to_ff(lines, ff, [ff.create_tensor([4, 6, 32], DataType.DT_FLOAT, name="x")])
    (l,) = [l for l in ff.get_layers() if l.op_type == "SDPA"]
    assert [ff.cg.shape(v).dims[1] for v in ff.cg.layer_data_inputs(l.node)] == [4, 2, 2]
    assert "BATCHMATMUL" not in [l.op_type for l in ff.get_layers()]


def test_memory_plan_counts_the_expanded_copies():
    """executor_fusions: the SDPA node keeps its output and the LSE; with
    Hkv < H and a mask or dropout also the two [B, H, Sk, D] expansions of K
    and V, and nothing of the kind otherwise."""
    def sdpa_act(m):
        pcg = C.data_parallel_pcg(m.cg, 1)
        (p,) = native.plan_memory(pcg, 1, with_blocks=True, act_elem_bytes=2.0, executor_fusions=True)
        own = sum(b["bytes"] for b in p["blocks"] if b["kind"] == 0 and pcg.layer_op(b["node"]).op_type == "SDPA")
        return own, sum(b["bytes"] for b in p["blocks"] if b["kind"] == 0)

    expanded = 2 * (4 * 4 * 6 * 8) * 2.0      # two [B, H, Sk, D] tensors in bf16
    base, base_all = sdpa_act(_model(4))
    gqa, gqa_all = sdpa_act(_model(2))
    assert gqa == base, "without a mask or dropout: nothing beyond the LSE"
    assert gqa_all < base_all, "the K / V projections shrink"
    drop, drop_all = sdpa_act(_model(2, dropout=0.1))
    assert abs(drop - (gqa + expanded)) < 1e-6 and abs(drop_all - (gqa_all + expanded)) < 1e-6
    masked, _ = sdpa_act(_model(2, [4, 1, 1, 6]))
    assert abs(masked - (gqa + expanded)) < 1e-6
    # Hkv == H: a mask or dropout adds nothing
    assert sdpa_act(_model(4, dropout=0.1))[0] == base and sdpa_act(_model(4, [4, 1, 1, 6]))[0] == base


# ----------------------------------------------------------------- frontends
class GQAttn(nn.Module):
    """[4, 6, 32] -> 4 query heads over 2 K / V heads of 8 -> F.scaled_dot_product_attention(enable_gqa=True)."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.q, self.k, self.v, self.out = nn.Linear(32, 32), nn.Linear(32, 16), nn.Linear(32, 16), nn.Linear(32, 5)
        g = torch.Generator().manual_seed(7)
        if kind == "bool_mask":
            keep = torch.rand(4, 1, 6, 6, generator=g) < 0.6
            keep[..., 0] = True
            self.register_buffer("mask", keep)
        elif kind == "param_bias":
            self.mask = nn.Parameter(torch.randn(1, 4, 6, 6, generator=g))

    def forward(self, x):
        q = self.q(x).reshape(4, 6, 4, 8).permute(0, 2, 1, 3)
        k, v = (f(x).reshape(4, 6, 2, 8).permute(0, 2, 1, 3) for f in (self.k, self.v))
        if self.kind == "causal":
            a = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
        else:
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=self.mask, enable_gqa=True)
        return self.out(a.permute(0, 2, 1, 3).reshape(4, 6, 32))


def _import(kind, path):
    torch.manual_seed(11)
    net = GQAttn(kind).eval()
    ff = FFModel(FFConfig())
    x = ff.create_tensor([4, 6, 32], DataType.DT_FLOAT, name="x")
    pm = PyTorchModel(net)
    if path == "export":
        pm.graph = None          # what an untraceable (Hugging Face) model takes
    (out,) = pm.torch_to_ff(ff, [x])
    ff.compile(optimizer=SGDOptimizer(ff, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    copy_weights(ff, pm.weights() if path == "fx" and pm.graph is not None else None)
    return net, ff, pm


@pytest.mark.parametrize("path", ["export", "fx"])
@pytest.mark.parametrize("kind", ["causal", "bool_mask"])
def test_import_yields_one_sdpa_node_and_torchs_gradients(kind, path):
    net, ff, pm = _import(kind, path)
    assert (pm.graph is None) == (path == "export")
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("SDPA") == 1 and "SOFTMAX" not in types and "BATCHMATMUL" not in types, types
    (l,) = [l for l in ff.get_layers() if l.op_type == "SDPA"]
    assert [ff.cg.shape(v).dims[1] for v in ff.cg.layer_data_inputs(l.node)][:3] == [4, 2, 2]
    g = torch.Generator().manual_seed(12)
    inp, dout = torch.randn(4, 6, 32, generator=g), torch.randn(4, 6, 5, generator=g)
    ex = ff.executor
    out = ex.forward({"x": inp}, training=True)
    want = net(inp)
    torch.testing.assert_close(out.float(), want, rtol=1e-5, atol=1e-5)
    ex.backward(dout)
    want.backward(dout)
    kernels = [n for n in ex.parameter_names() if n.endswith(".kernel")]
    for lin in (net.q, net.k, net.v, net.out):
        wt = lin.weight.detach().t()
        (kn,) = [n for n in kernels if ex.get_parameter(n).shape == wt.shape and torch.equal(ex.get_parameter(n), wt)]
        torch.testing.assert_close(ex.get_parameter_grad(kn), lin.weight.grad.t(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(ex.get_parameter_grad(kn[:-len("kernel")] + "bias"), lin.bias.grad, rtol=1e-5,
                                   atol=1e-5)


@pytest.mark.parametrize("path", ["export", "fx"])
def test_learned_bias_with_gqa_is_refused_by_name(path):
    with pytest.raises(NotImplementedError, match="enable_gqa with a learned attention bias"):
        _import("param_bias", path)


def test_torch_compile_trains_to_torchs_weights():
    """torch.compile(backend="flexflow") gets the node through the fx path: one
    SDPA node, and an ordinary PyTorch loop reaches eager PyTorch's weights."""
    import warnings

    from flexflow_train_amd.frontends import torch_compile as TC

    torch.manual_seed(0)
    net, ref = GQAttn("causal"), GQAttn("causal")
    ref.load_state_dict(net.state_dict())
    x = torch.randn(4, 6, 32)
    y = torch.randint(0, 5, (4, 6))
    torch._dynamo.reset()
    before = len(TC.COMPILED)
    f = torch.compile(net, backend=fft.backend(cpu_only=True))
    opt, opt_r = torch.optim.SGD(net.parameters(), lr=0.1), torch.optim.SGD(ref.parameters(), lr=0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # no eager fallback
        for _ in range(3):
            lf = F.cross_entropy(f(x).reshape(-1, 5), y.reshape(-1))
            lr_ = F.cross_entropy(ref(x).reshape(-1, 5), y.reshape(-1))
            lf.backward()
            lr_.backward()
            opt.step()
            opt_r.step()
            opt.zero_grad()
            opt_r.zero_grad()
    assert len(TC.COMPILED) > before, "the flexflow backend compiled nothing"
    ff = TC.COMPILED[-1]
    for p, r in zip(net.parameters(), ref.parameters()):
        torch.testing.assert_close(p, r, rtol=1e-4, atol=1e-5)
    types = _layer_types(ff)
    assert types.count("SDPA") == 1 and "BATCHMATMUL" not in types, types


def _layer_types(compiled):
    """Layer types of a module that the flexflow backend compiled."""
    for attr in ("ff", "ffmodel", "model"):
        m = getattr(compiled, attr, None)
        if m is not None and hasattr(m, "get_layers"):
            return [l.op_type for l in m.get_layers()]
    raise AssertionError(f"no FFModel on {type(compiled).__name__}: {dir(compiled)}")
