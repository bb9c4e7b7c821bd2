"""CPU half of the convolution / pooling geometry suite.

* the fp64 helpers of conv_refs.py agree with plain autograd;
* the derived forward / dgrad bounds hold for an fp32 CPU convolution rounded
  to bf16 on every geometry of the GPU suite (the "reference alone" check: the
  GPU tests cannot fail for a reason that is in the test);
* Conv2DOp's and Pool2DOp's torch fallbacks honour asymmetric attributes;
* the torch importers refuse what the CONV2D / POOL2D operators cannot express
  (dilation, string padding, non-zero padding modes, ceil_mode, averages that
  count the padding) and pass both window dimensions.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_refs as R
from flexflow_train_amd.core import DataType, FFConfig, FFModel, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights, string_to_ff

ALL_CASES = R.DENSE_CASES + R.GROUPED_CASES


# ------------------------------------------------------------------ helpers
@pytest.mark.parametrize("case", [R.DENSE_CASES[2], R.GROUPED_CASES[1]], ids=R.case_id)
def test_conv_helpers_agree_with_autograd(case):
    x, w, b, dy, geom = R.conv_inputs(case, 0)
    ref, T = R.conv_fwd_ref(x, w, b, geom)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == tuple(dy.shape)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, b.double(), stride=geom["stride"], padding=geom["padding"], dilation=geom["dilation"],
                 groups=geom["groups"])
    assert torch.equal(ref, y.detach())
    gx, gw = torch.autograd.grad(y, (xr, wr), dy.double())
    dx, dw = R.conv_bwd_ref(x, w, dy, geom)
    assert torch.equal(dx, gx) and torch.equal(dw, gw)
    Tx, Tw = R.conv_bwd_abs(x, w, dy, geom)
    assert (T >= ref.abs() - 1e-12).all() and (Tx >= dx.abs() - 1e-12).all() and (Tw >= dw.abs() - 1e-12).all()


def test_unreached_pixels():
    # computed independently: a pixel is reached when some (p, r) has p*s - pad + r*d == h
    for case in ALL_CASES:
        N, C, H, W, Ko, Rr, S, st, pd, dl = case[:10]
        P = (H + 2 * pd[0] - dl[0] * (Rr - 1) - 1) // st[0] + 1
        Q = (W + 2 * pd[1] - dl[1] * (S - 1) - 1) // st[1] + 1
        rows = {p * st[0] - pd[0] + r * dl[0] for p in range(P) for r in range(Rr)}
        cols = {q * st[1] - pd[1] + s * dl[1] for q in range(Q) for s in range(S)}
        want = torch.tensor([[not (h in rows and w in cols) for w in range(W)] for h in range(H)])
        assert torch.equal(R.unreached(case), want), case
    assert int(R.unreached(R.DENSE_CASES[0]).sum()) == 9      # the last column of a 9 x 12 image
    assert int(R.unreached(R.DENSE_CASES[3]).sum()) == 19     # last row and column of 10 x 10
    assert int(R.unreached(R.DENSE_CASES[4]).sum()) > 0 and int(R.unreached(R.DENSE_CASES[5]).sum()) == 0


def test_assert_elementwise_excludes_nothing():
    ref = torch.arange(12, dtype=torch.float64).view(3, 4)
    tol = torch.full_like(ref, 0.5)
    R.assert_elementwise(ref + 0.25, ref, tol)
    out = ref.clone()
    out[2, 1] += 0.75
    with pytest.raises(AssertionError, match=r"worst at \(2, 1\): got 9\.75, reference 9, bound 0\.5"):
        R.assert_elementwise(out, ref, tol, "probe")
    out = ref.clone()
    out[0, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"\(0, 3\)"):
        R.assert_elementwise(out, ref, tol)
    assert R.worst_ratio(ref + 0.25, ref, tol) == 0.5


def test_bn_helpers_agree_with_autograd():
    torch.manual_seed(0)
    x = (torch.randn(3, 8, 5, 4) * 2 + 0.5).to(torch.bfloat16)
    res = torch.randn(3, 8, 5, 4).to(torch.bfloat16)
    dy = torch.randn(3, 8, 5, 4).to(torch.bfloat16)
    gamma, beta = 1 + 0.1 * torch.randn(8, dtype=torch.float64), 0.1 * torch.randn(8, dtype=torch.float64)
    mean, var = R.bn_stats_ref(x)
    rstd = 1 / (var + 1e-5).sqrt()
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = torch.relu(F.batch_norm(xr, None, None, gr, br, training=True, eps=1e-5) + rr)
    yr.backward(dy.double())
    y, _ = R.bn_apply_ref(x, gamma * rstd, beta - mean * gamma * rstd, res, True)
    torch.testing.assert_close(y, yr.detach(), rtol=1e-12, atol=1e-12)
    b = R.bn_bwd_ref(dy, x, y > 0, mean, rstd, gamma)
    torch.testing.assert_close(b["dx"], xr.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dgamma"], gr.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dbeta"], br.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["g"], rr.grad, rtol=0, atol=0)


def test_pool_helpers():
    torch.manual_seed(0)
    x = torch.randn(2, 8, 13, 10).to(torch.bfloat16)
    k, s, p = (3, 2), (2, 1), (1, 0)
    y, _ = R.pool_ref(x, k, s, p, True)
    dy = torch.randn(y.shape).to(torch.bfloat16)
    y, dx = R.pool_ref(x, k, s, p, True, dy=dy)
    assert y.dtype == torch.float64 and dx.shape == x.shape
    # an fp32 average rounded to bf16 stays within the bounds
    y32 = F.avg_pool2d(x.float(), k, s, p, count_include_pad=False).to(torch.bfloat16)
    R.assert_elementwise(y32, y, R.pool_avg_fwd_bound(x, y, k, s, p), "avg fwd")
    x32 = x.float().requires_grad_(True)
    F.avg_pool2d(x32, k, s, p, count_include_pad=False).backward(dy.float())
    R.assert_elementwise(x32.grad.to(torch.bfloat16), dx, R.pool_bwd_bound(dy, dx, x.shape, k, s, p, True), "avg bwd")


# ------------------------------------------------------- the reference alone
@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_bounds_hold_for_fp32_reference(case):
    """An fp32 CPU convolution rounded to bf16 — what a correct kernel
    computes, up to summation order — is inside the derived forward, dgrad
    and wgrad bounds."""
    x, w, b, dy, geom = R.conv_inputs(case, 0)
    Ko, Cg, Rr, S = w.shape
    ref, T = R.conv_fwd_ref(x, w, b, geom)
    y32 = F.conv2d(x.float(), w.float(), b.float(), **geom)
    for act in ("none", "relu"):
        R.assert_elementwise(R.ACTS[act](y32).to(torch.bfloat16), R.ACTS[act](ref), R.fwd_bound(ref, T, Rr * S * Cg),
                             f"fwd {act}")
    dx, dw = R.conv_bwd_ref(x, w, dy, geom)
    Tx, Tw = R.conv_bwd_abs(x, w, dy, geom)
    x32, w32 = x.float().requires_grad_(True), w.float().requires_grad_(True)
    F.conv2d(x32, w32, None, **geom).backward(dy.float())
    KG = Rr * S * Ko // geom["groups"]
    R.assert_elementwise(x32.grad.to(torch.bfloat16), dx, R.dgrad_bound(dx, Tx, KG), "dgrad")
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    acc = (x32.grad.to(torch.bfloat16).float() + base.float()).to(torch.bfloat16)
    R.assert_elementwise(acc, dx + base.double(), R.dgrad_beta_bound(dx, dx + base.double(), Tx, KG), "dgrad beta")
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    if npix <= 1024:
        R.assert_elementwise(w32.grad, dw, R.wgrad_bound(Tw, npix, 1), "wgrad")
    assert R.relerr(w32.grad, dw) < 1e-5
    # the unreached pixels of the reference are exact zeros
    un = R.unreached(case)
    assert not dx[:, :, un].any()


# ------------------------------------------------------------- operators
def test_conv_op_torch_fallback_asymmetric():
    from flexflow_train_amd.ops import conv as CV
    from flexflow_train_amd.ops.base import OpContext

    torch.manual_seed(1)
    for (kh, kw), (sh, sw), (ph, pw) in (((3, 3), (2, 1), (0, 1)), ((3, 2), (1, 2), (1, 0))):
        x = torch.randn(2, 16, 11, 9, dtype=torch.float64)
        w = torch.randn(24, 16, kh, kw, dtype=torch.float64) * 0.1
        b = torch.randn(24, dtype=torch.float64)
        ctx = OpContext("CONV2D", {"kernel_h": kh, "kernel_w": kw, "stride_h": sh, "stride_w": sw, "padding_h": ph,
                                   "padding_w": pw}, "c", compute_dtype=torch.float64)
        op = CV.Conv2DOp()
        Wp = op.to_physical(ctx.attrs, 0, w).reshape(w.shape)     # logical-shaped piece over the physical data
        (y,), saved = op.forward(ctx, [x], [Wp, b])
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, br, stride=(sh, sw), padding=(ph, pw))
        torch.testing.assert_close(y, yr.detach(), rtol=1e-12, atol=1e-12)
        dy = torch.randn_like(yr)
        yr.backward(dy)
        dW, db = torch.zeros_like(Wp), torch.zeros_like(b)
        (dx,) = op.backward(ctx, saved, [dy], [dW, db], [True])
        torch.testing.assert_close(dx, xr.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(op.to_logical(ctx.attrs, 0, dW), wr.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(db, br.grad, rtol=1e-5, atol=1e-5)    # the fallback sums the bias gradient in fp32


@pytest.mark.parametrize("avg", [False, True])
def test_pool_op_torch_fallback_asymmetric(avg):
    from flexflow_train_amd.ops import conv as CV
    from flexflow_train_amd.ops.base import OpContext

    torch.manual_seed(2)
    x = torch.randn(2, 24, 13, 10, dtype=torch.float64)
    k, s, p = (3, 2), (2, 1), (1, 0)
    ctx = OpContext("POOL2D", {"kernel_h": k[0], "kernel_w": k[1], "stride_h": s[0], "stride_w": s[1],
                               "padding_h": p[0], "padding_w": p[1], "pool_type": "avg" if avg else "max"}, "p",
                    compute_dtype=torch.float64)
    op = CV.Pool2DOp()
    (y,), saved = op.forward(ctx, [x], [])
    dy = torch.randn_like(y)
    yr, dxr = R.pool_ref(x, k, s, p, avg, dy=dy)
    torch.testing.assert_close(y, yr, rtol=0, atol=0)
    (dx,) = op.backward(ctx, saved, [dy], [], [True])
    torch.testing.assert_close(dx, dxr, rtol=0, atol=0)


# ------------------------------------------------------------- importers
class _One(nn.Module):
    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x):
        return self.layer(x)


REFUSED = [
    ("dilation", lambda: nn.Conv2d(8, 8, 3, padding=2, dilation=2)),
    ("padding", lambda: nn.Conv2d(8, 8, 3, padding="same")),
    ("padding_mode", lambda: nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect")),
    ("ceil_mode", lambda: nn.MaxPool2d(3, 2, ceil_mode=True)),
    ("dilation", lambda: nn.MaxPool2d(3, 1, dilation=2)),
    ("count_include_pad", lambda: nn.AvgPool2d(3, 1, 1)),
]


def _import(net, shape=(2, 8, 9, 9)):
    ff = FFModel(FFConfig())
    x = ff.create_tensor(list(shape), DataType.DT_FLOAT, name="x")
    pm = PyTorchModel(net)
    pm.torch_to_ff(ff, [x])
    return ff, pm


@pytest.mark.parametrize("arg,make", REFUSED, ids=[f"{i}-{a}" for i, (a, _) in enumerate(REFUSED)])
def test_importers_refuse_what_the_operators_cannot_express(arg, make):
    torch.manual_seed(0)
    net = _One(make()).eval()
    # fx importer, in memory and to the .ff text
    with pytest.raises((ValueError, NotImplementedError), match=arg):
        _import(net)
    with pytest.raises((ValueError, NotImplementedError), match=arg):
        PyTorchModel(net).torch_to_string()
    # flexflow.torch.compile (module form)
    from flexflow_train_amd.frontends import torch_compile as TC
    with pytest.raises((ValueError, NotImplementedError), match=arg):
        TC.compile(net, [torch.randn(2, 8, 9, 9)])


@pytest.mark.parametrize("arg,make", REFUSED, ids=[f"{i}-{a}" for i, (a, _) in enumerate(REFUSED)])
def test_onnx_path_refuses_the_same(arg, make):
    """torch -> ONNX -> FFModel: the exporter writes dilations and
    count_include_pad (or refuses the layer itself), the importer refuses
    them: no dilated model arrives as an undilated convolution."""
    from flexflow_train_amd.frontends.onnx import ONNXModel, export_torch

    x = torch.randn(2, 8, 9, 9)
    with pytest.raises((ValueError, NotImplementedError), match=arg):
        data = export_torch(_One(make()).eval(), x)
        ff = FFModel(FFConfig())
        ONNXModel(data).apply(ff, {"input.1": ff.create_tensor([2, 8, 9, 9], DataType.DT_FLOAT)})


def test_onnx_importer_refuses_implicit_and_uneven_pads():
    from flexflow_train_amd.frontends.onnx import ONNXModel, export_torch

    def graph(**attrs):
        om = ONNXModel(export_torch(_One(nn.Conv2d(8, 8, 3, padding=1)).eval(), torch.randn(2, 8, 9, 9)))
        conv = [n for n in om.graph.nodes if n.op_type == "Conv"][0]
        conv.attrs.update(attrs)
        ff = FFModel(FFConfig())
        om.apply(ff, {"input.1": ff.create_tensor([2, 8, 9, 9], DataType.DT_FLOAT)})

    graph()
    with pytest.raises(NotImplementedError, match="auto_pad"):
        graph(auto_pad="SAME_UPPER")
    with pytest.raises(NotImplementedError, match="pads"):
        graph(pads=[1, 1, 2, 1])


@pytest.mark.parametrize("make,op", [(lambda: nn.Conv2d(8, 8, 3, padding=2, dilation=2), "conv"),
                                     (lambda: nn.MaxPool2d(3, 2, ceil_mode=True), "max_pool2d"),
                                     (lambda: nn.AvgPool2d(3, 1, 1), "avg_pool2d")], ids=["conv", "max", "avg"])
def test_export_importer_maps_no_convolution_or_pooling(make, op):
    """The torch.export importer lowers no aten convolution or pooling at
    all: every such model is refused by name, none imports as another
    operator."""
    from flexflow_train_amd.frontends.torch_export import ATenImporter

    with pytest.raises(NotImplementedError, match=op):
        imp = ATenImporter(_One(make()).eval(), [torch.randn(2, 8, 9, 9)])
        ff = FFModel(FFConfig())
        imp.to_ff(ff, [ff.create_tensor([2, 8, 9, 9], DataType.DT_FLOAT, name="x")])


def _functional_graph(fn, conv=None):
    """The flat graph of the torch.compile backend: parameters as
    placeholders, layers as functional calls."""
    import torch.fx as fx

    g = fx.Graph()
    x = g.placeholder("x")
    ex = [torch.randn(2, 8, 9, 9)]
    if conv is not None:
        w, b = g.placeholder("w"), g.placeholder("b")
        ex += [conv.weight, conv.bias]
        out = fn(x, w, b)(g)
    else:
        out = fn(x)(g)
    g.output(out)
    return fx.GraphModule(nn.Module(), g), ex


FUNCTIONAL_REFUSED = [
    ("dilation", True, lambda x, w, b: lambda g: g.call_function(F.conv2d, (x, w, b, 1, 2, 2))),
    ("dilation", True, lambda x, w, b: lambda g: g.call_function(F.conv2d, (x, w, b), {"padding": 2, "dilation": 2})),
    ("padding", True, lambda x, w, b: lambda g: g.call_function(F.conv2d, (x, w, b, 1, "same"))),
    ("ceil_mode", False, lambda x: lambda g: g.call_function(F.max_pool2d, (x, 3, 2, 0, 1, True))),
    ("ceil_mode", False, lambda x: lambda g: g.call_function(F.max_pool2d, (x, 3, 2), {"ceil_mode": True})),
    ("dilation", False, lambda x: lambda g: g.call_function(F.max_pool2d, (x, 3, 1, 0, 2))),
    ("count_include_pad", False, lambda x: lambda g: g.call_function(F.avg_pool2d, (x, 3, 1, 1))),
    ("ceil_mode", False, lambda x: lambda g: g.call_function(F.avg_pool2d, (x, 3, 2, 0, True))),
]


@pytest.mark.parametrize("arg,is_conv,fn", FUNCTIONAL_REFUSED,
                         ids=[f"{i}-{a}" for i, (a, _, _) in enumerate(FUNCTIONAL_REFUSED)])
def test_compile_backend_carries_every_argument(arg, is_conv, fn):
    """torch.compile's backend rebinds functional calls to modules: stride,
    padding, dilation, ceil_mode and count_include_pad travel with them,
    positional or by keyword, so the importer refuses the graph (the backend
    then runs it eagerly) instead of compiling another operator."""
    from flexflow_train_amd.frontends import torch_compile as TC

    conv = nn.Conv2d(8, 8, 3) if is_conv else None
    gm, ex = _functional_graph(fn, conv)
    mod, data_pos = TC._rebind_parameter_ops(gm, ex)
    assert data_pos == [0]
    with pytest.raises((ValueError, NotImplementedError), match=arg):
        TC.CompiledModel(mod, [ex[0]])
    with pytest.warns(UserWarning, match=arg):
        run = TC.flexflow_backend(gm, ex)
    assert not hasattr(run, "compiled_model")


def _run(ff, pm, inp):
    cfg_opt = SGDOptimizer(ff, lr=0.0)
    ff.compile(optimizer=cfg_opt)
    copy_weights(ff, pm.weights())
    return ff.executor.forward({"x": inp}, training=False).float()


@pytest.mark.parametrize("mode", ["memory", "text"])
@pytest.mark.parametrize("make", [lambda: nn.MaxPool2d((3, 2), (2, 1), (1, 0)),
                                  lambda: nn.AvgPool2d((3, 2), (2, 1), (1, 0), count_include_pad=False),
                                  lambda: nn.AvgPool2d(2, 2),        # count_include_pad without padding: no difference
                                  lambda: nn.Conv2d(8, 16, (3, 2), (2, 1), (0, 1))],
                         ids=["max", "avg", "avg-nopad", "conv"])
def test_importers_pass_both_dimensions(make, mode):
    torch.manual_seed(3)
    net = _One(make()).eval()
    inp = torch.randn(2, 8, 13, 10)
    if mode == "memory":
        ff, pm = _import(net, inp.shape)
    else:
        pm = PyTorchModel(net)
        ff = FFModel(FFConfig())
        x = ff.create_tensor(list(inp.shape), DataType.DT_FLOAT, name="x")
        string_to_ff(pm.torch_to_string(), ff, [x])
    want = net(inp)
    got = _run(ff, pm, inp)
    assert got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


def test_compile_matches_torch_on_asymmetric_pooling():
    from flexflow_train_amd.frontends import torch_compile as TC

    torch.manual_seed(4)
    net = nn.Sequential(nn.Conv2d(8, 16, (3, 2), (2, 1), (0, 1)), nn.MaxPool2d((3, 2), (2, 1), (1, 0)),
                        nn.AvgPool2d((2, 3), (1, 2), (1, 0), count_include_pad=False)).eval()
    inp = torch.randn(2, 8, 13, 10)
    cfg = FFConfig()
    cfg.cpu_only = True
    cm = TC.compile(net, [inp], cfg)
    with torch.no_grad():
        torch.testing.assert_close(cm(inp), net(inp), rtol=1e-5, atol=1e-6)


def test_square_pool_line_keeps_the_reference_format():
    def fields(layer):
        line = [ln for ln in PyTorchModel(_One(layer)).torch_to_string() if "POOL2D" in ln][0]
        return [i.strip() for i in line.split(";")][4:]

    sq = fields(nn.MaxPool2d(3, 2, 1))
    assert len(sq) == 5 and sq[:3] == ["3", "2", "1"]            # k, s, p, pool type, activation
    rect = fields(nn.MaxPool2d((3, 2), (2, 1), (1, 0)))
    assert len(rect) == 8 and rect[:3] == ["3", "2", "1"] and rect[5:] == ["2", "1", "0"]
