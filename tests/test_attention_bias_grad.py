"""A learned attention bias gets its gradient from SDPA's torch fallback (CPU,
fp32, against torch autograd at the tolerance of test_attention_sdpa.py):
through FFModel.create_weight and through the importers' ``fuse_attention_bias``."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights

B, H, SQ, SK, D = 2, 2, 6, 8, 8
TOL = dict(rtol=1e-5, atol=1e-5)


def _compiled(build):
    cfg = FFConfig()
    cfg.cpu_only = True     # the fp32 torch fallback, also where a GPU is visible
    m = FFModel(cfg)
    build(m)
    m.compile(optimizer=SGDOptimizer(m, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    return m


@pytest.mark.parametrize("form", [(1, H, SQ, SK), (1, H, 1, SK), (B, 1, SQ, 1)])
def test_fallback_gives_the_mask_weight_torchs_gradient(form):
    def build(m):
        q, k, v = (m.create_tensor([B, H, s, D], DataType.DT_FLOAT, name=n) for n, s in zip("qkv", (SQ, SK, SK)))
        m.scaled_dot_product_attention(q, k, v, mask=m.create_weight(list(form), name="bias"), name="attn")

    ex = _compiled(build).executor
    g = torch.Generator().manual_seed(sum(form))
    qv, kv, vv, do = (torch.randn(B, H, s, D, generator=g) for s in (SQ, SK, SK, SQ))
    bias = torch.randn(form, generator=g)
    if form[3] == SK:
        bias[..., 2:4] = float("-inf")      # two key columns masked for every query
    if form[2] == SQ:
        bias[0, -1, 3] = float("-inf")      # every key of one query row
    ex.set_parameter("bias.w", bias)
    ex.forward({"q": qv, "k": kv, "v": vv}, training=True)
    ex.backward(do)
    # torch gives NaN for the dead row: the reference fills it, as the operator's definition does
    bt = bias.clone().requires_grad_(True)
    s = qv @ kv.transpose(-1, -2) / D ** 0.5 + bt
    rowdead = torch.isneginf(s).all(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(rowdead, 0.0), -1).masked_fill(rowdead, 0.0)
    (p @ vv).backward(do)
    got = ex.get_parameter_grad("bias.w")
    torch.testing.assert_close(got, bt.grad, **TOL)
    assert bt.grad.abs().sum() > 0 and (got[torch.isneginf(bias)] == 0).all(), "a pair under -inf and a fully masked row have gradient 0"


class Attn(nn.Module):    # the ``param_bias`` module of test_attention_sdpa.py
    def __init__(self):
        super().__init__()
        self.q, self.k, self.v, self.out = nn.Linear(16, 16), nn.Linear(16, 16), nn.Linear(16, 16), nn.Linear(16, 5)
        self.mask = nn.Parameter(torch.randn(1, 2, 6, 6, generator=torch.Generator().manual_seed(7)))

    def forward(self, x):
        q, k, v = (f(x).reshape(4, 6, 2, 8).permute(0, 2, 1, 3) for f in (self.q, self.k, self.v))
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=self.mask)
        return self.out(a.permute(0, 2, 1, 3).reshape(4, 6, 16))


def test_importer_opt_in_yields_one_sdpa_node_with_a_bias_gradient():
    torch.manual_seed(11)
    net = Attn().eval()
    pm = PyTorchModel(net, fuse_attention_bias=True)
    assert pm.graph is None, "a mask that a parameter feeds goes through torch.export"
    ff = _compiled(lambda m: pm.torch_to_ff(m, [m.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")]))
    copy_weights(ff)
    types = [l.op_type for l in ff.get_layers()]
    assert types.count("SDPA") == 1 and "BATCHMATMUL" not in types and "SOFTMAX" not in types, types
    g = torch.Generator().manual_seed(12)
    inp, dout = torch.randn(4, 6, 16, generator=g), torch.randn(4, 6, 5, generator=g)
    ex = ff.executor
    want = net(inp)
    torch.testing.assert_close(ex.forward({"x": inp}, training=True).float(), want, **TOL)
    ex.backward(dout)
    want.backward(dout)
    (wn,) = [n for n in ex.parameter_names() if n.startswith("mask")]
    torch.testing.assert_close(ex.get_parameter_grad(wn), net.mask.grad, **TOL)
