"""Gradient of the flash kernels' score bias (attn_bwd_dbias_kernel through
``K.attention_bwd(..., bias_grad=)``) and the SDPA operator on top.

B = 3: an odd step count where the batch is summed (both stages of the double
buffer, the last-step path); Sq = 72 and Sk = 132: a full and a partial tile
each.  Reference: fp64 on the same bf16 inputs.  Bound: relative Frobenius
5e-3 (``_BF`` of test_attention_bias_gpu.py); profiles/attn_bias_grad.txt."""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, SQ, SK = 3, 2, 72, 132
_BF = 5e-3
SEED = 4321
# (bias batch, bias heads), (output batch, output heads); the last: a [B, H] bias summed to [1, H]
FORMS = [((1, H), (1, H)), ((B, H), (B, H)), ((1, 1), (1, 1)), ((B, 1), (B, 1)), ((B, H), (1, H))]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def _inputs(D):
    g = torch.Generator().manual_seed(D)
    return tuple(torch.randn(B, s, H, D, generator=g).to(DEV, torch.bfloat16) for s in (SQ, SK, SK, SQ))  # q k v do


@functools.lru_cache(maxsize=None)
def _bias(bb, hb):
    # random, four key columns at -inf for every query and one query row wholly at -inf
    bias = 2 * torch.randn(bb, hb, SQ, SK, generator=torch.Generator().manual_seed(17 * bb + hb))
    bias[..., 60:64] = float("-inf")
    bias[-1, -1, 5] = float("-inf")
    return bias.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref64(D, bform, p):
    # dS = P (keep rs dP - delta), [B, H, Sq, Sk] in fp64; a row with every key masked has P = 0
    q, k, v, do = (t.double().transpose(1, 2) for t in _inputs(D))
    s = q @ k.transpose(-1, -2) / math.sqrt(D) + _bias(*bform).double()
    dead = torch.isneginf(s).all(-1, keepdim=True)
    pr = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    keep = torch.ones_like(pr)
    if p:
        m, rs = attention_dropout_mask(B, H, SQ, SK, p, SEED, DEV)
        keep = m.double() * rs
    delta = (do * ((pr * keep) @ v)).sum(-1, keepdim=True)
    return pr * (keep * (do @ v.transpose(-1, -2)) - delta)


def _run(D, bias, p, bias_grad):
    q, k, v, do = _inputs(D)
    kw = dict(bias=bias, dropout_p=p, seed=SEED) if p else dict(bias=bias)
    o, lse = K.attention_fwd(q, k, v, **kw)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    assert K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, bias_grad=bias_grad, **kw) == 0
    return dq, dk, dv


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("bform,oform", FORMS)
@pytest.mark.parametrize("D", [64, 128])
def test_gradient_against_fp64(D, bform, oform, p):
    bias = _bias(*bform)
    want, masked = _ref64(D, bform, p), torch.isneginf(bias).expand(B, H, SQ, SK)
    for ax in (0, 1):
        if oform[ax] == 1:      # an entry is masked where every source that sums into it is
            want, masked = want.sum(ax, keepdim=True), masked.all(ax, keepdim=True)
    got = torch.full((*oform, SQ, SK), float("nan"), device=DEV)
    n0 = K.STATS["attention_bias_grad"]
    _run(D, bias, p, got)
    assert K.STATS["attention_bias_grad"] == n0 + 1
    err = _rel(got, want)
    print(f"attn_bias_grad D={D} bias={bform} out={oform} p={p}: {err:.3e}")
    assert torch.isfinite(got).all() and err <= _BF, err
    assert masked[..., 60:64].all() and (got[masked] == 0).all(), "under -inf and in the dead row: exactly 0"


def test_other_gradients_unchanged_repeatable_and_guarded():
    D, bias = 64, _bias(1, H)
    base = _run(D, bias, 0.0, None)
    buf = torch.full((1, H, SQ, SK + 4), float("nan"), device=DEV)
    view = buf[..., :SK]                      # row stride Sk + 4
    for a, b in zip(base, _run(D, bias, 0.0, view)):
        assert torch.equal(a, b), "dq / dk / dv do not depend on bias_grad"
    assert torch.isnan(buf[..., SK:]).all() and torch.isfinite(view).all()
    first = view.clone()
    _run(D, bias, 0.0, view)
    assert torch.equal(view, first), "two calls give equal bits"


@pytest.mark.parametrize("case,match", [("no_bias", "needs a bias"), ("bf16", "fp32"), ("shape", "has shape"),
                                        ("key_stride", "contiguous"), ("gqa", "grouped-query")])
def test_refusals(case, match):
    q, k, v, do = _inputs(64)
    bias = None if case == "no_bias" else _bias(1, H)
    grad = {"bf16": torch.empty(1, H, SQ, SK, device=DEV, dtype=torch.bfloat16),
            "shape": torch.empty(1, H, SQ + 1, SK, device=DEV),
            "key_stride": torch.empty(1, H, SQ, 2 * SK, device=DEV)[..., ::2]}.get(
                case, torch.empty(1, H, SQ, SK, device=DEV))
    if case == "gqa":
        k, v = k[:, :, :1], v[:, :, :1]
    n0 = (K.STATS["attention_bwd"], K.STATS["attention_bias_grad"])
    with pytest.raises(ValueError, match=match):
        K.attention_bwd(q, k, v, torch.empty_like(q), torch.empty(B, H, SQ, device=DEV), do, torch.empty_like(q),
                        torch.empty_like(k), torch.empty_like(v), bias=bias, bias_grad=grad)
    assert (K.STATS["attention_bwd"], K.STATS["attention_bias_grad"]) == n0, "refused before any launch"


def _model():
    from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer

    m = FFModel(FFConfig())
    q, k, v = (m.create_tensor([4, 2, 64, 64], DataType.DT_FLOAT, name=n) for n in "qkv")
    w = m.create_weight([1, 2, 64, 64], name="bias")
    a = m.scaled_dot_product_attention(q, k, v, mask=w, name="attn0")
    m.scaled_dot_product_attention(a, k, v, mask=w, name="attn1")
    m.compile(optimizer=SGDOptimizer(m, lr=0.5), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    # bf16-representable values: the fp64 reference reads the same numbers
    ex.set_parameter("bias.w", torch.randn(1, 2, 64, 64, generator=torch.Generator().manual_seed(5)).bfloat16().float())
    return ex


def test_model_shared_learned_bias():
    """Two SDPA layers share one create_weight bias.  Graphed against eager: the bound of
    test_attention_bias_gpu.py's graphed model is max(twice their difference without the feature,
    1e-5); without the feature this model trains nothing, so its floor, 1e-5."""
    g = torch.Generator().manual_seed(6)
    feeds = {n: torch.randn(4, 2, 64, 64, generator=g).bfloat16().float().to(DEV) for n in "qkv"}
    dout, y = (torch.randn(4, 2, 64, 64, generator=g).to(DEV) for _ in range(2))
    ex = _model()
    n0 = K.STATS["attention_bias_grad"]
    ex.forward(feeds, training=True)
    ex.backward(dout)
    assert K.STATS["attention_bias_grad"] == n0 + 2, "the flash dbias kernel ran for both layers"
    wd = ex.get_parameter("bias.w").double().to(DEV).requires_grad_(True)
    a = feeds["q"].double()
    for _ in range(2):
        a = torch.nn.functional.scaled_dot_product_attention(a, feeds["k"].double(), feeds["v"].double(), attn_mask=wd)
    a.backward(dout.double())
    err = _rel(ex.get_parameter_grad("bias.w").to(DEV), wd.grad)
    print(f"attn_bias_grad model: shared bias gradient {err:.3e}")
    assert err <= _BF, err

    def weights(graphed):
        ex = _model()
        step = ex.make_graphed_train_step(feeds, y, warmup=1) if graphed else ex.train_step   # warmup: one eager step
        for _ in range(2 if graphed else 3):
            step(feeds, y)
        torch.cuda.synchronize()
        return ex.get_parameter("bias.w").double().cpu()

    we, wg = weights(False), weights(True)
    assert float((we - _model().get_parameter("bias.w").double().cpu()).norm()) > 0, "the bias moves"
    d = float((wg - we).norm() / we.norm())
    print(f"attn_bias_grad model: graphed vs eager {d:.3e}")
    assert d <= 1e-5, d
