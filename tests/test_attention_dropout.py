"""Attention dropout: the mask definition (ops/attention.py
attention_dropout_mask, the torch reference of what the flash kernels
regenerate) and the operator's fp32 CPU path.

The statistics use fixed inputs (seed 1234, B = 2, H = 3), so they are
deterministic: drop rate and pairwise mask agreement within 4 sigma of the
binomial expectation for independent masks.
"""
import math

import pytest
import torch

from flexflow_train_amd.ops import attention as A
from flexflow_train_amd.ops import base as opbase

B, H, SEED = 2, 3, 1234
SHAPES = [(200, 200), (96, 160), (64, 64)]
PS = [0.1, 0.5]


def test_mask_is_deterministic():
    a, sa = A.attention_dropout_mask(B, H, 96, 160, 0.1, SEED)
    b, sb = A.attention_dropout_mask(B, H, 96, 160, 0.1, SEED)
    assert a.dtype == torch.bool and tuple(a.shape) == (B, H, 96, 160)
    assert torch.equal(a, b) and sa == sb
    # the seed as a 1-element int64 tensor (the device step word's form) is the same seed
    c, _ = A.attention_dropout_mask(B, H, 96, 160, 0.1, torch.tensor([SEED]))
    assert torch.equal(a, c)


def test_mask_scalar_reference():
    """A few elements against the definition evaluated in Python integers."""
    M32, M64 = (1 << 32) - 1, (1 << 64) - 1
    Sq, Sk, p = 96, 160, 0.5
    T = int(round(p * (1 << 24)))
    mask, scale = A.attention_dropout_mask(B, H, Sq, Sk, p, SEED)
    assert scale == (1 << 24) / ((1 << 24) - T)
    for (b, h, q, k) in [(0, 0, 0, 0), (1, 2, 95, 159), (0, 1, 31, 64), (1, 0, 64, 31), (1, 1, 50, 7)]:
        z = (SEED + 0x9E3779B97F4A7C15 * (b * H + h + 1)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        x = ((q * Sk + k) ^ (z & M32)) & M32
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M32
        x ^= x >> 15
        x = (x * 0x846CA68B) & M32
        x ^= x >> 16
        assert bool(mask[b, h, q, k]) == ((x >> 8) >= T), (b, h, q, k)


def _within(rate, expect, n, what):
    sigma = math.sqrt(expect * (1 - expect) / n)
    z = abs(rate - expect) / sigma
    print(f"{what}: {rate:.5f} expected {expect:.5f} ({z:.2f} sigma, n = {n})")
    assert z < 4.0, (what, rate, expect, z)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_mask_statistics(Sq, Sk, p):
    T = int(round(p * (1 << 24)))
    rate = T / (1 << 24)
    m, scale = A.attention_dropout_mask(B, H, Sq, Sk, p, SEED)
    assert scale == pytest.approx(1 / (1 - rate), rel=1e-12)
    _within(1.0 - m.double().mean().item(), rate, m.numel(), "drop rate")
    agree = (1 - rate) ** 2 + rate ** 2   # two independent masks agree with this probability
    other, _ = A.attention_dropout_mask(B, H, Sq, Sk, p, SEED + 1)
    pairs = {"heads": (m[:, :-1], m[:, 1:]), "batches": (m[:-1], m[1:]), "seeds": (m, other),
             "adjacent rows": (m[:, :, :-1], m[:, :, 1:]), "adjacent columns": (m[..., :-1], m[..., 1:])}
    for what, (x, y) in pairs.items():
        _within((x == y).double().mean().item(), agree, x.numel(), what)


def test_mask_argument_errors():
    with pytest.raises(ValueError):
        A.attention_dropout_mask(1, 1, 8, 8, 1.0, 0)
    with pytest.raises(ValueError):
        A.attention_dropout_mask(1, 1, 8, 8, 1.5, 0)
    with pytest.raises(ValueError):      # shape arguments only: refused before anything is allocated
        A.attention_dropout_mask(1, 1, 1 << 16, 1 << 16, 0.1, 0)
    m, s = A.attention_dropout_mask(1, 1, 8, 8, 0.0, 0)
    assert bool(m.all()) and s == 1.0


# ---------------------------------------------------------------- model level
def _model(dropout):
    from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer

    cfg = FFConfig()
    cfg.cpu_only = True
    cfg.print_freq = 0
    m = FFModel(cfg)
    x = m.create_tensor([4, 16, 32], DataType.DT_FLOAT, name="x")
    a = m.multihead_attention(x, x, x, 32, 4, dropout=dropout, name="mha")
    m.softmax(m.dense(a, 8, name="head"), name="sm")
    m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              output=a)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.3)
    return ex


def test_model_attention_dropout_cpu():
    feeds = {"x": torch.randn(4, 16, 32, generator=torch.Generator().manual_seed(1))}

    def fwd(ex, training):
        return ex.forward(feeds, training=training, keep_outputs=True).detach().clone()

    plain_a, plain_b, drop = _model(0.0), _model(0.0), _model(0.5)
    ref = fwd(plain_a, False)
    # two dropout = 0 builds set the tolerance of the eval comparison
    tol = (ref - fwd(plain_b, False)).abs().max().item()
    ev = fwd(drop, False)
    assert (ev - ref).abs().max().item() <= tol, "eval forward must not depend on the dropout attribute"
    assert torch.equal(fwd(plain_a, True), ref), "dropout = 0: training forward equals eval forward"
    t1, t2 = fwd(drop, True), fwd(drop, True)
    assert not torch.allclose(t1, ev, rtol=1e-3, atol=1e-3), "training forward must apply the dropout"
    assert not torch.allclose(t1, t2, rtol=1e-3, atol=1e-3), "consecutive training forwards draw different masks"
    assert torch.equal(fwd(drop, False), ev)


def test_sequence_parallel_path_warns_once(monkeypatch):
    """Sequence-parallel attention does not apply the dropout: the operator
    says so once and computes what it computed before."""
    import warnings

    E, Hl, kd, Bn, S = 32, 4, 8, 2, 8
    calls = []

    def fake_fwd(q, k, v, causal, scale, grp, mode):
        calls.append(mode)
        return A._torch_attention(q, k, v, causal, scale), torch.zeros(Bn, Hl, S)

    monkeypatch.setattr(A.SP, "sp_attention_fwd", fake_fwd)
    monkeypatch.setattr(A.SP, "choose_mode", lambda attrs, Hl, grp: "ring")
    g = torch.Generator().manual_seed(5)
    W = torch.randn(E * 3 * Hl * kd + Hl * kd * E, generator=g).view(-1, Hl) * 0.3
    x = torch.randn(Bn, S, E, generator=g)
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = opbase.OpContext(op_type="MULTIHEAD_ATTENTION",
                           attrs={"embed_dim": E, "num_heads": Hl, "kdim": 0, "vdim": 0, "dropout": 0.5},
                           name="mha", training=True)
    ctx.extra["seq_group"] = type("Group", (), {"size": 2})()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        (a,), saved = impl.forward(ctx, [x, x, x], [W])
        (b,), _ = impl.forward(ctx, [x, x, x], [W])
    assert len([w for w in seen if "attention dropout is not applied" in str(w.message)]) == 1
    assert len(calls) == 2 and saved[-1] is None and "attn_drop_counter" not in ctx.extra
    torch.testing.assert_close(a, _reference(x, W, (E, Hl, kd), False, None), rtol=1e-4, atol=1e-5)
    assert torch.equal(a, b)


# ------------------------------------------------------------------- op level
def _reference(x, W, dims, causal, drop):
    E, Hl, kd = dims
    ws = A._split_weights(W, E, Hl, kd, kd, E, E, E)
    Bn, S, _ = x.shape
    qkv = (x.reshape(-1, E) @ ws["qkv"]).view(Bn, S, 3, Hl, kd)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(kd)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop[0].to(p.dtype) * drop[1]
    o = (p @ v).transpose(1, 2).reshape(Bn * S, Hl * kd)
    return (o @ ws["o"]).view(Bn, S, E)


@pytest.mark.parametrize("causal", [False, True])
def test_op_gradients_cpu(causal):
    """Two forwards, then their backwards in reverse order: each backward
    regenerates the mask of its own forward (the saved copy of the step word)."""
    E, Hl, kd, Bn, S, p = 32, 4, 8, 2, 24, 0.5
    g = torch.Generator().manual_seed(3)
    W = torch.randn(E * 3 * Hl * kd + Hl * kd * E, generator=g).view(-1, Hl) * 0.3
    xs = [torch.randn(Bn, S, E, generator=g) for _ in range(2)]
    douts = [torch.randn(Bn, S, E, generator=g) for _ in range(2)]
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = opbase.OpContext(op_type="MULTIHEAD_ATTENTION",
                           attrs={"embed_dim": E, "num_heads": Hl, "kdim": 0, "vdim": 0, "dropout": p,
                                  "causal": causal}, name="mha", seed=77, training=True)
    runs = []
    for x in xs:
        (out,), saved = impl.forward(ctx, [x, x, x], [W])
        runs.append((out, saved))
    masks = []
    for i, (out, saved) in enumerate(runs):
        rec_p, rec_seed, rec_step = saved[-1]
        assert rec_p == p and int(rec_step) == i + 1
        masks.append(A.attention_dropout_mask(Bn, Hl, S, S, p, rec_seed + int(rec_step)))
    assert not torch.equal(masks[0][0], masks[1][0])
    for i in (1, 0):
        out, saved = runs[i]
        xr, Wr = xs[i].clone().requires_grad_(True), W.clone().requires_grad_(True)
        ref = _reference(xr, Wr, (E, Hl, kd), causal, masks[i])
        torch.testing.assert_close(out, ref.detach(), rtol=1e-4, atol=1e-5)
        ref.backward(douts[i])
        dW = torch.zeros_like(W)
        gins = impl.backward(ctx, saved, [douts[i]], [dW], [True, False, False])
        torch.testing.assert_close(gins[0], xr.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(dW, Wr.grad, rtol=1e-4, atol=1e-5)
    # eval: no mask, no counter advance
    ctx.training = False
    (out,), saved = impl.forward(ctx, [xs[0], xs[0], xs[0]], [W])
    assert saved[-1] is None and int(ctx.extra["attn_drop_counter"]) == 2
    torch.testing.assert_close(out, _reference(xs[0], W, (E, Hl, kd), causal, None), rtol=1e-4, atol=1e-5)
