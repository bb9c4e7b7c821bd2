"""Grouped-query attention (fewer K / V heads than query heads) in the flash
attention kernels (the GQA instantiations of attention.hip), and the SDPA
operator on top of them.

Shapes: B = 2, H = 6 query heads over Hkv in {1, 2, 3} K / V heads; (Sq, Sk) =
(200, 136) non-causal crosses the 128-query block and the 64-key tile,
(200, 200) causal, (40, 8) non-causal is one partial tile; D in {64, 128}.
The reference is fp64 attention on the same bf16 inputs with K / V
repeat_interleave'd to H heads, autograd doing the group sum.  Bounds are the
project's: relative Frobenius 5e-3 for o / dq / dk / dv and 1e-4 absolute for
the LSE in the log2 domain.  Every case prints its errors.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 6
CASES = [(200, 136, False), (200, 200, True), (40, 8, False)]
_BF = 5e-3
_LSE = 1e-4
LOG2E = 1.4426950408889634


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def _inputs(Sq, Sk, D, Hkv):
    g = torch.Generator().manual_seed(Sq * 1000 + Sk + D + 7 * Hkv)
    q = torch.randn(B, Sq, H, D, generator=g).to(DEV, torch.bfloat16)
    k = torch.randn(B, Sk, Hkv, D, generator=g).to(DEV, torch.bfloat16)
    v = torch.randn(B, Sk, Hkv, D, generator=g).to(DEV, torch.bfloat16)
    do = torch.randn(B, Sq, H, D, generator=g).to(DEV, torch.bfloat16)
    return q, k, v, do


@functools.lru_cache(maxsize=None)
def _ref64(Sq, Sk, D, Hkv, causal):
    """fp64 attention on K / V expanded to H heads: (o, lse log2, dq, dk, dv),
    [B, S, heads, D] / [B, H, Sq]; dk / dv have Hkv heads (autograd sums the group)."""
    q, k, v, do = _inputs(Sq, Sk, D, Hkv)
    G = H // Hkv
    qd, kd, vd = (t.double().transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
    ke, ve = kd.repeat_interleave(G, dim=1), vd.repeat_interleave(G, dim=1)
    s = qd @ ke.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    lse = torch.logsumexp(s.detach(), -1) * LOG2E
    o = torch.softmax(s, -1) @ ve
    o.backward(do.double().transpose(1, 2))
    return (o.detach().transpose(1, 2), lse, qd.grad.transpose(1, 2), kd.grad.transpose(1, 2),
            vd.grad.transpose(1, 2))


def _run(q, k, v, do, **kw):
    o, lse = K.attention_fwd(q, k, v, **kw)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    path = K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, **kw)
    return (o, lse, dq, dk, dv), path


def _errors(got, want):
    for t in got:
        assert not torch.isnan(t).any()
    errs = {n: _rel(g, w) for n, g, w in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4]),
                                             (want[0], want[2], want[3], want[4]))}
    errs["lse"] = float((got[1].double() - want[1]).abs().max())
    return errs


def _check(tag, got, want):
    errs = _errors(got, want)
    print(f"attn_gqa {tag}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    for n in ("o", "dq", "dk", "dv"):
        assert errs[n] <= _BF, (tag, n, errs[n])
    assert errs["lse"] <= _LSE, (tag, errs["lse"])
    return errs


def _expanded(k, v, G):
    return k.repeat_interleave(G, dim=2), v.repeat_interleave(G, dim=2)


# --------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("Hkv", [1, 2, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk,causal", CASES)
def test_gqa_against_fp64(Sq, Sk, causal, D, Hkv):
    q, k, v, do = _inputs(Sq, Sk, D, Hkv)
    n0 = K.STATS["attention_gqa"]
    got, path = _run(q, k, v, do, causal=causal)
    assert K.STATS["attention_gqa"] == n0 + 2
    assert path == 0, "the GQA backward is always the dQ + dK/dV pair"
    assert got[0].shape == (B, Sq, H, D) and got[1].shape == (B, H, Sq)
    assert got[3].shape == (B, Sk, Hkv, D) and got[4].shape == (B, Sk, Hkv, D)
    _check(f"Hkv={Hkv} Sq={Sq} Sk={Sk} D={D} causal={causal}", got, _ref64(Sq, Sk, D, Hkv, causal))


# ------------------------------- 2. against the existing kernels on expanded K/V
@pytest.mark.parametrize("Hkv", [1, 2, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk,causal", CASES)
def test_gqa_against_expanded_call(Sq, Sk, causal, D, Hkv, monkeypatch):
    # the expanded call is to run the dQ + dK/dV pair, the kernels whose GQA
    # forms are under test: where it is eligible for the one-pass backward
    # (D = 64, non-causal, Sk <= 512) that kernel forms dQ in another order
    monkeypatch.setenv("FFK_ATTN_BWD_ONEPASS", "0")
    q, k, v, do = _inputs(Sq, Sk, D, Hkv)
    G = H // Hkv
    want = _ref64(Sq, Sk, D, Hkv, causal)
    got, _ = _run(q, k, v, do, causal=causal)
    ke, ve = _expanded(k, v, G)
    n0 = K.STATS["attention_gqa"]
    exp, path = _run(q, ke, ve, do, causal=causal)
    assert K.STATS["attention_gqa"] == n0 and path == 0
    # every query head does the same arithmetic on the same bits
    assert torch.equal(got[0], exp[0]), "o"
    assert torch.equal(got[1], exp[1]), "lse"
    assert torch.equal(got[2], exp[2]), "dq"
    # dk / dv: the expanded call rounds every head's gradient to bf16 before the group sum
    dk_sum = exp[3].view(B, Sk, Hkv, G, D).sum(3, dtype=torch.float32)
    dv_sum = exp[4].view(B, Sk, Hkv, G, D).sum(3, dtype=torch.float32)
    tag = f"Hkv={Hkv} Sq={Sq} Sk={Sk} D={D} causal={causal}"
    for n, mine, theirs, ref in (("dk", got[3], dk_sum, want[3]), ("dv", got[4], dv_sum, want[4])):
        e_gqa, e_exp = _rel(mine, ref), _rel(theirs, ref)
        print(f"attn_gqa vs expanded {tag}: {n} gqa {e_gqa:.3e} expanded-and-summed (fp32) {e_exp:.3e}")
        assert e_gqa <= _BF and e_gqa <= e_exp + _BF, (tag, n, e_gqa, e_exp)


# ------------------------------------------------ 3. Hkv == H: today's kernels
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk,causal", CASES)
def test_equal_heads_take_the_existing_kernels(Sq, Sk, causal, D):
    q, k, v, do = _inputs(Sq, Sk, D, H)
    n0 = K.STATS["attention_gqa"]
    got, _ = _run(q, k, v, do, causal=causal)
    assert K.STATS["attention_gqa"] == n0
    # a call that never heard of GQA: the extension entry points without kv_heads
    ext = K.ext()
    view = lambda t: (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    o = torch.empty_like(q)
    lse = torch.empty(B, H, Sq, device=DEV, dtype=torch.float32)
    sc = 1.0 / math.sqrt(D)
    st = torch.cuda.current_stream().cuda_stream
    ext.attention_fwd(view(q), view(k), view(v), view(o), lse.data_ptr(), B, H, Sq, Sk, D, sc, causal, st)
    assert torch.equal(o, got[0]) and torch.equal(lse, got[1])
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty_like(lse)
    n_ws = ext.attention_bwd_workspace(B, H, Sq, Sk, D, causal, False)
    ws = torch.empty(max(n_ws, 1), device=DEV, dtype=torch.float32)
    ext.attention_bwd(view(q), view(k), view(v), view(o), view(do), view(dq), view(dk), view(dv), lse.data_ptr(),
                      delta.data_ptr(), B, H, Sq, Sk, D, sc, causal, st, ws=ws.data_ptr() if n_ws else 0)
    torch.cuda.synchronize()
    assert torch.equal(dq, got[2]) and torch.equal(dk, got[3]) and torch.equal(dv, got[4])


# -------------------------------------- 4. strided operands, guarded outputs
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_fused_buffers_strided_and_guarded(causal, D, Hkv):
    S = 200
    q, k, v, do = _inputs(S, S, D, Hkv)
    want, _ = _run(q, k, v, do, causal=causal)
    fused = torch.empty(B, S, H + 2 * Hkv, D, device=DEV, dtype=torch.bfloat16)
    fused[:, :, :H], fused[:, :, H:H + Hkv], fused[:, :, H + Hkv:] = q, k, v
    qs, ks, vs = fused[:, :, :H], fused[:, :, H:H + Hkv], fused[:, :, H + Hkv:]
    assert not ks.is_contiguous()
    # gradient buffer with two guard heads between and around the slices, all NaN
    W = H + 2 * Hkv + 4
    grad = torch.full((B, S, W, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    a, b_, c = 1, 1 + H + 1, 1 + H + 1 + Hkv + 1
    dq, dk, dv = grad[:, :, a:a + H], grad[:, :, b_:b_ + Hkv], grad[:, :, c:c + Hkv]
    before = grad.clone()
    o, lse = K.attention_fwd(qs, ks, vs, causal=causal)
    path = K.attention_bwd(qs, ks, vs, o, lse, do, dq, dk, dv, causal=causal)
    assert path == 0
    got = (o, lse, dq, dk, dv)
    for n, x, y in zip(("o", "lse", "dq", "dk", "dv"), got, want):
        assert torch.equal(x, y), n
    written = torch.zeros(W, dtype=torch.bool)
    written[a:a + H] = written[b_:b_ + Hkv] = written[c:c + Hkv] = True
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(grad)[:, :, ~written], bits(before)[:, :, ~written]), \
        "bytes outside the three slices were written"
    assert not torch.isnan(grad[:, :, written]).any()


# -------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing():
    Sq, Sk, D, Hkv = 200, 136, 64, 2
    q, k, v, do = _inputs(Sq, Sk, D, Hkv)
    o, lse = K.attention_fwd(q, k, v)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    g = torch.Generator().manual_seed(3)
    k4, v4 = (torch.randn(B, Sk, 4, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    k3 = torch.randn(B, Sk, 3, D, generator=g).to(DEV, torch.bfloat16)
    lens = torch.full((B,), 100, dtype=torch.int32, device=DEV)
    snap = dict(K.STATS)
    with pytest.raises(ValueError, match="H % Hkv"):
        K.attention_fwd(q, k4, v4)
    with pytest.raises(ValueError, match="v has 3 heads, k has 2"):
        K.attention_fwd(q, k, k3)
    with pytest.raises(ValueError, match="grouped-query.*dropout_p"):
        K.attention_fwd(q, k, v, dropout_p=0.1, seed=1)
    with pytest.raises(ValueError, match="grouped-query.*kv_lens"):
        K.attention_fwd(q, k, v, kv_lens=lens)
    with pytest.raises(ValueError, match="grouped-query.*q_lens"):
        K.attention_fwd(q, k, v, q_lens=lens)
    with pytest.raises(ValueError, match="grouped-query.*seg_lens"):
        K.attention_fwd(q, k, v, seg_lens=torch.full((B, 1), 100, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="grouped-query.*bias"):
        K.attention_fwd(q, k, v, bias=torch.zeros(B, H, Sq, Sk, device=DEV))
    with pytest.raises(ValueError, match="grouped-query.*dbias"):
        K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv,
                        dbias=tuple(torch.zeros(H * D, device=DEV) for _ in range(3)))
    with pytest.raises(ValueError, match="grouped-query.*dropout_p"):
        K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, dropout_p=0.1, seed=1)
    wide = torch.empty(B, Sk, H, D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="dk has shape.*grouped-query"):
        K.attention_bwd(q, k, v, o, lse, do, dq, wide, dv)
    with pytest.raises(ValueError, match="dv has shape.*grouped-query"):
        K.attention_bwd(q, k, v, o, lse, do, dq, dk, wide)
    # shapes wrong for other reasons keep the old text
    with pytest.raises(ValueError, match="q/k/v shape mismatch"):
        K.attention_fwd(q, k, v[:, :100])
    assert dict(K.STATS) == snap, "a refused call launched or counted something"
    # the C++ entry refuses the same combinations by name
    ext = K.ext()
    view = lambda t: (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    args = (view(q), view(k), view(v), view(o), lse.data_ptr(), B, H, Sq, Sk, D, 0.125, False, 0)
    with pytest.raises(ValueError, match="must divide"):
        ext.attention_fwd(*args, kv_heads=4)
    with pytest.raises(ValueError, match="kv_heads.*dropout"):
        ext.attention_fwd(*args, drop_t=1000, seed=1, kv_heads=2)
    with pytest.raises(ValueError, match="kv_heads.*kv_lens"):
        ext.attention_fwd(*args, kv_lens=lens.data_ptr(), kv_heads=2)
    with pytest.raises(ValueError, match="kv_heads.*kv_lens"):
        ext.attention_fwd(*args, q_lens=lens.data_ptr(), kv_heads=2)
    with pytest.raises(ValueError, match="kv_heads.*bias"):
        ext.attention_fwd(*args, bias=(lse.data_ptr(), 0, 0, 0), kv_heads=2)


# ----------------------------------------------------------- 6. the operator
def _sdpa_op(attrs, inputs, do, training=True):
    from flexflow_train_amd.ops import base as opbase

    impl = opbase.get_impl("SDPA")
    ctx = opbase.OpContext(op_type="SDPA", attrs=attrs, name="sdpa", training=training,
                           compute_dtype=torch.bfloat16, device=torch.device(DEV))
    (o,), saved = impl.forward(ctx, inputs, [])
    return o, impl.backward(ctx, saved, [do], [], [True] * len(inputs)), saved


@pytest.mark.parametrize("case", ["none", "causal", "key_mask", "dropout", "fp32"])
@pytest.mark.parametrize("D", [64, 128])
def test_operator_with_fewer_kv_heads(D, case):
    Hkv, G = 2, H // 2
    Sq, Sk = (192, 192) if case == "causal" else (200, 136)
    dt = torch.float32 if case == "fp32" else torch.bfloat16
    g = torch.Generator().manual_seed(31 + D)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, dt)
    k, v = (torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, dt) for _ in range(2))
    do = torch.randn(B, H, Sq, D, generator=g).to(DEV, dt)
    attrs, mask = {}, None
    if case == "causal":
        attrs["causal"] = True
    elif case == "key_mask":
        mask = torch.zeros(B, 1, 1, Sk).masked_fill(torch.arange(Sk).view(1, 1, 1, Sk) >= torch.tensor([Sk, 77]).view(
            B, 1, 1, 1), float("-inf")).to(DEV)
        attrs["mask"] = True
    elif case == "dropout":
        attrs["dropout"] = 0.1
    n0 = {n: K.STATS[n] for n in ("attention_gqa", "attention_bias", "attention_dropout", "attention_fwd")}
    o, grads, saved = _sdpa_op(attrs, [q, k, v] + ([mask] if mask is not None else []), do)
    d = {n: K.STATS[n] - n0[n] for n in n0}
    assert d["attention_gqa"] == (2 if case in ("none", "causal") else 0), d
    assert d["attention_bias"] == (2 if case == "key_mask" else 0), d
    assert d["attention_dropout"] == (2 if case == "dropout" else 0), d
    assert d["attention_fwd"] == (0 if case == "fp32" else 1), d
    assert o.shape == (B, H, Sq, D) and grads[0].shape == q.shape
    assert grads[1].shape == (B, Hkv, Sk, D) and grads[2].shape == (B, Hkv, Sk, D)
    # fp64 on K / V expanded to H heads
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qd @ kd.repeat_interleave(G, dim=1).transpose(-1, -2) / math.sqrt(D)
    if case == "causal":
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    if mask is not None:
        s = s + mask.double()
    p = torch.softmax(s, -1)
    if case == "dropout":
        # the forward's drop record (p, host seed, device step word): the mask has H heads
        p_drop, seed, step = saved[8]
        keep, rs = attention_dropout_mask(B, H, Sq, Sk, p_drop, seed + int(step), DEV)
        assert not keep.all() and keep.shape == (B, H, Sq, Sk)
        p = p * keep.double() * rs
    ref = p @ vd.repeat_interleave(G, dim=1)
    ref.backward(do.double())
    errs = {n: _rel(a, b) for n, a, b in zip(("o", "dq", "dk", "dv"), (o, *grads[:3]),
                                             (ref.detach(), qd.grad, kd.grad, vd.grad))}
    print(f"attn_gqa operator {case} D={D}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert max(errs.values()) <= (_BF if dt == torch.bfloat16 else 1e-5), errs


# ------------------------------------------------------------- 7. a model
def _two_layer_model(Hkv):
    """dense -> reshape / transpose -> SDPA twice, 4 query heads over Hkv K / V heads of D = 64."""
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    Hq = 4
    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    h = x
    for i in range(2):
        q, k, v = (m.transpose(m.reshape(m.dense(h, nh * 64, name=f"{n}{i}"), [4, 64, nh, 64]), [0, 2, 1, 3])
                   for n, nh in (("q", Hq), ("k", Hkv), ("v", Hkv)))
        a = m.scaled_dot_product_attention(q, k, v, causal=True, name=f"attn{i}")
        h = m.add(h, m.dense(m.reshape(m.transpose(a, [0, 2, 1, 3]), [4, 64, Hq * 64]), 128, name=f"o{i}"))
    m.softmax(m.dense(h, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.1)
    return ex


def test_model_graphed_step_matches_eager():
    """Two SDPA layers built with FFModel.scaled_dot_product_attention and
    Hkv = 2 < H = 4: the captured step reaches the eager step's weights.  The
    bound is the one test_attention_bias_gpu.py uses for the same check: twice
    what graphed against eager differ by in the same model with Hkv == H, at
    least 1e-5."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 8, (4, 64), generator=g).to(DEV)

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(Hkv):
        ex = _two_layer_model(Hkv)
        for _ in range(3):
            ex.train_step({"input": x}, y)
        return params(ex)

    def graphed(Hkv):
        ex = _two_layer_model(Hkv)
        step = ex.make_graphed_train_step({"input": x}, y, warmup=1)   # one eager step, then two replays
        step({"input": x}, y)
        step({"input": x}, y)
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    n0 = K.STATS["attention_gqa"]
    d0 = worst(graphed(4), eager(4))
    assert K.STATS["attention_gqa"] == n0, "Hkv == H takes the existing kernels"
    bound = max(2 * d0, 1e-5)
    want = eager(2)
    assert K.STATS["attention_gqa"] == n0 + 12     # two layers, three forwards and three backwards
    d1 = worst(graphed(2), want)
    print(f"attn_gqa graphed vs eager: Hkv == H {d0:.3e}, Hkv = 2 {d1:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
