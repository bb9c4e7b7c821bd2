"""Flash attention at head dimension 256 (csrc/kernels/attention256.hip):
forward, dQ and dK/dV against fp64 torch on the same bf16 inputs, at the
smallest shapes that reach every path of the kernels (one element, exact
tiles, both tails with cross-attention, causal across a query-block boundary,
GQA and MQA), then views, guarded tails, reproducibility, refusals and the
operators.  The error is the relative Frobenius error of tests/test_kernels_gpu.py.

Tolerance 5e-3, the bound of the D = 64 / 128 tests.  Measured on an MI355X at
the shapes below (profiles/attn_d256.txt): the D = 256 kernels reach at most
2.6e-3 against fp64 (o, lse, dq, dk, dv over all cases), and
ops.attention._torch_attention fed the same bf16 inputs, the path these
calls took before, reaches 1.7e-3."""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV, BF16, D = "cuda", torch.bfloat16, 256
_TOL = 5e-3
_LN2 = math.log(2.0)


def _rel64(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _ref(q, k, v, do, causal):
    """fp64 softmax(scale Q K^T + causal mask) V on [B, S, H, D] inputs and its autograd gradients."""
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kd.repeat_interleave(G, 2)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(s.shape[2:], dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vd.repeat_interleave(G, 2))
    o.backward(do.double())
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), -1), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad,
            "p": p.detach()}


def _err(n, got, ref, ins):
    """Relative Frobenius error of result n.  With one key dS = P (dP - delta) is exactly zero and dq / dk have
    no norm to be relative to: they are measured against the term that cancels, scale (P dP) K and its dk form."""
    if n == "lse":
        return _rel64(got[n] * _LN2, ref[n])
    if n in ("dq", "dk") and float(ref[n].norm()) == 0.0:
        q, k, v, do = (t.double() for t in ins)
        pdp = ref["p"] * torch.einsum("bqhd,bkhd->bhqk", do, v.repeat_interleave(q.shape[2] // k.shape[2], 2))
        whole = torch.einsum("bhqk,bkhd->bqhd" if n == "dq" else "bhqk,bqhd->bkhd", pdp, k if n == "dq" else q)
        return ((got[n].double() - ref[n]).norm() / (whole / math.sqrt(D)).norm()).item()
    return _rel64(got[n], ref[n])


def _run(q, k, v, do, causal, out=None, grads=None):
    o, lse = K.attention_fwd(q, k, v, causal=causal, out=out)
    dq, dk, dv = grads if grads is not None else (torch.empty_like(t) for t in (q, k, v))
    assert K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, causal=causal) == 0
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


@functools.lru_cache(maxsize=None)
def _case(B, H, Hkv, Sq, Sk, causal):
    """Inputs, the kernels' results and the fp64 reference of one shape, made once and shared."""
    g = torch.Generator().manual_seed(1000 * Sq + Sk)
    q, do = (torch.randn(B, Sq, H, D, generator=g).to(DEV, BF16) for _ in range(2))
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g).to(DEV, BF16) for _ in range(2))
    n0 = K.STATS["attention_d256"]
    got = _run(q, k, v, do, causal)
    assert K.STATS["attention_d256"] == n0 + 2, "the forward and the backward take the D = 256 kernels"
    return (q, k, v, do), got, _ref(q, k, v, do, causal)


CASES = [(1, 1, 1, 1, 1, False), (2, 3, 3, 64, 64, False), (1, 2, 2, 129, 67, False), (1, 2, 2, 130, 130, True),
         (2, 4, 2, 96, 96, True), (1, 4, 1, 65, 200, False)]
EXACT, TAILS, GQA = CASES[1], CASES[2], CASES[4]


@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_fp64(case):
    ins, got, ref = _case(*case)
    errs = {n: _err(n, got, ref, ins) for n in got}
    print(f"attn_d256 {case}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert max(errs.values()) < _TOL, errs


def test_strided_views_equal_contiguous_bits():
    """q / k / v as slices of one packed [B, S, 3, H, D] buffer, dq / dk / dv into slices of a second."""
    (q, k, v, do), want, _ = _case(*EXACT)
    qkv = torch.stack([q, k, v], dim=2)
    dqkv = torch.empty_like(qkv)
    got = _run(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], do, False, grads=(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]))
    for n in want:
        assert torch.equal(got[n], want[n]), n


def test_tails_are_never_read_or_written():
    """Inputs are views into NaN-filled buffers whose rows after the view are NaN; outputs go into
    NaN-prefilled buffers.  The results are those of the clean call and the guard rows keep their bytes."""
    (q, k, v, do), want, _ = _case(*TAILS)

    def guarded(t, fill):
        buf = torch.full((t.shape[0], t.shape[1] + 3, *t.shape[2:]), float("nan"), device=DEV, dtype=BF16)
        if fill:
            buf[:, :t.shape[1]] = t
        return buf

    ins = [guarded(t, True) for t in (q, k, v, do)]
    outs = [guarded(t, False) for t in (q, q, k, v)]   # o, dq, dk, dv
    before = [b.clone() for b in outs]
    cut = lambda b, t: b[:, :t.shape[1]]
    got = _run(*(cut(b, t) for b, t in zip(ins, (q, k, v, do))), False, out=cut(outs[0], q),
               grads=tuple(cut(b, t) for b, t in zip(outs[1:], (q, k, v))))
    for n in want:
        assert torch.isfinite(got[n]).all() and torch.equal(got[n], want[n]), n
    for b, b0, t in zip(outs, before, (q, q, k, v)):
        assert torch.equal(b[:, t.shape[1]:].view(torch.int16), b0[:, t.shape[1]:].view(torch.int16))


def test_backward_is_reproducible():
    (q, k, v, do), want, _ = _case(*GQA)
    again = _run(q, k, v, do, True)
    for n in want:
        assert torch.equal(again[n], want[n]), n


@pytest.mark.parametrize("name", ["dropout", "kv_lens", "q_lens", "seg_lens", "bias", "window", "dbias"])
def test_refusals_name_the_feature(name):
    (q, k, v, do), got, _ = _case(*EXACT)
    B, Sq, H, _ = q.shape
    i32 = lambda *s: torch.full(s, 8, device=DEV, dtype=torch.int32)
    kw = {"dropout": dict(dropout_p=0.1), "kv_lens": dict(kv_lens=i32(B)), "q_lens": dict(q_lens=i32(B)),
          "seg_lens": dict(seg_lens=i32(B, 1)), "bias": dict(bias=torch.zeros(1, 1, Sq, Sq, device=DEV)),
          "window": dict(window=8, causal=True),
          "dbias": dict(dbias=tuple(torch.zeros(H * D, device=DEV) for _ in range(3)))}[name]
    snap = dict(K.STATS)
    with pytest.raises(ValueError, match=f"head dim 256.*{name}"):
        if name == "dbias":
            K.attention_bwd(q, k, v, got["o"], got["lse"], do, *(torch.empty_like(t) for t in (q, k, v)), **kw)
        else:
            K.attention_fwd(q, k, v, **kw)
    assert dict(K.STATS) == snap, "a refused call launched or counted something"


# ------------------------------------------------------------------ operators
def _op(op_type, attrs, inputs, weights, do):
    from flexflow_train_amd.ops import base as opbase

    impl = opbase.get_impl(op_type)
    ctx = opbase.OpContext(op_type=op_type, attrs=attrs, name="op", training=True, compute_dtype=BF16,
                           device=torch.device(DEV))
    (o,), saved = impl.forward(ctx, inputs, weights)
    wg = [torch.zeros(w.shape, device=DEV) for w in weights]
    return [o, impl.backward(ctx, saved, [do], wg, [True] * len(inputs))[:3], wg]


def test_sdpa_operator_gqa_causal():
    g = torch.Generator().manual_seed(3)
    q, do = (torch.randn(2, 4, 96, D, generator=g).to(DEV, BF16) for _ in range(2))
    k, v = (torch.randn(2, 2, 96, D, generator=g).to(DEV, BF16) for _ in range(2))
    n0 = K.STATS["attention_d256"]
    o, grads, _ = _op("SDPA", {"causal": True}, [q, k, v], [], do)
    assert K.STATS["attention_d256"] == n0 + 2
    t = lambda x: x.transpose(1, 2)
    ref = _ref(t(q), t(k), t(v), t(do), True)
    errs = {n: _rel64(a, t(ref[n])) for n, a in zip(("o", "dq", "dk", "dv"), (o, *grads))}
    print("attn_d256 SDPA: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert max(errs.values()) < _TOL, errs


def test_multihead_attention_operator(monkeypatch):
    """Self-attention, E = 512 over 2 heads, biases on: against fp64 on the bf16 weights, and against the
    FF_ATTN_D256=0 run of the same operator (the path before these kernels), which is the reference there."""
    g = torch.Generator().manual_seed(4)
    E, H, B, S = 512, 2, 2, 80
    x, do = (torch.randn(B, S, E, generator=g).to(DEV, BF16) for _ in range(2))
    W = (torch.randn(E * 3 * E + E * E, generator=g) * 0.05).to(DEV, BF16).view(-1, H)
    b_in, b_out = ((torch.randn(n, generator=g) * 0.1).to(DEV, BF16) for n in (3 * E, E))
    attrs = {"embed_dim": E, "num_heads": H, "kdim": 0, "vdim": 0, "causal": False}
    names = ("out", "dx", "dW", "db_in", "db_out")

    def run():
        o, (dx, *_), wg = _op("MULTIHEAD_ATTENTION", attrs, [x, x, x], [W, b_in, b_out], do)
        return dict(zip(names, (o, dx, *wg)))

    n0 = K.STATS["attention_d256"]
    got = run()
    assert K.STATS["attention_d256"] == n0 + 2
    monkeypatch.setenv("FF_ATTN_D256", "0")
    old = run()
    assert K.STATS["attention_d256"] == n0 + 2, "FF_ATTN_D256=0 restores the torch path"
    xd, Wd, bi, bo = (t.double().requires_grad_(True) for t in (x, W, b_in, b_out))
    Wqkv, Wo = Wd.reshape(-1)[:E * 3 * E].view(E, 3 * E), Wd.reshape(-1)[E * 3 * E:].view(E, E)
    q, k, v = (xd.reshape(-1, E) @ Wqkv + bi).view(B, S, 3, H, D).unbind(2)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D), -1)
    ref = (torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(-1, E) @ Wo + bo).view(B, S, E)
    ref.backward(do.double())
    want = dict(zip(names, (ref.detach(), xd.grad, Wd.grad, bi.grad, bo.grad)))
    e64 = {n: _rel64(got[n], want[n]) for n in names}
    eold = {n: _rel64(got[n], old[n]) for n in names}
    print("attn_d256 MHA vs fp64: " + " ".join(f"{n} {e:.3e}" for n, e in e64.items()))
    print("attn_d256 MHA vs FF_ATTN_D256=0: " + " ".join(f"{n} {e:.3e}" for n, e in eold.items()))
    assert max(e64.values()) < _TOL and max(eold.values()) < _TOL, (e64, eold)


def test_llama_trains_to_the_fallback_weights(monkeypatch):
    """A tiny LLaMA with D = 256 heads (hidden 512, 2 heads, 1 K / V head) reaches in three steps the weights
    of its FF_ATTN_D256=0 run.  Bound, as in tests/test_swiglu_gpu.py: twice what a re-rounding does to this
    model where none of the new code runs (FF_ATTN_D256=0 with perform_fusion on against off), at least 1e-5."""
    from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType
    from flexflow_train_amd.models.llama import LlamaConfig, build_llama

    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 256, (2, 65), generator=g, dtype=torch.int32)
    feeds, labels = {"input_ids": ids[:, :64].contiguous().to(DEV)}, ids[:, 1:].long().contiguous().to(DEV)

    def train(fuse=True):
        cfg = FFConfig()
        cfg.perform_fusion = fuse
        m = FFModel(cfg)
        build_llama(m, LlamaConfig(vocab_size=256, hidden_size=512, num_layers=2, num_heads=2, num_kv_heads=1,
                                   intermediate_size=512, sequence_length=64, batch_size=2))
        m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
        ex, gw = m.executor, torch.Generator().manual_seed(0)
        for n in sorted(ex.parameter_names()):
            ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=gw) * 0.1
                             + (1.0 if n.endswith("gamma") else 0.0))
        for _ in range(3):
            ex.train_step(feeds, labels)
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    worst = lambda p, r: max(float((p[n] - r[n]).norm() / r[n].norm()) for n in p)
    n0 = K.STATS["attention_d256"]
    got = train()
    assert K.STATS["attention_d256"] == n0 + 12   # two layers, three forwards and three backwards
    monkeypatch.setenv("FF_ATTN_D256", "0")
    want = train()
    bound = max(2 * worst(train(fuse=False), want), 1e-5)
    assert K.STATS["attention_d256"] == n0 + 12
    d1 = worst(got, want)
    print(f"attn_d256 llama vs FF_ATTN_D256=0: {d1:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
