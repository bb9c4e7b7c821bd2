"""Sliding-window causal attention in the flash kernels (WINDOW instantiations
of attention.hip): key k is visible to query q iff 0 <= q - k < W.  S = 400 is
3 query blocks and a 16-row tail, 6 key tiles and a 16-key tail: block 2 skips
tiles on the left, key block 0's query loop ends early, the last tiles are
partial.  Reference: fp64 with the band mask applied explicitly.  Bounds are the
project's: relative Frobenius 5e-3 for o / dq / dk / dv, 1e-4 for the LSE (log2)."""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, S = 2, 4, 400
LOG2E = 1.4426950408889634


@functools.lru_cache(maxsize=None)
def _inputs(D, Hkv):
    g = torch.Generator().manual_seed(400 + D + 7 * Hkv)
    q, do = (torch.randn(B, S, H, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    k, v = (torch.randn(B, S, Hkv, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    return q, k, v, do


def _run(q, k, v, do, **kw):
    o, lse = K.attention_fwd(q, k, v, causal=True, **kw)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    assert K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, causal=True, **kw) == 0
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("W", [1, 17, 64, 100, 129])
@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("D", [64, 128])
def test_window_against_fp64(D, Hkv, W):
    q, k, v, do = _inputs(D, Hkv)
    n0 = K.STATS["attention_window"]
    got = _run(q, k, v, do, window=W)
    assert K.STATS["attention_window"] == n0 + 2
    qd, kd, vd = (t.double().transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (kd, vd))
    d = torch.arange(S, device=DEV).view(S, 1) - torch.arange(S, device=DEV).view(1, S)   # q - k
    s = (qd @ ke.transpose(-1, -2) / math.sqrt(D)).masked_fill((d < 0) | (d >= W), float("-inf"))
    o = torch.softmax(s, -1) @ ve
    o.backward(do.double().transpose(1, 2))
    want = (o.detach(), None, qd.grad, kd.grad, vd.grad)
    errs = {n: float((got[i].double() - want[i].transpose(1, 2)).norm() / want[i].norm())
            for n, i in (("o", 0), ("dq", 2), ("dk", 3), ("dv", 4))}
    if W == 1:
        # one key per row: dS = P (dP - delta) is exactly 0 and so are the fp64 dq / dk; the error is taken
        # relative to the term that cancels, scale * (dO . V) K for dq and scale * (dO . V) Q for dk
        G = H // Hkv
        dp = (do.double() * v.double().repeat_interleave(G, dim=2)).sum(-1, keepdim=True) / math.sqrt(D)
        errs["dq"] = float(got[2].double().norm() / (dp * k.double().repeat_interleave(G, dim=2)).norm())
        errs["dk"] = float(got[3].double().norm() / (dp * q.double()).view(B, S, Hkv, G, D).sum(3).norm())
    errs["lse"] = float((got[1].double() - torch.logsumexp(s.detach(), -1) * LOG2E).abs().max())
    print(f"attn_window D={D} Hkv={Hkv} W={W}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(errs[n] <= 5e-3 for n in ("o", "dq", "dk", "dv")) and errs["lse"] <= 1e-4, errs
    if W == 1:   # every row sees only itself: o = v up to one bf16 rounding
        torch.testing.assert_close(got[0], v.repeat_interleave(H // Hkv, dim=2), rtol=2.0 ** -7, atol=0)
    assert all(torch.equal(a, b) for a, b in zip(got, _run(q, k, v, do, window=W))), "two calls give equal bits"


def test_window_over_all_keys_is_plain_causal():
    q, k, v, do = _inputs(64, 1)
    plain = _run(q, k, v, do)
    n0 = K.STATS["attention_window"]
    for W in (S, 4096):
        assert all(torch.equal(a, b) for a, b in zip(_run(q, k, v, do, window=W), plain)), W
    assert K.STATS["attention_window"] == n0


def test_refusals_launch_nothing():
    q, k, v, do = _inputs(64, 4)
    o, lse = K.attention_fwd(q, k, v, causal=True, window=64)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lens = torch.full((B,), 100, dtype=torch.int32, device=DEV)
    bias = torch.zeros(1, 1, S, S, device=DEV)
    snap = dict(K.STATS)
    with pytest.raises(ValueError, match="window must be >= 1"):
        K.attention_fwd(q, k, v, causal=True, window=0)
    with pytest.raises(ValueError, match="window needs causal"):
        K.attention_fwd(q, k, v, window=64)
    for what, kw in (("dropout_p", dict(dropout_p=0.1, seed=1)), ("kv_lens", dict(kv_lens=lens)),
                     ("q_lens", dict(q_lens=lens)), ("seg_lens", dict(seg_lens=lens.view(B, 1))),
                     ("bias", dict(bias=bias))):
        with pytest.raises(ValueError, match=f"window cannot be combined with .*{what}"):
            K.attention_fwd(q, k, v, causal=True, window=64, **kw)
        with pytest.raises(ValueError, match=f"window cannot be combined with .*{what}"):
            K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, causal=True, window=64, **kw)
    for what, kw in (("dbias", dict(dbias=tuple(torch.zeros(H * 64, device=DEV) for _ in range(3)))),
                     ("bias_grad", dict(bias_grad=torch.zeros(1, 1, S, S, device=DEV)))):
        with pytest.raises(ValueError, match=f"window cannot be combined with .*{what}"):
            K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, causal=True, window=64, **kw)
    assert dict(K.STATS) == snap, "a refused call launched or counted something"


def _model(window):
    # dense -> reshape / transpose -> SDPA twice: 4 query heads over 2 K / V heads of D = 64, S = 160
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    h = m.create_tensor([2, 160, 128], DataType.DT_FLOAT, name="input")
    for i in range(2):
        q, k, v = (m.transpose(m.reshape(m.dense(h, nh * 64, name=f"{n}{i}"), [2, 160, nh, 64]), [0, 2, 1, 3])
                   for n, nh in (("q", 4), ("k", 2), ("v", 2)))
        a = m.scaled_dot_product_attention(q, k, v, causal=True, window=window, name=f"attn{i}")
        h = m.add(h, m.dense(m.reshape(m.transpose(a, [0, 2, 1, 3]), [2, 160, 256]), 128, name=f"o{i}"))
    m.softmax(m.dense(h, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    g = torch.Generator().manual_seed(0)
    for n in sorted(m.executor.parameter_names()):
        m.executor.set_parameter(n, torch.randn(m.executor.get_parameter(n).shape, generator=g) * 0.1)
    return m.executor


def test_model_graphed_step_matches_eager():
    """One eager step and two replays reach the weights of three eager steps, within test_attention_gqa_gpu.py's
    bound for this comparison: twice what the same model without the window differs by, at least 1e-5."""
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(2, 160, 128, generator=g).to(DEV), torch.randint(0, 8, (2, 160), generator=g).to(DEV)

    def diff(window):
        res = []
        for graphed in (False, True):
            ex = _model(window)
            step = ex.make_graphed_train_step({"input": x}, y, warmup=1) if graphed else ex.train_step
            for _ in range(2 if graphed else 3):
                step({"input": x}, y)
            torch.cuda.synchronize()
            res.append({n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())})
        return max(float((res[1][n] - res[0][n]).norm() / res[0][n].norm()) for n in res[0])

    d0 = diff(None)
    n0 = K.STATS["attention_window"]
    d1 = diff(64)
    assert K.STATS["attention_window"] > n0
    print(f"attn_window graphed vs eager: no window {d0:.3e}, window 64 {d1:.3e} (bound {max(2 * d0, 1e-5):.3e})")
    assert d1 <= max(2 * d0, 1e-5), (d1, d0)
