"""The one-pass attention backward (attention.hip attn_bwd_onepass_kernel:
D = 64, non-causal, Sk <= 512, no dbias): one workgroup per (batch, head)
walks the keys in at most two 256-key blocks and forms dQ, dK and dV from a
single S / P / dP / dS per tile.

Shapes: one and two key blocks, a second block that is full (512), short
(320 -> 64 keys, 160 -> ragged first block) and absent, query counts that are
one tile, an odd and an even number of tiles (the two wave groups alternate
on dQ tiles) and ragged in both the 64-row tile and the 32-row subtile, and
Sq != Sk in both directions.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 3
SHAPES = [(512, 512), (320, 320), (200, 200), (100, 100), (64, 64), (96, 512), (512, 160)]

# relative Frobenius error of a bf16 gradient against fp64 (the suite's bound
# for bf16 operators, test_kernels_gpu.py _BF_OP; 2.0-2.5e-3 measured for the
# two-kernel backward), and between two backward variants (the bound of
# test_attention_bwd_fused_delta)
_BF_OP = 5e-3
_VARIANTS = 2e-3


def _rel64(a, b):
    a = a.double()
    b = b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _ref_attn(q, k, v, causal):
    """Attention in the inputs' precision (fp64 tensors for the bounds)."""
    qf, kf, vf = (t.transpose(1, 2) for t in (q, k, v))  # [B,H,S,D]
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        Sq, Sk = s.shape[-2:]
        mask = torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ vf).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _case(Sq, Sk, D=64, causal=False, heavy_tail=False):
    """Inputs, the forward's o / lse and the fp64 gradients of one shape;
    computed once and shared (nothing below writes to them).  Self-attention
    shapes use views of one packed [B, S, 3, H, D] buffer."""
    g = torch.Generator(device=DEV).manual_seed(1000 * Sq + Sk + D + int(causal))
    if Sq == Sk:
        qkv = torch.randn(B, Sq, 3, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
        if heavy_tail:
            qkv[:, 256:, 1] *= 3
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        q = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
        kv = torch.randn(B, Sk, 2, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
        k, v = kv[:, :, 0], kv[:, :, 1]
    do = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    o, lse = K.attention_fwd(q, k, v, causal=causal)
    qf, kf, vf = (t.double().requires_grad_(True) for t in (q, k, v))
    _ref_attn(qf, kf, vf, causal).backward(do.double())
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, o=o, lse=lse, do=do, ref=(qf.grad, kf.grad, vf.grad), causal=causal)


def _grads(c, packed=None):
    """Run the backward into fresh buffers; returns (dq, dk, dv)."""
    q, k, v = c["q"], c["k"], c["v"]
    if packed is None:
        packed = q.shape[1] == k.shape[1]
    if packed:
        d = torch.empty(q.shape[0], q.shape[1], 3, q.shape[2], q.shape[3], device=DEV, dtype=torch.bfloat16)
        dq, dk, dv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    else:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    K.attention_bwd(q, k, v, c["o"], c["lse"], c["do"], dq, dk, dv, causal=c["causal"])
    torch.cuda.synchronize()
    return dq, dk, dv


def _check_fp64(c):
    n0 = K.STATS["attention_bwd_onepass"]
    got = _grads(c)
    assert K.STATS["attention_bwd_onepass"] == n0 + 1
    for name, a, r in zip(("dQ", "dK", "dV"), got, c["ref"]):
        err = _rel64(a, r)
        print(name, tuple(a.shape), f"{err:.3e}")
        assert err < _BF_OP, (name, err)


@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_onepass_against_fp64(Sq, Sk, monkeypatch):
    monkeypatch.delenv("FFK_ATTN_BWD_ONEPASS", raising=False)
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    _check_fp64(_case(Sq, Sk))


@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_onepass_against_two_kernel_backward(Sq, Sk, monkeypatch):
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    c = _case(Sq, Sk)
    monkeypatch.setenv("FFK_ATTN_BWD_ONEPASS", "0")
    n0 = K.STATS["attention_bwd_onepass"]
    old = _grads(c)
    assert K.STATS["attention_bwd_onepass"] == n0
    monkeypatch.setenv("FFK_ATTN_BWD_ONEPASS", "1")
    new = _grads(c)
    assert K.STATS["attention_bwd_onepass"] == n0 + 1
    for name, a, r in zip(("dQ", "dK", "dV"), new, old):
        err = _rel64(a, r)
        print(name, f"{err:.3e}")
        assert err < _VARIANTS, (name, err)


def test_onepass_second_key_block_carries_the_mass(monkeypatch):
    """K rows >= 256 scaled by 3: the softmax mass sits in the second key
    block, so a dropped or mis-ordered second sweep of the dQ sum shows."""
    monkeypatch.delenv("FFK_ATTN_BWD_ONEPASS", raising=False)
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    _check_fp64(_case(512, 512, heavy_tail=True))


@pytest.mark.parametrize("Sq,Sk", [(512, 512), (200, 200)])
def test_onepass_bit_reproducible(Sq, Sk, monkeypatch):
    monkeypatch.delenv("FFK_ATTN_BWD_ONEPASS", raising=False)
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    c = _case(Sq, Sk)
    n0 = K.STATS["attention_bwd_onepass"]
    a, b = _grads(c), _grads(c)
    assert K.STATS["attention_bwd_onepass"] == n0 + 2
    for name, x, y in zip(("dQ", "dK", "dV"), a, b):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("Sq,Sk", [(200, 200), (96, 512)])
def test_onepass_no_stray_writes(Sq, Sk, monkeypatch):
    """dQ / dK / dV are views into sentinel-filled buffers with one extra head
    slot and eight extra sequence rows: nothing outside the views changes."""
    monkeypatch.delenv("FFK_ATTN_BWD_ONEPASS", raising=False)
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    c = _case(Sq, Sk)
    D, sentinel = 64, -1024.0
    bufs, views, inside = [], [], []
    for S in (Sq, Sk, Sk):
        big = torch.full((B, S + 8, H + 1, D), sentinel, device=DEV, dtype=torch.bfloat16)
        m = torch.zeros(B, S + 8, H + 1, D, device=DEV, dtype=torch.bool)
        m[:, :S, :H] = True
        bufs.append(big)
        views.append(big[:, :S, :H])
        inside.append(m)
    n0 = K.STATS["attention_bwd_onepass"]
    K.attention_bwd(c["q"], c["k"], c["v"], c["o"], c["lse"], c["do"], *views)
    torch.cuda.synchronize()
    assert K.STATS["attention_bwd_onepass"] == n0 + 1
    for name, big, m, v, r in zip(("dQ", "dK", "dV"), bufs, inside, views, c["ref"]):
        assert bool((big[~m] == sentinel).all()), name
        assert _rel64(v, r) < _BF_OP, name


@pytest.mark.parametrize("Sq,Sk,D,causal", [(512, 512, 64, True), (320, 320, 128, False), (640, 640, 64, False)],
                         ids=["causal", "d128", "sk640"])
def test_onepass_falls_back(Sq, Sk, D, causal, monkeypatch):
    """Calls outside the kernel's shapes run the existing kernels whatever the
    switch says: identical bits, and the one-pass counter stands still."""
    monkeypatch.delenv("FFK_ATTN_BWD_FUSED_DELTA", raising=False)
    c = _case(Sq, Sk, D, causal)
    n0 = K.STATS["attention_bwd_onepass"]
    monkeypatch.setenv("FFK_ATTN_BWD_ONEPASS", "0")
    off = _grads(c)
    monkeypatch.setenv("FFK_ATTN_BWD_ONEPASS", "1")
    on = _grads(c)
    assert K.STATS["attention_bwd_onepass"] == n0
    for name, x, y in zip(("dQ", "dK", "dV"), on, off):
        assert torch.equal(x, y), name
