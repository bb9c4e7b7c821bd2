"""Attention dropout inside the flash kernels (attention.hip DROP
instantiations of the forward, dQ and dK/dV kernels) against the torch
reference of the mask definition (ops/attention.py attention_dropout_mask).

Shapes cross the 64-key tile, the 128-query block and the 32-row subtile
edges, D = 64 and 128, causal and not; self-attention shapes use views of one
packed [B, S, 3, H, D] buffer, the others separate strided K / V.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 2, 3
SEED = 1234
SHAPES = [(200, 200, 64, False), (200, 200, 64, True), (96, 160, 64, False), (160, 96, 128, False),
          (130, 130, 128, True)]
PS = [0.1, 0.5]

# relative Frobenius error of a bf16 result against fp64: the suite's bound
# for bf16 operators (test_kernels_gpu.py _BF_OP)
_BF_OP = 5e-3


def _rel64(a, b):
    a = a.double()
    b = b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _ref_attn(q, k, v, causal, drop=None):
    """Attention in the inputs' precision; drop = (keep mask [B,H,Sq,Sk], keep scale)."""
    qf, kf, vf = (t.transpose(1, 2) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        Sq, Sk = s.shape[-2:]
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop[0].to(p.dtype) * drop[1]
    return (p @ vf).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _inputs(Sq, Sk, D, causal):
    """q, k (randn * 0.5: no kept probability underflows), v, dO and the
    p = 0 forward; computed once and shared (nothing below writes to them)."""
    g = torch.Generator(device=DEV).manual_seed(1000 * Sq + Sk + D + int(causal))
    if Sq == Sk:
        qkv = torch.randn(B, Sq, 3, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
        qkv[:, :, :2] *= 0.5
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        q = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16, generator=g) * 0.5
        kv = torch.randn(B, Sk, 2, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
        kv[:, :, 0] *= 0.5
        k, v = kv[:, :, 0], kv[:, :, 1]
    do = torch.randn(B, Sq, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    o0, lse0 = K.attention_fwd(q, k, v, causal=causal)
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, do=do, o0=o0, lse0=lse0, causal=causal)


@functools.lru_cache(maxsize=None)
def _case(Sq, Sk, D, causal, p):
    """The dropout forward of one shape, the reference mask and the fp64
    output and gradients through the masked reference."""
    c = dict(_inputs(Sq, Sk, D, causal))
    drop = attention_dropout_mask(B, H, Sq, Sk, p, SEED, DEV)
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, dropout_p=p, seed=SEED)
    qf, kf, vf = (t.double().requires_grad_(True) for t in (c["q"], c["k"], c["v"]))
    ref = _ref_attn(qf, kf, vf, causal, drop)
    ref.backward(c["do"].double())
    torch.cuda.synchronize()
    c.update(p=p, drop=drop, o=o, lse=lse, ref_o=ref.detach(), ref=(qf.grad, kf.grad, vf.grad))
    return c


def _grads(c, **kw):
    """The backward into fresh buffers (packed for self-attention shapes); returns (path, (dq, dk, dv))."""
    q, k, v = c["q"], c["k"], c["v"]
    if q.shape[1] == k.shape[1]:
        d = torch.empty(B, q.shape[1], 3, H, q.shape[3], device=DEV, dtype=torch.bfloat16)
        dq, dk, dv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    else:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    path = K.attention_bwd(q, k, v, kw.pop("o", c.get("o", c["o0"])), kw.pop("lse", c.get("lse", c["lse0"])), c["do"],
                           dq, dk, dv, causal=c["causal"], **kw)
    torch.cuda.synchronize()
    return path, (dq, dk, dv)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_forward_mask_is_the_reference_mask(Sq, Sk, D, causal, p):
    """V = 0 except V[j D + i, h, i] = 1 for one block j of D keys: O[b, q, h, i]
    is exactly zero iff probability (q, j D + i) is dropped, masked or past Sk."""
    c = _inputs(Sq, Sk, D, causal)
    keep, _ = attention_dropout_mask(B, H, Sq, Sk, p, SEED, DEV)
    if causal:
        keep = keep & torch.ones(Sq, Sk, device=DEV, dtype=torch.bool).tril()
    got = torch.zeros(B, H, Sq, Sk, device=DEV, dtype=torch.bool)
    if Sq == Sk:   # the packed layout, with the V slot rewritten per block
        buf = torch.stack([c["q"], c["k"], torch.zeros_like(c["q"])], dim=2)
        q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
    else:
        q, k = c["q"], c["k"]
        v = torch.zeros(B, Sk, 2, H, D, device=DEV, dtype=torch.bfloat16)[:, :, 1]
    eye = torch.eye(D, device=DEV, dtype=torch.bfloat16)
    for j in range((Sk + D - 1) // D):
        n = min(D, Sk - j * D)
        v.zero_()
        v[:, j * D:j * D + n] = eye[:n].view(1, n, 1, D)
        o, _ = K.attention_fwd(q, k, v, causal=causal, dropout_p=p, seed=SEED)
        got[:, :, :, j * D:j * D + n] = (o[..., :n] != 0).permute(0, 2, 1, 3)
    torch.cuda.synchronize()
    bad = int((got != keep).sum())
    assert bad == 0, f"{bad} of {keep.numel()} mask bits differ"
    assert 0 < int((~keep).sum()) < keep.numel()


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_forward_against_fp64(Sq, Sk, D, causal, p):
    c = _case(Sq, Sk, D, causal, p)
    err = _rel64(c["o"], c["ref_o"])
    print(f"O {Sq}x{Sk} D{D} causal={causal} p={p}: {err:.3e}")
    assert err < _BF_OP, err
    assert torch.equal(c["lse"], c["lse0"]), "the LSE is that of the undropped softmax"
    assert not torch.equal(c["o"], c["o0"])


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_backward_against_fp64(Sq, Sk, D, causal, p, monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _case(Sq, Sk, D, causal, p)
    n0 = K.STATS["attention_bwd_onepass"]
    path, got = _grads(c, dropout_p=p, seed=SEED)
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0
    for name, a, r in zip(("dQ", "dK", "dV"), got, c["ref"]):
        err = _rel64(a, r)
        print(f"{name} {Sq}x{Sk} D{D} causal={causal} p={p}: {err:.3e}")
        assert err < _BF_OP, (name, err)


def test_backward_dbias_slab_with_dropout():
    """The dbias epilogues see the final accumulators: column sums of the
    returned gradients, at the bound of test_kernels_gpu.py test_attention_fwd_bwd."""
    c = _case(200, 200, 64, False, 0.1)
    dbias = [torch.full((H * 64,), 0.25, device=DEV) for _ in range(3)]
    path, got = _grads(c, dropout_p=0.1, seed=SEED, dbias=dbias)
    assert path == 0
    for i, (g, r) in enumerate(zip(got, c["ref"])):
        assert _rel64(g, r) < _BF_OP, i
        gd = g.double()
        err = (dbias[i] - 0.25 - gd.sum((0, 1)).reshape(-1)).abs().max()
        scale = gd.abs().sum((0, 1)).max()
        assert err < 3e-2 * scale, ("dbias", i, float(err), float(scale))


@pytest.mark.parametrize("Sq,Sk,D,causal", [(200, 200, 64, False), (130, 130, 128, True), (96, 160, 64, False)])
def test_unchanged_when_off(Sq, Sk, D, causal, monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(Sq, Sk, D, causal)
    n0 = K.STATS["attention_dropout"]
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, dropout_p=0.0, seed=SEED)
    assert torch.equal(o, c["o0"]) and torch.equal(lse, c["lse0"])
    pa, a = _grads(c)
    pb, b = _grads(c, dropout_p=0.0, seed=SEED)
    assert pa == pb and K.STATS["attention_dropout"] == n0
    for name, x, y in zip(("dQ", "dK", "dV"), a, b):
        assert torch.equal(x, y), name


def test_bert_shape_keeps_the_onepass_backward_when_off(monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(512, 512, 64, False)
    n0 = K.STATS["attention_bwd_onepass"]
    path, _ = _grads(c, dropout_p=0.0)
    assert path == 1 and K.STATS["attention_bwd_onepass"] == n0 + 1
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], dropout_p=0.1, seed=SEED)
    path, _ = _grads(c, o=o, lse=lse, dropout_p=0.1, seed=SEED)
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0 + 1


def _fwd_bwd(c, **kw):
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=c["causal"], **kw)
    _, g = _grads(c, o=o, lse=lse, **kw)
    return (o, lse) + g


def test_seeds():
    c = _inputs(96, 160, 64, False)
    a = _fwd_bwd(c, dropout_p=0.1, seed=SEED)
    b = _fwd_bwd(c, dropout_p=0.1, seed=SEED)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    word = torch.tensor([7], device=DEV, dtype=torch.int64)
    d = _fwd_bwd(c, dropout_p=0.1, seed=SEED - 7, seed_dev=word)
    for x, y in zip(a, d):
        assert torch.equal(x, y), "seed = s, seed_dev = [c] is seed = s + c"
    e = _fwd_bwd(c, dropout_p=0.1, seed=SEED + 1)
    assert torch.equal(a[1], e[1])     # the LSE does not see the mask
    for x, y in zip(a[:1] + a[2:], e[:1] + e[2:]):
        assert not torch.equal(x, y)


def test_graph_replay_follows_the_device_seed():
    c = _inputs(200, 200, 64, True)
    word = torch.zeros(1, device=DEV, dtype=torch.int64)

    def run():
        return _fwd_bwd_nosync(c, word)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held = run()
    replays = []
    for n in (1, 2):
        word.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in held])
        want = _fwd_bwd(c, dropout_p=0.1, seed=SEED, seed_dev=torch.tensor([n], device=DEV, dtype=torch.int64))
        for x, y in zip(replays[-1], want):
            assert torch.equal(x, y), n
    for i in (0, 2, 3, 4):
        assert not torch.equal(replays[0][i], replays[1][i])


def _fwd_bwd_nosync(c, word):
    """_fwd_bwd without the host synchronisation (capturable)."""
    q, k, v = c["q"], c["k"], c["v"]
    kw = dict(causal=c["causal"], dropout_p=0.1, seed=SEED, seed_dev=word)
    o, lse = K.attention_fwd(q, k, v, **kw)
    d = torch.empty(B, q.shape[1], 3, H, q.shape[3], device=DEV, dtype=torch.bfloat16)
    K.attention_bwd(q, k, v, o, lse, c["do"], d[:, :, 0], d[:, :, 1], d[:, :, 2], **kw)
    return o, lse, d[:, :, 0], d[:, :, 1], d[:, :, 2]


def _classifier(dropout):
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    a = m.multihead_attention(x, x, x, 128, 2, dropout=dropout, name="mha")
    m.softmax(m.dense(a, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    return ex


def test_model_graphed_step_matches_eager():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 8, (4, 64), generator=g).to(DEV)

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(dropout):
        ex = _classifier(dropout)
        for _ in range(3):
            ex.train_step({"input": x}, y)
        return params(ex)

    def graphed(dropout):
        ex = _classifier(dropout)
        step = ex.make_graphed_train_step({"input": x}, y, warmup=1)   # one eager step, then two replays
        step()
        step()
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    plain = eager(0.0)
    d0 = worst(graphed(0.0), plain)          # graphed against eager without dropout sets the bound
    bound = max(2 * d0, 1e-5)
    n0 = K.STATS["attention_dropout"]
    want = eager(0.1)
    assert K.STATS["attention_dropout"] == n0 + 6     # three forwards and three backwards
    d1 = worst(graphed(0.1), want)
    apart = worst(want, plain)
    print(f"graphed vs eager: dropout 0.0 {d0:.3e}, dropout 0.1 {d1:.3e} (bound {bound:.3e}); "
          f"dropout 0.1 vs 0.0 weights {apart:.3e}")
    assert d1 <= bound, (d1, bound)
    assert apart >= 100 * bound, (apart, bound)


def test_argument_errors():
    c = _inputs(96, 160, 64, False)
    q, k, v = c["q"], c["k"], c["v"]
    for p in (1.0, 1.5):
        with pytest.raises(ValueError):
            K.attention_fwd(q, k, v, dropout_p=p)
    bad_words = [torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
                 torch.zeros(2, device=DEV, dtype=torch.int64)]
    for word in bad_words:
        with pytest.raises(ValueError):
            K.attention_fwd(q, k, v, dropout_p=0.1, seed_dev=word)
        with pytest.raises(ValueError):
            _grads(c, dropout_p=0.1, seed_dev=word)
    # Sq * Sk = 2^32: refused on the shapes, before any launch (q / k / v are 8 MB each)
    big = torch.empty(1, 1 << 16, 1, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.attention_fwd(big, big, big, dropout_p=0.1)
