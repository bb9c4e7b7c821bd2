"""Per-sample key lengths in the flash kernels (attention.hip VARLEN
instantiations of the forward, dQ and dK/dV kernels): keys at or past
kv_lens[b] do not exist for sample b.

Shapes cross the 64-key tile, the 128-key block and the 32-row subtile, D = 64
and 128, causal and not; self-attention shapes use views of one packed
[B, S, 3, H, D] buffer, the others separate strided K / V.  The lengths of a
shape are Sk, one just past a tile edge (129 or 65), one exact tile edge (64)
and 1.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 4, 3
SEED = 1234
SHAPES = [(200, 200, 64, False), (200, 200, 64, True), (96, 160, 64, False), (160, 96, 128, False),
          (130, 130, 128, True)]
PS = [0.0, 0.1]

# relative Frobenius error of a bf16 result against fp64: the suite's bound
# for bf16 operators (test_kernels_gpu.py _BF_OP)
_BF_OP = 5e-3
# the LSE (fp32, log2 domain) against fp64: the suite's tolerance for an LSE
# (test_kernels_gpu.py test_attention_strided_views); the kernel's scores are
# fp32 MFMA sums of bf16 products and its exp2 / log2 are the 1-ulp hardware
# approximations, orders of magnitude inside it
_LSE_TOL = dict(rtol=1e-4, atol=1e-3)


def _lens_of(Sk):
    return [Sk, 129 if Sk > 129 else 65, 64, 1]


def _dev_lens(vals):
    return torch.tensor(vals, device=DEV, dtype=torch.int32)


def _rel64(a, b):
    a = a.double()
    b = b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _dead(lens, Sk):
    """[B, Sk] bool: key k does not exist for sample b."""
    return torch.arange(Sk, device=DEV).view(1, Sk) >= lens.view(-1, 1)


def _ref_attn(q, k, v, causal, lens, drop=None):
    """Masked attention in the inputs' precision (every row needs a live
    key); returns (o, lse in the log2 domain)."""
    qf, kf, vf = (t.transpose(1, 2) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    Sq, Sk = s.shape[-2:]
    s = s.masked_fill(_dead(lens, Sk)[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop[0].to(p.dtype) * drop[1]
    return (p @ vf).transpose(1, 2), torch.logsumexp(s, -1) * math.log2(math.e)


@functools.lru_cache(maxsize=None)
def _inputs(Sq, Sk, D, causal):
    """q, k (randn * 0.5), v, dO, the lengths and the forward without lengths;
    computed once and shared (nothing below writes to them)."""
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
    return dict(q=q, k=k, v=v, do=do, o0=o0, lse0=lse0, causal=causal, lens=_dev_lens(_lens_of(Sk)))


def _drop_kw(p):
    return dict(dropout_p=p, seed=SEED) if p else {}


@functools.lru_cache(maxsize=None)
def _case(Sq, Sk, D, causal, p):
    """The forward of one shape with lengths (and dropout p) and the fp64
    output, LSE and gradients through the masked reference."""
    c = dict(_inputs(Sq, Sk, D, causal))
    drop = attention_dropout_mask(B, H, Sq, Sk, p, SEED, DEV) if p else None
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=c["lens"], **_drop_kw(p))
    qf, kf, vf = (t.double().requires_grad_(True) for t in (c["q"], c["k"], c["v"]))
    ref, ref_lse = _ref_attn(qf, kf, vf, causal, c["lens"], drop)
    ref.backward(c["do"].double())
    torch.cuda.synchronize()
    c.update(p=p, o=o, lse=lse, ref_o=ref.detach(), ref_lse=ref_lse.detach(), ref=(qf.grad, kf.grad, vf.grad))
    return c


def _grads(c, q=None, k=None, v=None, fill=None, **kw):
    """The backward into fresh buffers (packed for self-attention shapes,
    pre-filled with `fill` if given); returns (path, (dq, dk, dv))."""
    q = c["q"] if q is None else q
    k = c["k"] if k is None else k
    v = c["v"] if v is None else v
    if q.shape[1] == k.shape[1]:
        d = torch.empty(B, q.shape[1], 3, H, q.shape[3], device=DEV, dtype=torch.bfloat16)
        dq, dk, dv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    else:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if fill is not None:
        for t in (dq, dk, dv):
            t.fill_(fill)
    path = K.attention_bwd(q, k, v, kw.pop("o", c.get("o", c["o0"])), kw.pop("lse", c.get("lse", c["lse0"])), c["do"],
                           dq, dk, dv, causal=c["causal"], **kw)
    torch.cuda.synchronize()
    return path, (dq, dk, dv)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_forward_against_fp64(Sq, Sk, D, causal, p):
    c = _case(Sq, Sk, D, causal, p)
    err = _rel64(c["o"], c["ref_o"])
    worst = (c["lse"].double() - c["ref_lse"]).abs().max().item()
    print(f"O {Sq}x{Sk} D{D} causal={causal} p={p}: {err:.3e}; LSE max abs {worst:.3e}")
    assert err < _BF_OP, err
    assert torch.allclose(c["lse"].double(), c["ref_lse"], **_LSE_TOL), worst
    assert not torch.equal(c["o"], c["o0"])


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_backward_against_fp64(Sq, Sk, D, causal, p, monkeypatch):
    """dQ, dK and dV against fp64 through the same mask, at the suite's bf16
    bound over the whole tensor.  The sample of length 1 is the hard one at
    p = 0.1: its only probability is 1, so its exact dQ and dK are zero, while
    its O = rs V[0] is rounded to bf16.  A backward that takes delta from
    rowsum(dO * O) turns that rounding into dS (6e-3 to 1.1e-2 over the whole
    tensor); the kernels with lengths and dropout take delta from the
    probabilities and are at 2.3e-3 to 2.4e-3, as at p = 0."""
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _case(Sq, Sk, D, causal, p)
    n0, v0 = K.STATS["attention_bwd_onepass"], K.STATS["attention_varlen"]
    path, got = _grads(c, kv_lens=c["lens"], **_drop_kw(p))
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0 and K.STATS["attention_varlen"] == v0 + 1
    for name, a, r in zip(("dQ", "dK", "dV"), got, c["ref"]):
        err = _rel64(a, r)
        print(f"{name} {Sq}x{Sk} D{D} causal={causal} p={p}: {err:.3e}")
        assert err < _BF_OP, (name, err)


def _padded(c, value):
    """Copies of q / k / v (same layout) whose K and V rows past each
    sample's length hold `value`."""
    q, k, v = c["q"], c["k"], c["v"]
    Sk = k.shape[1]
    dead = _dead(c["lens"], Sk)[:, :, None, None]
    if q.shape[1] == Sk:
        buf = torch.stack([q, k, v], dim=2)
        q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
    else:
        buf = torch.stack([k, v], dim=2)
        k, v = buf[:, :, 0], buf[:, :, 1]
    k.masked_fill_(dead, value)
    v.masked_fill_(dead, value)
    return q, k, v


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_padding_cannot_leak(Sq, Sk, D, causal, p):
    """NaN against zeros in the K / V rows past each length, and in the
    gradient buffers before the call: the same bits come out, all finite, and
    dK = dV = 0 past the length."""
    c = _inputs(Sq, Sk, D, causal)
    runs = []
    for value in (float("nan"), 0.0):
        q, k, v = _padded(c, value)
        kw = dict(kv_lens=c["lens"], **_drop_kw(p))
        o, lse = K.attention_fwd(q, k, v, causal=causal, **kw)
        _, g = _grads(c, q, k, v, fill=value, o=o, lse=lse, **kw)
        runs.append((o, lse) + g)
    for name, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), *runs):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name
    dead = _dead(c["lens"], Sk)
    for name, g in (("dK", runs[0][3]), ("dV", runs[0][4])):
        assert int(dead.sum()) > 0 and (g[dead] == 0).all(), name
        assert (g[~dead] != 0).any(), name


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", [(200, 200, 64, False), (200, 200, 64, True), (130, 130, 128, True),
                                            (160, 96, 128, False)])
def test_rows_without_a_live_key(Sq, Sk, D, causal, p):
    """A sample of length 0 (causal or not: with the causal rule key <= query
    every row of a sample with keys sees key 0, so a length of 0 is the causal
    case whose rows see nothing): o = 0, lse = -inf, dQ = 0, and its dK / dV
    are 0; NaN nowhere, although the padding is NaN."""
    c = dict(_inputs(Sq, Sk, D, causal))
    c["lens"] = _dev_lens([Sk, 0, 65, 0])
    q, k, v = _padded(c, float("nan"))
    kw = dict(kv_lens=c["lens"], **_drop_kw(p))
    o, lse = K.attention_fwd(q, k, v, causal=causal, **kw)
    _, (dq, dk, dv) = _grads(c, q, k, v, fill=float("nan"), o=o, lse=lse, **kw)
    for b in (1, 3):
        assert (o[b] == 0).all() and (lse[b] == float("-inf")).all()
        assert (dq[b] == 0).all() and (dk[b] == 0).all() and (dv[b] == 0).all()
    for b in (0, 2):
        assert torch.isfinite(lse[b]).all() and (o[b] != 0).any() and (dq[b] != 0).any()
    for name, t in (("O", o), ("dQ", dq), ("dK", dk), ("dV", dv)):
        assert torch.isfinite(t).all(), name
    assert not torch.isnan(lse).any()
    # the samples with keys do not see their neighbours' lengths
    c["lens"] = _dev_lens([Sk, Sk, 65, 1])
    o2, lse2 = K.attention_fwd(q, k, v, causal=causal, **dict(kw, kv_lens=c["lens"]))
    for b in (0, 2):
        assert torch.equal(o[b], o2[b]) and torch.equal(lse[b], lse2[b])


@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_full_lengths_are_the_call_without_lengths(Sq, Sk, D, causal):
    c = _inputs(Sq, Sk, D, causal)
    full = _dev_lens([Sk] * B)
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=full)
    assert torch.equal(o, c["o0"]) and torch.equal(lse, c["lse0"])
    # values past Sk are clamped to Sk by the kernels
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=_dev_lens([Sk + 1, 1 << 30, Sk, Sk]))
    assert torch.equal(o, c["o0"]) and torch.equal(lse, c["lse0"])


@pytest.mark.parametrize("Sq,Sk,D,causal", [(200, 200, 64, False), (130, 130, 128, True), (96, 160, 64, False)])
def test_unchanged_when_off(Sq, Sk, D, causal, monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(Sq, Sk, D, causal)
    n0 = K.STATS["attention_varlen"]
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=None)
    assert torch.equal(o, c["o0"]) and torch.equal(lse, c["lse0"])
    pa, a = _grads(c)
    pb, b = _grads(c, kv_lens=None)
    assert pa == pb and K.STATS["attention_varlen"] == n0
    for name, x, y in zip(("dQ", "dK", "dV"), a, b):
        assert torch.equal(x, y), name


def test_bert_shape_keeps_the_onepass_backward_when_off(monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(512, 512, 64, False)
    n0 = K.STATS["attention_bwd_onepass"]
    path, _ = _grads(c, kv_lens=None)
    assert path == 1 and K.STATS["attention_bwd_onepass"] == n0 + 1
    lens = _dev_lens([512, 300, 64, 1])
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], kv_lens=lens)
    path, (_, dk, _) = _grads(c, o=o, lse=lse, kv_lens=lens)
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0 + 1
    assert (dk[1, 300:] == 0).all() and (dk[1, :300] != 0).any()


@pytest.mark.parametrize("p", PS)
def test_backward_dbias_slab_with_lengths(p):
    """The dbias epilogues see the final accumulators, and the key blocks past
    a length write zero partials into every slab row: column sums of the
    returned gradients, at the bound of test_attention_dropout_gpu.py
    test_backward_dbias_slab_with_dropout."""
    c = _case(200, 200, 64, False, p)
    dbias = [torch.full((H * 64,), 0.25, device=DEV) for _ in range(3)]
    path, got = _grads(c, kv_lens=c["lens"], dbias=dbias, **_drop_kw(p))
    assert path == 0
    for i, g in enumerate(got):   # the column sums first: they are what this test adds
        gd = g.double()
        err = (dbias[i] - 0.25 - gd.sum((0, 1)).reshape(-1)).abs().max()
        scale = gd.abs().sum((0, 1)).max()
        print(f"dbias {i} p={p}: {float(err):.3e} of {float(scale):.3e}")
        assert err < 3e-2 * scale, ("dbias", i, float(err), float(scale))
    for i, (g, r) in enumerate(zip(got, c["ref"])):
        assert _rel64(g, r) < _BF_OP, i


def _fwd_bwd(c, lens, sync=True):
    q, k, v = c["q"], c["k"], c["v"]
    kw = dict(causal=c["causal"], dropout_p=0.1, seed=SEED, kv_lens=lens)
    o, lse = K.attention_fwd(q, k, v, **kw)
    d = torch.empty(B, q.shape[1], 3, H, q.shape[3], device=DEV, dtype=torch.bfloat16)
    K.attention_bwd(q, k, v, o, lse, c["do"], d[:, :, 0], d[:, :, 1], d[:, :, 2], **kw)
    if sync:
        torch.cuda.synchronize()
    return o, lse, d[:, :, 0], d[:, :, 1], d[:, :, 2]


def test_graph_replay_follows_the_lengths_tensor():
    c = _inputs(200, 200, 64, True)
    lens = _dev_lens([200, 200, 200, 200])

    def run():
        return _fwd_bwd(c, lens, sync=False)

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
    for vals in ([200, 129, 64, 1], [17, 200, 0, 65]):
        lens.copy_(_dev_lens(vals))
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in held])
        want = _fwd_bwd(c, _dev_lens(vals))
        for x, y in zip(replays[-1], want):
            assert torch.equal(x, y), vals
    for i in range(5):
        assert not torch.equal(replays[0][i], replays[1][i])


def _classifier(key_lengths):
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    lens = m.create_tensor([4], DataType.DT_INT32, create_grad=False, name="lens") if key_lengths else None
    a = m.multihead_attention(x, x, x, 128, 2, name="mha", key_lengths=lens)
    m.softmax(m.dense(a, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    return ex


def test_model_graphed_step_matches_eager():
    """The classifier of test_attention_dropout_gpu.py with a key_lengths
    input and another lengths batch on every step: the captured step reads the
    lengths of the batch it is fed."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 8, (4, 64), generator=g).to(DEV)
    batches = [_dev_lens(v) for v in ([64, 33, 5, 17], [1, 64, 40, 9], [20, 2, 64, 50])]

    def feeds(i, on):
        return {"input": x, "lens": batches[i]} if on else {"input": x}

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(on):
        ex = _classifier(on)
        for i in range(3):
            ex.train_step(feeds(i, on), y)
        return params(ex)

    def graphed(on):
        ex = _classifier(on)
        step = ex.make_graphed_train_step(feeds(0, on), y, warmup=1)   # one eager step, then two replays
        step(feeds(1, on), y)
        step(feeds(2, on), y)
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    plain = eager(False)
    d0 = worst(graphed(False), plain)        # graphed against eager without lengths sets the bound
    bound = max(2 * d0, 1e-5)
    n0 = K.STATS["attention_varlen"]
    want = eager(True)
    assert K.STATS["attention_varlen"] == n0 + 6     # three forwards and three backwards
    d1 = worst(graphed(True), want)
    apart = worst(want, plain)
    print(f"graphed vs eager: no lengths {d0:.3e}, lengths {d1:.3e} (bound {bound:.3e}); "
          f"lengths vs none weights {apart:.3e}")
    assert d1 <= bound, (d1, bound)
    assert apart >= 100 * bound, (apart, bound)


def test_argument_errors():
    c = _inputs(96, 160, 64, False)
    q, k, v = c["q"], c["k"], c["v"]
    bad = [torch.ones(B, device=DEV, dtype=torch.int64),            # dtype
           torch.ones(B, device=DEV, dtype=torch.float32),
           torch.ones(B + 1, device=DEV, dtype=torch.int32),        # shape
           torch.ones(B, 1, device=DEV, dtype=torch.int32),
           torch.ones(B, dtype=torch.int32),                        # device
           torch.ones(2 * B, device=DEV, dtype=torch.int32)[::2],   # not contiguous
           [160] * B]                                               # not a tensor
    n0 = K.STATS["attention_fwd"]
    for lens in bad:
        with pytest.raises(ValueError):
            K.attention_fwd(q, k, v, kv_lens=lens)
        with pytest.raises(ValueError):
            _grads(c, kv_lens=lens)
    assert K.STATS["attention_fwd"] == n0
