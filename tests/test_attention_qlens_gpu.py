"""Per-sample query lengths in the flash kernels (the VARLEN instantiations of
the forward, dQ and dK/dV kernels of attention.hip): queries at or past
q_lens[b] do not exist for sample b, with or without key lengths.

The shapes, inputs and key lengths are those of test_attention_varlen_gpu.py.
The query lengths of a shape are Sq, one just past a 128-row block or a
64-row tile (129 or 65), one exact tile edge (64) and 1: a dead block, a dead
wave in a live block and dead rows in a live wave all occur.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask
from test_attention_varlen_gpu import (_BF_OP, _LSE_TOL, B, DEV, H, PS, SEED, SHAPES, _dead, _dev_lens, _drop_kw, _grads,
                                       _inputs, _lens_of, _rel64)

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _qlens_of(Sq):
    return [Sq, 129 if Sq > 129 else 65, 64, 1]


def _ref_attn2(q, k, v, causal, klens, qlens, drop=None):
    """Attention through the two-axis mask in the inputs' precision: dead keys
    get probability 0, dead query rows o = 0 (and no gradient).  Returns
    (o, lse in the log2 domain, valid on the live rows)."""
    Sq, Sk = q.shape[1], k.shape[1]
    qdead = _dead(qlens, Sq)
    qf, kf, vf = (t.transpose(1, 2) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    s = s.masked_fill(_dead(klens, Sk)[:, None, None, :], NEG_INF)
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device, dtype=torch.bool).triu(1), NEG_INF)
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop[0].to(p.dtype) * drop[1]
    o = (p @ vf).masked_fill(qdead[:, None, :, None], 0.0)
    return o.transpose(1, 2), torch.logsumexp(s, -1) * math.log2(math.e)


@functools.lru_cache(maxsize=None)
def _case(Sq, Sk, D, causal, p, keys):
    """One shape with query lengths (and key lengths if `keys`): the kernels'
    forward and the fp64 output, LSE and gradients through the mask."""
    c = dict(_inputs(Sq, Sk, D, causal))
    c["qlens"] = _dev_lens(_qlens_of(Sq))
    c["klens"] = c["lens"] if keys else None
    drop = attention_dropout_mask(B, H, Sq, Sk, p, SEED, DEV) if p else None
    n0 = K.STATS["attention_qlens"]
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=c["klens"], q_lens=c["qlens"], **_drop_kw(p))
    assert K.STATS["attention_qlens"] == n0 + 1
    qf, kf, vf = (t.double().requires_grad_(True) for t in (c["q"], c["k"], c["v"]))
    ref, ref_lse = _ref_attn2(qf, kf, vf, causal, c["lens"] if keys else _dev_lens([Sk] * B), c["qlens"], drop)
    ref.backward(c["do"].double())
    torch.cuda.synchronize()
    c.update(p=p, o=o, lse=lse, ref_o=ref.detach(), ref_lse=ref_lse.detach(), ref=(qf.grad, kf.grad, vf.grad))
    return c


def _kw(c, p=0.0):
    return dict(kv_lens=c["klens"], q_lens=c["qlens"], **_drop_kw(p))


# ------------------------------------------------------------- 1. fp64 check
@pytest.mark.parametrize("keys", [True, False], ids=["both", "q_only"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_forward_against_fp64(Sq, Sk, D, causal, p, keys):
    c = _case(Sq, Sk, D, causal, p, keys)
    qdead = _dead(c["qlens"], Sq)
    assert int(qdead.sum()) > 0
    assert (c["o"][qdead] == 0).all(), "dead rows of o are exactly zero"
    assert (c["lse"].transpose(1, 2)[qdead] == NEG_INF).all(), "dead rows have lse = -inf"
    # the dead rows are zero on both sides: the norms are those of the live rows
    err = _rel64(c["o"], c["ref_o"])
    live = ~qdead[:, None, :].expand(B, H, Sq)
    got, want = c["lse"].double()[live], c["ref_lse"][live]
    worst = (got - want).abs().max().item()
    print(f"O {Sq}x{Sk} D{D} causal={causal} p={p} keys={keys}: {err:.3e}; LSE max abs {worst:.3e}")
    assert err < _BF_OP, err
    assert torch.allclose(got, want, **_LSE_TOL), worst


@pytest.mark.parametrize("keys", [True, False], ids=["both", "q_only"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_backward_against_fp64(Sq, Sk, D, causal, p, keys, monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _case(Sq, Sk, D, causal, p, keys)
    n0, q0, v0 = K.STATS["attention_bwd_onepass"], K.STATS["attention_qlens"], K.STATS["attention_varlen"]
    path, got = _grads(c, fill=float("nan"), **_kw(c, p))
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0 and K.STATS["attention_qlens"] == q0 + 1
    assert K.STATS["attention_varlen"] == v0 + int(keys), "attention_varlen counts the calls with key lengths"
    assert (got[0][_dead(c["qlens"], Sq)] == 0).all(), "dead rows of dQ are exactly zero"
    if keys:
        kdead = _dead(c["lens"], Sk)
        assert (got[1][kdead] == 0).all() and (got[2][kdead] == 0).all()
    for name, a, r in zip(("dQ", "dK", "dV"), got, c["ref"]):
        assert torch.isfinite(a).all(), name
        err = _rel64(a, r)
        print(f"{name} {Sq}x{Sk} D{D} causal={causal} p={p} keys={keys}: {err:.3e}")
        assert err < _BF_OP, (name, err)


# --------------------------------------------------- 2. padding cannot leak
def _dirty(c, value):
    """Copies of q / k / v / dO (same layout) whose dead query rows (q, dO) and
    dead key rows (k, v) hold `value`."""
    q, k, v = c["q"], c["k"], c["v"]
    Sq, Sk = q.shape[1], k.shape[1]
    qdead = _dead(c["qlens"], Sq)[:, :, None, None]
    kdead = _dead(c["lens"], Sk)[:, :, None, None]
    if Sq == Sk:
        buf = torch.stack([q, k, v], dim=2)
        q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
    else:
        q = q.clone()
        buf = torch.stack([k, v], dim=2)
        k, v = buf[:, :, 0], buf[:, :, 1]
    q.masked_fill_(qdead, value)
    k.masked_fill_(kdead, value)
    v.masked_fill_(kdead, value)
    return q, k, v, c["do"].clone().masked_fill_(qdead, value)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_padding_cannot_leak(Sq, Sk, D, causal, p):
    """NaN against zeros in the dead rows of Q, O, dO and of the LSE handed to
    the backward, in the dead rows of K / V, and in the output and gradient
    buffers before the calls: the same bits come out, with no NaN."""
    c = dict(_inputs(Sq, Sk, D, causal))
    c.update(qlens=_dev_lens(_qlens_of(Sq)), klens=c["lens"])
    qdead = _dead(c["qlens"], Sq)
    runs = []
    for value in (float("nan"), 0.0):
        q, k, v, do = _dirty(c, value)
        out = torch.full((B, Sq, H, D), value, device=DEV, dtype=torch.bfloat16)
        o, lse = K.attention_fwd(q, k, v, causal=causal, out=out, **_kw(c, p))
        o_in = o.clone().masked_fill_(qdead[:, :, None, None], value)
        lse_in = lse.clone().masked_fill_(qdead[:, None, :], value)
        _, g = _grads(dict(c, do=do), q, k, v, fill=value, o=o_in, lse=lse_in, **_kw(c, p))
        runs.append((o, lse) + g)
    for name, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), *runs):
        assert not torch.isnan(a).any(), name
        assert name == "LSE" or torch.isfinite(a).all(), name
        assert torch.equal(a, b), name
    o, lse, dq, dk, dv = runs[0]
    assert (o[qdead] == 0).all() and (dq[qdead] == 0).all() and (lse.transpose(1, 2)[qdead] == NEG_INF).all()
    assert torch.isfinite(lse.transpose(1, 2)[~qdead]).all()
    kdead = _dead(c["lens"], Sk)
    assert (dk[kdead] == 0).all() and (dv[kdead] == 0).all() and (dk[~kdead] != 0).any() and (dv[~kdead] != 0).any()


# ----------------------------------------------------------- 3. edge lengths
@pytest.mark.parametrize("keys", [True, False], ids=["both", "q_only"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_edge_lengths(Sq, Sk, D, causal, p, keys):
    """[33, 0, 128, 97]: one row past a wave, no live query at all, a whole
    block, one row past three waves (clamped to Sq where Sq is shorter)."""
    c = dict(_inputs(Sq, Sk, D, causal))
    c["klens"] = c["lens"] if keys else None

    def run(vals):
        c["qlens"] = _dev_lens(vals)
        o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, **_kw(c, p))
        _, g = _grads(c, fill=float("nan"), o=o, lse=lse, **_kw(c, p))
        return (o, lse) + g

    o, lse, dq, dk, dv = first = run([33, 0, 128, 97])
    for name, t in (("o", o), ("dQ", dq), ("dK", dk), ("dV", dv)):
        assert (t[1] == 0).all(), f"{name} of the sample with no live query"
        assert torch.isfinite(t).all(), name
        assert (t[0] != 0).any() and (t[2] != 0).any(), name
    assert (lse[1] == NEG_INF).all() and not torch.isnan(lse).any()
    for b, n in ((0, 33), (2, min(128, Sq)), (3, min(97, Sq))):
        assert (o[b, n:] == 0).all() and (dq[b, n:] == 0).all() and (lse[b, :, n:] == NEG_INF).all()
        assert torch.isfinite(lse[b, :, :n]).all()
    # another length for sample 1 (now partly live) and for sample 3: samples 0 and 2 keep their bits
    second = run([33, 70, 128, 1])
    for name, a, b2 in zip(("O", "LSE", "dQ", "dK", "dV"), first, second):
        for b in (0, 2):
            assert torch.equal(a[b], b2[b]), (name, b)
    assert (second[0][1, :70] != 0).any() and (second[4][1] != 0).any()


# ----------------------------------------------------------- 4. full lengths
@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
def test_full_lengths_are_the_call_without_query_lengths(Sq, Sk, D, causal):
    c = dict(_inputs(Sq, Sk, D, causal))
    q, k, v = c["q"], c["k"], c["v"]
    full = _dev_lens([Sq] * B)
    # alone: the forward without any lengths
    for vals in ([Sq] * B, [Sq + 1, 1 << 30, Sq, Sq]):
        o, lse = K.attention_fwd(q, k, v, causal=causal, q_lens=_dev_lens(vals))
        assert torch.equal(o, c["o0"]) and torch.equal(lse, c["lse0"]), vals
    # next to key lengths: the same call without q_lens, forward and backward
    o1, lse1 = K.attention_fwd(q, k, v, causal=causal, kv_lens=c["lens"])
    _, g1 = _grads(c, o=o1, lse=lse1, kv_lens=c["lens"])
    for vals in ([Sq] * B, [Sq + 7, 1 << 30, Sq, Sq]):
        o2, lse2 = K.attention_fwd(q, k, v, causal=causal, kv_lens=c["lens"], q_lens=_dev_lens(vals))
        assert torch.equal(o1, o2) and torch.equal(lse1, lse2), vals
        _, g2 = _grads(c, o=o2, lse=lse2, kv_lens=c["lens"], q_lens=_dev_lens(vals))
        for name, x, y in zip(("dQ", "dK", "dV"), g1, g2):
            assert torch.equal(x, y), (name, vals)
    # full query lengths alone against full key lengths alone: the same kernels, either pointer null
    _, ga = _grads(c, q_lens=full)
    _, gb = _grads(c, kv_lens=_dev_lens([Sk] * B))
    for name, x, y in zip(("dQ", "dK", "dV"), ga, gb):
        assert torch.equal(x, y), name
    # negative values are clamped to 0
    runs = []
    for vals in ([-5, Sq, -(1 << 31), 64], [0, Sq, 0, 64]):
        o, lse = K.attention_fwd(q, k, v, causal=causal, q_lens=_dev_lens(vals))
        _, g = _grads(c, o=o, lse=lse, q_lens=_dev_lens(vals))
        runs.append((o, lse) + g)
    for a, b2 in zip(*runs):
        assert torch.equal(a, b2)
    assert (runs[0][0][0] == 0).all() and (runs[0][1][2] == NEG_INF).all()


# ------------------------------------------------------ 5. unchanged when off
@pytest.mark.parametrize("Sq,Sk,D,causal", [(200, 200, 64, False), (130, 130, 128, True), (96, 160, 64, False)])
def test_unchanged_when_off(Sq, Sk, D, causal, monkeypatch):
    """q_lens=None next to key lengths: the key-lengths call (dead keys as the
    key-lengths tests define them), no count, and the bits of the call whose
    query lengths are all Sq."""
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(Sq, Sk, D, causal)
    n0, v0 = K.STATS["attention_qlens"], K.STATS["attention_varlen"]
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=c["lens"], q_lens=None)
    path, (dq, dk, dv) = _grads(c, o=o, lse=lse, kv_lens=c["lens"], q_lens=None)
    assert path == 0 and K.STATS["attention_qlens"] == n0 and K.STATS["attention_varlen"] == v0 + 2
    kdead = _dead(c["lens"], Sk)
    assert (dk[kdead] == 0).all() and (dv[kdead] == 0).all() and torch.isfinite(lse).all() and (dq != 0).any()
    o2, lse2 = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=c["lens"], q_lens=_dev_lens([Sq] * B))
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    # and no lengths at all: the call as it was
    o3, lse3 = K.attention_fwd(c["q"], c["k"], c["v"], causal=causal, kv_lens=None, q_lens=None)
    assert torch.equal(o3, c["o0"]) and torch.equal(lse3, c["lse0"]) and K.STATS["attention_qlens"] == n0 + 1


def test_bert_shape_keeps_the_onepass_backward_when_off(monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    c = _inputs(512, 512, 64, False)
    n0 = K.STATS["attention_bwd_onepass"]
    path, _ = _grads(c, kv_lens=None, q_lens=None)
    assert path == 1 and K.STATS["attention_bwd_onepass"] == n0 + 1
    qlens = _dev_lens([512, 300, 64, 1])
    o, lse = K.attention_fwd(c["q"], c["k"], c["v"], q_lens=qlens)
    path, (dq, _, _) = _grads(c, o=o, lse=lse, q_lens=qlens)
    assert path == 0 and K.STATS["attention_bwd_onepass"] == n0 + 1
    assert (dq[1, 300:] == 0).all() and (dq[1, :300] != 0).any()


# -------------------------------------------------------------- 6. dbias slab
@pytest.mark.parametrize("p", PS)
def test_backward_dbias_slab_with_both_lengths(p):
    """The dbias partials of dead 32-row query pieces (whole dead blocks
    included) are written as zeros: column sums of the returned gradients, at
    the bound of test_attention_varlen_gpu.py test_backward_dbias_slab_with_lengths."""
    c = _case(200, 200, 64, False, p, True)
    dbias = [torch.full((H * 64,), 0.25, device=DEV) for _ in range(3)]
    path, got = _grads(c, dbias=dbias, **_kw(c, p))
    assert path == 0
    for i, g in enumerate(got):
        gd = g.double()
        err = (dbias[i] - 0.25 - gd.sum((0, 1)).reshape(-1)).abs().max()
        scale = gd.abs().sum((0, 1)).max()
        print(f"dbias {i} p={p}: {float(err):.3e} of {float(scale):.3e}")
        assert err < 3e-2 * scale, ("dbias", i, float(err), float(scale))
    for i, (g, r) in enumerate(zip(got, c["ref"])):
        assert _rel64(g, r) < _BF_OP, i


# ------------------------------------------------------------ 7. graph replay
def _fwd_bwd(c, lens, sync=True):
    q, k, v = c["q"], c["k"], c["v"]
    kw = dict(causal=c["causal"], dropout_p=0.1, seed=SEED, kv_lens=lens, q_lens=lens)
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
    assert (replays[1][0][2] == 0).all() and (replays[0][0][3, 1:] == 0).all()


# -------------------------------------------------------------- 8. model step
def _classifier(key_lengths, query_lengths=False):
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    lens = m.create_tensor([4], DataType.DT_INT32, create_grad=False, name="lens") if key_lengths else None
    a = m.multihead_attention(x, x, x, 128, 2, name="mha", key_lengths=lens, query_lengths=query_lengths)
    m.softmax(m.dense(a, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    return ex


def test_model_graphed_step_matches_eager():
    """The classifier of test_attention_varlen_gpu.py, another lengths batch on
    every step and labels -100 at the padded positions (the loss ignores
    them): the captured step with query_lengths follows the batch it is fed,
    and trains the weights that key lengths alone train."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 8, (4, 64), generator=g).to(DEV)
    vals = ([64, 33, 5, 17], [1, 64, 40, 9], [20, 2, 64, 50])
    batches = [_dev_lens(v) for v in vals]
    labels = [torch.where(_dead(b, 64), torch.full_like(y, -100), y) for b in batches]

    def feeds(i, on):
        return {"input": x, "lens": batches[i]} if on else {"input": x}

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(*mode):
        ex = _classifier(*mode)
        for i in range(3):
            ex.train_step(feeds(i, mode[0]), labels[i])
        return params(ex)

    def graphed(*mode):
        ex = _classifier(*mode)
        step = ex.make_graphed_train_step(feeds(0, mode[0]), labels[0], warmup=1)   # one eager step, then two replays
        step(feeds(1, mode[0]), labels[1])
        step(feeds(2, mode[0]), labels[2])
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    d0 = worst(graphed(False), eager(False))   # graphed against eager without lengths sets the bound
    bound = max(2 * d0, 1e-5)
    keys_only = eager(True)
    n0 = K.STATS["attention_qlens"]
    want = eager(True, True)
    assert K.STATS["attention_qlens"] == n0 + 6     # three forwards and three backwards
    d1 = worst(graphed(True, True), want)
    d2 = worst(want, keys_only)
    print(f"graphed vs eager: no lengths {d0:.3e}, query lengths {d1:.3e}; query lengths vs key lengths only "
          f"{d2:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
    assert d2 <= bound, (d2, bound)


# --------------------------------------------------------- 9. argument errors
def test_argument_errors():
    c = _inputs(96, 160, 64, False)
    q, k, v = c["q"], c["k"], c["v"]
    bad = [torch.ones(B, device=DEV, dtype=torch.int64),            # dtype
           torch.ones(B, device=DEV, dtype=torch.float32),
           torch.ones(B + 1, device=DEV, dtype=torch.int32),        # shape
           torch.ones(B, 1, device=DEV, dtype=torch.int32),
           torch.ones(B, dtype=torch.int32),                        # device
           torch.ones(2 * B, device=DEV, dtype=torch.int32)[::2],   # not contiguous
           [96] * B]                                                # not a tensor
    n0, b0, q0 = K.STATS["attention_fwd"], K.STATS["attention_bwd"], K.STATS["attention_qlens"]
    for lens in bad:
        with pytest.raises(ValueError, match="q_lens"):
            K.attention_fwd(q, k, v, q_lens=lens)
        with pytest.raises(ValueError, match="q_lens"):
            K.attention_fwd(q, k, v, kv_lens=c["lens"], q_lens=lens)
        with pytest.raises(ValueError, match="q_lens"):
            _grads(c, q_lens=lens)
    assert K.STATS["attention_fwd"] == n0 and K.STATS["attention_bwd"] == b0 and K.STATS["attention_qlens"] == q0
