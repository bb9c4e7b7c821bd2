"""Packed sequences in the flash kernels (the PACKED instantiations of the
forward, dQ and dK/dV kernels of attention.hip): several sequences
("segments") laid end to end in each row ("pack") of [N, T, H, D] tensors,
their lengths in seg_lens [N, M]; attention stays inside a segment.

N = 3 packs of T = 200 tokens, M = 6 slots, max_seqlen = 192, H = 2.  Pack 0
is [1, 31, 33, 0, 64, 70]: its boundaries 1, 32, 65, 129, 199 fall off every
32-row and 64-row grid, a slot in the middle is empty and one tail token is
left.  Pack 1 is an exactly full [130, 70]: its first segment spans two
128-row blocks.  Pack 2 is over-full ([100, 90, 50, 7, 0, 3]: the 50 is
clamped to 10, the rest to 0).  A second packing has an all-empty pack, a
length above max_seqlen and a pack of one short segment.
"""
import functools
import math

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops.attention import attention_dropout_mask, packed_segments

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, T, M, MS, H = 3, 200, 6, 192, 2
SEED = 4321
PACKINGS = {
    "mixed": [[1, 31, 33, 0, 64, 70], [130, 70, 0, 0, 0, 0], [100, 90, 50, 7, 0, 3]],
    "empty": [[0, 0, 0, 0, 0, 0], [250, 20, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0]],
}
# what the definition makes of them: (start, len) per slot
CLAMPED = {
    "mixed": [[(0, 1), (1, 31), (32, 33), (65, 0), (65, 64), (129, 70)],
              [(0, 130), (130, 70), (200, 0), (200, 0), (200, 0), (200, 0)],
              [(0, 100), (100, 90), (190, 10), (200, 0), (200, 0), (200, 0)]],
    "empty": [[(0, 0)] * 6, [(0, 192), (192, 8), (200, 0), (200, 0), (200, 0), (200, 0)],
              [(0, 5), (5, 0), (5, 0), (5, 0), (5, 0), (5, 0)]],
}
HEADS = [(64, False), (64, True), (128, False), (128, True)]
PS = [0.0, 0.1]
# relative Frobenius error of a bf16 result against fp64: the suite's bound
# for bf16 operators (test_kernels_gpu.py _BF_OP)
_BF_OP = 5e-3
# the LSE (fp32, log2 domain) against fp64: test_attention_varlen_gpu.py _LSE_TOL
_LSE_TOL = dict(rtol=1e-4, atol=1e-3)
NEG_INF = float("-inf")


def _seg(name):
    return torch.tensor(PACKINGS[name], device=DEV, dtype=torch.int32)


def _rel64(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _tail_mask(name):
    """[N, T] bool: the token is past its pack's last segment."""
    ends = torch.tensor([row[-1][0] + row[-1][1] for row in CLAMPED[name]], device=DEV)
    return torch.arange(T, device=DEV).view(1, T) >= ends.view(N, 1)


def _drop_kw(p):
    return dict(dropout_p=p, seed=SEED) if p else {}


@functools.lru_cache(maxsize=None)
def _inputs(D):
    g = torch.Generator(device=DEV).manual_seed(77 + D)
    qkv = torch.randn(N, T, 3, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    qkv[:, :, :2] *= 0.5
    do = torch.randn(N, T, H, D, device=DEV, dtype=torch.bfloat16, generator=g)
    return qkv, do


def _packed_call(qkv, do, seg, causal, p, fill=float("nan")):
    """Forward and backward of the packed call into buffers pre-filled with
    `fill`: (o, lse, dq, dk, dv)."""
    D = qkv.shape[-1]
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out = torch.full((N, T, H, D), fill, device=DEV, dtype=torch.bfloat16)
    kw = dict(causal=causal, seg_lens=seg, max_seqlen=MS, **_drop_kw(p))
    o, lse = K.attention_fwd(q, k, v, out=out, **kw)
    d = torch.full((N, T, 3, H, D), fill, device=DEV, dtype=torch.bfloat16)
    path = K.attention_bwd(q, k, v, o, lse, do, d[:, :, 0], d[:, :, 1], d[:, :, 2], **kw)
    assert path == 0
    return o, lse, d[:, :, 0], d[:, :, 1], d[:, :, 2]


@functools.lru_cache(maxsize=None)
def _case(name, D, causal, p):
    qkv, do = _inputs(D)
    n0 = K.STATS["attention_packed"]
    got = _packed_call(qkv, do, _seg(name), causal, p)
    assert K.STATS["attention_packed"] == n0 + 2
    torch.cuda.synchronize()
    return got


def test_segment_offsets_follow_the_definition():
    for name in PACKINGS:
        off = K.attention_segment_offsets(_seg(name), T, MS)
        assert off.dtype == torch.int32 and off.tolist() == [[list(p) for p in row] for row in CLAMPED[name]], name
        start, lens, seg_id = packed_segments(_seg(name), T, MS)           # the torch definition
        assert torch.equal(off[:, :, 0].long(), start) and torch.equal(off[:, :, 1].long(), lens)
        assert torch.equal(seg_id < 0, _tail_mask(name))
    neg = torch.tensor([[-3, 7, 1 << 30]], device=DEV, dtype=torch.int32)
    assert K.attention_segment_offsets(neg, 40).tolist() == [[[0, 0], [0, 7], [7, 33]]]
    assert K.attention_segment_offsets(neg, 40, 16).tolist() == [[[0, 0], [0, 7], [7, 16]]]


# ------------------------------------------- 1. bit equality with the padded call
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D,causal", HEADS)
@pytest.mark.parametrize("name", list(PACKINGS))
def test_bit_equal_to_the_padded_call(name, D, causal, p):
    """The segments unpacked into a [N * M, max_seqlen] batch (NaN as padding)
    and run through the lengths kernels with kv_lens = q_lens = lens: the same
    arithmetic in the same local coordinates, so the same bits."""
    qkv, do = _inputs(D)
    o, lse, dq, dk, dv = _case(name, D, causal, p)
    flat = [sl for row in CLAMPED[name] for sl in row]
    pad = torch.full((N * M, MS, 3, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    pdo = torch.full((N * M, MS, H, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    for i, (st, ln) in enumerate(flat):
        pad[i, :ln] = qkv[i // M, st:st + ln]
        pdo[i, :ln] = do[i // M, st:st + ln]
    lens = torch.tensor([ln for _, ln in flat], device=DEV, dtype=torch.int32)
    kw = dict(causal=causal, kv_lens=lens, q_lens=lens, **_drop_kw(p))
    po, plse = K.attention_fwd(pad[:, :, 0], pad[:, :, 1], pad[:, :, 2], **kw)
    pd = torch.empty_like(pad)
    K.attention_bwd(pad[:, :, 0], pad[:, :, 1], pad[:, :, 2], po, plse, pdo, pd[:, :, 0], pd[:, :, 1], pd[:, :, 2], **kw)
    torch.cuda.synchronize()
    live = 0
    for i, (st, ln) in enumerate(flat):
        n = i // M
        assert torch.equal(o[n, st:st + ln], po[i, :ln]), ("o", i)
        assert torch.equal(lse[n, :, st:st + ln], plse[i, :, :ln]), ("lse", i)
        for j, (name_, g) in enumerate((("dq", dq), ("dk", dk), ("dv", dv))):
            assert torch.equal(g[n, st:st + ln], pd[i, :ln, j]), (name_, i)
        live += ln
    assert live == int((~_tail_mask(name)).sum())


# --------------------------------------------------------- 2. against fp64
def _ref64(name, D, causal, p):
    """Dense attention of every segment on its own, in fp64, with the dropout
    mask of sample n * M + m of the [N * M, H, max_seqlen, max_seqlen] batch:
    (o, lse in the log2 domain, dq, dk, dv), zeros outside the segments."""
    qkv, do = _inputs(D)
    x = qkv.double().requires_grad_(True)
    keep = attention_dropout_mask(N * M, H, MS, MS, p, SEED, DEV) if p else None
    o = torch.zeros(N, T, H, D, device=DEV, dtype=torch.float64)
    lse = torch.full((N, H, T), NEG_INF, device=DEV, dtype=torch.float64)
    for n, row in enumerate(CLAMPED[name]):
        for m, (st, ln) in enumerate(row):
            if not ln:
                continue
            q, k, v = (x[n, st:st + ln, j].transpose(0, 1) for j in range(3))          # [H, len, D]
            s = q @ k.transpose(-1, -2) / math.sqrt(D)
            if causal:
                s = s.masked_fill(torch.ones(ln, ln, device=DEV, dtype=torch.bool).triu(1), NEG_INF)
            pr = torch.softmax(s, -1)
            if keep is not None:
                pr = pr * keep[0][n * M + m, :, :ln, :ln].to(pr.dtype) * keep[1]
            o[n, st:st + ln] = (pr @ v).transpose(0, 1)
            lse[n, :, st:st + ln] = (torch.logsumexp(s, -1) * math.log2(math.e)).detach()
    o.backward(do.double())
    g = x.grad
    return o.detach(), lse, g[:, :, 0], g[:, :, 1], g[:, :, 2]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D,causal", HEADS)
def test_forward_and_backward_against_fp64(D, causal, p):
    got = _case("mixed", D, causal, p)
    want = _ref64("mixed", D, causal, p)
    live = ~_tail_mask("mixed")[:, None, :].expand(N, H, T)
    a, b = got[1].double()[live], want[1][live]
    print(f"packed D{D} causal={causal} p={p}: LSE max abs {float((a - b).abs().max()):.3e}")
    assert torch.allclose(a, b, **_LSE_TOL)
    for nm, x, y in zip(("O", "dQ", "dK", "dV"), (got[0],) + got[2:], (want[0],) + want[2:]):
        err = _rel64(x, y)
        print(f"packed D{D} causal={causal} p={p}: {nm} {err:.3e}")
        assert err < _BF_OP, (nm, err)


# ---------------------------------------------------- 3. neighbour and tail
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("D,causal", HEADS)
@pytest.mark.parametrize("name", list(PACKINGS))
def test_neighbour_and_tail(name, D, causal, p):
    """Into NaN-filled buffers: every row of a segment is written and finite,
    every tail row is exactly zero (lse = -inf).  NaN in the tail rows of q,
    k, v and dO changes no bit of any output."""
    clean = _case(name, D, causal, p)
    tail = _tail_mask(name)
    assert int(tail.sum()) > 0
    o, lse = clean[:2]
    for nm, t in zip(("o", "dq", "dk", "dv"), (o,) + clean[2:]):
        assert torch.isfinite(t).all(), nm
        assert (t[tail] == 0).all(), nm
        # (dQ and dK of a row with one key are exactly zero, and dropout can drop a short row's every key)
        assert p or nm in ("dq", "dk") or (t[~tail].float().abs().sum(-1) > 0).all(), f"{nm}: a live row is zero"
    assert (lse.transpose(1, 2)[tail] == NEG_INF).all() and torch.isfinite(lse.transpose(1, 2)[~tail]).all()
    qkv, do = _inputs(D)
    qkv, do = qkv.clone(), do.clone()
    qkv[tail] = float("nan")
    do[tail] = float("nan")
    dirty = _packed_call(qkv, do, _seg(name), causal, p)
    for nm, a, b in zip(("o", "lse", "dq", "dk", "dv"), dirty, clean):
        assert not torch.isnan(a).any(), nm
        assert torch.equal(a, b), nm


# ------------------------------------------------------------ 4. graph replay
def test_graph_replay_follows_the_segment_lengths():
    qkv, do = _inputs(64)
    seg = _seg("mixed").clone()

    def run(s):
        return _packed_call(qkv, do, s, True, 0.1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(seg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held = run(seg)
    replays = []
    for name in ("empty", "mixed"):
        seg.copy_(_seg(name))
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in held])
        for nm, x, y in zip(("o", "lse", "dq", "dk", "dv"), replays[-1], _case(name, 64, True, 0.1)):
            assert torch.equal(x, y), (name, nm)
    for i in range(5):
        assert not torch.equal(replays[0][i], replays[1][i])


# -------------------------------------------------------------- 5. model step
def _classifier(packed):
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    seg = m.create_tensor([4, 3], DataType.DT_INT32, create_grad=False, name="seg_lens") if packed else None
    a = m.multihead_attention(x, x, x, 128, 2, name="mha", packed_sequences=seg, max_seqlen=48 if packed else None)
    m.softmax(m.dense(a, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    return ex


def test_model_graphed_step_matches_eager():
    """The classifier of test_attention_qlens_gpu.py with packed sequences:
    another packing on every step, labels -100 on the tails.  The captured
    step follows the packing it is fed, at the bound that graphed against
    eager sets without packing."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 64, 128, generator=g).to(DEV)
    y = torch.randint(0, 8, (4, 64), generator=g).to(DEV)
    vals = ([[33, 5, 17], [48, 16, 0], [0, 0, 0], [1, 0, 40]], [[1, 48, 9], [20, 20, 20], [64, 0, 0], [0, 7, 0]],
            [[20, 2, 42], [0, 0, 64], [48, 1, 1], [30, 30, 30]])
    batches = [torch.tensor(v, device=DEV, dtype=torch.int32) for v in vals]
    labels = [torch.where(packed_segments(b, 64, 48)[2] < 0, torch.full_like(y, -100), y) for b in batches]
    assert all((l == -100).any() and (l != -100).any() for l in labels)

    def feeds(i, on):
        return {"input": x, "seg_lens": batches[i]} if on else {"input": x}

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(on):
        ex = _classifier(on)
        for i in range(3):
            ex.train_step(feeds(i, on), labels[i])
        return params(ex)

    def graphed(on):
        ex = _classifier(on)
        step = ex.make_graphed_train_step(feeds(0, on), labels[0], warmup=1)   # one eager step, then two replays
        step(feeds(1, on), labels[1])
        step(feeds(2, on), labels[2])
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    d0 = worst(graphed(False), eager(False))   # graphed against eager without packing sets the bound
    bound = max(2 * d0, 1e-5)
    n0 = K.STATS["attention_packed"]
    want = eager(True)
    assert K.STATS["attention_packed"] == n0 + 6     # three forwards and three backwards
    d1 = worst(graphed(True), want)
    print(f"graphed vs eager: unpacked {d0:.3e}, packed {d1:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
    assert worst(want, eager(False)) > 1e-3, "the packing changes what the model computes"


# --------------------------------------------------------- 6. argument errors
def test_argument_errors():
    qkv, do = _inputs(64)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    seg = _seg("mixed")
    lens = torch.full((N,), T, device=DEV, dtype=torch.int32)
    n0, b0, p0 = K.STATS["attention_fwd"], K.STATS["attention_bwd"], K.STATS["attention_packed"]
    o, lse = torch.empty(N, T, H, 64, device=DEV, dtype=torch.bfloat16), torch.empty(N, H, T, device=DEV)
    d = torch.empty_like(qkv)

    def bwd(**kw):
        kw.setdefault("seg_lens", seg)
        return K.attention_bwd(q, k, v, o, lse, do, d[:, :, 0], d[:, :, 1], d[:, :, 2], **kw)

    for kw in (dict(kv_lens=lens), dict(q_lens=lens), dict(kv_lens=lens, q_lens=lens)):
        with pytest.raises(ValueError, match="packed sequences.*kv_lens / q_lens"):
            K.attention_fwd(q, k, v, seg_lens=seg, **kw)
        with pytest.raises(ValueError, match="packed sequences.*kv_lens / q_lens"):
            bwd(**kw)
    kv = torch.randn(N, 96, 2, H, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="packed sequences.*cross-attention"):
        K.attention_fwd(q, kv[:, :, 0], kv[:, :, 1], seg_lens=seg)
    bad = [seg.long(), seg.float(),                                          # dtype
           seg.reshape(-1), seg[:, :, None], seg[:2],                        # rank, batch
           seg.cpu(), PACKINGS["mixed"]]                                     # device, not a tensor
    for s in bad:
        with pytest.raises(ValueError, match="seg_lens"):
            K.attention_fwd(q, k, v, seg_lens=s)
        with pytest.raises(ValueError, match="seg_lens"):
            bwd(seg_lens=s)
    for ms in (0, T + 1):
        with pytest.raises(ValueError, match="max_seqlen"):
            K.attention_fwd(q, k, v, seg_lens=seg, max_seqlen=ms)
    with pytest.raises(ValueError, match="seg_offsets"):
        K.attention_fwd(q, k, v, seg_lens=seg, seg_offsets=torch.zeros(N, M, device=DEV, dtype=torch.int32))
    dbias = [torch.zeros(H * 64, device=DEV) for _ in range(3)]
    for atomic in (False, True):
        with pytest.raises(ValueError, match="packed sequences.*dbias"):
            bwd(dbias=dbias, dbias_atomic=atomic)
    assert (K.STATS["attention_fwd"], K.STATS["attention_bwd"], K.STATS["attention_packed"]) == (n0, b0, p0)
    # the native entry points refuse the same combinations
    view, ext = K._view4, K.ext()
    off = K.attention_segment_offsets(seg, T, MS)
    args = (view(q), view(k), view(v), view(o), lse.data_ptr(), N, H)
    tail = (64, 0.125, False, torch.cuda.current_stream().cuda_stream, 0, 0, 0)
    with pytest.raises(ValueError, match="packed sequences.*kv_lens / q_lens"):
        ext.attention_fwd(*args, MS, MS, *tail, lens.data_ptr(), 0, off.data_ptr(), M, T)
    with pytest.raises(ValueError, match="packed sequences.*self-attention"):
        ext.attention_fwd(*args, MS, 96, *tail, 0, 0, off.data_ptr(), M, T)
    with pytest.raises(ValueError, match="max_seqlen"):
        ext.attention_fwd(*args, T + 8, T + 8, *tail, 0, 0, off.data_ptr(), M, T)
    torch.cuda.synchronize()


# ------------------------------------------------------ 7. unchanged when off
@pytest.mark.parametrize("D,causal", HEADS)
def test_unchanged_when_off(D, causal, monkeypatch):
    """seg_lens=None: the call as it was, with and without lengths, and no
    count of a packed call."""
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    qkv, do = _inputs(D)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    lens = torch.tensor([T, 129, 1], device=DEV, dtype=torch.int32)
    n0 = K.STATS["attention_packed"]
    for kw in ({}, dict(kv_lens=lens), dict(kv_lens=lens, q_lens=lens)):
        runs = []
        for off in ({}, dict(seg_lens=None, max_seqlen=None, seg_offsets=None)):
            o, lse = K.attention_fwd(q, k, v, causal=causal, **kw, **off)
            d = torch.empty_like(qkv)
            path = K.attention_bwd(q, k, v, o, lse, do, d[:, :, 0], d[:, :, 1], d[:, :, 2], causal=causal, **kw, **off)
            runs.append((o, lse, d, path))
        assert runs[0][3] == runs[1][3] == (1 if (D == 64 and not causal and not kw) else 0)
        for a, b in zip(runs[0][:3], runs[1][:3]):
            assert torch.equal(a, b)
    assert K.STATS["attention_packed"] == n0
    # a single segment that fills every pack is the call without lengths, bit for bit
    full = torch.tensor([[T] + [0] * (M - 1)] * N, device=DEV, dtype=torch.int32)
    o0, lse0 = K.attention_fwd(q, k, v, causal=causal)
    o1, lse1 = K.attention_fwd(q, k, v, causal=causal, seg_lens=full)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


def test_bert_shape_keeps_the_onepass_backward_when_off(monkeypatch):
    for var in ("FFK_ATTN_BWD_ONEPASS", "FFK_ATTN_BWD_FUSED_DELTA"):
        monkeypatch.delenv(var, raising=False)
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(2, 512, 3, H, 64, device=DEV, dtype=torch.bfloat16, generator=g)
    do = torch.randn(2, 512, H, 64, device=DEV, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    d = torch.empty_like(qkv)
    n0 = K.STATS["attention_bwd_onepass"]
    o, lse = K.attention_fwd(q, k, v, seg_lens=None)
    assert K.attention_bwd(q, k, v, o, lse, do, d[:, :, 0], d[:, :, 1], d[:, :, 2], seg_lens=None) == 1
    assert K.STATS["attention_bwd_onepass"] == n0 + 1
    seg = torch.tensor([[300, 212], [512, 0]], device=DEV, dtype=torch.int32)
    o, lse = K.attention_fwd(q, k, v, seg_lens=seg)
    assert K.attention_bwd(q, k, v, o, lse, do, d[:, :, 0], d[:, :, 1], d[:, :, 2], seg_lens=seg) == 0
    assert K.STATS["attention_bwd_onepass"] == n0 + 1 and torch.isfinite(d).all()
