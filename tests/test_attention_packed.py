"""Packed sequences of MULTIHEAD_ATTENTION off the GPU (attribute
`packed_sequences` = M: every row of the batch holds up to M sequences end to
end and the fourth input [batch, M] gives their lengths): the IR checks,
serialisation with and without the attribute, the operator's torch path
against dense fp64 attention of every segment on its own, NaN in the tails,
the FFModel / BERT interface, a packed BERT against the padded one, and the
strategy search.
"""
import json
import math

import pytest
import torch

from dist_util import assert_params_close
from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.models.bert import BertConfig, build_bert
from flexflow_train_amd.ops import attention as A
from flexflow_train_amd.ops import base as opbase
# graphs of one attention node as the commits before packed sequences serialised them
from test_attention_qlens import PARENT_3, PARENT_4
# the small BERT and its padded batch (labels -100 past each length) of the key-lengths tests
from test_attention_varlen import B, S, VOCAB, _bert_batch, _bert_cfg

F32, I32 = C.DataType.FLOAT, C.DataType.INT32
P = C.ParallelTensorShape


def _op(**kw):
    return C.OpAttrs("MULTIHEAD_ATTENTION", embed_dim=32, num_heads=4, **kw)


# ------------------------------------------------------------------------ IR
def test_serial_shape_inference():
    op3, opp = _op(), _op(packed_sequences=3)
    x, seg = C.TensorShape([8, 16, 32], F32), C.TensorShape([8, 3], I32)
    assert C.num_data_inputs(opp) == 4 and opp.has("packed_sequences") and not opp.has("max_seqlen")
    assert not op3.has("packed_sequences") and not op3.has("max_seqlen")
    (o,) = C.infer_output_shapes(opp, [x, x, x, seg])
    assert o == C.infer_output_shapes(op3, [x, x, x])[0]
    assert C.infer_weight_shapes(opp, [x, x, x, seg]) == C.infer_weight_shapes(op3, [x, x, x])
    C.infer_output_shapes(_op(packed_sequences=3, max_seqlen=16), [x, x, x, seg])
    C.infer_output_shapes(_op(packed_sequences=3, max_seqlen=1), [x, x, x, C.TensorShape([8, 3], C.DataType.INT64)])
    with pytest.raises(ValueError, match="expected 4 inputs"):
        C.infer_output_shapes(opp, [x, x, x])
    with pytest.raises(ValueError, match="expected 3 inputs"):
        C.infer_output_shapes(op3, [x, x, x, seg])
    for bad, why in ((C.TensorShape([8], I32), "rank 2"), (C.TensorShape([8, 3, 1], I32), "rank 2"),
                     (C.TensorShape([8, 3], F32), "integer dtype"), (C.TensorShape([4, 3], I32), "batch mismatch"),
                     (C.TensorShape([8, 4], I32), "differs from M")):
        with pytest.raises(ValueError, match=f"packed_sequences.*{why}"):
            C.infer_output_shapes(opp, [x, x, x, bad])
    kv = C.TensorShape([8, 24, 32], F32)
    with pytest.raises(ValueError, match="packed_sequences needs equal q / k / v sequence extents"):
        C.infer_output_shapes(opp, [x, kv, kv, seg])
    for ms in (0, -1, 17):
        with pytest.raises(ValueError, match="max_seqlen must lie in 1"):
            C.infer_output_shapes(_op(packed_sequences=3, max_seqlen=ms), [x, x, x, seg])
    with pytest.raises(ValueError, match="max_seqlen needs packed_sequences"):
        C.infer_output_shapes(_op(max_seqlen=8), [x, x, x])
    with pytest.raises(ValueError, match="packed_sequences must be at least 1"):
        C.infer_output_shapes(_op(packed_sequences=0), [x, x, x])
    for kw in (dict(key_lengths=True), dict(key_lengths=True, query_lengths=True)):
        with pytest.raises(ValueError, match="packed_sequences excludes key_lengths / query_lengths"):
            C.infer_output_shapes(_op(packed_sequences=3, **kw), [x, x, x, seg])


def test_parallel_shape_inference():
    op3, opp = _op(), _op(packed_sequences=3, max_seqlen=12)
    x = P([8, 16, 32], [2, 1, 1], 1, 2, F32)      # batch degree 2, head (replica) degree 2
    seg = P([8, 3], [2, 1], 1, 2, I32)
    assert C.infer_parallel_output_shapes(opp, [x, x, x, seg]) == C.infer_parallel_output_shapes(op3, [x, x, x])
    assert C.infer_parallel_weight_shapes(opp, [x, x, x, seg]) == C.infer_parallel_weight_shapes(op3, [x, x, x])
    assert C.is_valid_parallelization(opp, [x, x, x, seg])
    assert not C.is_valid_parallelization(opp, [x, x, x, P([8, 3], [1, 1], 1, 2, I32)]), "batch degree differs from q"
    assert not C.is_valid_parallelization(opp, [x, x, x, P([8, 3], [2, 1], 1, 1, I32)]), "replica degree differs"
    assert not C.is_valid_parallelization(opp, [x, x, x, P([8, 3], [2, 3], 1, 2, I32)]), "a partitioned segment dim"
    assert not C.is_valid_parallelization(opp, [x, x, x, P([8], [2], 1, 2, I32)]), "rank 1"
    kv = P([8, 24, 32], [2, 1, 1], 1, 2, F32)
    assert not C.is_valid_parallelization(opp, [x, kv, kv, seg]), "q / k sequence extents differ"
    s = P([8, 16, 32], [1, 2, 1], 1, 1, F32)      # a sharded sequence: invalid with packs, not a crash
    assert not C.is_valid_parallelization(opp, [s, s, s, P([8, 3], [1, 1], 1, 1, I32)])
    with pytest.raises(ValueError, match="unpartitioned sequence dim"):
        C.infer_parallel_output_shapes(opp, [s, s, s, P([8, 3], [1, 1], 1, 1, I32)])


def _one_node_graph(M=None, max_seqlen=None, lengths=False):
    cfg = FFConfig()
    cfg.cpu_only = True
    m = FFModel(cfg)
    x = m.create_tensor([2, 8, 16], DataType.DT_FLOAT, name="x")
    kw = {}
    if lengths:
        kw["key_lengths"] = m.create_tensor([2], DataType.DT_INT32, create_grad=False, name="lens")
    if M:
        kw["packed_sequences"] = m.create_tensor([2, M], DataType.DT_INT32, create_grad=False, name="lens")
    m.multihead_attention(x, x, x, 16, 2, name="mha", max_seqlen=max_seqlen, **kw)
    return m


def test_graphs_without_the_attribute_serialise_as_before():
    assert _one_node_graph().cg.to_json() == PARENT_3
    assert _one_node_graph(lengths=True).cg.to_json() == PARENT_4
    # with it: the 4-input graph with a [2, 3] input and the attributes in place of key_lengths
    want = PARENT_4.replace('{"ints":[2]}', '{"ints":[2,3]}').replace('"dims":[2]}', '"dims":[2,3]}')
    assert want != PARENT_4
    assert _one_node_graph(3).cg.to_json() == want.replace('"key_lengths":true,', '').replace(
        '"num_heads":2,', '"num_heads":2,"packed_sequences":3,')
    assert _one_node_graph(3, 5).cg.to_json() == want.replace('"key_lengths":true,', '"max_seqlen":5,').replace(
        '"num_heads":2,', '"num_heads":2,"packed_sequences":3,')


def test_ffmodel_interface_serialises_and_reloads():
    m = _one_node_graph(3, 5)
    text = m.cg.to_json()
    assert C.ComputationGraph.from_json(text).to_json() == text
    assert '"packed_sequences":3' in text and '"max_seqlen":5' in text
    with pytest.raises(ValueError, match="max_seqlen needs packed_sequences"):
        _one_node_graph(max_seqlen=4)
    with pytest.raises(ValueError, match="max_seqlen must lie in 1"):
        _one_node_graph(3, 9)
    cfg = FFConfig()
    cfg.cpu_only = True
    m = FFModel(cfg)
    x = m.create_tensor([2, 8, 16], DataType.DT_FLOAT, name="x")
    kv = m.create_tensor([2, 12, 16], DataType.DT_FLOAT, name="kv")
    lens = m.create_tensor([2], DataType.DT_INT32, create_grad=False, name="lens")
    seg = m.create_tensor([2, 3], DataType.DT_INT32, create_grad=False, name="seg")
    with pytest.raises(ValueError, match="equal q / k / v sequence extents"):
        m.multihead_attention(x, kv, kv, 16, 2, name="mha", packed_sequences=seg)
    with pytest.raises(ValueError, match="packed_sequences excludes key_lengths"):
        m.multihead_attention(x, x, x, 16, 2, name="mha", packed_sequences=seg, key_lengths=lens)
    with pytest.raises(ValueError, match="must be a \\[batch, M\\] tensor"):
        m.multihead_attention(x, x, x, 16, 2, name="mha", packed_sequences=lens)


# ------------------------------------------------------------------ torch path
# fp32 against fp64, sums of at most 24 terms of O(1) values: the tolerance of
# test_attention_qlens.py test_torch_path_against_truncated_samples
_F32_OP = dict(rtol=1e-4, atol=1e-5)
T_, M_, H_, D_ = 24, 5, 2, 16
# a zero-length slot in the middle; an all-empty pack; an exactly full pack; an
# over-full one (the 15 is clamped to 6, the rest to 0); lengths above max_seqlen
SEG = [[7, 0, 9, 3, 0], [0, 0, 0, 0, 0], [10, 14, 0, 0, 0], [8, 10, 15, 4, 1], [30, 2, 0, 0, 40]]


def _clamped(seg, T, ms):
    out = []
    for row in seg:
        pos, r = 0, []
        for n in row:
            n = max(0, min(n, ms, T - pos))
            r.append((pos, n))
            pos += n
        out.append(r)
    return out


def _tail(seg, T, ms):
    ends = torch.tensor([r[-1][0] + r[-1][1] for r in _clamped(seg, T, ms)])
    return torch.arange(T).view(1, T) >= ends.view(-1, 1)


def _qkv(seed, Nn=len(SEG), Tn=T_):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(Nn, Tn, H_, D_, generator=g) for _ in range(4)]


def _run_torch_path(q, k, v, do, seg, causal, ms, p=0.0):
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    st = torch.tensor(seg, dtype=torch.int32)
    drop = A.attention_dropout_mask(len(seg) * len(seg[0]), H_, ms, ms, p, 99) if p else None
    o = A._torch_packed_attention(qs, ks, vs, causal, 1.0 / math.sqrt(D_), st, ms, drop)
    o.backward(do)
    return o.detach(), qs.grad, ks.grad, vs.grad


def test_packed_segments_definition():
    for ms in (T_, 12):
        start, lens, seg_id = A.packed_segments(torch.tensor(SEG, dtype=torch.int32), T_, ms)
        want = _clamped(SEG, T_, ms)
        assert start.tolist() == [[s for s, _ in r] for r in want] and lens.tolist() == [[n for _, n in r] for r in want]
        for n, r in enumerate(want):
            ids = [-1] * T_
            for m, (s, ln) in enumerate(r):
                ids[s:s + ln] = [m] * ln
            assert seg_id[n].tolist() == ids
    assert _clamped(SEG, T_, T_)[3] == [(0, 8), (8, 10), (18, 6), (24, 0), (24, 0)]
    assert _clamped(SEG, T_, 12)[4] == [(0, 12), (12, 2), (14, 0), (14, 0), (14, 10)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("ms", [T_, 12], ids=["max_T", "max_12"])
@pytest.mark.parametrize("causal", [False, True])
def test_torch_path_against_dense_segments(causal, ms, p):
    """Every segment cut out and run on its own as dense attention in fp64
    (with the dropout mask of sample n * M + m) gives its rows of o, dQ, dK
    and dV; the tail rows are zero."""
    q, k, v, do = _qkv(31)
    o, dq, dk, dv = _run_torch_path(q, k, v, do, SEG, causal, ms, p)
    keep = A.attention_dropout_mask(len(SEG) * M_, H_, ms, ms, p, 99) if p else None
    for n, row in enumerate(_clamped(SEG, T_, ms)):
        for m, (s, ln) in enumerate(row):
            if not ln:
                continue
            qb, kb, vb = (t[n, s:s + ln].double().transpose(0, 1).requires_grad_(True) for t in (q, k, v))
            sc = qb @ kb.transpose(-1, -2) / math.sqrt(D_)
            if causal:
                sc = sc.masked_fill(torch.ones(ln, ln, dtype=torch.bool).triu(1), float("-inf"))
            pr = torch.softmax(sc, -1)
            if keep is not None:
                pr = pr * keep[0][n * M_ + m, :, :ln, :ln].double() * keep[1]
            ref = pr @ vb
            ref.backward(do[n, s:s + ln].double().transpose(0, 1))
            for name, got, want in (("o", o, ref.detach()), ("dq", dq, qb.grad), ("dk", dk, kb.grad), ("dv", dv, vb.grad)):
                torch.testing.assert_close(got[n, s:s + ln].double().transpose(0, 1), want, **_F32_OP,
                                           msg=lambda t: f"{name}[{n}, {m}]: {t}")
    tail = _tail(SEG, T_, ms)
    assert tail[1].all() and (ms < T_ or not tail[2].any()) and int(tail.sum()) > T_
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert (t[tail] == 0).all(), name
        assert torch.isfinite(t).all(), name


@pytest.mark.parametrize("causal", [False, True])
def test_torch_path_nan_in_the_tails(causal):
    """NaN in every tail row of q, k, v and of the incoming gradient: every
    output and gradient is finite and equal to the run on clean inputs."""
    q, k, v, do = _qkv(32)
    clean = _run_torch_path(q, k, v, do, SEG, causal, 12)
    tail = _tail(SEG, T_, 12)
    dirty = [t.clone() for t in (q, k, v, do)]
    for t in dirty:
        t[tail] = float("nan")
    got = _run_torch_path(*dirty, SEG, causal, 12)
    for name, a, c in zip(("o", "dq", "dk", "dv"), got, clean):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, c), name


def test_operator_attribute_and_refusals():
    g = torch.Generator().manual_seed(5)
    W = torch.randn(32 * 3 * 4 * 8 + 4 * 8 * 32, generator=g).view(-1, 4) * 0.3
    x = torch.randn(2, 8, 32, generator=g)
    attrs = {"embed_dim": 32, "num_heads": 4, "kdim": 0, "vdim": 0, "causal": False, "packed_sequences": 3}
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = opbase.OpContext(op_type="MULTIHEAD_ATTENTION", attrs=attrs, name="mha", training=True)
    seg = torch.tensor([[3, 0, 4], [2, 2, 9]], dtype=torch.int64)
    (out,), saved = impl.forward(ctx, [x, x, x, seg], [W])
    assert (out[0, 7:] == 0).all() and (out[0, :7] != 0).any() and (out[1] != 0).all(dim=-1).all()   # no bias: o Wo = 0
    # a segment is attention over its own rows: the same rows of a batch that holds it alone
    one = torch.tensor([[3, 0, 0], [0, 0, 0]], dtype=torch.int64)
    (alone,), _ = impl.forward(ctx, [x, x, x, one], [W])
    torch.testing.assert_close(alone[0, :3], out[0, :3])
    assert (alone[1] == 0).all()
    grads = impl.backward(ctx, saved, [torch.ones_like(out)], [torch.zeros_like(W)], [True, False, False])
    assert len(grads) == 4 and grads[3] is None and torch.isfinite(grads[0]).all()
    with pytest.raises(ValueError, match="packed_sequences needs the segment lengths input"):
        impl.forward(ctx, [x, x, x], [W])
    for bad in (seg.float(), seg[:, :2], seg.reshape(-1)):
        with pytest.raises(ValueError, match="segment lengths must be an integer tensor"):
            impl.forward(ctx, [x, x, x, bad], [W])
    both = opbase.OpContext(op_type="MULTIHEAD_ATTENTION", attrs=dict(attrs, key_lengths=True), name="mha")
    with pytest.raises(ValueError, match="packed_sequences excludes key_lengths"):
        impl.forward(both, [x, x, x, seg], [W])
    ctx.extra["seq_group"] = type("Group", (), {"size": 2})()
    with pytest.raises(NotImplementedError, match="packed sequences are not supported on the sequence-parallel"):
        impl.forward(ctx, [x, x, x, seg], [W])


# --------------------------------------------------------------- model level
M_BERT = 3
TAIL_ID = VOCAB - 1      # the token id of the tail positions: no live position holds it


def _padded_batch():
    feeds, labels, live = _bert_batch(0)
    feeds = dict(feeds, input_ids=feeds["input_ids"] % TAIL_ID)      # live ids in [0, VOCAB - 2]
    return feeds, labels, live


def _packed_batch():
    """The sequences of the padded batch packed first-fit into rows of S
    tokens, in B rows so that the loss is averaged over as many positions:
    position ids restart per sequence, labels are -100 on the tails."""
    feeds, labels, _ = _padded_batch()
    lens = feeds["seq_lens"].tolist()
    rows = []
    for b, n in enumerate(lens):
        for r in rows:
            if sum(lens[i] for i in r) + n <= S and len(r) < M_BERT:
                r.append(b)
                break
        else:
            rows.append([b])
    assert len(rows) < B and any(len(r) > 1 for r in rows)
    ids = torch.full((B, S), TAIL_ID, dtype=torch.int32)
    pos = torch.zeros(B, S, dtype=torch.int32)
    lab = torch.full((B, S), -100)
    seg = torch.zeros(B, M_BERT, dtype=torch.int32)
    for n, r in enumerate(rows):
        at = 0
        for m, b in enumerate(r):
            ln = lens[b]
            ids[n, at:at + ln] = feeds["input_ids"][b, :ln]
            pos[n, at:at + ln] = torch.arange(ln, dtype=torch.int32)
            lab[n, at:at + ln] = labels[b, :ln]
            seg[n, m] = ln
            at += ln
    packed = {"input_ids": ids, "position_ids": pos, "token_type_ids": torch.zeros(B, S, dtype=torch.int32),
              "seg_lens": seg}
    return packed, lab


def _bert_model(cfg=None, **kw):
    cfg = cfg or FFConfig()
    cfg.cpu_only = True
    cfg.print_freq = 0
    m = FFModel(cfg)
    inputs, probs = build_bert(m, _bert_cfg(**kw))
    return m, inputs, probs


def _train_bert(feeds, labels, steps=3, **kw):
    m, _, _ = _bert_model(**kw)
    m.compile(optimizer=SGDOptimizer(m, lr=0.5), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    first = {n: ex.get_parameter(n).detach().clone() for n in sorted(ex.parameter_names())}
    for _ in range(steps):
        ex.train_step(feeds, labels)
    return first, {n: ex.get_parameter(n).detach().clone() for n in sorted(ex.parameter_names())}


def test_bert_config_and_graph():
    assert BertConfig().packed_sequences == 0 and BertConfig().max_seqlen == 0
    for kw in (dict(key_lengths=True), dict(key_lengths=True, query_lengths=True)):
        with pytest.raises(ValueError, match="packed_sequences excludes"):
            _bert_model(packed_sequences=3, **kw)
    with pytest.raises(ValueError, match="max_seqlen needs packed_sequences"):
        _bert_model(max_seqlen=8)
    m, inputs, _ = _bert_model(packed_sequences=3, max_seqlen=12)
    assert sorted(inputs) == ["input_ids", "position_ids", "seg_lens", "token_type_ids"]
    assert list(inputs["seg_lens"].dims) == [B, 3]
    attn = [l for l in m.get_layers() if l.op_type == "MULTIHEAD_ATTENTION"]
    assert len(attn) == 2 and all(len(m.cg.layer_data_inputs(l.node)) == 4 for l in attn)
    text = m.cg.to_json()
    assert text.count('"packed_sequences":3') == 2 and text.count('"max_seqlen":12') == 2
    assert C.ComputationGraph.from_json(text).to_json() == text
    # off by default: the graph built before
    m0, _, _ = _bert_model()
    assert "packed_sequences" not in m0.cg.to_json() and "max_seqlen" not in m0.cg.to_json()


def test_bert_trains_the_same_weights_packed_and_padded():
    """The same sequences padded (key and query lengths) and packed: every
    live token sees the same keys at the same positions and the loss averages
    over as many rows, so three steps reach the same weights, at the bound of
    test_attention_qlens.py's with / without comparison.  A tail token adds
    exactly nothing to the gradient of its embedding row."""
    feeds, labels, _ = _padded_batch()
    _, padded = _train_bert(feeds, labels, key_lengths=True, query_lengths=True)
    pfeeds, plabels = _packed_batch()
    assert (pfeeds["input_ids"] == TAIL_ID).any() and int((plabels != -100).sum()) == int((labels != -100).sum())
    first, packed = _train_bert(pfeeds, plabels, packed_sequences=M_BERT)
    assert_params_close(padded, packed)
    word = "embeddings.word.weight" if "embeddings.word.weight" in packed else \
        [n for n in packed if n.startswith("embeddings.word")][0]
    assert torch.equal(packed[word][TAIL_ID], first[word][TAIL_ID]), "a tail token moved its embedding row"
    assert not torch.equal(packed[word][:TAIL_ID], first[word][:TAIL_ID])


def test_strategy_search_over_a_packed_model():
    from flexflow_train_amd.search import native

    m, _, _ = _bert_model(packed_sequences=3, max_seqlen=12)
    attn = [l for l in m.get_layers() if l.op_type == "MULTIHEAD_ATTENTION"][0]
    cands = [json.loads(c) for c in C.candidate_configs(m.cg, attn.node, 8)]
    assert cands and all(c["seq"] == 1 for c in cands), "no sequence-parallel config for a packed node"
    assert any(c["kind"] == "heads" for c in cands) and any(c["batch"] == 8 for c in cands)
    cm = native.cost_model()
    cfg = json.dumps({"world": 8, "budget": 100, "time_limit": 20, "seed": 1})
    for pcg, rep in (C.graph_optimize(m.cg, cm, cfg)[:2], C.mcmc_search(m.cg, cm, cfg)[:2],
                     C.unity_search(C.data_parallel_pcg(m.cg, 8), cm, cfg)[:2]):
        rep = json.loads(rep)
        assert math.isfinite(rep["cost"]) and 0 < rep["cost"] <= rep["data_parallel_cost"] * 1.0000001
        pcg.reinfer_shapes()      # every node's parallel shapes are valid
    dp = json.loads(C.data_parallel_strategy(m.cg, 8))
    pcg, mapping, _ = C.lower_strategy(m.cg, json.dumps(dp), 8)
    degrees = [pcg.shape(v).shard_degrees() for v in pcg.layer_data_inputs(mapping[attn.node])]
    assert degrees == [[8, 1, 1]] * 3 + [[8, 1]]      # data parallelism shards packs, M stays whole


def test_cost_model_prices_max_seqlen():
    """The node is priced with max_seqlen keys per query (an upper bound):
    cheaper than the unpacked node, and cheaper with a smaller max_seqlen."""
    x, seg = C.TensorShape([8, 256, 32], F32), C.TensorShape([8, 4], I32)

    def flops(op, ins):
        return C.estimate_op_work(op, ins, C.infer_weight_shapes(op, ins), C.infer_output_shapes(op, ins))["flops"]

    whole, packed = flops(_op(), [x, x, x]), flops(_op(packed_sequences=4), [x, x, x, seg])
    short = flops(_op(packed_sequences=4, max_seqlen=64), [x, x, x, seg])
    assert whole == packed > short
    # the attention core's share shrinks by max_seqlen / T
    core = 4 * 8 * 4 * 256 * 256 * 8
    assert whole - short == pytest.approx(core * (1 - 64 / 256))


def test_local_execution_rejects_the_node():
    cfg = FFConfig()
    cfg.local_execution = True
    m, _, _ = _bert_model(cfg, packed_sequences=3)
    with pytest.raises(ValueError, match="the fourth input"):
        m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    with pytest.raises(ValueError, match="the fourth input"):
        C.LocalTrainingBacking(m.cg)
