"""Per-sample key lengths of MULTIHEAD_ATTENTION off the GPU: the IR (3- and
4-input shape inference, serial and parallel), the operator's fp32 torch path
against a per-sample truncated computation, the FFModel / BERT interface, the
strategy search, data parallelism on gloo ranks and the executors that must
refuse the input.
"""
import json
import math

import pytest
import torch

from dist_util import assert_params_close, run_distributed, run_single
from flexflow_train_amd import _ffcore as C
from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.models.bert import BertConfig, build_bert
from flexflow_train_amd.ops import attention as A
from flexflow_train_amd.ops import base as opbase

F32, I32, I64 = C.DataType.FLOAT, C.DataType.INT32, C.DataType.INT64
P = C.ParallelTensorShape


def _ops():
    return (C.OpAttrs("MULTIHEAD_ATTENTION", embed_dim=32, num_heads=4),
            C.OpAttrs("MULTIHEAD_ATTENTION", embed_dim=32, num_heads=4, key_lengths=True))


# ------------------------------------------------------------------------ IR
def test_serial_shape_inference():
    op3, op4 = _ops()
    x, kv = C.TensorShape([8, 16, 32], F32), C.TensorShape([8, 24, 32], F32)
    assert C.num_data_inputs(op3) == 3 and C.num_data_inputs(op4) == 4
    assert not op3.has("key_lengths"), "a node without lengths serialises as before"
    for dt in (I32, I64):
        (o,) = C.infer_output_shapes(op4, [x, kv, kv, C.TensorShape([8], dt)])
        assert o == C.infer_output_shapes(op3, [x, kv, kv])[0] and o.dims == [8, 16, 32]
    assert C.infer_weight_shapes(op4, [x, kv, kv, C.TensorShape([8], I32)]) == C.infer_weight_shapes(op3, [x, kv, kv])
    bad = [([x, kv, kv], "expected 4 inputs"),
           ([x, kv, kv, C.TensorShape([8], F32)], "integer dtype"),
           ([x, kv, kv, C.TensorShape([4], I32)], "batch mismatch"),
           ([x, kv, kv, C.TensorShape([8, 1], I32)], "rank 1")]
    for ins, what in bad:
        with pytest.raises(ValueError, match=what):
            C.infer_output_shapes(op4, ins)
    with pytest.raises(ValueError, match="expected 3 inputs"):
        C.infer_output_shapes(op3, [x, kv, kv, C.TensorShape([8], I32)])


def test_parallel_shape_inference():
    op3, op4 = _ops()
    # batch degree 2, head (replica) degree 2
    x = P([8, 16, 32], [2, 1, 1], 1, 2, F32)
    lens = P([8], [2], 1, 2, I32)
    assert C.infer_parallel_output_shapes(op4, [x, x, x, lens]) == C.infer_parallel_output_shapes(op3, [x, x, x])
    assert C.infer_parallel_weight_shapes(op4, [x, x, x, lens]) == C.infer_parallel_weight_shapes(op3, [x, x, x])
    assert not C.is_valid_parallelization(op4, [x, x, x, P([8], [1], 1, 2, I32)]), "batch degree differs from q"
    assert not C.is_valid_parallelization(op4, [x, x, x, P([8], [2], 1, 1, I32)]), "replica degree differs from q"
    assert not C.is_valid_parallelization(op4, [x, x, x, P([8], [2], 1, 2, F32)]), "not an integer"
    # a sequence degree above 1 is fine without lengths and invalid (not a crash) with them
    s = P([8, 16, 32], [1, 2, 1], 1, 1, F32)
    assert C.is_valid_parallelization(op3, [s, s, s])
    assert not C.is_valid_parallelization(op4, [s, s, s, P([8], [1], 1, 1, I32)])
    with pytest.raises(ValueError, match="unpartitioned sequence"):
        C.infer_parallel_output_shapes(op4, [s, s, s, P([8], [1], 1, 1, I32)])


# ------------------------------------------------------------------ op level
def _weights(E, Hl, kd, g):
    return torch.randn(E * 3 * Hl * kd + Hl * kd * E, generator=g).view(-1, Hl) * 0.3


# fp32 operator against an fp32 reference that sums in another order (20 keys
# against the sample's own count; chains of 32-term dot products of O(1)
# values, each off by up to 32 * 2^-24 of its terms' magnitudes): the tolerance
# of test_attention_dropout.py test_op_gradients_cpu
_F32_OP = dict(rtol=1e-4, atol=1e-5)


def _op(causal):
    return opbase.get_impl("MULTIHEAD_ATTENTION"), opbase.OpContext(
        op_type="MULTIHEAD_ATTENTION", attrs={"embed_dim": 32, "num_heads": 4, "kdim": 0, "vdim": 0, "causal": causal,
                                              "key_lengths": True}, name="mha", training=True)


@pytest.mark.parametrize("causal", [False, True])
def test_torch_path_against_truncated_samples(causal):
    """Cross-attention (the rows of q stay, the keys are cut): sample b with
    its keys cut to lens[b] and no lengths gives the same output rows, the
    same dX of q, the same dX of its live k / v rows, zero for the dead ones
    and, summed over the samples, the same dW.  The padded input rows hold
    other (large, finite) values: they pass through the K / V projections, whose
    weight gradient multiplies them by the zero dK / dV rows."""
    E, Hl, kd, Bn, Sq, Sk = 32, 4, 8, 4, 12, 20
    lens = [20, 7, 1, 13]
    g = torch.Generator().manual_seed(3)
    W = _weights(E, Hl, kd, g)
    x = torch.randn(Bn, Sq, E, generator=g)
    kv = torch.randn(Bn, Sk, E, generator=g)
    dout = torch.randn(Bn, Sq, E, generator=g)
    impl, ctx = _op(causal)
    dirty = kv.clone()
    for b, n in enumerate(lens):
        dirty[b, n:] = 1e3
    dW = torch.zeros_like(W)
    (out,), saved = impl.forward(ctx, [x, dirty, dirty, torch.tensor(lens, dtype=torch.int32)], [W])
    gins = impl.backward(ctx, saved, [dout], [dW], [True, True, True, False])
    assert len(gins) == 4 and gins[3] is None
    assert all(torch.isfinite(t).all() for t in (out, dW, gins[0], gins[1], gins[2]))
    ctx3 = opbase.OpContext(op_type="MULTIHEAD_ATTENTION", attrs=dict(ctx.attrs), name="mha", training=True)
    dW_ref = torch.zeros_like(W)
    for b, n in enumerate(lens):
        xb, kb = x[b:b + 1], kv[b:b + 1, :n]
        (ob,), sb = impl.forward(ctx3, [xb, kb, kb], [W])
        gb = impl.backward(ctx3, sb, [dout[b:b + 1]], [dW_ref], [True, True, True])
        torch.testing.assert_close(out[b:b + 1], ob, **_F32_OP)
        torch.testing.assert_close(gins[0][b:b + 1], gb[0], **_F32_OP)
        for j in (1, 2):
            torch.testing.assert_close(gins[j][b:b + 1, :n], gb[j], **_F32_OP)
            assert (gins[j][b, n:] == 0).all()
    torch.testing.assert_close(dW, dW_ref, rtol=1e-4, atol=1e-5)


def test_torch_path_rows_without_a_live_key():
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(3, 6, 2, 8, generator=g).requires_grad_(True) for _ in range(3))
    lens = torch.tensor([6, 0, 2], dtype=torch.int32)
    o = A._torch_attention(q, k, v, False, 1.0 / math.sqrt(8), None, lens)
    o.sum().backward()
    assert (o[1] == 0).all() and (o[0] != 0).any()
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all() and (t.grad[1] == 0).all()
    assert (k.grad[2, 2:] == 0).all() and (v.grad[2, 2:] == 0).all() and (v.grad[2, :2] != 0).any()


def test_operator_input_errors():
    g = torch.Generator().manual_seed(5)
    W, x = _weights(32, 4, 8, g), torch.randn(2, 8, 32, generator=g)
    impl, ctx = _op(False)
    for lens in (torch.ones(2), torch.ones(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="key lengths"):
            impl.forward(ctx, [x, x, x, lens], [W])
    # the sequence-parallel path has no lengths: an error, not a full-length result
    ctx.extra["seq_group"] = type("Group", (), {"size": 2})()
    with pytest.raises(NotImplementedError, match="key lengths"):
        impl.forward(ctx, [x, x, x, torch.ones(2, dtype=torch.int32)], [W])


# --------------------------------------------------------------- model level
B, S, VOCAB = 8, 16, 64


def _bert_cfg(**kw):
    return BertConfig(vocab_size=VOCAB, hidden_size=32, num_encoder_layers=2, num_heads=4, dim_feedforward=64,
                      sequence_length=S, batch_size=B, max_position_embeddings=S, **kw)


def _bert_batch(pad_id):
    """A padded batch: token ids past each length are `pad_id`, labels there
    are -100 (ignored by the loss)."""
    g = torch.Generator().manual_seed(7)
    lens = torch.tensor([16, 9, 1, 12, 5, 16, 3, 8], dtype=torch.int32)
    live = torch.arange(S).view(1, S) < lens.view(B, 1)
    ids = torch.randint(0, VOCAB, (B, S), generator=g, dtype=torch.int32)
    ids = torch.where(live, ids, torch.full_like(ids, pad_id))
    labels = torch.where(live, torch.randint(0, VOCAB, (B, S), generator=g), torch.full((B, S), -100))
    feeds = {"input_ids": ids, "position_ids": torch.arange(S, dtype=torch.int32).repeat(B, 1),
             "token_type_ids": torch.zeros(B, S, dtype=torch.int32), "seq_lens": lens}
    return feeds, labels, live


def _bert_model(key_lengths, cfg=None):
    cfg = cfg or FFConfig()
    cfg.cpu_only = True
    cfg.print_freq = 0
    m = FFModel(cfg)
    inputs, probs = build_bert(m, _bert_cfg(key_lengths=key_lengths))
    return m, inputs, probs


def _train_bert(pad_id, key_lengths=True, steps=3):
    m, inputs, _ = _bert_model(key_lengths)
    m.compile(optimizer=SGDOptimizer(m, lr=0.5), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    feeds, labels, live = _bert_batch(pad_id)
    if not key_lengths:
        feeds.pop("seq_lens")
    for _ in range(steps):
        ex.train_step(feeds, labels)
    out = ex.forward(feeds, training=False, keep_outputs=True).detach().clone()
    return {n: ex.get_parameter(n).detach().clone() for n in sorted(ex.parameter_names())}, out, live


def test_ffmodel_builds_serialises_and_reloads():
    m, inputs, _ = _bert_model(True)
    assert set(inputs) == {"input_ids", "position_ids", "token_type_ids", "seq_lens"}
    attn = [l for l in m.get_layers() if l.op_type == "MULTIHEAD_ATTENTION"]
    assert len(attn) == 2
    for l in attn:
        ins = m.cg.layer_data_inputs(l.node)
        assert len(ins) == 4 and ins[3] == inputs["seq_lens"].vref
        assert m.cg.shape(ins[3]).dims == [B] and m.cg.shape(ins[3]).dtype == I32
    text = m.cg.to_json()
    again = C.ComputationGraph.from_json(text)
    assert again.to_json() == text
    assert len(again.layer_data_inputs(attn[0].node)) == 4
    # the default builds the graph it built before: three inputs, no new attribute
    m0, inputs0, _ = _bert_model(False)
    assert "seq_lens" not in inputs0 and "key_lengths" not in m0.cg.to_json()
    assert all(len(m0.cg.layer_data_inputs(l.node)) == 3 for l in m0.get_layers()
               if l.op_type == "MULTIHEAD_ATTENTION")


def test_bert_with_key_lengths_ignores_the_padded_token_ids():
    pa, oa, live = _train_bert(pad_id=0)
    pb, ob, _ = _train_bert(pad_id=VOCAB - 1)
    moved = max(float((pa[n] - pb[n]).abs().max()) for n in pa if n != "embeddings.word.kernel")
    assert moved == 0.0, "the padded ids reached the weights"
    assert torch.equal(oa[live], ob[live]), "the padded ids reached a live position"
    assert torch.isfinite(oa).all()
    # without the lengths input the same two batches train different weights
    qa, _, _ = _train_bert(0, key_lengths=False)
    qb, _, _ = _train_bert(VOCAB - 1, key_lengths=False)
    assert max(float((qa[n] - qb[n]).abs().max()) for n in qa) > 1e-4
    assert max(float((qa[n] - pa[n]).abs().max()) for n in qa) > 1e-4


def test_strategy_search_over_a_model_with_lengths():
    from flexflow_train_amd.search import native

    m, _, _ = _bert_model(True)
    attn = [l for l in m.get_layers() if l.op_type == "MULTIHEAD_ATTENTION"][0]
    cands = [json.loads(c) for c in C.candidate_configs(m.cg, attn.node, 8)]
    assert cands and all(c["seq"] == 1 for c in cands), "no sequence-parallel config for a node with lengths"
    assert any(c["kind"] == "heads" for c in cands) and any(c["batch"] == 8 for c in cands)
    cm = native.cost_model()
    cfg = json.dumps({"world": 8, "budget": 100, "time_limit": 20, "seed": 1})
    for pcg, rep in (C.graph_optimize(m.cg, cm, cfg)[:2], C.mcmc_search(m.cg, cm, cfg)[:2],
                     C.unity_search(C.data_parallel_pcg(m.cg, 8), cm, cfg)[:2]):
        rep = json.loads(rep)
        assert math.isfinite(rep["cost"]) and 0 < rep["cost"] <= rep["data_parallel_cost"] * 1.0000001
        pcg.reinfer_shapes()      # every node's parallel shapes are valid
    # the data-parallel lowering shards the lengths with the batch
    dp = json.loads(C.data_parallel_strategy(m.cg, 8))
    pcg, mapping, _ = C.lower_strategy(m.cg, json.dumps(dp), 8)
    node = mapping[attn.node]
    degrees = [pcg.shape(v).shard_degrees() for v in pcg.layer_data_inputs(node)]
    assert degrees == [[8, 1, 1]] * 3 + [[8]]


def lengths_classifier(m):
    """An MHA classifier with a lengths input (module level: the gloo workers import it)."""
    x = m.create_tensor([8, 12, 32], DataType.DT_FLOAT, name="x")
    lens = m.create_tensor([8], DataType.DT_INT32, create_grad=False, name="lens")
    a = m.multihead_attention(x, x, x, 32, 4, name="mha", key_lengths=lens)
    m.softmax(m.dense(a, 6, name="head"), name="sm")
    g = torch.Generator().manual_seed(9)
    feeds = {"x": torch.randn(8, 12, 32, generator=g),
             "lens": torch.tensor([12, 1, 7, 3, 12, 5, 2, 9], dtype=torch.int32)}
    return feeds, torch.randint(0, 6, (8, 12), generator=g, dtype=torch.int32)


def test_two_rank_data_parallel_matches_one_rank():
    single = run_single(lengths_classifier, steps=3)
    multi = run_distributed(lengths_classifier, world=2, steps=3)
    assert_params_close(single["params"], multi["params"])


def test_local_execution_rejects_key_lengths():
    cfg = FFConfig()
    cfg.local_execution = True
    m, _, _ = _bert_model(True, cfg)
    with pytest.raises(ValueError, match="attention key lengths"):
        m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    with pytest.raises(ValueError, match="attention key lengths"):
        C.LocalTrainingBacking(m.cg)
