"""Per-sample query lengths of MULTIHEAD_ATTENTION off the GPU (attribute
`query_lengths`: the key lengths input also bounds the query axis): the IR
checks, serialisation with and without the attribute, the operator's torch
path against per-sample truncated fp64 attention, NaN in the padding, the
FFModel / BERT interface, the strategy search and the executor that refuses
the node.
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
# the small BERT and its padded batch (labels -100 past each length) of the key-lengths tests
from test_attention_varlen import B, S, VOCAB, _bert_batch, _bert_cfg

F32, I32 = C.DataType.FLOAT, C.DataType.INT32
P = C.ParallelTensorShape


def _op(**kw):
    return C.OpAttrs("MULTIHEAD_ATTENTION", embed_dim=32, num_heads=4, **kw)


# ------------------------------------------------------------------------ IR
def test_serial_shape_inference():
    op3, opq = _op(), _op(key_lengths=True, query_lengths=True)
    x, lens = C.TensorShape([8, 16, 32], F32), C.TensorShape([8], I32)
    assert C.num_data_inputs(opq) == 4 and opq.has("query_lengths")
    assert not op3.has("query_lengths") and not _op(key_lengths=True).has("query_lengths")
    (o,) = C.infer_output_shapes(opq, [x, x, x, lens])
    assert o == C.infer_output_shapes(op3, [x, x, x])[0]
    assert C.infer_weight_shapes(opq, [x, x, x, lens]) == C.infer_weight_shapes(op3, [x, x, x])
    # on a 3-input node: an error, with or without the fourth input offered
    only_q = _op(query_lengths=True)
    assert C.num_data_inputs(only_q) == 3
    with pytest.raises(ValueError, match="query_lengths needs key_lengths"):
        C.infer_output_shapes(only_q, [x, x, x])
    with pytest.raises(ValueError, match="expected 3 inputs"):
        C.infer_output_shapes(only_q, [x, x, x, lens])
    with pytest.raises(ValueError, match="expected 4 inputs"):
        C.infer_output_shapes(opq, [x, x, x])
    # one tensor bounds both axes: the sequence extents must agree
    kv = C.TensorShape([8, 24, 32], F32)
    C.infer_output_shapes(_op(key_lengths=True), [x, kv, kv, lens])
    with pytest.raises(ValueError, match="equal query and key sequence extents"):
        C.infer_output_shapes(opq, [x, kv, kv, lens])


def test_parallel_shape_inference():
    op3, opq = _op(), _op(key_lengths=True, query_lengths=True)
    x = P([8, 16, 32], [2, 1, 1], 1, 2, F32)      # batch degree 2, head (replica) degree 2
    lens = P([8], [2], 1, 2, I32)
    assert C.infer_parallel_output_shapes(opq, [x, x, x, lens]) == C.infer_parallel_output_shapes(op3, [x, x, x])
    assert C.infer_parallel_weight_shapes(opq, [x, x, x, lens]) == C.infer_parallel_weight_shapes(op3, [x, x, x])
    assert C.is_valid_parallelization(opq, [x, x, x, lens])
    assert not C.is_valid_parallelization(opq, [x, x, x, P([8], [1], 1, 2, I32)]), "batch degree differs from q"
    assert not C.is_valid_parallelization(_op(query_lengths=True), [x, x, x]), "no key_lengths"
    kv = P([8, 24, 32], [2, 1, 1], 1, 2, F32)
    assert C.is_valid_parallelization(_op(key_lengths=True), [x, kv, kv, lens])
    assert not C.is_valid_parallelization(opq, [x, kv, kv, lens]), "q / k sequence extents differ"
    with pytest.raises(ValueError, match="equal query and key sequence extents"):
        C.infer_parallel_output_shapes(opq, [x, kv, kv, lens])
    s = P([8, 16, 32], [1, 2, 1], 1, 1, F32)      # a sharded sequence: invalid with lengths, not a crash
    assert not C.is_valid_parallelization(opq, [s, s, s, P([8], [1], 1, 1, I32)])


# graphs of one attention node as the parent commit serialised them
_HEAD = '{"format":"ffmi355x.computation_graph.v1","layers":[{"id":0,"inputs":[],"name":"x","op":{"attrs":' \
        '{"data_type":"float","dims":{"ints":[2,8,16]}},"op_type":"INPUT"},"outputs":[{"create_grad":true,"shape":' \
        '{"data_type":"float","dims":[2,8,16]}}]},'
_LENS = '{"id":1,"inputs":[],"name":"lens","op":{"attrs":{"data_type":"int32","dims":{"ints":[2]}},"op_type":"INPUT"},' \
        '"outputs":[{"create_grad":false,"shape":{"data_type":"int32","dims":[2]}}]},'


def _weights_json(first):
    return ('{"id":%d,"inputs":[],"name":"mha.weight","op":{"attrs":{"data_type":"float","dims":{"ints":[512,2]},'
            '"initializer":"{\\"type\\":\\"glorot_uniform\\",\\"seed\\":0}"},"op_type":"WEIGHT"},"outputs":'
            '[{"create_grad":true,"initializer":{"seed":0,"type":"glorot_uniform"},"shape":{"data_type":"float",'
            '"dims":[512,2]}}]},'
            '{"id":%d,"inputs":[],"name":"mha.input_bias","op":{"attrs":{"data_type":"float","dims":{"ints":[24,2]},'
            '"initializer":"{\\"type\\":\\"zero\\"}"},"op_type":"WEIGHT"},"outputs":[{"create_grad":true,'
            '"initializer":{"type":"zero"},"shape":{"data_type":"float","dims":[24,2]}}]},'
            '{"id":%d,"inputs":[],"name":"mha.output_bias","op":{"attrs":{"data_type":"float","dims":{"ints":[16]},'
            '"initializer":"{\\"type\\":\\"zero\\"}"},"op_type":"WEIGHT"},"outputs":[{"create_grad":true,'
            '"initializer":{"type":"zero"},"shape":{"data_type":"float","dims":[16]}}]},' % (first, first + 1, first + 2))


def _mha_json(node, inputs, attrs):
    return ('{"id":%d,"inputs":%s,"name":"mha","op":{"attrs":{"add_bias_kv":false,"add_zero_attn":false,"bias":true,'
            '"causal":false,"dropout":{"f":0.0},"embed_dim":16,"kdim":0,%s"num_heads":2,"seq_parallel_mode":"auto",'
            '"vdim":0},"op_type":"MULTIHEAD_ATTENTION"},"outputs":[{"create_grad":true,"shape":{"data_type":"float",'
            '"dims":[2,8,16]}}]}]}' % (node, inputs, attrs))


PARENT_3 = _HEAD + _weights_json(1) + _mha_json(4, "[[0,0],[0,0],[0,0],[1,0],[2,0],[3,0]]", "")
PARENT_4 = _HEAD + _LENS + _weights_json(2) + _mha_json(5, "[[0,0],[0,0],[0,0],[1,0],[2,0],[3,0],[4,0]]",
                                                        '"key_lengths":true,')


def _one_node_graph(lengths, query_lengths=False):
    cfg = FFConfig()
    cfg.cpu_only = True
    m = FFModel(cfg)
    x = m.create_tensor([2, 8, 16], DataType.DT_FLOAT, name="x")
    lens = m.create_tensor([2], DataType.DT_INT32, create_grad=False, name="lens") if lengths else None
    m.multihead_attention(x, x, x, 16, 2, name="mha", key_lengths=lens, query_lengths=query_lengths)
    return m


def test_graphs_without_the_attribute_serialise_as_before():
    assert _one_node_graph(False).cg.to_json() == PARENT_3
    assert _one_node_graph(True).cg.to_json() == PARENT_4
    json.loads(PARENT_3), json.loads(PARENT_4)
    # with the attribute: that graph plus the one attribute
    assert _one_node_graph(True, True).cg.to_json() == PARENT_4.replace('"num_heads":2', '"num_heads":2,"query_lengths":true')


def test_ffmodel_interface_serialises_and_reloads():
    m = _one_node_graph(True, True)
    text = m.cg.to_json()
    again = C.ComputationGraph.from_json(text)
    assert again.to_json() == text and '"query_lengths":true' in text
    with pytest.raises(ValueError, match="query_lengths"):
        _one_node_graph(False, True)
    # cross-attention extents differ: refused when the node is added
    cfg = FFConfig()
    cfg.cpu_only = True
    m = FFModel(cfg)
    x = m.create_tensor([2, 8, 16], DataType.DT_FLOAT, name="x")
    kv = m.create_tensor([2, 12, 16], DataType.DT_FLOAT, name="kv")
    lens = m.create_tensor([2], DataType.DT_INT32, create_grad=False, name="lens")
    with pytest.raises(ValueError, match="equal query and key sequence extents"):
        m.multihead_attention(x, kv, kv, 16, 2, name="mha", key_lengths=lens, query_lengths=True)


# ------------------------------------------------------------------ torch path
# fp32 against fp64, sums of at most 96 terms of O(1) values: the tolerance of
# test_attention_varlen.py test_torch_path_against_truncated_samples
_F32_OP = dict(rtol=1e-4, atol=1e-5)
LENS = [96, 33, 64, 1]


def _qkv(seed, Bn=4, Sn=96, Hn=2, Dn=16):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(Bn, Sn, Hn, Dn, generator=g) for _ in range(4)]


def _plain_attention64(q, k, v, causal):
    """softmax(q k^T / sqrt(D)) v of one sample [S, H, D] in fp64, no lengths."""
    qt, kt, vt = (t.transpose(0, 1) for t in (q, k, v))
    s = qt @ kt.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        n = s.shape[-1]
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ vt).transpose(0, 1)


def _run_torch_path(q, k, v, do, lens, causal):
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    lt = torch.tensor(lens, dtype=torch.int32)
    o = A._torch_attention(qs, ks, vs, causal, 1.0 / math.sqrt(q.shape[-1]), None, lt, lt)
    o.backward(do)
    return o.detach(), qs.grad, ks.grad, vs.grad


@pytest.mark.parametrize("causal", [False, True])
def test_torch_path_against_truncated_samples(causal):
    """Sample b cut to lens[b] rows on both axes and run without lengths, in
    fp64, gives the live rows of o, dQ, dK and dV; the dead rows are zero."""
    q, k, v, do = _qkv(21)
    o, dq, dk, dv = _run_torch_path(q, k, v, do, LENS, causal)
    for b, n in enumerate(LENS):
        qb, kb, vb = (t[b, :n].double().requires_grad_(True) for t in (q, k, v))
        ref = _plain_attention64(qb, kb, vb, causal)
        ref.backward(do[b, :n].double())
        for name, got, want in (("o", o, ref.detach()), ("dq", dq, qb.grad), ("dk", dk, kb.grad), ("dv", dv, vb.grad)):
            torch.testing.assert_close(got[b, :n].double(), want, **_F32_OP, msg=lambda m: f"{name}[{b}]: {m}")
            assert (got[b, n:] == 0).all(), (name, b)


@pytest.mark.parametrize("causal", [False, True])
def test_torch_path_nan_in_the_dead_rows(causal):
    """NaN in the dead rows of q, k, v and of the incoming gradient: all
    outputs finite and equal to the run on clean inputs, dead o / dQ rows 0."""
    q, k, v, do = _qkv(22)
    clean = _run_torch_path(q, k, v, do, LENS, causal)
    dirty = [t.clone() for t in (q, k, v, do)]
    for b, n in enumerate(LENS):
        for t in dirty:
            t[b, n:] = float("nan")
    got = _run_torch_path(*dirty, LENS, causal)
    for name, a, c in zip(("o", "dq", "dk", "dv"), got, clean):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, c), name
    for b, n in enumerate(LENS):
        assert (got[0][b, n:] == 0).all() and (got[1][b, n:] == 0).all()
        assert (got[0][b, :n] != 0).any()
        assert n == 1 or (got[1][b, :n] != 0).any()   # one key: its probability is 1 and dQ = 0 exactly


def test_torch_path_length_zero():
    q, k, v, do = _qkv(23, Bn=3, Sn=6, Hn=2, Dn=8)
    o, dq, dk, dv = _run_torch_path(q, k, v, do, [6, 0, 2], False)
    assert (o[1] == 0).all() and (dq[1] == 0).all() and (dk[1] == 0).all() and (dv[1] == 0).all()
    assert (o[0] != 0).any() and (o[2, :2] != 0).any() and (o[2, 2:] == 0).all()
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all()
    # query lengths alone (no key lengths): the dead rows of o / dQ are zero, every key is live
    qs = q.clone().requires_grad_(True)
    o = A._torch_attention(qs, k, v, False, 1.0 / math.sqrt(8), None, None, torch.tensor([6, 0, 2], dtype=torch.int32))
    o.backward(do)
    assert (o[1] == 0).all() and (qs.grad[1] == 0).all() and (o[2, 2:] == 0).all() and (o[2, :2] != 0).any()


def test_operator_attribute_and_sequence_parallel_refusal():
    g = torch.Generator().manual_seed(5)
    W = torch.randn(32 * 3 * 4 * 8 + 4 * 8 * 32, generator=g).view(-1, 4) * 0.3
    x = torch.randn(2, 8, 32, generator=g)
    attrs = {"embed_dim": 32, "num_heads": 4, "kdim": 0, "vdim": 0, "causal": False, "key_lengths": True,
             "query_lengths": True}
    impl = opbase.get_impl("MULTIHEAD_ATTENTION")
    ctx = opbase.OpContext(op_type="MULTIHEAD_ATTENTION", attrs=attrs, name="mha", training=True)
    lens = torch.tensor([8, 3], dtype=torch.int32)
    (out,), _ = impl.forward(ctx, [x, x, x, lens], [W])
    assert (out[1, 3:] == 0).all() and (out[1, :3] != 0).any() and (out[0] != 0).any()   # no bias: o Wo = 0
    with pytest.raises(ValueError, match="query_lengths needs the key lengths"):
        impl.forward(ctx, [x, x, x], [W])
    ctx.extra["seq_group"] = type("Group", (), {"size": 2})()
    with pytest.raises(NotImplementedError, match="lengths are not supported on the sequence-parallel"):
        impl.forward(ctx, [x, x, x, lens], [W])


# --------------------------------------------------------------- model level
def _bert_model(cfg=None, **kw):
    cfg = cfg or FFConfig()
    cfg.cpu_only = True
    cfg.print_freq = 0
    m = FFModel(cfg)
    inputs, probs = build_bert(m, _bert_cfg(**kw))
    return m, inputs, probs


def _train_bert(steps=3, **kw):
    m, _, _ = _bert_model(**kw)
    m.compile(optimizer=SGDOptimizer(m, lr=0.5), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    feeds, labels, live = _bert_batch(0)
    for _ in range(steps):
        ex.train_step(feeds, labels)
    ex.forward(feeds, training=False, keep_outputs=True)
    (step,) = [s for s in ex.steps if s.name == "encoder.0.attn"]
    attn0 = ex._env[step.outputs[0]].detach().clone()
    return {n: ex.get_parameter(n).detach().clone() for n in sorted(ex.parameter_names())}, attn0, live


def test_bert_config_and_graph():
    with pytest.raises(ValueError, match="query_lengths"):
        _bert_model(query_lengths=True)
    assert BertConfig().query_lengths is False and BertConfig().key_lengths is False
    m, inputs, _ = _bert_model(key_lengths=True, query_lengths=True)
    attn = [l for l in m.get_layers() if l.op_type == "MULTIHEAD_ATTENTION"]
    assert len(attn) == 2 and all(len(m.cg.layer_data_inputs(l.node)) == 4 for l in attn)
    text = m.cg.to_json()
    assert text.count('"query_lengths":true') == 2
    assert C.ComputationGraph.from_json(text).to_json() == text
    # off by default: the graph of the key-lengths model is the one built before
    m0, _, _ = _bert_model(key_lengths=True)
    assert "query_lengths" not in m0.cg.to_json()


def test_bert_trains_the_same_weights_with_query_lengths():
    """The loss ignores the padded positions, so skipping them as queries
    changes no gradient: three steps on the same padded batch with key lengths
    only and with query lengths too."""
    pk, ak, live = _train_bert(key_lengths=True)
    pq, aq, _ = _train_bert(key_lengths=True, query_lengths=True)
    assert_params_close(pk, pq)
    assert torch.isfinite(aq).all()
    # a padded position's attention output: o = 0 through the output projection, the bias exactly
    bias = pq["encoder.0.attn.output_bias"]
    assert (~live).any() and torch.equal(aq[~live], bias.expand_as(aq)[~live])
    assert not torch.equal(ak[~live], bias.expand_as(ak)[~live]), "with key lengths only the padded rows are computed"
    torch.testing.assert_close(aq[live], ak[live], rtol=1e-4, atol=1e-5)


def test_strategy_search_over_a_model_with_query_lengths():
    from flexflow_train_amd.search import native

    m, _, _ = _bert_model(key_lengths=True, query_lengths=True)
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
    dp = json.loads(C.data_parallel_strategy(m.cg, 8))
    pcg, mapping, _ = C.lower_strategy(m.cg, json.dumps(dp), 8)
    degrees = [pcg.shape(v).shard_degrees() for v in pcg.layer_data_inputs(mapping[attn.node])]
    assert degrees == [[8, 1, 1]] * 3 + [[8]]


def test_local_execution_rejects_the_node():
    cfg = FFConfig()
    cfg.local_execution = True
    m, _, _ = _bert_model(cfg, key_lengths=True, query_lengths=True)
    with pytest.raises(ValueError, match="attention key lengths"):
        m.compile(optimizer=SGDOptimizer(m, lr=0.1), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    with pytest.raises(ValueError, match="attention key lengths"):
        C.LocalTrainingBacking(m.cg)
