"""Device-side MoE: routing kernels, grouped (ragged) MFMA GEMMs, the EXPERTS
operator on them, and hipGraph capture of an MoE step.

Bounds: relative Frobenius 5e-3 for bf16 outputs and 1e-5 for fp32 outputs
against fp64 products of the same bf16 inputs (the output-rounding bounds of
tests/test_kernels_gpu.py, profiles/r6/g01_tol_probe.jsonl)."""
import functools

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops import base as opbase
from flexflow_train_amd.ops import moe as moe_mod

pytestmark = pytest.mark.gpu

_BF, _F32 = 5e-3, 1e-5
DEV = "cuda"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _to_dev(r):
    return K.MoeRouting(*[t.to(DEV) if torch.is_tensor(t) else t for t in r])


# ------------------------------------------------------------------ routing
def _ids(B, k, E, unused=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor([e for e in range(E) if e != unused])
    return torch.stack([pool[torch.randperm(len(pool), generator=g)[:k]] for _ in range(B)]).to(torch.int32)


@pytest.mark.parametrize("case", ["unused", "window", "one_token", "one_expert", "multi_block"])
def test_route_matches_reference(case):
    if case == "unused":
        ids, e0, El = _ids(257, 2, 8, unused=5), 0, 8
    elif case == "window":
        ids, e0, El = _ids(257, 2, 8), 2, 3
    elif case == "one_token":
        ids, e0, El = _ids(1, 2, 4), 0, 4
    elif case == "one_expert":
        ids, e0, El = torch.full((300, 2), 3, dtype=torch.int32), 0, 8
    else:   # several routing blocks, more experts than a wave
        ids, e0, El = _ids(1500, 2, 100, unused=17), 10, 80
    ref = K.moe_route_reference(ids, e0, El)
    n = int(ref.offsets[-1])
    if case == "window":
        assert 0 < n < ids.numel() and bool((ref.pos < 0).any())
    dids = ids.to(DEV)
    first = None
    for _ in range(2):
        r = K.moe_route(dids, e0, El)
        torch.cuda.synchronize()
        got = (r.offsets.cpu(), r.perm[:n].cpu(), r.pos.cpu(), r.tile_group.cpu(), r.tile_row0.cpu(), r.n_tiles.cpu())
        want = (ref.offsets, ref.perm[:n], ref.pos, ref.tile_group, ref.tile_row0, ref.n_tiles)
        for name, g, w in zip(("offsets", "perm", "pos", "tile_group", "tile_row0", "n_tiles"), got, want):
            assert torch.equal(g, w), name
        tail = r.perm[n:].cpu()
        assert bool(((tail >= 0) & (tail < ids.numel())).all())
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got))


def test_gather_combine_dgate_colsum():
    torch.manual_seed(3)
    B, k, E, D = 257, 2, 8, 72
    ids = _ids(B, k, E, unused=1)
    ref_r = K.moe_route_reference(ids, 2, 5)            # pairs outside the window: pos = -1
    r = _to_dev(ref_r)
    n = int(ref_r.offsets[-1])
    x = torch.randn(B, D).bfloat16()
    gate = torch.rand(B, k).bfloat16()
    y = torch.randn(B * k, D).bfloat16()
    dout = torch.randn(B, D).bfloat16()
    xs = K.moe_gather_rows(x.to(DEV), r)
    assert torch.equal(xs.cpu(), K.moe_gather_rows_reference(x, ref_r))
    assert not xs[n:].any()
    xg = K.moe_gather_rows(x.to(DEV), r, scale=gate.to(DEV))
    assert torch.equal(xg.cpu(), K.moe_gather_rows_reference(x, ref_r, gate))
    assert _rel(K.moe_combine(y.to(DEV), r, gate.to(DEV)), K.moe_combine_reference(y.double(), ref_r, gate.double())) < _BF
    assert _rel(K.moe_combine(y.to(DEV), r), K.moe_combine_reference(y.double(), ref_r)) < _BF
    dg = K.moe_dgate(dout.to(DEV), y.to(DEV), r)
    dref = (y.double()[ref_r.pos.long().clamp(min=0)] * dout.double().unsqueeze(1)).sum(-1) * (ref_r.pos >= 0)
    assert _rel(dg, dref) < _F32
    assert not dg.cpu()[ref_r.pos < 0].any()
    cs = K.moe_segment_colsum(y.to(DEV), r)
    off = ref_r.offsets.tolist()
    cref = torch.stack([y[off[e]:off[e + 1]].double().sum(0) for e in range(5)])
    assert _rel(cs, cref) < _F32


# ------------------------------------------------------------- grouped GEMM
SIZES = [0, 1, 63, 64, 65, 130, 0]      # empty, one row, tile - 1, tile, tile + 1, tiles + tail, empty
N_ROWS, EXTRA = sum(SIZES), 29          # 323 live rows + 29 pairs that are not local (rows >= n)
SENT = 777.0


@functools.lru_cache(maxsize=None)
def _layout():
    e_of = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    ids = torch.cat([e_of, torch.full((EXTRA,), len(SIZES))]).to(torch.int32).unsqueeze(1)
    ref = K.moe_route_reference(ids, 0, len(SIZES))
    assert ref.offsets.tolist() == [0, 0, 1, 64, 128, 193, 323, 323]
    assert int(ref.n_tiles) == 8 and ref.tile_group.numel() == 13     # more launched tiles than live ones
    return ref, _to_dev(ref)


@functools.lru_cache(maxsize=None)
def _operands(Kd, N):
    g = torch.Generator().manual_seed(Kd * 1000 + N)
    P, E = N_ROWS + EXTRA, len(SIZES)
    rn = lambda *s: (torch.randn(*s, generator=g)).bfloat16()  # noqa: E731
    return {"a": rn(P, Kd), "w": rn(E, Kd, N) * 0.1, "wt": rn(E, N, Kd) * 0.1, "bias": rn(E, N), "g": rn(P, N),
            "aux": rn(P, N)}


def _groups():
    off = _layout()[0].offsets.tolist()
    return [(e, off[e], off[e + 1]) for e in range(len(SIZES))]


def _gelu64(u):
    return torch.nn.functional.gelu(u, approximate="tanh")


def _gelu_grad64(p):
    p = p.clone().requires_grad_(True)
    with torch.enable_grad():
        return torch.autograd.grad(_gelu64(p).sum(), p)[0]


@pytest.mark.parametrize("Kd", [192, 72])
def test_grouped_nn(Kd):
    N = 72
    ref_r, r = _layout()
    o = _operands(Kd, N)
    a, w, bias = o["a"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV)
    P = a.shape[0]
    # plain
    out = torch.full((P, N), SENT, dtype=torch.bfloat16, device=DEV)
    n0 = K.STATS["grouped_gemm"]
    K.grouped_gemm(a, w, r, "nn", out=out)
    assert K.STATS["grouped_gemm"] == n0 + 1
    want = torch.cat([o["a"][lo:hi].double() @ o["w"][e].double() for e, lo, hi in _groups()])
    assert _rel(out[:N_ROWS], want) < _BF
    assert bool((out[N_ROWS:] == SENT).all())          # rows >= n are never written
    # bias + GELU + pre
    out = torch.full((P, N), SENT, dtype=torch.bfloat16, device=DEV)
    pre = torch.full((P, N), SENT, dtype=torch.bfloat16, device=DEV)
    K.grouped_gemm(a, w, r, "nn", bias=bias, act="gelu", pre=pre, out=out)
    u = torch.cat([o["a"][lo:hi].double() @ o["w"][e].double() + o["bias"][e].double() for e, lo, hi in _groups()])
    assert _rel(pre[:N_ROWS], u) < _BF
    assert _rel(out[:N_ROWS], _gelu64(u)) < _BF
    assert bool((out[N_ROWS:] == SENT).all()) and bool((pre[N_ROWS:] == SENT).all())
    # per group too: a row block computed with its neighbour's weight would pass no group-wise bound
    for e, lo, hi in _groups():
        if hi > lo:
            assert _rel(pre[lo:hi], u[lo:hi]) < _BF, e


@pytest.mark.parametrize("Kd", [192, 72])
def test_grouped_nt(Kd):
    N = 72                                               # C [P, N] = G [P, Kd] W[e]^T, W[e] = [N, Kd]
    ref_r, r = _layout()
    o = _operands(Kd, N)
    a, wt, aux = o["a"].to(DEV), o["wt"].to(DEV), o["aux"].to(DEV)
    P = a.shape[0]
    out = torch.full((P, N), SENT, dtype=torch.bfloat16, device=DEV)
    K.grouped_gemm(a, wt, r, "nt", out=out)
    want = torch.cat([o["a"][lo:hi].double() @ o["wt"][e].double().t() for e, lo, hi in _groups()])
    assert _rel(out[:N_ROWS], want) < _BF
    assert bool((out[N_ROWS:] == SENT).all())
    for e, lo, hi in _groups():
        if hi > lo:
            assert _rel(out[lo:hi], want[lo:hi]) < _BF, e
    # activation-gradient epilogue with the per-expert bias gradient
    out = torch.full((P, N), SENT, dtype=torch.bfloat16, device=DEV)
    db = torch.full((len(SIZES), N), SENT, dtype=torch.float32, device=DEV)
    K.grouped_gemm(a, wt, r, "nt", aux=aux, act="gelu", dbias=db, out=out)
    want = want * _gelu_grad64(o["aux"][:N_ROWS].double())
    assert _rel(out[:N_ROWS], want) < _BF
    assert bool((out[N_ROWS:] == SENT).all())
    dbw = torch.stack([want[lo:hi].sum(0) for e, lo, hi in _groups()])
    assert _rel(db, dbw) < _BF                           # sums of the bf16-rounded result
    assert not db[0].any() and not db[6].any()           # empty experts: exact zeros
    exact = torch.stack([out[lo:hi].double().sum(0) for e, lo, hi in _groups()])
    assert _rel(db, exact) < _F32


@pytest.mark.parametrize("Kd", [192, 72])
def test_grouped_tn(Kd):
    N = 72                                               # dW[e] [Kd, N] = A[rows_e]^T G[rows_e]
    ref_r, r = _layout()
    o = _operands(Kd, N)
    a, g = o["a"].to(DEV), o["g"].to(DEV)
    E = len(SIZES)
    want = torch.stack([o["a"][lo:hi].double().t() @ o["g"][lo:hi].double() for e, lo, hi in _groups()])
    live = [e for e, lo, hi in _groups() if hi > lo]
    # beta = 0: fp32 and bf16 outputs, exact zeros for the empty groups
    for dt, tol in ((torch.float32, _F32), (torch.bfloat16, _BF)):
        out = torch.full((E, Kd, N), SENT, dtype=dt, device=DEV)
        K.grouped_gemm(a, g, r, "tn", out=out, beta=0.0)
        assert _rel(out, want) < tol
        for e in live:
            assert _rel(out[e], want[e]) < tol, e
        assert not out[0].any() and not out[6].any()
    # beta = 1 into a pre-filled fp32 buffer; the empty groups' slices stay bit-identical
    base = torch.randn(E, Kd, N, generator=torch.Generator().manual_seed(5))
    out = base.to(DEV)
    K.grouped_gemm(a, g, r, "tn", out=out, beta=1.0)
    assert _rel(out, want + base.double()) < _F32
    assert torch.equal(out[0].cpu(), base[0]) and torch.equal(out[6].cpu(), base[6])
    # ragged contraction: whatever the neighbouring groups hold never enters a group's dW
    for e, lo, hi in _groups():
        if hi == lo:
            continue
        res = []
        for fill in (0.0, 1e4):
            a2, g2 = torch.full_like(a, fill), torch.full_like(g, fill)
            a2[lo:hi], g2[lo:hi] = a[lo:hi], g[lo:hi]
            res.append(K.grouped_gemm(a2, g2, r, "tn", out_dtype=torch.float32)[e].clone())
        assert torch.equal(res[0], res[1]), e
        assert _rel(res[1], want[e]) < _F32, e


# ----------------------------------------------------------------- operator
def _bf(t):
    return t.bfloat16().double()


def _op_problem(act, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, D, H, O, E, k = 96, 64, 128, 72, 5, 2
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ids = _ids(B, k, E, unused=3, seed=seed)
    p = {"x": rn(B, D), "gate": torch.softmax(rn(B, k), -1), "w1": rn(E, D, H) * 0.2, "b1": rn(E, H) * 0.1,
         "w2": rn(E, H, O) * 0.2, "b2": rn(E, O) * 0.1, "dout": rn(B, O)}
    p = {n: t.bfloat16() for n, t in p.items()}
    p["ids"] = ids
    p["act"] = act
    return p


def _op_reference(p):
    """fp64 with bf16 rounding where the operator stores: pre, h, y, out; dy, du, dxs, dx."""
    x, gate, w1, b1, w2, b2, dout = (p[n].double() for n in ("x", "gate", "w1", "b1", "w2", "b2", "dout"))
    ids, act = p["ids"].long(), p["act"]
    B, k = ids.shape
    fwd = _gelu64 if act == "gelu" else torch.relu
    dact = _gelu_grad64 if act == "gelu" else (lambda t: (t > 0).double())
    out = torch.zeros(B, w2.shape[2], dtype=torch.float64)
    dx = torch.zeros_like(x)
    dgate = torch.zeros(B, k, dtype=torch.float64)
    dW1, db1, dW2, db2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    for e in range(w1.shape[0]):
        b, j = (ids == e).nonzero(as_tuple=True)
        if not b.numel():
            continue
        u = x[b] @ w1[e] + b1[e]
        pre, h = _bf(u), _bf(fwd(u))
        y = _bf(h @ w2[e] + b2[e])
        out.index_add_(0, b, y * gate[b, j].unsqueeze(1))
        dgate[b, j] = (dout[b] * y).sum(1)
        dy = _bf(dout[b] * gate[b, j].unsqueeze(1))
        dW2[e], db2[e] = h.t() @ dy, dy.sum(0)
        du = _bf((dy @ w2[e].t()) * dact(pre))
        dW1[e], db1[e] = x[b].t() @ du, du.sum(0)
        dx.index_add_(0, b, _bf(du @ w1[e].t()))
    return {"out": _bf(out), "dx": _bf(dx), "dgate": dgate, "dW1": dW1, "db1": db1, "dW2": dW2, "db2": db2}


def _op_run(p, monkeypatch, grouped, grad_dtype=torch.float32):
    monkeypatch.setenv("FF_MOE_GROUPED", "1" if grouped else "0")
    E, D, H = p["w1"].shape
    O = p["w2"].shape[2]
    impl = opbase.get_impl("EXPERTS")
    ctx = opbase.OpContext(op_type="EXPERTS", attrs={"num_experts": E, "hidden_size": H, "out_dim": O,
                                                      "activation": p["act"], "use_bias": True}, name="moe")
    ws = [p[n].to(DEV) for n in ("w1", "b1", "w2", "b2")]
    outs, saved = impl.forward(ctx, [p["x"].to(DEV), p["ids"].to(DEV), p["gate"].to(DEV)], ws)
    grads = [torch.zeros(w.shape, device=DEV, dtype=grad_dtype) for w in ws]
    gins = impl.backward(ctx, saved, [p["dout"].to(DEV)], grads, [True, False, True])
    torch.cuda.synchronize()
    assert gins[1] is None
    return {"out": outs[0], "dx": gins[0], "dgate": gins[2], "dW1": grads[0], "db1": grads[1], "dW2": grads[2],
            "db2": grads[3]}, saved


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_experts_grouped_vs_per_expert(act, monkeypatch):
    p = _op_problem(act)
    assert 3 not in p["ids"]                                   # one expert unused
    ref = _op_reference(p)
    base, saved_b = _op_run(p, monkeypatch, grouped=False)
    assert saved_b[0] == "rep"
    lib_calls = []
    real = moe_mod.matmul
    monkeypatch.setattr(moe_mod, "matmul", lambda *a, **kw: (lib_calls.append(1), real(*a, **kw))[1])
    before = dict(K.STATS)
    got, saved_g = _op_run(p, monkeypatch, grouped=True)
    assert saved_g[0] == "grouped"
    assert K.STATS["grouped_gemm"] - before.get("grouped_gemm", 0) == 6      # 2 forward + 4 backward
    assert K.STATS["moe_route"] - before.get("moe_route", 0) == 1
    assert not lib_calls                                        # no library GEMM through the operator
    for name in ("blaslt_gemm", "gemm", "gemmp", "gemm256", "bmm", "bias_act_fwd", "act_bwd"):
        assert K.STATS[name] == before.get(name, 0), name
    for name, want in ref.items():
        eg, eb = _rel(got[name], want), _rel(base[name], want)
        print(f"moe_grouped_error act={act} {name}: grouped {eg:.3e} per-expert {eb:.3e}")
        assert eg <= max(1.5 * eb, _BF), (name, eg, eb)


def test_experts_grouped_bf16_weight_grads_accumulate(monkeypatch):
    """acc_grad semantics: the weight gradients are added into the buffers passed in, bf16 too."""
    p = _op_problem("relu", seed=1)
    ref = _op_reference(p)
    monkeypatch.setenv("FF_MOE_GROUPED", "1")
    E, D, H = p["w1"].shape
    O = p["w2"].shape[2]
    impl = opbase.get_impl("EXPERTS")
    ctx = opbase.OpContext(op_type="EXPERTS", attrs={"num_experts": E, "hidden_size": H, "out_dim": O,
                                                      "activation": "relu", "use_bias": True}, name="moe")
    ws = [p[n].to(DEV) for n in ("w1", "b1", "w2", "b2")]
    for dt, tol in ((torch.float32, _BF), (torch.bfloat16, _BF)):       # bf16 du / dy operands; one output rounding
        grads = [torch.ones(w.shape, device=DEV, dtype=dt) for w in ws]
        outs, saved = impl.forward(ctx, [p["x"].to(DEV), p["ids"].to(DEV), p["gate"].to(DEV)], ws)
        impl.backward(ctx, saved, [p["dout"].to(DEV)], grads, [False, False, False])
        for got, name in zip(grads, ("dW1", "db1", "dW2", "db2")):
            assert _rel(got, ref[name] + 1.0) < tol, (name, dt)


# ------------------------------------------------------------------ capture
def test_experts_capture_replays_new_routing(monkeypatch):
    """torch.cuda.graph around ExpertsOp forward + backward; the replay runs on
    a batch whose routing differs from the captured one."""
    monkeypatch.delenv("FF_MOE_GROUPED", raising=False)
    pa, pb = _op_problem("gelu", seed=0), _op_problem("gelu", seed=7)
    ha = torch.bincount(pa["ids"].reshape(-1).long(), minlength=5)
    hb = torch.bincount(pb["ids"].reshape(-1).long(), minlength=5)
    assert not torch.equal(ha, hb)
    E, D, H = pa["w1"].shape
    O = pa["w2"].shape[2]
    impl = opbase.get_impl("EXPERTS")
    ctx = opbase.OpContext(op_type="EXPERTS", attrs={"num_experts": E, "hidden_size": H, "out_dim": O,
                                                      "activation": "gelu", "use_bias": True}, name="moe")
    ws = [pa[n].to(DEV) for n in ("w1", "b1", "w2", "b2")]
    static = {n: pa[n].to(DEV) for n in ("x", "ids", "gate", "dout")}
    grads = [torch.zeros(w.shape, device=DEV, dtype=torch.float32) for w in ws]

    def run():
        for g in grads:
            g.zero_()
        outs, saved = impl.forward(ctx, [static["x"], static["ids"], static["gate"]], ws)
        gins = impl.backward(ctx, saved, [static["dout"]], grads, [True, False, True])
        return outs[0], gins[0], gins[2]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held = run()
    for prob in (pb, pa):
        for n, t in static.items():
            t.copy_(prob[n].to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in held] + [g.clone() for g in grads]
        want = list(run()) + grads                     # eager, same static inputs
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        ref = _op_reference(dict(pa, **{n: prob[n] for n in static}))      # the weights stay pa's
        assert _rel(got[0], ref["out"]) < _BF and _rel(got[3], ref["dW1"]) < _BF


def _moe_classifier():
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType

    m = FFModel(FFConfig())
    x = m.create_tensor([64, 64], DataType.DT_FLOAT, name="input")
    h = m.moe(x, 4, 2, 128, name="moe")
    m.softmax(m.dense(h, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              metrics=[MetricsType.METRICS_ACCURACY])
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.2)
    return ex


def _params(ex):
    torch.cuda.synchronize()
    return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}


def test_moe_model_graphed_step_matches_eager(monkeypatch):
    g = torch.Generator().manual_seed(11)
    xa, xb = torch.randn(64, 64, generator=g), torch.randn(64, 64, generator=g) * 2 + 0.5
    ya, yb = (torch.randint(0, 8, (64, 1), generator=g, dtype=torch.int32) for _ in range(2))
    seen = []
    real_fwd = moe_mod.ExpertsOp.forward

    def spy(self, ctx, inputs, weights):
        if not torch.cuda.is_current_stream_capturing():
            seen.append(inputs[1].detach().clone())
        return real_fwd(self, ctx, inputs, weights)

    def eager():
        ex = _moe_classifier()
        for x, y in ((xa, ya), (xa, ya), (xb, yb)):
            ex.train_step({"input": x.to(DEV)}, y.to(DEV))
        return _params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    # run-to-run difference of the per-expert path on the same inputs sets the bound
    monkeypatch.setenv("FF_MOE_GROUPED", "0")
    d = worst(eager(), eager())
    bound = 2 * d if d > 0 else 1e-5
    monkeypatch.delenv("FF_MOE_GROUPED")

    monkeypatch.setattr(moe_mod.ExpertsOp, "forward", spy)
    want = eager()
    monkeypatch.setattr(moe_mod.ExpertsOp, "forward", real_fwd)
    hist = [torch.bincount(i.reshape(-1).long().cpu(), minlength=4) for i in seen]
    assert len(hist) == 3 and not torch.equal(hist[0], hist[2]), hist     # B routes differently from A

    ex = _moe_classifier()
    n0 = K.STATS["grouped_gemm"]
    step = ex.make_graphed_train_step({"input": xa.to(DEV)}, ya.to(DEV), warmup=1)   # one eager step on A
    assert K.STATS["grouped_gemm"] > n0
    step({"input": xa.to(DEV)}, ya.to(DEV))
    step({"input": xb.to(DEV)}, yb.to(DEV))
    got = _params(ex)
    err = worst(got, want)
    print(f"moe_graphed_vs_eager worst rel {err:.3e} bound {bound:.3e} (per-expert run-to-run {d:.3e})")
    assert err <= bound, (err, bound)
