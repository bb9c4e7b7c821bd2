"""Gated (SwiGLU) experts on the GPU (moe_swiglu.hip).  Bound: relative Frobenius 5e-3 for bf16 outputs against
fp64 of the same bf16 inputs (as tests/test_moe_grouped_gpu.py); measured errors: profiles/moe_swiglu.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops import base as opbase
from flexflow_train_amd.ops import moe as moe_mod

pytestmark = pytest.mark.gpu

_BF = 5e-3
DEV = "cuda"
NAN = float("nan")
SIZES = [0, 1, 65, 130, 30, 20]     # rows per global expert: unused, one row, crosses a tile, tiles + tail
ROUTINGS = {"all": (0, 5), "window": (1, 3)}    # (e0, El): expert 5's pairs (and 0's, 4's) lie beyond offsets[El]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _bf(t):
    return t.bfloat16().double()


@functools.lru_cache(maxsize=None)
def _route(name):
    e0, El = ROUTINGS[name]
    ids = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES)).to(torch.int32).unsqueeze(1)
    ref = K.moe_route_reference(ids, e0, El)
    assert ref.offsets.tolist()[-1] == sum(SIZES[e0:e0 + El]) < ids.numel()
    return ref, K.MoeRouting(*[t.to(DEV) if torch.is_tensor(t) else t for t in ref])


@pytest.mark.parametrize("routing", list(ROUTINGS))
@pytest.mark.parametrize("D,H,O", [(64, 128, 72), (72, 40, 24)])   # the second: K tail, H < 64, odd H / 8
def test_kernels_against_fp64(D, H, O, routing):
    ref_r, r = _route(routing)
    El, P = ref_r.num_local, ref_r.pairs
    off = ref_r.offsets.tolist()
    n = off[-1]
    g = torch.Generator().manual_seed(D + H)
    xs, w1, w2, dy = (torch.randn(*s, generator=g).bfloat16() for s in ((P, D), (El, D, 2 * H), (El, H, O), (P, O)))
    w1, w2 = (w1 * 0.2).bfloat16(), (w2 * 0.2).bfloat16()
    gu = torch.full((P, 2 * H), NAN, dtype=torch.bfloat16, device=DEV)
    h = torch.full((P, H), NAN, dtype=torch.bfloat16, device=DEV)
    dgu = torch.full((P, 2 * H), NAN, dtype=torch.bfloat16, device=DEV)
    before = dict(K.STATS)
    K.grouped_gemm_swiglu(xs.to(DEV), w1.to(DEV), r, gu, h)
    K.grouped_gemm_swiglu_bwd(dy.to(DEV), w2.to(DEV), r, gu, out=dgu)
    torch.cuda.synchronize()
    moved = {k: v - before.get(k, 0) for k, v in K.STATS.items() if v != before.get(k, 0)}
    assert moved == {"grouped_gemm_swiglu": 1, "grouped_gemm_swiglu_bwd": 1}
    gu, h, dgu = gu.cpu(), h.cpu(), dgu.cpu()
    for t in (gu, h, dgu):      # rows at or beyond offsets[El] are never written, every live row is
        assert bool(t[n:].isnan().all()) and bool(t[:n].isfinite().all())
    want_gu = torch.cat([xs[off[e]:off[e + 1]].double() @ w1[e].double() for e in range(El)])
    dh = torch.cat([dy[off[e]:off[e + 1]].double() @ w2[e].double().t() for e in range(El)])
    gs, us = gu[:n, :H].double(), gu[:n, H:].double()            # kernel B's inputs are the stored g, u
    s = torch.sigmoid(gs)
    pairs = {"g": (gu[:n, :H], want_gu[:, :H]), "u": (gu[:n, H:], want_gu[:, H:]),
             "h": (h[:n], F.silu(want_gu[:, :H]) * want_gu[:, H:]),
             "dg": (dgu[:n, :H], dh * us * s * (1 + gs * (1 - s))), "du": (dgu[:n, H:], dh * gs * s)}
    for name, (got, want) in pairs.items():
        err = _rel(got, want)
        print(f"moe_swiglu_kernel_error D={D} H={H} O={O} {routing} {name}: {err:.3e}")
        assert err <= _BF, (name, err)
        for e in range(El):     # per group too: a block computed with its neighbour's weight passes no group bound
            if off[e + 1] > off[e]:
                assert _rel(got[off[e]:off[e + 1]], want[off[e]:off[e + 1]]) <= _BF, (name, e)


# ----------------------------------------------------------------- operator
def _ids(B, k, E, unused=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor([e for e in range(E) if e != unused])
    return torch.stack([pool[torch.randperm(len(pool), generator=g)[:k]] for _ in range(B)]).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _problem(seed=0):
    g = torch.Generator().manual_seed(seed)
    B, D, H, O, E, k = 96, 64, 128, 72, 5, 2
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = {"x": rn(B, D), "gate": torch.softmax(rn(B, k), -1), "w1": rn(E, D, 2 * H) * 0.2, "w2": rn(E, H, O) * 0.2,
         "dout": rn(B, O)}
    p = {n: t.bfloat16() for n, t in p.items()}
    p["ids"] = _ids(B, k, E, unused=3, seed=seed)
    return p


def _reference(p):
    """fp64 with bf16 rounding where the operator stores: gu, h (from the unrounded g, u), y, out; dy, dgu, dxs, dx."""
    x, gate, w1, w2, dout = (p[n].double() for n in ("x", "gate", "w1", "w2", "dout"))
    ids = p["ids"].long()
    H = w2.shape[1]
    out, dx, dgate = torch.zeros(x.shape[0], w2.shape[2]).double(), torch.zeros_like(x), torch.zeros_like(gate)
    dW1, dW2 = torch.zeros_like(w1), torch.zeros_like(w2)
    for e in range(w1.shape[0]):
        b, j = (ids == e).nonzero(as_tuple=True)
        if not b.numel():
            continue
        r = x[b] @ w1[e]
        gu, h = _bf(r), _bf(F.silu(r[:, :H]) * r[:, H:])
        y = _bf(h @ w2[e])
        out.index_add_(0, b, y * gate[b, j].unsqueeze(1))
        dgate[b, j] = (dout[b] * y).sum(1)
        dy = _bf(dout[b] * gate[b, j].unsqueeze(1))
        dW2[e] = h.t() @ dy
        dh, gs, us = dy @ w2[e].t(), gu[:, :H], gu[:, H:]
        s = torch.sigmoid(gs)
        dgu = _bf(torch.cat([dh * us * s * (1 + gs * (1 - s)), dh * gs * s], 1))
        dW1[e] = x[b].t() @ dgu
        dx.index_add_(0, b, _bf(dgu @ w1[e].t()))
    return {"out": _bf(out), "dx": _bf(dx), "dgate": dgate, "dW1": dW1, "dW2": dW2}


def _ctx(p, use_bias=False):
    E, D, H2 = p["w1"].shape
    attrs = {"num_experts": E, "hidden_size": H2 // 2, "out_dim": p["w2"].shape[2], "activation": "swiglu",
             "use_bias": use_bias}
    return opbase.get_impl("EXPERTS"), opbase.OpContext(op_type="EXPERTS", attrs=attrs, name="moe")


def _run(p):
    impl, ctx = _ctx(p)
    ws = [p["w1"].to(DEV), p["w2"].to(DEV)]
    outs, saved = impl.forward(ctx, [p["x"].to(DEV), p["ids"].to(DEV), p["gate"].to(DEV)], ws)
    grads = [torch.zeros(w.shape, device=DEV, dtype=torch.float32) for w in ws]
    gins = impl.backward(ctx, saved, [p["dout"].to(DEV)], grads, [True, False, True])
    torch.cuda.synchronize()
    return {"out": outs[0], "dx": gins[0], "dgate": gins[2], "dW1": grads[0], "dW2": grads[1]}, saved


@pytest.mark.parametrize("fused", [True, False])
def test_experts_swiglu_vs_per_expert(fused, monkeypatch):
    p = _problem()
    ref = _reference(p)
    monkeypatch.setenv("FF_MOE_GROUPED", "0")
    base, saved_b = _run(p)
    assert saved_b[0] == "rep"
    monkeypatch.setenv("FF_MOE_GROUPED", "1")
    monkeypatch.setenv("FF_MOE_SWIGLU_FUSED", "1" if fused else "0")
    lib_calls = []
    real = moe_mod.matmul
    monkeypatch.setattr(moe_mod, "matmul", lambda *a, **kw: (lib_calls.append(1), real(*a, **kw))[1])
    before = dict(K.STATS)
    got, saved_g = _run(p)
    assert saved_g[0] == "grouped" and not lib_calls
    moved = {k: v - before.get(k, 0) for k, v in K.STATS.items() if v != before.get(k, 0)}
    want_moved = ({"grouped_gemm_swiglu": 1, "grouped_gemm_swiglu_bwd": 1, "grouped_gemm": 4} if fused
                  else {"grouped_gemm": 6, "swiglu": 2})
    assert {k: v for k, v in moved.items() if not k.startswith("moe_")} == want_moved
    assert moved["moe_route"] == 1
    for name, want in ref.items():
        eg, eb = _rel(got[name], want), _rel(base[name], want)
        print(f"moe_swiglu_operator_error fused={fused} {name}: grouped {eg:.3e} per-expert {eb:.3e}")
        assert eg <= max(1.5 * eb, _BF), (name, eg, eb)


def test_capture_replays_new_routing(monkeypatch):
    """torch.cuda.graph around forward + backward; replays on a batch routed differently from the captured one
    are bit-equal to the eager run on the same inputs."""
    monkeypatch.delenv("FF_MOE_GROUPED", raising=False)
    monkeypatch.delenv("FF_MOE_SWIGLU_FUSED", raising=False)
    pa, pb = _problem(0), _problem(7)
    assert not torch.equal(torch.bincount(pa["ids"].reshape(-1)), torch.bincount(pb["ids"].reshape(-1)))
    impl, ctx = _ctx(pa)
    ws = [pa["w1"].to(DEV), pa["w2"].to(DEV)]
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
    for prob in (pb, pa, pb):
        for n, t in static.items():
            t.copy_(prob[n].to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in held] + [g.clone() for g in grads]
        want = list(run()) + grads                     # eager, same static inputs
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert _rel(got[0], _reference(dict(pa, **{n: prob[n] for n in static}))["out"]) < _BF


def test_refusals_before_any_launch():
    p, (ref_r, r) = _problem(), _route("all")
    t = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    P = ref_r.pairs
    impl, ctx_bias = _ctx(p, use_bias=True)
    ins = [p["x"].to(DEV), p["ids"].to(DEV), p["gate"].to(DEV)]
    w1, w2 = p["w1"].to(DEV), p["w2"].to(DEV)
    snap = dict(K.STATS)
    bad = [lambda: impl.forward(ctx_bias, ins, [w1, t(5, 128), w2, t(5, 72)]),           # use_bias=True
           lambda: impl.forward(_ctx(p)[1], ins, [w1[:, :, :128].contiguous(), w2]),     # w1 of width H
           lambda: K.grouped_gemm_swiglu(t(P, 64), t(5, 64, 2 * 36), r),                 # H % 8 != 0
           lambda: K.grouped_gemm_swiglu_bwd(t(P, 24), t(5, 36, 24), r, t(P, 72)),
           lambda: K.grouped_gemm_swiglu(t(P, 64), t(4, 64, 80), r),                     # El differs from the routing
           # the C++ entries refuse the same by name (std::invalid_argument)
           lambda: K.ext().grouped_gemm_swiglu(*[t(64, 64).data_ptr()] * 8, 5, 8, 64, 36, 0),
           lambda: K.ext().grouped_gemm_swiglu_bwd(*[t(64, 64).data_ptr()] * 8, 300, 8, 64, 40, 0)]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
    assert dict(K.STATS) == snap, "a refused call launched or counted something"


# -------------------------------------------------------------------- model
def _moe_llama():
    from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType
    from flexflow_train_amd.models.llama import LlamaConfig, build_llama

    m = FFModel(FFConfig())
    build_llama(m, LlamaConfig(vocab_size=256, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2,
                               intermediate_size=256, sequence_length=32, batch_size=2, num_experts=4,
                               experts_per_token=2))
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.1
                         + (1.0 if n.endswith("gamma") else 0.0))
    return ex


# about 3.5 times the worst relative difference measured between the graphed and the eager step's weights
# (2.85e-8, profiles/moe_swiglu.txt; tests/test_moe_grouped_gpu.py records 6.6e-8 for its MoE classifier)
GRAPHED_BOUND = 1e-7


def test_moe_llama_graphed_step_matches_eager():
    ids = torch.randint(0, 256, (2, 2, 33), generator=torch.Generator().manual_seed(11), dtype=torch.int32)
    (fa, la), (fb, lb) = (({"input_ids": i[:, :32].contiguous().to(DEV)}, i[:, 1:].long().contiguous().to(DEV))
                          for i in ids)

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    ex = _moe_llama()
    start = params(ex)
    for f, l in ((fa, la), (fa, la), (fb, lb)):
        ex.train_step(f, l)
    want = params(ex)
    assert all(not torch.equal(want[n], start[n]) for n in want if "experts" in n or "router" in n)
    ex = _moe_llama()
    n0 = K.STATS["grouped_gemm_swiglu"], K.STATS["grouped_gemm_swiglu_bwd"]
    step = ex.make_graphed_train_step(fa, la, warmup=1)          # one eager step on A
    assert K.STATS["grouped_gemm_swiglu"] > n0[0] and K.STATS["grouped_gemm_swiglu_bwd"] > n0[1]
    step(fa, la)
    step(fb, lb)
    got = params(ex)
    err = max(float((got[n] - want[n]).norm() / want[n].norm()) for n in got)
    print(f"moe_llama_graphed_vs_eager worst rel {err:.3e} bound {GRAPHED_BOUND:.1e}")
    assert err <= GRAPHED_BOUND, err
