"""swiglu.hip on the GPU: the element-wise pair and the dual-weight GEMM against fp64 torch on the same inputs,
their refusals, and the tiny LLaMA with the SWIGLU node fused, unfused and graphed.

Bounds: bf16 outputs are within 5e-3 relative Frobenius of fp64 (the project's output-rounding bound,
profiles/r6/g01_tol_probe.jsonl); fp32 outputs within 8x the error of the same formulas evaluated by torch in
fp32 on the CPU (tests/test_rmsnorm_rope_gpu.py's rule).  The model tests take their bound from the same model
with swiglu_op=False, as that file's graphed test takes its bound from a model without the new operators.
"""
import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
_BF = 5e-3


def _rel64(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).norm().item()
    return 0.0 if d == 0.0 else d / max(b.norm().item(), 1e-300)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _formulas(g, u, dy, ct):
    g, u, dy = g.to(ct), u.to(ct), dy.to(ct)
    s = 1 / (1 + torch.exp(-g))
    return g * s * u, dy * u * s * (1 + g * (1 - s)), dy * g * s


def _halves(M, N, dtype):
    """Two [M, N] halves of a NaN-filled [M, 2N + 8] buffer, and its guard columns."""
    buf = torch.full((M, 2 * N + 8), float("nan"), device=DEV, dtype=dtype)
    return buf[:, :N], buf[:, N:2 * N], buf[:, 2 * N:]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("M,N", [(1, 8), (3, 72), (257, 520)])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_elementwise(dtype, M, N, strided):
    gen = torch.Generator().manual_seed(1000 * M + N)
    g, u, dy = (torch.randn(M, N, generator=gen) * s for s in (2.0, 1.0, 1.0))
    g.view(-1)[:4] = torch.tensor([20.0, -20.0, 90.0, -90.0])
    g, u, dy = (t.to(dtype) for t in (g, u, dy))   # the rounded inputs are the inputs of every evaluation
    want = _formulas(g, u, dy, torch.float64)
    floor = [_rel64(a, b) for a, b in zip(_formulas(g, u, dy, F32), want)]
    n0 = K.STATS["swiglu"]
    if strided:
        gd, ud, gguard = _halves(M, N, dtype)
        gd.copy_(g), ud.copy_(u)
        dg, du, dguard = _halves(M, N, dtype)
        y = K.swiglu_fwd(gd, ud)
        K.swiglu_bwd(dy.to(DEV), gd, ud, dg, du)
        for guard in (gguard, dguard):
            assert torch.equal(_bits(guard), _bits(torch.full_like(guard, float("nan")))), "guard columns written"
        assert torch.equal(_bits(gd), _bits(g.to(DEV))) and torch.equal(_bits(ud), _bits(u.to(DEV)))
    else:
        y = K.swiglu_fwd(g.to(DEV), u.to(DEV))
        dg, du = K.swiglu_bwd(dy.to(DEV), g.to(DEV), u.to(DEV))
    assert K.STATS["swiglu"] == n0 + 2
    for name, got, ref, fl in zip(("y", "dgate", "dup"), (y, dg, du), want, floor):
        err, bound = _rel64(got, ref), (_BF if dtype == BF16 else 8 * fl)
        print(f"swiglu {name} {str(dtype)[6:]} [{M}, {N}] strided={int(strided)}: {err:.3e} (bound {bound:.3e})")
        assert torch.isfinite(got).all(), name
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("M,N,Kd", [(1, 8, 8), (130, 72, 72), (257, 136, 200), (64, 64, 1024)])
def test_gemm_swiglu(M, N, Kd, strided):
    from flexflow_train_amd.ops.gemm import matmul

    gen = torch.Generator().manual_seed(M + N + Kd)
    x = torch.randn(M, Kd, generator=gen).to(BF16)
    wg, wu = ((torch.randn(Kd, N, generator=gen) * Kd ** -0.5).to(BF16) for _ in range(2))
    g64, u64 = x.double() @ wg.double(), x.double() @ wu.double()
    want = (g64, u64, torch.nn.functional.silu(g64) * u64)
    wg, wu = wg.to(DEV), wu.to(DEV)
    n0 = K.STATS["gemm_swiglu"]
    if strided:
        xd = torch.full((M, Kd + 8), float("nan"), device=DEV, dtype=BF16)[:, :Kd]
        xd.copy_(x)
        go, uo, guard = _halves(M, N, BF16)
        _, _, y = K.gemm_swiglu(xd, wg, wu, go, uo)
        assert torch.equal(_bits(guard), _bits(torch.full_like(guard, float("nan")))), "guard columns written"
    else:
        xd = x.to(DEV)
        go, uo, y = K.gemm_swiglu(xd, wg, wu)
    assert K.STATS["gemm_swiglu"] == n0 + 1
    for name, got, ref in zip(("gate_out", "up_out", "y"), (go, uo, y), want):
        err = _rel64(got, ref)
        print(f"gemm_swiglu {name} [{M}, {N}, {Kd}] strided={int(strided)}: {err:.3e} (bound {_BF:.0e})")
        assert err <= _BF, (name, err)
    for name, got, w in (("gate_out", go, wg), ("up_out", uo, wu)):
        err = _rel64(got, matmul(xd, w))
        print(f"gemm_swiglu {name} vs matmul [{M}, {N}, {Kd}] strided={int(strided)}: {err:.3e}")
        assert err <= _BF, (name, err)


def test_refusals_launch_nothing():
    def t(*shape, dtype=BF16):
        return torch.zeros(*shape, device=DEV, dtype=dtype)

    off = torch.zeros(16 * 8 + 8, device=DEV, dtype=BF16)[4:4 + 16 * 8].view(16, 8)   # 8 bytes past an aligned base
    snap = dict(K.STATS)
    bad = [lambda: K.gemm_swiglu(t(16, 8), t(8, 12), t(8, 12)),                        # N % 8
           lambda: K.gemm_swiglu(t(16, 12), t(12, 8), t(12, 8)),                       # K % 8
           lambda: K.gemm_swiglu(off, t(8, 8), t(8, 8)),                               # misaligned base
           lambda: K.gemm_swiglu(t(16, 8, dtype=F32), t(8, 8, dtype=F32), t(8, 8, dtype=F32)),
           lambda: K.swiglu_fwd(t(16, 12), t(16, 12)),
           lambda: K.swiglu_fwd(off, t(16, 8)),
           lambda: K.swiglu_bwd(t(16, 8), t(16, 8), t(16, 8, dtype=F32)),
           # the C++ entries refuse the same by name (std::invalid_argument), before any launch
           lambda: K.ext().gemm_swiglu(*[t(16, 16).data_ptr()] * 6, 16, 12, 8, 16, 16, 16, 16, 16, 0),
           lambda: K.ext().swiglu_fwd(K.DT_BF16, *[t(16, 16).data_ptr()] * 3, 16, 12, 16, 16, 16, 0)]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
    assert not K.gemm_swiglu_supported(t(16, 8), t(8, 12), t(8, 12)) and K.gemm_swiglu_supported(t(16, 8), t(8, 8), t(8, 8))
    assert dict(K.STATS) == snap, "a refused call launched or counted something"


# ---------------------------------------------------------------------- model
def _llama(swiglu_op, fuse=True):
    from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType
    from flexflow_train_amd.models.llama import LlamaConfig, build_llama

    cfg = FFConfig()
    cfg.perform_fusion = fuse
    m = FFModel(cfg)
    build_llama(m, LlamaConfig(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
                               intermediate_size=512, sequence_length=64, batch_size=2, swiglu_op=swiglu_op))
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == BF16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.1
                         + (1.0 if n.endswith("gamma") else 0.0))
    return ex


def _batch():
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 256, (2, 65), generator=g, dtype=torch.int32)
    return {"input_ids": ids[:, :64].contiguous().to(DEV)}, ids[:, 1:].long().contiguous().to(DEV)


def _params(ex):
    torch.cuda.synchronize()
    return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}


def _worst(p, q):
    return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)


@pytest.mark.parametrize("forward", ["gemm_swiglu", "pair"])
def test_llama_fused_gradients_match_unfused(forward, monkeypatch):
    """Parameter gradients of one forward + backward of the fused step (either forward) against the same
    model with only the gate / up fusion pass switched off, from the same weights: what the strided
    weight-gradient GEMMs, the accumulating dh GEMM and grad_acc produce, in magnitude and not only in sign.
    The two differ by bf16 re-roundings of y and dh, one tensor per layer and direction.  Bound: twice what
    such a re-rounding does to this model's gradients where none of the new code runs -- swiglu_op=False
    with perform_fusion on against off, which re-rounds the residual sums."""
    from flexflow_train_amd.ops import dense
    from flexflow_train_amd.runtime.executor import Executor

    feeds, labels = _batch()

    def grads(swiglu_op, fuse):
        ex = _llama(swiglu_op, fuse)
        ex.forward(feeds, training=True)
        ex.backward(ex.compute_loss(labels))
        torch.cuda.synchronize()
        return ex, {n: ex.get_parameter_grad(n).double().cpu() for n in sorted(ex.parameter_names())}

    d0 = _worst(grads(False, True)[1], grads(False, False)[1])
    bound = max(2 * d0, 1e-5)
    monkeypatch.setattr(dense, "_swiglu_fused_wins", lambda *a: forward == "gemm_swiglu")
    n0 = {k: K.STATS[k] for k in ("gemm_swiglu", "swiglu")}
    ex, got = grads(True, True)
    kinds = [s.op_type for s in ex.steps]
    assert kinds.count("FUSED_GATE_UP_SWIGLU") == 2 and "SWIGLU" not in kinds
    # two layers: the dual-weight GEMM + swiglu_bwd, or swiglu_fwd + swiglu_bwd
    assert K.STATS["gemm_swiglu"] - n0["gemm_swiglu"] == (2 if forward == "gemm_swiglu" else 0)
    assert K.STATS["swiglu"] - n0["swiglu"] == (2 if forward == "gemm_swiglu" else 4)
    assert all(float(g.norm()) > 0 for g in got.values()), "every parameter has a gradient"
    monkeypatch.setattr(Executor, "_fuse_gate_up_swiglu", lambda self: None)
    ref_ex, want = grads(True, True)
    assert [s.op_type for s in ref_ex.steps].count("SWIGLU") == 2
    d1 = _worst(got, want)
    print(f"llama swiglu fused ({forward}) vs unfused gradients: {d1:.3e}; swiglu_op=False {d0:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)


def test_llama_graphed_step_matches_eager():
    feeds, labels = _batch()

    def eager(swiglu_op):
        ex = _llama(swiglu_op)
        for _ in range(3):
            ex.train_step(feeds, labels)
        return _params(ex)

    def graphed(swiglu_op):
        ex = _llama(swiglu_op)
        step = ex.make_graphed_train_step(feeds, labels, warmup=1)   # one eager step, then two replays
        step(feeds, labels)
        step(feeds, labels)
        return _params(ex)

    d0 = _worst(graphed(False), eager(False))
    bound = max(2 * d0, 1e-5)
    n0 = K.STATS["swiglu"] + K.STATS["gemm_swiglu"]
    want = eager(True)
    assert K.STATS["swiglu"] + K.STATS["gemm_swiglu"] >= n0 + 12   # 3 steps x 2 layers, forward and backward
    d1 = _worst(graphed(True), want)
    print(f"llama swiglu graphed vs eager: {d1:.3e}; swiglu_op=False {d0:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
