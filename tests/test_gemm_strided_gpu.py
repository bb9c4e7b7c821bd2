"""Every GEMM kernel on strided operands and guarded outputs.

The production dispatcher (ops/gemm.py::matmul) offers row-strided operands
and outputs -- slices of a fused QKV buffer, views of a padded weight, rows of
a concatenated output -- to every hand-written candidate.  Here each launcher
(K.gemm, K.gemm256, every K.gemmp variant, K.gemm_f32 and every candidate the
autotuner would time) runs on operands embedded in NaN and writes into views
embedded in a sentinel, over all four transpose combinations:

  * results are compared per element with the fp64 product of the same values;
  * everything outside the output view must keep its bits;
  * beta == 0 must overwrite a NaN-filled output, and the NaN around the
    operands must leave no trace (in C, in ``pre`` or in the bias gradient);
  * alpha / beta != 1, the sigmoid / tanh epilogues and the layouts that pick
    gemmt's general epilogue and gemmpp's fallback are covered.

Harness, layouts, shapes and the derivation of every bound: the docstring of
test_gemm_strided.py, whose helpers this file shares.
"""
import functools

import pytest
import torch

from flexflow_train_amd import kernels as K
from flexflow_train_amd.ops import gemm as G
from test_gemm_strided import (_ACT64, _BF, _F32X, SENTINEL, SHAPES, TRANS, _check_linear, _embed, _guard_intact,
                               _guarded, _linear_ref, _problem, _rel64)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
ACTS = ["relu", "sigmoid", "tanh", "gelu"]
VARIANTS = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
# (operand layout, output layout)
LAYOUT_PAIRS = [("dense", "dense"), ("wide", "wide"), ("wide", "c4")]
# id, output dtype, alpha, beta, bias
LINEAR = [("plain", BF16, 1.0, 0.0, False), ("plain_f32", F32, 1.0, 0.0, False), ("f32_beta1", F32, 1.0, 1.0, False),
          ("bf16_beta1", BF16, 1.0, 1.0, False), ("general_bf16", BF16, 0.5, 0.5, False),
          ("general_f32", F32, 0.5, 0.5, False), ("bias", BF16, 1.0, 0.0, True)]

# (launcher, gemmp variant, splits): gemm's split-K keeps the fused epilogues,
# gemm256's and gemmp's are plain
TARGETS = [("gemm", None, 1), ("gemm", None, 2), ("gemm256", None, 1), ("gemm256", None, 2)] + \
          [("gemmp", v, 1) for v in VARIANTS]
_tid = lambda t: t[0] + ("" if t[1] is None else f"-v{t[1]}") + (f"-split{t[2]}" if t[2] > 1 else "")


@functools.lru_cache(maxsize=None)
def _dev_problem(M, N, Kd, ta, tb, dtype=BF16):
    return {k: v.to(DEV) for k, v in _problem(M, N, Kd, ta, tb, dtype).items()}


def _embed1d(t, fill):
    """1-D counterpart of ``_embed`` (bias, dbias): 8 elements either side."""
    buf = torch.full((t.numel() + 16,), fill, device=t.device, dtype=t.dtype)
    view = buf[8:8 + t.numel()]
    view.copy_(t)
    return view, buf


def _guard1d_intact(buf):
    want = torch.full_like(buf, SENTINEL).view(torch.int32)
    got = buf.view(torch.int32)
    return torch.equal(got[:8], want[:8]) and torch.equal(got[-8:], want[-8:])


def _call(target, a, b, ta, tb, **kw):
    """One launch of ``target``; asserts through K.STATS that the native kernel ran."""
    kind, variant, splits = target
    splits = kw.pop("splits", splits)
    before = K.STATS[kind]
    if kind == "gemm":
        r = K.gemm(a, b, trans_a=ta, trans_b=tb, splits=splits, **kw)
    elif kind == "gemm256":
        r = K.gemm256(a, b, trans_a=ta, trans_b=tb, splits=splits, **kw)
    else:
        r = K.gemmp(a, b, trans_a=ta, trans_b=tb, splits=splits, variant=variant, **kw)
    assert K.STATS[kind] == before + 1
    return r


def _operands(p, layout):
    return _embed(p["a"], NAN, layout)[0], _embed(p["b"], NAN, layout)[0]


def _run_linear(run, p, M, N, Kd, ab_layout, out_layout, epi, tag, bias_dtype=None):
    """One linear epilogue of LINEAR through ``run(a, b, **kw)``: per-element
    bound, finite inside the view, sentinel intact outside it."""
    name, odt, alpha, beta, with_bias = epi
    a, b = _operands(p, ab_layout)
    out, buf = _guarded((M, N), odt, DEV, out_layout, p["c0"] if beta else None)
    kw = {"alpha": alpha, "beta": beta, "out": out}
    if with_bias:
        kw["bias"] = _embed1d(p["bias"].to(bias_dtype or p["bias"].dtype), NAN)[0]
    r = run(a, b, **kw)
    assert r.data_ptr() == out.data_ptr()
    what = f"{tag} {name} a/b={ab_layout} out={out_layout}"
    _check_linear(out, _linear_ref(p, alpha, beta, with_bias), p["mag"], Kd, what)
    assert _guard_intact(buf, out), f"{what}: wrote outside the output view"


# ---------------------------------------------------------------------------
# bf16 kernels


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,Kd", SHAPES)
@pytest.mark.parametrize("target", TARGETS, ids=_tid)
def test_linear_epilogues(target, M, N, Kd, ta, tb):
    """plain / beta / alpha-beta / bias, bf16 and fp32 outputs, every layout.
    (264, 136, 320) also runs every gemmp variant at splits = 2: five K-tiles,
    an uneven split for gemmt and gemms, reduced to one by the others."""
    p = _dev_problem(M, N, Kd, ta, tb)
    kind, variant, splits = target
    split_degrees = [splits] + ([2] if kind == "gemmp" and Kd == 320 else [])
    for s in split_degrees:
        run = lambda a, b, **kw: _call(target, a, b, ta, tb, splits=s, **kw)
        for ab_layout, out_layout in LAYOUT_PAIRS:
            for epi in LINEAR:
                if epi[4] and s > 1 and kind != "gemm":
                    continue   # split-K with a fused epilogue: test_rejections
                _run_linear(run, p, M, N, Kd, ab_layout, out_layout, epi, f"{_tid(target)} splits={s}")


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,Kd", SHAPES)
@pytest.mark.parametrize("target", [t for t in TARGETS if t[2] == 1 or t[0] == "gemm"], ids=_tid)
def test_activation_epilogues(target, M, N, Kd, ta, tb):
    """bias + pre + activation into a dense (guarded) output, operands wide:
    ``pre`` per element, the activation by the Frobenius bound."""
    p = _dev_problem(M, N, Kd, ta, tb)
    a, b = _operands(p, "wide")
    bias = _embed1d(p["bias"], NAN)[0]
    u = _linear_ref(p, bias=True)
    for act in ACTS:
        out, obuf = _guarded((M, N), BF16, DEV, "dense", None)
        pre, pbuf = _guarded((M, N), BF16, DEV, "dense", None)
        _call(target, a, b, ta, tb, bias=bias, act=act, out=out, pre=pre)
        what = f"{_tid(target)} {act}"
        _check_linear(pre, u, p["mag"], Kd, what + " pre")
        assert bool(torch.isfinite(out).all()), what
        assert _rel64(out, _ACT64[act](u)) < _BF, what
        assert _guard_intact(obuf, out) and _guard_intact(pbuf, pre), what


def _sums_fp32_gradient(variant, act):
    """gemms (8) and gemmt (3 and up, for the activations it instantiates) sum
    the fp32 gradient; every other kernel sums the bf16 values it stored.
    Sigmoid / tanh reach gemmq from every variant but 0, 2 and 8."""
    return variant == 8 or (variant >= 3 and act in ("relu", "gelu"))


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,Kd", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_activation_gradient_epilogue(variant, M, N, Kd, ta, tb):
    """C = (A B) * act'(aux) with the bias gradient accumulated into a dbias
    pre-filled with 0.5; operands wide in NaN (a masked row of a transposed A
    then holds NaN, which a 0/1 multiply would carry into dbias)."""
    p = _dev_problem(M, N, Kd, ta, tb)
    a, b = _operands(p, "wide")
    aux = _embed(p["aux"], NAN, "dense")[0]
    for act in ACTS:
        x = p["aux"].double().requires_grad_(True)
        _ACT64[act](x).backward(torch.ones_like(x))
        gr = p["prod"] * x.grad
        out, obuf = _guarded((M, N), BF16, DEV, "dense", None)
        db, dbuf = _embed1d(torch.full((N,), 0.5, device=DEV, dtype=F32), SENTINEL)
        _call(("gemmp", variant, 1), a, b, ta, tb, act=act, aux=aux, act_bwd=True, dbias=db, out=out)
        what = f"gemmp-v{variant} act_bwd {act}"
        assert bool(torch.isfinite(out).all()), what
        assert _rel64(out, gr) < _BF, what
        assert bool(torch.isfinite(db).all()), what + ": non-finite dbias"
        if _sums_fp32_gradient(variant, act):
            assert _rel64(db, gr.sum(0) + 0.5) < 1e-3, what
        else:
            assert _rel64(db, out.double().sum(0) + 0.5) < 1e-4, what
        assert _guard_intact(obuf, out) and _guard1d_intact(dbuf), what


@pytest.mark.parametrize("dbg", [16, 32], ids=["nontemporal", "lds_staged"])
@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_gemmt_wide_store_variants(M, N, Kd, dbg):
    """gemmt's other two 16-byte store paths (streaming stores; the C tile
    staged through LDS and flushed as whole rows) at 8-byte alignment."""
    p = _dev_problem(M, N, Kd, False, False)
    run = lambda a, b, **kw: _call(("gemmp", 3, 1), a, b, False, False, _dbg=dbg, **kw)
    for ab_layout, out_layout in LAYOUT_PAIRS:
        _run_linear(run, p, M, N, Kd, ab_layout, out_layout, LINEAR[0], f"gemmt dbg={dbg}")


# ---------------------------------------------------------------------------
# exact-fp32 kernel


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,Kd", SHAPES)
@pytest.mark.parametrize("idt", [F32, BF16], ids=["fp32", "bf16"])
def test_gemm_f32(idt, M, N, Kd, ta, tb):
    """K.gemm_f32 through its ``_ld2d`` strides: fp32 operands (fp32 out) and
    bf16 operands (bf16 and fp32 out); bias in the inputs' dtype, ``pre`` in
    the output's."""
    p = _dev_problem(M, N, Kd, ta, tb, idt)

    def run(a, b, **kw):
        before = K.STATS["gemm_f32"]
        r = K.gemm_f32(a, b, ta, tb, **kw)
        assert K.STATS["gemm_f32"] == before + 1
        return r

    for ab_layout, out_layout in LAYOUT_PAIRS:
        for epi in LINEAR:
            if idt == F32 and epi[1] == BF16:   # fp32 operands write fp32: only "bias" has no fp32 twin
                if not epi[4]:
                    continue
                epi = (epi[0] + "_f32", F32) + epi[2:]
            _run_linear(run, p, M, N, Kd, ab_layout, out_layout, epi, f"gemm_f32 {idt}", bias_dtype=idt)
    a, b = _operands(p, "wide")
    bias = _embed1d(p["bias"], NAN)[0]
    u = _linear_ref(p, bias=True)
    for odt in ([F32] if idt == F32 else [BF16, F32]):
        for act in ACTS:
            out, obuf = _guarded((M, N), odt, DEV, "dense", None)
            pre, pbuf = _guarded((M, N), odt, DEV, "dense", None)
            run(a, b, bias=bias, act=act, out=out, pre=pre)
            what = f"gemm_f32 {idt} -> {odt} {act}"
            _check_linear(pre, u, p["mag"], Kd, what + " pre")
            assert bool(torch.isfinite(out).all()), what
            assert _rel64(out, _ACT64[act](u)) < (_F32X if odt == F32 else _BF), what
            assert _guard_intact(obuf, out) and _guard_intact(pbuf, pre), what


# ---------------------------------------------------------------------------
# what the autotuner would time


_HAND_WRITTEN = {"hip", "hip:2", "hip256:1", "p:1", "t:1", "u:1", "v:1", "w:1", "x:1", "s:1", "s:2"}


@pytest.mark.parametrize("ta,tb", [(False, True), (True, False)], ids=["NT", "TN"])
def test_every_dispatch_candidate(ta, tb, monkeypatch):
    """Every entry of ops.gemm._candidates for a strided signature, library
    candidates included (hipBLASLt takes the wide output, not c4)."""
    monkeypatch.setenv("FF_GEMM256", "1")
    M, N, Kd = 264, 136, 320
    p = _dev_problem(M, N, Kd, ta, tb)
    a, b = _operands(p, "wide")
    seen = set()
    for out_layout in ("c4", "wide"):
        for epi in LINEAR:
            name, odt, alpha, beta, with_bias = epi
            if alpha != 1.0:
                continue   # matmul has no alpha
            bias = _embed1d(p["bias"], NAN)[0] if with_bias else None
            probe = _guarded((M, N), odt, DEV, out_layout, None)[0]
            cands = G._candidates(a, b, ta, tb, bias, "none", None, probe, beta)
            seen |= set(cands)
            for cname, fn in cands.items():
                out, buf = _guarded((M, N), odt, DEV, out_layout, p["c0"] if beta else None)
                fn(a, b, ta, tb, bias, "none", out, beta, None)
                what = f"candidate {cname} {name} out={out_layout} ta={ta} tb={tb}"
                _check_linear(out, _linear_ref(p, 1.0, beta, with_bias), p["mag"], Kd, what)
                assert _guard_intact(buf, out), f"{what}: wrote outside the output view"
    want = _HAND_WRITTEN | ({"n:1", "y:1"} if tb and not ta else set()) | (set() if G._LIB_OFF else {"blas"})
    assert want <= seen, f"candidates never offered: {sorted(want - seen)}"


@pytest.mark.parametrize("act", ["none", "gelu", "sigmoid"])
def test_every_dispatch_candidate_writes_pre(act):
    """bias + ``pre`` (+ activation) into dense guarded views, operands wide:
    every candidate, library ones included, must write the pre-activation."""
    M, N, Kd, ta, tb = 264, 136, 320, False, True
    p = _dev_problem(M, N, Kd, ta, tb)
    a, b = _operands(p, "wide")
    bias = _embed1d(p["bias"], NAN)[0]
    u = _linear_ref(p, bias=True)
    probe = [_guarded((M, N), BF16, DEV, "dense", None)[0] for _ in range(2)]
    cands = G._candidates(a, b, ta, tb, bias, act, probe[0], probe[1], 0.0)
    assert {"hip", "p:1", "s:1"} <= set(cands)
    for cname, fn in cands.items():
        out, obuf = _guarded((M, N), BF16, DEV, "dense", None)
        pre, pbuf = _guarded((M, N), BF16, DEV, "dense", None)
        fn(a, b, ta, tb, bias, act, out, 0.0, pre)
        what = f"candidate {cname} {act}"
        _check_linear(pre, u, p["mag"], Kd, what + " pre")
        if act == "none":
            _check_linear(out, u, p["mag"], Kd, what)
        else:
            assert bool(torch.isfinite(out).all()) and _rel64(out, _ACT64[act](u)) < _BF, what
        assert _guard_intact(obuf, out) and _guard_intact(pbuf, pre), what


@pytest.mark.parametrize("act", ["none", "gelu"])
def test_matmul_pre_with_strided_out_leaves_the_kernels(act):
    """``pre`` is indexed with out's row stride by every bf16 kernel, so a
    strided ``out`` with ``pre`` is served by the library path: right values,
    a dense ``pre``, and no hand-written GEMM launched."""
    M, N, Kd = 72, 40, 128
    p = _dev_problem(M, N, Kd, False, True)
    a, b = _operands(p, "wide")
    bias = _embed1d(p["bias"], NAN)[0]
    u = _linear_ref(p, bias=True)
    for out_layout in ("wide", "c4"):
        out, obuf = _guarded((M, N), BF16, DEV, out_layout, None)
        pre, pbuf = _guarded((M, N), BF16, DEV, "dense", None)
        before = {k: K.STATS[k] for k in ("gemm", "gemm256", "gemmp")}
        G.matmul(a, b, trans_b=True, bias=bias, act=act, out=out, pre=pre)
        assert {k: K.STATS[k] for k in before} == before
        _check_linear(pre, u, p["mag"], Kd, f"matmul pre {act} {out_layout}")
        if act == "none":
            _check_linear(out, u, p["mag"], Kd, f"matmul out {out_layout}")
        else:
            assert bool(torch.isfinite(out).all()) and _rel64(out, _ACT64[act](u)) < _BF
        assert _guard_intact(obuf, out) and _guard_intact(pbuf, pre)


# ---------------------------------------------------------------------------
# host-side refusals: nothing here reaches a launch


def test_rejections():
    M, N, Kd = 72, 40, 128
    p = _dev_problem(M, N, Kd, False, False)
    a, b = _operands(p, "wide")
    bias = p["bias"].clone()
    flat = lambda: torch.zeros(M * N, device=DEV, dtype=BF16)
    wide_out = lambda dt=BF16: _guarded((M, N), dt, DEV, "wide", None)[0]
    launchers = {"gemm": K.gemm, "gemm256": K.gemm256, "gemmp": K.gemmp}

    def refused(fn, *args, **kw):
        before = dict(K.STATS)
        with pytest.raises((ValueError, RuntimeError)):
            fn(*args, **kw)
        assert dict(K.STATS) == before

    # lda % 8 != 0 (the base stays 16-byte aligned)
    odd = torch.full((M, Kd + 4), NAN, device=DEV, dtype=BF16)[:, :Kd]
    assert odd.stride(0) % 8 == 4 and odd.data_ptr() % 16 == 0
    # an operand base offset by 4 elements (8 bytes), lda % 8 == 0
    shifted = torch.full((M, Kd + 8), NAN, device=DEV, dtype=BF16)[:, 4:4 + Kd]
    assert shifted.stride(0) % 8 == 0 and shifted.data_ptr() % 16 == 8
    # ldc % 4 != 0
    c2 = torch.zeros(M, N + 2, device=DEV, dtype=BF16)[:, :N]
    for name, fn in launchers.items():
        refused(fn, odd, b)
        refused(fn, shifted, b)
        refused(fn, a, b, out=c2)
        # pre / aux with a strided out: the kernels would index them with ldc
        refused(fn, a, b, bias=bias, act="gelu", out=wide_out(), pre=flat())
    refused(K.gemmp, a, b, act="gelu", aux=flat(), act_bwd=True, out=wide_out())
    # K % 64 != 0 (gemm takes K % 8)
    a72 = torch.zeros(M, 72, device=DEV, dtype=BF16)
    b72 = torch.zeros(72, N, device=DEV, dtype=BF16)
    refused(K.gemm256, a72, b72)
    refused(K.gemmp, a72, b72)
    assert not K.gemm256_supported(a72, b72) and not K.gemmp_supported(a72, b72)
    # split-K with a fused epilogue: the wrappers fall back to one split, the
    # launchers themselves refuse
    out = torch.zeros(M, N, device=DEV, dtype=BF16)
    ws = torch.zeros(2 * M * N, device=DEV, dtype=F32)
    dims = (M, N, Kd, a.stride(0), b.stride(0), N, False, False)
    refused(K.ext().gemm256, a.data_ptr(), b.data_ptr(), out.data_ptr(), bias.data_ptr(), 0, *dims, 0, 1.0, 0.0, 0,
            2, ws.data_ptr(), 0)
    for variant in VARIANTS:
        refused(K.ext().gemmp, a.data_ptr(), b.data_ptr(), out.data_ptr(), bias.data_ptr(), 0, 0, 0, *dims, 0, False,
                1.0, 0.0, 0, 2, ws.data_ptr(), 0, 0, variant)
        # epilogues no kernel of the family has: bias with beta, bias into fp32
        refused(K.gemmp, a, b, bias=bias, beta=1.0, out=torch.zeros(M, N, device=DEV, dtype=BF16), variant=variant)
        refused(K.gemmp, a, b, bias=bias, out=torch.zeros(M, N, device=DEV, dtype=F32), variant=variant)
    assert bool((out == 0).all())
