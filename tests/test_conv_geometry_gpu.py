"""The bf16 MFMA convolution kernels (csrc/kernels/conv.hip) on the geometries
the square, undilated cases of test_conv_gpu.py / test_conv_grouped_gpu.py
never reach: asymmetric stride / padding / dilation, the non-parity strided
dgrad, parity classes without taps, input pixels no window reaches, exact and
one-past tile sizes, K-tiles a tap changes inside, the two-pass statistics
reduce, every epilogue activation with and without bias.

Every output is compared element by element (conv_refs.assert_elementwise,
nothing excluded) with an fp64 CPU reference of the same bf16-rounded inputs,
under the bounds derived in conv_refs.py, in addition to the project's
Frobenius bounds (5e-3 for bf16 outputs, 1e-5 for fp32 ones).  The
approximate activations (sigmoid via __expf, fast_tanh, gelu_tanh) have a
measured error, recorded with its margin in
profiles/conv_bnpool_tolerances.txt.
"""
import functools

import pytest
import torch

import conv_refs as R
from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"

# Largest |y - ref| of the kernel's approximate activations against the fp64
# reference, measured on an MI355X over the activation cases below:
# profiles/conv_bnpool_tolerances.txt, section 1.  The bound is 2^-8 |ref|
# plus twice the measured value.
ACT_ERR = {"sigmoid": 1.9528e-3, "tanh": 1.9528e-3, "gelu": 7.8044e-3}
ACT_CASES = [R.DENSE_CASES[0], R.DENSE_CASES[6]]


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _krsc(w):
    """OIHW CPU weight -> the kernels' physical [K][R][S][C] on the GPU."""
    return w.permute(0, 2, 3, 1).contiguous().to(DEV)


def _oihw(dw, w):
    """flat fp32 [K][R][S][C] gradient -> OIHW fp64 on the CPU."""
    Ko, Cg, Rr, S = w.shape
    return dw.view(Ko, Rr, S, Cg).permute(0, 3, 1, 2).double().cpu()


@functools.lru_cache(maxsize=None)
def _fwd(case):
    """Inputs and the forward reference of a case, computed once (read-only)."""
    x, w, b, dy, geom = R.conv_inputs(case, 0)
    ref, T = R.conv_fwd_ref(x, w, b, geom)
    return x, w, b, geom, ref, T


@functools.lru_cache(maxsize=None)
def _fwd_nobias(case):
    x, w, b, dy, geom = R.conv_inputs(case, 0)
    return R.conv_fwd_ref(x, w, None, geom)


@functools.lru_cache(maxsize=None)
def _bwd(case):
    x, w, b, dy, geom = R.conv_inputs(case, 1)
    dx, dw = R.conv_bwd_ref(x, w, dy, geom)
    Tx, Tw = R.conv_bwd_abs(x, w, dy, geom)
    return x, w, dy, geom, dx, dw, Tx, Tw


def wgrad_splits(Ko, NG, npix, splits):
    """The number of split-K slabs conv2d_wgrad runs (conv.hip wgrad_plan): the
    request, or for 0 the heuristic (~2048 workgroups, >= 8 K-tiles each),
    clamped to the K-tile count and rounded to whole K-tiles per split."""
    nk = (npix + 63) // 64
    if splits <= 0:
        tiles = ((Ko + 127) // 128) * ((NG + (64 if NG <= 64 else 128) - 1) // (64 if NG <= 64 else 128))
        splits = min((2048 + tiles - 1) // tiles, max(1, nk // 8))
    splits = max(1, min(splits, nk))
    per = (nk + splits - 1) // splits
    return (nk + per - 1) // per


def wgrad_into_half_bound(dw_ref, Tw, npix, eff):
    """The derived wgrad bound, plus the one fp32 rounding of the final
    0.5 + dw (the buffer starts at 0.5, which the test subtracts exactly in
    fp64): 2^-24 (|dw| + 0.5)."""
    return R.wgrad_bound(Tw, npix, eff) + R.U24 * (dw_ref.abs() + 0.5)


def _g(geom):
    return geom["stride"], geom["padding"], geom["dilation"]


def act_bound(act, ref_pre, T, KG):
    """Element-wise bound of act(conv): derived for none / relu, bf16 rounding
    plus twice the measured approximation error for the others."""
    if act in ("none", "relu"):
        return R.fwd_bound(ref_pre, T, KG)
    return R.U8 * R.ACTS[act](ref_pre).abs() + 2 * ACT_ERR[act]


def run_fwd(case, act, bias, stats):
    """(y, stats or None, reference of act(conv), pre-activation reference, T, KG) of one dense forward."""
    x, w, b, geom, ref, T = _fwd(case)
    if not bias:
        ref, T = _fwd_nobias(case)
    Ko, Cg, Rr, S = w.shape
    st = torch.full((2 * Ko,), float("nan"), device=DEV) if stats else None
    y = K.conv2d_fwd(_nhwc(x), _krsc(w), b.to(DEV) if bias else None, *_g(geom), act=act, stats=st)
    return y, st, R.ACTS[act](ref), ref, T, Rr * S * Cg


def _check_stats(stats, y):
    Ko = y.shape[1]
    yd = y.double().cpu()
    assert R.relerr(stats[:Ko], yd.sum((0, 2, 3))) < 1e-5
    assert R.relerr(stats[Ko:], (yd * yd).sum((0, 2, 3))) < 1e-5


# --------------------------------------------------------------------- dense
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_fwd_and_stats(case):
    y, stats, ref, ref_pre, T, KG = run_fwd(case, "relu", True, True)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    R.assert_elementwise(y, ref, act_bound("relu", ref_pre, T, KG), "y")
    assert R.relerr(y, ref) < 5e-3
    _check_stats(stats, y)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_dgrad(case):
    x, w, dy, geom, dx_ref, _, Tx, _ = _bwd(case)
    Ko, Cg, Rr, S = w.shape
    KG = Rr * S * Ko
    un = R.unreached(case)
    dyd, wd = _nhwc(dy), _krsc(w)
    # beta = 0 overwrites whatever the buffer held, the unreached pixels included
    out = _nhwc(torch.full(x.shape, float("nan"), dtype=torch.bfloat16))
    K.conv2d_dgrad(dyd, wd, tuple(x.shape), *_g(geom), out=out, beta=0.0)
    assert torch.isfinite(out).all()
    assert not out.cpu()[:, :, un].any()
    R.assert_elementwise(out, dx_ref, R.dgrad_bound(dx_ref, Tx, KG), "dx")
    assert R.relerr(out, dx_ref) < 5e-3
    # a fresh output buffer gives the same bits
    assert torch.equal(K.conv2d_dgrad(dyd, wd, tuple(x.shape), *_g(geom)), out)
    # beta = 1 into a random base
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    acc = _nhwc(base.clone())
    K.conv2d_dgrad(dyd, wd, tuple(x.shape), *_g(geom), out=acc, beta=1.0)
    total = dx_ref + base.double()
    assert torch.equal(acc.cpu()[:, :, un], base[:, :, un])
    R.assert_elementwise(acc, total, R.dgrad_beta_bound(dx_ref, total, Tx, KG), "dx + base")
    assert R.relerr(acc, total) < 5e-3


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.case_id)
def test_dense_wgrad(case):
    x, w, dy, geom, _, dw_ref, _, Tw = _bwd(case)
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    nk = (npix + 63) // 64
    xd, dyd = _nhwc(x), _nhwc(dy)
    # 0: the heuristic; 64: the two-pass slab reduce where there are that many
    # K-tiles; nk + 5: more splits than K-tiles (clamped)
    for splits in (0, 1, 3, 64, nk + 5):
        dw = torch.full((w.numel(),), 0.5, device=DEV)
        K.conv2d_wgrad(xd, dyd, dw, w.shape[2], w.shape[3], *_g(geom), splits=splits)
        got = _oihw(dw, w) - 0.5
        if npix <= 1024:
            eff = wgrad_splits(w.shape[0], w.shape[1] * w.shape[2] * w.shape[3], npix, splits)
            R.assert_elementwise(got, dw_ref, wgrad_into_half_bound(dw_ref, Tw, npix, eff), f"dw splits={splits}")
        assert R.relerr(got, dw_ref) < 1e-5, splits


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["none", "sigmoid", "tanh", "gelu"])
@pytest.mark.parametrize("case", ACT_CASES, ids=R.case_id)
def test_dense_activations(case, act, bias):
    # the unbiased runs go without the statistics epilogue
    y, stats, ref, ref_pre, T, KG = run_fwd(case, act, bias, stats=bias)
    assert max(ACT_ERR.values()) <= 1e-2      # a larger measured error is a finding, not a tolerance
    err = (y.double().cpu() - ref).abs()
    print(f"FIGURE act {act} {R.case_id(case)} bias={bias}: max error {err.max().item():.4e} "
          f"beyond output rounding {(err - R.U8 * ref.abs()).clamp_min(0).max().item():.1e}")
    R.assert_elementwise(y, ref, act_bound(act, ref_pre, T, KG), f"{act} y")
    assert R.relerr(y, ref) < 5e-3
    if stats is not None:
        _check_stats(stats, y)


# ------------------------------------------------------------------- grouped
@pytest.mark.parametrize("case", R.GROUPED_CASES, ids=R.case_id)
def test_grouped_fwd_and_stats(case):
    x, w, b, geom, ref_pre, T = _fwd(case)
    Ko, Cg, Rr, S = w.shape
    groups = geom["groups"]
    stats = torch.full((2 * Ko,), float("nan"), device=DEV)
    y, wexp = K.conv2d_grouped_fwd(_nhwc(x), _krsc(w), b.to(DEV), *_g(geom), groups=groups, act="relu", stats=stats)
    ref = torch.relu(ref_pre)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    R.assert_elementwise(y, ref, R.fwd_bound(ref_pre, T, Rr * S * Cg), "y")
    assert R.relerr(y, ref) < 5e-3
    _check_stats(stats, y)


@pytest.mark.parametrize("case", R.GROUPED_CASES, ids=R.case_id)
def test_grouped_dgrad_wgrad(case):
    x, w, dy, geom, dx_ref, dw_ref, Tx, Tw = _bwd(case)
    Ko, Cg, Rr, S = w.shape
    groups = geom["groups"]
    KG = Rr * S * Ko // groups
    un = R.unreached(case)
    wp = _krsc(w)
    dyd = _nhwc(dy)
    wexp = K.conv2d_grouped_expand(wp, tuple(x.shape), *_g(geom), groups=groups)
    out = _nhwc(torch.full(x.shape, float("nan"), dtype=torch.bfloat16))
    K.conv2d_grouped_dgrad(dyd, wexp, tuple(wp.shape), tuple(x.shape), *_g(geom), groups=groups, out=out, beta=0.0)
    assert torch.isfinite(out).all()
    assert not out.cpu()[:, :, un].any()
    R.assert_elementwise(out, dx_ref, R.dgrad_bound(dx_ref, Tx, KG), "dx")
    assert R.relerr(out, dx_ref) < 5e-3
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    acc = _nhwc(base.clone())
    K.conv2d_grouped_dgrad(dyd, wexp, tuple(wp.shape), tuple(x.shape), *_g(geom), groups=groups, out=acc, beta=1.0)
    total = dx_ref + base.double()
    assert torch.equal(acc.cpu()[:, :, un], base[:, :, un])
    R.assert_elementwise(acc, total, R.dgrad_beta_bound(dx_ref, total, Tx, KG), "dx + base")
    assert R.relerr(acc, total) < 5e-3
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    dw = torch.full((w.numel(),), 0.5, device=DEV)
    K.conv2d_grouped_wgrad(_nhwc(x), dyd, dw, Rr, S, *_g(geom), groups=groups)
    got = _oihw(dw, w) - 0.5
    assert npix <= 1024
    # the grouped plan's slabs: at most one per K-tile
    R.assert_elementwise(got, dw_ref, wgrad_into_half_bound(dw_ref, Tw, npix, (npix + 63) // 64), "dw")
    assert R.relerr(got, dw_ref) < 1e-5


# ------------------------------------------------------------------ operator
def test_conv_op_asymmetric_attributes():
    """Conv2DOp on the HIP path with stride_h != stride_w and padding_h !=
    padding_w: pins the h / w order of ops/conv.py::_geom."""
    from flexflow_train_amd.ops import conv as CV
    from flexflow_train_amd.ops.base import OpContext

    case = R.DENSE_CASES[1]      # (2, 16, 11, 9) -> 24 filters, stride (2, 1), pad (0, 1)
    x, w, b, geom, ref, T = _fwd(case)
    _, _, dy, _, dx_ref, dw_ref, Tx, Tw = _bwd(case)
    x1, w1 = R.conv_inputs(case, 1)[:2]
    Ko, C, Rr, S = w.shape
    ctx = OpContext("CONV2D", {"kernel_h": Rr, "kernel_w": S, "stride_h": 2, "stride_w": 1, "padding_h": 0,
                               "padding_w": 1}, "c", device=torch.device(DEV), compute_dtype=torch.bfloat16)
    op = CV.Conv2DOp()
    n0 = K.STATS["conv2d_fwd"]
    (y,), saved = op.forward(ctx, [_nhwc(x)], [_krsc(w).reshape(Ko, C, Rr, S), b.to(DEV)])
    assert saved[0] == "hip" and K.STATS["conv2d_fwd"] == n0 + 1
    R.assert_elementwise(y, ref, R.fwd_bound(ref, T, Rr * S * C), "y")
    assert R.relerr(y, ref) < 5e-3
    # backward of the seed-1 problem (its own forward first: the op saves its input)
    (_,), saved = op.forward(ctx, [_nhwc(x1)], [_krsc(w1).reshape(Ko, C, Rr, S), b.to(DEV)])
    dW = torch.zeros(w.numel(), device=DEV)
    db = torch.zeros(Ko, device=DEV)
    (dx,) = op.backward(ctx, saved, [_nhwc(dy)], [dW, db], [True])
    R.assert_elementwise(dx, dx_ref, R.dgrad_bound(dx_ref, Tx, Rr * S * Ko), "dx")
    assert R.relerr(dx, dx_ref) < 5e-3
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    R.assert_elementwise(_oihw(dW, w), dw_ref, R.wgrad_bound(Tw, npix, wgrad_splits(Ko, Rr * S * C, npix, 0)), "dW")
    assert R.relerr(_oihw(dW, w), dw_ref) < 1e-5
    assert R.relerr(db, dy.double().sum((0, 2, 3))) < 1e-5
