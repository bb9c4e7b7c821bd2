"""Column sums of operand ``b`` from the weight-gradient GEMM:
``K.gemmp(a, b, trans_a=True, variant=6, splits=s, bsum=db)`` (gemmt.hip,
``gemmt_kk_kernel<..., BS = true>``).

Shapes: the smallest that reach every way the partition of the sums over the
grid can go wrong.  M = 256 / 264 / 520 gives gm = 1 / 2 / 3 row tiles (the
last one partial); N = 256, 264 (column guard) and 520 (three column tiles);
K = 128 / 320 / 448 is 4 / 10 / 14 k-steps of 32, a multiple and not a
multiple of gm, over 1, 2 and 3 splits (2 / 5 / 7 K-tiles: uneven remainders).
Operands sit in NaN (``_embed``), the output in a sentinel view, ``db`` in a
sentinel 1-D buffer.

Bound on ``db`` (derived): the products with 1.0 are exact, so ``db`` is an
fp32 sum, in some order, of the K values of the column, the starting value
and the partial sums that meet in atomics (at most 2 * gm * splits).  Any
fp32 summation order of n terms errs by at most gamma_(n-1) * sum |terms|,
gamma_m = m u / (1 - m u), u = 2^-24, with n = K + 2 * gm * splits + 1.

C (and so the reduced split-K result) must be bit-identical to the call
without ``bsum``."""
import functools

import pytest
import torch

from flexflow_train_amd import kernels as K
from test_gemm_strided import SENTINEL, _check_linear, _embed, _guard_intact, _guarded, _problem

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
MS, NS, KS, SPLITS = (256, 264, 520), (256, 264, 520), (128, 320, 448), (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _dev_problem(M, N, Kd):
    p = {k: v.to(DEV) for k, v in _problem(M, N, Kd, True, False).items()}
    p["colsum"] = p["b"].double().sum(0)
    p["colabs"] = p["b"].double().abs().sum(0)
    return p


def _embed1d(t):
    buf = torch.full((t.numel() + 16,), SENTINEL, device=t.device, dtype=t.dtype)
    view = buf[8:8 + t.numel()]
    view.copy_(t)
    return view, buf


def _guard1d_intact(buf):
    want = torch.full_like(buf, SENTINEL).view(torch.int32)
    got = buf.view(torch.int32)
    return torch.equal(got[:8], want[:8]) and torch.equal(got[-8:], want[-8:])


def bsum_bound(Kd, gm, splits, absum):
    """gamma_(n-1) * sum |terms| of the module docstring (fp64 tensor)."""
    m = (Kd + 2 * gm * splits + 1) - 1
    u = 2.0 ** -24
    return m * u / (1.0 - m * u) * absum


def _bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32}[t.dtype])


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("Kd", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_bsum_beside_the_weight_gradient(M, N, Kd, splits):
    p = _dev_problem(M, N, Kd)
    a = _embed(p["a"], NAN, "wide")[0]
    b = _embed(p["b"], NAN, "wide")[0]
    gm = (M + 255) // 256
    eff = min(splits, Kd // 64)   # the launcher caps the split count at the K-tile count
    start = 0.25 * torch.arange(N, device=DEV, dtype=F32) + 1.0
    want = start.double() + p["colsum"]
    bound = bsum_bound(Kd, gm, eff, p["colabs"] + start.double().abs())
    for dtype in (BF16, F32):
        for beta in (0.0, 1.0):
            tag = f"{dtype} beta={beta}"
            inside = p["c0"] if beta else None
            c_ref, ref_buf = _guarded((M, N), dtype, DEV, "wide", inside)
            c, c_buf = _guarded((M, N), dtype, DEV, "wide", inside)
            db, db_buf = _embed1d(start)
            before = K.STATS["gemmp"]
            K.gemmp(a, b, trans_a=True, variant=6, splits=splits, out=c_ref, beta=beta)
            K.gemmp(a, b, trans_a=True, variant=6, splits=splits, out=c, beta=beta, bsum=db)
            assert K.STATS["gemmp"] == before + 2
            assert _guard_intact(c_buf, c) and _guard_intact(ref_buf, c_ref), tag
            assert _guard1d_intact(db_buf), tag
            assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(db).all()), tag
            assert torch.equal(_bits(c), _bits(c_ref)), f"{tag}: C differs from the call without bsum"
            ref = p["prod"] + (beta * p["c0"].double() if beta else 0.0)
            _check_linear(c, ref, p["mag"], Kd, tag)
            ratio = ((db.double() - want).abs() / bound).max().item()
            print(f"M={M} N={N} K={Kd} splits={splits} {tag}: worst |db - ref| / bound = {ratio:.4f}")
            assert ratio <= 1.0, f"{tag}: worst |db - ref| / bound = {ratio:.3f}"


def test_bsum_accumulates_over_calls():
    """``+=``: two calls add the column sums twice."""
    M, N, Kd = 264, 264, 320
    p = _dev_problem(M, N, Kd)
    db = torch.zeros(N, device=DEV, dtype=F32)
    out = torch.empty(M, N, device=DEV, dtype=BF16)
    for s in (1, 2):
        K.gemmp(p["a"], p["b"], trans_a=True, variant=6, splits=s, out=out, bsum=db)
    bound = 2 * bsum_bound(Kd, 2, 2, p["colabs"]) + 2.0 ** -23 * p["colabs"]
    assert bool(((db.double() - 2 * p["colsum"]).abs() <= bound).all())


def test_bsum_refusals():
    M, N, Kd = 264, 264, 128
    p = _dev_problem(M, N, Kd)
    a, b = p["a"], p["b"]
    db = torch.zeros(N, device=DEV, dtype=F32)
    out = torch.zeros(M, N, device=DEV, dtype=BF16)
    before = dict(K.STATS)
    for kw in (dict(variant=10), dict(variant=3), dict(variant=6, bias=p["bias"])):
        with pytest.raises(ValueError):
            K.gemmp(a, b, trans_a=True, out=out, bsum=db, **kw)
    with pytest.raises(ValueError):   # A B: no bsum
        K.gemmp(a.t().contiguous(), b, variant=6, out=out, bsum=db)
    with pytest.raises(ValueError):
        K.gemmp(a, b, trans_a=True, variant=6, out=out, bsum=db[:N - 8])
    with pytest.raises(ValueError):
        K.gemmp(a, b, trans_a=True, variant=6, out=out, bsum=db.to(BF16))
    # the native launcher refuses what the wrapper would have caught
    for variant, ta in ((10, True), (4, True), (6, False)):
        aa = a if ta else a.t().contiguous()
        with pytest.raises((ValueError, RuntimeError)):
            K.ext().gemmp(aa.data_ptr(), b.data_ptr(), out.data_ptr(), 0, 0, 0, 0, M, N, Kd, aa.stride(0), b.stride(0),
                          out.stride(0), ta, False, 0, False, 1.0, 0.0, 0, 1, 0, torch.cuda.current_stream().cuda_stream,
                          0, variant, db.data_ptr())
    torch.cuda.synchronize()
    assert dict(K.STATS) == before
    assert not bool(db.any()) and not bool(out.any())
