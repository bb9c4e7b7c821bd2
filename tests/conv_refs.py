"""fp64 CPU references, derived element-wise bounds and the element-wise
assertion shared by the convolution / BatchNorm / pooling suites
(test_conv_geometry.py, test_conv_geometry_gpu.py, test_bnpool_paths_gpu.py).
A plain helper module, like golden_files.py.

Every reference runs in float64 on the CPU, on the same bf16-rounded inputs
the kernel under test gets.

Derived bounds
--------------
u8 = 2^-8 is the unit roundoff of bf16 (8 significand bits, round to nearest:
|round(v) - v| <= 2^-8 |v|); u24 = 2^-24 is that of fp32.

Convolution (conv.hip): the products of bf16 operands are exact in fp32 (8 x 8
significand bits); the MFMA accumulates ``KG`` of them in fp32.  Any summation
order of n fp32 additions has |error| <= (n - 1) u24 sum|terms| + O(u24^2), so
with T = the same convolution of the absolute values the accumulator is
within KG * u24 * T of the exact sum; the bound takes twice that, for the
rounding of the perturbed accumulator (bias add, one more fp32 rounding, then
the bf16 rounding of a value that is not the exact one).  ReLU is
1-Lipschitz, so the bound survives it.

  forward (none, relu)   u8 |ref| + 2 KG u24 T            KG = R S C / groups
  dgrad, beta = 0        u8 |ref| + 2 KG u24 T            KG = R S K / groups
  dgrad, beta != 0       u8 (|ref_conv| + |ref_total|) + 2 KG u24 T
                         (the product is rounded to bf16 before beta * old is
                         added and the sum rounded again)
  wgrad (fp32 output)    2 (N P Q + splits) u24 T         T = wgrad(|x|, |dy|)
                         (N P Q exact products, then one add per split slab
                         and the += into the buffer; no output rounding)

For grouped convolutions the kernels accumulate the block-diagonal expanded
weight's zeros too; KG above counts the non-zero products only, which is all
that can carry error.
"""
import torch
import torch.nn.functional as F

U8 = 2.0 ** -8
U24 = 2.0 ** -24

# Dense bf16 geometries: (N, C, H, W, K, R, S, stride, pad, dil)
DENSE_CASES = [
    (2, 16, 9, 12, 24, 3, 3, (1, 2), (1, 0), (1, 1)),    # asymmetric stride and pad; unreached input pixels
    (2, 16, 11, 9, 24, 3, 3, (2, 1), (0, 1), (1, 1)),    # the H-sharded shape: ph = 0, pw = 1
    (1, 24, 13, 10, 72, 3, 2, (2, 3), (1, 1), (1, 1)),   # C = 24 straddles K-tiles; sh != sw; non-square filter
    (2, 8, 10, 10, 16, 3, 3, (2, 2), (0, 0), (1, 1)),    # last input row and column unreached
    (2, 16, 10, 11, 16, 2, 2, (3, 3), (0, 0), (1, 1)),   # stride > kernel: parity classes without taps
    (1, 16, 7, 7, 16, 1, 1, (1, 1), (2, 2), (1, 1)),     # border outputs see only padding: y = act(bias)
    (2, 16, 12, 12, 24, 3, 3, (1, 1), (2, 2), (2, 2)),   # dilation
    (2, 16, 13, 12, 24, 3, 3, (2, 2), (2, 2), (2, 2)),   # dilation with stride: non-parity strided dgrad
    (1, 32, 9, 14, 40, 2, 3, (1, 2), (1, 3), (1, 3)),    # asymmetric dilation
    (1, 8, 8, 16, 64, 3, 3, (1, 1), (1, 1), (1, 1)),     # M = 128 exactly, BN = 64, C = 8 wraps 8 times per K-tile
    (1, 72, 3, 43, 136, 3, 3, (1, 1), (1, 1), (1, 1)),   # M = 129; last N-tile has 8 columns; KG = 648
    (4, 8, 64, 64, 16, 3, 3, (1, 1), (1, 1), (1, 1)),    # 128 M-tiles: two-pass statistics reduce
]
# Grouped: (N, C, H, W, K, R, S, stride, pad, dil, groups)
GROUPED_CASES = [
    (2, 64, 9, 12, 64, 3, 3, (1, 2), (1, 0), (1, 1), 16),
    (1, 96, 10, 10, 48, 3, 3, (2, 2), (2, 2), (2, 2), 4),
]

ACTS = {"none": lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh,
        "gelu": lambda t: F.gelu(t, approximate="tanh")}


def case_id(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


def conv_inputs(case, seed):
    """bf16 CPU tensors of a case: x [N,C,H,W], w [K,C/groups,R,S] (OIHW), bias [K], dy [N,K,P,Q]."""
    N, C, H, W, Ko, R, S, stride, pad, dil = case[:10]
    groups = case[10] if len(case) > 10 else 1
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Ko, C // groups, R, S, generator=g) / (R * S * C / groups) ** 0.5).to(torch.bfloat16)
    b = (0.1 * torch.randn(Ko, generator=g)).to(torch.bfloat16)
    P = (H + 2 * pad[0] - dil[0] * (R - 1) - 1) // stride[0] + 1
    Q = (W + 2 * pad[1] - dil[1] * (S - 1) - 1) // stride[1] + 1
    dy = torch.randn(N, Ko, P, Q, generator=g).to(torch.bfloat16)
    return x, w, b, dy, dict(stride=stride, padding=pad, dilation=dil, groups=groups)


def conv_fwd_ref(x, w, b, geom):
    """(pre-activation fp64 reference, T = the convolution of absolute values)."""
    xd, wd = x.double(), w.double()
    bd = None if b is None else b.double()
    ref = F.conv2d(xd, wd, bd, **geom)
    T = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), **geom)
    return ref, T


def conv_bwd_ref(x, w, dy, geom):
    """fp64 (dx, dw [OIHW]) from autograd."""
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, **geom).backward(dy.double())
    return xr.grad, wr.grad


def conv_bwd_abs(x, w, dy, geom):
    """(T_dx, T_dw): the gradients' sums of absolute terms (autograd of the
    convolution of absolute values with |dy|)."""
    return conv_bwd_ref(x.abs(), w.abs(), dy.abs(), geom)


def unreached(case):
    """bool [H, W]: input pixels that no window (tap) of the convolution reads,
    from the convolution's own structure (dx of an all-ones problem)."""
    N, C, H, W, Ko, R, S, stride, pad, dil = case[:10]
    x = torch.ones(1, 1, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, torch.ones(1, 1, R, S, dtype=torch.float64), stride=stride, padding=pad, dilation=dil).sum().backward()
    return x.grad[0, 0] == 0


def fwd_bound(ref, T, KG):
    return U8 * ref.abs() + 2 * KG * U24 * T


def dgrad_bound(ref, T, KG):
    return U8 * ref.abs() + 2 * KG * U24 * T


def dgrad_beta_bound(ref_conv, ref_total, T, KG):
    return U8 * (ref_conv.abs() + ref_total.abs()) + 2 * KG * U24 * T


def wgrad_bound(T, npix, splits):
    return 2 * (npix + splits) * U24 * T


def relerr(a, ref):
    """Relative Frobenius error against an fp64 reference (on the CPU)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def worst_ratio(out, ref, tol):
    """max over all elements of |out - ref| / tol (tol > 0 wherever out != ref)."""
    out, ref, tol = out.detach().double().cpu(), ref.detach().double().cpu(), tol.detach().double().cpu()
    err = (out - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return ratio.nan_to_num(nan=float("inf")).max().item()


def assert_elementwise(out, ref, tol, what=""):
    """|out - ref| <= tol at every element (nothing is excluded; a non-finite
    value fails).  On failure names the worst element."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).detach().cpu().expand_as(ref)
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    err = (out - ref).abs()
    bad = ~(err <= tol)          # NaN compares false: it fails
    if bad.any():
        excess = torch.where(bad, (err - tol).nan_to_num(nan=float("inf"), posinf=float("inf")), torch.zeros_like(err))
        flat = int(excess.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements out of bound; worst at {idx}: "
                             f"got {out[idx].item():.9g}, reference {ref[idx].item():.9g}, "
                             f"bound {tol[idx].item():.3g}")


# ---------------------------------------------------------------------------
# BatchNorm, from the formulas in the header of bnpool.hip
def bn_stats_ref(x):
    """fp64 (mean, biased var, rstd-less) per channel of a [N,C,H,W] tensor."""
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    var = (xd * xd).mean((0, 2, 3)) - mean * mean
    return mean, var.clamp_min(0)


def _c(v):
    return v.detach().double().cpu().view(1, -1, 1, 1)


def bn_apply_ref(x, scale, shift, res, relu):
    """(fp64 y = x * scale + shift (+ res) [ReLU], its bound) with the kernel's fp32 scale / shift:
    one bf16 output rounding, and an FMA, an add and the fp32 parameter reads
    (4 roundings, each relative to a term's magnitude)."""
    xd = x.double().cpu()
    xs, sh = xd * _c(scale), _c(shift)
    rd = res.double().cpu() if res is not None else torch.zeros(())
    y = xs + sh + rd
    mag = xs.abs() + sh.abs() + rd.abs()
    if relu:
        y = torch.relu(y)
    return y, U8 * y.abs() + 4 * U24 * mag


def bn_bwd_ref(dy, x, mask, mean, rstd, gamma, s1=None, s2=None):
    """fp64 BatchNorm backward from bf16 dy / x, the kernel's fp32 mean / rstd
    and the ReLU mask (None: no ReLU):
      g = dy * mask, dbeta = sum g, dgamma = sum g * xhat,
      dx = A g + B x + D, A = gamma rstd, B = -A rstd dgamma / M, D = -A dbeta / M - B mean.
    ``s1`` / ``s2``: build dx from these sums (the kernel's own) instead.
    -> dict(g, dbeta, dgamma, rms1, rms2, dx, dx_bound)."""
    g = dy.double().cpu()
    if mask is not None:
        g = g * mask.double().cpu()
    xd = x.double().cpu()
    M = xd.numel() // xd.shape[1]
    xhat = (xd - _c(mean)) * _c(rstd)
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xhat).sum((0, 2, 3))
    gam = torch.ones(xd.shape[1], dtype=torch.float64) if gamma is None else gamma.detach().double().cpu()
    A = _c(gam) * _c(rstd)
    u1 = _c(dbeta if s1 is None else s1)
    u2 = _c(dgamma if s2 is None else s2)
    B = -A * _c(rstd) * u2 / M
    D = -A * u1 / M - B * _c(mean)
    dx = A * g + B * xd + D
    # fp32: A, B, D carry <= 4 roundings each, the two FMAs two more; D's parts may cancel
    mag = (A * g).abs() + (B * xd).abs() + (A * u1 / M).abs() + (B * _c(mean)).abs()
    return dict(g=g, dbeta=dbeta, dgamma=dgamma, A=A, xhat=xhat, M=M, rms1=(g * g).sum((0, 2, 3)).sqrt(),
                rms2=((g * xhat) ** 2).sum((0, 2, 3)).sqrt(), dx=dx, dx_bound=U8 * dx.abs() + 8 * U24 * mag)


# ---------------------------------------------------------------------------
# Pooling
def pool_ref(x, k, s, p, avg, count_pad=False, dy=None):
    """fp64 (y, dx or None) of F.max_pool2d / F.avg_pool2d."""
    xr = x.double().cpu().contiguous().requires_grad_(dy is not None)
    y = F.avg_pool2d(xr, k, s, p, count_include_pad=count_pad) if avg else F.max_pool2d(xr, k, s, p)
    dx = None
    if dy is not None:
        y.backward(dy.double().cpu())
        dx = xr.grad
    return y.detach(), dx


def pool_avg_fwd_bound(x, ref, k, s, p):
    """u8 |ref| + 2^-20 sum|window|: the fp32 sum of <= 256 bf16 values and the division (the
    worst-case (taps + 1) u24 <= 2^-16 relative to sum|window| / taps, written relative to the
    window sum itself)."""
    area = k[0] * k[1]
    return U8 * ref.abs() + 2.0 ** -20 * F.avg_pool2d(x.double().cpu().abs(), k, s, p, count_include_pad=True) * area


def pool_bwd_bound(dy, ref, x_shape, k, s, p, avg):
    """The same shape of bound for the gather over the covering windows: u8 |ref| + 2^-20 sum of
    |dy| over the windows that cover the pixel."""
    dyd = dy.double().cpu().abs()
    xr = torch.zeros(tuple(x_shape), dtype=torch.float64, requires_grad=True)
    # the sum of |dy| over the covering windows = backward of a sum-pool
    (F.avg_pool2d(xr, k, s, p, count_include_pad=True) * (k[0] * k[1])).backward(dyd)
    return U8 * ref.abs() + 2.0 ** -20 * xr.grad
