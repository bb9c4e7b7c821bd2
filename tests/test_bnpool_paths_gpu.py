"""BatchNorm and pooling kernels (csrc/kernels/bnpool.hip) on the paths the
252-row cases of test_conv_gpu.py never reach: the reduce kernel's row loop
(more than 1024 x RL rows) and the apply kernels' vector loops (more than
8192 x 256 vectors of 8: M * C above 16.8 M elements) iterating more than
once, C > 512 with a partly empty second block column,
fewer rows than row lanes, cancellation in E[x^2] - mean^2, bn_stats
(overwrite), fp32 and absent gamma / beta, the FFK_BN_UNROLL = 2 / 4 kernel
templates (in a child process: the variable is read once), max-pooling ties,
asymmetric windows, unreached input pixels, count_pad, need_argmax=False and
grid-stride loops that iterate.

References are fp64 on the CPU from the same bf16 inputs (conv_refs.py), every
comparison is element-wise.  The bounds are the derived ones of conv_refs.py;
the two that cannot be derived (mean and rstd: the order of the atomic bucket
additions) are measured on an MI355X and recorded with their margin in
profiles/conv_bnpool_tolerances.txt.
"""
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":      # the FFK_BN_UNROLL child: the repository root is not on its path
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R
from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5

# 4 x the largest error of the batch statistics against fp64 seen on an MI355X
# over BN_CASES (profiles/conv_bnpool_tolerances.txt, section 2): |mean - ref|
# relative to the channel's rms, |rstd - ref| relative to rstd.  The offset
# input (mean 8, std 0.5) measures 2.54e-5 in rstd: 4 x that is above the 1e-4
# ceiling of a bound, so the case is held to the ceiling itself (3.94 x) and
# reported as a finding in that file: fp32 (sum, sum of squares) statistics
# lose (mean / std)^2 * 1e-7 of rstd to the cancellation in E[x^2] - mean^2.
MEAN_BOUND = 2.3e-7
RSTD_BOUND = 8.1e-7
RSTD_BOUND_OFFSET = 1e-4

# name -> (shape, input (mean, std), parameter dtype or None, rstd bound)
BN_CASES = {
    # 360000 rows at 1024 x 256 row lanes: bn_reduce_kernel's loop iterates twice (the apply
    # kernels' loops do not: 360000 vectors in 1407 blocks)
    "rows360000-c8": ((4, 8, 300, 300), (0.5, 2.0), torch.bfloat16, RSTD_BOUND),
    "rows51200-c64": ((8, 64, 80, 80), (0.5, 2.0), torch.bfloat16, RSTD_BOUND),      # above 1024 * RL rows
    "c520": ((2, 520, 5, 7), (0.5, 2.0), torch.bfloat16, RSTD_BOUND),    # gy = 2, one live group in the second column
    "c1024": ((2, 1024, 3, 5), (0.5, 2.0), torch.bfloat16, RSTD_BOUND),  # C > 512, power-of-two group count
    "rows75-c24": ((3, 24, 5, 5), (0.5, 2.0), torch.bfloat16, RSTD_BOUND),           # fewer rows than row lanes
    "offset": ((8, 64, 80, 80), (8.0, 0.5), torch.bfloat16, RSTD_BOUND_OFFSET),      # cancellation in E[x^2] - mean^2
    "fp32-params": ((3, 24, 9, 7), (0.5, 2.0), torch.float32, RSTD_BOUND),           # param_dtype
    "no-params": ((3, 24, 9, 7), (0.5, 2.0), None, RSTD_BOUND),                      # gamma = beta = None
}
# 18.5 M elements = 2.31 M vectors of 8, above the 8192 x 256 threads of bn_apply_kernel and
# bn_bwd_apply_kernel: their grid-stride loops iterate twice for part of the grid (and the
# reduce kernel's 9 times)
BN_APPLY_LOOP_CASE = ((8, 64, 190, 190), (0.5, 2.0), torch.bfloat16, RSTD_BOUND)
# The FFK_BN_UNROLL children run with both grids capped at 256 workgroups (FFK_BN_RED_BLOCKS,
# FFK_BN_APPLY_BLOCKS), so that at (8, 64, 80, 80) the U-row / U-vector advance of every loop
# (r += U * step, v0 += U * step) is taken: 409600 vectors over 256 x 256 threads is 6.25 per
# thread (two passes of the U = 4 loop, the second partial), 51200 rows over 256 x 32 row
# lanes the same.  Covering it at the default caps would need 67 M elements.
UNROLL_CHILD_ENV = {"FFK_BN_RED_BLOCKS": "256", "FFK_BN_APPLY_BLOCKS": "256"}


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bn_inputs(shape, dist, pdt, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = (torch.randn(shape, generator=g) * dist[1] + dist[0]).to(torch.bfloat16)
    dy = torch.randn(shape, generator=g).to(torch.bfloat16)
    res = torch.randn(shape, generator=g).to(torch.bfloat16)
    gamma = beta = None
    if pdt is not None:
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(pdt)
        beta = (0.1 * torch.randn(C, generator=g)).to(pdt)
    return x, dy, res, gamma, beta


def bn_roundtrip(shape, dist, pdt, rstd_bound, relu, residual=False, check=True):
    """bn_stats -> bn_finalize -> bn_apply -> bn_bwd (mask from y, and for a
    plain ReLU also recomputed from x) against fp64.  Returns the figures
    (errors of mean / rstd, worst error / bound ratios); ``check`` asserts."""
    x, dy, res, gamma, beta = _bn_inputs(shape, dist, pdt)
    if not residual:
        res = None
    C = shape[1]
    M = x.numel() // C
    xd, dyd = _nhwc(x), _nhwc(dy)
    resd = _nhwc(res) if residual else None
    gd = None if gamma is None else gamma.to(DEV)
    bd = None if beta is None else beta.to(DEV)
    fig = {}

    # ---- forward
    stats = torch.zeros(2 * C, device=DEV)
    K.bn_stats(xd, stats)
    scale, shift, mean, rstd = K.bn_finalize(stats, gd, bd, M, EPS)
    y = K.bn_apply(xd, scale, shift, relu, residual=resd)
    mref, vref = R.bn_stats_ref(x)
    rref = 1 / (vref + EPS).sqrt()
    rms = (vref + mref * mref).sqrt()
    fig["mean_err"] = ((mean.double().cpu() - mref).abs() / rms).max().item()
    fig["rstd_err"] = ((rstd.double().cpu() - rref).abs() / rref).max().item()
    gam = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    bet = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    m64, r64 = mean.double().cpu(), rstd.double().cpu()
    sc_ref, sh_ref = gam * r64, bet - m64 * gam * r64
    # scale / shift from the kernel's own mean and rstd: <= 3 fp32 roundings per term
    sc_tol = 4 * R.U24 * sc_ref.abs()
    sh_tol = 4 * R.U24 * (bet.abs() + (m64 * gam * r64).abs())
    y_ref, y_tol = R.bn_apply_ref(x, scale, shift, res, relu)
    fig["y_ratio"] = R.worst_ratio(y, y_ref, y_tol)
    print(f"FIGURE bn fwd {tuple(shape)} relu={relu}: mean_err {fig['mean_err']:.3e} rstd_err {fig['rstd_err']:.3e} "
          f"y_ratio {fig['y_ratio']:.3f}")
    if check:
        assert fig["mean_err"] <= MEAN_BOUND
        assert fig["rstd_err"] <= rstd_bound
        R.assert_elementwise(scale, sc_ref, sc_tol, "scale")
        R.assert_elementwise(shift, sh_ref, sh_tol, "shift")
        R.assert_elementwise(y, y_ref, y_tol, "y")

    # ---- backward
    ss = torch.stack([scale, shift]).reshape(-1).contiguous()
    forms = [("y", 1)] if relu else [("none", 0)]
    if relu and not residual:
        forms.append(("x", 2))
    for form, code in forms:
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        if code == 2:
            dx, dres = K.bn_bwd(dyd, xd, None, mean, rstd, gd, True, dgamma=dg, dbeta=db, scale_shift=ss)
            v = x.double() * scale.double().cpu().view(1, -1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1)
            mask, near = v > 0, v.abs() < 1e-6
        else:
            dx, dres = K.bn_bwd(dyd, xd, y, mean, rstd, gd, relu, dgamma=dg, dbeta=db, want_masked=residual)
            mask, near = (y.cpu() > 0) if relu else None, None
        ref = R.bn_bwd_ref(dy, x, mask, mean, rstd, gamma)
        # dgamma / dbeta: relative 1e-4.  A signed sum of M terms can come out arbitrarily close
        # to zero, where an error relative to its value means nothing, so the error is taken
        # relative to the sum's scale: |ref| plus the rms of its terms, sqrt(sum t^2), which is the
        # size a sum of M such terms has.  A wrong row, group or mask changes a sum by the order
        # of that scale; fp32 accumulation sits near 1e-6 of it.
        g_tol = 1e-4 * (ref["dgamma"].abs() + ref["rms2"])
        b_tol = 1e-4 * (ref["dbeta"].abs() + ref["rms1"])
        # dx = A g + B x + D twice.  With the kernel's own sums in B and D the bound holds only
        # the apply pass's arithmetic (a tight check of bn_bwd_apply_kernel, which reads exactly
        # those sums).  Against the fp64 sums, as the issue specifies, the bound also carries
        # what the sums' own bounds above let through: A (b_tol + |xhat| g_tol) / M.
        own = R.bn_bwd_ref(dy, x, mask, mean, rstd, gamma, s1=db, s2=dg)
        full_tol = own["dx_bound"] + ref["A"].abs() * (b_tol.view(1, -1, 1, 1)
                                                     + ref["xhat"].abs() * g_tol.view(1, -1, 1, 1)) / ref["M"]
        g_ratio = R.worst_ratio(dg, ref["dgamma"], g_tol)
        b_ratio = R.worst_ratio(db, ref["dbeta"], b_tol)
        dxc = dx.double().cpu()
        excluded = 0.0
        if near is not None:
            # the mask is recomputed in fp32: an element may differ only where the fp64 value is within 1e-6 of zero
            excluded = near.double().mean().item()
            dxc = torch.where(near, own["dx"], dxc)
            ref["dx"] = torch.where(near, own["dx"], ref["dx"])
        fig[f"dx_ratio_{form}"] = R.worst_ratio(dxc, own["dx"], own["dx_bound"])
        fig[f"dgamma_ratio_{form}"], fig[f"dbeta_ratio_{form}"] = g_ratio, b_ratio
        print(f"FIGURE bn bwd {tuple(shape)} mask={form}: dgamma_ratio {g_ratio:.3f} dbeta_ratio {b_ratio:.3f} "
              f"dx_ratio {fig[f'dx_ratio_{form}']:.3f} excluded {excluded:.2e}")
        if check:
            assert excluded <= 1e-3
            R.assert_elementwise(dg, ref["dgamma"], g_tol, "dgamma")
            R.assert_elementwise(db, ref["dbeta"], b_tol, "dbeta")
            R.assert_elementwise(dxc, own["dx"], own["dx_bound"], f"dx (mask from {form}, the kernel's sums)")
            R.assert_elementwise(dxc, ref["dx"], full_tol, f"dx (mask from {form}, fp64 sums)")
            if residual:
                assert torch.equal(dres.double().cpu(), ref["g"])      # the masked dy: selected, not computed
            else:
                assert dres is None
    return fig


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name", list(BN_CASES))
def test_batchnorm_paths(name, relu):
    assert max(MEAN_BOUND, RSTD_BOUND, RSTD_BOUND_OFFSET) <= 1e-4      # a larger bound is a finding, not a tolerance
    bn_roundtrip(*BN_CASES[name], relu)


def test_batchnorm_apply_loops_iterate():
    """M * C above 8192 x 256 x 8: the grid-stride loops of bn_apply_kernel and
    bn_bwd_apply_kernel iterate (see BN_APPLY_LOOP_CASE); forward, and the
    backward with the mask from y and from x."""
    shape = BN_APPLY_LOOP_CASE[0]
    assert shape[0] * shape[1] * shape[2] * shape[3] // 8 > 8192 * 256
    bn_roundtrip(*BN_APPLY_LOOP_CASE, True)


def test_batchnorm_residual_and_masked_gradient():
    bn_roundtrip(*BN_CASES["c520"], True, residual=True)


@pytest.mark.parametrize("shape", [(3, 24, 5, 5), (2, 64, 20, 20)])
def test_bn_stats_overwrite(shape):
    """bn_stats(overwrite=True) into a NaN-filled buffer equals the
    add-into-zero form bit for bit.  At most 32 workgroups per channel column
    here, so each of the 16 buckets takes at most two atomic additions and
    their order cannot change the sum."""
    x = _nhwc(_bn_inputs(shape, (0.5, 2.0), None)[0])
    C = shape[1]
    add = torch.zeros(2 * C, device=DEV)
    K.bn_stats(x, add)
    over = torch.full((2 * C,), float("nan"), device=DEV)
    K.bn_stats(x, over, overwrite=True)
    assert torch.equal(add, over)
    xd = x.double().cpu()
    assert R.relerr(over[:C], xd.sum((0, 2, 3))) < 1e-5 and R.relerr(over[C:], (xd * xd).sum((0, 2, 3))) < 1e-5
    K.bn_stats(x, add)          # the default form accumulates
    assert R.relerr(add, 2 * over.double()) < 1e-6


@pytest.mark.parametrize("unroll", [2, 4])
def test_bn_unroll_variants(unroll):
    """The U = 2 / 4 instantiations of the reduce and apply kernels:
    FFK_BN_UNROLL is read once per process, so each runs in a fresh child,
    which prints its worst error / bound ratio.  The children's grids are
    capped so that the U-fold advance of every loop is taken (UNROLL_CHILD_ENV)."""
    env = dict(os.environ, FFK_BN_UNROLL=str(unroll), **UNROLL_CHILD_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BN_UNROLL_WORST")]
    assert len(line) == 1, r.stdout[-2000:]
    _, u, worst, mean_err, rstd_err = line[0].split()
    print(f"FIGURE bn unroll {u}: worst ratio {worst} mean_err {mean_err} rstd_err {rstd_err}")
    assert int(u) == unroll
    assert float(worst) <= 1.0
    assert float(mean_err) <= MEAN_BOUND and float(rstd_err) <= RSTD_BOUND


# ------------------------------------------------------------------- pooling
def _pool_inputs(shape, k, s, p, relu_input=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(torch.bfloat16)
    if relu_input:
        x = torch.relu(x - 1)      # 84 % exact zeros
    P = (shape[2] + 2 * p[0] - k[0]) // s[0] + 1
    Q = (shape[3] + 2 * p[1] - k[1]) // s[1] + 1
    dy = torch.randn((shape[0], shape[1], P, Q), generator=g).to(torch.bfloat16)
    return x, dy


def _pool_check(shape, k, s, p, avg, count_pad=False, relu_input=False):
    x, dy = _pool_inputs(shape, k, s, p, relu_input)
    y, arg = K.pool2d_fwd(_nhwc(x), k, s, p, avg, count_pad=count_pad)
    y_ref, dx_ref = R.pool_ref(x, k, s, p, avg, count_pad, dy=dy)
    assert y.shape == y_ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    if avg:
        assert arg is None
        R.assert_elementwise(y, y_ref, R.pool_avg_fwd_bound(x, y_ref, k, s, p), "y")
    else:
        assert torch.equal(y.double().cpu(), y_ref)       # the bf16 value is selected, not computed
    dx = K.pool2d_bwd(_nhwc(dy), arg, tuple(shape), k, s, p, avg, count_pad=count_pad)
    R.assert_elementwise(dx, dx_ref, R.pool_bwd_bound(dy, dx_ref, shape, k, s, p, avg), "dx")
    return x, y, dx, dx_ref


def test_maxpool_ties_follow_scan_order():
    """A tie decides where the gradient goes only when the maximum itself is
    tied, here when a whole window is zero (y == 0).  On relu(randn - 1), 84 %
    zeros, that is over a fifth of the 2352 windows (asserted: more than a
    tenth).  torch routes such a tie to the first tap in scan order, as the
    kernel's strict > does; a kernel that picked another tap would move those
    windows' whole gradients."""
    x, y, dx, dx_ref = _pool_check((2, 24, 14, 14), (3, 3), (2, 2), (1, 1), False, relu_input=True)
    assert (x == 0).double().mean() > 0.8 and (y == 0).double().mean() > 0.1


@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
def test_pool_asymmetric_window(avg):
    _pool_check((2, 24, 13, 10), (3, 2), (2, 1), (1, 0), avg)


@pytest.mark.parametrize("avg", [False, True], ids=["max", "avg"])
def test_pool_unreached_pixels(avg):
    """k = 3, s = 2, p = 0 on 10 x 10: the last row and column are in no window."""
    x, y, dx, dx_ref = _pool_check((2, 24, 10, 10), (3, 3), (2, 2), (0, 0), avg)
    dx = dx.cpu()
    assert not dx[:, :, 9, :].any() and not dx[:, :, :, 9].any()


@pytest.mark.parametrize("k,s,p", [((3, 3), (1, 1), (1, 1)), ((3, 2), (2, 1), (1, 0))])
def test_avgpool_count_pad(k, s, p):
    _pool_check((2, 24, 13, 10), k, s, p, True, count_pad=True)


def test_maxpool_without_argmax():
    x, _ = _pool_inputs((2, 24, 14, 14), (3, 3), (2, 2), (1, 1))
    xd = _nhwc(x)
    y, arg = K.pool2d_fwd(xd, (3, 3), (2, 2), (1, 1), False)
    y2, arg2 = K.pool2d_fwd(xd, (3, 3), (2, 2), (1, 1), False, need_argmax=False)
    assert arg is not None and arg2 is None
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape,k,s,p,avg", [
    ((4, 64, 260, 260), (2, 2), (2, 2), (0, 0), False),    # backward: 2.16 M threads, above the 8192 x 256 cap
    ((8, 64, 260, 260), (3, 3), (1, 1), (1, 1), True),     # 4.3 M threads in both directions
], ids=["max-2.16M", "avg-4.3M"])
def test_pool_grid_stride_loops(shape, k, s, p, avg):
    _pool_check(shape, k, s, p, avg)


if __name__ == "__main__":
    f = bn_roundtrip(*BN_CASES["rows51200-c64"], True, check=False)
    worst = max(v for k, v in f.items() if k.endswith("ratio") or "_ratio_" in k)
    print(f"BN_UNROLL_WORST {os.environ.get('FFK_BN_UNROLL', '1')} {worst:.4f} {f['mean_err']:.3e} {f['rstd_err']:.3e}")
