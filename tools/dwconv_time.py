#!/usr/bin/env python3
"""Time the depthwise convolution kernels (dwconv.hip, HIP events) against the
path a depthwise convolution took before them, on the same tensors in the same
process: K.conv2d_grouped_* (bf16: the 64-group super-group MFMA kernels, given
their pre-expanded weight, so the expansion is not charged to them) and
K.conv32_* (fp32).  Interleaved rounds; medians and the spread (min - max over
the rounds) as JSON lines (tools/rmsnorm_rope_time.py's clock and report).
GB_per_s is the minimal traffic over the median: x + y once for forward and
dgrad, x + dy once for wgrad.

    python tools/dwconv_time.py [rounds]
    python tools/dwconv_time.py --tiny [rounds]     # toy sizes (a rehearsal)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rmsnorm_rope_time import CUDA, DEV, TINY, interleaved, report  # noqa: E402

import torch  # noqa: E402

from flexflow_train_amd import kernels as K  # noqa: E402

# (C, H = W, filter, stride), N = 64, padding "same"
SHAPES = [(32, 112, 3, 1), (144, 56, 3, 2), (384, 14, 3, 1), (960, 7, 3, 1), (96, 56, 7, 1), (384, 14, 7, 1)]


def one(N, C, H, R, st, dtype, rounds, iters):
    stride, pad = (st, st), (R // 2, R // 2)
    gen = torch.Generator().manual_seed(0)
    nhwc = lambda t: t.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    x = nhwc(torch.randn(N, C, H, H, generator=gen))
    w = (torch.randn(C, R, R, 1, generator=gen) / R).to(dtype).to(DEV)
    y = K.dwconv_fwd(x, w, None, stride, pad)
    dy = nhwc(torch.randn(tuple(y.shape), generator=gen))
    dx, dw = torch.empty_like(x), torch.zeros(C * R * R, device=DEV)
    xs = tuple(x.shape)
    new = {"dw_fwd": lambda: K.dwconv_fwd(x, w, None, stride, pad),
           "dw_dgrad": lambda: K.dwconv_dgrad(dy, w, xs, stride, pad, out=dx, beta=0.0),
           "dw_wgrad": lambda: K.dwconv_wgrad(x, dy, dw, R, R, stride, pad)}
    if dtype == torch.bfloat16:
        wexp = K.conv2d_grouped_expand(w, xs, stride, pad, groups=C)
        old = {"old_fwd": lambda: K.conv2d_grouped_fwd(x, w, None, stride, pad, groups=C, wexp=wexp),
               "old_dgrad": lambda: K.conv2d_grouped_dgrad(dy, wexp, tuple(w.shape), xs, stride, pad, groups=C,
                                                           out=dx, beta=0.0),
               "old_wgrad": lambda: K.conv2d_grouped_wgrad(x, dy, dw, R, R, stride, pad, groups=C)}
    else:
        old = {"old_fwd": lambda: K.conv32_fwd(x, w, None, stride, pad, groups=C),
               "old_dgrad": lambda: K.conv32_dgrad(dy, w, xs, stride, pad, groups=C, out=dx, beta=0.0),
               "old_wgrad": lambda: K.conv32_wgrad(x, dy, dw, R, R, stride, pad, groups=C)}
    el = x.element_size()
    traffic = (x.numel() + y.numel()) * el
    nbytes = {f"{side}_{p}": traffic for side in ("dw", "old") for p in ("fwd", "dgrad", "wgrad")}
    for p in ("fwd", "dgrad", "wgrad"):   # each pass against its counterpart, alternating
        t = interleaved({f"dw_{p}": new[f"dw_{p}"], f"old_{p}": old[f"old_{p}"]}, iters, rounds)
        report("dwconv", [N, C, H, H, R, st, str(dtype).split(".")[-1]], t, nbytes)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if not CUDA:
        raise SystemExit("dwconv_time: needs a GPU")
    if TINY:
        one(2, 64, 14, 3, 1, torch.bfloat16, rounds, 3)
        one(2, 64, 14, 3, 1, torch.float32, rounds, 3)
    else:
        for C, H, R, st in SHAPES:
            one(64, C, H, R, st, torch.bfloat16, rounds, 50)
        one(64, 144, 56, 3, 1, torch.float32, rounds, 50)
