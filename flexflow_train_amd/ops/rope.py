"""ROPE: rotary position embedding of the last dim.

The input is read as [outer, S, inner, D]: ``seq_dim`` (default -2, never the
last dim) is the position axis, D the rotary dim.  With c = cos(p * theta^(-2i
/ D)), s = sin(...) for i in [0, D / 2):

* half-split (Hugging Face / NeoX, the default): y[i] = x[i] c - x[i + D/2] s,
  y[i + D/2] = x[i + D/2] c + x[i] s;
* ``interleaved`` (Meta / GPT-J): the same on the pairs (2i, 2i + 1).

No weights and nothing saved: the backward is the rotation of dy by the
negative angle.  bf16 / fp32 on the GPU with D % 16 == 0 runs the RoPE kernel of rmsnorm.hip
(kernels.rope); everything else (CPU, other dtypes, other even D) runs
the same definition in torch from the same fp64-built table.
"""
from __future__ import annotations

import torch

from .. import kernels as K
from .base import OpImpl, register


def _seq_dim(ctx, x) -> int:
    sd = int(ctx.a("seq_dim", -2))
    if not -x.dim() <= sd < x.dim() or sd % x.dim() == x.dim() - 1:
        raise ValueError(f"{ctx.name}: seq_dim must name a dim other than the last")
    return sd % x.dim()


def torch_rope(x, theta: float, seq_dim: int, interleaved: bool, inverse: bool = False):
    """The definition in torch: fp32 math (fp64 for an fp64 input) on the
    table kernels.rope_table builds, one rounding to x's dtype."""
    D = x.shape[-1]
    if D % 2:
        raise ValueError("rope: the rotary dim (last dim) must be even")
    sd = seq_dim % x.dim()
    S = x.shape[sd]
    tab = K.rope_table(S, D, theta, x.device)
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    shape = [1] * x.dim()
    shape[sd], shape[-1] = S, D // 2
    c = tab[..., 0].to(ct).reshape(shape)
    s = tab[..., 1].to(ct).reshape(shape)
    if inverse:
        s = -s
    xf = x.to(ct)
    if interleaved:
        a, b = xf[..., 0::2], xf[..., 1::2]
        y = torch.stack([a * c - b * s, b * c + a * s], dim=-1).reshape(x.shape)
    else:
        a, b = xf[..., :D // 2], xf[..., D // 2:]
        y = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    return y.to(x.dtype)


def _apply(ctx, x, inverse: bool):
    theta = float(ctx.a("theta", 10000.0))
    inter = bool(ctx.a("interleaved", False))
    sd = _seq_dim(ctx, x)
    if (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.shape[-1] % 16 == 0 and x.numel() > 0
            and K.use_hip(x)):
        return K.rope(x.contiguous(), theta, sd, inter, inverse=inverse)
    return torch_rope(x, theta, sd, inter, inverse=inverse)


@register("ROPE")
class RopeOp(OpImpl):
    def forward(self, ctx, inputs, weights):
        x = inputs[0]
        if x.dim() < 2:
            raise ValueError(f"{ctx.name}: needs an input of rank >= 2")
        return [_apply(ctx, x, False)], None

    def backward(self, ctx, saved, grad_outputs, weight_grads, need_input_grad):
        return [_apply(ctx, grad_outputs[0], True)]
