"""MULTIHEAD_ATTENTION operator (projections + flash attention + output proj)
and SDPA, the same attention core without projections (end of this file).

Parity: lib/local-execution/src/ops/attention.cc and lib/kernels/src/cuda/ops/
attention_kernels.cu (cuDNN multi-head attention with fused projections;
weights laid out as [qSize*kdim + kSize*kdim + vSize*vdim + vdim*embed, heads],
op-attrs attention.cc:136-170).

Local-piece layout (head-parallel degree h -> this rank owns Hl = H/h heads):
the logical weight piece [P, Hl] is stored physically as
  self-attention (q/k/v feature sizes equal):
      Wqkv [E, 3, Hl, kdim] (row-major, = one [E, 3*Hl*kdim] GEMM operand)
      Wo   [Hl*vdim, E]
  otherwise: Wq [Eq, Hl*k] | Wk [Ek, Hl*k] | Wv [Ev, Hl*v] | Wo [Hl*v, E]
input bias piece [2k+v, Hl] -> physically [3, Hl, k] (added by the QKV GEMM
epilogue); output bias [E] is added on partial-sum replica 0 only.
The fused QKV output [B, S, 3, Hl, k] is consumed by the flash kernel in
place (strided views), and dQKV is produced in the same packed layout, so the
backward needs exactly one GEMM for dW_qkv and one for dX.

Key lengths (optional fourth input, an integer tensor [B]): keys >= lens[b] of
sample b do not exist.  They get probability 0, dK = dV = 0, and their K / V
rows are never read, so padding content (NaN included) cannot reach an output;
a row without a live key gives o = 0 and dQ = 0.  The flash kernels read the
lengths from the device tensor (a captured step follows a new batch's lengths);
the torch fallback applies the same definition as a mask.

Query lengths (attribute ``query_lengths``): the fourth input also gives each
sample's query length, for self-attention over a padded batch.  Queries >=
lens[b] do not exist: their rows of q and of the incoming gradient are never
read, o = 0 and dQ = 0 there, and they add nothing to dK / dV.  The kernels
skip them, so the attention work of a sample follows lens[b]^2.  Exact when
the loss ignores the padded positions (their incoming gradient is zero).

Packed sequences (attribute ``packed_sequences`` = M; the fourth input is then
an integer tensor [B, M]): every row ("pack") of the [B, T, E] input holds up
to M sequences ("segments") end to end from token 0, of the given lengths
(0: an empty slot).  Segment (n, m) occupies tokens [start, start + len) of
pack n, start = the sum of the pack's earlier clamped lengths, len clamped to
[0, min(max_seqlen, T - start)].  Attention is self-attention inside each
segment in segment-local coordinates (query i sees keys 0 .. len - 1 of its
segment, 0 .. i with ``causal``); the tokens after the last segment (the tail)
see nothing and are seen by nothing: o = 0 and dQ = dK = dV = 0 there, and
their content (NaN included) reaches no output.  The dropout mask of segment
(n, m) is that of sample n * M + m of attention_dropout_mask(B * M, H,
max_seqlen, max_seqlen, ...).  Every other operator of the model runs on the
dense [B, T, E] tensors, which now hold no padding between sequences.
"""
from __future__ import annotations

import math
import os
import warnings

import torch

from .. import kernels as K
from ..parallel import sequence as SP
from .base import OpContext, OpImpl, acc_grad, register
from .gemm import matmul, wgrad_matmul

# q/k/v projection-bias gradients from the attention backward kernels'
# epilogues instead of a separate column-sum pass over dQKV
# (FF_ATTN_FUSED_DBIAS=1).  Round 2 did this with one fp32 atomic per column
# per wave onto H*D addresses, which made dK/dV 117 -> 220 us and dQ 76 -> 150
# us (profiles/ab_attn_dbias_r2.txt).  Round 3: each wave stores its 32-row
# partial sums into a slab row (a reduce-scatter, no atomics) and one
# reduction adds the slab; measured even with the 25 us pass it replaces
# (BERT-large 723-727 vs 728 samples/s, profiles/ab_attn_dbias_slab_r3.txt),
# so the pass stays the default.
_FUSED_DBIAS = os.environ.get("FF_ATTN_FUSED_DBIAS", "0") == "1"


def _dims(ctx: OpContext, q, k, v, W):
    H_local = W.shape[-1] if W.dim() == 2 else None
    E = int(ctx.a("embed_dim"))
    H = int(ctx.a("num_heads"))
    kd = int(ctx.a("kdim") or 0) or E // H
    vd = int(ctx.a("vdim") or 0) or E // H
    Hl = H // max(1, ctx.input_copy_degree)
    if H_local is not None:
        Hl = H_local
    return E, Hl, kd, vd, q.shape[-1], k.shape[-1], v.shape[-1]


def _split_weights(W, E, Hl, kd, vd, Eq, Ek, Ev):
    flat = W.reshape(-1)
    if Eq == Ek == Ev and kd == vd:
        n_qkv = Eq * 3 * Hl * kd
        Wqkv = flat[:n_qkv].view(Eq, 3 * Hl * kd)
        Wo = flat[n_qkv:n_qkv + Hl * vd * E].view(Hl * vd, E)
        # per-projection strided views of the fused operand, for attention whose
        # q / k / v are different tensors of the same width (cross-attention)
        W3 = Wqkv.view(Eq, 3, Hl * kd)
        return {"qkv": Wqkv, "o": Wo, "q": W3[:, 0], "k": W3[:, 1], "v": W3[:, 2]}
    o0 = 0
    Wq = flat[o0:o0 + Eq * Hl * kd].view(Eq, Hl * kd)
    o0 += Eq * Hl * kd
    Wk = flat[o0:o0 + Ek * Hl * kd].view(Ek, Hl * kd)
    o0 += Ek * Hl * kd
    Wv = flat[o0:o0 + Ev * Hl * vd].view(Ev, Hl * vd)
    o0 += Ev * Hl * vd
    Wo = flat[o0:o0 + Hl * vd * E].view(Hl * vd, E)
    return {"q": Wq, "k": Wk, "v": Wv, "o": Wo}


def packed_segments(seg_lens, T, max_seqlen=None):
    """(start, len) int64 [N, M] each, and the segment id of every token
    int64 [N, T] (-1: the tail), of a packed batch: the definition that
    kernels.attention_segment_offsets implements on the device."""
    N, M = seg_lens.shape
    ms = T if max_seqlen is None else int(max_seqlen)
    start = torch.zeros(N, M, dtype=torch.int64, device=seg_lens.device)
    lens = torch.zeros_like(start)
    pos = torch.zeros(N, dtype=torch.int64, device=seg_lens.device)
    for m in range(M):
        ln = torch.minimum(seg_lens[:, m].to(torch.int64).clamp(0, ms), T - pos)
        start[:, m], lens[:, m] = pos, ln
        pos = pos + ln
    tok = torch.arange(T, device=seg_lens.device).view(1, 1, T)
    inside = (tok >= start[:, :, None]) & (tok < (start + lens)[:, :, None])            # [N, M, T]
    seg_id = torch.where(inside.any(1), inside.to(torch.int64).argmax(1), torch.full_like(pos, -1)[:, None])
    return start, lens, seg_id


def _torch_packed_attention(q, k, v, causal, scale, seg_lens, max_seqlen=None, drop=None):
    # q,k,v: [N, T, H, D]; seg_lens [N, M].  The block-diagonal (and causal) mask in physical coordinates;
    # drop = (keep mask [N * M, H, max_seqlen, max_seqlen], keep scale) in segment-local coordinates
    N, T, H, _ = q.shape
    M = seg_lens.shape[1]
    start, _, seg_id = packed_segments(seg_lens, T, max_seqlen)
    tail = seg_id < 0                                                                   # [N, T]
    # tail rows are never read: zeros in their place (0 * NaN), and no gradient flows into them
    qt, kt, vt = (t.masked_fill(tail[:, :, None, None], 0).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qt.float(), kt.float().transpose(-1, -2)) * scale                  # [N, H, T, T]
    see = (seg_id[:, :, None] == seg_id[:, None, :]) & ~tail[:, :, None]                # [N, Tq, Tk]
    if causal:
        see = see & ~torch.ones(T, T, dtype=torch.bool, device=s.device).triu(1)
    s = s.masked_fill(~see[:, None], float("-inf"))
    s = s.masked_fill(tail[:, None, :, None], 0.0)   # a tail row: finite scores for the softmax, zeroed below
    p = torch.softmax(s, -1)
    p = p.masked_fill(~see[:, None], 0.0)
    if drop is not None:
        keep, rs = drop
        sid = seg_id.clamp(min=0)
        loc = torch.arange(T, device=q.device).view(1, T) - torch.gather(start, 1, sid)   # local coordinate
        ms = keep.shape[-1]
        loc = loc.clamp(0, ms - 1)
        smp = torch.arange(N, device=q.device).view(N, 1) * M + sid                       # sample n * M + m
        kp = keep[smp[:, None, :, None], torch.arange(H, device=q.device).view(1, H, 1, 1),
                  loc[:, None, :, None], loc[:, None, None, :]]                           # [N, H, T, T]
        p = p * kp.to(p.dtype) * rs
    o = torch.matmul(p, vt.float())
    o = o.masked_fill(tail[:, None, :, None], 0)
    return o.transpose(1, 2).to(q.dtype)


def _torch_attention(q, k, v, causal, scale, drop=None, kv_lens=None, q_lens=None, bias=None):
    # q,k,v: [B, S, H, D] -> [B, S, H, D]; drop = (keep mask [B, H, Sq, Sk], keep scale)
    # kv_lens, q_lens: [B] integer key / query lengths (module docstring)
    # bias: additive float mask broadcastable to [B, H, Sq, Sk]; a row with every key at -inf gives zeros
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    dead = qdead = None
    if q_lens is not None:
        Sq = q.shape[1]
        qdead = torch.arange(Sq, device=q.device).view(1, Sq) >= q_lens.view(-1, 1).clamp(0, Sq)  # [B, Sq]
        # dead Q rows are never read: zeros in their place; the fill of the
        # output below does the same to the incoming gradient's dead rows
        qt = qt.masked_fill(qdead[:, None, :, None], 0)
    if kv_lens is not None:
        Sk = k.shape[1]
        dead = torch.arange(Sk, device=k.device).view(1, Sk) >= kv_lens.view(-1, 1).clamp(0, Sk)  # [B, Sk]
        # dead K / V rows are never read: zeros in their place, so that neither
        # 0 * NaN in the products nor their gradients can carry padding content
        kt = kt.masked_fill(dead[:, None, :, None], 0)
        vt = vt.masked_fill(dead[:, None, :, None], 0)
    s = torch.matmul(qt.float(), kt.float().transpose(-1, -2)) * scale
    if dead is not None:
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
        # a row with no live key: finite scores for the softmax, zeroed below
        s = s.masked_fill(dead.all(-1)[:, None, None, None], 0.0)
    if causal:
        Sq, Sk = s.shape[-2:]
        mask = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    rowdead = None
    if bias is not None:
        s = s + bias.to(s.dtype)
        # a row with every key masked: finite scores for the softmax, zeroed below
        rowdead = torch.isneginf(s).all(-1, keepdim=True)
        s = s.masked_fill(rowdead, 0.0)
    p = torch.softmax(s, -1)
    if dead is not None:
        p = p.masked_fill(dead[:, None, None, :], 0.0)
    if rowdead is not None:
        p = p.masked_fill(rowdead, 0.0)
    if drop is not None:
        p = p * drop[0].to(p.dtype) * drop[1]
    o = torch.matmul(p, vt.float())
    if qdead is not None:
        o = o.masked_fill(qdead[:, None, :, None], 0)
    return o.transpose(1, 2).to(q.dtype)


_M32 = 0xFFFFFFFF


def _i64(x: int) -> int:
    """A 64-bit pattern as the signed value torch's int64 holds."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def attention_dropout_mask(B, H, Sq, Sk, p, seed, device="cpu"):
    """Keep mask of attention dropout: (bool [B, H, Sq, Sk], keep scale).

    The definition that the flash kernels (csrc/kernels/attention.hip)
    regenerate element by element; this is its second, independent
    implementation, in torch integer ops on any device.  The decision for
    probability (b, h, q, k) is a pure function of (seed, b, h, q, k, p):

      key  = low 32 bits of splitmix64(seed, b * H + h):
               z = seed + 0x9E3779B97F4A7C15 * (b * H + h + 1)   (mod 2^64)
               z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
               z = (z ^ (z >> 27)) * 0x94D049BB133111EB
               z ^= z >> 31
      x    = mix32((q * Sk + k) ^ key), 32-bit, logical shifts:
               x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
      keep iff (x >> 8) >= T,   T = round(p * 2^24)

    Kept probabilities are scaled by 2^24 / (2^24 - T), exactly unbiased for
    the realised drop rate T / 2^24.  ``seed`` is the effective seed (host
    seed plus the device step word, mod 2^64): an int, or a 1-element int64
    tensor (read without a host synchronisation).  Needs Sq * Sk < 2^32 and
    p < 1; p <= 0 keeps everything.
    """
    T = K.attention_dropout_threshold(p)
    if Sq * Sk >= 1 << 32:
        raise ValueError(f"attention: dropout needs Sq * Sk < 2^32, got {Sq} x {Sk}")
    device = torch.device(device)
    if T == 0:
        return torch.ones(B, H, Sq, Sk, dtype=torch.bool, device=device), 1.0
    i64 = dict(dtype=torch.int64, device=device)
    if isinstance(seed, torch.Tensor):
        s = seed.reshape(1).to(**i64)
    else:
        s = torch.tensor([_i64(int(seed))], **i64)

    def lsr(z, n):  # logical shift right of a 64-bit pattern held in int64
        return (z >> n) & ((1 << (64 - n)) - 1)

    # int64 add / multiply wrap mod 2^64, which is the arithmetic wanted
    z = s + torch.arange(1, B * H + 1, **i64) * _i64(0x9E3779B97F4A7C15)
    z = (z ^ lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * _i64(0x94D049BB133111EB)
    z = z ^ lsr(z, 31)
    key = (z & _M32).view(B, H, 1, 1)
    idx = (torch.arange(Sq, **i64).view(Sq, 1) * Sk + torch.arange(Sk, **i64).view(1, Sk)).view(1, 1, Sq, Sk)
    x = idx ^ key                     # values stay in [0, 2^32): >> is logical
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32       # < 2^63: no wrap
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32       # may wrap mod 2^64: the low 32 bits are unaffected
    x = x ^ (x >> 16)
    return (x >> 8) >= T, float(1 << 24) / float((1 << 24) - T)


def _drop_seed(ctx: OpContext) -> int:
    """Host part of the attention-dropout seed (ctx.seed is per operator and rank)."""
    return (int(ctx.seed) * 7919 + 0x5DEECE66D) & ((1 << 63) - 1)


def _drop_step(ctx: OpContext, device) -> torch.Tensor:
    """Advance the operator's device-resident forward counter and return a
    private copy of its new value: the step word of this forward's mask, kept
    for its backward.  Both are device operations, so a captured forward
    draws a fresh mask on every replay, and the sequence of masks depends only
    on the number of training forwards run."""
    cnt = ctx.extra.get("attn_drop_counter")
    if cnt is None or cnt.device != device:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # created inside a capture, the counter's zero fill would be replayed too
            raise RuntimeError("attention dropout: run one eager training forward before graph capture")
        cnt = ctx.extra["attn_drop_counter"] = torch.zeros(1, dtype=torch.int64, device=device)
    cnt.add_(1)
    return cnt.clone()


def _fallback_mask(drop, B, H, Sq, Sk):
    """(keep mask, keep scale) of the torch fallback from a forward's drop record."""
    if drop is None:
        return None
    p, seed, step = drop
    return attention_dropout_mask(B, H, Sq, Sk, p, step + _i64(seed), step.device)


def _layout_dims(attrs: dict, Hl: int):
    E = int(attrs["embed_dim"])
    H = int(attrs["num_heads"])
    kd = int(attrs.get("kdim") or 0) or E // H
    vd = int(attrs.get("vdim") or 0) or E // H
    Eq, Ek, Ev = (attrs.get("_in_features") or [E, E, E])[:3]
    return E, kd, vd, int(Eq), int(Ek), int(Ev)


def _blocks(E, kd, vd, Eq, Ek, Ev):
    # per-head logical column: [Wq: Eq x k][Wk: Ek x k][Wv: Ev x v][Wo: v x E]
    return [(Eq, kd), (Ek, kd), (Ev, vd), (vd, E)]


@register("MULTIHEAD_ATTENTION")
class MultiHeadAttentionOp(OpImpl):
    def to_physical(self, attrs, index, piece):
        if index > 1:
            return piece
        Hl = piece.shape[-1]
        E, kd, vd, Eq, Ek, Ev = _layout_dims(attrs, Hl)
        if index == 1:  # [2k+v, Hl] -> q[Hl, k] | k[Hl, k] | v[Hl, v]
            return torch.cat([piece[:kd].t().reshape(-1), piece[kd:2 * kd].t().reshape(-1),
                              piece[2 * kd:].t().reshape(-1)])
        parts, o = [], 0
        mats = []
        for (r, c) in _blocks(E, kd, vd, Eq, Ek, Ev):
            mats.append(piece[o:o + r * c].view(r, c, Hl))
            o += r * c
        q, k, v, wo = mats
        if Eq == Ek == Ev and kd == vd:
            qkv = torch.stack([m.permute(0, 2, 1) for m in (q, k, v)], dim=1)  # [E, 3, Hl, k]
            parts.append(qkv.reshape(-1))
        else:
            for m in (q, k, v):
                parts.append(m.permute(0, 2, 1).reshape(-1))                   # [Ein, Hl, d]
        parts.append(wo.permute(2, 0, 1).reshape(-1))                           # [Hl, v, E]
        return torch.cat(parts)

    def to_logical(self, attrs, index, piece):
        if index > 1:
            return piece
        Hl = piece.shape[-1]
        E, kd, vd, Eq, Ek, Ev = _layout_dims(attrs, Hl)
        flat = piece.reshape(-1)
        if index == 1:
            q = flat[:Hl * kd].view(Hl, kd).t()
            k = flat[Hl * kd:2 * Hl * kd].view(Hl, kd).t()
            v = flat[2 * Hl * kd:].view(Hl, vd).t()
            return torch.cat([q, k, v], dim=0).contiguous()
        cols = []
        if Eq == Ek == Ev and kd == vd:
            n = Eq * 3 * Hl * kd
            qkv = flat[:n].view(Eq, 3, Hl, kd)
            for j in range(3):
                cols.append(qkv[:, j].permute(0, 2, 1).reshape(Eq * kd, Hl))
            o = n
        else:
            o = 0
            for (r, c) in _blocks(E, kd, vd, Eq, Ek, Ev)[:3]:
                cols.append(flat[o:o + r * Hl * c].view(r, Hl, c).permute(0, 2, 1).reshape(r * c, Hl))
                o += r * Hl * c
        wo = flat[o:o + Hl * vd * E].view(Hl, vd, E).permute(1, 2, 0).reshape(vd * E, Hl)
        cols.append(wo)
        return torch.cat(cols, dim=0).contiguous()

    def init_weight(self, ctx, index, logical_shape, initializer, gen):
        # glorot per projection block (fan_in=E, fan_out=H*kdim), not on the
        # flattened [P, H] tensor whose fans are meaningless.
        if index != 0 or initializer.get("type") not in ("glorot_uniform", "glorot_normal"):
            return None
        P, H = logical_shape
        E = int(ctx.a("embed_dim"))
        kd = int(ctx.a("kdim") or 0) or E // int(ctx.a("num_heads"))
        bound = math.sqrt(6.0 / (E + H * kd))
        if initializer["type"] == "glorot_uniform":
            return (torch.rand(P, H, generator=gen) * 2 - 1) * bound
        return torch.randn(P, H, generator=gen) * math.sqrt(2.0 / (E + H * kd))

    def init_spec(self, ctx, index, logical_shape, initializer):
        if index != 0 or initializer.get("type") not in ("glorot_uniform", "glorot_normal"):
            return None
        P, H = logical_shape
        E = int(ctx.a("embed_dim"))
        kd = int(ctx.a("kdim") or 0) or E // int(ctx.a("num_heads"))
        if initializer["type"] == "glorot_uniform":
            bound = math.sqrt(6.0 / (E + H * kd))
            return (0, -bound, bound, 0.0, 0.0)
        return (1, 0.0, math.sqrt(2.0 / (E + H * kd)), 0.0, 0.0)

    def forward(self, ctx: OpContext, inputs, weights):
        q_in, k_in, v_in = inputs[:3]
        lens = None
        # packed sequences: the fourth input is [B, M] segment lengths
        M_pack = int(ctx.a("packed_sequences", 0) or 0)
        seg = None
        if M_pack:
            if len(inputs) < 4:
                raise ValueError(f"{ctx.name}: packed_sequences needs the segment lengths input")
            seg = inputs[3]
            if seg.dtype.is_floating_point or seg.dim() != 2 or tuple(seg.shape) != (q_in.shape[0], M_pack):
                raise ValueError(f"{ctx.name}: packed_sequences: segment lengths must be an integer tensor "
                                 f"[batch, {M_pack}], got {seg.dtype} {tuple(seg.shape)}")
            if bool(ctx.a("key_lengths", False)) or bool(ctx.a("query_lengths", False)):
                raise ValueError(f"{ctx.name}: packed_sequences excludes key_lengths / query_lengths")
            if not (q_in is k_in and k_in is v_in) and not (q_in.shape[1] == k_in.shape[1] == v_in.shape[1]):
                raise ValueError(f"{ctx.name}: packed_sequences needs equal q / k / v sequence extents")
            seg = seg.to(torch.int32).contiguous()
        elif len(inputs) > 3:  # per-sample key lengths
            lens = inputs[3].reshape(-1)
            if lens.dtype.is_floating_point or lens.shape[0] != q_in.shape[0]:
                raise ValueError(f"{ctx.name}: key lengths must be an integer tensor [batch], got "
                                 f"{lens.dtype} {tuple(inputs[3].shape)}")
            lens = lens.to(torch.int32).contiguous()
        # query_lengths: the same tensor bounds the query axis (self-attention over a padded batch)
        qlens = None
        if bool(ctx.a("query_lengths", False)):
            if lens is None:
                raise ValueError(f"{ctx.name}: query_lengths needs the key lengths input")
            qlens = lens
        W = weights[0]
        b_in = weights[1] if len(weights) > 1 else None
        b_out = weights[2] if len(weights) > 2 and ctx.sum_index == 0 else None
        E, Hl, kd, vd, Eq, Ek, Ev = _dims(ctx, q_in, k_in, v_in, W)
        ws = _split_weights(W, E, Hl, kd, vd, Eq, Ek, Ev)
        B, Sq = q_in.shape[0], q_in.shape[1]
        Sk = k_in.shape[1]
        causal = bool(ctx.a("causal", False))
        scale = 1.0 / math.sqrt(kd)
        self_attn = (q_in is k_in) and (k_in is v_in) and "qkv" in ws
        x2 = q_in.reshape(-1, Eq).contiguous()
        bias_qkv = b_in.reshape(-1) if b_in is not None else None  # [3, Hl, k] order
        if self_attn:
            qkv = matmul(x2, ws["qkv"], bias=bias_qkv)                  # [B*S, 3*Hl*k]
            qkv5 = qkv.view(B, Sq, 3, Hl, kd)
            q, k, v = qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2]
            proj = qkv
        else:
            bq = bk = bv = None
            if bias_qkv is not None:
                bq, bk, bv = bias_qkv[:Hl * kd], bias_qkv[Hl * kd:2 * Hl * kd], bias_qkv[2 * Hl * kd:]
            q = matmul(x2, ws["q"], bias=bq).view(B, Sq, Hl, kd)
            k = matmul(k_in.reshape(-1, Ek).contiguous(), ws["k"], bias=bk).view(B, Sk, Hl, kd)
            v = matmul(v_in.reshape(-1, Ev).contiguous(), ws["v"], bias=bv).view(B, Sk, Hl, vd)
            proj = (q, k, v)
        grp = ctx.extra.get("seq_group")
        use_flash = (q.is_cuda and q.dtype == torch.bfloat16 and kd == vd and kd in (64, 128) and K.available())
        # dropout on the attention probabilities: training only.  drop = (p,
        # host seed, this forward's copy of the device step word), saved for
        # the backward; the mask is attention_dropout_mask(seed + step word)
        p_drop = float(ctx.a("dropout", 0.0) or 0.0) if ctx.training else 0.0
        drop = None
        max_seqlen = (int(ctx.a("max_seqlen", 0) or 0) or Sq) if seg is not None else None
        seg_off = None
        if grp is not None and grp.size > 1:
            if seg is not None:
                raise NotImplementedError(f"{ctx.name}: packed sequences are not supported on the sequence-parallel "
                                          "(ring / Ulysses) attention path")
            if lens is not None:
                raise NotImplementedError(f"{ctx.name}: key lengths are not supported on the sequence-parallel "
                                          "(ring / Ulysses) attention path")
            if qlens is not None:
                raise NotImplementedError(f"{ctx.name}: query lengths are not supported on the sequence-parallel "
                                          "(ring / Ulysses) attention path")
            if p_drop > 0 and not ctx.extra.get("attn_drop_warned"):
                ctx.extra["attn_drop_warned"] = True
                warnings.warn(f"{ctx.name}: attention dropout is not applied on the sequence-parallel path")
            # sequence-sharded q/k/v: Ulysses all-to-all or ring attention
            o, lse = SP.sp_attention_fwd(q, k, v, causal, scale, grp, SP.choose_mode(ctx.attrs, Hl, grp))
            lse = ("sp", lse)
        else:
            if p_drop > 0 and K.attention_dropout_threshold(p_drop):
                drop = (p_drop, _drop_seed(ctx), _drop_step(ctx, q.device))
            if use_flash and seg is not None:
                kw = dict(dropout_p=drop[0], seed=drop[1], seed_dev=drop[2]) if drop else {}
                # once per forward, on the device; kept for the backward
                seg_off = K.attention_segment_offsets(seg, Sq, max_seqlen)
                o, lse = K.attention_fwd(q, k, v, causal=causal, scale=scale, seg_lens=seg, max_seqlen=max_seqlen,
                                         seg_offsets=seg_off, **kw)
            elif seg is not None:
                o, lse = _torch_packed_attention(q, k, v, causal, scale, seg, max_seqlen,
                                                 _fallback_mask(drop, B * M_pack, Hl, max_seqlen, max_seqlen)), None
            elif use_flash:
                kw = dict(dropout_p=drop[0], seed=drop[1], seed_dev=drop[2]) if drop else {}
                o, lse = K.attention_fwd(q, k, v, causal=causal, scale=scale, kv_lens=lens, q_lens=qlens, **kw)
            else:
                o, lse = _torch_attention(q, k, v, causal, scale, _fallback_mask(drop, B, Hl, Sq, Sk), lens,
                                          qlens), None
        o2 = o.reshape(B * Sq, Hl * vd)
        out = matmul(o2, ws["o"], bias=b_out)
        saved = (x2, k_in if not self_attn else None, v_in if not self_attn else None, proj, o, lse, ws,
                 self_attn, (B, Sq, Sk, Hl, kd, vd, Eq, Ek, Ev, E, causal, scale), (lens, qlens, seg, max_seqlen, seg_off),
                 drop)
        return [out.view(B, Sq, E)], saved

    def backward(self, ctx, saved, grad_outputs, weight_grads, need_input_grad):
        x2, k_in, v_in, proj, o, lse, ws, self_attn, dims, (lens, qlens, seg, max_seqlen, seg_off), drop = saved
        no_lens_grad = [None] if (lens is not None or seg is not None) else []   # the lengths input gets no gradient
        B, Sq, Sk, Hl, kd, vd, Eq, Ek, Ev, E, causal, scale = dims
        dW = weight_grads[0]
        db_in = weight_grads[1] if len(weight_grads) > 1 else None
        db_out = weight_grads[2] if len(weight_grads) > 2 else None  # identical on every partial replica
        dout = grad_outputs[0].reshape(B * Sq, E).contiguous()
        o2 = o.reshape(B * Sq, Hl * vd)
        gpu = dout.is_cuda and dout.dtype == torch.bfloat16 and K.available()
        # ---- output projection
        dW_views = _split_weights(dW, E, Hl, kd, vd, Eq, Ek, Ev) if dW is not None else None
        if ctx.extra.pop("db_done", False):
            db_out = None   # accumulated by the consuming add+LayerNorm's backward (layernorm_bwd dsum)
        if db_out is not None:
            if gpu:
                K.colsum_act(dout, None, "none", db_out, write_dx=False)
            else:
                acc_grad(db_out, dout.float().sum(0))
        wbeta = ctx.extra.get("wgrad_beta", [1.0])[0]
        if dW_views is not None:
            if gpu:
                wgrad_matmul(ctx, o2, dout, dW_views["o"], wbeta)
            else:
                acc_grad(dW_views["o"], o2.float().t() @ dout.float())
        do = matmul(dout, ws["o"], trans_b=True) if gpu else dout @ ws["o"].to(dout.dtype).t()
        do4 = do.view(B, Sq, Hl, vd)
        # ---- attention core
        if self_attn:
            qkv = proj
            qkv5 = qkv.view(B, Sq, 3, Hl, kd)
            q, k, v = qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2]
        else:
            q, k, v = proj
        if isinstance(lse, tuple):
            dq_, dk_, dv_ = SP.sp_attention_bwd(do4, lse[1], causal, scale, ctx.extra["seq_group"])
            if self_attn:
                dproj = torch.stack([dq_, dk_, dv_], dim=2).reshape(B * Sq, 3 * Hl * kd)
            else:
                dq, dk, dv = dq_, dk_, dv_
        elif lse is not None:
            if self_attn:
                dproj = torch.empty_like(qkv)
                d5 = dproj.view(B, Sq, 3, Hl, kd)
                dq, dk, dv = d5[:, :, 0], d5[:, :, 1], d5[:, :, 2]
            else:
                dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            fused_db = None
            # packed sequences: the column-sum pass below (tail rows of dQKV are zeros)
            if _FUSED_DBIAS and seg is None and self_attn and db_in is not None and kd == vd \
                    and db_in.dtype == torch.float32 and db_in.is_contiguous():
                dbf = db_in.reshape(-1)
                n = Hl * kd
                fused_db = (dbf[:n], dbf[n:2 * n], dbf[2 * n:3 * n])
            kw = dict(dropout_p=drop[0], seed=drop[1], seed_dev=drop[2]) if drop else {}
            if seg is not None:
                kw.update(seg_lens=seg, max_seqlen=max_seqlen, seg_offsets=seg_off)
            K.attention_bwd(q, k, v, o, lse, do4, dq, dk, dv, causal=causal, scale=scale, dbias=fused_db,
                            kv_lens=lens, q_lens=qlens, **kw)
            if fused_db is not None:
                db_in = None   # accumulated by the attention backward kernels
        else:
            qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
            if seg is not None:
                ref = _torch_packed_attention(qf, kf, vf, causal, scale, seg, max_seqlen,
                                              _fallback_mask(drop, B * seg.shape[1], Hl, max_seqlen, max_seqlen))
            else:
                ref = _torch_attention(qf, kf, vf, causal, scale, _fallback_mask(drop, B, Hl, Sq, Sk), lens, qlens)
            ref.float().backward(do4.float())
            dq, dk, dv = (t.grad.to(do.dtype) for t in (qf, kf, vf))
            if self_attn:
                dproj = torch.stack([dq, dk, dv], dim=2).reshape(B * Sq, 3 * Hl * kd)
        # ---- input projections
        dx_q = dx_k = dx_v = None
        if self_attn:
            d2 = dproj.view(B * Sq, 3 * Hl * kd)
            # on the GPU the bias gradient rides in the weight-gradient GEMM where
            # that wins (wgrad_matmul bsum); the column-sum pass otherwise
            bsum = db_in.reshape(-1) if (db_in is not None and gpu) else None
            if db_in is not None and not gpu:
                acc_grad(db_in, d2.float().sum(0))
            if bsum is not None and dW_views is None:
                K.colsum_act(d2, None, "none", bsum, write_dx=False)
            if dW_views is not None:
                if gpu:
                    if not wgrad_matmul(ctx, x2, d2, dW_views["qkv"], wbeta, bsum) and bsum is not None:
                        K.colsum_act(d2, None, "none", bsum, write_dx=False)
                else:
                    acc_grad(dW_views["qkv"], x2.float().t() @ d2.float())
            if need_input_grad[0]:
                acc = ctx.extra.get("grad_acc", [None])[0]
                if gpu and acc is not None and acc.dtype == d2.dtype and acc.is_contiguous():
                    matmul(d2, ws["qkv"], trans_b=True, out=acc.view(B * Sq, Eq), beta=1.0)
                    return [acc, None, None] + no_lens_grad
                dx_q = (matmul(d2, ws["qkv"], trans_b=True) if gpu else d2 @ ws["qkv"].to(d2.dtype).t()).view(B, Sq, Eq)
            return [dx_q, None, None] + no_lens_grad
        srcs = ((x2, dq, "q", Eq, Sq, kd), (k_in.reshape(-1, Ek).contiguous(), dk, "k", Ek, Sk, kd),
                (v_in.reshape(-1, Ev).contiguous(), dv, "v", Ev, Sk, vd))
        outs = []
        for j, (xin, dp, key, Ein, S, dd) in enumerate(srcs):
            d2 = dp.reshape(B * S, Hl * dd).contiguous()
            if db_in is not None:
                seg = db_in.reshape(-1)[j * Hl * kd:(j * Hl * kd) + Hl * dd]
                acc_grad(seg, d2.float().sum(0))
            if dW_views is not None:
                if gpu:
                    wgrad_matmul(ctx, xin, d2, dW_views[key], wbeta)
                else:
                    acc_grad(dW_views[key], xin.float().t() @ d2.float())
            if need_input_grad[j]:
                dxx = matmul(d2, ws[key], trans_b=True) if gpu else d2 @ ws[key].to(d2.dtype).t()
                outs.append(dxx.view(B, S, Ein))
            else:
                outs.append(None)
        return outs + no_lens_grad


def _flash_bias_ok(mask, Sk) -> bool:
    """The BIAS kernels' rules for a [*, *, *, Sk] float mask (kernels._attn_bias raises on them)."""
    if mask.dtype not in (torch.float32, torch.bfloat16) or Sk % 4:
        return False
    if mask.dtype == torch.bfloat16:
        return True   # upcast into a dense fp32 tensor by the kernel interface
    if Sk > 1 and mask.stride(3) != 1:
        return False
    if any(mask.shape[i] != 1 and mask.stride(i) % 4 for i in range(3)):
        return False
    return mask.data_ptr() % 16 == 0


def _expand_kv(x, G: int):
    """[B, Hkv, S, D] -> [B, Hkv * G, S, D], K / V head j serving query heads j * G .. (torch's enable_gqa)."""
    return x if G == 1 else x.repeat_interleave(G, dim=1)


@register("SDPA")
class ScaledDotProductAttentionOp(OpImpl):
    """softmax(scale * q k^T + mask) v without projections.

    Inputs q [B, H, Sq, D], k / v [B, H, Sk, D] and an optional additive mask
    broadcastable to [B, H, Sq, Sk] (float; -inf masks a pair; a bool mask, True
    = attend, is converted); attributes ``causal``, ``dropout`` and ``scale``
    (absent or 0: 1 / sqrt(D)).  Output [B, H, Sq, D].  A row with every key
    masked gives zeros where torch gives NaN.  The mask gets no gradient: a
    learned bias keeps the unfused operator chain in the importers.

    bf16 on the GPU with D in {64, 128} runs on the flash kernels, which take
    the [B, H, S, D] storage in place through [B, S, H, D] views (their
    addressing is by stride); a mask goes to their BIAS instantiations when
    Sk % 4 == 0 and its strides allow 16-byte loads.  Dropout draws its mask
    from the operator's device step counter like MULTIHEAD_ATTENTION, so a
    captured step gets a new mask per replay.  Everything else (CPU, fp32,
    other head dims, Sk % 4 != 0, odd mask strides) runs _torch_attention,
    the same definition in torch.

    Grouped-query attention: k / v may have Hkv heads, [B, Hkv, Sk, D], with
    Hkv dividing H (read from the shapes; no attribute).  Query head h attends
    over K / V head h // (H // Hkv), torch's ``enable_gqa``; dk / dv come back
    with Hkv heads, summed over each group.  Without a mask or dropout the
    flash case runs the GQA kernels in place on the Hkv-head storage.  With a
    mask the BIAS kernels take, or with dropout, K and V are expanded to H
    heads once (G times the K / V bytes, still no Sq x Sk tensor), the
    existing kernels run as for Hkv == H, and dk / dv are reduced over the
    group in fp32 and cast once.  Everything else runs _torch_attention on
    K / V expanded inside the autograd graph.  The dropout mask and the
    fallback's mask keep H as their head count."""

    def forward(self, ctx: OpContext, inputs, weights):
        q, k, v = inputs[:3]
        mask = inputs[3] if len(inputs) > 3 else None
        if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise ValueError(f"{ctx.name}: q / k / v must be [batch, heads, seq, head_dim]")
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        Hkv = k.shape[1]
        if v.shape[1] != Hkv:
            raise ValueError(f"{ctx.name}: k has {Hkv} heads and v has {v.shape[1]}: grouped-query K / V need "
                             "equal head counts")
        if Hkv < 1 or H % Hkv:
            raise ValueError(f"{ctx.name}: {H} query heads are not a multiple of {Hkv} K / V heads "
                             "(grouped-query attention needs H % Hkv == 0)")
        G = H // Hkv
        causal = bool(ctx.a("causal", False))
        if causal and mask is not None:
            raise ValueError(f"{ctx.name}: causal cannot be combined with a mask")
        if causal and Sq != Sk:
            raise ValueError(f"{ctx.name}: causal needs Sq == Sk")
        scale = float(ctx.a("scale", 0.0) or 0.0) or 1.0 / math.sqrt(D)
        if mask is not None:
            if mask.dtype == torch.bool:
                mask = torch.zeros(mask.shape, dtype=torch.float32, device=mask.device).masked_fill(~mask, float("-inf"))
            elif not mask.dtype.is_floating_point:
                raise ValueError(f"{ctx.name}: the mask must be a float or bool tensor, got {mask.dtype}")
            elif mask.dtype not in (torch.float32, torch.bfloat16):
                mask = mask.float()
            full = (B, H, Sq, Sk)
            if mask.dim() != 4 or any(mask.shape[i] not in (1, full[i]) for i in range(4)):
                raise ValueError(f"{ctx.name}: mask shape {tuple(mask.shape)} is not broadcastable to {list(full)}")
            if mask.shape[3] != Sk:
                mask = mask.expand(*mask.shape[:3], Sk).contiguous()
        p_drop = float(ctx.a("dropout", 0.0) or 0.0) if ctx.training else 0.0
        drop = None
        if p_drop > 0 and K.attention_dropout_threshold(p_drop):
            drop = (p_drop, _drop_seed(ctx), _drop_step(ctx, q.device))
        use_flash = (q.is_cuda and q.dtype == torch.bfloat16 and k.dtype == q.dtype and v.dtype == q.dtype
                     and D in (64, 128) and v.shape[3] == D and K.available()
                     and (mask is None or _flash_bias_ok(mask, Sk)))
        if use_flash:
            q, k, v = (t if t.stride(3) == 1 and t.is_contiguous() else t.contiguous() for t in (q, k, v))
            if G > 1 and (mask is not None or drop):
                # the BIAS / DROP kernels have no GQA form: K / V expanded to H
                # heads once, kept for the backward
                k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
            o = torch.empty(B, H, Sq, D, device=q.device, dtype=q.dtype)
            kw = dict(dropout_p=drop[0], seed=drop[1], seed_dev=drop[2]) if drop else {}
            _, lse = K.attention_fwd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), causal=causal,
                                     scale=scale, out=o.transpose(1, 2), bias=mask, **kw)
        else:
            o = _torch_attention(q.transpose(1, 2), _expand_kv(k, G).transpose(1, 2),
                                 _expand_kv(v, G).transpose(1, 2), causal, scale,
                                 _fallback_mask(drop, B, H, Sq, Sk), bias=mask).transpose(1, 2).contiguous()
            lse = None
        return [o], (q, k, v, mask, o, lse, causal, scale, drop, Hkv)

    def backward(self, ctx, saved, grad_outputs, weight_grads, need_input_grad):
        q, k, v, mask, o, lse, causal, scale, drop, Hkv = saved
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        G = H // Hkv
        do = grad_outputs[0]
        tail = [None] if mask is not None else []   # the mask gets no gradient
        if lse is not None:
            do = do.to(q.dtype).contiguous()
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            kw = dict(dropout_p=drop[0], seed=drop[1], seed_dev=drop[2]) if drop else {}
            t = lambda x: x.transpose(1, 2)
            K.attention_bwd(t(q), t(k), t(v), t(o), lse, t(do), t(dq), t(dk), t(dv), causal=causal, scale=scale,
                            bias=mask, **kw)
            if k.shape[1] != Hkv:
                # the expanded path: the group sum in fp32, one cast
                dk = dk.view(B, Hkv, G, Sk, D).sum(2, dtype=torch.float32).to(q.dtype)
                dv = dv.view(B, Hkv, G, Sk, D).sum(2, dtype=torch.float32).to(q.dtype)
        else:
            qf, kf, vf = (x.detach().float().requires_grad_(True) for x in (q, k, v))
            # K / V expanded inside the graph: autograd does the group sum
            ref = _torch_attention(qf.transpose(1, 2), _expand_kv(kf, G).transpose(1, 2),
                                   _expand_kv(vf, G).transpose(1, 2), causal, scale,
                                   _fallback_mask(drop, B, H, Sq, Sk), bias=mask)
            ref.float().backward(do.float().transpose(1, 2))
            dq, dk, dv = (x.grad.to(do.dtype) for x in (qf, kf, vf))
        need = list(need_input_grad) + [False] * 3
        return [dq if need[0] else None, dk if need[1] else None, dv if need[2] else None] + tail
