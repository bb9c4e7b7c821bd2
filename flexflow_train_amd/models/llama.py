"""LLaMA-style decoder-only causal LM built through the FFModel API.

Pre-norm blocks of RMS norm, bias-free q / k / v projections, rotary position
embeddings on q and k, causal grouped-query attention (``SDPA``), and a SwiGLU
MLP (SiLU spelled multiply(gate, sigmoid(gate))); a final RMS norm, the LM
head and a softmax.  No learned positions and no biases anywhere.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Tuple

import numpy as np

from ..core import ActiMode, AggrMode, DataType, FFModel
from ..core.initializers import NormInitializer


@dataclasses.dataclass
class LlamaConfig:
    vocab_size: int = 32000
    hidden_size: int = 1024
    num_layers: int = 8
    num_heads: int = 16
    num_kv_heads: int = 4
    intermediate_size: int = 2816
    sequence_length: int = 2048
    batch_size: int = 4
    rms_norm_eps: float = 1e-6
    rope_theta: float = 10000.0
    initializer_range: float = 0.02

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads


def build_llama(model: FFModel, cfg: LlamaConfig) -> Tuple[Dict[str, object], object]:
    B, S, E = cfg.batch_size, cfg.sequence_length, cfg.hidden_size
    H, Hkv, D = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    if H * D != E or H % Hkv:
        raise ValueError("llama: hidden_size must be num_heads * head_dim and num_heads a multiple of num_kv_heads")
    init = NormInitializer(0, 0.0, cfg.initializer_range)
    none = ActiMode.AC_MODE_NONE

    def dense(t, n, name):
        return model.dense(t, n, none, False, kernel_initializer=init, name=name)

    tok = model.create_tensor([B, S], DataType.DT_INT32, create_grad=False, name="input_ids")
    x = model.embedding(tok, cfg.vocab_size, E, AggrMode.AGGR_MODE_NONE, kernel_initializer=init, name="embed_tokens")
    for i in range(cfg.num_layers):
        p = f"layers{i}"
        h = model.rms_norm(x, cfg.rms_norm_eps, name=f"{p}.input_norm")
        q = model.reshape(dense(h, H * D, f"{p}.q_proj"), [B, S, H, D], name=f"{p}.q_heads")
        k = model.reshape(dense(h, Hkv * D, f"{p}.k_proj"), [B, S, Hkv, D], name=f"{p}.k_heads")
        v = model.reshape(dense(h, Hkv * D, f"{p}.v_proj"), [B, S, Hkv, D], name=f"{p}.v_heads")
        q = model.rope(q, cfg.rope_theta, seq_dim=1, name=f"{p}.q_rope")
        k = model.rope(k, cfg.rope_theta, seq_dim=1, name=f"{p}.k_rope")
        q, k, v = (model.transpose(t, [0, 2, 1, 3], name=f"{p}.{n}_t") for t, n in ((q, "q"), (k, "k"), (v, "v")))
        a = model.scaled_dot_product_attention(q, k, v, causal=True, name=f"{p}.attn")
        a = model.reshape(model.transpose(a, [0, 2, 1, 3], name=f"{p}.attn_t"), [B, S, E], name=f"{p}.attn_merge")
        x = model.add(x, dense(a, E, f"{p}.o_proj"), name=f"{p}.attn_residual")
        h = model.rms_norm(x, cfg.rms_norm_eps, name=f"{p}.post_attn_norm")
        gate = dense(h, cfg.intermediate_size, f"{p}.gate_proj")
        up = dense(h, cfg.intermediate_size, f"{p}.up_proj")
        act = model.multiply(gate, model.sigmoid(gate, name=f"{p}.gate_sigmoid"), name=f"{p}.gate_silu")
        h = dense(model.multiply(act, up, name=f"{p}.gate_up"), E, f"{p}.down_proj")
        x = model.add(x, h, name=f"{p}.mlp_residual")
    x = model.rms_norm(x, cfg.rms_norm_eps, name="norm")
    logits = dense(x, cfg.vocab_size, "lm_head")
    probs = model.softmax(logits, -1, name="softmax")
    return {"input_ids": tok}, probs


def llama_synthetic(cfg: LlamaConfig, rng: np.random.Generator):
    B, S = cfg.batch_size, cfg.sequence_length
    ids = rng.integers(0, cfg.vocab_size, (B, S + 1), dtype=np.int32)
    return {"input_ids": ids[:, :S].copy()}, ids[:, 1:].astype(np.int64)
