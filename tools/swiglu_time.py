#!/usr/bin/env python3
"""Time the SwiGLU kernels (HIP events) against what they replace, in the same
process: interleaved rounds, medians and the spread (min - max over the rounds)
as JSON lines (tools/rmsnorm_rope_time.py's clock and report).

    python tools/swiglu_time.py elementwise [rounds]  # K.swiglu_fwd / bwd, and the SWIGLU node against the
                                                      # sigmoid / multiply / multiply chain through the executor
    python tools/swiglu_time.py gemm [rounds]         # K.gemm_swiglu against two autotuned GEMMs + K.swiglu_fwd
    python tools/swiglu_time.py model [rounds]        # build_llama steps: swiglu_op off, on unfused, on fused
    python tools/swiglu_time.py baseline [rounds]     # the swiglu_op=False step alone (also runs on a checkout
                                                      # without the operator: the parent commit's figure)
    python tools/swiglu_time.py --tiny ...            # toy sizes (a rehearsal; also runs on the CPU)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rmsnorm_rope_time import CUDA, DEV, TINY, _chain_model, interleaved, report  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flexflow_train_amd import kernels as K  # noqa: E402
from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType  # noqa: E402


def elementwise(rounds):
    dt = torch.bfloat16 if CUDA else torch.float32
    iters = 3 if TINY else 50
    for M, N in ([(64, 72)] if TINY else [(8192, 2816), (8192, 11008)]):
        gen = torch.Generator().manual_seed(0)
        g, u, dy = (torch.randn(M, N, generator=gen).to(dt).to(DEV) for _ in range(3))
        el = g.element_size() * M * N
        if CUDA:
            y = torch.empty_like(g)
            both = torch.empty(M, 2 * N, device=DEV, dtype=dt)
            report("swiglu_kernels", [M, N],
                   interleaved({"swiglu_fwd": lambda: K.swiglu_fwd(g, u, y),
                                "swiglu_bwd": lambda: K.swiglu_bwd(dy, g, u, both[:, :N], both[:, N:])}, iters, rounds),
                   {"swiglu_fwd": 3 * el, "swiglu_bwd": 5 * el})
        # through the executor: one SWIGLU node against the three-op chain (forward, forward + backward);
        # up = 0.5 * t in both models, so that gate and up are two tensors
        f1, b1 = _chain_model((M, N), lambda m, t: m.swiglu(t, m.scalar_multiply(t, 0.5)))
        f2, b2 = _chain_model((M, N), lambda m, t: m.multiply(m.multiply(t, m.sigmoid(t)), m.scalar_multiply(t, 0.5)))
        report("swiglu_operator", [M, N],
               interleaved({"node_fwd": f1, "chain_fwd": f2, "node_fwd_bwd": b1, "chain_fwd_bwd": b2},
                           max(2, iters // 5), rounds), {})


def gemm(rounds):
    from flexflow_train_amd.ops.gemm import matmul

    if not CUDA:
        raise SystemExit("swiglu_time gemm: needs a GPU")
    shapes = [(64, 64, 72)] if TINY else [(M, Kd, N) for M in (512, 2048, 8192)
                                          for Kd, N in ((1024, 2816), (4096, 11008))]
    for M, Kd, N in shapes:
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(M, Kd, generator=gen).to(torch.bfloat16).to(DEV)
        wg, wu = ((torch.randn(Kd, N, generator=gen) * Kd ** -0.5).to(torch.bfloat16).to(DEV) for _ in range(2))
        gu = torch.empty(M, 2 * N, device=DEV, dtype=torch.bfloat16)
        g, u, y = gu[:, :N], gu[:, N:], torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        matmul(x, wg, out=g)   # settles the autotuner's picks before anything is timed
        matmul(x, wu, out=u)
        t = interleaved({"gemm_swiglu": lambda: K.gemm_swiglu(x, wg, wu, g, u, y),
                         "pair": lambda: (matmul(x, wg, out=g), matmul(x, wu, out=u), K.swiglu_fwd(g, u, y)),
                         "two_gemms": lambda: (matmul(x, wg, out=g), matmul(x, wu, out=u))},
                        3 if TINY else 20, rounds)
        report("gemm_swiglu", [M, N, Kd], t, {})


def _llama_step(lc, fuse):
    from flexflow_train_amd.models.llama import build_llama, llama_synthetic

    cfg = FFConfig()
    cfg.perform_fusion = fuse
    m = FFModel(cfg)
    build_llama(m, lc)
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-4), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    feeds, labels = llama_synthetic(lc, np.random.default_rng(0))
    feeds = {k: torch.from_numpy(v).to(ex.cfg.device) for k, v in feeds.items()}
    labels = torch.from_numpy(labels).to(ex.cfg.device)
    return lambda: ex.train_step(feeds, labels)


def _llama_sizes():
    sizes = {"tiny": dict(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
                          intermediate_size=512, sequence_length=64, batch_size=2)}
    if not TINY:
        sizes["8x1024"] = dict(vocab_size=32000, hidden_size=1024, num_layers=8, num_heads=16, num_kv_heads=4,
                               intermediate_size=2816, sequence_length=2048, batch_size=4)
    return sizes


def model(rounds):
    from flexflow_train_amd.models.llama import LlamaConfig
    from flexflow_train_amd.ops.dense import swiglu_report

    for name, kw in _llama_sizes().items():
        steps = {"chain": _llama_step(LlamaConfig(**kw), True),
                 "swiglu_unfused": _llama_step(LlamaConfig(swiglu_op=True, **kw), False),
                 "swiglu_fused": _llama_step(LlamaConfig(swiglu_op=True, **kw), True)}
        report("llama_step", name, interleaved(steps, 3 if TINY else 10, rounds), {})
    print(swiglu_report(), flush=True)


def baseline(rounds):
    from flexflow_train_amd.models.llama import LlamaConfig

    for name, kw in _llama_sizes().items():
        report("llama_step", name, interleaved({"chain": _llama_step(LlamaConfig(**kw), True)},
                                               3 if TINY else 10, rounds), {})


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "elementwise"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    {"elementwise": elementwise, "gemm": gemm, "model": model, "baseline": baseline}[mode](n)
