#!/usr/bin/env python3
"""Time the RMSNorm and RoPE kernels (HIP events) against their comparators in
the same process, and a LLaMA-style training step with and without the
add + RMS-norm fusion.  Interleaved rounds; medians and the spread (min - max
over the rounds) are printed as JSON lines.

    python tools/rmsnorm_rope_time.py kernels [rounds]   # RMSNorm / LayerNorm / operator chain, RoPE / chain
    python tools/rmsnorm_rope_time.py model [rounds]     # build_llama steps, perform_fusion on and off
    python tools/rmsnorm_rope_time.py --tiny ...         # toy sizes (a rehearsal; also runs on the CPU)

Comparators: K.layernorm_fwd / K.layernorm_bwd at the same (M, N) (RMSNorm
does strictly less work), and the operator chains an importer emits for the
same math without these operators (pow -> mean -> scalar_add -> rsqrt ->
multiply for the norm, without the final gamma multiply, so the chain is
under-counted; split / negate / concat / two multiplies / add for the
rotation), run through the executor forward + backward.  Both models of such
a pair start with the same learned element-wise scale, so that the operators
behind it have a gradient to compute; its cost is in both figures.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flexflow_train_amd import kernels as K  # noqa: E402
from flexflow_train_amd.core import (AdamOptimizer, DataType, FFConfig, FFModel, LossType,  # noqa: E402
                                     SGDOptimizer)

TINY = "--tiny" in sys.argv
if TINY:
    sys.argv.remove("--tiny")
CUDA = torch.cuda.is_available()
DEV = "cuda" if CUDA else "cpu"


def _time(fn, iters):
    """ms per call over `iters` calls after a warm-up."""
    for _ in range(3):
        fn()
    if not CUDA:
        import time
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / iters
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(fns, iters, rounds):
    """{name: [ms per round]} with the candidates alternating inside every round."""
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            t[n].append(_time(fn, iters))
    return t


def report(what, shape, t, nbytes):
    for n, v in t.items():
        med = statistics.median(v)
        rec = {"what": what, "shape": shape, "case": n, "ms_median": round(med, 4), "ms_min": round(min(v), 4),
               "ms_max": round(max(v), 4)}
        if nbytes.get(n):
            rec["GB_per_s"] = round(nbytes[n] / med / 1e6, 1)
        print(json.dumps(rec), flush=True)


def _chain_model(shape, build):
    from flexflow_train_amd import _ffcore as C
    from flexflow_train_amd.core.model import Tensor

    m = FFModel(FFConfig())
    x = m.create_tensor(list(shape), DataType.DT_FLOAT, name="x")
    # a learned scale in front (the same in both models) gives the operators
    # under test an input that needs a gradient, so their backward runs
    w = m.cg.create_weight(C.TensorShape([shape[-1]], C.datatype_from_string("float")),
                           '{"type":"constant","value":1.0}', True, "scale.w")
    build(m, m.multiply(x, Tensor(m, w, "scale.w"), name="scale"))
    m.compile(optimizer=SGDOptimizer(m, lr=0.0), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    xin = torch.randn(*shape, generator=g).to(ex.cfg.compute_dtype).to(ex.cfg.device)
    dy = torch.randn(*shape, generator=g).to(ex.cfg.compute_dtype).to(ex.cfg.device)

    def fwd():
        ex.forward({"x": xin}, training=True)

    def both():
        ex.forward({"x": xin}, training=True)
        ex.backward(dy)
    return fwd, both


def kernels(rounds):
    dt = torch.bfloat16 if CUDA else torch.float32
    shapes = [(64, 512), (256, 128)] if TINY else [(8192, 4096), (8 * 32 * 2048, 128)]
    iters = 3 if TINY else 50
    for M, N in shapes:
        g = torch.Generator().manual_seed(0)
        x, dy = (torch.randn(M, N, generator=g).to(dt).to(DEV) for _ in range(2))
        gamma, beta = torch.ones(N, dtype=dt, device=DEV), torch.zeros(N, dtype=dt, device=DEV)
        dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        fns, nb = {}, {}
        el = x.element_size() * M * N
        if CUDA:
            _, s, rstd = K.rmsnorm_fwd(x, gamma, 1e-6)
            _, s2, mean, rstd2 = K.layernorm_fwd(x, gamma, beta, 1e-5)
            fns = {"rmsnorm_fwd": lambda: K.rmsnorm_fwd(x, gamma, 1e-6),
                   "layernorm_fwd": lambda: K.layernorm_fwd(x, gamma, beta, 1e-5),
                   "rmsnorm_bwd": lambda: K.rmsnorm_bwd(dy, s, rstd, gamma, dg),
                   "layernorm_bwd": lambda: K.layernorm_bwd(dy, s2, mean, rstd2, gamma, dg, db)}
            nb = {"rmsnorm_fwd": 2 * el, "layernorm_fwd": 2 * el, "rmsnorm_bwd": 3 * el, "layernorm_bwd": 3 * el}
        report("rmsnorm", [M, N], interleaved(fns, iters, rounds), nb)
        # through the executor: one RMS_NORM node against the importer's chain (forward, forward + backward)
        f1, b1 = _chain_model((M, N), lambda m, t: m.rms_norm(t, 1e-6, False))
        f2, b2 = _chain_model((M, N), lambda m, t: m.multiply(
            t, m.rsqrt(m.scalar_add(m.mean(m.pow(t, 2.0), [1], True), 1e-6))))
        report("rmsnorm_operator", [M, N],
               interleaved({"node_fwd": f1, "chain_fwd": f2, "node_fwd_bwd": b1, "chain_fwd_bwd": b2},
                           max(2, iters // 5), rounds), {})
    shape = (2, 16, 2, 32) if TINY else (8, 2048, 32, 128)
    B, S, H, D = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(*shape, generator=g).to(dt).to(DEV)
    if CUDA:
        y = torch.empty_like(x)
        el = 2 * x.numel() * x.element_size()
        report("rope", list(shape),
               interleaved({"rope": lambda: K.rope(x, 10000.0, 1, out=y),
                            "rope_inverse_inplace": lambda: K.rope(y, 10000.0, 1, inverse=True, out=y),
                            "rope_interleaved": lambda: K.rope(x, 10000.0, 1, True, out=y)}, iters, rounds),
               {"rope": el, "rope_inverse_inplace": el, "rope_interleaved": el})
    tab = K.rope_table(S, D, 10000.0, "cpu")
    cos = torch.cat([tab[..., 0]] * 2, -1).reshape(1, S, 1, D).numpy()
    sin = torch.cat([tab[..., 1]] * 2, -1).reshape(1, S, 1, D).numpy()

    def chain(m, t):
        a, b = m.split(t, [D // 2, D // 2], 3)
        rot = m.concat([m.scalar_multiply(b, -1.0), a], 3)
        return m.add(m.multiply(t, m.create_constant_array(np.ascontiguousarray(cos), name="cos")),
                     m.multiply(rot, m.create_constant_array(np.ascontiguousarray(sin), name="sin")))
    f1, b1 = _chain_model(shape, lambda m, t: m.rope(t, seq_dim=1))
    f2, b2 = _chain_model(shape, chain)
    report("rope_operator", list(shape),
           interleaved({"node_fwd": f1, "chain_fwd": f2, "node_fwd_bwd": b1, "chain_fwd_bwd": b2},
                       max(2, iters // 5), rounds), {})


def model(rounds):
    from flexflow_train_amd.models.llama import LlamaConfig, build_llama, llama_synthetic

    cfgs = {"tiny": LlamaConfig(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
                                intermediate_size=512, sequence_length=64, batch_size=2)}
    if not TINY:
        cfgs["8x1024"] = LlamaConfig(vocab_size=32000, hidden_size=1024, num_layers=8, num_heads=16, num_kv_heads=4,
                                     intermediate_size=2816, sequence_length=2048, batch_size=4)
    for name, lc in cfgs.items():
        steps = {}
        for fuse in (True, False):
            cfg = FFConfig()
            cfg.perform_fusion = fuse
            m = FFModel(cfg)
            build_llama(m, lc)
            m.compile(optimizer=AdamOptimizer(m, alpha=1e-4), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
            ex = m.executor
            feeds, labels = llama_synthetic(lc, np.random.default_rng(0))
            feeds = {k: torch.from_numpy(v).to(ex.cfg.device) for k, v in feeds.items()}
            labels = torch.from_numpy(labels).to(ex.cfg.device)
            steps["fused" if fuse else "unfused"] = (lambda ex=ex, f=feeds, y=labels: ex.train_step(f, y))
        report("llama_step", name, interleaved(steps, 3 if TINY else 10, rounds), {})


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    {"kernels": kernels, "model": model}[mode](n)
