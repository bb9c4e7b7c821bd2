#!/usr/bin/env python3
"""EXPERTS forward + backward: the device-routed grouped-GEMM path against the
per-expert library-GEMM path (FF_MOE_GROUPED=0), one process, interleaved
repetitions; then a whole MoE training step, hipGraph replay against eager.

    python tools/bench_moe.py [--tokens 8192] [--dim 1024] [--hidden 4096] [--experts 8 64] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flexflow_train_amd.ops import base as opbase  # noqa: E402

DEV = "cuda"


def _ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _launches(fn):
    """GPU kernels of one call (torch.profiler); None when the tracer is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:  # noqa: BLE001 - the count is a side figure of the timing
        return None


def bench_operator(B, D, H, E, k, act, reps, iters, emit):
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV, torch.bfloat16)  # noqa: E731
    x, dout = rn(B, D), rn(B, D)
    vals, ids = torch.topk(torch.softmax(torch.randn(B, E, generator=g), -1), k, -1)
    ids, gate = ids.to(DEV, torch.int32), vals.to(DEV, torch.bfloat16)
    ws = [rn(E, D, H) * 0.05, rn(E, H) * 0.1, rn(E, H, D) * 0.05, rn(E, D) * 0.1]
    grads = [torch.zeros(w.shape, device=DEV, dtype=torch.float32) for w in ws]
    impl = opbase.get_impl("EXPERTS")
    ctx = opbase.OpContext(op_type="EXPERTS", attrs={"num_experts": E, "hidden_size": H, "out_dim": D,
                                                      "activation": act, "use_bias": True}, name="moe")

    def run(mode):
        os.environ["FF_MOE_GROUPED"] = mode
        outs, saved = impl.forward(ctx, [x, ids, gate], ws)
        impl.backward(ctx, saved, [dout], grads, [True, False, True])

    times = {"1": [], "0": []}
    for mode in ("1", "0"):
        run(mode)
    for _ in range(reps):
        for mode in ("1", "0"):
            times[mode].append(_ms(lambda: run(mode), iters))
    n1, n0 = _launches(lambda: run("1")), _launches(lambda: run("0"))
    os.environ.pop("FF_MOE_GROUPED", None)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    flops = 3 * 2 * 2 * B * k * D * H
    emit({"bench": "experts_fwd_bwd", "tokens": B, "D": D, "H": H, "E": E, "k": k, "act": act,
          "rows_per_expert": B * k // E, "grouped_ms": round(med(times["1"]), 4),
          "per_expert_ms": round(med(times["0"]), 4), "grouped_ms_all": [round(t, 4) for t in times["1"]],
          "per_expert_ms_all": [round(t, 4) for t in times["0"]],
          "grouped_over_per_expert": round(med(times["1"]) / med(times["0"]), 4),
          "grouped_tflops": round(flops / med(times["1"]) / 1e9, 1), "grouped_launches": n1,
          "per_expert_launches": n0})


def bench_step(B, D, H, E, k, reps, iters, emit):
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType, MetricsType

    m = FFModel(FFConfig())
    x = m.create_tensor([B, D], DataType.DT_FLOAT, name="input")
    h = m.moe(x, E, k, H, name="moe")
    m.softmax(m.dense(h, 16, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-4), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY,
              metrics=[MetricsType.METRICS_ACCURACY])
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    feeds = {"input": torch.randn(B, D, generator=g).to(DEV)}
    labels = torch.randint(0, 16, (B, 1), generator=g, dtype=torch.int32).to(DEV)

    def eager(mode):
        if mode is None:
            os.environ.pop("FF_MOE_GROUPED", None)
        else:
            os.environ["FF_MOE_GROUPED"] = mode
        ex.train_step(feeds, labels)

    for mode in ("0", None):
        eager(mode)
    t = {"per_expert": [], "grouped": [], "graphed": []}
    for _ in range(reps):
        t["per_expert"].append(_ms(lambda: eager("0"), iters))
        t["grouped"].append(_ms(lambda: eager(None), iters))
    os.environ.pop("FF_MOE_GROUPED", None)
    step = ex.make_graphed_train_step(feeds, labels, warmup=1)
    step()
    for _ in range(reps):
        t["graphed"].append(_ms(step, iters))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    emit({"bench": "moe_train_step", "tokens": B, "D": D, "H": H, "E": E, "k": k,
          "eager_per_expert_ms": round(med(t["per_expert"]), 4), "eager_grouped_ms": round(med(t["grouped"]), 4),
          "graphed_ms": round(med(t["graphed"]), 4),
          "graphed_over_eager_per_expert": round(med(t["graphed"]) / med(t["per_expert"]), 4),
          "all_ms": {n: [round(v, 4) for v in vs] for n, vs in t.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--experts", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--act", default="gelu")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for E in a.experts:
        bench_operator(a.tokens, a.dim, a.hidden, E, a.topk, a.act, a.reps, a.iters, emit)
    if not a.no_step:
        for E in a.experts:
            bench_step(a.tokens, a.dim, a.hidden, E, a.topk, a.reps, a.iters, emit)


if __name__ == "__main__":
    main()
