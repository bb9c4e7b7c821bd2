#!/usr/bin/env python3
"""Weight-gradient GEMM with the bias gradient fused (gemmp ``bsum``) against
the plain GEMM and the plain GEMM followed by the column-sum pass, one process,
random data, arms interleaved, median of 3 rounds x 10 calls each:

    python tools/bench_wgrad_bsum.py [--tokens 65536] [--shapes 1024x3072,1024x30528]

One JSON line per shape: the autotuner's plain pick, the three times (ms), the
fused form's times per split count and what ``wgrad_matmul`` decides."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from flexflow_train_amd import kernels as K  # noqa: E402
from flexflow_train_amd.ops import gemm as G  # noqa: E402


def _round(fn, calls=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--shapes", default="1024x3072,1024x30528")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgrad_bsum: needs a GPU")
    dev = "cuda"
    for shp in a.shapes.split(","):
        M, N = (int(v) for v in shp.split("x"))
        x = torch.randn(a.tokens, M, device=dev, dtype=torch.bfloat16)
        g = torch.randn(a.tokens, N, device=dev, dtype=torch.bfloat16)
        dW = torch.zeros(M, N, device=dev, dtype=torch.float32)
        db = torch.zeros(N, device=dev, dtype=torch.float32)
        G.matmul(x, g, trans_a=True, out=dW, beta=0.0)          # autotunes the plain GEMM
        plain_pick = [v for k, v in G.choices().items() if k[0] == tuple(x.shape) and k[1] == tuple(g.shape)][-1]
        arms = {"plain": lambda: G.matmul(x, g, trans_a=True, out=dW, beta=0.0),
                "plain+colsum": lambda: (G.matmul(x, g, trans_a=True, out=dW, beta=0.0),
                                         K.colsum_act(g, None, "none", db, write_dx=False)),
                "colsum": lambda: K.colsum_act(g, None, "none", db, write_dx=False)}
        for sp in sorted(G._plain_splits(M, N, a.tokens)[1]):
            arms[f"w:{sp}"] = (lambda s_: (lambda: K.gemmp(x, g, trans_a=True, out=dW, beta=0.0, splits=s_,
                                                           variant=6)))(sp)
            arms[f"w:{sp}+bsum"] = (lambda s_: (lambda: K.gemmp(x, g, trans_a=True, out=dW, beta=0.0, splits=s_,
                                                                variant=6, bsum=db)))(sp)
        for fn in arms.values():   # warm every arm
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(a.rounds):   # interleaved: every arm once per round
            for k, fn in arms.items():
                t[k].append(_round(fn))
        med = {k: round(statistics.median(v), 4) for k, v in t.items()}
        fused = {k: v for k, v in med.items() if k.endswith("+bsum")}
        best = min(fused, key=fused.get)
        sp = G._bsum_splits(x, g, dW, 0.0, db)
        print(json.dumps({"a": [a.tokens, M], "b": [a.tokens, N], "plain_pick": plain_pick, "ms": med,
                          "best_fused": best, "fused_beats_plain+colsum": fused[best] < med["plain+colsum"],
                          "fused_over_plain_pct": round(100 * (fused[best] / med["plain"] - 1), 2),
                          "wgrad_matmul_decision": f"w:{sp}+bsum" if sp else "plain+colsum"}), flush=True)
        del x, g, dW, db


if __name__ == "__main__":
    main()
