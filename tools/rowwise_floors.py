"""Floors behind the fp32 bounds of tests/test_rowwise_paths_gpu.py.

For every fp32 bound of that file: the test's own reference formula evaluated
in torch fp32 on the CPU, on the test's inputs, against its fp64 evaluation
(relative Frobenius error; absolute error for tanh near zero).  The bound is
8x the largest floor over the cases, rounded up to one significant digit.

    python tools/rowwise_floors.py                      # floors and bounds
    python tools/rowwise_floors.py --observed LOG ...   # + the kernels' maxima

LOG is the output of `pytest -s tests/test_rowwise_paths_gpu.py` on the GPU
(its "OBS <bound> <case> <error> <bound value>" lines).
"""
import argparse
import collections
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_rowwise_paths_gpu as T  # noqa: E402

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
rel = T._rel64


def bound_of(floor: float) -> float:
    if floor == 0.0:
        return 0.0
    v = 8 * floor
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def floors():
    fl = collections.defaultdict(float)

    def put(key, v):
        fl[key] = max(fl[key], v)

    # softmax + CE
    for case, (dtype, M, V, Vv) in T.CE_CASES.items():
        for logits, labels, isbig, _ in T.ce_inputs(dtype, M, V, Vv):
            scale = T._f32(1.0 / 16)
            l64, g64, _, _ = T.ce_ref(logits, labels, Vv, scale, F64)
            l32, g32, _, _ = T.ce_ref(logits, labels, Vv, scale, F32)
            for sel, sfx in ((~isbig, ""), (isbig, "_big")):
                if sel.any():
                    put("ce_loss" + sfx, rel(l32[sel], l64[sel]))
                    if dtype == F32:
                        put("ce_grad" + sfx, rel(g32[sel], g64[sel]))
    for N in (1, 7, 200, 257, 1000):
        x, dy = T.softmax_inputs(F32, N)
        y64 = T.softmax_ref(x, F64)
        put("softmax_fwd", rel(T.softmax_ref(x, F32), y64))
        y = y64.float()
        put("softmax_bwd", rel(T.softmax_bwd_ref(dy, y, F32), T.softmax_bwd_ref(dy, y, F64)))
    # optimizers: the fp32 evaluation carries the state, each step is compared
    # with the fp64 step from the same state
    for layout in ("n8", "n8p4"):
        for gdt in (F32, BF16):
            for dec in (False, True):
                for gs in (1.0, 1.0 / 128):
                    n = T.ADAM_N[layout]
                    w, grads = T.opt_inputs(n, gdt)
                    m, v = torch.zeros(n), torch.zeros(n)
                    for step in (1, 2, 3):
                        g = grads[step - 1]
                        w64, m64, v64 = T.adam_ref(w, g, m, v, step, gs, dec, F64)
                        w32, m, v = T.adam_ref(w, g, m, v, step, gs, dec, F32)
                        put("adam_update", rel(w32.double() - w.double(), w64 - w.double()))
                        put("adam_m_v", max(rel(m, m64), rel(v, v64)))
                        w = w32
    for case, (gdt, has_mom, nesterov, gs) in T.SGD_CASES.items():
        n = 8 * 1031 + 4
        w, grads = T.opt_inputs(n, gdt, seed=23)
        mom = torch.zeros(n) if has_mom else None
        for step in (1, 2, 3):
            g = grads[step - 1]
            w64, mom64 = T.sgd_ref(w, g, mom, nesterov, gs, F64)
            w32, mom = T.sgd_ref(w, g, mom, nesterov, gs, F32)
            put("sgd_update", rel(w32.double() - w.double(), w64 - w.double()))
            if has_mom:
                put("sgd_mom", rel(mom, mom64))
            w = w32
    for n in T.SUMSQ_N:
        x = T.sumsq_inputs(n)
        r64 = T.sumsq_ref(x, 0.5, F64).item()
        put("sum_squares", abs(T.sumsq_ref(x, 0.5, F32).item() - r64) / r64)
    # layernorm: fp32 y / dx, and the column sums (fp32 outputs for both input
    # types).  As in the test, the statistics come from the unrounded x [+ r]
    # and only xhat's numerator from the stored, rounded sum.
    def put_ln(sub, v):
        put("ln_colsum", v)
        put("ln_colsum." + sub, v)

    for M, N in T.LN_SHAPES:
        for dtype in (F32, BF16):
            dt = "f32" if dtype == F32 else "bf16"
            x, r, dy, dres, gamma, beta, start = T.ln_inputs(M, N, dtype)
            for rr, gm, dr in ((None, gamma, None), (r, gamma, dres), (r, None, None), (None, gamma, dres)):
                s = x if rr is None else (x.float() + rr.float()).to(dtype)
                dx64, dg64, db64 = T.ln_bwd_ref(dy, s, x, rr, gm, dr, F64)
                dx32, dg32, db32 = T.ln_bwd_ref(dy, s, x, rr, gm, dr, F32)
                put_ln("dgamma_" + dt, rel(start[0] + dg32, start[0].double() + dg64))
                put_ln("dbeta_" + dt, rel(start[1] + db32, start[1].double() + db64))
                if dtype == F32:
                    bt = None if gm is None else beta
                    put("ln_y_f32", rel(T.ln_fwd_ref(x, rr, gm, bt, F32), T.ln_fwd_ref(x, rr, gm, bt, F64)))
                    put("ln_dx_f32", rel(dx32, dx64))
                    # dsum: the column sum of the fp32 dx itself
                    put_ln("dsum_f32", rel(start[2] + dx32.sum(0), start[2].double() + dx32.double().sum(0)))
    # activations
    for act in T.ACTS:
        for M, N in T.ACT_SHAPES:
            for dtype in (F32, BF16):
                x, bias, dy = T.act_inputs(act, M, N, dtype)
                start = torch.linspace(-1, 1, N)
                u32 = x.float() + bias.float()
                pre = u32.to(dtype)
                g64 = dy.double() * T.act_grad_fn(act, pre.double(), True)
                g32 = dy.float() * T.act_grad_fn(act, pre.float(), False)
                put("act_dbias_" + act, rel(start + g32.sum(0), start.double() + g64.sum(0)))
                put("act_dbias_none", rel(start + dy.float().sum(0), start.double() + dy.double().sum(0)))
                if dtype != F32:
                    continue
                for u in (u32, x):
                    y64 = T.act_fn(act, u.double() if u is x else x.double() + bias.double(), True)
                    y32 = T.act_fn(act, u, False)
                    put("act_fwd_" + act, rel(y32, y64))
                    if act == "tanh":
                        put("tanh0_abs", (y32[:, 2:4].double() - y64[:, 2:4]).abs().max().item())
                put("act_bwd_" + act, rel(g32, g64))
    return fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--observed", nargs="*", default=[], help="pytest -s logs from the GPU")
    args = ap.parse_args()
    torch.set_num_threads(1)   # one summation order
    fl = floors()
    obs = collections.defaultdict(float)
    nobs = collections.Counter()
    for path in args.observed:
        for line in open(path):
            i = line.find("OBS ")
            if i < 0:
                continue
            f = line[i:].split()
            if len(f) >= 5:
                # "bound.part" is one part of the checks that share a bound: it
                # gets a line of its own and counts towards the bound's line
                for key in {f[1], f[1].split(".")[0]}:
                    obs[key] = max(obs[key], float(f[3]))
                    nobs[key] += 1
    # bounds that are not 8x a floor: bf16 output rounding (test_kernels_gpu.py's
    # constants, one value's worst case)
    fixed = {"bf16_elem": 2.0 ** -8, "bf16_out": T._BF, "bf16_op": T._BF_OP}
    print(f"{'name':<24}{'fp32 floor':>12}{'bound':>10}{'kernel max':>12}{'checks':>8}")
    for key in sorted(set(fl) | set(obs)):
        base = key.split(".")[0]
        floor = f"{fl[key]:.2e}" if key in fl else "-"
        bound = bound_of(fl[base]) if base in fl else fixed.get(base, float("nan"))
        seen = f"{obs[key]:.2e}" if key in obs else "-"
        print(f"{key:<24}{floor:>12}{bound:>10.0e}{seen:>12}{nobs[key]:>8}")


if __name__ == "__main__":
    main()
