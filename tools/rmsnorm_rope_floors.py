"""Floors behind the fp32 bounds of tests/test_rmsnorm_rope_gpu.py.

For every fp32 bound of that file: the test's own reference formula evaluated
in torch fp32 on the CPU, on the test's inputs, against its fp64 evaluation
(relative Frobenius error).  The bound is 8x the largest floor over the cases,
rounded up to one significant digit (the rule of
profiles/r9/rowwise_tolerances.txt).

    python tools/rmsnorm_rope_floors.py                      # floors and bounds
    python tools/rmsnorm_rope_floors.py --observed LOG ...   # + the kernels' maxima

LOG is the output of `pytest -s tests/test_rmsnorm_rope_gpu.py` on the GPU
(its "OBS <bound> <case> <error> <bound value>" lines).
"""
import argparse
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import test_rmsnorm_rope_gpu as T  # noqa: E402
from rowwise_floors import bound_of  # noqa: E402

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
rel = T._rel64


def floors():
    fl = collections.defaultdict(float)

    def put(key, v):
        fl[key] = max(fl[key], v)

    # RMSNorm: fp32 y / dx / rstd, and dgamma (an fp32 output for both input
    # types).  As in the test, rstd comes from the unrounded x [+ r] and xhat's
    # numerator from the stored, rounded sum.
    for M, N in T.RMS_SHAPES:
        for dtype in (F32, BF16):
            dt = "f32" if dtype == F32 else "bf16"
            x, r, dy, dres, gamma, start = T.rms_inputs(M, N, dtype)
            for rr, gm, dr in ((r, gamma, dres), (None, gamma, None), (r, None, None), (None, gamma, dres)):
                s = x if rr is None else (x.float() + rr.float()).to(dtype)
                dx64, dg64 = T.rms_bwd_ref(dy, s, x, rr, gm, dr, F64)
                dx32, dg32 = T.rms_bwd_ref(dy, s, x, rr, gm, dr, F32)
                for key in ("rms_dgamma", "rms_dgamma." + dt):
                    put(key, rel(start + dg32, start.double() + dg64))
                put("rms_rstd", rel(T.rms_stats(x, rr, F32)[1], T.rms_stats(x, rr, F64)[1]))
                if dtype == F32:
                    put("rms_y_f32", rel(T.rms_fwd_ref(x, rr, gm, F32), T.rms_fwd_ref(x, rr, gm, F64)))
                    put("rms_dx_f32", rel(dx32, dx64))
    # RoPE in fp32 from the wrapper's own table (built on the CPU here: the
    # same fp64 computation, rounded once)
    from flexflow_train_amd import kernels as K
    for shape, sd in T.ROPE_SHAPES:
        x = T.rope_inputs(shape, F32)
        table = K.rope_table(shape[sd], shape[-1], T._THETA, "cpu")
        for inter in (False, True):
            for inv in (False, True):
                put("rope_f32", rel(T.rope_ref(x, table, sd, inter, inv, F32), T.rope_ref(x, table, sd, inter, inv, F64)))
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
                for key in {f[1], f[1].split(".")[0]}:
                    obs[key] = max(obs[key], float(f[3]))
                    nobs[key] += 1
    # bounds that are not 8x a floor: bf16 output rounding (the constants of
    # test_rowwise_paths_gpu.py), the table's one fp32 rounding, and the
    # there-and-back bound worked out in test_rope_paths
    fixed = {"bf16_out": T._BF, "bf16_op": T._BF_OP, "rope_table_abs": T._TABLE_ABS,
             "rope_roundtrip_bf16": 2.0 ** -21 + 2.0 ** -7, "rope_roundtrip_f32": 2.0 ** -21}
    print(f"{'name':<24}{'fp32 floor':>12}{'bound':>10}{'kernel max':>12}{'checks':>8}")
    for key in sorted(set(fl) | set(obs)):
        base = key.split(".")[0]
        floor = f"{fl[key]:.2e}" if key in fl else "-"
        bound = bound_of(fl[base]) if base in fl else fixed.get(base, float("nan"))
        seen = f"{obs[key]:.2e}" if key in obs else "-"
        print(f"{key:<24}{floor:>12}{bound:>10.0e}{seen:>12}{nobs[key]:>8}")


if __name__ == "__main__":
    main()
