"""Every dispatch path of the embedding kernels (csrc/kernels/embedding.hip)
against the fp64 references of tensorop_refs.py, with about 15 % of the ids out
of range (-1 and >= n): they read as zeros forward and add nothing backward.

  embed_fwd_kernel              none (a copy) / sum / avg, bf16 and fp32 tables, int32 and int64 ids
  embed_bwd_kernel              D < 64: one 8-column chunk per thread
  embed_bwd_wave_kernel         D >= 64: the 8-way unrolled loop (c + 7*64 < D, D >= 512) and its tail
  embed_reduce_copies_kernel    rows > 8 n: `copies` replicas of the table gradient, then their sum
  embed_bwd_small_kernel        n <= 8 without bags (its own tests are in test_kernels_gpu.py)

Bounds: forward `none` is torch.equal; forward sum / avg is one bf16 ulp per
element, or 8 x the fp32 floor (relative Frobenius) for fp32 tables; backward
is fp32 atomics in no fixed order: relative Frobenius error against 8 x the
fp32 floor, both measured against fp64 on a table gradient pre-filled with
0.5.  Rows that no valid id names keep 0.5 exactly.  The measured checks print
FIGURE lines (pytest -s); profiles/tensorops_tolerances.txt records them.
"""
import pytest
import torch

import tensorop_refs as R

pytestmark = pytest.mark.gpu

BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
FILL = 0.5


def _K():
    from flexflow_train_amd import kernels as K
    assert K.available(), "HIP kernel extension must be loaded on a GPU box"
    return K


def _copies(n, rows, D, aggr):
    """The replica count of kernels.embedding_bwd (its formula, restated)."""
    if rows <= 8 * n or (n <= 8 and aggr == "none"):
        return 1
    return int(min(256, rows // (8 * n), max(1, (64 << 20) // max(1, n * D * 4))))


def _figure(name, err, floor, what):
    bound = R.FLOOR_FACTOR * floor
    print(f"FIGURE {name} shape={what} floor={floor:.4e} bound={bound:.4e} kernel={err:.4e}")
    assert err <= bound, f"{name}: kernel error {err:.4e} above {R.FLOOR_FACTOR:g} x the fp32 floor {floor:.4e}"


def _check(name, n, D, idx_shape, aggr, dtype, itype, oor=0.15, idx=None, copies=None, forward=True, backward=True):
    K = _K()
    g = torch.Generator().manual_seed(n * 31 + D)
    if idx is None:
        idx = R.embedding_ids(idx_shape, n, seed=n + D, out_of_range=oor, dtype=itype)
    idx = idx.to(itype)
    L = 1 if aggr == "none" else idx.shape[-1]
    rows = idx.numel()
    tag = f"{name}.{aggr}.{'bf16' if dtype == BF else 'f32'}"
    what = f"n{n}xD{D}xrows{rows}xL{L}"
    if copies is not None:
        assert _copies(n, rows, D, aggr) == copies
    out_shape = tuple(idx.shape) + (D,) if aggr == "none" else tuple(idx.shape[:-1]) + (D,)
    if forward:
        W = torch.randn(n, D, generator=g).to(dtype)
        out = K.embedding_fwd(idx.cuda(), W.cuda(), aggr)
        ref = R.embedding_ref(idx, W, aggr)
        assert out.dtype == dtype and tuple(out.shape) == out_shape
        if aggr == "none":
            assert torch.equal(out.cpu(), ref.to(dtype))
        elif dtype == BF:
            R.assert_ulp(out, ref, dtype, tag + " forward")
        else:
            _figure("emb_fwd." + tag, R.relerr(out, ref), R.relerr(R.embedding_ref(idx, W, aggr, acc=F32), ref), what)
    if backward:
        dout = torch.randn(out_shape, generator=g).to(dtype)
        dW = torch.full((n, D), FILL, device="cuda")
        K.embedding_bwd(idx.cuda(), dout.cuda(), dW, aggr)
        torch.cuda.synchronize()
        dW = dW.cpu()
        ref = R.embedding_grad_ref(idx, dout, n, aggr, fill=FILL)
        lo = R.embedding_grad_ref(idx, dout, n, aggr, acc=F32, fill=FILL)
        _figure("emb_bwd." + tag, R.relerr(dW, ref), R.relerr(lo, ref), what)
        untouched = ~R.embedding_touched(idx, n)
        assert (dW[untouched] == FILL).all(), "a table row that no valid id names changed"


# (aggr, table dtype, id dtype): pruned so that every value of each occurs on every path
COMBOS3 = [("none", BF, I64), ("sum", F32, I32), ("avg", BF, I32)]
COMBOS2 = [("none", BF, I32), ("avg", F32, I64)]


def _ids(combos):
    return [f"{a}-{'bf16' if d == BF else 'f32'}-{'i32' if i == I32 else 'i64'}" for a, d, i in combos]


@pytest.mark.parametrize("aggr,dtype,itype", COMBOS3, ids=_ids(COMBOS3))
@pytest.mark.parametrize("D", [8, 24, 56])
def test_chunked_backward(D, aggr, dtype, itype):
    """D < 64: embed_bwd_kernel, 1, 3 and 7 chunks per row."""
    _check("chunk", 100, D, (32, 7), aggr, dtype, itype, copies=1)


WAVE = [(D,) + c for D in (64, 72, 256, 512, 520, 1088) for c in COMBOS2] + [(520, "sum", BF, I64)]


@pytest.mark.parametrize("D,aggr,dtype,itype", WAVE, ids=[f"D{w[0]}-{i}" for w, i in zip(WAVE, _ids([w[1:] for w in WAVE]))])
def test_wave_backward(D, aggr, dtype, itype):
    """embed_bwd_wave_kernel: tail only (64, 256); a tail that is no multiple of
    64 (72); exactly one unrolled trip (512); unrolled plus tail (520); two
    unrolled trips plus tail (1088)."""
    _check("wave", 100, D, (32, 7), aggr, dtype, itype, copies=1)


# (n, rows, copies, D, table dtype, id dtype): both scatter kernels (D = 32 chunked, D = 128 wave) at every count
REPLICAS = [(16, 256, 2, 32, BF, I32), (16, 256, 2, 128, F32, I64),
            (16, 4096, 32, 32, BF, I32), (16, 4096, 32, 128, F32, I64), (16, 4096, 32, 32, F32, I64),
            (16, 4096, 32, 128, BF, I32), (9, 18432, 256, 32, BF, I32), (9, 18432, 256, 128, F32, I64)]


@pytest.mark.parametrize("n,rows,copies,D,dtype,itype", REPLICAS,
                         ids=[f"copies{r[2]}-D{r[3]}-{'bf16' if r[4] == BF else 'f32'}" for r in REPLICAS])
def test_replicas(n, rows, copies, D, dtype, itype):
    """rows > 8 n: both scatter kernels write `copies` replicas (row bj -> replica
    bj % copies), embed_reduce_copies_kernel adds them onto dW; 256 is the cap."""
    _check(f"replica{copies}", n, D, (rows,), "none", dtype, itype, copies=copies)


def test_replicas_bagged():
    _check("replica32_bag", 16, 128, (1024, 4), "sum", BF, I64, copies=32)


@pytest.mark.parametrize("n,dtype,itype", [(8, BF, I64), (8, F32, I32), (9, BF, I64)], ids=["n8-bf16", "n8-f32", "n9-bf16"])
def test_small_table_boundary(n, dtype, itype):
    """rows = 3000, D = 136: n = 8 takes embed_bwd_small_kernel, n = 9 the wave kernel with 41 replicas."""
    _check("small_boundary", n, 136, (3000,), "none", dtype, itype, copies=1 if n == 8 else 41)


def test_small_table_with_bag_of_one():
    """n <= 8 with aggr = sum and L = 1 is not the small kernel's case (it has no
    bags): the wave kernel with replicas must serve it."""
    _check("small_sum_L1", 5, 136, (3000, 1), "sum", BF, I32, copies=75)


def test_small_table_id_below_template_width():
    """n = 3 runs the small kernel's E = 4 instance: id 3 is out of range but has an
    accumulator there.  Nothing may be added anywhere for it."""
    g = torch.Generator().manual_seed(40)
    idx = torch.randint(0, 4, (513,), generator=g)
    idx[:7] = 3
    assert (idx == 3).sum() > 50
    _check("small_id3", 3, 136, (513,), "none", BF, I64, idx=idx, copies=1)
    _check("small_only_id3", 3, 136, (64,), "none", BF, I64, idx=torch.full((64,), 3), copies=1)


def test_forward_second_trip():
    """B * D / 8 = 4100 * 256 chunks > 4096 blocks x 256 threads: embed_fwd_kernel loops again."""
    _check("fwd2", 500, 2048, (4100,), "none", BF, I32, backward=False)
    _check("fwd2", 500, 2048, (4100, 2), "avg", F32, I64, backward=False)


def test_wave_backward_second_trip():
    """16389 rows > 4096 blocks x 4 waves."""
    _check("wave2", 5000, 64, (16389,), "none", BF, I64, copies=1, forward=False)


def test_chunked_backward_second_trip():
    """1048600 one-chunk rows > 4096 blocks x 256 threads; rows <= 8 n keeps copies = 1."""
    _check("chunk2", 200000, 8, (1048600,), "none", BF, I32, copies=1, forward=False)


def test_replica_sum_second_trip():
    """n * D / 4 = 532480 vectors > 2048 blocks x 256 threads in
    embed_reduce_copies_kernel (copies = 2); no out-of-range ids, to keep the
    reference cheap."""
    _check("replica_sum2", 2080, 1024, (33280,), "none", BF, I64, oor=0.0, copies=2, forward=False)


@pytest.mark.parametrize("n,D,shape,aggr,dtype", [(50, 64, (300,), "none", BF), (50, 8, (60, 5), "sum", F32),
                                                  (4, 136, (300,), "none", BF), (9, 32, (600,), "none", F32)],
                         ids=["wave", "chunk", "small", "replicas"])
def test_all_ids_out_of_range(n, D, shape, aggr, dtype):
    """Forward is all zeros, backward leaves dW as it was (replicas: 600 rows > 8 * 9, 8 replicas that stay zero)."""
    K = _K()
    idx = R.embedding_ids(shape, n, seed=41, out_of_range=1.0)
    assert ((idx < 0) | (idx >= n)).all()
    W = torch.randn(n, D, generator=torch.Generator().manual_seed(42)).to(dtype)
    out = K.embedding_fwd(idx.cuda(), W.cuda(), aggr)
    assert (out == 0).all() and not torch.signbit(out).any()
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(43)).to(dtype)
    dW = torch.full((n, D), FILL, device="cuda")
    K.embedding_bwd(idx.cuda(), dout.cuda(), dW, aggr)
    torch.cuda.synchronize()
    assert (dW == FILL).all()
