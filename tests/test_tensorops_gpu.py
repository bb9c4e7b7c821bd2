"""Numerics of the general tensor-operator kernels (csrc/kernels/tensorops.hip)
against fp64 CPU references on the same rounded inputs (tensorop_refs.py),
plus the CPU mirror of the counter-based initialiser.

Bounds (tensorop_refs.py has the reasoning): data movement is compared with
torch.equal; element-wise results are held to one ulp of the output dtype
(2^-8 |ref| for bf16, 2^-22 |ref| for fp32); compare / ceil / round are exact;
sums, scatter-add, the MSE metric sums and the fast-intrinsic unary ops are held
to 8 x the fp32 floor measured in the test itself (a torch fp32 CPU evaluation
of the same formula against the fp64 reference).  Such checks print a line
that starts with FIGURE (pytest -s); profiles/tensorops_tolerances.txt records
them.

Sizes: every kernel launches through grid1 (at most 256 blocks of 256
threads), so n = 2 * 65536 + 37 = 131109 elements is the smallest tensor whose
grid-stride loop takes a second (and a partial third) trip; the 8-wide vector
path (2048 blocks x 256 threads x 8) needs 2 * 4194304 + 24.

Parity: reference kernel tests under lib/kernels/test/src/test_*_kernel.cc
(concat, split, reverse, gather, reduction, transpose, element-wise).
"""
import math

import numpy as np
import pytest
import torch

import tensorop_refs as R
from flexflow_train_amd.runtime.initializers import counter_init_piece, counter_spec

gpu = pytest.mark.gpu

N2 = 2 * 65536 + 37            # second grid-stride trip of a grid1 kernel
SHAPE2 = (3, 43703)            # N2 elements
NV2 = 2 * 4194304 + 24         # second trip of the 8-wide vector path


def _K():
    from flexflow_train_amd import kernels as K
    assert K.available(), "HIP kernel extension must be loaded on a GPU box"
    return K


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _floor_check(name, err, floor, shape):
    """A measured bound: the kernel's error against FLOOR_FACTOR x the fp32 floor."""
    bound = R.FLOOR_FACTOR * floor
    print(f"FIGURE {name} shape={'x'.join(map(str, shape))} floor={floor:.4e} bound={bound:.4e} kernel={err:.4e}")
    assert err <= bound, f"{name}: kernel error {err:.4e} above {R.FLOOR_FACTOR:g} x the fp32 floor {floor:.4e}"


# ---------------------------------------------------------------- CPU tests
def test_counter_init_is_layout_independent():
    spec = counter_spec({"type": "glorot_uniform"}, (24, 40))
    full = counter_init_piece(spec, (24, 40), [(0, 24), (0, 40)], 1234, "cpu")
    piece = counter_init_piece(spec, (24, 40), [(8, 16), (10, 30)], 1234, "cpu")
    assert torch.equal(full[8:16, 10:30], piece)
    b = math.sqrt(6.0 / 64)
    assert full.abs().max() <= b and full.std() > b / 3


def test_counter_init_distributions():
    n = 1 << 16
    x = counter_init_piece(counter_spec({"type": "normal", "mean": 1.0, "stddev": 2.0}, (n,)), (n,), [(0, n)], 7,
                           "cpu")
    assert abs(x.mean().item() - 1.0) < 0.05 and abs(x.std().item() - 2.0) < 0.05
    t = counter_init_piece(counter_spec({"type": "truncated_normal", "stddev": 1.0}, (n,)), (n,), [(0, n)], 7, "cpu")
    assert t.min() >= -2.0 and t.max() <= 2.0 and 0.8 < t.std().item() < 0.92
    c = counter_init_piece(counter_spec({"type": "constant", "value": 3.5}, (5, 3)), (5, 3), [(0, 5), (0, 3)], 7,
                           "cpu")
    assert torch.all(c == 3.5)


# ---------------------------------------------------------------- GPU tests
DT = [torch.float32, torch.bfloat16]
BCAST = [((4, 8, 16), (4, 8, 16)), ((4, 8, 16), (16,)), ((4, 1, 16), (1, 8, 1)), ((2, 3, 4, 5), (3, 1, 5)),
         ((7,), (1,)), ((4, 1, 16), (4, 1, 16))]
BIN_FN = {"EW_ADD": torch.add, "EW_SUB": torch.sub, "EW_MUL": torch.mul, "EW_DIV": torch.div,
          "EW_MAX": torch.maximum, "EW_MIN": torch.minimum}


def _binary_inputs(shapes, op, dtype, seed=0):
    g = _gen(seed)
    a = torch.randn(shapes[0], generator=g).to(dtype)
    b = torch.randn(shapes[1], generator=g).to(dtype)
    if op == "EW_DIV":
        b = (b.float().sign() * (b.float().abs() + 0.5)).to(dtype)
    return a, b


def _binary_grad_fn(op, which):
    """(a, b, dy) -> autograd gradient w.r.t. a (0) or b (1), in the precision of the inputs."""
    def fn(a, b, dy):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        BIN_FN[op](a, b).backward(dy)
        return (a.grad, b.grad)[which]
    return fn


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shapes", BCAST)
@pytest.mark.parametrize("op", ["EW_ADD", "EW_SUB", "EW_MUL", "EW_DIV", "EW_MAX", "EW_MIN"])
def test_binary_broadcast_fwd_bwd(dtype, shapes, op):
    K = _K()
    a, b = _binary_inputs(shapes, op, dtype)
    y = K.binary(a.cuda(), b.cuda(), op)
    ref = BIN_FN[op](a.double(), b.double())
    assert y.dtype == dtype
    R.assert_ulp(y, ref, dtype, f"{op} forward")
    dy = torch.randn(ref.shape, generator=_gen(1)).to(dtype)
    for which, src in ((0, a), (1, b)):
        g = K.binary_grad(dy.cuda(), a.cuda(), b.cuda(), op, which)
        assert g.shape == src.shape and g.dtype == dtype
        gfn = _binary_grad_fn(op, which)
        gref = gfn(a.double(), b.double(), dy.double())
        if tuple(src.shape) == tuple(ref.shape):
            # no reduction: at most three fp32 roundings (div) and the output rounding
            R.assert_ulp(g, gref, dtype, f"{op} grad {which}")
        else:
            floor = R.fp32_floor_rel(gfn, [a, b, dy], dtype)
            _floor_check(f"binary_grad.{op}.{which}.{'bf16' if dtype == torch.bfloat16 else 'f32'}",
                         R.relerr(g, gref), floor, tuple(ref.shape) + ("to",) + tuple(src.shape))


def _compare_check(op, fn, dtype):
    K = _K()
    a = torch.randint(0, 3, (6, 5), generator=_gen(0)).to(dtype)
    b = torch.randint(0, 3, (5,), generator=_gen(1)).to(dtype)
    y = K.binary(a.cuda(), b.cuda(), op)
    assert y.dtype == dtype and torch.equal(y.cpu(), fn(a, b).to(dtype))


CMP = [("EW_EQUAL", torch.eq), ("EW_GREATER", torch.gt), ("EW_LESS", torch.lt)]


@gpu
@pytest.mark.parametrize("op,fn", CMP)
def test_binary_compare(op, fn):
    _compare_check(op, fn, torch.float32)


@gpu
@pytest.mark.parametrize("op,fn", CMP)
def test_binary_compare_bf16(op, fn):
    _compare_check(op, fn, torch.bfloat16)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n", [8, 2048 * 8, 999, 1001])
def test_binary_vector_path_boundaries(dtype, n):
    """binary_flat8_kernel at one vector and at one full block row, and the
    n % 8 in {7, 1} fallback to binary_nd_kernel: no element dropped or left
    unwritten."""
    K = _K()
    a, b = _binary_inputs(((n,), (n,)), "EW_ADD", dtype, seed=n)
    for op in ("EW_ADD", "EW_MUL"):
        y = K.binary(a.cuda(), b.cuda(), op)
        R.assert_ulp(y, BIN_FN[op](a.double(), b.double()), dtype, f"{op} n={n}")


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_binary_unaligned_operand(dtype, which):
    """n = 4104 (a multiple of 8) with an operand that starts one element into a
    longer tensor, 2 or 4 bytes off 16-byte alignment: binary_nd's `aligned`
    test must send it to binary_nd_kernel, with the result of the aligned call."""
    K = _K()
    n = 4104
    a, b = _binary_inputs(((n + 1,), (n + 1,)), "EW_MUL", dtype, seed=3)
    ac, bc = a.cuda(), b.cuda()
    assert ac.data_ptr() % 16 == 0 and bc.data_ptr() % 16 == 0
    av, bv = ac[1:], bc[1:]
    aa, ba = av.clone(), bv.clone()
    assert av.data_ptr() % 16 != 0 and aa.data_ptr() % 16 == 0 and av.is_contiguous()
    y_aligned = K.binary(aa, ba, "EW_MUL")
    y = K.binary(av if which in ("a", "both") else aa, bv if which in ("b", "both") else ba, "EW_MUL")
    assert torch.equal(y, y_aligned)
    R.assert_ulp(y, a[1:].double() * b[1:].double(), dtype, "unaligned mul")


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_binary_second_trip_nd(dtype):
    """(3, 1) against (1, 43703): binary_nd_kernel and binary_grad_nd_kernel loop
    a second time; sum_to reduces 43703 (to a) and 3 (to b) elements per output."""
    K = _K()
    a, b = _binary_inputs(((3, 1), (1, SHAPE2[1])), "EW_MUL", dtype, seed=4)
    y = K.binary(a.cuda(), b.cuda(), "EW_SUB")
    assert tuple(y.shape) == SHAPE2
    R.assert_ulp(y, a.double() - b.double(), dtype, "sub, second trip")
    dy = torch.randn(SHAPE2, generator=_gen(5)).to(dtype)
    for which, src in ((0, a), (1, b)):
        g = K.binary_grad(dy.cuda(), a.cuda(), b.cuda(), "EW_MUL", which)
        gfn = _binary_grad_fn("EW_MUL", which)
        gref = gfn(a.double(), b.double(), dy.double())
        floor = R.fp32_floor_rel(gfn, [a, b, dy], dtype)
        _floor_check(f"binary_grad2.EW_MUL.{which}.{'bf16' if dtype == torch.bfloat16 else 'f32'}",
                     R.relerr(g, gref), floor, SHAPE2 + ("to",) + tuple(src.shape))


@gpu
@pytest.mark.parametrize("dtype,op", [(torch.float32, "EW_MUL"), (torch.bfloat16, "EW_ADD")])
def test_binary_second_trip_flat(dtype, op):
    """binary_flat8_kernel past 2048 blocks x 256 threads x 8 elements."""
    K = _K()
    a, b = _binary_inputs(((NV2,), (NV2,)), op, dtype, seed=6)
    y = K.binary(a.cuda(), b.cuda(), op)
    R.assert_ulp(y, BIN_FN[op](a.double(), b.double()), dtype, f"{op} flat, second trip")


SUM_TO = [((5, 7, 9, 4), (1, 7, 1, 4)),      # two reduced dims with a kept one between them
          ((70000, 3), (1, 3)),              # one long serial sum per output
          ((2, 65573), (1, 65573))]          # more outputs than one grid: sum_to_kernel's second trip


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("shape,target", SUM_TO)
def test_sum_to(shape, target, beta, dtype):
    """ext().sum_to: out = sum over the reduced dims of an fp32 tensor (+ beta * out)."""
    K = _K()
    g = _gen(7)
    full = torch.randn(shape, generator=g)
    old = torch.randn(target, generator=g).to(dtype)
    dims = [d for d in range(len(shape)) if target[d] != shape[d]]

    def fn(f, o):
        return f.sum(dims, keepdim=True) + beta * o

    out = old.cuda().clone()
    fc = full.cuda()
    K.ext().sum_to(K._dt(out), fc.data_ptr(), out.data_ptr(), list(shape), list(target), beta,
                   torch.cuda.current_stream().cuda_stream)
    floor = R.fp32_floor_rel(fn, [full, old], dtype)
    _floor_check(f"sum_to.beta{int(beta)}.{'bf16' if dtype == torch.bfloat16 else 'f32'}",
                 R.relerr(out, fn(full.double(), old.double())), floor, tuple(shape) + ("to",) + tuple(target))


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape,perm", [((4, 5, 6), (2, 0, 1)), ((2, 3, 4, 5), (0, 2, 1, 3)), ((8, 16), (1, 0)),
                                        ((2, 3, 4, 5, 6, 2), (5, 4, 3, 2, 1, 0)), (SHAPE2, (1, 0))])
def test_permute(dtype, shape, perm):
    K = _K()
    x = torch.randn(shape, generator=_gen(8)).to(dtype)
    assert torch.equal(K.permute(x.cuda(), perm).cpu(), x.permute(perm).contiguous())


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("axis", [0, 1, 2, -1])
def test_concat_split_reverse(dtype, axis):
    K = _K()
    xs = [torch.randn(3, 4, 5, device="cuda").to(dtype) for _ in range(2)]
    xs.append(torch.randn([3, 4, 5][:axis % 3] + [2] + [3, 4, 5][axis % 3 + 1:], device="cuda").to(dtype))
    y = K.concat(xs, axis)
    assert torch.equal(y, torch.cat(xs, axis))
    sizes = [int(x.shape[axis]) for x in xs]
    for a, b in zip(K.split(y, sizes, axis), torch.split(y, sizes, axis)):
        assert torch.equal(a, b.contiguous())
    assert torch.equal(K.reverse(y, axis), torch.flip(y, [axis]))


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_concat_split_reverse_second_trip(dtype):
    """slice_copy_multi_kernel (both directions) with a piece of 3 x 23703 > 65536
    elements beside a shorter one, and reverse_kernel on N2 elements."""
    K = _K()
    g = _gen(9)
    xs = [torch.randn(3, ln, generator=g).to(dtype) for ln in (20000, 23703)]
    ref = torch.cat(xs, 1)
    y = K.concat([x.cuda() for x in xs], 1)
    assert tuple(y.shape) == SHAPE2 and torch.equal(y.cpu(), ref)
    for a, b in zip(K.split(y, [20000, 23703], 1), xs):
        assert torch.equal(a.cpu(), b)
    for axis in (0, 1):
        assert torch.equal(K.reverse(y, axis).cpu(), torch.flip(ref, [axis]))


@gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_concat_split_many_pieces(axis):
    """More pieces than one launch carries (16): chunked multi-piece copies,
    pieces of different lengths (DLRM's interaction concat has 9)."""
    K = _K()
    xs = []
    for i in range(21):
        shp = [6, 8]
        shp[axis] = 1 + i % 4
        xs.append(torch.randn(shp, device="cuda").to(torch.bfloat16))
    y = K.concat(xs, axis)
    assert torch.equal(y, torch.cat(xs, axis))
    sizes = [int(x.shape[axis]) for x in xs]
    for a, b in zip(K.split(y, sizes, axis), torch.split(y, sizes, axis)):
        assert torch.equal(a, b.contiguous())


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("to_slice", [0, 1])
def test_slice_copy(to_slice, accumulate, dtype):
    """ext().slice_copy (the native executor's concat / split gradients): the
    slice [3, 5, 7] at offset 4 of a [3, 11, 7] tensor, copied or accumulated in
    either direction onto a pre-filled destination."""
    K = _K()
    outer, total, off, ln, inner = 3, 11, 4, 5, 7
    g = _gen(10)
    big = torch.randn(outer, total, inner, generator=g).to(dtype)
    sl = torch.randn(outer, ln, inner, generator=g).to(dtype)
    src, dst = (big, sl) if to_slice else (sl, big)
    out = dst.cuda().clone()
    sc = src.cuda()
    K.ext().slice_copy(K._dt(out), sc.data_ptr(), out.data_ptr(), outer, ln, inner, total, off, to_slice, accumulate,
                       torch.cuda.current_stream().cuda_stream)
    out = out.cpu()
    touched = torch.zeros(dst.shape, dtype=torch.bool)
    if to_slice:
        touched[:] = True
        moved = big[:, off:off + ln]
    else:
        touched[:, off:off + ln] = True
        moved = sl
    assert torch.equal(_bits(out)[~touched], _bits(dst)[~touched]), "the untouched region changed"
    if accumulate:
        R.assert_ulp(out[touched], dst.double()[touched] + moved.double().reshape(-1), dtype, "accumulate")
    else:
        assert torch.equal(_bits(out)[touched], _bits(moved).reshape(-1))


def _scatter_check(K, name, dy, idx, dim, x_shape):
    dx = K.scatter_add(dy.cuda(), idx.cuda(), dim, list(x_shape))
    assert dx.dtype == torch.float32
    ref = R.scatter_add_ref(dy, idx, dim, x_shape)
    lo = torch.zeros(tuple(x_shape)).scatter_add_(
        dim, R.wrap_index(idx, x_shape[dim])[0].clamp(0, x_shape[dim] - 1),
        torch.where(R.wrap_index(idx, x_shape[dim])[1], dy.float(), torch.zeros(())))
    _floor_check(name, R.relerr(dx, ref), R.relerr(lo, ref), tuple(idx.shape) + ("to",) + tuple(x_shape))
    untouched = R.scatter_count_ref(idx, dim, x_shape) == 0
    assert (dx.cpu()[untouched] == 0).all(), "an element no index points at is not 0"


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dim", [0, 1, 2])
@pytest.mark.parametrize("ibits", [torch.int32, torch.int64])
def test_gather_scatter(dtype, dim, ibits):
    """Negative (wrapping), out-of-range (gather 0, scatter skip) and duplicated indices."""
    K = _K()
    shape = (6, 50, 10)
    x = torch.randn(shape, generator=_gen(11)).to(dtype)
    ishape = list(shape)
    ishape[dim] = 13
    idx = R.edge_indices(ishape, shape[dim], seed=12 + dim, dtype=ibits)
    y = K.gather(x.cuda(), idx.cuda(), dim)
    assert y.dtype == dtype and torch.equal(_bits(y), _bits(R.gather_ref(x, idx, dim)))
    dy = torch.randn(ishape, generator=_gen(13)).to(dtype)
    _scatter_check(K, f"scatter_add.dim{dim}.{'bf16' if dtype == torch.bfloat16 else 'f32'}", dy, idx, dim, shape)


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_gather_scatter_second_trip(dtype):
    K = _K()
    x = torch.randn(3, 61, generator=_gen(14)).to(dtype)
    idx = R.edge_indices(SHAPE2, 61, seed=15, dtype=torch.int32)
    y = K.gather(x.cuda(), idx.cuda(), 1)
    assert torch.equal(_bits(y), _bits(R.gather_ref(x, idx, 1)))
    dy = torch.randn(SHAPE2, generator=_gen(16)).to(dtype)
    _scatter_check(K, f"scatter_add2.{'bf16' if dtype == torch.bfloat16 else 'f32'}", dy, idx, 1, (3, 61))


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_scatter_add_hot_address(dtype):
    """4096 contributions onto one element (named by k and by k - len) among 1000
    spread ones.  The addends are multiples of 2^-6 below 8, so every partial sum
    of the 4096 is exact in fp32 in any order: the atomics' order cannot move the
    result, the fp32 floor is 0 and the check is exact (a lost or doubled
    contribution is at least 2^-6)."""
    K = _K()
    idx = R.hot_indices(4096, 1000, 50, seed=17)
    dy = ((torch.randn(idx.numel(), generator=_gen(18)) * 64).round().clamp(-511, 511) / 64).to(dtype)
    assert torch.equal(dy.double(), (dy.double() * 64).round() / 64)
    _scatter_check(K, f"scatter_add_hot.{'bf16' if dtype == torch.bfloat16 else 'f32'}", dy, idx, 0, (50,))
    x = torch.randn(50, generator=_gen(19)).to(dtype)
    assert torch.equal(_bits(K.gather(x.cuda(), idx.cuda(), 0)), _bits(R.gather_ref(x, idx, 0)))


def _reduce_ref(xd, op, dims):
    if op == "sum":
        return xd.sum(dims)
    if op == "mean":
        return xd.mean(dims)
    if op == "max":
        return xd.amax(dims)
    if op == "min":
        return xd.amin(dims)
    for d in sorted(dims, reverse=True):
        xd = xd.prod(d)
    return xd


def _reduce_check(K, x, rng, op, dtype, name):
    """max / min are held to one output ulp (they move an input value), sum /
    mean / prod to the measured fp32 floor.

    Known difference, out of scope here: the kernel folds with fmaxf / fminf,
    which drop a NaN operand where torch propagates it, so no max / min input
    of this suite holds a NaN."""
    dims = tuple(range(rng[0], rng[1] + 1))
    y = K.reduce_contig(x.cuda(), rng[0], rng[1], op)
    ref = _reduce_ref(x.double(), op, dims)
    assert y.dtype == dtype and tuple(y.shape) == tuple(ref.shape)
    if op in ("max", "min"):
        R.assert_ulp(y, ref, dtype, name)
    else:
        floor = R.fp32_floor_rel(lambda t: _reduce_ref(t, op, dims), [x], dtype)
        _floor_check(f"reduce_{op}.{name}.{'bf16' if dtype == torch.bfloat16 else 'f32'}", R.relerr(y, ref), floor,
                     tuple(x.shape) + ("dims",) + dims)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("op", ["sum", "mean", "max", "min", "prod"])
@pytest.mark.parametrize("rng", [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2)])
def test_reduce(dtype, op, rng):
    x = (torch.rand(5, 7, 9, generator=_gen(20)) + 0.5).to(dtype)
    _reduce_check(_K(), x, rng, op, dtype, "small")


REDUCE_EDGE = {"last_dim_5000": ((4, 5000), (1, 1)),       # inner = 1, a long serial loop
               "outer_1": ((9, 7), (0, 0)),
               "red_1": ((5, 1, 7), (1, 1)),
               "second_trip": ((3, N2), (0, 0))}            # N2 outputs, red = 3


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("op", ["sum", "mean", "max", "min", "prod"])
@pytest.mark.parametrize("case", list(REDUCE_EDGE))
def test_reduce_edges(dtype, op, case):
    shape, rng = REDUCE_EDGE[case]
    g = _gen(21)
    if op == "prod" and case == "last_dim_5000":
        x = (1.0 + 0.01 * torch.randn(shape, generator=g)).to(dtype)    # the product of 5000 factors stays finite
    else:
        x = torch.randn(shape, generator=g).to(dtype)
    _reduce_check(_K(), x, rng, op, dtype, case)


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_reduce_inf_zero_sign(dtype):
    """max / min over rows that hold +-inf; prod with a zero and with sign changes."""
    K = _K()
    x = torch.randn(6, 33, generator=_gen(22)).to(dtype)
    x[0, 5], x[1, 7], x[2, 0], x[2, 32] = float("inf"), float("-inf"), float("inf"), float("-inf")
    x[3] = float("-inf")
    x[4] = float("inf")
    for op in ("max", "min"):
        y = K.reduce_contig(x.cuda(), 1, 1, op).cpu()
        assert torch.equal(_bits(y), _bits(_reduce_ref(x.float(), op, (1,)).to(dtype)))
        y0 = K.reduce_contig(x.cuda(), 0, 0, op).cpu()
        assert torch.equal(_bits(y0), _bits(_reduce_ref(x.float(), op, (0,)).to(dtype)))
    p = (torch.randn(4, 9, generator=_gen(23)).abs() + 0.5).to(dtype)
    p[0, 4] = 0.0                       # a zero: the product is exactly 0
    p[1, ::2] *= -1                     # five sign changes: negative
    p[2, 1::2] *= -1                    # four: positive
    p[3, 0] = -0.0                      # -0 times a positive rest
    y = K.reduce_contig(p.cuda(), 1, 1, "prod").cpu()
    ref = p.double().prod(1)
    assert y[0] == 0 and not torch.signbit(y[0]) and y[1] < 0 and y[2] > 0 and y[3] == 0 and torch.signbit(y[3])
    floor = R.fp32_floor_rel(lambda t: t.prod(1), [p], dtype)
    _floor_check(f"reduce_prod.signs.{'bf16' if dtype == torch.bfloat16 else 'f32'}", R.relerr(y, ref), floor, (4, 9))


def _topk_check(K, x, k):
    """K.topk of the CPU tensor x [rows, n] against topk_ref.  Everything is
    asserted on host copies, and the indices are range-checked before anything
    indexes with them."""
    n = x.shape[-1]
    v, i = K.topk(x.cuda(), k)
    torch.cuda.synchronize()
    v, i = v.cpu(), i.cpu()
    assert i.dtype == torch.int64 and v.dtype == x.dtype and tuple(i.shape) == tuple(x.shape[:-1]) + (k,)
    assert int(i.min()) >= 0 and int(i.max()) < n, f"index outside [0, {n}): {int(i.min())} .. {int(i.max())}"
    assert (i.sort(-1).values.diff(dim=-1) > 0).all() or k == 1, "indices of a row are not distinct"
    assert torch.equal(_bits(torch.gather(x, -1, i)), _bits(v)), "values are not x at the indices, bit for bit"
    tv, _ = torch.topk(x.float(), k, dim=-1)
    torch.testing.assert_close(v.float(), tv, rtol=0, atol=0, equal_nan=True)
    rv, ri = R.topk_ref(x, k)
    assert torch.equal(i, ri), "indices differ from the (NaN first, value desc, index asc) order"
    assert torch.equal(_bits(v), _bits(rv))


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,k", [(10, 1), (100, 5), (1000, 16), (4096, 64)])
def test_topk(dtype, n, k):
    x = torch.randn(13, n, generator=_gen(24)).to(dtype)
    _topk_check(_K(), x, k)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_topk_ties_and_specials(dtype, rows, n):
    """Tie-heavy rows, a constant row, rows with +inf / -inf / +0 / -0; k = 1, 8
    and n; rows = 5 leaves the second block one wave of its four."""
    K = _K()
    x = R.tie_heavy_rows(rows, n, seed=25 + n)
    if rows == 5:
        x[1] = 0.5
        if n >= 63:
            x[2, 3], x[2, 40], x[2, 7], x[2, 50] = float("inf"), float("inf"), float("-inf"), float("-inf")
            x[3, ::3] = -0.0
            x[3, 1::3] = 0.0
            x[4] = torch.randn(n, generator=_gen(26))
            x[4, 5], x[4, 6] = -0.0, 0.0
    x = x.to(dtype)
    for k in sorted({1, min(8, n), n}):
        _topk_check(K, x, k)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("tie_heavy", [False, True])
def test_topk_nan(dtype, tie_heavy):
    """Rows with 0, 1, k - 1, k + 3 and n NaNs at n = 100, k = 8: NaN sorts first
    (torch.topk's rule) and every index stays inside the row."""
    K = _K()
    n, k = 100, 8
    counts = [0, 1, k - 1, k + 3, n]
    x = R.tie_heavy_rows(len(counts), n, seed=27) if tie_heavy else torch.randn(len(counts), n, generator=_gen(28))
    for r, c in enumerate(counts):
        x[r, torch.randperm(n, generator=_gen(29 + r))[:c]] = float("nan")
    x = x.to(dtype)
    _topk_check(K, x, k)
    _topk_check(K, x, n)


FAST_OPS = [("POW", 3.0), ("LOG", 0.0), ("SQRT", 0.0), ("RSQRT", 0.0), ("SIN", 0.0), ("COS", 0.0)]


def _unary_fn(op, s):
    return {"SCALAR_ADD": lambda t: t + s, "SCALAR_SUB": lambda t: t - s, "SCALAR_MULTIPLY": lambda t: t * s,
            "SCALAR_TRUE_DIV": lambda t: t / s, "POW": lambda t: t ** s, "LOG": torch.log, "SQRT": torch.sqrt,
            "RSQRT": torch.rsqrt, "SIN": torch.sin, "COS": torch.cos,
            "LEAKYRELU": lambda t: torch.where(t > 0, t, t * s), "CEIL": torch.ceil, "ROUND": torch.round,
            "IDENTITY": lambda t: t}[op]


def _unary_grad_fn(op, s):
    fwd = _unary_fn(op, s)

    def fn(x, dy):
        if op in ("CEIL", "ROUND"):
            return torch.zeros_like(dy)
        x = x.clone().requires_grad_(True)
        fwd(x).backward(dy)
        return x.grad
    return fn


def _unary_input(op, n, dtype, seed=1):
    x = torch.randn(n, generator=_gen(seed)) * 3
    if op in ("LOG", "SQRT", "RSQRT"):
        x = x.abs() + 0.1
    if op in ("CEIL", "ROUND"):
        # halves (round is half-to-even), integers and both zeros among the rest
        x[:12] = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 6.5, 3.0, -4.0, 0.0, -0.0])
    return x.to(dtype)


def _unary_check(dtype, op, scalar, n):
    K = _K()
    tag = "bf16" if dtype == torch.bfloat16 else "f32"
    s = float(np.float32(scalar))          # the kernel receives the scalar as fp32
    x = _unary_input(op, n, dtype)
    dy = torch.randn(n, generator=_gen(2)).to(dtype)
    y = K.unary(x.cuda(), op, scalar)
    gx = K.unary(x.cuda(), op, scalar, dy=dy.cuda())
    fn, gfn = _unary_fn(op, s), _unary_grad_fn(op, s)
    ref, gref = fn(x.double()), gfn(x.double(), dy.double())
    assert y.dtype == dtype and gx.dtype == dtype
    if op in dict(FAST_OPS):
        _floor_check(f"unary_{op}.{tag}", R.maxabs(y, ref), R.fp32_floor_abs(fn, [x], dtype), (n,))
        _floor_check(f"unary_{op}_grad.{tag}", R.maxabs(gx, gref), R.fp32_floor_abs(gfn, [x, dy], dtype), (n,))
        return
    if op in ("CEIL", "ROUND", "IDENTITY"):
        assert torch.equal(_bits(y), _bits(R.round_to(ref, dtype)))
    else:
        R.assert_ulp(y, ref, dtype, op)
    if op in ("CEIL", "ROUND", "IDENTITY", "SCALAR_ADD", "SCALAR_SUB"):
        assert torch.equal(gx.cpu().float(), R.round_to(gref, dtype).float())
    else:
        R.assert_ulp(gx, gref, dtype, op + " grad")


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("op,scalar", [("SCALAR_ADD", 1.5), ("SCALAR_SUB", 0.5), ("SCALAR_MULTIPLY", -2.0),
                                       ("SCALAR_TRUE_DIV", 4.0), ("POW", 3.0), ("LOG", 0.0), ("SQRT", 0.0),
                                       ("RSQRT", 0.0), ("SIN", 0.0), ("COS", 0.0), ("LEAKYRELU", 0.1),
                                       ("CEIL", 0.0), ("ROUND", 0.0), ("IDENTITY", 0.0)])
def test_unary(dtype, op, scalar):
    """Scalar / piecewise ops and their gradients: one output ulp; ceil, round
    (half-to-even, with x.5 inputs) and identity exact.  pow / log / sqrt /
    rsqrt / sin / cos go through the fast intrinsics: largest absolute error of
    the op and of its gradient against 8 x the fp32 floor, on randn * 3 (abs +
    0.1 for log / sqrt / rsqrt), where __sinf / __cosf are in their accurate
    range."""
    _unary_check(dtype, op, scalar, 1000)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("op,scalar", [("LEAKYRELU", 0.1), ("ROUND", 0.0)])
def test_unary_second_trip(dtype, op, scalar):
    """unary_kernel forward and backward on N2 elements."""
    _unary_check(dtype, op, scalar, N2)


def _mse_check(dtype, shape, with_grad):
    K = _K()
    g = _gen(30)
    p = torch.randn(shape, generator=g).to(dtype)
    y = torch.randn(shape, generator=g).to(dtype)
    start = torch.tensor([3.25, -1.5])
    m = start.cuda()
    grad = torch.empty(shape, dtype=dtype, device="cuda") if with_grad else None
    K.mse(p.cuda(), y.cuda(), grad, m, 0.25)
    d = p.double() - y.double()
    if with_grad:
        R.assert_ulp(grad, 0.25 * d, dtype, "mse grad")
    ref = start.double() + torch.stack([(d * d).sum(), d.abs().sum()])
    d32 = p.float() - y.float()
    lo = start + torch.stack([(d32 * d32).sum(), d32.abs().sum()])
    _floor_check(f"mse_metrics.{'bf16' if dtype == torch.bfloat16 else 'f32'}", R.relerr(m, ref), R.relerr(lo, ref),
                 shape)


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_mse(dtype):
    """grad = scale (p - y) to one ulp; the two metric sums accumulate onto
    non-zero starting values."""
    _mse_check(dtype, (37, 19), True)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape,with_grad", [((37, 19), False), (SHAPE2, True), (SHAPE2, False)])
def test_mse_paths(dtype, shape, with_grad):
    """grad = None, and N2 elements: mse_kernel's second trip, 256 blocks whose
    partial sums meet in the last block to finish."""
    _mse_check(dtype, shape, with_grad)


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("label_f32", [False, True])
@pytest.mark.parametrize("with_grad", [True, False])
def test_mse_full(dtype, label_f32, with_grad):
    """mse_full on N2 elements: predictions in ``dtype`` with labels in the same
    dtype or fp32; loss += sq / cols, count += rows exactly once (every block
    contributes to the sums, the count is added once), sq and abs sums; slot 1 is not touched."""
    K = _K()
    rows, cols = SHAPE2
    g = _gen(31)
    p = torch.randn(SHAPE2, generator=g).to(dtype)
    y = torch.randn(SHAPE2, generator=g)
    y = y if label_f32 else y.to(dtype)
    start = torch.tensor([1.5, 9.0, 7.0, -2.25, 4.5, 11.0])
    m = start.cuda()
    grad = torch.empty(SHAPE2, dtype=dtype, device="cuda") if with_grad else None
    K.mse_full(p.cuda(), y.cuda(), grad, m, 0.5, cols, rows)
    m = m.cpu()
    d = p.double() - y.double()
    if with_grad:
        R.assert_ulp(grad, 0.5 * d, dtype, "mse_full grad")
    assert m[2].item() == 7.0 + rows and m[1].item() == 9.0 and m[5].item() == 11.0
    sums = [0, 3, 4]
    ref = start.double()[sums] + torch.stack([(d * d).sum() / cols, (d * d).sum(), d.abs().sum()])
    d32 = p.float() - y.float()
    lo = start[sums] + torch.stack([(d32 * d32).sum() / cols, (d32 * d32).sum(), d32.abs().sum()])
    _floor_check(f"mse_full_metrics.{'bf16' if dtype == torch.bfloat16 else 'f32'}.label_{'f32' if label_f32 else 'same'}",
                 R.relerr(m[sums], ref), R.relerr(lo, ref), SHAPE2)


@gpu
@pytest.mark.parametrize("init", [{"type": "uniform", "min": -0.3, "max": 0.7}, {"type": "glorot_uniform"},
                                  {"type": "normal", "mean": 0.1, "stddev": 0.5}, {"type": "truncated_normal"},
                                  {"type": "constant", "value": -1.25}, {"type": "zero"}])
def test_init_gpu_matches_cpu_mirror(init):
    _K()
    full = (64, 48)
    box = [(16, 48), (8, 40)]
    spec = counter_spec(init, full)
    g = counter_init_piece(spec, full, box, 99, "cuda")
    c = counter_init_piece(spec, full, box, 99, "cpu")
    assert g.shape == (32, 32)
    torch.testing.assert_close(g.cpu(), c, rtol=1e-4, atol=1e-4)
    whole = counter_init_piece(spec, full, [(0, 64), (0, 48)], 99, "cuda")
    assert torch.equal(whole[16:48, 8:40], g)


@gpu
@pytest.mark.parametrize("init", [{"type": "uniform", "min": -0.3, "max": 0.7},
                                  {"type": "normal", "mean": 0.1, "stddev": 0.5}])
def test_init_second_trip(init):
    """init_kernel on a piece of N2 elements inside a larger logical tensor."""
    _K()
    full = (5, SHAPE2[1] + 9)
    box = [(1, 4), (4, 4 + SHAPE2[1])]
    spec = counter_spec(init, full)
    g = counter_init_piece(spec, full, box, 77, "cuda")
    c = counter_init_piece(spec, full, box, 77, "cpu")
    assert tuple(g.shape) == SHAPE2
    torch.testing.assert_close(g.cpu(), c, rtol=1e-4, atol=1e-4)
