"""CPU checks of tests/tensorop_refs.py: each fp64 reference equals torch on
the inputs torch accepts, the kernels' extra index rules do what the module's
header says, and the input builders meet the conditions the GPU suites
(test_tensorops_gpu.py, test_embedding_paths_gpu.py) rely on.
"""
import pytest
import torch
import torch.nn.functional as F

import tensorop_refs as R


# ------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("dim", [0, 1, 2])
def test_gather_scatter_refs_equal_torch_on_valid_indices(dim):
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(6, 50, 10, generator=g).to(torch.bfloat16)
    ishape = [6, 50, 10]
    ishape[dim] = 13
    idx = torch.randint(0, x.shape[dim], ishape, generator=g)
    assert torch.equal(R.gather_ref(x, idx, dim), torch.gather(x, dim, idx))
    dy = torch.randn(ishape, generator=g).to(torch.bfloat16)
    ref = torch.zeros(x.shape, dtype=torch.float64).scatter_add_(dim, idx, dy.double())
    assert torch.equal(R.scatter_add_ref(dy, idx, dim, x.shape), ref)
    cnt = torch.zeros(x.shape, dtype=torch.int64).scatter_add_(dim, idx, torch.ones(ishape, dtype=torch.int64))
    assert torch.equal(R.scatter_count_ref(idx, dim, x.shape), cnt)


def test_gather_scatter_refs_index_rule():
    x = torch.arange(1.0, 6.0)                       # len 5
    idx = torch.tensor([0, 4, -1, -5, 5, -6, 100, -100])
    y = R.gather_ref(x, idx, 0)
    assert y.tolist() == [1.0, 5.0, 5.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    dx = R.scatter_add_ref(torch.ones(8), idx, 0, (5,))
    assert dx.tolist() == [2.0, 0.0, 0.0, 0.0, 2.0] and dx.dtype == torch.float64
    assert R.scatter_count_ref(idx, 0, (5,)).tolist() == [2, 0, 0, 0, 2]
    # negative indices equal torch on their wrapped value
    k = torch.tensor([-1, -3, 2])
    assert torch.equal(R.gather_ref(x, k, 0), x[k])


# ---------------------------------------------------------------------- top-k
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_ref_equals_torch(dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 100, generator=g).to(dtype)
    x[1, :3] = float("nan")
    x[2, 7] = float("inf")
    x[2, 9] = float("-inf")
    x[3] = float("nan")
    for k in (1, 8, 100):
        v, i = R.topk_ref(x, k)
        tv, _ = torch.topk(x.float(), k, dim=-1)
        assert v.dtype == dtype and i.dtype == torch.int64
        torch.testing.assert_close(v.float(), tv, rtol=0, atol=0, equal_nan=True)
        assert torch.equal(torch.gather(x, -1, i).view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           v.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


def test_topk_ref_order():
    nan = float("nan")
    x = torch.tensor([[1.0, nan, 3.0, 3.0, -0.0, 0.0, nan, float("inf")]])
    v, i = R.topk_ref(x, 8)
    assert i.tolist() == [[1, 6, 7, 2, 3, 0, 4, 5]]   # NaN by index, inf, the tied 3s by index, 1, -0 before +0 by index
    assert torch.isnan(v[0, :2]).all() and v[0, 2:].tolist() == [float("inf"), 3.0, 3.0, 1.0, -0.0, 0.0]
    assert torch.signbit(v[0, 6]) and not torch.signbit(v[0, 7])


def test_tie_heavy_rows_condition():
    x = R.tie_heavy_rows(5, 100, seed=11)
    assert torch.equal(x.to(torch.bfloat16).float(), x)            # ties survive bf16
    assert R.tied_pick_share(x, 8) >= 0.30
    assert R.tied_pick_share(R.tie_heavy_rows(5, 65, seed=12), 65) >= 0.30
    # the measure itself: a row of distinct values has no tied pick
    assert R.tied_pick_share(torch.arange(20.0).reshape(2, 10), 4) == 0.0


# ------------------------------------------------------------------- builders
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape,length", [((6, 13, 10), 50), ((13, 50, 10), 6), ((6, 50, 13), 10), ((3, 43703), 3)])
def test_edge_indices_condition(shape, length, dtype):
    idx = R.edge_indices(shape, length, seed=5, dtype=dtype)
    assert idx.dtype == dtype and tuple(idx.shape) == shape
    neg, oor = R.index_shares(idx, length)
    assert neg >= 0.10 and oor >= 0.10
    k = idx.long()
    assert (k >= length).any() and (k < -length).any()            # out of range on both sides
    assert (k == length // 3).double().mean() >= 0.15             # the duplicated share
    _, valid = R.wrap_index(idx, length)
    assert 0.5 < valid.double().mean() < 0.9


def test_hot_indices_condition():
    idx = R.hot_indices(4096, 1000, 50, seed=9)
    cnt = R.scatter_count_ref(idx, 0, (50,))
    assert int(cnt.max()) >= 4096 and int(cnt.max()) >= 1000
    assert int((cnt > 0).sum()) > 40                               # and a spread remainder
    assert (idx < 0).any() and (idx >= 0).any()                    # the hot address is named both ways


def test_embedding_ids_condition():
    for n in (3, 100, 5000):
        idx = R.embedding_ids((32, 7), n, seed=2)
        k = idx.reshape(-1)
        share = ((k < 0) | (k >= n)).double().mean().item()
        assert 0.12 <= share <= 0.18
        assert (k == -1).any() and (k >= n).any() and (k == n).any()
    assert ((R.embedding_ids((64,), 10, seed=2, out_of_range=0.0) >= 0).all())


# ------------------------------------------------------------------ embedding
@pytest.mark.parametrize("aggr", ["none", "sum", "avg"])
def test_embedding_refs_equal_torch_on_valid_ids(aggr):
    g = torch.Generator().manual_seed(4)
    n, D = 40, 24
    W = torch.randn(n, D, generator=g, dtype=torch.float64).requires_grad_(True)
    idx = torch.randint(0, n, (9, 5), generator=g)
    if aggr == "none":
        out = F.embedding(idx, W)
    else:
        out = F.embedding_bag(idx, W, mode="sum" if aggr == "sum" else "mean")
    ref = R.embedding_ref(idx, W.detach(), aggr)
    torch.testing.assert_close(ref, out.detach(), rtol=1e-14, atol=1e-14)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    torch.testing.assert_close(R.embedding_grad_ref(idx, dout, n, aggr), W.grad, rtol=1e-13, atol=1e-13)
    assert torch.equal(R.embedding_touched(idx, n), (W.grad != 0).any(-1))


@pytest.mark.parametrize("aggr", ["none", "sum", "avg"])
def test_embedding_refs_out_of_range_rule(aggr):
    """Ids outside [0, n) add nothing; AVG still divides by the bag length."""
    n, D = 5, 8
    W = torch.arange(1.0, n * D + 1).reshape(n, D)
    idx = torch.tensor([[0, -1, 4, 5], [7, -1, -2, 5]])
    ref = R.embedding_ref(idx, W, aggr)
    if aggr == "none":
        assert torch.equal(ref[0, 0], W[0].double()) and torch.equal(ref[0, 2], W[4].double())
        assert (ref[0, 1] == 0).all() and (ref[0, 3] == 0).all() and (ref[1] == 0).all()
    else:
        div = 4.0 if aggr == "avg" else 1.0
        assert torch.equal(ref[0], (W[0] + W[4]).double() / div) and (ref[1] == 0).all()
    dout = torch.ones(ref.shape)
    dW = R.embedding_grad_ref(idx, dout, n, aggr)
    scale = 0.25 if aggr == "avg" else 1.0
    assert torch.equal(dW[0], torch.full((D,), scale, dtype=torch.float64)) and torch.equal(dW[0], dW[4])
    assert (dW[1:4] == 0).all()
    assert R.embedding_touched(idx, n).tolist() == [True, False, False, False, True]


# --------------------------------------------------------------------- bounds
def test_assert_ulp_and_floors():
    ref = torch.tensor([1.0, -2.0, 0.0, float("inf")], dtype=torch.float64)
    R.assert_ulp(ref.float().to(torch.bfloat16), ref, torch.bfloat16)
    R.assert_ulp(torch.tensor([1.0 + 2.0 ** -8, -2.0, 0.0, float("inf")]), ref, torch.bfloat16)
    for bad in ([1.0 + 2.0 ** -7, -2.0, 0.0, float("inf")], [1.0, -2.0, 1e-30, float("inf")],
                [1.0, -2.0, 0.0, 3.0e38], [float("nan"), -2.0, 0.0, float("inf")]):
        with pytest.raises(AssertionError):
            R.assert_ulp(torch.tensor(bad), ref, torch.bfloat16)
    with pytest.raises(AssertionError):                            # a truncating kernel: one whole ulp low
        R.assert_ulp(torch.tensor([1.0 + 2.0 ** -21]), torch.tensor([1.0], dtype=torch.float64), torch.float32)
    x = torch.rand(70000, 3, generator=torch.Generator().manual_seed(1))
    fl = R.fp32_floor_rel(lambda t: t.sum(0), [x])
    assert 0 < fl < 1e-5
    assert 1e-4 < R.fp32_floor_rel(lambda t: t.sum(0), [x], torch.bfloat16) < 2.0 ** -8
    assert R.fp32_floor_abs(torch.sin, [x]) < 1e-6
