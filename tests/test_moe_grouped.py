"""CPU checks of the MoE routing / grouped-GEMM references (the oracles of
tests/test_moe_grouped_gpu.py) against the argsort-based order of the
per-expert path of ops/moe.py."""
import pytest
import torch

from flexflow_train_amd import kernels as K


def _argsort_route(ids, e0, El):
    """The per-expert path's routing (ops/moe.py ExpertsOp.forward, replicated mode)."""
    eg = ids.reshape(-1).long()
    sel = ((eg >= e0) & (eg < e0 + El)).nonzero().squeeze(1)
    le = eg[sel] - e0
    order = torch.argsort(le, stable=True)
    return sel[order], torch.bincount(le, minlength=El)


def _ids(B, k, E, unused=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    pool = [e for e in range(E) if e != unused]
    rows = [torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]] for _ in range(B)]
    return torch.stack(rows).to(torch.int32)


@pytest.mark.parametrize("B,k,E,e0,El,unused", [
    (257, 2, 8, 0, 8, 5),      # an expert nobody selects
    (100, 2, 8, 2, 3, None),   # sharded window: most pairs are not local
    (100, 2, 8, 2, 3, 3),      # window with an empty expert
    (1, 2, 4, 0, 4, None),
])
def test_route_reference_matches_argsort(B, k, E, e0, El, unused):
    ids = _ids(B, k, E, unused)
    r = K.moe_route(ids, e0, El)     # CPU tensors: the reference
    sel, counts = _argsort_route(ids, e0, El)
    n = sel.numel()
    P = B * k
    assert r.offsets.tolist() == [0] + torch.cumsum(counts, 0).tolist()
    assert int(r.offsets[-1]) == n
    assert torch.equal(r.perm[:n].long(), sel)
    assert bool(((r.perm >= 0) & (r.perm < P)).all())
    pos = torch.full((P,), -1, dtype=torch.long)
    pos[sel] = torch.arange(n)
    assert torch.equal(r.pos.reshape(-1).long(), pos)
    if unused is not None and e0 <= unused < e0 + El:
        assert counts[unused - e0] == 0
    # tile map: every 64-row tile of every expert, in order
    T = (P + 63) // 64 + El
    assert r.tile_group.numel() == T and r.tile_row0.numel() == T
    nt = int(r.n_tiles)
    assert nt == int(((counts + 63) // 64).sum())
    off = r.offsets.tolist()
    seen = []
    for t in range(nt):
        e, r0 = int(r.tile_group[t]), int(r.tile_row0[t])
        assert off[e] <= r0 < off[e + 1] and (r0 - off[e]) % 64 == 0
        seen.append((e, r0))
    assert seen == sorted(seen) and len(set(seen)) == nt
    assert bool((r.tile_group[nt:] == -1).all()) and bool((r.tile_row0[nt:] == n).all())


def test_gather_combine_dgate_references():
    torch.manual_seed(1)
    B, k, E, D = 37, 2, 6, 16
    ids = _ids(B, k, E, unused=4)
    e0, El = 1, 4
    r = K.moe_route(ids, e0, El)
    sel, _ = _argsort_route(ids, e0, El)
    n = sel.numel()
    tok = torch.arange(B).repeat_interleave(k)
    x, gate = torch.randn(B, D), torch.rand(B, k)
    xs = K.moe_gather_rows(x, r)
    assert torch.equal(xs[:n], x[tok[sel]]) and not xs[n:].any()
    xg = K.moe_gather_rows(x, r, scale=gate)
    torch.testing.assert_close(xg[:n], x[tok[sel]] * gate.reshape(-1)[sel].unsqueeze(1))
    y = torch.randn(B * k, D)
    ref = torch.zeros(B, D).index_add_(0, tok[sel], y[:n] * gate.reshape(-1)[sel].unsqueeze(1))
    torch.testing.assert_close(K.moe_combine(y, r, gate), ref)
    ref1 = torch.zeros(B, D).index_add_(0, tok[sel], y[:n])
    torch.testing.assert_close(K.moe_combine(y, r), ref1)
    dout = torch.randn(B, D)
    dg = torch.zeros(B * k)
    dg[sel] = (dout[tok[sel]] * y[:n]).sum(1)
    torch.testing.assert_close(K.moe_dgate(dout, y, r).reshape(-1), dg)


def test_grouped_gemm_reference_forms():
    torch.manual_seed(2)
    B, k, E, Kd, N = 50, 2, 5, 16, 24
    ids = _ids(B, k, E, unused=2)
    r = K.moe_route(ids, 0, E)
    off = r.offsets.tolist()
    a, w = torch.randn(B * k, Kd), torch.randn(E, Kd, N)
    bias = torch.randn(E, N)
    pre = torch.zeros(B * k, N)
    out = K.grouped_gemm(a, w, r, "nn", bias=bias, act="relu", pre=pre)
    for e in range(E):
        u = a[off[e]:off[e + 1]] @ w[e] + bias[e]
        torch.testing.assert_close(pre[off[e]:off[e + 1]], u)
        torch.testing.assert_close(out[off[e]:off[e + 1]], torch.relu(u))
    g = torch.randn(B * k, N)
    dw = K.grouped_gemm(a, g, r, "tn")
    assert not dw[2].any()
    for e in range(E):
        torch.testing.assert_close(dw[e], a[off[e]:off[e + 1]].t() @ g[off[e]:off[e + 1]])
    db = torch.empty(E, Kd)
    da = K.grouped_gemm(g, w, r, "nt", dbias=db)
    for e in range(E):
        torch.testing.assert_close(da[off[e]:off[e + 1]], g[off[e]:off[e + 1]] @ w[e].t())
        torch.testing.assert_close(db[e], da[off[e]:off[e + 1]].sum(0))


def test_grouped_gemm_supported_rejects_unaligned():
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)  # noqa: E731
    a, w = bf(16, 64), bf(2, 64, 64)
    assert not K.grouped_gemm_supported(a, w, "nn")                  # CPU tensors: never the kernel
    ok = K.grouped_gemm_layout_ok
    assert ok(a, w, "nn") and ok(a, bf(2, 72, 64), "nt") and ok(a, bf(16, 72), "tn")
    assert ok(bf(16, 24), bf(2, 24, 8), "nn")                        # multiples of 8, not of 64
    assert not ok(a.float(), w, "nn")
    assert not ok(bf(16, 60), bf(2, 60, 64), "nn")                   # lda = 60: rows not 16-byte aligned
    assert not ok(a, bf(2, 64, 12), "nn")                            # ldb = ldc = 12
    assert not ok(a[:, :56], w[:, :56], "nn")                        # strided views
    assert not ok(a, bf(16, 12), "tn")
    assert not ok(bf(17, 64)[1:, 4:60], bf(2, 56, 64), "nn")        # misaligned base, strided
    assert not ok(a, bf(2, 32, 64), "nn")                            # inner dimensions differ
    assert not ok(a, bf(257, 64, 8), "nn")                           # more local experts than the router takes
