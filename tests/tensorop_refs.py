"""fp64 CPU references, derived bounds and input builders shared by the
tensor-operator and embedding suites (test_tensorop_refs.py,
test_tensorops_gpu.py, test_embedding_paths_gpu.py).  A plain helper module,
like conv_refs.py: torch / numpy only, it never imports the extension.

Every reference runs in float64 on the CPU, on the same (already rounded)
inputs the kernel under test gets.

Index rule of gather / scatter-add (tensorops.hip): k < 0 -> k + len; an index
still outside [0, len) reads as 0 in gather and is skipped by scatter-add.
Embedding ids (embedding.hip) do not wrap: an id outside [0, n) contributes
zeros forward and nothing backward, and AVG divides by the bag length L, not
by the number of valid ids.

Top-k order: a strict total order over (value, index) pairs -- NaN first
(torch.topk's rule: NaN is the largest value), then value descending (+0 and
-0 are equal), then index ascending.

Derived bounds
--------------
U8 = 2^-8 is one bf16 ulp relative to the value (8 significand bits).  A kernel
that computes an element-wise result in fp32 and rounds it once to bf16 is
within half of that of the fp32 value (round to nearest); the other half
allows for the fp32 step and a reference that sits at a rounding boundary.
U22 = 2^-22 is the same allowance for an fp32 output (half an fp32 ulp is
2^-24 relative; division and the scalar's own fp32 rounding take the rest).

Measured bounds
---------------
Sums whose order is not fixed (atomics) or is long (serial reductions), and
the fast-intrinsic unary ops, cannot be bounded from the code alone.  Their
bound is 8 x the "fp32 floor": the error, against the fp64 reference, of the
same formula evaluated by torch in fp32 on the CPU on the test's own inputs
and rounded to the output dtype (``fp32_floor_rel`` / ``fp32_floor_abs``).
The tests compute the floor where they use it; profiles/tensorops_tolerances.txt
records floors, bounds and what the kernels measured on an MI355X.
"""
import numpy as np
import torch

U8 = 2.0 ** -8
U22 = 2.0 ** -22
FLOOR_FACTOR = 8.0


# --------------------------------------------------------------- comparisons
def relerr(a, ref):
    """Relative Frobenius error against an fp64 reference (on the CPU)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def maxabs(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (a - ref).abs().max().item()


def assert_ulp(out, ref, dtype, what=""):
    """|out - ref| <= u |ref| at every element, u = 2^-8 (bf16) or 2^-22 (fp32);
    where the reference is infinite the output must be that infinity.  A NaN
    fails."""
    u = U8 if dtype == torch.bfloat16 else U22
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    inf = torch.isinf(ref)
    ok = torch.where(inf, out == ref, (out - ref).abs() <= u * ref.abs())
    if not bool(ok.all()):
        bad = (~ok).reshape(-1).nonzero()[0].item()
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ref.numel()} elements beyond {u:.3g} |ref|; first at flat "
                             f"{bad}: got {out.reshape(-1)[bad].item():.9g}, reference {ref.reshape(-1)[bad].item():.9g}")


def round_to(ref64, dtype):
    """The fp64 reference rounded once to ``dtype`` (what an exact kernel stores)."""
    return ref64.to(torch.float32).to(dtype) if dtype == torch.bfloat16 else ref64.to(dtype)


def fp32_floor_rel(fn, inputs, out_dtype=torch.float32):
    """Relative Frobenius error of fn(fp32 inputs) rounded to out_dtype against fn(fp64 inputs)."""
    ref = fn(*[t.double() for t in inputs])
    lo = fn(*[t.float() for t in inputs]).to(out_dtype)
    return relerr(lo, ref)


def fp32_floor_abs(fn, inputs, out_dtype=torch.float32):
    ref = fn(*[t.double() for t in inputs])
    lo = fn(*[t.float() for t in inputs]).to(out_dtype)
    return maxabs(lo, ref)


# ------------------------------------------------------------ gather / scatter
def wrap_index(idx, length):
    """(wrapped int64 index, valid mask) under the kernels' rule."""
    k = idx.long()
    k = torch.where(k < 0, k + length, k)
    return k, (k >= 0) & (k < length)


def gather_ref(x, idx, dim):
    """y[o, j, i] = x[o, idx[o, j, i], i] in x's dtype (pure data movement); invalid -> 0."""
    k, valid = wrap_index(idx, x.shape[dim])
    y = torch.gather(x, dim, k.clamp(0, x.shape[dim] - 1))
    return torch.where(valid, y, torch.zeros_like(y))


def scatter_add_ref(dy, idx, dim, x_shape):
    """fp64 dx of gather: dx[o, idx[o, j, i], i] += dy[o, j, i]; invalid indices are skipped."""
    k, valid = wrap_index(idx, x_shape[dim])
    dx = torch.zeros(tuple(x_shape), dtype=torch.float64)
    return dx.scatter_add_(dim, k.clamp(0, x_shape[dim] - 1), torch.where(valid, dy.double(), torch.zeros((), dtype=torch.float64)))


def scatter_count_ref(idx, dim, x_shape):
    """int64 number of valid contributions each element of dx receives."""
    k, valid = wrap_index(idx, x_shape[dim])
    return torch.zeros(tuple(x_shape), dtype=torch.int64).scatter_add_(dim, k.clamp(0, x_shape[dim] - 1), valid.long())


# ---------------------------------------------------------------------- top-k
def topk_ref(x, k):
    """(values in x's dtype, int64 indices) of the k first elements of every
    row of x [..., n] in the order NaN first, value descending, index ascending."""
    n = x.shape[-1]
    v = x.detach().double().cpu().numpy()
    isn = np.isnan(v)
    key = np.where(isn, np.inf, v)
    pos = np.broadcast_to(np.arange(n), v.shape)
    # lexsort: the last key is the primary one
    order = np.lexsort((pos, -key, ~isn), axis=-1)[..., :k]
    idx = torch.from_numpy(np.ascontiguousarray(order)).long()
    return torch.gather(x.detach().cpu(), -1, idx), idx


# ------------------------------------------------------------------ embedding
def embedding_ref(idx, W, aggr, acc=torch.float64):
    """Forward in ``acc`` (fp64: the reference; fp32: the floor): idx [..., L] ->
    [..., L, D] (none) or [..., D] (sum / avg over the bag)."""
    n = W.shape[0]
    k = idx.long()
    valid = (k >= 0) & (k < n)
    rows = W.to(acc)[k.clamp(0, n - 1)] * valid.unsqueeze(-1).to(acc)
    if aggr == "none":
        return rows
    out = rows.sum(-2)
    return out / idx.shape[-1] if aggr == "avg" else out


def embedding_grad_ref(idx, dout, n, aggr, acc=torch.float64, fill=0.0):
    """dW [n, D] of embedding_ref for the output gradient ``dout``, accumulated
    in ``acc`` onto a table filled with ``fill``."""
    D = dout.shape[-1]
    k = idx.long().reshape(-1)
    valid = (k >= 0) & (k < n)
    if aggr == "none":
        g = dout.to(acc).reshape(-1, D)
    else:
        L = idx.shape[-1]
        g = dout.to(acc).reshape(-1, 1, D).expand(-1, L, D).reshape(-1, D)
        if aggr == "avg":
            g = g / L
    dW = torch.full((n, D), fill, dtype=acc)
    return dW.index_add_(0, k[valid], g[valid])


def embedding_touched(idx, n):
    """bool [n]: table rows that at least one valid id names."""
    k = idx.long().reshape(-1)
    k = k[(k >= 0) & (k < n)]
    t = torch.zeros(n, dtype=torch.bool)
    t[k] = True
    return t


# ------------------------------------------------------------- input builders
TIE_VALUES = (-3.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0)   # exact in bf16: ties survive both dtypes


def tie_heavy_rows(rows, n, seed):
    """fp32 [rows, n] drawn from TIE_VALUES (8 distinct bf16-exact numbers)."""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(TIE_VALUES)[torch.randint(0, len(TIE_VALUES), (rows, n), generator=g)]


def tied_pick_share(x, k):
    """Share of the top-k picks of x [rows, n] whose value occurs more than once in their row."""
    v, _ = topk_ref(x, k)
    xd = x.double()
    same = (xd.unsqueeze(-2) == v.double().unsqueeze(-1)).sum(-1)   # [rows, k] occurrences in the row
    return (same > 1).double().mean().item()


def edge_indices(shape, length, seed, negative=0.15, out_of_range=0.15, duplicated=0.2, dtype=torch.int64):
    """Indices into an axis of ``length``: a ``negative`` share in [-length, -1]
    (valid, they wrap), an ``out_of_range`` share split between >= length and
    < -length, a ``duplicated`` share all equal to one hot index, and the rest
    uniform in [0, length)."""
    g = torch.Generator().manual_seed(seed)
    numel = int(np.prod(shape))
    idx = torch.randint(0, length, (numel,), generator=g)
    perm = torch.randperm(numel, generator=g)
    n_neg, n_oor, n_dup = (int(round(s * numel)) for s in (negative, out_of_range, duplicated))
    neg, oor, dup = perm[:n_neg], perm[n_neg:n_neg + n_oor], perm[n_neg + n_oor:n_neg + n_oor + n_dup]
    idx[neg] = -1 - torch.randint(0, length, (n_neg,), generator=g)
    hi = length + torch.randint(0, 3 * length + 7, (n_oor,), generator=g)
    lo = -length - 1 - torch.randint(0, 3 * length + 7, (n_oor,), generator=g)
    idx[oor] = torch.where(torch.arange(n_oor) % 2 == 0, hi, lo)
    idx[dup] = length // 3
    return idx.reshape(shape).to(dtype)


def index_shares(idx, length):
    """(negative-and-valid share, out-of-range share) of an index tensor."""
    k = idx.long()
    neg = ((k < 0) & (k >= -length)).double().mean().item()
    oor = ((k >= length) | (k < -length)).double().mean().item()
    return neg, oor


def hot_indices(hot, spread, length, seed, dtype=torch.int64):
    """1-d indices: ``hot`` entries on one address (given as k and as k - length
    alternately) shuffled among ``spread`` uniform ones."""
    g = torch.Generator().manual_seed(seed)
    k = length // 2
    h = torch.where(torch.arange(hot) % 2 == 0, torch.tensor(k), torch.tensor(k - length))
    idx = torch.cat([h, torch.randint(0, length, (spread,), generator=g)])
    return idx[torch.randperm(hot + spread, generator=g)].to(dtype)


def embedding_ids(shape, n, seed, out_of_range=0.15, dtype=torch.int64):
    """Ids in [0, n) with an ``out_of_range`` share split between -1 and values >= n."""
    g = torch.Generator().manual_seed(seed)
    numel = int(np.prod(shape))
    idx = torch.randint(0, n, (numel,), generator=g)
    n_oor = int(round(out_of_range * numel))
    where = torch.randperm(numel, generator=g)[:n_oor]
    hi = n + torch.randint(0, 5, (n_oor,), generator=g)
    idx[where] = torch.where(torch.arange(n_oor) % 2 == 0, torch.full((n_oor,), -1), hi)
    return idx.reshape(shape).to(dtype)
