"""rmsnorm.hip on the GPU: every launch path of the RMSNorm forward / backward
and of the RoPE kernel against fp64 references of the same operation on the
same rounded inputs, and the LLaMA-style model built on them.

Every reference takes a compute dtype ``ct``.  The tests call it with fp64;
tools/rmsnorm_rope_floors.py calls the same function with fp32 on the CPU, on
the same inputs, to measure the floor each fp32 bound is set from (8x the
floor, rounded up to one digit: profiles/rmsnorm_rope_tolerances.txt).  Inputs
are built on the CPU from seeded generators so that both see the same values.

Path -> shapes that reach it
----------------------------
rms_fwd_kernel / rms_bwd_kernel<L = N / 8, C = 1>   (1, 64) (37, 64) (37, 128) (130, 256): M a multiple of
    (N in {64, 128, 256}: 64 / L rows per wave)      neither the rows of a wave nor those of a block
rms_fwd_kernel / rms_bwd_kernel<L = 64, C = N / 512> (3, 512) one block; (1030, 1536) C = 3; (5, 4096) C = 8,
                                                     one row in flight; (4133, 512) second trip of the row
                                                     loop with the grid at its cap of 512
rms_fwd_generic / rms_bwd_generic / rms_dgamma_generic  (1, 8) (37, 520) (3, 4104)
rms_ws_reduce_kernel                                 every case that asks for dgamma
rope_kernel<T, half-split | interleaved>             ROPE_SHAPES, forward and inverse
"""
import math

import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

# bf16 outputs against fp64 on the same inputs (test_rowwise_paths_gpu.py's _BF / _BF_OP): _BF where
# only the output rounding remains, _BF_OP where bf16 intermediates take part
_BF, _BF_OP = 3e-3, 5e-3

# fp32 bounds: 8x the floor of the same formula in torch fp32 on the CPU, rounded up to one digit
_RMS_Y_F32 = 9e-7      # profiles/rmsnorm_rope_tolerances.txt: rms_y_f32
_RMS_DX_F32 = 1e-6     # profiles/rmsnorm_rope_tolerances.txt: rms_dx_f32
_RMS_RSTD = 8e-7       # profiles/rmsnorm_rope_tolerances.txt: rms_rstd
_RMS_DGAMMA = 2e-6     # profiles/rmsnorm_rope_tolerances.txt: rms_dgamma
_ROPE_F32 = 3e-7       # profiles/rmsnorm_rope_tolerances.txt: rope_f32
# one fp32 rounding of a value in [-1, 1] is at most 6e-8
_TABLE_ABS = 1e-7


def _rel64(a, b):
    """Relative Frobenius error in fp64; 0 when both are exactly zero."""
    a, b = a.double(), b.double()
    d = (a - b).norm().item()
    return 0.0 if d == 0.0 else d / max(b.norm().item(), 1e-300)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _obs(key, tag, value, bound):
    """Print the observed figure under its bound's name in the tolerance file
    (tools/rmsnorm_rope_floors.py --observed collects the maxima), return it."""
    print(f"OBS {key} {tag} {value:.3e} {bound:.1e}")
    return value


def _ran(name, n0, by=1):
    assert K.STATS[name] == n0 + by, f"native {name} did not run"


# -------------------------------------------------------------------- RMSNorm
RMS_SHAPES = [(1, 64), (37, 64), (37, 128), (130, 256),            # N / 8 lanes per row
              (3, 512), (1030, 1536), (5, 4096), (4133, 512),      # one wave per row, the row in registers
              (1, 8), (37, 520), (3, 4104)]                        # block per row
RMS_COMBOS = {  # id: (residual, save_sum, gamma, dres, dgamma)
    "all": (True, True, True, True, True),
    "plain": (False, True, True, False, False),
    "nogamma": (True, False, False, False, True),
    "dres": (False, True, True, True, False),
}
_RMS_EPS = float(torch.tensor(1e-6, dtype=torch.float32))


def rms_inputs(M, N, dtype, seed=31):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    x, r, dy, dres = mk(M, N) + 0.3, mk(M, N), mk(M, N), mk(M, N)
    gamma = 1 + 0.1 * mk(N)
    start = 0.5 * mk(N)     # dgamma accumulates into this
    return tuple(t.to(dtype) for t in (x, r, dy, dres, gamma)) + (start,)


def rms_stats(x, r, ct=torch.float64):
    """(sum, rstd) of the rows of x [+ r] in ``ct``: the forward kernels take the statistics from the unrounded sum."""
    t = x.to(ct) if r is None else x.to(ct) + r.to(ct)
    return t, (t.pow(2).mean(1, keepdim=True) + _RMS_EPS).rsqrt()


def rms_fwd_ref(x, r, gamma, ct=torch.float64):
    t, rstd = rms_stats(x, r, ct)
    y = t * rstd
    return y if gamma is None else y * gamma.to(ct)


def rms_bwd_ref(dy, s, x, r, gamma, dres, ct=torch.float64):
    """(dx, colsum(dy * xhat)).  As in the kernels, xhat is the stored (rounded) sum s times the rstd of the
    unrounded x [+ r], which the forward hands to the backward."""
    _, rstd = rms_stats(x, r, ct)
    dy = dy.to(ct)
    xh = s.to(ct) * rstd
    g = dy if gamma is None else dy * gamma.to(ct)
    dx = rstd * (g - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(ct)
    return dx, (dy * xh).sum(0)


@pytest.mark.parametrize("combo", list(RMS_COMBOS))
@pytest.mark.parametrize("M,N", RMS_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_rmsnorm_paths(dtype, M, N, combo):
    use_res, save_sum, use_gamma, use_dres, want_dg = RMS_COMBOS[combo]
    x, r, dy, dres, gamma, start = (t.to(DEV) for t in rms_inputs(M, N, dtype))
    r = r if use_res else None
    gamma = gamma if use_gamma else None
    dres = dres if use_dres else None
    bf = dtype == BF16
    dt = "bf16" if bf else "f32"
    tag = f"{dt}-{M}x{N}-{combo}"
    n0, n1 = K.STATS["rmsnorm_fwd"], K.STATS["rmsnorm_bwd"]
    y, s, rstd = K.rmsnorm_fwd(x, gamma, _RMS_EPS, residual=r, save_sum=save_sum)
    _ran("rmsnorm_fwd", n0)
    ky, by = ("bf16_out", _BF) if bf else ("rms_y_f32", _RMS_Y_F32)
    assert _obs(ky, "rms_y-" + tag, _rel64(y, rms_fwd_ref(x, r, gamma)), by) < by
    assert rstd.dtype == F32 and rstd.shape == (M,)
    assert _obs("rms_rstd", tag, _rel64(rstd, rms_stats(x, r)[1].reshape(-1)), _RMS_RSTD) < _RMS_RSTD
    # the stored sum is the fp32 sum rounded once
    s_own = x if r is None else (x.float() + r.float()).to(dtype)
    if use_res and save_sum:
        assert torch.equal(_bits(s), _bits(s_own))
    elif use_res:
        assert s is None
        s = s_own
    else:
        assert s is x
    dg = start.clone() if want_dg else None
    dx = K.rmsnorm_bwd(dy, s, rstd, gamma, dg, dres=dres)
    _ran("rmsnorm_bwd", n1)
    # the reference takes the kernel's own statistics path: rstd of the unrounded sum
    dx_ref, dg_ref = rms_bwd_ref(dy, s, x, r, gamma, dres)
    kx, bx = ("bf16_op", _BF_OP) if bf else ("rms_dx_f32", _RMS_DX_F32)
    assert _obs(kx, "rms_dx-" + tag, _rel64(dx, dx_ref), bx) < bx
    if want_dg:   # an fp32 output for both input types; it accumulates into its start
        assert _obs("rms_dgamma." + dt, tag, _rel64(dg, start.double() + dg_ref), _RMS_DGAMMA) < _RMS_DGAMMA
        again = start.clone()
        dx2 = K.rmsnorm_bwd(dy, s, rstd, gamma, again, dres=dres)
        assert torch.equal(_bits(dg), _bits(again)), "dgamma is added in a fixed order"
        assert torch.equal(_bits(dx), _bits(dx2))


def test_rmsnorm_wrapper_checks():
    x = torch.randn(4, 64, device=DEV, dtype=BF16)
    with pytest.raises(ValueError, match="multiple of 8"):
        K.rmsnorm_fwd(torch.randn(4, 12, device=DEV, dtype=BF16), None, 1e-6)
    with pytest.raises(ValueError, match="contiguous"):
        K.rmsnorm_fwd(torch.randn(64, 4, device=DEV, dtype=BF16).t(), None, 1e-6)
    with pytest.raises(ValueError, match="bf16 or fp32"):
        K.rmsnorm_fwd(x.half(), None, 1e-6)
    with pytest.raises(ValueError, match="gamma"):
        K.rmsnorm_fwd(x, torch.ones(64, device=DEV), 1e-6)
    with pytest.raises(ValueError, match="16-byte aligned"):
        K.rmsnorm_fwd(torch.randn(4 * 64 + 1, device=DEV, dtype=BF16)[1:].view(4, 64), None, 1e-6)
    with pytest.raises(ValueError, match="expected a GPU tensor"):
        K.rmsnorm_fwd(x.cpu(), None, 1e-6)
    y, s, rstd = K.rmsnorm_fwd(x, None, 1e-6)
    with pytest.raises(ValueError, match="dgamma"):
        K.rmsnorm_bwd(x, s, rstd, None, torch.zeros(64, device=DEV, dtype=BF16))
    with pytest.raises(ValueError, match="rstd"):
        K.rmsnorm_bwd(x, s, rstd[:3], None)


# ----------------------------------------------------------------------- RoPE
ROPE_SHAPES = [((2, 3, 130, 64), -2), ((2, 130, 3, 128), 1), ((1, 1, 1, 16), -2), ((3, 7, 80), -2)]
_THETA = 10000.0


def rope_inputs(shape, dtype, seed=32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def rope_ref(x, table, seq_dim, interleaved, inverse, ct=torch.float64):
    """The rotation by the table's own (cos, sin), in ``ct``: isolates the kernel from the table."""
    sd = seq_dim % x.dim()
    D = x.shape[-1]
    shape = [1] * x.dim()
    shape[sd], shape[-1] = x.shape[sd], D // 2
    c, s = table[..., 0].to(ct).reshape(shape), table[..., 1].to(ct).reshape(shape)
    if inverse:
        s = -s
    xf = x.to(ct)
    if interleaved:
        a, b = xf[..., 0::2], xf[..., 1::2]
        return torch.stack([a * c - b * s, b * c + a * s], -1).flatten(-2)
    a, b = xf[..., :D // 2], xf[..., D // 2:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
@pytest.mark.parametrize("shape,seq_dim", ROPE_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_rope_paths(dtype, shape, seq_dim, interleaved, inverse):
    x = rope_inputs(shape, dtype).to(DEV)
    keep = x.clone()
    S, D = shape[seq_dim], shape[-1]
    tag = f"{'bf16' if dtype == BF16 else 'f32'}-{'x'.join(map(str, shape))}-{int(interleaved)}{int(inverse)}"
    n0 = K.STATS["rope"]
    y = K.rope(x, _THETA, seq_dim, interleaved, inverse)
    _ran("rope", n0)
    assert torch.equal(x, keep) and y.shape == x.shape and y.dtype == dtype
    table = K.rope_table(S, D, _THETA, x.device)
    assert table.shape == (S, D // 2, 2) and table.dtype == F32
    kb, bb = ("bf16_out", _BF) if dtype == BF16 else ("rope_f32", _ROPE_F32)
    assert _obs(kb, "rope-" + tag, _rel64(y, rope_ref(x, table, seq_dim, interleaved, inverse)), bb) < bb
    # position 0: cos = 1, sin = 0, the row comes back bit for bit
    sd = seq_dim % x.dim()
    assert torch.equal(_bits(y.select(sd, 0)), _bits(x.select(sd, 0)))
    # in place (out = x): every thread reads both members of its pairs before it writes either
    z = x.clone()
    assert K.rope(z, _THETA, seq_dim, interleaved, inverse, out=z) is z
    assert torch.equal(_bits(z), _bits(y))
    # there and back.  In units of the pair's norm |p|: each pass rounds two products and a sum to fp32
    # (3 * 2^-24) and the rounded table has c^2 + s^2 within 2^-23 of 1, together 2^-21.  A bf16 output
    # is rounded once per pass, by at most 2^-8 of the value (half an ulp of 8 significant bits): the
    # first pass's error vector has norm <= 2^-8 |p| and keeps it under the inverse rotation, the
    # second rounding adds <= 2^-8 |x_i| <= 2^-8 |p|.  One output rounding each way and no more: 2^-7
    back = K.rope(y, _THETA, seq_dim, interleaved, not inverse)
    lim = 2.0 ** -21 + (2.0 ** -7 if dtype == BF16 else 0.0)
    xd, D2 = x.double(), D // 2
    if interleaved:
        nrm = (xd[..., 0::2] ** 2 + xd[..., 1::2] ** 2).sqrt().repeat_interleave(2, -1)
    else:
        nrm = (xd[..., :D2] ** 2 + xd[..., D2:] ** 2).sqrt().repeat(*([1] * (x.dim() - 1)), 2)
    worst = float(((back.double() - xd).abs() / nrm.clamp_min(1e-30)).max())
    assert _obs("rope_roundtrip_" + ("bf16" if dtype == BF16 else "f32"), tag, worst, lim) <= lim


@pytest.mark.parametrize("S,D,theta", [(130, 64, 10000.0), (130, 128, 10000.0), (7, 80, 500000.0)])
def test_rope_table_against_fp64(S, D, theta):
    table = K.rope_table(S, D, theta, torch.device(DEV)).cpu().double()
    inv = torch.tensor(theta, dtype=torch.float64) ** (-torch.arange(0, D // 2, dtype=torch.float64) * 2.0 / D)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None, :]
    err = max(float((table[..., 0] - torch.cos(ang)).abs().max()), float((table[..., 1] - torch.sin(ang)).abs().max()))
    assert _obs("rope_table_abs", f"{S}x{D}", err, _TABLE_ABS) < _TABLE_ABS
    assert K.rope_table(S, D, theta, torch.device(DEV)) is K.rope_table(S, D, theta, torch.device(DEV)), "cached"


def test_rope_wrapper_checks_and_operator_fallback():
    from flexflow_train_amd.ops import base as opbase

    x = torch.randn(2, 5, 24, device=DEV, dtype=BF16)
    with pytest.raises(ValueError, match="multiple of 16"):
        K.rope(x)
    with pytest.raises(ValueError, match="seq_dim"):
        K.rope(torch.randn(2, 5, 32, device=DEV, dtype=BF16), seq_dim=-1)
    with pytest.raises(ValueError, match="contiguous"):
        K.rope(torch.randn(2, 32, 5, device=DEV, dtype=BF16).transpose(1, 2))
    with pytest.raises(ValueError, match="bf16 or fp32"):
        K.rope(torch.randn(2, 5, 32, device=DEV, dtype=torch.float16))
    # D = 24: the operator takes the torch fallback of the same definition
    impl = opbase.get_impl("ROPE")
    ctx = opbase.OpContext(op_type="ROPE", attrs={}, name="rope", training=True)
    n0 = K.STATS["rope"]
    (y,), saved = impl.forward(ctx, [x], [])
    (dx,) = impl.backward(ctx, saved, [y], [], [True])
    assert K.STATS["rope"] == n0 and saved is None
    table = K.rope_table(5, 24, _THETA, x.device)
    assert _rel64(y, rope_ref(x, table, -2, False, False)) < _BF
    assert _rel64(dx, x) < _BF_OP, "the backward is the inverse rotation"
    # D = 32: the HIP kernel both ways
    x = torch.randn(2, 5, 32, device=DEV, dtype=BF16)
    (y,), saved = impl.forward(ctx, [x], [])
    (dx,) = impl.backward(ctx, saved, [y], [], [True])
    assert K.STATS["rope"] == n0 + 2 and _rel64(dx, x) < _BF_OP


# ---------------------------------------------------------------------- model
def _llama(fuse=True):
    from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType
    from flexflow_train_amd.models.llama import LlamaConfig, build_llama

    cfg = FFConfig()
    cfg.perform_fusion = fuse
    m = FFModel(cfg)
    build_llama(m, LlamaConfig(vocab_size=256, hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
                               intermediate_size=512, sequence_length=64, batch_size=2))
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    assert ex.cfg.compute_dtype == torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.1
                         + (1.0 if n.endswith("gamma") else 0.0))
    return ex


def _gqa_two_layer_model():
    """tests/test_attention_gqa_gpu.py's graphed two-layer model (Hkv = 2 of H = 4), none of the new
    operators: what graphed and eager steps differ by there sets the bound here."""
    from flexflow_train_amd.core import AdamOptimizer, DataType, FFConfig, FFModel, LossType

    m = FFModel(FFConfig())
    x = m.create_tensor([4, 64, 128], DataType.DT_FLOAT, name="input")
    h = x
    for i in range(2):
        q, k, v = (m.transpose(m.reshape(m.dense(h, nh * 64, name=f"{n}{i}"), [4, 64, nh, 64]), [0, 2, 1, 3])
                   for n, nh in (("q", 4), ("k", 2), ("v", 2)))
        a = m.scaled_dot_product_attention(q, k, v, causal=True, name=f"attn{i}")
        h = m.add(h, m.dense(m.reshape(m.transpose(a, [0, 2, 1, 3]), [4, 64, 256]), 128, name=f"o{i}"))
    m.softmax(m.dense(h, 8, name="head"), name="softmax")
    m.compile(optimizer=AdamOptimizer(m, alpha=1e-2), loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = m.executor
    g = torch.Generator().manual_seed(0)
    for n in sorted(ex.parameter_names()):
        ex.set_parameter(n, torch.randn(ex.get_parameter(n).shape, generator=g) * 0.1)
    return ex


def test_llama_graphed_step_matches_eager():
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 256, (2, 65), generator=g, dtype=torch.int32)
    feeds, labels = {"input_ids": ids[:, :64].contiguous().to(DEV)}, ids[:, 1:].long().contiguous().to(DEV)
    bx = torch.randn(4, 64, 128, generator=g).to(DEV)
    by = torch.randint(0, 8, (4, 64), generator=g).to(DEV)

    def params(ex):
        torch.cuda.synchronize()
        return {n: ex.get_parameter(n).double().cpu() for n in sorted(ex.parameter_names())}

    def eager(make, f, y):
        ex = make()
        for _ in range(3):
            ex.train_step(f, y)
        return ex, params(ex)

    def graphed(make, f, y):
        ex = make()
        step = ex.make_graphed_train_step(f, y, warmup=1)   # one eager step, then two replays
        step(f, y)
        step(f, y)
        return params(ex)

    def worst(p, q):
        return max(float((p[n] - q[n]).norm() / q[n].norm()) for n in p)

    d0 = worst(graphed(_gqa_two_layer_model, {"input": bx}, by), eager(_gqa_two_layer_model, {"input": bx}, by)[1])
    bound = max(2 * d0, 1e-5)
    n0 = {k: K.STATS[k] for k in ("rmsnorm_fwd", "rmsnorm_bwd", "rope", "attention_gqa")}
    ex, want = eager(_llama, feeds, labels)
    fused = [s for s in ex.steps if s.op_type == "FUSED_ADD_RMS_NORM"]
    assert len(fused) == 4 and sum(1 for s in fused if s.ctx.extra.get("emit_sum")) == 3
    # three steps: 5 norms, 4 rotations each way, 2 attention layers
    assert K.STATS["rmsnorm_fwd"] == n0["rmsnorm_fwd"] + 15 and K.STATS["rmsnorm_bwd"] == n0["rmsnorm_bwd"] + 15
    assert K.STATS["rope"] == n0["rope"] + 24
    assert K.STATS["attention_gqa"] == n0["attention_gqa"] + 12
    d1 = worst(graphed(_llama, feeds, labels), want)
    print(f"llama graphed vs eager: {d1:.3e}; the GQA two-layer model {d0:.3e} (bound {bound:.3e})")
    assert d1 <= bound, (d1, bound)
    moved = max(float((want[n] - 1.0).abs().max()) for n in want if n.endswith("gamma"))
    assert moved > 1e-3, "gamma trained"
