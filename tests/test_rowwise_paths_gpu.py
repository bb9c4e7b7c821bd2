"""Launch branches of the row-wise, element-wise and optimizer kernels that
test_kernels_gpu.py does not enter, against fp64 references of the same
operation on the same rounded inputs.

Every reference below takes a compute dtype ``ct``.  The tests call it with
fp64; tools/rowwise_floors.py calls the same function with fp32 on the CPU,
on the same inputs, to measure the floor each fp32 bound is set from (8x the
floor, rounded up to one digit: profiles/r9/rowwise_tolerances.txt).  Inputs
are built on the CPU from seeded generators so that both see the same values.

Branch -> test case that reaches it
-----------------------------------
softmax.hip
  softmax_ce_kernel<bf16, int32|int64, VEC>    test_softmax_ce_paths[a-*]
  softmax_ce_kernel<bf16, int32|int64, scalar> test_softmax_ce_paths[b-*]
  softmax_ce_kernel<float, int32|int64, VEC>   test_softmax_ce_paths[c-*]
  softmax_ce_kernel<float, int32|int64, scalar> test_softmax_ce_paths[d-*]
  softmax_ce_reg_kernel, one chunk / row narrower than a block (threads that
    keep tm == -inf)                           test_softmax_ce_paths[e1-*, e2-*]
  write_grad=False, ignore_index != -100, label >= valid_cols, tied maxima
                                               every test_softmax_ce_paths case
  softmax_fwd / softmax_bwd <bf16>, N < 256, N = 1, N % 256 != 0
                                               test_softmax_fwd_bwd_paths
optimizer.hip
  adam8_kernel<float|bf16>                     test_adam_paths[n8-*]
  adam_kernel<float|bf16> (n % 8 == 4)         test_adam_paths[n8p4-*]
  adam_kernel<bf16> (g 8-byte aligned only)    test_adam_paths[goff8-*]
  decoupled=False, grad_scale != 1, hp={lr, step}  test_adam_paths[*-coupled-*, *-gs128-*, *-hp]
  sgd_kernel<float|bf16>, mom=None, plain / Nesterov momentum, bf16 copy
                                               test_sgd_paths
  gradients the wrappers refuse (fp32 off 16 bytes, bf16 off 8, other types,
    wrong length)                              test_optimizer_gradient_contract
  sumsq_kernel (one thread, one block, many blocks)  test_sum_squares
layernorm.hip
  ln_fwd_kernel / ln_bwd_kernel: one block (M=3), second trip of the row loop +
    grid cap 512 + 8 reduce chunks (M=4133), C=3 with 3 reduce chunks (1030x1536)
                                               test_layernorm_paths[tiled shapes]
  ln_fwd_generic / ln_bwd_generic (dres, dsum, dgamma, dbeta)
                                               test_layernorm_paths[generic shapes]
  no residual, save_sum=False, gamma=beta=None, dres, dsum alone (workspace
    slice 2 only), dgamma alone, dbeta alone, all three
                                               test_layernorm_paths[*-all|dsum|nogamma|dbeta]
elementwise.hip
  bias_act_fwd_kernel / act_bwd_kernel / colsum_act_kernel <bf16|float, every
    activation code>, alpha, partial last 512-column block (N=520, 1032),
    fewer rows than a 32-row batch (M=1), no bias, save_pre=False, pre=None,
    write_dx=False, dbias=None                 test_activation_paths
  cast_kernel<float, bf16>, <bf16, float>      test_cast_bitwise
  dropout_kernel<float>                        test_dropout_fp32
  axpby_kernel: the package has no Python wrapper for it, so it has no test.
"""
import math

import numpy as np
import pytest
import torch

from flexflow_train_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

# bf16 outputs against fp64 on the same inputs (test_kernels_gpu.py): _BF where
# only the output rounding remains, _BF_OP where bf16 intermediates take part
_BF, _BF_OP = 3e-3, 5e-3

# fp32 bounds: 8x the floor of the same formula in torch fp32 on the CPU,
# rounded up to one digit.  Every constant: profiles/r9/rowwise_tolerances.txt
_CE_LOSS = 4e-6        # profiles/r9/rowwise_tolerances.txt: ce_loss
_CE_LOSS_BIG = 3e-5    # profiles/r9/rowwise_tolerances.txt: ce_loss_big
_CE_GRAD = 3e-6        # profiles/r9/rowwise_tolerances.txt: ce_grad
_CE_GRAD_BIG = 8e-4    # profiles/r9/rowwise_tolerances.txt: ce_grad_big
_SM_FWD = 7e-7         # profiles/r9/rowwise_tolerances.txt: softmax_fwd
_SM_BWD = 2e-6         # profiles/r9/rowwise_tolerances.txt: softmax_bwd
_ADAM_UPD = 4e-4       # profiles/r9/rowwise_tolerances.txt: adam_update
_ADAM_MV = 7e-7        # profiles/r9/rowwise_tolerances.txt: adam_m_v
_SGD_UPD = 3e-4        # profiles/r9/rowwise_tolerances.txt: sgd_update
_SGD_MOM = 4e-7        # profiles/r9/rowwise_tolerances.txt: sgd_mom
_SUMSQ = 6e-7          # profiles/r9/rowwise_tolerances.txt: sum_squares
_LN_Y_F32 = 7e-7       # profiles/r9/rowwise_tolerances.txt: ln_y_f32
_LN_DX_F32 = 9e-7      # profiles/r9/rowwise_tolerances.txt: ln_dx_f32
_LN_COLSUM = 2e-6      # profiles/r9/rowwise_tolerances.txt: ln_colsum (dgamma, dbeta, dsum)
_TANH0_ABS = 9e-7      # profiles/r9/rowwise_tolerances.txt: tanh0_abs (absolute)
# profiles/r9/rowwise_tolerances.txt: act_fwd_*, act_bwd_*, act_dbias_*
_ACT_FWD = {"none": 3e-7, "relu": 3e-7, "sigmoid": 4e-7, "tanh": 6e-7, "gelu": 5e-7, "elu": 3e-7, "exp": 2e-6}
_ACT_BWD = {"none": 0.0, "relu": 0.0, "sigmoid": 9e-7, "tanh": 2e-6, "gelu": 4e-6, "elu": 2e-7, "exp": 4e-7}
_ACT_DBIAS = {"none": 9e-7, "relu": 9e-7, "sigmoid": 2e-6, "tanh": 2e-6, "gelu": 3e-6, "elu": 9e-7, "exp": 1e-6}


def _f32(v):
    """The fp32 value a kernel argument becomes, as a Python float."""
    return float(np.float32(v))


def _rel64(a, b):
    """Relative Frobenius error in fp64; 0 when both are exactly zero."""
    a, b = a.double(), b.double()
    d = (a - b).norm().item()
    return 0.0 if d == 0.0 else d / max(b.norm().item(), 1e-300)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _obs(key, tag, value, bound):
    """Print the observed figure under its bound's name in the tolerance file
    (tools/rowwise_floors.py --observed collects the maxima), return it."""
    print(f"OBS {key} {tag} {value:.3e} {bound:.1e}")
    return value


def _ran(name, n0, by=1):
    assert K.STATS[name] == n0 + by, f"native {name} did not run"


# --------------------------------------------------------------- softmax + CE
_IGN = 7   # ignore_index of every case; also a legal column of the other rows
CE_CASES = {  # id: (dtype, M, V, valid_cols)
    "a": (BF16, 4, 65544, 65539),   # streaming, vector
    "b": (BF16, 5, 1003, 1003),     # streaming, scalar
    "c": (F32, 7, 2056, 2051),      # streaming, vector
    "d": (F32, 7, 1001, 1001),      # streaming, scalar
    "e1": (BF16, 3, 8, 5),          # register kernel, one thread has a chunk
    "e2": (BF16, 3, 136, 131),      # register kernel, 17 of 256 threads have one
}
_CE_ROLES = ["ign", "oor", "big_tie2", "tie1", "big"]


def ce_inputs(dtype, M, V, Vv, seed=20):
    """Launches of M rows: (logits [M, V], labels [M] int64, big [M] bool), CPU.
    Rows: ignored through ignore_index; label == valid_cols (out of range);
    +-big logits with the maximum at two columns and the label on the second;
    the maximum at two columns and the label on the first; +-big logits with a
    random label; rows whose label is their argmax.  Padding columns hold
    2 * big, so a kernel that reads them shows."""
    g = torch.Generator().manual_seed(seed)
    big = 80.0 if dtype == BF16 else 1e4
    roles = list(_CE_ROLES)
    while len(roles) % M:
        roles.append("plain")
    R = len(roles)
    c1, c2 = 1, Vv - 2
    x = (torch.randn(R, V, generator=g) * 3).to(dtype).float()
    labels = torch.randint(0, Vv, (R,), generator=g)
    labels[labels == _IGN] = 0
    for r, role in enumerate(roles):
        if role.startswith("big"):
            x[r] = (x[r] * (big / 9)).clamp(-0.98 * big, 0.98 * big)
            x[r, 0] = -big
            x[r, c2] = big
        if role == "big_tie2":
            x[r, c1] = big
            labels[r] = c2
        elif role == "tie1":
            x[r, c1] = x[r, c2] = x[r, :Vv].max() + 1
            labels[r] = c1
        elif role == "ign":
            labels[r] = _IGN
        elif role == "oor":
            labels[r] = Vv
    x[:, Vv:] = 2 * big
    x = x.to(dtype)
    for r, role in enumerate(roles):
        if role == "plain":
            labels[r] = x[r, :Vv].float().argmax()
    isbig = torch.tensor([role.startswith("big") for role in roles])
    return [(x[i:i + M].clone(), labels[i:i + M].clone(), isbig[i:i + M].clone(), roles[i:i + M])
            for i in range(0, R, M)]


def ce_ref(logits, labels, Vv, scale, ct=torch.float64):
    """(row loss, gradient over the valid columns, correct, counted) by the
    kernel's formula: lse = max + log(sum exp(x - max)), p = exp(x - lse)."""
    x = logits[:, :Vv].to(ct)
    lab = labels.long()
    valid = (lab != _IGN) & (lab >= 0) & (lab < Vv)
    m = x.max(1, keepdim=True).values
    lse = m + (x - m).exp().sum(1, keepdim=True).log()
    li = lab.clamp(0, Vv - 1)[:, None]
    loss = torch.where(valid, (lse - x.gather(1, li))[:, 0], torch.zeros((), dtype=ct, device=x.device))
    onehot = torch.zeros_like(x).scatter_(1, li, 1.0)
    grad = ((x - lse).exp() - onehot) * scale * valid[:, None].to(ct)
    cols = torch.arange(Vv, device=x.device)
    first = torch.where(x == m, cols, Vv).min(1).values   # first index of the maximum: ties are defined
    correct = int((valid & (first == lab)).sum())
    return loss, grad, correct, int(valid.sum())


@pytest.mark.parametrize("ldt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", list(CE_CASES))
def test_softmax_ce_paths(case, ldt):
    dtype, M, V, Vv = CE_CASES[case]
    scale = _f32(1.0 / 16)
    for logits_c, labels_c, isbig_c, roles in ce_inputs(dtype, M, V, Vv):
        logits, labels, isbig = logits_c.to(DEV), labels_c.to(DEV), isbig_c.to(DEV)
        loss_ref, grad_ref, correct, counted = ce_ref(logits, labels, Vv, scale)
        g = logits.clone()
        metrics = torch.zeros(4, device=DEV)
        row_loss = torch.full((M,), -1.0, device=DEV)
        n0 = K.STATS["softmax_ce"]
        K.softmax_ce(g, labels.to(ldt), scale, metrics=metrics, valid_cols=Vv, ignore_index=_IGN,
                     row_loss=row_loss)
        _ran("softmax_ce", n0)
        # loss: per row and summed (fp32 outputs for both logit types)
        for name, sel, bound in (("ce_loss", ~isbig, _CE_LOSS), ("ce_loss_big", isbig, _CE_LOSS_BIG)):
            if sel.any():
                assert _obs(name, case, _rel64(row_loss[sel], loss_ref[sel]), bound) < bound
        sum_key, sum_bound = ("ce_loss_big", _CE_LOSS_BIG) if isbig.any() else ("ce_loss", _CE_LOSS)
        ref_sum = loss_ref.sum().item()
        assert _obs(sum_key, f"sum-{case}", abs(metrics[0].item() - ref_sum) / abs(ref_sum), sum_bound) < sum_bound
        assert metrics[2].item() == counted
        assert metrics[1].item() == correct
        assert metrics[3].item() == 0
        # rows that do not count: zero loss, zero gradient, bit for bit
        for r, role in enumerate(roles):
            if role in ("ign", "oor"):
                assert row_loss[r].item() == 0
                assert int(_bits(g[r]).ne(0).sum()) == 0, (role, "gradient row is not all +0")
        if V > Vv:
            assert int(_bits(g[:, Vv:]).ne(0).sum()) == 0, "padding columns are not all +0"
        # the gradient
        counts = (labels != _IGN) & (labels < Vv)
        for sel, kf, bf32 in ((~isbig, "ce_grad", _CE_GRAD), (isbig, "ce_grad_big", _CE_GRAD_BIG)):
            name, bound = ("bf16_out", _BF) if dtype == BF16 else (kf, bf32)
            if sel.any():
                assert _obs(name, f"ce-{case}", _rel64(g[sel][:, :Vv], grad_ref[sel]), bound) < bound
            rows = torch.nonzero(counts & sel)[:, 0]
            if rows.numel():   # the label column on its own: negative, and the reference's value
                lab_g, lab_ref = g[rows, labels[rows]].double(), grad_ref[rows, labels[rows]]
                assert (lab_g < 0).all()
                # one or two values, so per element: the fp32 bound, plus for bf16 the
                # worst rounding of one value (half an ulp of 8 significant bits)
                name, bound = ("bf16_elem", 2.0 ** -8 + bf32) if dtype == BF16 else (kf, bf32)
                err = ((lab_g - lab_ref).abs() / lab_ref.abs()).max().item()
                assert _obs(name, f"ce-label-{case}", err, bound) < bound
        # write_grad=False: the logits stay, loss and metrics are the same
        keep = logits.clone()
        metrics2 = torch.zeros(4, device=DEV)
        row_loss2 = torch.full((M,), -1.0, device=DEV)
        K.softmax_ce(keep, labels.to(ldt), scale, metrics=metrics2, valid_cols=Vv, ignore_index=_IGN,
                     write_grad=False, row_loss=row_loss2)
        assert torch.equal(_bits(keep), _bits(logits))
        assert torch.equal(row_loss2, row_loss)
        assert torch.equal(metrics2, metrics)


# -------------------------------------------------------------------- softmax
def softmax_inputs(dtype, N, seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, N, generator=g) * 2
    x[2] = (torch.randn(N, generator=g) * 30).clamp(-78, 78)
    x[2, 0] = 80.0
    x[2, N - 1] = -80.0 if N > 1 else 80.0
    dy = torch.randn(5, N, generator=g)
    return x.to(dtype), dy.to(dtype)


def softmax_ref(x, ct=torch.float64):
    x = x.to(ct)
    e = (x - x.max(1, keepdim=True).values).exp()
    return e * (1.0 / e.sum(1, keepdim=True))


def softmax_bwd_ref(dy, y, ct=torch.float64):
    dy, y = dy.to(ct), y.to(ct)
    return y * (dy - (dy * y).sum(1, keepdim=True))


@pytest.mark.parametrize("N", [1, 7, 200, 257, 1000])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_softmax_fwd_bwd_paths(dtype, N):
    x, dy = (t.to(DEV) for t in softmax_inputs(dtype, N))
    n0, n1 = K.STATS["softmax_fwd"], K.STATS["softmax_bwd"]
    y = K.softmax_fwd(x)
    _ran("softmax_fwd", n0)
    bf, bb = (_BF, _BF) if dtype == BF16 else (_SM_FWD, _SM_BWD)
    kf, kb = ("bf16_out", "bf16_out") if dtype == BF16 else ("softmax_fwd", "softmax_bwd")
    assert _obs(kf, f"softmax_fwd-{N}", _rel64(y, softmax_ref(x)), bf) < bf
    # backward against the VJP at the kernel's own (rounded) y
    dx = K.softmax_bwd(dy, y)
    _ran("softmax_bwd", n1)
    assert _obs(kb, f"softmax_bwd-{N}", _rel64(dx, softmax_bwd_ref(dy, y)), bb) < bb


# ------------------------------------------------------------------ optimizer
ADAM_HP = dict(lr=_f32(1e-3), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-8), wd=_f32(0.01))
ADAM_N = {"n8": 8 * 1031, "n8p4": 8 * 1031 + 4, "goff8": 8 * 1031}


def opt_inputs(n, gdtype, seed=22):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g)
    grads = [(torch.randn(n, generator=g) * (1 + 0.5 * i)).to(gdtype) for i in range(3)]
    return w, grads


def adam_ref(w, g, m, v, step, gs, decoupled, ct=torch.float64, lr=ADAM_HP["lr"], b1=ADAM_HP["b1"],
             b2=ADAM_HP["b2"], eps=ADAM_HP["eps"], wd=ADAM_HP["wd"]):
    """One step of optimizer.hip's Adam from (w, m, v): the new (w, m, v)."""
    w, g, m, v = w.to(ct), g.to(ct), m.to(ct), v.to(ct)
    gg = g * gs
    if not decoupled:
        gg = gg + wd * w
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 - b1 ** step
    bc2s = math.sqrt(1.0 - b2 ** step)
    upd = (m / bc1) / (v.sqrt() / bc2s + eps)
    if decoupled:
        upd = upd + wd * w
    return w - lr * upd, m, v


def _adam_cases():
    out = []
    for layout in ("n8", "n8p4", "goff8"):
        for gdt in (F32, BF16):
            if layout == "goff8" and gdt == F32:
                continue   # a 4-wide fp32 load needs 16 bytes; only bf16 gradients may be 8-byte aligned
            for dec in (False, True):
                for gs in (1.0, 1.0 / 128):
                    for hp in (False, True):
                        out.append(pytest.param(layout, gdt, dec, gs, hp, id="-".join(
                            (layout, "bf16" if gdt == BF16 else "f32", "decoupled" if dec else "coupled",
                             "gs1" if gs == 1.0 else "gs128", "hp" if hp else "host"))))
    return out


@pytest.mark.parametrize("layout,gdtype,decoupled,gs,use_hp", _adam_cases())
def test_adam_paths(layout, gdtype, decoupled, gs, use_hp):
    n = ADAM_N[layout]
    w_c, grads_c = opt_inputs(n, gdtype)
    w = w_c.to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    wb = torch.zeros(n, device=DEV, dtype=BF16)
    hp = torch.zeros(2, device=DEV) if use_hp else None
    h = ADAM_HP
    for step in (1, 2, 3):
        g = grads_c[step - 1].to(DEV)
        if layout == "goff8":   # the same values 8 bytes into a 16-byte aligned buffer
            buf = torch.zeros(n + 8, device=DEV, dtype=BF16)
            buf[4:4 + n] = g
            g = buf[4:4 + n]
            assert g.data_ptr() % 16 == 8
        w_ref, m_ref, v_ref = adam_ref(w, g, m, v, step, gs, decoupled)
        w0 = w.double()
        lr_arg, step_arg = h["lr"], step
        if use_hp:   # the kernel must read lr and step from the device, not these
            hp.copy_(torch.tensor([h["lr"], float(step)]))
            lr_arg, step_arg = 3 * h["lr"], step + 5
        n0 = K.STATS["adam_step"]
        K.adam_step(w, g, m, v, wb, lr_arg, h["b1"], h["b2"], h["eps"], h["wd"], step_arg, grad_scale=gs,
                    decoupled=decoupled, hp=hp)
        _ran("adam_step", n0)
        tag = f"{layout}-{gdtype}-{decoupled}-{gs:.3g}-{use_hp}-s{step}"
        assert _obs("adam_update", tag, _rel64(w.double() - w0, w_ref - w0), _ADAM_UPD) < _ADAM_UPD
        assert _obs("adam_m_v", "m-" + tag, _rel64(m, m_ref), _ADAM_MV) < _ADAM_MV
        assert _obs("adam_m_v", "v-" + tag, _rel64(v, v_ref), _ADAM_MV) < _ADAM_MV
        assert torch.equal(wb, w.to(BF16))


SGD_HP = dict(lr=_f32(0.1), mu=_f32(0.9), wd=_f32(1e-4))
SGD_CASES = {  # id: (gradient dtype, momentum buffer, nesterov, grad_scale)
    "nomom": (F32, False, False, 1.0),
    "momentum": (F32, True, False, 1.0),
    "nesterov": (F32, True, True, 1.0),
    "bf16": (BF16, True, True, 1.0),
    "gs128": (F32, True, False, 1.0 / 128),
    "bf16-nomom-gs128": (BF16, False, False, 1.0 / 128),
}


def sgd_ref(w, g, mom, nesterov, gs, ct=torch.float64, lr=SGD_HP["lr"], mu=SGD_HP["mu"], wd=SGD_HP["wd"]):
    """One step of optimizer.hip's SGD from (w, mom): the new (w, mom)."""
    w, g = w.to(ct), g.to(ct)
    gg = g * gs + wd * w
    if mom is not None:
        mom = mu * mom.to(ct) + gg
        gg = gg + mu * mom if nesterov else mom
    return w - lr * gg, mom


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd_paths(case):
    gdtype, has_mom, nesterov, gs = SGD_CASES[case]
    n = 8 * 1031 + 4
    w_c, grads_c = opt_inputs(n, gdtype, seed=23)
    w = w_c.to(DEV)
    mom = torch.zeros(n, device=DEV) if has_mom else None
    wb = torch.zeros(n, device=DEV, dtype=BF16)
    h = SGD_HP
    for step in (1, 2, 3):
        g = grads_c[step - 1].to(DEV)
        w_ref, mom_ref = sgd_ref(w, g, mom, nesterov, gs)
        w0 = w.double()
        n0 = K.STATS["sgd_step"]
        K.sgd_step(w, g, mom, wb, h["lr"], h["mu"], h["wd"], nesterov, grad_scale=gs)
        _ran("sgd_step", n0)
        assert _obs("sgd_update", f"{case}-s{step}", _rel64(w.double() - w0, w_ref - w0), _SGD_UPD) < _SGD_UPD
        if has_mom:
            assert _obs("sgd_mom", f"{case}-s{step}", _rel64(mom, mom_ref), _SGD_MOM) < _SGD_MOM
        assert torch.equal(wb, w.to(BF16))


def test_optimizer_gradient_contract():
    """What the wrappers accept as g: fp32 on 16 bytes, bf16 on 8 (the 4-wide
    kernels read four bf16 at a time); anything else is refused before a launch."""
    n = 64
    w = torch.ones(n, device=DEV)
    m, v, mom = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    g32 = torch.zeros(n + 4, device=DEV)[2:2 + n]                   # fp32, 8 bytes off
    g16 = torch.zeros(n + 8, device=DEV, dtype=BF16)[2:2 + n]       # bf16, 4 bytes off
    assert g32.data_ptr() % 16 == 8 and g16.data_ptr() % 8 == 4
    n0, n1 = K.STATS["adam_step"], K.STATS["sgd_step"]
    for g, err in ((g32, ValueError), (g16, ValueError), (torch.zeros(n, device=DEV, dtype=torch.float16), TypeError),
                   (torch.zeros(n + 4, device=DEV), ValueError)):
        with pytest.raises(err):
            K.adam_step(w, g, m, v, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
        with pytest.raises(err):
            K.sgd_step(w, g, mom, None, 0.1, 0.9, 0.0, False)
    assert (K.STATS["adam_step"], K.STATS["sgd_step"]) == (n0, n1)
    assert torch.equal(w, torch.ones(n, device=DEV))


SUMSQ_N = [4, 4 * 255, 4 * 70001]


def sumsq_inputs(n, seed=24):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def sumsq_ref(x, start, ct=torch.float64):
    x = x.to(ct)
    return (x * x).sum() + start


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sum_squares(n):
    x = sumsq_inputs(n).to(DEV)
    out = torch.full((1,), 0.5, device=DEV)   # accumulated into, not overwritten
    n0 = K.STATS["sum_squares"]
    K.sum_squares(x, out)
    _ran("sum_squares", n0)
    ref = sumsq_ref(x, 0.5).item()
    assert _obs("sum_squares", str(n), abs(out.item() - ref) / ref, _SUMSQ) < _SUMSQ


# ------------------------------------------------------------------ layernorm
LN_SHAPES = [(3, 512), (4133, 512), (1030, 1536),      # register-resident rows (N % 512 == 0)
             (5, 8), (259, 520), (3, 4104)]            # generic
LN_COMBOS = {  # id: (residual, save_sum, gamma/beta, dres, (dgamma, dbeta, dsum))
    "all": (True, True, True, True, (True, True, True)),
    "dsum": (False, True, True, False, (False, False, True)),
    "nogamma": (True, False, False, False, (True, False, False)),
    "dbeta": (False, True, True, True, (False, True, False)),
}
_LN_EPS = _f32(1e-5)


def ln_inputs(M, N, dtype, seed=25):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    x, r, dy, dres = mk(M, N) + 0.3, mk(M, N), mk(M, N), mk(M, N)
    gamma, beta = 1 + 0.1 * mk(N), 0.1 * mk(N)
    start = 0.5 * mk(3, N)     # the column sums are accumulated into these
    return tuple(t.to(dtype) for t in (x, r, dy, dres, gamma, beta)) + (start,)


def ln_stats(x, r, ct=torch.float64):
    """(sum, mean, rstd) of the rows of x [+ r], all in ``ct``: the statistics
    the forward kernels take from their unrounded sum."""
    t = x.to(ct) if r is None else x.to(ct) + r.to(ct)
    mean = t.mean(1, keepdim=True)
    rstd = ((t - mean).pow(2).mean(1, keepdim=True) + _LN_EPS).rsqrt()
    return t, mean, rstd


def ln_fwd_ref(x, r, gamma, beta, ct=torch.float64):
    t, mean, rstd = ln_stats(x, r, ct)
    y = (t - mean) * rstd
    if gamma is not None:
        y = y * gamma.to(ct) + beta.to(ct)
    return y


def ln_bwd_ref(dy, s, x, r, gamma, dres, ct=torch.float64):
    """(dx, colsum(dy * xhat), colsum(dy)).  As in the kernels, xhat is the
    stored (rounded) sum s normalised by the statistics of the unrounded
    x [+ r], which the forward hands to the backward."""
    _, mean, rstd = ln_stats(x, r, ct)
    dy = dy.to(ct)
    xh = (s.to(ct) - mean) * rstd
    g = dy if gamma is None else dy * gamma.to(ct)
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(ct)
    return dx, (dy * xh).sum(0), dy.sum(0)


@pytest.mark.parametrize("combo", list(LN_COMBOS))
@pytest.mark.parametrize("M,N", LN_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_layernorm_paths(dtype, M, N, combo):
    use_res, save_sum, use_gamma, use_dres, (want_dg, want_db, want_ds) = LN_COMBOS[combo]
    x, r, dy, dres, gamma, beta, start = (t.to(DEV) for t in ln_inputs(M, N, dtype))
    r = r if use_res else None
    gamma, beta = (gamma, beta) if use_gamma else (None, None)
    dres = dres if use_dres else None
    bf = dtype == BF16
    dt = "bf16" if bf else "f32"
    tag = f"{dt}-{M}x{N}-{combo}"
    n0, n1 = K.STATS["layernorm_fwd"], K.STATS["layernorm_bwd"]
    y, s, mean, rstd = K.layernorm_fwd(x, gamma, beta, _LN_EPS, residual=r, save_sum=save_sum)
    _ran("layernorm_fwd", n0)
    ky, by = ("bf16_out", _BF) if bf else ("ln_y_f32", _LN_Y_F32)
    assert _obs(ky, "ln_y-" + tag, _rel64(y, ln_fwd_ref(x, r, gamma, beta)), by) < by
    # the stored sum is the fp32 sum rounded once
    s_own = x if r is None else (x.float() + r.float()).to(dtype)
    if use_res and save_sum:
        assert torch.equal(_bits(s), _bits(s_own))
    elif use_res:
        assert s is None
        s = s_own
    else:
        assert s is x
    outs = [start[i].clone() if want else None for i, want in enumerate((want_dg, want_db, want_ds))]
    dx = K.layernorm_bwd(dy, s, mean, rstd, gamma, outs[0], outs[1], dres=dres, dsum=outs[2])
    _ran("layernorm_bwd", n1)
    dx_ref, dg_ref, db_ref = ln_bwd_ref(dy, s, x, r, gamma, dres)
    kx, bx = ("bf16_op", _BF_OP) if bf else ("ln_dx_f32", _LN_DX_F32)
    assert _obs(kx, "ln_dx-" + tag, _rel64(dx, dx_ref), bx) < bx
    # the column sums are fp32 outputs for both input types
    if want_dg:
        assert _obs("ln_colsum.dgamma_" + dt, tag, _rel64(outs[0], start[0].double() + dg_ref), _LN_COLSUM) \
            < _LN_COLSUM
    if want_db:
        assert _obs("ln_colsum.dbeta_" + dt, tag, _rel64(outs[1], start[1].double() + db_ref), _LN_COLSUM) \
            < _LN_COLSUM
    if want_ds:   # the kernel sums its fp32 dx; the stored dx is that rounded to bf16
        ks, bs = ("bf16_out", _BF) if bf else ("ln_colsum.dsum_f32", _LN_COLSUM)
        assert _obs(ks, "ln_dsum-" + tag, _rel64(outs[2], start[2].double() + dx.double().sum(0)), bs) < bs


# ---------------------------------------------------------------- activations
ACTS = ["none", "relu", "sigmoid", "tanh", "gelu", "elu", "exp"]
ACT_SHAPES = [(1, 8), (37, 520), (300, 1032)]
_ALPHA = _f32(0.7)
_K0, _K1 = 0.7978845608028654, 0.044715


def act_inputs(act, M, N, dtype, seed=26):
    """x, bias, dy (CPU).  Columns 0-3 have no bias: 0 / 1 hold +-20 in row 0
    (gelu / sigmoid / tanh saturate), 2 / 3 values within 1e-3 of zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g) * 2
    bias = torch.randn(N, generator=g)
    if act == "exp":
        x, bias = x.clamp(-4, 4), bias.clamp(-1, 1)
    bias[:4] = 0
    x[:, 2] = (torch.rand(M, generator=g) * 2 - 1) * 1e-3
    x[:, 3] = (torch.rand(M, generator=g) * 2 - 1) * 1e-3
    if act != "exp":
        x[0, 0], x[0, 1] = 20.0, -20.0
    dy = torch.randn(M, N, generator=g)
    return x.to(dtype), bias.to(dtype), dy.to(dtype)


def act_fn(act, u, exact):
    """The activation: exact functions for the fp64 reference, elementwise.hip's
    own formulas (exact=False) for the fp32 floor."""
    if act == "relu":
        return torch.relu(u)
    if act == "sigmoid":
        return torch.sigmoid(u) if exact else 1.0 / (1.0 + (-u).exp())
    if act == "tanh":
        return torch.tanh(u) if exact else 1.0 - 2.0 / ((2.0 * u).exp() + 1.0)
    if act == "gelu":
        if exact:
            return torch.nn.functional.gelu(u, approximate="tanh")
        return u * (1.0 / (1.0 + (-2.0 * _K0 * u * (1.0 + _K1 * u * u)).exp()))
    if act == "elu":
        return torch.where(u > 0, u, _ALPHA * (torch.expm1(u) if exact else u.exp() - 1.0))
    if act == "exp":
        return u.exp()
    return u


def act_grad_fn(act, u, exact):
    if exact:
        uu = u.detach().clone().requires_grad_(True)
        act_fn(act, uu, True).backward(torch.ones_like(uu))
        return uu.grad
    if act == "relu":
        return (u > 0).to(u.dtype)
    if act == "sigmoid":
        s = 1.0 / (1.0 + (-u).exp())
        return s * (1.0 - s)
    if act == "tanh":
        t = 1.0 - 2.0 / ((2.0 * u).exp() + 1.0)
        return 1.0 - t * t
    if act == "gelu":
        s = 1.0 / (1.0 + (-2.0 * _K0 * u * (1.0 + _K1 * u * u)).exp())
        w = u * (2.0 * _K0 * (1.0 + 3.0 * _K1 * u * u))
        return w * (s - s * s) + s
    if act == "elu":
        return torch.where(u > 0, torch.ones_like(u), _ALPHA * u.exp())
    if act == "exp":
        return u.exp()
    return torch.ones_like(u)


def _fwd_check(name, act, y, u64, bf):
    key, bound = ("bf16_out", _BF) if bf else ("act_fwd_" + act, _ACT_FWD[act])
    ref = act_fn(act, u64, True)
    assert _obs(key, name, _rel64(y, ref), bound) <= bound
    if act == "tanh":   # values near zero: absolute error (plus the output rounding for bf16)
        a = (y[:, 2:4].double() - ref[:, 2:4]).abs() - (ref[:, 2:4].abs() * 2.0 ** -9 if bf else 0.0)
        assert _obs("tanh0_abs", name, a.max().item(), _TANH0_ABS) < _TANH0_ABS


@pytest.mark.parametrize("M,N", ACT_SHAPES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_activation_paths(dtype, act, M, N):
    x, bias, dy = (t.to(DEV) for t in act_inputs(act, M, N, dtype))
    bf = dtype == BF16
    tag = f"-{'bf16' if bf else 'f32'}-{act}-{M}x{N}"
    # ---- forward: with bias (+ saved pre-activation), without bias, save_pre=False
    n0 = K.STATS["bias_act_fwd"]
    y, pre = K.bias_act_fwd(x, bias, act, alpha=_ALPHA)
    _ran("bias_act_fwd", n0)
    assert torch.equal(_bits(pre), _bits((x.float() + bias.float()).to(dtype)))
    _fwd_check("act_fwd" + tag, act, y, x.double() + bias.double(), bf)
    y_nb, pre_nb = K.bias_act_fwd(x, None, act, alpha=_ALPHA)
    assert pre_nb is x
    _fwd_check("act_fwd_nobias" + tag, act, y_nb, x.double(), bf)
    y_np, pre_np = K.bias_act_fwd(x, bias, act, alpha=_ALPHA, save_pre=False)
    assert pre_np is x and torch.equal(_bits(y_np), _bits(y))
    # ---- backward from the stored pre-activation
    g_ref = dy.double() * act_grad_fn(act, pre.double(), True)
    start = torch.linspace(-1, 1, N, device=DEV)
    dbias = start.clone()
    n0 = K.STATS["colsum_act"]
    dx = K.colsum_act(dy, pre, act, dbias, alpha=_ALPHA)
    _ran("colsum_act", n0)
    kx, bx = ("bf16_out", _BF) if bf else ("act_bwd_" + act, _ACT_BWD[act])
    assert _obs(kx, "act_bwd" + tag, _rel64(dx, g_ref), bx) <= bx
    kd, bd = "act_dbias_" + act, _ACT_DBIAS[act]
    db_ref = start.double() + g_ref.sum(0)
    assert _obs(kd, "act_dbias" + tag, _rel64(dbias, db_ref), bd) < bd
    # dbias=None: the same dx; act_bwd: the same product rounded once
    assert torch.equal(_bits(K.colsum_act(dy, pre, act, None, alpha=_ALPHA)), _bits(dx))
    n0 = K.STATS["act_bwd"]
    assert torch.equal(_bits(K.act_bwd(dy, pre, act, alpha=_ALPHA)), _bits(dx))
    _ran("act_bwd", n0)
    # write_dx=False: only the column sums
    dbias2 = start.clone()
    assert K.colsum_act(dy, pre, act, dbias2, write_dx=False, alpha=_ALPHA) is None
    assert _obs(kd, "act_dbias_nodx" + tag, _rel64(dbias2, db_ref), bd) < bd
    # pre=None: a plain column sum of dy, whatever activation is named
    dbias3 = start.clone()
    dx3 = K.colsum_act(dy, None, act, dbias3, alpha=_ALPHA)
    assert torch.equal(_bits(dx3), _bits(dy))
    assert _obs("act_dbias_none", "colsum_plain" + tag, _rel64(dbias3, start.double() + dy.double().sum(0)),
                _ACT_DBIAS["none"]) < _ACT_DBIAS["none"]


def test_cast_bitwise():
    g = torch.Generator().manual_seed(27)
    n = 8 * 517
    x = torch.randn(n, generator=g) * 10
    # exactly halfway between two bf16 neighbours, even and odd low bit, both signs
    lo = torch.randn(1024, generator=g).to(BF16)
    up = (lo.view(torch.int16) + 1).view(BF16)      # next bf16 away from zero
    x[:1024] = (lo.float() + up.float()) / 2
    x = x.to(DEV)
    assert (x[:1024].view(torch.int32) & 0xFFFF == 0x8000).all()
    n0 = K.STATS["cast"]
    b = K.cast_(x, torch.empty(n, device=DEV, dtype=BF16))
    assert torch.equal(_bits(b), _bits(x.to(BF16)))
    f = K.cast_(b, torch.empty(n, device=DEV, dtype=F32))
    _ran("cast", n0, 2)
    assert torch.equal(_bits(f), _bits(b.float()))


def test_dropout_fp32():
    g = torch.Generator().manual_seed(28)
    n = 8 * 1031
    x = (1 + torch.rand(n, generator=g)).to(DEV)       # [1, 2): a dropped value is the only zero
    p = 0.25
    n0 = K.STATS["dropout"]
    y = K.dropout(x, p, 1234)
    yb = K.dropout(x.to(BF16), p, 1234)
    _ran("dropout", n0, 2)
    keep = y != 0
    assert torch.equal(keep, yb != 0)                  # the mask depends on (seed, index) only
    assert 0.70 < keep.float().mean().item() < 0.80
    ref = x.double()[keep] / (1.0 - _f32(p))
    ulp = torch.from_numpy(np.spacing(ref.float().cpu().numpy())).to(DEV).double()
    assert ((y[keep].double() - ref).abs() <= 2 * ulp).all()
    assert torch.equal(_bits(K.dropout(x, 0.0, 99)), _bits(x))
