#!/usr/bin/env python3
"""Time the flash-attention forward and backward (HIP events) on the BERT-large
and GPT-3-medium shapes; FF_PKG_ROOT selects the package tree (same-box A/B of
two builds: FF_PKG_ROOT=ab_prev python tools/attn_time.py).

    python tools/attn_time.py [iters]
    python tools/attn_time.py --onepass-ab                            (same-process A/B of the one-pass backward)
    python tools/attn_time.py --dropout 0.1                           (attention dropout against p = 0)
    python tools/attn_time.py --varlen [--dropout 0.1]                (per-sample key lengths against full length)
    python tools/attn_time.py --varlen --queries [--dropout 0.1]      (the same lengths as query lengths too)
    python tools/attn_time.py --packed [--dropout 0.1]                (packed sequences against the padded batch)
    python tools/attn_time.py --bias key|full                         (additive mask / bias against no bias, kv_lens
                                                                       and the unfused operator chain)
    python tools/attn_time.py --gqa G                                 (grouped-query K / V heads, H / G of them,
                                                                       against the expanded call and the H-head call)

--d128 appends two D = 128 shapes to whichever mode is run.
"""
import json
import os
import sys

sys.path.insert(0, os.environ.get("FF_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flexflow_train_amd import kernels as K  # noqa: E402

SHAPES = {"bert-large": (64, 512, 16, 64, False), "gpt3-medium": (16, 2048, 16, 64, True),
          # the shipped bench batches
          "bert-large-b128": (128, 512, 16, 64, False), "gpt3-medium-b32": (32, 2048, 16, 64, True)}
if "--d128" in sys.argv:
    sys.argv.remove("--d128")
    SHAPES.update({"d128": (8, 1024, 16, 128, False), "d128-causal": (8, 1024, 16, 128, True)})


def _time(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def env_ab(var, which, iters, rounds=5):
    """Interleaved same-process A/B of one kernel switch (env `var` 0 vs 1,
    read per launch by attention.hip) on the forward or the backward."""
    import statistics
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        o, lse = K.attention_fwd(q, k, v, causal=causal)
        if which == "fwd":
            fn = lambda: K.attention_fwd(q, k, v, causal=causal, out=o)  # noqa: E731
        else:
            fn = lambda: K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1],  # noqa: E731
                                         dqkv[:, :, 2], causal=causal)
        t = {0: [], 1: []}
        for _ in range(rounds):
            for p in (0, 1):
                os.environ[var] = str(p)
                t[p].append(_time(fn, iters))
        fl = 4 * B * H * S * S * D * (0.5 if causal else 1.0) * (1.0 if which == "fwd" else 2.5)
        med = {p: statistics.median(v) for p, v in t.items()}
        print(json.dumps({"shape": name, "switch": var, "pass": which, "ms_0": round(med[0], 4),
                          "ms_1": round(med[1], 4), "tflops_0": round(fl / med[0] / 1e9, 1),
                          "tflops_1": round(fl / med[1] / 1e9, 1),
                          "rounds_0": [round(x, 4) for x in t[0]], "rounds_1": [round(x, 4) for x in t[1]]}),
              flush=True)
    os.environ.pop(var, None)


def pmc_run(n=5):
    """A few dispatches of each kernel for a counter pass (rocprofv3 --pmc):
    forward and backward, at both bench shapes."""
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        o, lse = K.attention_fwd(q, k, v, causal=causal)
        for _ in range(n):
            K.attention_fwd(q, k, v, causal=causal, out=o)
        for p in ("0", "1"):   # the dQ + dK/dV kernels, then the one-pass kernel where it applies
            os.environ["FFK_ATTN_BWD_ONEPASS"] = p
            for _ in range(n):
                K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], causal=causal)
        os.environ.pop("FFK_ATTN_BWD_ONEPASS", None)
        torch.cuda.synchronize()
        print(name, "done", flush=True)


def dropout_ab(p, iters, rounds=5):
    """Interleaved same-process timing of the forward and the backward with
    attention dropout `p` against p = 0.  With p > 0 the backward is the
    dQ + dK/dV kernel pair at every shape (the one-pass kernel of the BERT
    shapes has no dropout form)."""
    import statistics
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        t = {}
        for _ in range(rounds):
            for pp in (0.0, p):
                kw = dict(causal=causal, dropout_p=pp, seed=1234)
                o, lse = K.attention_fwd(q, k, v, **kw)
                t.setdefault(("fwd", pp), []).append(_time(lambda: K.attention_fwd(q, k, v, out=o, **kw), iters))
                t.setdefault(("bwd", pp), []).append(_time(
                    lambda: K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], **kw),
                    iters))
        fl = 4 * B * H * S * S * D * (0.5 if causal else 1.0)
        med = {key: statistics.median(v) for key, v in t.items()}
        rec = {"shape": name, "dropout": p}
        for which, mul in (("fwd", 1.0), ("bwd", 2.5)):
            for pp, tag in ((0.0, "p0"), (p, "drop")):
                rec[f"{which}_ms_{tag}"] = round(med[(which, pp)], 4)
                rec[f"{which}_tflops_{tag}"] = round(mul * fl / med[(which, pp)] / 1e9, 1)
            rec[f"{which}_rounds_p0"] = [round(x, 4) for x in t[(which, 0.0)]]
            rec[f"{which}_rounds_drop"] = [round(x, 4) for x in t[(which, p)]]
        print(json.dumps(rec), flush=True)


def varlen_ab(iters, rounds=5, seed=0, p=0.0, queries=False):
    """Interleaved same-process timing of the forward and the backward with
    per-sample key lengths drawn uniformly from [Sk / 8, Sk] (fixed seed)
    against the same call without lengths, and against lengths all equal to
    Sk (the cost of the length-aware kernels alone).  With lengths the
    backward is the dQ + dK/dV kernel pair at every shape.  `p` > 0 adds
    attention dropout to all three variants (`--varlen --dropout p`): "full"
    against "none" is then the cost of the forms with lengths and dropout,
    whose dQ kernel takes delta from the probabilities.  `live_tiles` is
    the fraction of 64-key tiles with a live key (the causal shapes count the
    tiles at or below the diagonal of each 128-query block only).
    `queries` adds a fourth variant, "varlen_q": the same lengths as the query
    lengths too (self-attention over a padded batch).  `live_pairs_q` is its
    share of live (128-query block, 64-key tile) pairs: of the pairs counted
    by `live_tiles`, those whose block also has a live query."""
    import statistics
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        lens_cpu = torch.randint(S // 8, S + 1, (B,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
        variants = {"none": None, "full": torch.full((B,), S, device="cuda", dtype=torch.int32),
                    "varlen": lens_cpu.cuda()}
        if queries:
            variants["varlen_q"] = variants["varlen"]
        live = live_q = total = 0
        for n in lens_cpu.tolist():
            for qb in range((S + 127) // 128):
                cap = min((S + 63) // 64, (qb * 128 + 128 + 63) // 64) if causal else (S + 63) // 64
                total += cap
                live += min(cap, (n + 63) // 64)
                if qb * 128 < n:
                    live_q += min(cap, (n + 63) // 64)
        t = {}
        for _ in range(rounds):
            for tag, lens in variants.items():
                kw = dict(causal=causal, kv_lens=lens, dropout_p=p, seed=1234)
                if tag == "varlen_q":
                    kw["q_lens"] = lens
                o, lse = K.attention_fwd(q, k, v, **kw)
                t.setdefault(("fwd", tag), []).append(_time(lambda: K.attention_fwd(q, k, v, out=o, **kw), iters))
                t.setdefault(("bwd", tag), []).append(_time(
                    lambda: K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], **kw),
                    iters))
        med = {key: statistics.median(x) for key, x in t.items()}
        rec = {"shape": name, "seed": seed, "dropout": p, "mean_len": round(float(lens_cpu.float().mean()), 1),
               "live_tiles": round(live / total, 4)}
        if queries:
            rec["live_pairs_q"] = round(live_q / total, 4)
        for which in ("fwd", "bwd"):
            for tag in variants:
                rec[f"{which}_ms_{tag}"] = round(med[(which, tag)], 4)
                rec[f"{which}_rounds_{tag}"] = [round(x, 4) for x in t[(which, tag)]]
        print(json.dumps(rec), flush=True)


def first_fit(lens, T):
    """Sequences of these lengths packed first-fit into rows of T tokens:
    a list of rows, each the list of its sequences' indices."""
    rows, room = [], []
    for i, n in enumerate(lens):
        for r in range(len(rows)):
            if room[r] >= n:
                rows[r].append(i)
                room[r] -= n
                break
        else:
            rows.append([i])
            room.append(T - n)
    return rows


def packed_ab(iters, rounds=5, seed=0, p=0.0):
    """Interleaved same-process timing of the forward and the backward over B
    sequences of lengths uniform in [S / 8, S] (fixed seed), padded ([B, S]
    with kv_lens = q_lens = lens) against packed first-fit into rows of T = S
    tokens ([N, S] with seg_lens [N, M], M the most sequences of a row).
    `exit_padded` / `exit_packed` are the shares of forward workgroups that
    leave at once (their 128-query block is past the sample's or segment's
    length); `tokens_padded` / `tokens_packed` the tokens the rest of a model
    would run over."""
    import statistics
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        lens = torch.randint(S // 8, S + 1, (B,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
        ll = lens.tolist()
        rows = first_fit(ll, S)
        N, M = len(rows), max(len(r) for r in rows)
        seg = torch.zeros(N, M, dtype=torch.int32)
        for n, r in enumerate(rows):
            seg[n, :len(r)] = torch.tensor([ll[i] for i in r], dtype=torch.int32)
        nq = (S + 127) // 128
        dead_pad = sum(1 for n in ll for qb in range(nq) if qb * 128 >= n)
        dead_pack = sum(1 for n in seg.reshape(-1).tolist() for qb in range(nq) if qb * 128 >= n)
        t = {}
        for tag, rows_n, kw in (("padded", B, dict(kv_lens=lens.cuda(), q_lens=lens.cuda())),
                                ("packed", N, dict(seg_lens=seg.cuda(), max_seqlen=S))):
            qkv = torch.randn(rows_n, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
            do = torch.randn(rows_n, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
            t[tag] = dict(qkv=qkv, do=do, d=torch.empty_like(qkv), kw=dict(kw, causal=causal, dropout_p=p, seed=1234),
                          fwd=[], bwd=[])
        for _ in range(rounds):
            for tag, c in t.items():
                q, k, v = c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2]
                d, kw = c["d"], c["kw"]
                if "seg_lens" in kw:   # as the operator does: the offsets once per forward, kept for the backward
                    kw = dict(kw, seg_offsets=K.attention_segment_offsets(kw["seg_lens"], S, S))
                o, lse = K.attention_fwd(q, k, v, **c["kw"])
                c["fwd"].append(_time(lambda: K.attention_fwd(q, k, v, out=o, **c["kw"]), iters))
                c["bwd"].append(_time(lambda: K.attention_bwd(q, k, v, o, lse, c["do"], d[:, :, 0], d[:, :, 1],
                                                              d[:, :, 2], **kw), iters))
        rec = {"shape": name, "seed": seed, "dropout": p, "sequences": B, "mean_len": round(float(lens.float().mean()), 1),
               "packs": N, "M": M, "tokens_padded": B * S, "tokens_packed": N * S, "tokens_live": int(lens.sum()),
               "exit_padded": round(dead_pad / (B * nq), 4), "exit_packed": round(dead_pack / (N * M * nq), 4)}
        for which in ("fwd", "bwd"):
            for tag, c in t.items():
                rec[f"{which}_ms_{tag}"] = round(statistics.median(c[which]), 4)
                rec[f"{which}_rounds_{tag}"] = [round(x, 4) for x in c[which]]
        print(json.dumps(rec), flush=True)


def bias_ab(kind, iters, rounds=5, seed=0):
    """Interleaved same-process timing of the forward and the backward with an
    additive score bias at the BERT-large and GPT-3-medium shapes, both
    non-causal (the BIAS kernels have no causal form): `key` is a key-padding
    mask [B, 1, 1, Sk] (0 / -inf, lengths uniform in [Sk / 8, Sk]), `full` a
    finite fp32 bias [1, H, Sq, Sk].  Next to it, in the same rounds: the same
    call without a bias, for `key` the call with kv_lens of the same lengths,
    and the unfused operator chain (BATCHMATMUL, SCALAR_MULTIPLY, EW_ADD,
    SOFTMAX, BATCHMATMUL on [B, H, S, D] tensors) forward and backward.
    `act_bytes_*`: what each form keeps for its backward beside q / k / v / o
    (the fp32 LSE against the bf16 probabilities [B, H, Sq, Sk])."""
    import statistics

    from flexflow_train_amd.ops import base as opbase

    def op(t, **attrs):
        return opbase.get_impl(t), opbase.OpContext(op_type=t, attrs=attrs, name=t.lower(), training=True,
                                                    compute_dtype=torch.bfloat16, device=torch.device("cuda"))

    for name in ("bert-large", "gpt3-medium"):
        B, S, H, D, _ = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        lens_cpu = torch.randint(S // 8, S + 1, (B,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
        if kind == "key":
            bias = torch.zeros(B, 1, 1, S).masked_fill(torch.arange(S).view(1, 1, 1, S) >= lens_cpu.view(B, 1, 1, 1),
                                                       float("-inf")).cuda()
        else:
            bias = 2 * torch.randn(1, H, S, S, device="cuda", generator=g)
        variants = {"none": {}, "bias": dict(bias=bias)}
        if kind == "key":
            variants["kv_lens"] = dict(kv_lens=lens_cpu.cuda())
        # the unfused chain on [B, H, S, D] copies
        qh, kh, vh, doh = (t.transpose(1, 2).contiguous() for t in (q, k, v, do))
        bm1, bm2, sc = op("BATCHMATMUL"), op("BATCHMATMUL"), op("SCALAR_MULTIPLY", scalar=1.0 / D ** 0.5)
        add, sm, tr = op("EW_ADD"), op("SOFTMAX", dim=-1), op("TRANSPOSE", perm=[0, 1, 3, 2])
        bias_c = bias.to(torch.bfloat16)

        def chain_fwd():
            saved = []

            def run(o, ins, need):
                outs, sv = o[0].forward(o[1], ins, [])
                saved.append((o[0], o[1], sv, need))
                return outs[0]

            kt = run(tr, [kh], [True])
            s = run(bm1, [qh, kt], [True, True])
            s = run(sc, [s], [True])
            s = run(add, [s, bias_c], [True, False])   # no gradient for the mask, as in SDPA
            pr = run(sm, [s], [True])
            return run(bm2, [pr, vh], [True, True]), saved

        def chain_bwd(saved):
            gr = doh
            for impl, ctx, sv, need in reversed(saved):
                grads = impl.backward(ctx, sv, [gr], [], need)
                gr = grads[1] if impl is bm1[0] and ctx is bm1[1] else grads[0]   # dK^T goes on to the transpose

        t = {}
        for _ in range(rounds):
            for tag, kw in variants.items():
                o, lse = K.attention_fwd(q, k, v, **kw)
                t.setdefault(("fwd", tag), []).append(_time(lambda: K.attention_fwd(q, k, v, out=o, **kw), iters))
                t.setdefault(("bwd", tag), []).append(_time(
                    lambda: K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], **kw),
                    iters))
            _, saved = chain_fwd()
            t.setdefault(("fwd", "unfused"), []).append(_time(lambda: chain_fwd(), max(3, iters // 5)))
            t.setdefault(("bwd", "unfused"), []).append(_time(lambda: chain_bwd(saved), max(3, iters // 5)))
            del saved
        med = {key: statistics.median(x) for key, x in t.items()}
        rec = {"shape": name + " non-causal", "bias": kind, "bias_shape": list(bias.shape),
               "mean_len": round(float(lens_cpu.float().mean()), 1) if kind == "key" else None,
               "act_bytes_flash": B * H * S * 4, "act_bytes_unfused": B * H * S * S * 2}
        for which in ("fwd", "bwd"):
            for tag in list(variants) + ["unfused"]:
                rec[f"{which}_ms_{tag}"] = round(med[(which, tag)], 4)
                rec[f"{which}_rounds_{tag}"] = [round(x, 4) for x in t[(which, tag)]]
            rec[f"{which}_bias_over_none"] = round(med[(which, "bias")] / med[(which, "none")], 3)
            rec[f"{which}_unfused_over_bias"] = round(med[(which, "unfused")] / med[(which, "bias")], 2)
        print(json.dumps(rec), flush=True)


GQA_SHAPES = {"b4-h32-d128-s2048-causal": (4, 2048, 32, 128, True), "b8-h16-d64-s2048-causal": (8, 2048, 16, 64, True)}


def gqa_ab(G, iters, rounds=5):
    """Interleaved same-process timing of the forward and the backward with
    Hkv = H / G K / V heads, three forms per shape in every round:
      gqa       the GQA kernels in place on [B, S, Hkv, D] K / V;
      expanded  what a caller had to do before: K / V copied out to H heads
                (repeat_interleave), the existing kernels, and in the backward
                the fp32 group sum of dK / dV and its cast (all of it timed);
      plain_1 / plain_2  the H-head call of the same flops, twice: the ceiling
                and its own run-to-run spread.
    A shape whose H is no multiple of G is skipped.  `dkdv_workgroups_*`: the
    dK/dV kernel's grid, B * heads * ceil(S / 128), against the 256 CUs."""
    import statistics
    for name, (B, S, H, D, causal) in GQA_SHAPES.items():
        if H % G:
            print(json.dumps({"shape": name, "G": G, "skipped": f"H = {H} is no multiple of G"}), flush=True)
            continue
        Hkv = H // G
        g = torch.Generator(device="cuda").manual_seed(0)
        q, do = (torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
        k, v = (torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
        kp, vp = (torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dkp, dvp = torch.empty_like(kp), torch.empty_like(vp)
        o = torch.empty_like(q)

        def exp_fwd():
            ke, ve = k.repeat_interleave(G, dim=2), v.repeat_interleave(G, dim=2)
            return ke, ve, K.attention_fwd(q, ke, ve, causal=causal, out=o)[1]

        def exp_bwd(ke, ve, lse):
            K.attention_bwd(q, ke, ve, o, lse, do, dq, dkp, dvp, causal=causal)
            return (dkp.view(B, S, Hkv, G, D).sum(3, dtype=torch.float32).to(torch.bfloat16),
                    dvp.view(B, S, Hkv, G, D).sum(3, dtype=torch.float32).to(torch.bfloat16))

        forms = ("gqa", "expanded", "plain_1", "plain_2")
        t = {}
        for _ in range(rounds):
            for tag in forms:
                if tag == "gqa":
                    _, lse = K.attention_fwd(q, k, v, causal=causal, out=o)
                    fwd = lambda: K.attention_fwd(q, k, v, causal=causal, out=o)  # noqa: E731
                    bwd = lambda: K.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, causal=causal)  # noqa: E731
                elif tag == "expanded":
                    ke, ve, lse = exp_fwd()
                    fwd = exp_fwd
                    bwd = lambda: exp_bwd(ke, ve, lse)  # noqa: E731
                else:
                    _, lse = K.attention_fwd(q, kp, vp, causal=causal, out=o)
                    fwd = lambda: K.attention_fwd(q, kp, vp, causal=causal, out=o)  # noqa: E731
                    bwd = lambda: K.attention_bwd(q, kp, vp, o, lse, do, dq, dkp, dvp, causal=causal)  # noqa: E731
                t.setdefault(("fwd", tag), []).append(_time(fwd, iters))
                t.setdefault(("bwd", tag), []).append(_time(bwd, iters))
        fl = 4 * B * H * S * S * D * (0.5 if causal else 1.0)
        med = {key: statistics.median(x) for key, x in t.items()}
        nkb = (S + 127) // 128
        rec = {"shape": name, "G": G, "Hkv": Hkv, "iters": iters, "rounds": rounds,
               "dkdv_workgroups_gqa": B * Hkv * nkb, "dkdv_workgroups_plain": B * H * nkb, "cus": 256,
               "kv_bytes_gqa": 2 * B * S * Hkv * D * 2, "kv_bytes_expanded": 2 * B * S * H * D * 2}
        for which, mul in (("fwd", 1.0), ("bwd", 2.5)):
            for tag in forms:
                xs = t[(which, tag)]
                rec[f"{which}_ms_{tag}"] = round(med[(which, tag)], 4)
                rec[f"{which}_tflops_{tag}"] = round(mul * fl / med[(which, tag)] / 1e9, 1)
                rec[f"{which}_spread_{tag}"] = round((max(xs) - min(xs)) / med[(which, tag)], 4)
                rec[f"{which}_rounds_{tag}"] = [round(x, 4) for x in xs]
            rec[f"{which}_gqa_over_plain"] = round(med[(which, "gqa")] / med[(which, "plain_1")], 3)
            rec[f"{which}_gqa_over_expanded"] = round(med[(which, "gqa")] / med[(which, "expanded")], 3)
            rec[f"{which}_plain_2_over_plain_1"] = round(med[(which, "plain_2")] / med[(which, "plain_1")], 3)
        print(json.dumps(rec), flush=True)


def main():
    if "--gqa" in sys.argv:            # grouped-query K / V heads against the expanded and the H-head call
        return gqa_ab(int(sys.argv[sys.argv.index("--gqa") + 1]), 200)
    if "--bias" in sys.argv:           # additive mask / bias against no bias, kv_lens and the unfused chain
        kind = sys.argv[sys.argv.index("--bias") + 1]
        if kind not in ("key", "full"):
            raise SystemExit("--bias takes key or full")
        return bias_ab(kind, 30)
    if "--packed" in sys.argv:         # packed sequences against the padded batch with key and query lengths
        return packed_ab(30, p=float(sys.argv[sys.argv.index("--dropout") + 1]) if "--dropout" in sys.argv else 0.0)
    if "--varlen" in sys.argv:         # per-sample key lengths against full length
        return varlen_ab(30, p=float(sys.argv[sys.argv.index("--dropout") + 1]) if "--dropout" in sys.argv else 0.0,
                         queries="--queries" in sys.argv)
    if "--dropout" in sys.argv:        # attention dropout against p = 0, forward and backward
        return dropout_ab(float(sys.argv[sys.argv.index("--dropout") + 1]), 30)
    if "--pmc-run" in sys.argv:
        return pmc_run()
    if "--onepass-ab" in sys.argv:     # one-pass backward (BERT shapes; the causal shapes are not eligible)
        return env_ab("FFK_ATTN_BWD_ONEPASS", "bwd", 30)
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for name, (B, S, H, D, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        do = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        dqkv = torch.empty_like(qkv)
        o, lse = K.attention_fwd(q, k, v, causal=causal)
        fwd = _time(lambda: K.attention_fwd(q, k, v, causal=causal, out=o), iters)
        bwd = _time(lambda: K.attention_bwd(q, k, v, o, lse, do, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2],
                                            causal=causal), iters)
        fl = 4 * B * H * S * S * D * (0.5 if causal else 1.0)
        print(json.dumps({"shape": name, "pkg": os.environ.get("FF_PKG_ROOT", "tree"), "fwd_ms": round(fwd, 4),
                          "bwd_ms": round(bwd, 4), "fwd_tflops": round(fl / fwd / 1e9, 1),
                          "bwd_tflops": round(2.5 * fl / bwd / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
