#!/usr/bin/env python3
"""Time the BERT-large training step over the same sequences padded and packed.

`--sequences` sequences of lengths uniform in [S / 8, S] (fixed seed) are run
 * padded: a [sequences, S] batch with key_lengths + query_lengths, and
 * packed: first-fit into rows of S tokens, a [packs, S] batch with
   packed_sequences = M (the most sequences of a row),
each as a captured training step (Adam, the model and settings of bench.py),
and reported in sequences per second.  One JSON line per variant and a summary.

    python tools/bert_packed_step.py [--sequences 128] [--seq 512] [--layers 24] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from attn_time import first_fit  # noqa: E402


def _step_time(cfg_kw, feeds, labels, args):
    from flexflow_train_amd.core import AdamOptimizer, FFConfig, FFModel, LossType
    from flexflow_train_amd.models.bert import bert_large, build_bert

    rows = labels.shape[0]
    cfg = FFConfig()
    cfg.batch_size = rows
    cfg.print_freq = 0
    cfg.only_data_parallel = True
    cfg.compute_dtype = "bfloat16"
    model = FFModel(cfg)
    build_bert(model, bert_large(batch_size=rows, sequence_length=args.seq, num_encoder_layers=args.layers, **cfg_kw))
    model.compile(optimizer=AdamOptimizer(model, alpha=1e-4, weight_decay=0.01, decoupled=True),
                  loss_type=LossType.LOSS_SPARSE_CATEGORICAL_CROSSENTROPY)
    ex = model.executor
    step = ex.make_graphed_train_step(feeds, labels)
    for _ in range(args.warmup):
        step(feeds, labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(feeds, labels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1000.0
    del step, ex, model
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=128)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    B, S, dev, vocab = args.sequences, args.seq, "cuda", 30522
    g = torch.Generator().manual_seed(args.seed)
    lens = torch.randint(S // 8, S + 1, (B,), generator=g, dtype=torch.int32)
    ids = torch.randint(0, vocab, (B, S), generator=g, dtype=torch.int32)
    lab = torch.randint(0, vocab, (B, S), generator=g)
    live = torch.arange(S).view(1, S) < lens.view(B, 1)
    pos = torch.arange(S, dtype=torch.int32).repeat(B, 1)
    padded = {"input_ids": ids, "position_ids": pos, "token_type_ids": torch.zeros(B, S, dtype=torch.int32),
              "seq_lens": lens}
    plab = torch.where(live, lab, torch.full_like(lab, -100))
    # the same sequences, first-fit into rows of S tokens; positions restart per sequence, labels -100 on the tails
    ll = lens.tolist()
    rows = first_fit(ll, S)
    N, M = len(rows), max(len(r) for r in rows)
    kids = torch.zeros(N, S, dtype=torch.int32)
    kpos = torch.zeros(N, S, dtype=torch.int32)
    klab = torch.full((N, S), -100)
    seg = torch.zeros(N, M, dtype=torch.int32)
    for n, r in enumerate(rows):
        at = 0
        for m, i in enumerate(r):
            kids[n, at:at + ll[i]], kpos[n, at:at + ll[i]] = ids[i, :ll[i]], pos[i, :ll[i]]
            klab[n, at:at + ll[i]] = lab[i, :ll[i]]
            seg[n, m] = ll[i]
            at += ll[i]
    packed = {"input_ids": kids, "position_ids": kpos, "token_type_ids": torch.zeros(N, S, dtype=torch.int32),
              "seg_lens": seg}
    out = {"sequences": B, "seq": S, "layers": args.layers, "mean_len": round(float(lens.float().mean()), 1),
           "packs": N, "M": M, "tokens_live": int(lens.sum()), "tokens_padded": B * S, "tokens_packed": N * S}
    for tag, kw, feeds, labels in (("padded", dict(key_lengths=True, query_lengths=True), padded, plab),
                                   ("packed", dict(packed_sequences=M), packed, klab)):
        feeds = {k: v.to(dev) for k, v in feeds.items()}
        ms = _step_time(kw, feeds, labels.to(dev), args)
        out[f"{tag}_ms"] = round(ms, 2)
        out[f"{tag}_sequences_per_sec"] = round(B / ms * 1000.0, 1)
        print(json.dumps({"variant": tag, "rows": labels.shape[0], "ms": round(ms, 2)}), flush=True)
    out["speedup"] = round(out["padded_ms"] / out["packed_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
