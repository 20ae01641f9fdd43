#!/usr/bin/env python3
"""Throughput of cross-encoder teacher scoring (CrossEncoder.score_cached: device pair assembly, packed encoder, classification head) on
synthetic MS MARCO-shaped pairs: queries of ~10 content tokens, passages with the length model of cldrd_amd.synthetic (median ~74 tokens),
max_len 256, random weights (BERT-base, DistilBERT and the MiniLM-L-6 shape: BERT, d 384, 12 heads of head dim 32, 6 layers, FFN 1536 - the
shape of cross-encoder/ms-marco-MiniLM-L-6-v2), pairs batched by length as retriever.rerank_top_passages batches them.

Prints pairs/s, model TFLOP/s and the fraction of the 2.5 PF dense 16-bit peak, with the FLOPs of SURVEY.md section 8 a4 over the real pair
lengths: nl * (8 L d^2 + 4 L d dff + 4 L^2 d) per pair (the model's FLOPs; the CLS-only last layer executes fewer).

    python tools/time_rerank.py [--pairs 32768] [--batch_size 2048] [--reps 3] [--out FILE] [--models NAME,NAME]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

PEAK_TFLOPS = 2500.0
MINILM_L6 = dict(arch="bert", vocab_size=30522, dim=384, n_heads=12, hidden_dim=1536, n_layers=6, max_position_embeddings=512)


def caches(n_q, n_p, max_len, seed=7):
    from cldrd_amd import synthetic as syn
    from cldrd_amd.dataset import SequenceTokenCache
    q_lens = (syn.randint(seed, 6, 15, n_q) + 2).astype(np.int32)          # ~10 content tokens + [CLS] / [SEP]
    p_lens = syn.msmarco_lengths(seed + 1, n_p, max_len).astype(np.int32)
    out = []
    for k, (n, lens) in enumerate(((n_q, q_lens), (n_p, p_lens))):
        ids = syn.token_ids(seed + 2 + k, n, max_len).astype(np.uint16)
        ar = np.arange(max_len)[None, :]
        ids = np.where(ar < lens[:, None], ids, 0).astype(np.uint16)
        ids[np.arange(n), lens - 1] = syn.SEP_ID
        out.append(SequenceTokenCache(np.arange(n, dtype=np.int64), ids, lens, {"rows": n, "max_length": max_len}))
    return out


def run(name, n_pairs, batch_size, reps, max_len=256):
    from cldrd_amd.encoder import _KNOWN, EncoderConfig
    from cldrd_amd.models.cross_encoder import CrossEncoder, pair_lengths
    from cldrd_amd.retriever.rerank_top_passages import length_batches
    cfg = EncoderConfig(**(MINILM_L6 if name == "minilm-l6-shape" else _KNOWN[name]))
    model = CrossEncoder(cfg, num_labels=1, seed=3, max_len=max_len).cuda()
    per_q = 200
    n_q = (n_pairs + per_q - 1) // per_q
    qc, pc = caches(n_q, n_pairs, max_len)
    q_rows = np.repeat(np.arange(n_q), per_q)[:n_pairs]
    p_rows = np.arange(n_pairs)
    _, _, lengths, _ = pair_lengths(qc.lens[q_rows] - 2, pc.lens[p_rows] - 2, max_len)
    L = lengths.astype(np.float64)
    d, f, nl = cfg.dim, cfg.hidden_dim, cfg.n_layers
    flops = float(np.sum(nl * (8 * L * d * d + 4 * L * d * f + 4 * L * L * d)))
    batches = length_batches(lengths, batch_size)

    def once():
        for b in batches:
            model.score_cached(qc, pc, q_rows[b], p_rows[b], max_len)
    once()                                                  # warm-up: kernels, allocator
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    tf = flops / best / 1e12
    return (f"{name}: {n_pairs} pairs (mean {L.mean():.1f} tokens, max {int(L.max())}) in batches of {batch_size}: "
            f"{n_pairs / best:,.0f} pairs/s, {best * 1e3:.1f} ms, model {tf:.1f} TFLOP/s = {tf / PEAK_TFLOPS:.3f} of the 2.5 PF peak "
            f"(CLDRD_AMP={os.environ.get('CLDRD_AMP', 'fp16')}, best of {reps})"), flops, n_pairs / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32768)
    ap.add_argument("--batch_size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--models", default="bert-base-uncased,distilbert-base-uncased,minilm-l6-shape")
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = [f"command: python tools/time_rerank.py {' '.join(sys.argv[1:])}",
             f"device: {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs)"]
    base = None
    for name in a.models.split(","):
        line, flops, pps = run(name, a.pairs, a.batch_size, a.reps)
        if name == "bert-base-uncased":
            base = (flops, pps)
        elif base:
            line += f"; {flops / base[0]:.3f} of BERT-base's model FLOPs, {pps / base[1]:.2f} x its pairs/s"
        lines.append(line)
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
