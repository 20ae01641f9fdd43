#!/usr/bin/env python3
"""Seconds per validation of a student on a dev run (evaluation.DevPool + RerankingEvaluator.compute_metrics_pool, what the trainer's
--dev_path runs at every checkpoint): a pool generated from a seed, no files - 1000 queries x 200 candidates drawn from an 8.84 M-id
collection, MS MARCO-shaped token counts (synthetic.msmarco_lengths; queries 6..30 tokens), full-size DistilBERT towers with random
weights - split into query encode, passage encode, score (cldrd_topk_rescore) and rank + metrics.

    python tools/time_dev_validation.py [--queries 1000] [--per_query 200] [--batch_size 512] [--repeats 3] [--fp32]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from cldrd_amd import synthetic as syn  # noqa: E402
from cldrd_amd.encoder import EncoderConfig  # noqa: E402
from cldrd_amd.evaluation import DevPool, RerankingEvaluator  # noqa: E402
from cldrd_amd.models import NwayDualEncoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--per_query", type=int, default=200)
ap.add_argument("--batch_size", type=int, default=512)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--fp32", action="store_true", help="the exact fp32 evaluation pass (model.eval_fp32)")
a = ap.parse_args()

N_COLLECTION, Q_LEN, P_LEN = 8841823, 30, 256
qids = np.repeat(np.arange(a.queries, dtype=np.int64) + 1_000_000, a.per_query)
pids = syn.randint(a.seed, 0, N_COLLECTION, a.queries * a.per_query)


def tokens(which, ids, max_len):
    """row i: [CLS] body [SEP] of the id's own length - a function of (seed, id) through the id's position in the pool"""
    n = ids.shape[0]
    if which == "q":
        lens = 6 + syn.randint(a.seed + 1, 0, max_len - 5, n)
    else:
        lens = syn.msmarco_lengths(a.seed + 2, n, max_len)
    body = syn.token_ids(a.seed + (3 if which == "q" else 4), n, max_len).astype(np.int32)
    sep = body[:, -1].copy()
    body[np.arange(max_len)[None, :] >= lens[:, None]] = 0
    body[np.arange(n), lens - 1] = sep
    return body, lens.astype(np.int32)


t0 = time.perf_counter()
pool = DevPool.from_pairs(qids, pids, tokens, Q_LEN, P_LEN, name="<synthetic dev run>")
t_pool = time.perf_counter() - t0
with tempfile.TemporaryDirectory() as td:
    qrels = os.path.join(td, "qrels.tsv")
    with open(qrels, "w") as fh:           # one relevant passage per query: its candidate at a pseudo-random run position
        at = syn.randint(a.seed + 5, 0, a.per_query, a.queries)
        for g in range(pool.n_queries):
            lo, hi = int(pool.starts[g]), int(pool.starts[g + 1])
            fh.write(f"{int(pool.query_ids[g])}\t0\t{int(pool.pids[lo + int(at[g]) % (hi - lo)])}\t1\n")
    ev = RerankingEvaluator(qrels)
torch.cuda.set_device(0)
model = NwayDualEncoder(EncoderConfig(arch="distilbert"), share_weights=False).cuda()
model.eval_fp32 = bool(a.fp32)
n_tok = int(pool.p_lens.sum())
print(f"dev validation, {'fp32' if a.fp32 else '16-bit'} evaluation pass, full-size DistilBERT towers (random weights), batches of {a.batch_size}: "
      f"{pool.n_queries} queries x {a.per_query} candidates = {pool.n_pairs} pairs, {pool.n_passages} distinct passages "
      f"(mean {n_tok / pool.n_passages:.1f} tokens, max {int(pool.p_lens.max())}); pool built on the host in {t_pool:.2f} s")
for r in range(a.repeats + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = ev.compute_metrics_pool(model, pool, batch_size=a.batch_size)
    total = time.perf_counter() - t0
    tm = ev.last_timings
    print(f"{'warm-up' if r == 0 else f'run {r}  '}: {total:.3f} s per validation = query encode {tm['query_encode_s']:.3f} + passage encode "
          f"{tm['passage_encode_s']:.3f} ({pool.n_passages / tm['passage_encode_s']:.0f} passages/s, {n_tok / tm['passage_encode_s'] / 1e6:.2f} M tokens/s) "
          f"+ score {tm['score_s']:.3f} + rank and metrics {tm['rank_metrics_s']:.3f}; MRR@10 {float(m['MRR@10']):.4f}")
