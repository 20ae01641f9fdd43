#!/usr/bin/env python3
"""int8-row mode of the flat index (retriever.retrieval_utils.FlatIPIndex) against fp16-row mode and fp32 mode, same process, same GPU:
resident bytes of the three modes after attach, attach seconds, search milliseconds per query tile of int8-row mode against fp16-row mode in
INTERLEAVED rounds (A B A B, both indexes attached side by side; device-resident ``search_device``), candidates and re-scored rows per query,
proof retries, and the top-10 / top-100 overlap of int8-row mode with fp32 mode and with fp16-row mode.

Workloads: one cfg5 shard (1 105 228 x 768 rows, 6 980 queries, k = 1000) of the two corpora of bench.py's retrieve leg (isotropic: Gaussian
direction x norm U(9, 12); CLS-like: synthetic.cls_like_corpus), and with ``--full`` the whole 8 841 823 rows of the isotropic corpus (int8-row
against fp16-row mode only: the fp32 mode does not fit beside them).  All rows are generated on the device and attached with
``from_device_rows``.

    timeout -k 10 900 python tools/time_index_int8.py [--rows 1105228] [--queries 6980] [--rounds 3] [--full] [--out profiles/index_int8_timing.txt]

One process, one GPU; not to be re-run after a fault before its cause is known."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cldrd_amd.synthetic as syn
from cldrd_amd.retriever import retrieval_utils as RU

DEV = torch.device("cuda", 0)
MB = 1 << 20
MODES = {"fp32": {}, "fp16": {"fp16_rows": True}, "int8": {"int8_rows": True}}


def isotropic(rows, d, seed, chunk=1 << 20):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    P = torch.empty(rows, d, device=DEV)
    for lo in range(0, rows, chunk):
        blk = torch.randn(min(chunk, rows - lo), d, device=DEV, generator=gen)
        blk *= (9.0 + 3.0 * torch.rand(blk.shape[0], 1, device=DEV, generator=gen)) / blk.norm(dim=1, keepdim=True)
        P[lo:lo + blk.shape[0]] = blk
    Q = torch.randn(6980, d, device=DEV, generator=gen)
    Q *= 10.0 / Q.norm(dim=1, keepdim=True)
    return P, Q


def attach(P, mode):
    """-> (index, seconds, resident bytes); the device rows the fp32 mode keeps are counted as its resident bytes"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    index = RU.FlatIPIndex.from_device_rows(P, **MODES[mode])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return index, dt, torch.cuda.memory_allocated() - before + (P.numel() * 4 if mode == "fp32" else 0)


def timed_search(index, Q, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D, I, st = index.search_device(Q, k)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, I, st


def overlap(Ia, Ib, k):
    a, b = Ia[:, :k].cpu().numpy(), Ib[:, :k].cpu().numpy()
    return float(np.mean([len(np.intersect1d(a[j], b[j])) / k for j in range(0, a.shape[0], 7)]))


def workload(name, P, Q, k, rounds, modes, out):
    rows, d = P.shape
    live, att = {}, {}
    for mode in modes:
        live[mode], att[mode + "_s"], att[mode + "_bytes"] = attach(P, mode)
    out.append(f"== {name}: {rows} x {d} rows (device rows -> from_device_rows), {Q.shape[0]} queries, k = {k}, {rounds} interleaved rounds ==")
    for mode in modes:
        out.append(f"{mode:5s} resident {att[mode + '_bytes'] / MB:9.1f} MB ({att[mode + '_bytes'] / (rows * d):.3f} B/element)  attach {att[mode + '_s']:6.3f} s")
    timed = [m for m in modes if m != "fp32"]
    secs = {m: [] for m in timed}
    last, stats = {}, {}
    for m in timed:
        live[m].search_device(Q, k)                                # warm-up: workspaces, clocks
    for _ in range(rounds):
        for m in timed:                                            # A B A B
            dt, last[m], _ = timed_search(live[m], Q, k)
            secs[m].append(dt)
    for m in modes:
        live[m].profile = True
        _, I, stats[m] = live[m].search_device(Q, k)
        live[m].profile = False
        last[m] = I
    for m in timed:
        st, tiles = stats[m], -(-Q.shape[0] // live[m].query_tile)
        med = statistics.median(secs[m])
        out.append(f"{m:5s} search median {med:.4f} s (rounds: {' '.join(f'{x:.4f}' for x in secs[m])}), query tile {live[m].query_tile}: "
                   f"{1e3 * med / tiles:.3f} ms / tile, {1e6 * med / Q.shape[0]:.1f} us / query")
        out.append(f"      candidates {st['candidates'] / Q.shape[0]:.0f} / query, rescored {st['rescored'] / Q.shape[0]:.0f} / query, scans {st['scans']} rescans "
                   f"{st['rescans']} unproven first pass {st['unproven_first_pass']} (bits {st['status_bits_first_pass']}) fallback queries "
                   f"{st['fallback_queries']}, pipeline {st['search_ms']:.1f} ms (HIP events)")
    a, b = statistics.median(secs["fp16"]), statistics.median(secs["int8"])
    spread = (max(secs["fp16"]) - min(secs["fp16"])) / a
    out.append(f"search int8-row / fp16-row (whole search, all queries): {b / a:.3f}; spread of the fp16 rounds {spread * 100:.1f} %")
    for other in modes:
        if other != "int8":
            out.append(f"overlap int8-row vs {other} (every 7th query, synthetic corpus): " +
                       "  ".join(f"top-{kk} {overlap(last['int8'], last[other], kk):.4f}" for kk in (10, 100, 1000) if kk <= k))
    out.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1105228)
    ap.add_argument("--queries", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also the whole 8 841 823-row collection on one GPU (int8-row against fp16-row mode)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "index_int8_timing.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    RU.cap_host_threads()
    out = ["command: python tools/time_index_int8.py " + " ".join(sys.argv[1:]),
           f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; attach chunk {RU.ATTACH_CHUNK_ROWS} rows", ""]
    d = 768
    P, Q = isotropic(args.rows, d, 1234)
    workload("isotropic (bench.py retrieve leg)", P, Q[:args.queries], args.k, args.rounds, ("fp32", "fp16", "int8"), out)
    del P
    P, u = syn.cls_like_corpus(args.rows, d, 777, DEV)
    Qc = syn.cls_like_queries(args.queries, u, 778)
    workload("CLS-like (bench.py retrieve leg, cls_like)", P, Qc, args.k, args.rounds, ("fp32", "fp16", "int8"), out)
    del P
    if args.full:
        torch.cuda.empty_cache()
        try:
            P, Q = isotropic(8841823, d, 1234)
            workload("isotropic, whole collection", P, Q[:args.queries], args.k, args.rounds, ("fp16", "int8"), out)
            del P
        except torch.cuda.OutOfMemoryError as exc:
            out.append(f"== isotropic, whole collection: not measured, the device memory does not hold the rows and both modes ({exc}) ==".replace("\n", " "))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
