#!/usr/bin/env python3
"""fp32 mode against fp16-row mode of the flat index (retriever.retrieval_utils.FlatIPIndex), same process, same GPU, interleaved A B A B:
resident bytes after attach and the peak during attach (``torch.cuda.memory_allocated`` / ``max_memory_allocated``), attach seconds, search
seconds (device-resident ``search_device``, median over the rounds), re-scored rows, scans / rescans / fallback queries, and the overlap of
the two modes' top-10 / top-100 / top-1000.

Workloads: one cfg5 shard (1 105 228 x 768 rows attached from a host array, 6 980 queries, k = 1000) of the two corpora of bench.py's
retrieve leg (isotropic: Gaussian direction x norm U(9, 12); CLS-like: synthetic.cls_like_corpus), and with ``--full`` the whole 8 841 823
rows of the isotropic corpus (generated on the device and attached with ``from_device_rows``: the host array would be 27 GB).

    timeout -k 10 900 python tools/time_index_fp16.py [--rows 1105228] [--queries 6980] [--rounds 3] [--full] [--out profiles/index_fp16_timing.txt]

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


def attach(rows_host, rows_dev, fp16_rows):
    """-> (index, seconds, resident bytes, peak bytes during attach); device rows the fp32 mode keeps are counted as its resident bytes"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    if rows_host is not None:
        index = RU.FlatIPIndex(rows_host.shape[1])
        index.add(rows_host)
        index.to_gpu(0, fp16_rows=fp16_rows)
    else:
        index = RU.FlatIPIndex.from_device_rows(rows_dev, fp16_rows=fp16_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extra = rows_dev.numel() * 4 if (rows_dev is not None and not fp16_rows) else 0
    return index, dt, torch.cuda.memory_allocated() - before + extra, torch.cuda.max_memory_allocated() - before + extra


def timed_search(index, Q, k):
    index.search_device(Q, k)                                     # warm-up (workspaces; clocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D, I, st = index.search_device(Q, k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    index.profile = True
    _, _, stp = index.search_device(Q, k)
    index.profile = False
    return dt, D, I, stp


def overlap(Ia, Ib, k):
    a, b = Ia[:, :k].cpu().numpy(), Ib[:, :k].cpu().numpy()
    return float(np.mean([len(np.intersect1d(a[j], b[j])) / k for j in range(0, a.shape[0], 7)]))


def workload(name, P, Q, k, rounds, host_rows, out):
    rows, d = P.shape
    rows_host = P.cpu().numpy() if host_rows else None
    rows_dev = None if host_rows else P
    del P
    rec = {m: dict(attach=[], search=[], resident=[], peak=[], stats=None) for m in ("fp32", "fp16")}
    last = {}
    for _ in range(rounds):
        live = {}
        for mode in ("fp32", "fp16"):                              # A B: both attached, then searched one after the other
            index, dt, res, peak = attach(rows_host, rows_dev, mode == "fp16")
            rec[mode]["attach"].append(dt), rec[mode]["resident"].append(res), rec[mode]["peak"].append(peak)
            live[mode] = index
        for mode in ("fp32", "fp16"):
            dt, D, I, st = timed_search(live[mode], Q, k)
            rec[mode]["search"].append(dt)
            rec[mode]["stats"] = st
            last[mode] = I
        del live, index
    out.append(f"== {name}: {rows} x {d} rows ({'host array -> to_gpu' if host_rows else 'device rows -> from_device_rows'}), {Q.shape[0]} queries, k = {k}, {rounds} rounds (A B A B) ==")
    for mode in ("fp32", "fp16"):
        r, st = rec[mode], rec[mode]["stats"]
        out.append(f"{mode:5s} resident {statistics.median(r['resident']) / MB:9.1f} MB ({statistics.median(r['resident']) / (rows * d):.2f} B/element)  "
                   f"attach peak {statistics.median(r['peak']) / MB:9.1f} MB  attach {statistics.median(r['attach']):6.3f} s  "
                   f"search median {statistics.median(r['search']):.4f} s (rounds: {' '.join(f'{x:.4f}' for x in r['search'])})")
        out.append(f"      rescored {st['rescored']} rows ({st['rescored'] / Q.shape[0]:.0f} / query), candidates {st['candidates'] / Q.shape[0]:.0f} / query, scans {st['scans']} "
                   f"rescans {st['rescans']} unproven first pass {st['unproven_first_pass']} fallback queries {st['fallback_queries']}, "
                   f"pipeline {st['search_ms']:.1f} ms (HIP events)")
    a, b = statistics.median(rec["fp32"]["search"]), statistics.median(rec["fp16"]["search"])
    out.append(f"search fp16-row / fp32: {b / a:.3f} ({(b / a - 1) * 100:+.1f} %)   resident fp32 / fp16-row: "
               f"{statistics.median(rec['fp32']['resident']) / statistics.median(rec['fp16']['resident']):.2f}")
    out.append("overlap of the two modes' results (every 7th query): " + "  ".join(f"top-{kk} {overlap(last['fp32'], last['fp16'], kk):.4f}" for kk in (10, 100, 1000) if kk <= k))
    out.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=1105228)
    ap.add_argument("--queries", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also the whole 8 841 823-row collection on one GPU (device rows)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "index_fp16_timing.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    RU.cap_host_threads()
    out = ["command: python tools/time_index_fp16.py " + " ".join(sys.argv[1:]),
           f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; attach chunk {RU.ATTACH_CHUNK_ROWS} rows", ""]
    d = 768
    P, Q = isotropic(args.rows, d, 1234)
    workload("isotropic (bench.py retrieve leg)", P, Q[:args.queries], args.k, args.rounds, True, out)
    del P
    P, u = syn.cls_like_corpus(args.rows, d, 777, DEV)
    Qc = syn.cls_like_queries(args.queries, u, 778)
    workload("CLS-like (bench.py retrieve leg, cls_like)", P, Qc, args.k, args.rounds, True, out)
    del P
    if args.full:
        torch.cuda.empty_cache()
        try:
            P, Q = isotropic(8841823, d, 1234)
            workload("isotropic, whole collection", P, Q[:args.queries], args.k, args.rounds, False, out)
            del P
        except torch.cuda.OutOfMemoryError as exc:
            out.append(f"== isotropic, whole collection: not measured, the device memory does not hold both modes side by side ({exc}) ==".replace("\n", " "))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
