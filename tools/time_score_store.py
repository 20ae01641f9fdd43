#!/usr/bin/env python3
"""Cost of the teacher score store (``retriever.score_store``) at training-set scale: 503 k queries x top-200 = 100.6 M pairs on synthetic
ids (distinct qids, distinct pids within a row), a store of that many entries.  Beside each figure the same operation in host numpy on the
pair key ``qid * 2^25 + pid`` (the synthetic ids fit it).  No teacher runs here: scoring 100 M pairs is about 35 GPU-minutes, which is what
a hit saves.

  append    one flush chunk (``--flush_pairs``, default 2^23) into an empty store: two stable ``torch.sort``, gather, duplicate check, copy to the
            host, three ``.npy`` files with fsync, ``meta.json``; host: ``np.lexsort`` of the chunk
  lookup    the whole batch against the store as TWO segments of ~50 M and, after the compaction, as ONE of 100.6 M, at hit rates 0, 0.5 and 1
            (HIP events); host: ``np.searchsorted`` of the batch's keys in the sorted key array, at hit rate 0.5
  compact   two ~50 M segments whose keys interleave: ``cldrd_pair_merge`` alone (HIP events) and ``compact()`` as a whole (merge, copy to
            the host, file write, commit, removal of the old files); host: ``np.lexsort`` of the concatenation
  open      close and re-open: read the ``.npy`` files, upload, order check on the device - for the two-segment and the one-segment store;
            host: ``np.load`` and the same order check in numpy

    python tools/time_score_store.py [--queries 503000] [--per_query 200] [--flush_pairs 8388608] [--work_dir DIR] [--out FILE]"""
import argparse
import os
import platform
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from time_curriculum_file import host_name

IDENTITY = {"teacher_sha256": "synthetic", "num_labels": 1, "max_len": 256, "arithmetic": "fp16"}
N_PASSAGES = 8_841_823


def device_pairs(n_q, k, seed=3):
    """row qid int64 [n_q] (distinct, the MS MARCO training range), pid int64 [n_q * k] (distinct within a row: 44207 k < 8.8 M), score fp32"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    qid = torch.randperm(max(1_200_000, n_q), device="cuda", generator=g)[:n_q].contiguous()
    pid = ((qid[:, None] * 7919 + torch.arange(k, device="cuda")[None, :] * 44207) % N_PASSAGES).reshape(-1).contiguous()
    return qid, pid, torch.randn(n_q * k, device="cuda", generator=g)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


REPS = 10


class Span:
    """seconds of REPS runs after a warm-up run, each between two HIP events: mean, least and most"""

    def __init__(self, ms):
        self.mean, self.lo, self.hi = sum(ms) / len(ms) / 1e3, min(ms) / 1e3, max(ms) / 1e3

    def __str__(self):
        return f"{self.mean:9.4f} s (mean of {REPS} runs after a warm-up run, {self.lo:.4f} .. {self.hi:.4f})"


def by_events(fn):
    out = fn()
    ms = []
    for _ in range(REPS):
        del out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, Span(ms)


def dir_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--queries", type=int, default=503_000)
    ap.add_argument("--per_query", type=int, default=200)
    ap.add_argument("--flush_pairs", type=int, default=1 << 23)
    ap.add_argument("--work_dir", default=None, help="where the stores go (deleted afterwards; default: a temp dir)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cldrd_amd  # noqa: F401
    from cldrd_amd import hip_ops as ops
    from cldrd_amd.retriever.score_store import TeacherScoreStore
    nq, k = a.queries, a.per_query
    n = nq * k
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"command: python tools/time_score_store.py --queries {nq} --per_query {k} --flush_pairs {a.flush_pairs}")
    prop = torch.cuda.get_device_properties(0)
    say(f"box: {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB); host "
        f"{host_name()}, {torch.get_num_threads()} torch threads; Python {platform.python_version()}, numpy {np.__version__}, torch {torch.__version__}")
    say(f"data: {nq} queries x {k} = {n} pairs generated on the device")
    row_qid, pid, score = device_pairs(nq, k)
    starts = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * k
    qid_pp = torch.repeat_interleave(row_qid, k)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory(dir=a.work_dir) as tmp:
        # ---- append of one flush chunk
        say("-- append of one flush chunk into an empty store")
        m = min(a.flush_pairs, n)
        at = torch.randperm(n, device="cuda")[:m]
        cq, cp, cs = qid_pp[at], pid[at], score[at]
        store = TeacherScoreStore(os.path.join(tmp, "chunk"), IDENTITY, "cuda")
        store.append(cq[:4096], cp[:4096], cs[:4096])                  # warm-up: torch's lazily loaded sort kernels
        _, t_sort = timed(lambda: torch.sort(cq[torch.sort(cp, stable=True).indices], stable=True))
        _, t_app = timed(lambda: store.append(cq[4096:], cp[4096:], cs[4096:]))
        store.close()
        say(f"append of {m - 4096} pairs (sort, duplicate check, copy to the host, 3 .npy files of {(m - 4096) * 20 / 2 ** 20:.0f} MiB with fsync, meta.json) "
            f"{t_app:9.3f} s; the two stable torch.sort alone {t_sort:9.3f} s")
        hq, hp = cq.cpu().numpy(), cp.cpu().numpy()
        t0 = time.perf_counter()
        order = np.lexsort((hp, hq))
        hq, hp = hq[order], hp[order]
        say(f"host: np.lexsort((pid, qid)) of the chunk and the two gathers {time.perf_counter() - t0:9.3f} s")
        del cq, cp, cs, hq, hp, order, at

        # ---- the store: two segments whose keys interleave
        side = torch.rand(n, device="cuda") < 0.5
        path = os.path.join(tmp, "store")
        store = TeacherScoreStore(path, IDENTITY, "cuda")
        for half in (side, ~side):
            _, t = timed(lambda: store.append(qid_pp[half], pid[half], score[half]))
            say(f"(setup: append of {int(half.sum())} pairs as one segment {t:.2f} s)")
        del side

        def lookups(tag):
            for rate in (0.0, 0.5, 1.0):
                probe = pid if rate == 1.0 else torch.where(torch.rand(n, device="cuda") < rate, pid, pid + N_PASSAGES)
                (s, hit), t = by_events(lambda: store.lookup(row_qid, starts, probe))
                hits = int(hit.sum())
                if rate == 1.0 and not torch.equal(s.view(torch.int32), score.view(torch.int32)):
                    raise SystemExit("lookup returned other bits than were stored")
                say(f"lookup of {n} pairs, {tag}, hit rate {rate:.1f} ({hits} hits; two zero fills and {len(store.segments)} launch(es)) {t}  "
                    f"({n / t.mean / 1e6:.0f} M pairs/s)")
                del probe, s, hit

        def reopen(tag):
            nonlocal store
            store.close(compact=False)
            t0 = time.perf_counter()
            store = TeacherScoreStore(path, IDENTITY, "cuda")
            torch.cuda.synchronize()
            say(f"open, {tag} ({dir_bytes(path) / 2 ** 30:.2f} GiB: np.load, upload, order check on the device) {time.perf_counter() - t0:9.3f} s")
            t0 = time.perf_counter()
            for name, _, _, _ in store.segments:
                q, p, _ = (np.load(os.path.join(path, f"{name}.{part}.npy")) for part in "qps")
                if not ((q[1:] > q[:-1]) | ((q[1:] == q[:-1]) & (p[1:] > p[:-1]))).all():
                    raise SystemExit("order check failed on the host")
            say(f"host: np.load and the same order check in numpy {time.perf_counter() - t0:9.3f} s")

        say("-- open and lookup, two segments")
        reopen("two segments")
        lookups("two segments")

        # ---- compaction
        say("-- compaction of the two segments")
        (_, aq, ap_, as_), (_, bq, bp, bs) = store.segments
        _, t_merge = by_events(lambda: ops.pair_merge(aq, ap_, as_, bq, bp, bs))
        say(f"cldrd_pair_merge alone, {aq.shape[0]} + {bq.shape[0]} entries (output allocation and flag read included) "
            f"{t_merge}  ({n / t_merge.mean / 1e6:.0f} M entries/s)")
        hq, hp = torch.cat([aq, bq]).cpu().numpy(), torch.cat([ap_, bp]).cpu().numpy()
        del aq, ap_, as_, bq, bp, bs
        _, t_c = timed(store.compact)
        say(f"compact() as a whole (merge, copy to the host, 3 .npy files of {n * 20 / 2 ** 30:.2f} GiB with fsync, commit, removal of the old files) {t_c:9.3f} s")
        t0 = time.perf_counter()
        order = np.lexsort((hp, hq))
        say(f"host: np.lexsort((pid, qid)) of the concatenation (order only, no gather) {time.perf_counter() - t0:9.3f} s")
        hkey = (hq * (1 << 25) + hp)[order]
        del hq, hp, order
        _, sq, sp, ss = store.segments[0]
        if not (torch.equal(sq * (1 << 25) + sp, torch.from_numpy(hkey).cuda())):
            raise SystemExit("the compacted segment is not the lexsorted union")

        say("-- open and lookup, one segment")
        reopen("one segment")
        lookups("one segment")
        probe = torch.where(torch.rand(n, device="cuda") < 0.5, pid, pid + N_PASSAGES)
        want = (qid_pp * (1 << 25) + probe).cpu().numpy()
        t0 = time.perf_counter()
        pos = np.minimum(np.searchsorted(hkey, want), hkey.shape[0] - 1)
        hit_h = hkey[pos] == want
        say(f"host: np.searchsorted of the {n} pair keys in the sorted key array, hit rate 0.5, and the equality check {time.perf_counter() - t0:9.3f} s")
        _, hit = store.lookup(row_qid, starts, probe)
        if not np.array_equal(hit.cpu().numpy().astype(bool), hit_h):
            raise SystemExit("device and host lookups disagree")
        say("device and host lookups agree on every pair")
        store.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
