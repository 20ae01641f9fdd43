#!/usr/bin/env python3
"""Cost of building a curriculum training file (dataset.curriculum_file) at training-set scale: a synthetic teacher-scored run of
503 k queries x top-200 (the MS MARCO training queries) is written by the native run-file writer (``write_run_file`` with arrays, as
``rerank_top_passages`` writes it), then the builder is timed in its three phases: parse (``read_teacher_run``), select
(``select_examples``: grouping, teacher order, duplicate check, sampling) and write (``write_examples``).  Host only, no GPU.

    python tools/time_curriculum_file.py [--queries 503000] [--per_query 200] [--label_mode 9] [--work_dir DIR] [--out FILE]
"""
import argparse
import os
import platform
import resource
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def synthetic_run(path, n_q, k, seed=3):
    """n_q queries (distinct qids of the MS MARCO training range) x k distinct pids each, fp32 scores descending per query."""
    from cldrd_amd.retriever.retrieve_top_passages import write_run_file
    rng = np.random.default_rng(seed)
    qids = np.sort(rng.choice(1_200_000, n_q, replace=False)).astype(np.int64)
    rng.shuffle(qids)
    pids = (qids[:, None] * 7919 + np.arange(k, dtype=np.int64)[None, :] * 44207) % 8_841_823      # distinct within a row (44207 k < 8.8 M)
    scores = -np.sort(rng.standard_normal((n_q, k)).astype(np.float32), axis=1)
    return write_run_file(path, qids.tolist(), pids, np.ascontiguousarray(scores))


def host_name():
    model = platform.processor() or platform.machine()
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return f"{model}, {os.cpu_count()} CPUs, {os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES') / 2 ** 30:.0f} GiB"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--queries", type=int, default=503_000)
    ap.add_argument("--per_query", type=int, default=200)
    ap.add_argument("--label_mode", default="9")
    ap.add_argument("--work_dir", default=None, help="where the synthetic run and the output go (deleted afterwards; default: a temp dir)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cldrd_amd  # noqa: F401
    from cldrd_amd.dataset import curriculum_file as C
    spec = C.curriculum_spec(a.label_mode)
    lines = []
    with tempfile.TemporaryDirectory(dir=a.work_dir) as tmp:
        run_path, out_path = os.path.join(tmp, "teacher.run"), os.path.join(tmp, "train.json")
        t0 = time.perf_counter()
        n_pairs = synthetic_run(run_path, a.queries, a.per_query)
        t_gen = time.perf_counter() - t0
        size = os.path.getsize(run_path)
        t = [time.perf_counter()]
        run = C.read_teacher_run(run_path)
        t.append(time.perf_counter())
        ex = C.select_examples(run, spec, seed=0)
        t.append(time.perf_counter())
        n = C.write_examples(out_path, ex)
        t.append(time.perf_counter())
        out_size = os.path.getsize(out_path)
    parse_s, select_s, write_s = np.diff(t)
    total = t[-1] - t[0]
    lines.append(f"command: python tools/time_curriculum_file.py --queries {a.queries} --per_query {a.per_query} --label_mode {a.label_mode}")
    lines.append(f"host: {host_name()}; Python {platform.python_version()}, numpy {np.__version__}; no GPU used")
    lines.append(f"input: {a.queries} queries x {a.per_query} = {n_pairs} pairs, {size / 2 ** 30:.2f} GiB run file "
                 f"(native writer: {t_gen:.1f} s)")
    lines.append(f"label mode {spec.label_mode}: {spec.n_rel} relT, {spec.n_most_hard} most hard from {spec.most_hard_ranks[0]}:"
                 f"{spec.most_hard_ranks[1]}, {spec.n_semi_hard} semi hard from {spec.semi_hard_ranks[0]}:{spec.semi_hard_ranks[1]}; "
                 f"{n} queries written ({out_size / 2 ** 20:.0f} MiB), {ex.n_skipped} skipped")
    lines.append(f"parse  {parse_s:7.1f} s  ({n_pairs / parse_s / 1e6:.2f} M pairs/s)")
    lines.append(f"select {select_s:7.1f} s  ({n_pairs / select_s / 1e6:.2f} M pairs/s)")
    lines.append(f"write  {write_s:7.1f} s  ({n / write_s / 1e3:.0f} k lines/s)")
    lines.append(f"total  {total:7.1f} s; peak resident memory {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GiB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
