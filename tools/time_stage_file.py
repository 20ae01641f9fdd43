#!/usr/bin/env python3
"""Cost of the training-data side of a curriculum stage once the GPU holds the search's ids and the teacher's scores, at training-set scale
(503 k queries x top-200 = 100.6 M pairs): the one-job path of ``retriever.build_stage_file`` against the host path of the three programs,
on the same data and the same box.  The data are generated on the device (distinct qids, distinct pids within a row, fp32 scores in run
order); the teacher scoring itself is not part of this (100 M pairs are about 35 GPU-minutes either way).

Parts (``--parts``, comma separated, run in this order):

  device   ``select_examples_device`` (finite check, ``cldrd_curriculum_select``, copy of the selected rows; the kernel also alone, by HIP
           events), the device-to-host copy of ids + scores + order (what the optional run files need), ``write_examples``
  rerank   the host work of ``rerank_top_passages`` around the scoring: the student run is written (native writer, not timed as host-path
           work: ``retrieve_top_passages`` writes it either way), then ``read_run`` and ``write_ranked_run`` are timed
  file     ``dataset.curriculum_file`` on that teacher run in its three phases, as ``tools/time_curriculum_file.py`` times them
           (``read_teacher_run``, ``select_examples``, ``write_examples``); with ``device`` also run, the two training files are compared

    python tools/time_stage_file.py [--queries 503000] [--per_query 200] [--label_mode 9] [--parts device,rerank,file] [--work_dir DIR] [--out FILE]

``--out`` is appended to, so the parts can be run as separate commands into one file."""
import argparse
import os
import platform
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from time_curriculum_file import host_name


def device_data(n_q, k, seed=3):
    """qid int64 [n_q] (distinct, the MS MARCO training range), pid int64 [n_q, k] (distinct within a row: 44207 k < 8.8 M), score fp32
    [n_q, k] in run order, count int32 [n_q] - on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    qid = torch.randperm(max(1_200_000, n_q), device="cuda", generator=g)[:n_q].contiguous()
    pid = (qid[:, None] * 7919 + torch.arange(k, device="cuda")[None, :] * 44207) % 8_841_823
    score = torch.randn(n_q, k, device="cuda", generator=g)
    return qid, pid.contiguous(), score, torch.full((n_q,), k, dtype=torch.int32, device="cuda")


class Heartbeat:
    """a line a minute while a long host phase runs"""
    def __init__(self, what):
        self.what, self.stop = what, threading.Event()

    def __enter__(self):
        t0 = time.perf_counter()

        def beat():
            while not self.stop.wait(60.0):
                print(f"  ... {self.what}: {time.perf_counter() - t0:.0f} s", flush=True)
        self.thread = threading.Thread(target=beat, daemon=True)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()


def timed(what, fn):
    with Heartbeat(what):
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_initialized():
            torch.cuda.synchronize()
        return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--queries", type=int, default=503_000)
    ap.add_argument("--per_query", type=int, default=200)
    ap.add_argument("--label_mode", default="9")
    ap.add_argument("--parts", default="device,rerank,file")
    ap.add_argument("--work_dir", default=None, help="where the run files and the outputs go (deleted afterwards; default: a temp dir)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = [p for p in a.parts.split(",") if p]
    if not parts or set(parts) - {"device", "rerank", "file"}:
        ap.error("--parts: device, rerank, file")
    import cldrd_amd  # noqa: F401
    from cldrd_amd import hip_ops as ops
    from cldrd_amd.dataset import curriculum_file as C
    from cldrd_amd.retriever import rerank_top_passages as R
    from cldrd_amd.retriever.retrieve_top_passages import write_run_file
    spec = C.curriculum_spec(a.label_mode)
    nq, k = a.queries, a.per_query
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"command: python tools/time_stage_file.py --queries {nq} --per_query {k} --label_mode {a.label_mode} --parts {','.join(parts)}")
    prop = torch.cuda.get_device_properties(0)
    say(f"box: {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB); host {host_name()}, {torch.get_num_threads()} torch threads; Python "
        f"{platform.python_version()}, numpy {np.__version__}, torch {torch.__version__}")
    say(f"data: {nq} queries x {k} = {nq * k} pairs generated on the device; label mode {spec.label_mode}: {spec.n_rel} relT, "
        f"{spec.n_most_hard} most hard from {spec.most_hard_ranks[0]}:{spec.most_hard_ranks[1]}, {spec.n_semi_hard} semi hard from "
        f"{spec.semi_hard_ranks[0]}:{spec.semi_hard_ranks[1]}; seed 0, no scores in the training file")
    qid, pid, score, count = device_data(nq, k)
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory(dir=a.work_dir) as tmp:
        dev_json, host_json = os.path.join(tmp, "train.device.json"), os.path.join(tmp, "train.host.json")
        student_run, teacher_run = os.path.join(tmp, "train.student.run"), os.path.join(tmp, "train.teacher.run")
        if "device" in parts:
            say("-- one job (device selection)")
            args = (spec.n_rel, spec.n_most_hard, spec.most_hard_ranks, spec.n_semi_hard, spec.semi_hard_ranks, 0)
            ops.curriculum_select(qid, pid, score, count, *args)           # warm-up: module load, and torch's own lazily loaded kernels
            C.select_examples_device(qid[:64], pid[:64], score[:64], count[:64], spec, seed=0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.curriculum_select(qid, pid, score, count, *args)
            e1.record()
            torch.cuda.synchronize()
            say(f"kernel alone (cldrd_curriculum_select, HIP events, second launch) {e0.elapsed_time(e1) / 1e3:9.4f} s")
            (ex, order), t_sel = timed("select", lambda: C.select_examples_device(qid, pid, score, count, spec, seed=0))
            say(f"select (select_examples_device: finite check, kernel, copy of the selected rows) {t_sel:9.3f} s  "
                f"({nq * k / t_sel / 1e6:.0f} M pairs/s)")
            _, t_d2h = timed("d2h", lambda: (pid.cpu(), score.cpu(), order.cpu()))
            say(f"device-to-host copy of ids + scores + order ({nq * k * 16 / 2 ** 30:.2f} GiB; only the optional run files need it) {t_d2h:9.3f} s")
            n, t_w = timed("write", lambda: C.write_examples(dev_json, ex))
            say(f"write (write_examples: {n} queries, {os.path.getsize(dev_json) / 2 ** 20:.0f} MiB, {ex.n_skipped} skipped) {t_w:9.3f} s")
            say(f"total select + write {t_sel + t_w:9.3f} s")
            del ex, order
        if "rerank" in parts or "file" in parts:
            qid_h, pid_h, score_h = qid.cpu().numpy(), pid.cpu().numpy(), score.cpu().numpy()
            starts = np.arange(nq + 1, dtype=np.int64) * k
            group = np.repeat(np.arange(nq, dtype=np.int64), k)
        if "rerank" in parts:
            say("-- three programs, host work of rerank_top_passages around the scoring")
            _, t_s = timed("student run", lambda: write_run_file(student_run, qid_h.tolist(), pid_h, score_h))
            say(f"(student run written by the native writer: {os.path.getsize(student_run) / 2 ** 30:.2f} GiB, {t_s:.1f} s; both paths pay this when the run is kept)")
            (qids, pids, grp, st), t_r = timed("read_run", lambda: R.read_run(student_run))
            say(f"read_run (np.loadtxt, np.unique over the pairs, grouping) {t_r:9.1f} s  ({nq * k / t_r / 1e6:.2f} M pairs/s)")
            assert np.array_equal(pids, pid_h.reshape(-1)) and np.array_equal(st, starts)
            _, t_wr = timed("write_ranked_run", lambda: R.write_ranked_run(teacher_run, qids, pids, grp, st, score_h.reshape(-1)))
            say(f"write_ranked_run (rank_order's lexsort, native writer; {os.path.getsize(teacher_run) / 2 ** 30:.2f} GiB) {t_wr:9.1f} s")
            say(f"total read_run + write_ranked_run {t_r + t_wr:9.1f} s  (the dict mapping of ids to cache rows in main is not included)")
            del qids, pids, grp, st
        if "file" in parts:
            say("-- three programs, dataset.curriculum_file on the teacher run")
            if not os.path.exists(teacher_run):
                _, t_wr = timed("write_ranked_run", lambda: R.write_ranked_run(teacher_run, np.repeat(qid_h, k), pid_h.reshape(-1), group, starts,
                                                                              score_h.reshape(-1)))
                say(f"(teacher run written by write_ranked_run: {os.path.getsize(teacher_run) / 2 ** 30:.2f} GiB, {t_wr:.1f} s)")
            run, t_p = timed("parse", lambda: C.read_teacher_run(teacher_run))
            say(f"parse  (read_teacher_run) {t_p:9.1f} s  ({nq * k / t_p / 1e6:.2f} M pairs/s)")
            ex, t_s = timed("select", lambda: C.select_examples(run, spec, seed=0))
            say(f"select (select_examples)  {t_s:9.1f} s  ({nq * k / t_s / 1e6:.2f} M pairs/s)")
            n, t_w = timed("write", lambda: C.write_examples(host_json, ex))
            say(f"write  (write_examples: {n} queries, {ex.n_skipped} skipped) {t_w:9.1f} s")
            say(f"total parse + select + write {t_p + t_s + t_w:9.1f} s")
            if os.path.exists(dev_json):
                with open(dev_json, "rb") as f1, open(host_json, "rb") as f2:
                    same = f1.read() == f2.read()
                say(f"the two training files are byte for byte the same: {same}")
                if not same:
                    raise SystemExit("the device selection and the host selection wrote different files")
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
