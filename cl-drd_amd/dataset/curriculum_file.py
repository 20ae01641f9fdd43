"""Curriculum training files from a teacher-scored candidate run: the step of a CL-DRD iteration between teacher scoring
(``retriever.rerank_top_passages``) and training (``trainer.nway_listwise``).

    python -m cldrd_amd.dataset.curriculum_file --run_path TEACHER.run --label_mode 9 --output_path OUT.json \\
        [--most_hard_ranks 11:100] [--semi_hard_ranks 101:200] [--n_most_hard N] [--seed S] [--with_scores]

Input: ``qid pid rank score`` per line (tabs or spaces; more columns are ignored), what ``rerank_top_passages`` writes.  A line with
fewer than 4 columns and a ``(qid, pid)`` pair that occurs twice are errors.  Within a query the teacher order is score descending, ties
by the rank column ascending, then by line order; queries are taken in the order their qid first appears.

Output: one ``{"qid", "relT_pids", "most_hard_pids", "semi_hard_pids"}`` JSON object per line, integer ids, what
``NwayDataset.create_from_relT_most_semi_hard_file`` and its wrappers read (label modes 2-10; mode 1 reads another format and is refused).
The file stands in for the reference's published ``5relT_25neg.train.json`` / ``10relT_20neg.train.json`` / ... files, whose making
the reference does not ship.  Counts come from the label-mode tables of ``dataset.nway_dataset``:

* ``relT_pids``: the teacher's top ``_REL[mode]`` pids, in teacher order;
* negatives: ``len(_NEG[mode])`` pids, ``most_hard_pids`` first.  By default ``most_hard_pids`` gets as many as the first run of equal
  labels in ``_NEG[mode]`` (mode 8: 12 / 13, 9: 10 / 10, 10: 5 / 5, 2 and 4: 10 / 10, 3, 5 and 7: all most-hard, 6: none) and
  ``semi_hard_pids`` the rest; ``n_most_hard`` overrides the split;
* each negative list is sampled uniformly without replacement from a window of teacher ranks (1-based, inclusive), and written in
  teacher order.  Default windows ``n_rel + 1 : 100`` (most hard) and ``101 : 200`` (semi hard) are this project's choice, not the
  reference's (it does not say how its files were cut).  A window must start after ``n_rel``, the two must not overlap, and each must
  hold at least the number drawn from it; otherwise ``ValueError`` before the run is read.

``--with_scores`` adds ``relT_scores``, ``most_hard_scores`` and ``semi_hard_scores``: the run's score of every written pid, parallel to
the pid lists (what ``NwayDataset(..., teacher_scores=True)`` and ``trainer.nway_listwise --distill_loss`` read).  A score is written as
Python prints the float64 parsed from the run, so its float32 cast is the float32 cast of the run's column; a non-finite score in a
written position raises ``ValueError``.  The pids do not depend on the flag, and without it the file is byte for byte what it was.

A query whose list does not reach the end of every window it draws from (nor ``n_rel``) is skipped and counted; no line is padded.

Sampling contract: a query's line is a pure function of the seed and that query's own lines.  Pair ``(qid, pid)`` gets the key
``splitmix64(splitmix64(splitmix64(seed) ^ qid) ^ pid)`` (uint64, wrap-around; ids as two's-complement uint64) and a window yields its
``n`` smallest keys (ties by pid).  So a file built from a subset or a shard of the run has the same lines for those queries as a file
built from the whole run, and shards can be built apart and concatenated.

Host work at training-set scale (503 k queries x top-200, ~100 M pairs): numpy arrays throughout - the run is parsed by ``np.loadtxt``,
grouped and ordered by sorts over the whole array, every window is gathered as one ``[queries, window]`` matrix; only the JSON lines are
formatted per query.  ``tools/time_curriculum_file.py`` times the three phases (profiles/curriculum_file_timing.txt).

:func:`select_examples_device` is the same selection on the search's ids and the teacher's scores while they are still ``[queries, K]``
arrays in HBM (one kernel launch, ``cldrd_curriculum_select``; same examples, bit for bit): what ``retriever.build_stage_file`` uses instead
of a run file (profiles/stage_file_timing.txt).
"""
from __future__ import annotations

import argparse
import json
import os
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .nway_dataset import _NEG, _REL, LABEL_MODES

DEFAULT_WINDOW_END = (100, 200)         # ours: last teacher rank of the most-hard / semi-hard windows

_U64 = np.uint64
_MASK64 = (1 << 64) - 1


def splitmix64(x) -> np.ndarray:
    """splitmix64's output function on every element (uint64 wrap-around arithmetic); ``x``: an integer array (signed values are taken
    as their two's-complement uint64) or a Python int."""
    if isinstance(x, (int, np.integer)):
        z = np.array([int(x) & _MASK64], dtype=_U64)
    else:
        z = np.asarray(x).astype(_U64)
    z = z + _U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


class CurriculumSpec(NamedTuple):
    label_mode: str
    n_rel: int
    n_most_hard: int
    n_semi_hard: int
    most_hard_ranks: Tuple[int, int]
    semi_hard_ranks: Tuple[int, int]

    @property
    def min_candidates(self) -> int:
        """Shortest candidate list a query may have to be written: it reaches n_rel and the end of every window drawn from."""
        return max([self.n_rel] + [hi for (_, hi), n in ((self.most_hard_ranks, self.n_most_hard), (self.semi_hard_ranks, self.n_semi_hard))
                                   if n > 0])


def parse_window(text) -> Tuple[int, int]:
    """``"LO:HI"`` (or a pair) -> (LO, HI): 1-based inclusive teacher ranks."""
    if isinstance(text, str):
        parts = text.split(":")
        if len(parts) != 2:
            raise ValueError(f"a rank window is LO:HI, got {text!r}")
        text = parts
    lo, hi = (int(v) for v in text)
    return lo, hi


def curriculum_spec(label_mode, most_hard_ranks=None, semi_hard_ranks=None, n_most_hard: Optional[int] = None) -> CurriculumSpec:
    """Counts and windows of one label mode; ``ValueError`` for a mode without this file format or windows that cannot be sampled."""
    mode = str(label_mode)
    if mode not in LABEL_MODES:
        raise ValueError(f"label mode {mode!r} is not one of {', '.join(LABEL_MODES)}")
    if mode == "1":
        raise ValueError("label mode 1 reads {qid, rel_pid, neg_pids} files (create_from_json_line_file), not relT / most-hard / "
                         "semi-hard files")
    n_rel, neg = _REL[mode], _NEG[mode]
    if n_most_hard is None:
        n_most_hard = 0
        while n_most_hard < len(neg) and neg[n_most_hard] == neg[0]:
            n_most_hard += 1
    n_most_hard = int(n_most_hard)
    if not 0 <= n_most_hard <= len(neg):
        raise ValueError(f"label mode {mode} has {len(neg)} negatives; n_most_hard={n_most_hard} is not in 0..{len(neg)}")
    n_semi = len(neg) - n_most_hard
    most = parse_window(most_hard_ranks) if most_hard_ranks is not None else (n_rel + 1, DEFAULT_WINDOW_END[0])
    semi = parse_window(semi_hard_ranks) if semi_hard_ranks is not None else (DEFAULT_WINDOW_END[0] + 1, DEFAULT_WINDOW_END[1])
    for name, (lo, hi), n in (("most-hard", most, n_most_hard), ("semi-hard", semi, n_semi)):
        if lo <= n_rel:
            raise ValueError(f"the {name} window {lo}:{hi} overlaps the {n_rel} relT ranks of label mode {mode}: it must start after {n_rel}")
        if hi < lo:
            raise ValueError(f"the {name} window {lo}:{hi} is empty")
        if hi - lo + 1 < n:
            raise ValueError(f"the {name} window {lo}:{hi} holds {hi - lo + 1} ranks, fewer than the {n} pids drawn from it")
    if max(most[0], semi[0]) <= min(most[1], semi[1]):
        raise ValueError(f"the most-hard window {most[0]}:{most[1]} and the semi-hard window {semi[0]}:{semi[1]} overlap")
    return CurriculumSpec(mode, n_rel, n_most_hard, n_semi, most, semi)


class TeacherRun(NamedTuple):
    qid: np.ndarray          # int64 [n], one entry per line
    pid: np.ndarray          # int64 [n]
    rank: np.ndarray         # int64 [n]
    score: np.ndarray        # float64 [n]


def read_teacher_run(path) -> TeacherRun:
    """The ``qid pid rank score`` columns of a run file, in line order."""
    dt = np.dtype([("qid", np.int64), ("pid", np.int64), ("rank", np.int64), ("score", np.float64)])
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # (an empty file)
            a = np.loadtxt(path, dtype=dt, usecols=(0, 1, 2, 3), ndmin=1)
    except ValueError as exc:
        raise ValueError(f"{path}: a teacher-scored run has `qid pid rank score` (4 columns, tabs or spaces) on every line: {exc}") from exc
    return TeacherRun(np.ascontiguousarray(a["qid"]), np.ascontiguousarray(a["pid"]), np.ascontiguousarray(a["rank"]),
                      np.ascontiguousarray(a["score"]))


class CurriculumExamples(NamedTuple):
    qid: np.ndarray          # int64 [m]: the written queries, in order of first appearance
    relT: np.ndarray         # int64 [m, n_rel]
    most_hard: np.ndarray    # int64 [m, n_most_hard]
    semi_hard: np.ndarray    # int64 [m, n_semi_hard]
    n_skipped: int           # queries with fewer than spec.min_candidates candidates
    relT_scores: Optional[np.ndarray] = None         # float64, parallel to relT / most_hard / semi_hard (select_examples(with_scores=True))
    most_hard_scores: Optional[np.ndarray] = None
    semi_hard_scores: Optional[np.ndarray] = None


def select_examples(run: TeacherRun, spec: CurriculumSpec, seed: int = 0, with_scores: bool = False) -> CurriculumExamples:
    """relT / most-hard / semi-hard pids of every query of ``run`` that has at least ``spec.min_candidates`` candidates;
    ``with_scores``: also the run's score of each of them (gathered with the indices of the pids)."""
    from ..retriever.rerank_top_passages import query_groups
    qid, pid = run.qid, run.pid
    if qid.shape[0] == 0:
        e = np.zeros(0, dtype=np.int64)
        f = np.zeros(0, dtype=np.float64)
        sc = (f.reshape(0, spec.n_rel), f.reshape(0, spec.n_most_hard), f.reshape(0, spec.n_semi_hard)) if with_scores else ()
        return CurriculumExamples(e, e.reshape(0, spec.n_rel), e.reshape(0, spec.n_most_hard), e.reshape(0, spec.n_semi_hard), 0, *sc)
    group, n_q = query_groups(qid)
    # duplicate pairs: one int64 code per pair, group * n_pids + pid code (< n^2, no overflow); half the time of a lexsort over
    # (group, pid) at 100 M pairs
    u_pid, p_code = np.unique(pid, return_inverse=True)
    pair = np.sort(group * u_pid.shape[0] + p_code.reshape(-1))
    dup = np.flatnonzero(pair[1:] == pair[:-1])
    if dup.shape[0]:
        g, p = divmod(int(pair[dup[0]]), u_pid.shape[0])
        raise ValueError(f"the run holds the pair (qid {qid[np.argmax(group == g)]}, pid {u_pid[p]}) more than once")
    del u_pid, p_code, pair
    # teacher order: query (first appearance), score descending, rank ascending, line order (lexsort is stable)
    order = np.lexsort((run.rank, -run.score, group))
    pid_t = pid[order]
    score_t = run.score[order] if with_scores else None
    counts = np.bincount(group, minlength=n_q)
    starts = np.zeros(n_q + 1, dtype=np.int64)
    np.cumsum(counts, out=starts[1:])
    q_ids = qid[order[starts[:-1]]]
    del order
    keep = counts >= spec.min_candidates
    first = starts[:-1][keep]
    q_ids = q_ids[keep]
    q_key = splitmix64(splitmix64(seed) ^ q_ids.astype(_U64))

    def sample(window, n):
        if n == 0:
            return np.zeros((first.shape[0], 0), dtype=np.int64), (np.zeros((first.shape[0], 0), dtype=np.float64) if with_scores else None)
        lo, hi = window
        at = first[:, None] + np.arange(lo - 1, hi)
        cand = pid_t[at]                                                           # [m, hi - lo + 1], teacher order
        key = splitmix64(q_key[:, None] ^ cand.astype(_U64))
        pick = np.lexsort((cand, key), axis=-1)[:, :n]                             # n smallest keys, ties by pid
        pick.sort(axis=1)                                                          # back to teacher order
        return np.take_along_axis(cand, pick, axis=1), (np.take_along_axis(score_t[at], pick, axis=1) if with_scores else None)

    at_rel = first[:, None] + np.arange(spec.n_rel)
    relT = pid_t[at_rel]
    most, most_s = sample(spec.most_hard_ranks, spec.n_most_hard)
    semi, semi_s = sample(spec.semi_hard_ranks, spec.n_semi_hard)
    if not with_scores:
        return CurriculumExamples(q_ids, relT, most, semi, int(n_q - first.shape[0]))
    relT_s = score_t[at_rel]
    bad = ~(np.isfinite(relT_s).all(axis=1) & np.isfinite(most_s).all(axis=1) & np.isfinite(semi_s).all(axis=1))
    if bad.any():
        raise ValueError(f"qid {int(q_ids[np.argmax(bad)])}: the run has a non-finite teacher score for a selected passage")
    return CurriculumExamples(q_ids, relT, most, semi, int(n_q - first.shape[0]), relT_s, most_s, semi_s)


DEVICE_MAX_K = 1024                     # candidates per query the selection kernel holds in LDS (cldrd_curriculum_select)


def select_examples_device(qid, pid, score, count, spec: CurriculumSpec, seed: int = 0, with_scores: bool = False):
    """:func:`select_examples` on what the GPU already holds: ``qid`` int64 [nq], ``pid`` int64 [nq, K] (candidates in run order), ``score``
    fp32 [nq, K] (the teacher's) and ``count`` int32 [nq] (live candidates per row; entries behind them are never read), all device tensors.

    Returns ``(examples, order)``.  ``examples`` is what :func:`select_examples` returns for the equivalent :class:`TeacherRun` - row q
    contributes the lines ``qid[q]  pid[q, j]  j + 1  float64(score[q, j])`` for j < count[q], rows in order: queries in row order, int64 /
    float64 arrays, scores the float64 of the fp32 values, ``n_skipped`` the rows with at least one and fewer than
    ``spec.min_candidates`` candidates (a row without a candidate has no line in that run and is not counted there either).
    ``order`` (device int32 [nq, K]): ``order[q, r]`` = run position of the candidate at teacher rank r, -1 at r >= count[q] - the host
    lexsort of that run, row by row.

    One kernel launch (``cldrd_curriculum_select``: one workgroup per query) and one device-to-host copy of the kept rows.  ``K > 1024``
    does not fit the kernel: the run is built from the arrays and goes through :func:`select_examples` (slow, no limit).

    The rows must have distinct qids and each row's live pids must be distinct (:func:`select_examples` raises on a repeated pair; this
    function does not look).  ``ValueError`` naming the first such qid when a live score is not finite."""
    import torch
    from .. import hip_ops as ops
    for t, name in ((qid, "qid"), (pid, "pid"), (score, "score"), (count, "count")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"select_examples_device: {name} must be a tensor on the GPU (select_examples is the host path)")
    if pid.dim() != 2 or score.shape != pid.shape or qid.shape != pid.shape[:1] or count.shape != pid.shape[:1]:
        raise ValueError("select_examples_device: qid [nq], pid [nq, K], score [nq, K], count [nq]")
    nq, K = pid.shape
    e, f = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
    widths = (spec.n_rel, spec.n_most_hard, spec.n_semi_hard)
    if nq == 0 or K == 0:
        sc = tuple(f.reshape(0, w) for w in widths) if with_scores else ()
        return (CurriculumExamples(e, *(e.reshape(0, w) for w in widths), 0, *sc),
                torch.full((nq, K), -1, dtype=torch.int32, device=pid.device))
    live = torch.arange(K, device=pid.device)[None, :] < count[:, None]
    bad = ((~torch.isfinite(score)) & live).any(dim=1)
    if bool(bad.any().item()):
        raise ValueError(f"qid {int(qid[torch.nonzero(bad)[0, 0]].item())}: a non-finite teacher score among the query's candidates")
    if K > DEVICE_MAX_K:
        return _select_examples_arrays(qid, pid, score, count, live, spec, seed, with_scores)
    order, keep, sel_pid, sel_score = ops.curriculum_select(qid, pid, score, count, spec.n_rel, spec.n_most_hard, spec.most_hard_ranks,
                                                            spec.n_semi_hard, spec.semi_hard_ranks, seed)
    rows = torch.nonzero(keep).reshape(-1)
    q_ids = qid.index_select(0, rows).cpu().numpy()
    pids = sel_pid.index_select(0, rows).cpu().numpy()
    n_skipped = int(((count > 0) & (keep == 0)).sum().item())
    cut = np.cumsum(widths)[:2]
    relT, most, semi = (np.ascontiguousarray(a) for a in np.split(pids, cut, axis=1))
    if not with_scores:
        return CurriculumExamples(q_ids, relT, most, semi, n_skipped), order
    scores = sel_score.index_select(0, rows).cpu().numpy().astype(np.float64)
    relT_s, most_s, semi_s = (np.ascontiguousarray(a) for a in np.split(scores, cut, axis=1))
    return CurriculumExamples(q_ids, relT, most, semi, n_skipped, relT_s, most_s, semi_s), order


def _select_examples_arrays(qid, pid, score, count, live, spec, seed, with_scores):
    """The ``K > DEVICE_MAX_K`` path of :func:`select_examples_device`: the equivalent :class:`TeacherRun` on the host."""
    import torch
    nq, K = pid.shape
    live_h = live.cpu().numpy()
    counts = live_h.sum(axis=1)
    at_q, at_j = np.nonzero(live_h)                                                # row-major: rows in order, run order inside
    run = TeacherRun(np.repeat(qid.cpu().numpy(), counts), pid.cpu().numpy()[at_q, at_j], at_j.astype(np.int64) + 1,
                     score.cpu().numpy()[at_q, at_j].astype(np.float64))
    if np.unique(run.qid).shape[0] != int((counts > 0).sum()):
        raise ValueError("select_examples_device: the rows must have distinct qids")
    ex = select_examples(run, spec, seed, with_scores=with_scores)
    starts = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(counts, out=starts[1:])
    line = np.lexsort((run.rank, -run.score, at_q))                                # the teacher order select_examples used
    order = np.full((nq, K), -1, dtype=np.int32)
    order[at_q, at_j] = (line - starts[at_q]).astype(np.int32)                     # lines of a row stay inside the row's span
    return ex, torch.from_numpy(order).to(pid.device)


def write_examples(path, ex: CurriculumExamples, chunk: int = 65536, with_scores: bool = False) -> int:
    """One JSON object per query; written under a temporary name next to ``path`` and renamed into place.  Returns the line count.
    ``with_scores``: each line also gets ``relT_scores`` / ``most_hard_scores`` / ``semi_hard_scores`` (``ex`` must carry them)."""
    if with_scores and (ex.relT_scores is None or ex.most_hard_scores is None or ex.semi_hard_scores is None):
        raise ValueError("write_examples(with_scores=True) needs examples selected with with_scores=True")
    path = str(path)
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    tmp = os.path.join(parent, f".{os.path.basename(path)}.tmp{os.getpid()}")
    try:
        with open(tmp, "w") as fh:
            for a in range(0, ex.qid.shape[0], chunk):
                b = a + chunk
                if with_scores:
                    fh.write("".join(json.dumps({"qid": q, "relT_pids": r, "most_hard_pids": m, "semi_hard_pids": s, "relT_scores": rs,
                                                 "most_hard_scores": ms, "semi_hard_scores": ss}) + "\n"
                                     for q, r, m, s, rs, ms, ss in zip(ex.qid[a:b].tolist(), ex.relT[a:b].tolist(), ex.most_hard[a:b].tolist(),
                                                                       ex.semi_hard[a:b].tolist(), ex.relT_scores[a:b].tolist(),
                                                                       ex.most_hard_scores[a:b].tolist(), ex.semi_hard_scores[a:b].tolist())))
                    continue
                fh.write("".join(json.dumps({"qid": q, "relT_pids": r, "most_hard_pids": m, "semi_hard_pids": s}) + "\n"
                                 for q, r, m, s in zip(ex.qid[a:b].tolist(), ex.relT[a:b].tolist(), ex.most_hard[a:b].tolist(),
                                                       ex.semi_hard[a:b].tolist())))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return int(ex.qid.shape[0])


def build_curriculum_file(run_path, output_path, label_mode, most_hard_ranks=None, semi_hard_ranks=None,
                          n_most_hard: Optional[int] = None, seed: int = 0, with_scores: bool = False) -> Tuple[int, int]:
    """Teacher-scored run -> training file of ``label_mode`` (``with_scores``: with the teacher's score of every written pid).
    Returns (queries written, queries skipped)."""
    spec = curriculum_spec(label_mode, most_hard_ranks, semi_hard_ranks, n_most_hard)
    ex = select_examples(read_teacher_run(run_path), spec, seed, with_scores=with_scores)
    return write_examples(output_path, ex, with_scores=with_scores), ex.n_skipped


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="cut a teacher-scored run (qid pid rank score) into a curriculum training file "
                                             "({qid, relT_pids, most_hard_pids, semi_hard_pids} per line) for one label mode")
    ap.add_argument("--run_path", required=True, help="qid pid rank score per line, e.g. the output of retriever.rerank_top_passages")
    ap.add_argument("--label_mode", required=True, help="2-10: relT / negative counts from dataset.nway_dataset (mode 1 uses another format)")
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--most_hard_ranks", default=None, type=parse_window,
                    help="LO:HI, 1-based inclusive teacher ranks the most-hard negatives are drawn from (default n_rel+1:100; "
                         "this project's choice, not the reference's)")
    ap.add_argument("--semi_hard_ranks", default=None, type=parse_window,
                    help="LO:HI for the semi-hard negatives (default 101:200; this project's choice, not the reference's)")
    ap.add_argument("--n_most_hard", default=None, type=int,
                    help="negatives drawn from the most-hard window, the rest from the semi-hard one (default: the label mode's first "
                         "run of equal negative labels)")
    ap.add_argument("--seed", default=0, type=int, help="sampling seed; a query's line depends only on it and that query's own lines")
    ap.add_argument("--with_scores", action="store_true", default=False,
                    help="also write relT_scores / most_hard_scores / semi_hard_scores: the run's score of every written pid "
                         "(what trainer.nway_listwise --distill_loss trains on)")
    return ap.parse_args(argv)


def main(args):
    n, skipped = build_curriculum_file(args.run_path, args.output_path, args.label_mode, args.most_hard_ranks, args.semi_hard_ranks,
                                       args.n_most_hard, args.seed, with_scores=getattr(args, "with_scores", False))
    need = curriculum_spec(args.label_mode, args.most_hard_ranks, args.semi_hard_ranks, args.n_most_hard).min_candidates
    print(f"wrote {n} queries to {args.output_path}; skipped {skipped} with fewer than {need} candidates")
    return n, skipped


if __name__ == "__main__":
    main(get_args())
