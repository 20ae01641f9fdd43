"""Re-rank a dev run with the student (or a cross-encoder) and score the result against qrels: ``evaluation/reranking_evaluator.py`` of the
reference (``RerankingEvaluator``, :25-273) - what its trainers import and its launch scripts' ``--dev_path`` / ``--dev_queries_path`` /
``--dev_qrels_path`` feed, to choose the checkpoint the next curriculum stage starts from.

Same call surface (``compute_metrics(model, dataloader, ...)``, ``direct_compute_metric(qid_to_ranklist, ...)``) and the metric semantics
of its ``_calculate_metrics_plain`` (:121-248), quirks included:

* qrels lines ``qid _ pid grade`` split on tab (dev) or single space (``is_trec``); grades <= 1e-5 are dropped;
* the binarisation point is 1.0 for both qrels kinds (the reference never passes another one here, unlike its ``RankingEvaluator``);
* ``Recall@k`` is reported at the ``mrr_at_k`` cut-offs (``recall_at_k`` only sizes the per-query tables and names the CSV columns);
* ``QueriesWithNoRelevant@k`` counts every ranked query whose reciprocal rank is 0 - queries without qrels too - while ``QueriesRanked``
  and every mean count only the queries that have qrels;
* the per-query tables have ``len(recall_at_k)`` rows, so ``len(mrr_at_k) > len(recall_at_k)`` is an IndexError in the reference: here a
  ValueError in the constructor;
* the key order of the returned dict.

Differences: ``output_rerank_path`` writes ``qid\\tpid\\trank\\tscore`` with ``write_run_file`` (the reference calls an undefined
``write_rankdata``); a ``(qid, pid)`` pair that occurs twice is scored once (its first occurrence, as ``read_run`` keeps it); inside a query
the order is score descending, ties in run order; a student's score is the exact re-score of the flat search (``dev_pool``: fp64
accumulated, rounded once) in both paths, never a second summation order.

``compute_metrics`` with a dataloader of ``RerankingDataset.collate_fn`` batches is the compatibility path; ``compute_metrics_pool`` takes a
:class:`~cldrd_amd.evaluation.dev_pool.DevPool` (tokenised once, every distinct query and passage encoded once) and is what the trainer
and the command lines use.  Both run under ``torch.no_grad()`` in eval mode, honour ``model.eval_fp32``, and leave the model's
training / eval flags and the towers' dropout step counters as they found them.

Pinned against the reference on the committed fixture: tests/test_dev_validation_host.py."""
from __future__ import annotations

import contextlib
import csv
import json
import os
import time
from typing import Dict, List

import numpy as np
import torch

from .. import hip_ops as ops
from ..retriever.rerank_top_passages import group_pairs, rank_order, write_ranked_run
from .dev_pool import DevPool, rescore_chunks

BEST_METRIC = "MRR@10"


@contextlib.contextmanager
def evaluation_state(model):
    """eval mode and no_grad for the duration; afterwards every module has the training flag it had and every tower the dropout step
    counter it had (an evaluation encode draws a seed it never uses) - a training run goes on as if nothing had been evaluated."""
    flags = [(m, m.training) for m in model.modules()]
    seeds = [(m, m.step_seed) for m, _ in flags if hasattr(m, "step_seed")]
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m, f in flags:
            m.training = f
        for m, s in seeds:
            m.step_seed = s


def _require_gpu(model):
    p = next(model.parameters(), None)
    if p is None or p.device.type != "cuda":
        raise RuntimeError("RerankingEvaluator needs the model on a GPU (no CPU path): move it with .cuda() first")
    return p.device


def _to_device(v, dev):
    if isinstance(v, torch.Tensor):
        return v.to(dev, non_blocking=True)
    if hasattr(v, "items"):
        return {k: _to_device(x, dev) if k != "lengths" else x for k, x in v.items()}
    return v


class RerankingEvaluator:
    def __init__(self, qrel_path: str, mrr_at_k: List[int] = [10, 100], ndcg_at_k: List[int] = [10, 100], recall_at_k: List[int] = [10, 100],
                 save_to_csv: bool = True, show_progress_bar: bool = False, is_trec: bool = False):
        self.mrr_at_k, self.ndcg_at_k, self.recall_at_k = list(mrr_at_k), list(ndcg_at_k), list(recall_at_k)
        if len(self.mrr_at_k) > len(self.recall_at_k):
            raise ValueError(f"mrr_at_k {self.mrr_at_k} has more cut-offs than recall_at_k {self.recall_at_k}: the per-query tables have one row "
                             "per recall_at_k entry (the reference fails with an IndexError here)")
        self.qid_to_relevant_data: Dict[int, Dict[int, float]] = {}
        sep = " " if is_trec else "\t"
        with open(qrel_path, "r") as fh:
            for line in fh:
                qid, _, pid, grade = line.strip().split(sep)
                if float(grade) <= 0.00001:
                    continue
                self.qid_to_relevant_data.setdefault(int(qid), {})[int(pid)] = float(grade)
        if save_to_csv:
            self.csv_file = "evluation_result.csv"            # (sic) the reference's attributes; nothing writes the file there either
            self.csv_header = ["epoch", "steps"] + [f"mrr@{k}" for k in self.mrr_at_k] + [f"ndcg@{k}" for k in self.ndcg_at_k]
        self.show_progress_bar = show_progress_bar
        self.is_trec = is_trec
        self.last_timings = {}

    # ---- scoring ------------------------------------------------------------------------------------------------------------
    def compute_metrics(self, model, dataloader, output_rerank_path=None, return_per_query=False, per_query_metrics_path=None,
                        is_cross_encoder=False):
        """The reference's loop over ``RerankingDataset.collate_fn`` batches (``query`` / ``passage``, or ``query_passage`` scored by a
        :class:`~cldrd_amd.models.cross_encoder.CrossEncoder` with ``is_cross_encoder``)."""
        dev = _require_gpu(model)
        qids, pids, scores = [], [], []
        with evaluation_state(model):
            for batch in dataloader:
                if is_cross_encoder:
                    s = model.scores(model(_to_device(batch["query_passage"], dev))).float()
                else:
                    q = model.query_embs(_to_device(batch["query"], dev)).float().contiguous()
                    p = model.passage_embs(_to_device(batch["passage"], dev)).float().contiguous()
                    # pair b = (query row b, passage row b): the exact re-score with one candidate per query
                    n = q.shape[0]
                    s = torch.zeros(n, 1, dtype=torch.float32, device=dev)
                    ones = torch.ones(n, dtype=torch.int32, device=dev)
                    rows = torch.arange(n, dtype=torch.int32, device=dev).view(n, 1)
                    for a, b in rescore_chunks(n):
                        ops.topk_rescore(q[a:b], p, ones[a:b], rows[a:b], s[a:b])
                scores.append(s.reshape(-1).cpu().numpy())
                qids.extend(int(v) for v in batch["qid"])
                pids.extend(int(v) for v in batch["pid"])
        qids, pids = np.asarray(qids, dtype=np.int64), np.asarray(pids, dtype=np.int64)
        scores = np.concatenate(scores) if scores else np.zeros(0, dtype=np.float32)
        # one entry per distinct pair (its first occurrence), queries by first appearance, run order inside: what read_run keeps
        qids, pids, group, starts, src = group_pairs(qids, pids)
        return self._finish(qids, pids, group, starts, scores[src], output_rerank_path, return_per_query, per_query_metrics_path)

    def compute_metrics_pool(self, model, pool: DevPool, batch_size: int = 512, output_rerank_path=None, return_per_query=False,
                             per_query_metrics_path=None):
        """The fast path: every distinct query and passage of ``pool`` encoded once, the pairs scored on the device, ranked on the host.
        ``last_timings``: seconds of the query encode, the passage encode, the scoring and the ranking + metrics of this call."""
        _require_gpu(model)
        tm = {}
        with evaluation_state(model):
            scores = pool.score(model, batch_size, timings=tm)
        t0 = time.perf_counter()
        out = self._finish(pool.qids, pool.pids, pool.group, pool.starts, scores, output_rerank_path, return_per_query, per_query_metrics_path)
        tm["rank_metrics_s"] = time.perf_counter() - t0
        self.last_timings = tm
        return out

    def _finish(self, qids, pids, group, starts, scores, output_rerank_path, return_per_query, per_query_metrics_path):
        if output_rerank_path is not None:
            write_ranked_run(output_rerank_path, qids, pids, group, starts, scores)
        order = rank_order(group, scores)
        self.last_scores = np.ascontiguousarray(scores[order], dtype=np.float32)          # in output order
        p_list = pids[order].tolist()
        ranking = {int(qids[a]): p_list[a:b] for a, b in zip(starts[:-1], starts[1:])}
        return self.direct_compute_metric(ranking, return_per_query, per_query_metrics_path)

    # ---- metrics ------------------------------------------------------------------------------------------------------------
    def direct_compute_metric(self, qid_to_ranklist, return_per_query=False, per_query_metrics_path=None):
        if not return_per_query:
            return self._calculate_metrics_plain(qid_to_ranklist, self.qid_to_relevant_data)
        local, rr, rec, ndcg, qidx_to_qid, qrels = self._calculate_metrics_plain(qid_to_ranklist, self.qid_to_relevant_data,
                                                                              return_per_query=True)
        if per_query_metrics_path is not None:
            self._output_per_query_metrics(qidx_to_qid, qrels, per_query_metrics_path, rr, rec, ndcg)
        return local, (rr, rec, ndcg)

    def _calculate_metrics_plain(self, ranking, qrels, binarization_point=1.0, return_per_query=False):
        nq = len(ranking)
        qidx_to_qid = dict(enumerate(ranking))
        rr = np.zeros((len(self.recall_at_k), nq))                # sized by recall_at_k, as the reference (:131-133)
        rec = np.zeros((len(self.recall_at_k), nq))
        ndcg = np.zeros((len(self.ndcg_at_k), nq))
        evaluated = 0
        for qi, (qid, docs) in enumerate(ranking.items()):
            if qid not in qrels:
                continue
            evaluated += 1
            rel_ids = np.array(list(qrels[qid].keys()))
            grades = np.array(list(qrels[qid].values()))
            docs = np.array(docs)
            pos = np.arange(1, docs.shape[0] + 1)
            bin_ids = rel_ids[grades >= binarization_point]
            hit = np.isin(docs, bin_ids)
            if hit.any():
                ranks = pos[hit]
                for ci, cutoff in enumerate(self.mrr_at_k):
                    rec[ci, qi] = (ranks <= cutoff).sum(axis=0) / bin_ids.shape[0]        # recall at the MRR cut-offs (:163-169)
                    if ranks[0] <= cutoff:
                        rr[ci, qi] = 1 / ranks[0]
            ghit = np.isin(docs, rel_ids)
            if ghit.any():
                ranks = pos[ghit]
                grade_of = dict(zip(rel_ids.tolist(), grades.tolist()))
                g_at_rank = np.array([grade_of[d] for d in docs[ghit].tolist()])
                ideal = np.sort(grades)[::-1]
                for ci, cutoff in enumerate(self.ndcg_at_k):
                    idcg = ideal[:cutoff] / np.log2(1 + np.arange(1, min(rel_ids.shape[0], cutoff) + 1))
                    # the reference divides every graded hit by log2(1 + rank) with the ranks beyond the cut-off set to 0 and zeroes the
                    # infinities (:199-207): the same array with zeros in those places, summed in the same order
                    inside = ranks <= cutoff
                    dcg = np.zeros(ranks.shape[0])
                    dcg[inside] = g_at_rank[inside] / np.log2(1 + ranks[inside])
                    ndcg[ci, qi] = dcg.sum(axis=-1) / idcg.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            mrr = rr.sum(axis=-1) / evaluated
            relevant = (rr > 0).sum(axis=-1)
            non_relevant = (rr == 0).sum(axis=-1)
            recall = rec.sum(axis=-1) / evaluated
            ndcg_mean = ndcg.sum(axis=-1) / evaluated
        out = {}
        for ci, cutoff in enumerate(self.mrr_at_k):
            out["MRR@" + str(cutoff)] = mrr[ci]
            out["Recall@" + str(cutoff)] = recall[ci]
            out["QueriesWithNoRelevant@" + str(cutoff)] = non_relevant[ci]
            out["QueriesWithRelevant@" + str(cutoff)] = relevant[ci]
        for ci, cutoff in enumerate(self.ndcg_at_k):
            out["nDCG@" + str(cutoff)] = ndcg_mean[ci]
        out["QueriesRanked"] = evaluated
        if return_per_query:
            return out, rr, rec, ndcg, qidx_to_qid, qrels
        return out

    def _output_per_query_metrics(self, qidx_to_qid, qrels, output_path, rr, rec, ndcg):
        with open(output_path, "w") as fh:
            w = csv.writer(fh)
            w.writerow(["query"] + [f"mrr@{k}" for k in self.mrr_at_k] + [f"recall@{k}" for k in self.recall_at_k] +
                       [f"ndcg@{k}" for k in self.ndcg_at_k])
            for qi, qid in qidx_to_qid.items():
                if qid not in qrels:
                    continue
                row = [qid]
                for table in (rr, rec, ndcg):
                    row += ["{:.3f}".format(table[d][qi]) for d in range(table.shape[0])]
                w.writerow(row)


# ---- the validation log of a training run (trainer.nway_listwise, evaluation.continue_rerank_evaluator) ------------------------
def write_dev_logs(filename, epoch, step, metrics, seconds):
    """One tab-separated line per validation; the header - ``epoch step`` + the metric keys in dict order + ``seconds`` - once."""
    new = not os.path.exists(filename)
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    with open(filename, "a") as fh:
        if new:
            fh.write("\t".join(["epoch", "step"] + list(metrics) + ["seconds"]) + "\n")
        fh.write("\t".join([str(epoch), str(step)] + [repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v))
                                                      for v in metrics.values()] + [f"{seconds:.3f}"]) + "\n")


def update_dev_best(path, best, metrics, step, epoch, checkpoint):
    """``best`` (None or the dict of an earlier call) against this validation: the highest ``MRR@10`` wins, a tie keeps the earlier step.
    Rewrites ``path`` (atomically) and returns the dict that now holds."""
    value = float(metrics[BEST_METRIC])
    if best is None or value > best["value"]:
        best = {"metric": BEST_METRIC, "value": value, "step": int(step), "epoch": int(epoch), "checkpoint": str(checkpoint)}
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w") as fh:
        json.dump(best, fh)
    os.replace(tmp, path)
    return best
