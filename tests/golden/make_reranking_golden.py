#!/usr/bin/env python3
"""Golden metrics of the reference's ``evaluation/reranking_evaluator.py`` (build container only; IMPORTS THE REFERENCE) through its
``direct_compute_metric`` on the committed ``evaluator_fixture`` qrels and run files (read, not changed): dev (tab) and TREC (space,
graded) qrels, default and custom cut-offs, per-query arrays and CSV files; plus a tiny qrels file with grade-0 lines written here
(``reranking_fixture/``, our own data).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reranking_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "evaluator_fixture")
FIX2 = os.path.join(HERE, "reranking_fixture")
sys.dont_write_bytecode = True

CUSTOM = dict(mrr_at_k=[5, 20], ndcg_at_k=[3, 7, 50], recall_at_k=[10, 100, 500])


def read_ranklists(path):
    ranking = {}
    with open(path) as fh:
        for line in fh:
            cols = line.strip().split("\t")
            ranking.setdefault(int(cols[0]), []).append(int(cols[1]))
    return ranking


def write_grade0_fixture():
    """qrels with grade-0 lines (dropped), a query whose only line has grade 0 (it then has no qrels at all), and a small run for them"""
    os.makedirs(FIX2, exist_ok=True)
    with open(os.path.join(FIX2, "qrels.grade0.tsv"), "w") as fh:
        fh.write("1\t0\t10\t1\n1\t0\t11\t0\n1\t0\t12\t2\n2\t0\t20\t0\n3\t0\t30\t1\n3\t0\t31\t0\n4\t0\t40\t3\n")
    with open(os.path.join(FIX2, "run.grade0.tsv"), "w") as fh:
        for q, docs in ((1, [11, 13, 12, 10, 14]), (2, [20, 21, 22]), (3, [31, 32, 33, 30]), (4, [41, 42]), (5, [50, 51])):
            for r, p in enumerate(docs):
                fh.write(f"{q}\t{p}\t{r + 1}\n")


def main():
    write_grade0_fixture()
    # the module file is loaded directly: the reference's evaluation/__init__.py pulls in faiss, which this image lacks
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_reranking_evaluator", "/root/reference/evaluation/reranking_evaluator.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    Ref = mod.RerankingEvaluator
    blob = {}

    def record(tag, ev, run_path, csv_path):
        d, (rr, rec, nd) = ev.direct_compute_metric(read_ranklists(run_path), return_per_query=True, per_query_metrics_path=csv_path)
        blob[tag + ".keys"] = np.array(list(d.keys()))
        blob[tag + ".values"] = np.array([float(v) for v in d.values()])
        blob[tag + ".rr"], blob[tag + ".rec"], blob[tag + ".ndcg"] = rr, rec, nd
        plain = ev.direct_compute_metric(read_ranklists(run_path))
        assert list(plain.keys()) == list(d.keys()) and [float(v) for v in plain.values()] == [float(v) for v in d.values()]

    for kind, qrels, trec in (("dev", "qrels.dev.tsv", False), ("trec", "qrels.trec.txt", True)):
        for run in ("run2.tsv", "run3.tsv", "run4.tsv"):
            record(f"{kind}.{run}", Ref(os.path.join(FIX, qrels), is_trec=trec), os.path.join(FIX, run),
                   os.path.join(FIX2, f"per_query.{kind}.{run}.csv"))
        record(f"{kind}.custom", Ref(os.path.join(FIX, qrels), is_trec=trec, **CUSTOM), os.path.join(FIX, "run3.tsv"),
               os.path.join(FIX2, f"per_query.{kind}.custom.csv"))
    record("grade0", Ref(os.path.join(FIX2, "qrels.grade0.tsv")), os.path.join(FIX2, "run.grade0.tsv"),
           os.path.join(FIX2, "per_query.grade0.csv"))
    np.savez_compressed(os.path.join(HERE, "reranking_evaluator.npz"), **blob)
    print("wrote", len(blob), "arrays")


if __name__ == "__main__":
    main()
