"""Host side of validation on a dev run (no GPU): evaluation.RerankingEvaluator against the metrics the REFERENCE's
``evaluation/reranking_evaluator.py`` produced on the committed fixtures (tests/golden/make_reranking_golden.py), evaluation.DevPool from
small text files, the ranking rule, and the command-line flags."""
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd.evaluation import DevPool, RerankingEvaluator
from cldrd_amd.evaluation import dev_pool as DP
from cldrd_amd.evaluation import reranking_evaluator as RE

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "evaluator_fixture")
FIX2 = os.path.join(HERE, "golden", "reranking_fixture")
CUSTOM = dict(mrr_at_k=[5, 20], ndcg_at_k=[3, 7, 50], recall_at_k=[10, 100, 500])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "reranking_evaluator.npz"))


def _ranklists(path):
    ranking = {}
    with open(path) as fh:
        for line in fh:
            cols = line.strip().split("\t")
            ranking.setdefault(int(cols[0]), []).append(int(cols[1]))
    return ranking


CASES = [(f"{kind}.{run}", os.path.join(FIX, qrels), trec, {}, os.path.join(FIX, run))
         for kind, qrels, trec in (("dev", "qrels.dev.tsv", False), ("trec", "qrels.trec.txt", True))
         for run in ("run2.tsv", "run3.tsv", "run4.tsv")]
CASES += [(f"{kind}.custom", os.path.join(FIX, qrels), trec, CUSTOM, os.path.join(FIX, "run3.tsv"))
          for kind, qrels, trec in (("dev", "qrels.dev.tsv", False), ("trec", "qrels.trec.txt", True))]
CASES += [("grade0", os.path.join(FIX2, "qrels.grade0.tsv"), False, {}, os.path.join(FIX2, "run.grade0.tsv"))]


@pytest.mark.parametrize("tag,qrels,trec,kw,run", CASES, ids=[c[0] for c in CASES])
def test_metrics_equal_the_reference(golden, tmp_path, tag, qrels, trec, kw, run):
    ev = RerankingEvaluator(qrels, is_trec=trec, **kw)
    csv_path = tmp_path / "per_query.csv"
    d, (rr, rec, nd) = ev.direct_compute_metric(_ranklists(run), return_per_query=True, per_query_metrics_path=str(csv_path))
    assert list(d.keys()) == golden[tag + ".keys"].tolist()                      # the reference's key order
    got = np.array([float(v) for v in d.values()])
    assert np.abs(got - golden[tag + ".values"]).max() <= 1e-12
    for mine, name in ((rr, ".rr"), (rec, ".rec"), (nd, ".ndcg")):
        assert mine.shape == golden[tag + name].shape and np.abs(mine - golden[tag + name]).max() <= 1e-12
    with open(os.path.join(FIX2, f"per_query.{tag}.csv"), "rb") as fh:
        assert csv_path.read_bytes() == fh.read()
    plain = ev.direct_compute_metric(_ranklists(run))
    assert list(plain.keys()) == list(d.keys()) and [float(v) for v in plain.values()] == got.tolist()


def test_fixture_cases_and_quirks(golden):
    """What the fixtures contain, seen in the numbers: ranked queries without qrels count as "no relevant" but not as ranked; grade-0
    lines are dropped (query 2 of the grade-0 fixture has no qrels left); Recall is reported at the MRR cut-offs."""
    ev = RerankingEvaluator(os.path.join(FIX, "qrels.dev.tsv"))
    ranking = _ranklists(os.path.join(FIX, "run3.tsv"))
    d = ev.direct_compute_metric(ranking)
    no_qrels = [q for q in ranking if q not in ev.qid_to_relevant_data]
    assert no_qrels and 9999 in ev.qid_to_relevant_data and 9999 not in ranking
    assert d["QueriesRanked"] == len(ranking) - len(no_qrels)
    assert d["QueriesWithNoRelevant@10"] + d["QueriesWithRelevant@10"] == len(ranking)
    assert any(len(set(docs)) < len(docs) for docs in ranking.values())        # a duplicated pid inside a ranking
    g = RerankingEvaluator(os.path.join(FIX2, "qrels.grade0.tsv"))
    assert sorted(g.qid_to_relevant_data) == [1, 3, 4] and g.qid_to_relevant_data[1] == {10: 1.0, 12: 2.0}
    c = RerankingEvaluator(os.path.join(FIX, "qrels.dev.tsv"), **CUSTOM)
    assert [k for k in c.direct_compute_metric(ranking) if k.startswith("Recall@")] == ["Recall@5", "Recall@20"]


def test_more_mrr_than_recall_cutoffs_is_a_value_error():
    with pytest.raises(ValueError, match=r"mrr_at_k \[10, 100, 1000\].*recall_at_k \[10, 100\]"):
        RerankingEvaluator(os.path.join(FIX, "qrels.dev.tsv"), mrr_at_k=[10, 100, 1000])
    RerankingEvaluator(os.path.join(FIX, "qrels.dev.tsv"), mrr_at_k=[10], recall_at_k=[10, 100])


# ---------------------------------------------------------------- DevPool
class Tok:
    """the toy tokenizer of tests/test_interop.py: [1] + one id per character + [2], cut to max_length"""
    name_or_path = "toy"
    sep_token = "|"
    calls = 0

    def __call__(self, texts, **kw):
        Tok.calls += len(texts)
        return {"input_ids": [[1] + [3 + (ord(c) % 7) for c in t][: kw["max_length"] - 2] + [2] for t in texts]}

    def __len__(self):
        return 10


def _pool_files(tmp_path):
    q, c, run = tmp_path / "queries.tsv", tmp_path / "collection.tsv", tmp_path / "run.tsv"
    q.write_text("7\talpha\n9\tbe\n11\tgamma delta\n13\tnever ranked\n")
    c.write_text("".join(f"{100 + j}\t{'x' * (j + 1)}\n" for j in range(12)) + "103\tlast text wins\n")
    # query 9 first; (9, 105) twice: kept once; passage 103 shared by queries 9 and 7; query 7's lines are interleaved with 11's
    run.write_text("9\t105\t1\t3.0\n9\t103\t2\t2.0\n7\t103\t1\t9.0\n9\t105\t3\t1.0\n11\t101\t1\t1.0\n7\t110\t2\t8.0\n9\t102\t4\t0.5\n"
                   "7\t100\t3\t7.0\n")
    return q, c, run


def test_dev_pool_pairs_tokens_and_table(tmp_path):
    from cldrd_amd.retriever.rerank_top_passages import read_run
    q, c, run = _pool_files(tmp_path)
    Tok.calls = 0
    pool = DevPool(str(run), str(q), str(c), Tok(), 6, 8)
    qids, pids, group, starts = read_run(str(run))
    assert pool.qids.tolist() == qids.tolist() == [9, 9, 9, 7, 7, 7, 11]
    assert pool.pids.tolist() == pids.tolist() == [105, 103, 102, 103, 110, 100, 101]
    assert pool.query_ids.tolist() == [9, 7, 11] and pool.n_pairs == 7
    assert pool.passage_ids.tolist() == [105, 103, 102, 110, 100, 101]          # distinct, 103 stored once
    assert pool.p_pos.tolist() == [0, 1, 2, 1, 3, 4, 5]
    assert Tok.calls == 3 + 6                                                 # the run's queries and passages, each once; not the tables
    assert pool.counts.tolist() == [3, 3, 1] and pool.counts.dtype == np.int32 and pool.cand_rows.dtype == np.int32
    assert pool.cand_rows.tolist() == [[0, 1, 2], [1, 3, 4], [5, -1, -1]]
    tok = Tok()
    want_q = tok(["be", "alpha", "gamma delta"], max_length=6)["input_ids"]
    assert pool.q_lens.tolist() == [len(t) for t in want_q] == [4, 6, 6]
    for row, t in zip(pool.q_tokens, want_q):
        assert row[:len(t)].tolist() == t and not row[len(t):].any()
    want_p = tok(["x" * 6, "last text wins", "xxx", "x" * 11, "x", "xx"], max_length=8)["input_ids"]      # a repeated id keeps its last text
    assert pool.p_lens.tolist() == [len(t) for t in want_p]
    for row, t in zip(pool.p_tokens, want_p):
        assert row[:len(t)].tolist() == t
    # batches: (length, pool position) order, fixed size, padded to the longest of the batch, token counts attached
    batches = pool._host_batches("p", 4)
    assert [b[0].tolist() for b in batches] == [[4, 5, 2, 0], [1, 3]]
    rows, b = batches[0]
    assert b["lengths"] == [3, 4, 5, 8] and tuple(b["input_ids"].shape) == (4, 8) and b["attention_mask"].sum(1).tolist() == [3, 4, 5, 8]


def test_dev_pool_top_k(tmp_path):
    q, c, run = _pool_files(tmp_path)
    pool = DevPool(str(run), str(q), str(c), Tok(), 6, 8, top_k=2)
    assert pool.qids.tolist() == [9, 9, 7, 7, 11] and pool.pids.tolist() == [105, 103, 103, 110, 101]
    assert pool.passage_ids.tolist() == [105, 103, 110, 101]
    assert pool.counts.tolist() == [2, 2, 1] and pool.cand_rows.tolist() == [[0, 1], [1, 2], [3, -1]]


def test_dev_pool_reads_an_existing_collection_token_cache(tmp_path):
    from cldrd_amd.dataset import SequenceTokenCache
    q, c, run = _pool_files(tmp_path)
    c.write_text("".join(f"{100 + j}\t{'x' * (j + 1)}\n" for j in range(12)))
    plain = DevPool(str(run), str(q), str(c), Tok(), 6, 8)
    cache_dir = tmp_path / "cache"
    cache_dir.mkdir()
    SequenceTokenCache.open_or_build(str(cache_dir), str(c), Tok(), 8)
    Tok.calls = 0
    cached = DevPool(str(run), str(q), str(c), Tok(), 6, 8, token_cache_dir=str(cache_dir))
    assert Tok.calls == 3                                                     # only the queries were tokenised
    assert np.array_equal(cached.p_tokens, plain.p_tokens) and np.array_equal(cached.p_lens, plain.p_lens)
    before = sorted(os.listdir(cache_dir))
    DevPool(str(run), str(q), str(c), Tok(), 6, 7, token_cache_dir=str(cache_dir))      # another length: no cache, none written
    assert sorted(os.listdir(cache_dir)) == before


def test_dev_pool_unknown_ids(tmp_path):
    q, c, run = _pool_files(tmp_path)
    with open(run, "a") as fh:
        fh.write("11\t555\t2\t0.1\n")
    with pytest.raises(KeyError, match="id 555 of .*run.tsv is not in the query / passage table"):
        DevPool(str(run), str(q), str(c), Tok(), 6, 8)
    from cldrd_amd.dataset import SequenceTokenCache
    (tmp_path / "cache").mkdir()
    SequenceTokenCache.open_or_build(str(tmp_path / "cache"), str(c), Tok(), 8)
    with pytest.raises(KeyError, match="id 555 "):
        DevPool(str(run), str(q), str(c), Tok(), 6, 8, token_cache_dir=str(tmp_path / "cache"))
    run.write_text("7\t100\n8\t101\n")
    with pytest.raises(KeyError, match="id 8 of "):
        DevPool(str(run), str(q), str(c), Tok(), 6, 8)


def test_rescore_is_chunked_by_queries(tmp_path, monkeypatch):
    """cldrd_topk_rescore has the query on blockIdx.y: at most 65535 per launch.  With the constant lowered, the launches of a pool of three
    queries - recorded by a stand-in for the op that computes the same table on the host."""
    import torch
    assert DP.RESCORE_CHUNK == 65535
    assert DP.rescore_chunks(65535) == [(0, 65535)] and DP.rescore_chunks(65536) == [(0, 65535), (65535, 65536)]
    assert DP.rescore_chunks(150000) == [(0, 65535), (65535, 131070), (131070, 150000)]
    q, c, run = _pool_files(tmp_path)
    pool = DevPool(str(run), str(q), str(c), Tok(), 6, 8)
    monkeypatch.setattr(DP, "RESCORE_CHUNK", 2)
    calls = []

    def fake(q32, P, counts, cand_rows, cand_scores, qmu=None):
        calls.append(q32.shape[0])
        assert q32.shape[0] <= 2 and counts.shape[0] == cand_rows.shape[0] == cand_scores.shape[0] == q32.shape[0]
        for i in range(q32.shape[0]):
            for j in range(int(counts[i])):
                cand_scores[i, j] = (q32[i].double() * P[int(cand_rows[i, j])].double()).sum().float()
    monkeypatch.setattr(DP.ops, "topk_rescore", fake)
    g = torch.Generator().manual_seed(0)
    qe, pe = torch.randn(3, 8, generator=g), torch.randn(6, 8, generator=g)
    scores = pool.score_embeddings(qe, pe)
    assert calls == [2, 1]
    want = (qe[pool.group].double() * pe[pool.p_pos].double()).sum(1).float().numpy()
    assert scores.dtype == np.float32 and np.array_equal(scores, want)
    with pytest.raises(ValueError, match="one row per distinct"):
        pool.score_embeddings(qe[:2], pe)


def test_ranking_rule_ties_in_run_order():
    group = np.array([0, 0, 0, 0, 1, 1, 1])
    scores = np.array([1.0, 2.0, 2.0, 1.0, -0.0, 0.0, 5.0], dtype=np.float32)
    from cldrd_amd.retriever.rerank_top_passages import rank_order
    assert rank_order(group, scores).tolist() == [1, 2, 0, 3, 6, 4, 5]


def test_dev_log_and_best_file(tmp_path):
    import json
    log, best_path = str(tmp_path / "log" / "dev_logs.log"), str(tmp_path / "dev_best.json")
    m = {"MRR@10": np.float64(0.25), "QueriesWithRelevant@10": np.int64(3), "QueriesRanked": 4}
    RE.write_dev_logs(log, 1, 4, m, 1.5)
    RE.write_dev_logs(log, 2, 8, m, 0.25)
    lines = open(log).read().splitlines()
    assert lines == ["epoch\tstep\tMRR@10\tQueriesWithRelevant@10\tQueriesRanked\tseconds", "1\t4\t0.25\t3\t4\t1.500", "2\t8\t0.25\t3\t4\t0.250"]
    best = RE.update_dev_best(best_path, None, m, 4, 1, "models/checkpoint_4.pth.tar")
    best = RE.update_dev_best(best_path, best, m, 8, 2, "models/checkpoint_8.pth.tar")            # a tie keeps the earlier step
    assert json.load(open(best_path)) == best == {"metric": "MRR@10", "value": 0.25, "step": 4, "epoch": 1,
                                                   "checkpoint": "models/checkpoint_4.pth.tar"}
    best = RE.update_dev_best(best_path, best, dict(m, **{"MRR@10": 0.5}), 12, 3, "models/checkpoint_12.pth.tar")
    assert json.load(open(best_path))["step"] == 12 and sorted(os.listdir(tmp_path)) == ["dev_best.json", "log"]


# ---------------------------------------------------------------- command lines
def test_trainer_dev_flags():
    from cldrd_amd.trainer import nway_listwise as T
    a = T.get_args([])
    assert a.dev_path is None and a.dev_queries_path is None and a.dev_qrels_path is None
    assert a.dev_top_k == 0 and a.dev_batch_size == 512 and a.dev_qrels_trec is False
    assert T._dev_validation(a) is None
    three = ["--dev_path", "run.tsv", "--dev_queries_path", "q.tsv", "--dev_qrels_path", "qrels.tsv"]
    b = T.get_args(three + ["--dev_top_k", "100", "--dev_batch_size", "256", "--dev_qrels_trec"])
    assert (b.dev_path, b.dev_queries_path, b.dev_qrels_path, b.dev_top_k, b.dev_batch_size, b.dev_qrels_trec) == \
        ("run.tsv", "q.tsv", "qrels.tsv", 100, 256, True)
    for drop in range(3):
        two = three[:2 * drop] + three[2 * drop + 2:]
        with pytest.raises(SystemExit):
            T.get_args(two)
    with pytest.raises(SystemExit):
        T.get_args(three[:2])
    with pytest.raises(SystemExit):
        T.get_args(three + ["--synthetic_steps", "5"])


def test_rerank_command_line_flags_old_and_new():
    from cldrd_amd.retriever import rerank_top_passages as R
    old = ["--run_path", "r", "--queries_path", "q", "--collection_path", "c", "--model_name_or_path", "m", "--output_path", "o"]
    a = R.get_args(old)
    assert (a.max_len, a.top_k, a.batch_size, a.token_cache_dir, a.fp32_encode, a.tokenizer_name_or_path) == (256, 0, 2048, "", False, None)
    assert a.dual_encoder is False
    b = R.get_args(old + ["--tokenizer_name_or_path", "t", "--max_len", "48", "--batch_size", "300", "--token_cache_dir", "d", "--top_k", "7",
                          "--fp32_encode"])
    assert (b.max_len, b.top_k, b.batch_size, b.token_cache_dir, b.fp32_encode, b.tokenizer_name_or_path) == (48, 7, 300, "d", True, "t")
    s = R.get_args(old + ["--dual_encoder", "--resume", "ck", "--share_weights"])
    assert (s.dual_encoder, s.resume, s.share_weights, s.query_max_len, s.passage_max_len, s.batch_size) == (True, "ck", True, 30, 256, 512)
    assert R.get_args(old + ["--dual_encoder", "--batch_size", "64"]).batch_size == 64


def test_continue_rerank_evaluator_flags_and_checkpoint_order(tmp_path):
    from cldrd_amd.evaluation import continue_rerank_evaluator as C
    a = C.get_args(["--resume_folder", "models/", "--dev_path", "r", "--dev_queries_path", "q", "--dev_qrels_path", "z", "--collection_path",
                    "c", "--output_path", "o"])
    assert (a.share_weights, a.dev_batch_size, a.dev_top_k, a.query_max_len, a.passage_max_len) == (False, 512, 0, 30, 256)
    for name in ("checkpoint_100.pth.tar", "checkpoint_8.pth.tar", "checkpoint_20.pth.tar", "checkpoint_x.pth.tar", "other.txt"):
        (tmp_path / name).write_text("")
    assert [s for s, _ in C.checkpoints_in_step_order(str(tmp_path))] == [8, 20, 100]


def test_a_model_on_the_host_is_refused(tmp_path):
    import selftest
    q, c, run = _pool_files(tmp_path)
    pool = DevPool(str(run), str(q), str(c), Tok(), 6, 8)
    model = selftest.build_tiny_model()
    ev = RerankingEvaluator(os.path.join(FIX, "qrels.dev.tsv"))
    was = model.training
    with pytest.raises(RuntimeError, match="GPU"):
        ev.compute_metrics_pool(model, pool)
    with pytest.raises(RuntimeError, match="GPU"):
        ev.compute_metrics(model, [])
    assert model.training == was


def test_trainer_builds_the_dev_pool_once_and_a_resumed_run_keeps_its_best(tmp_path):
    """train() hands rank 0 a pool and an evaluator built from the training flags (no GPU involved in building them); with --resume the best
    of the run so far is read back, a fresh run starts without one."""
    import json
    from cldrd_amd.trainer import nway_listwise as T
    from test_rerank_host import make_pair_tokenizer, words
    make_pair_tokenizer().save_pretrained(str(tmp_path / "tok"))
    (tmp_path / "c.tsv").write_text("".join(f"{100 + j}\t{words(3 + j, j)}\n" for j in range(6)))
    (tmp_path / "q.tsv").write_text("1\tw1 w2\n2\tw3\n")
    (tmp_path / "run.tsv").write_text("2\t103\n2\t100\n1\t103\n1\t105\n2\t101\n")
    (tmp_path / "qrels.tsv").write_text("1\t0\t105\t1\n2\t0\t100\t1\n")
    argv = ["--experiment_folder", str(tmp_path), "--run_folder", "r", "--collection_path", str(tmp_path / "c.tsv"), "--tokenizer_name_or_path",
            str(tmp_path / "tok"), "--query_max_len", "8", "--passage_max_len", "6", "--dev_path", str(tmp_path / "run.tsv"),
            "--dev_queries_path", str(tmp_path / "q.tsv"), "--dev_qrels_path", str(tmp_path / "qrels.tsv"), "--dev_top_k", "2"]
    dv = T._dev_validation(T.get_args(argv))
    assert dv.best is None and dv.batch_size == 512 and dv.pool.qids.tolist() == [2, 2, 1, 1] and dv.pool.pids.tolist() == [103, 100, 103, 105]
    assert dv.pool.p_lens.tolist() == [6, 5, 6] and dv.evaluator.qid_to_relevant_data == {1: {105: 1.0}, 2: {100: 1.0}}
    assert dv.log_file == str(tmp_path / "r" / "log" / "dev_logs.log") and dv.best_file == str(tmp_path / "r" / "dev_best.json")
    assert not os.path.exists(tmp_path / "r")                                  # nothing is written before the first validation
    os.makedirs(tmp_path / "r")
    kept = {"metric": "MRR@10", "value": 0.5, "step": 4, "epoch": 1, "checkpoint": "x"}
    (tmp_path / "r" / "dev_best.json").write_text(json.dumps(kept))
    assert T._dev_validation(T.get_args(argv)).best is None
    assert T._dev_validation(T.get_args(argv + ["--resume", "ckpt"])).best == kept
