"""Host side of the one-job stage file (``retriever.build_stage_file``): its command line, what it refuses before anything is loaded, the id ->
cache-row mapping, the batching it shares with ``rerank_top_passages``, and the C entry point's declaration and argument checks.  No GPU."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd.retriever import build_stage_file as B

REQUIRED = ["--index_path", "idx", "--queries_path", "q.tsv", "--collection_path", "c.tsv", "--teacher_name_or_path", "teacher",
            "--label_mode", "9", "--output_path", "out.json"]


def test_get_args_defaults():
    a = B.get_args(REQUIRED)
    assert (a.resume, a.model_name_or_path, a.tokenizer_name_or_path, a.share_weights) == ("", "distilbert-base-uncased", "distilbert-base-uncased", False)
    assert (a.query_max_len, a.top_k, a.use_float16) == (30, 200, False)
    assert (a.teacher_tokenizer_name_or_path, a.teacher_max_len, a.teacher_batch_size, a.token_cache_dir) == (None, 256, 2048, "")
    assert (a.most_hard_ranks, a.semi_hard_ranks, a.n_most_hard, a.seed, a.with_scores) == (None, None, None, 0, False)
    assert (a.student_run_path, a.teacher_run_path) == ("", "")
    b = B.get_args(REQUIRED + ["--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--with_scores", "--use_float16", "--share_weights"])
    assert (b.most_hard_ranks, b.semi_hard_ranks, b.with_scores, b.use_float16, b.share_weights) == ((11, 30), (31, 60), True, True, True)
    with pytest.raises(SystemExit):
        B.get_args(REQUIRED[:-2])


@pytest.fixture
def no_loading(monkeypatch):
    """every loader of the job fails: what is refused below is refused before a model, a tokenizer, an index or the GPU is touched"""
    import transformers
    from cldrd_amd.models import cross_encoder, nway_dual_encoder
    from cldrd_amd.retriever import retrieval_utils

    def fail(*a, **k):
        raise AssertionError("a loader ran before the arguments were validated")
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", fail)
    monkeypatch.setattr(cross_encoder.CrossEncoder, "from_pretrained", fail)
    monkeypatch.setattr(nway_dual_encoder.NwayDualEncoder, "__init__", fail)
    monkeypatch.setattr(retrieval_utils, "read_index", fail)
    monkeypatch.setattr(torch.cuda, "set_device", fail)


def test_a_bad_window_fails_before_anything_is_loaded(no_loading, tmp_path):
    q = tmp_path / "q.tsv"                                  # never opened: the windows come first
    args = REQUIRED[:]
    args[args.index("q.tsv")] = str(q)
    with pytest.raises(ValueError, match="overlap"):
        B.main(B.get_args(args + ["--most_hard_ranks", "11:120", "--semi_hard_ranks", "101:200"]))
    with pytest.raises(ValueError, match="fewer than the 10"):
        B.main(B.get_args(args + ["--semi_hard_ranks", "101:105"]))
    with pytest.raises(ValueError, match="label mode 1 "):
        B.main(B.get_args([("1" if v == "9" else v) for v in args]))
    with pytest.raises(ValueError, match="top_k"):
        B.main(B.get_args(args + ["--top_k", "0"]))


def test_a_repeated_qid_is_refused_before_anything_is_loaded(no_loading, tmp_path):
    q = tmp_path / "q.tsv"
    q.write_text("7\ta b\n3\tc\n\n9\td\n3\te f\n7\tg\n")
    args = REQUIRED[:]
    args[args.index("q.tsv")] = str(q)
    with pytest.raises(ValueError, match="qid 7 occurs more than once"):
        B.main(B.get_args(args))
    q.write_text("7\ta b\n3\tc\nno-tab-line\n9\td\n")
    assert B.read_query_ids(q).tolist() == [7, 3, 9]


def test_cache_rows_maps_ids_with_array_operations():
    keys = np.array([40, -3, 1 << 41, 7, 0], dtype=np.int64)
    ids = np.array([[7, 7, -3], [1 << 41, 0, 40]], dtype=np.int64)
    rows = B.cache_rows(keys, ids, "passage")
    assert rows.shape == ids.shape and rows.dtype == np.int64 and np.array_equal(keys[rows], ids)
    assert B.cache_rows(keys, np.zeros(0, dtype=np.int64), "passage").shape == (0,)
    for missing in (8, -4, (1 << 41) + 1, 1 << 50):
        with pytest.raises(KeyError, match=f"id {missing} is not in the passage table"):
            B.cache_rows(keys, np.array([7, missing, 40]), "passage")
    with pytest.raises(KeyError):
        B.cache_rows(np.zeros(0, dtype=np.int64), np.array([1]), "query")


class _Cache:
    def __init__(self, lens):
        self.lens = np.asarray(lens, dtype=np.int32)


class _Model:
    """score of a pair = 1000 * query row + passage row; records the batches it was given"""
    def __init__(self):
        self.batches = []

    def score_cached(self, q_cache, p_cache, q_rows, p_rows, max_len, **kw):
        self.batches.append((np.asarray(q_rows).copy(), np.asarray(p_rows).copy(), dict(kw)))
        return torch.from_numpy((1000.0 * np.asarray(q_rows) + np.asarray(p_rows)).astype(np.float32))


def test_score_pairs_is_the_batching_of_rerank_top_passages():
    from cldrd_amd.models.cross_encoder import pair_lengths
    from cldrd_amd.retriever import rerank_top_passages as R
    rng = np.random.default_rng(5)
    qc, pc = _Cache(rng.integers(3, 12, 9)), _Cache(rng.integers(3, 40, 50))
    q_rows, p_rows = rng.integers(0, 9, 101), rng.integers(0, 50, 101)
    m = _Model()
    got = R.score_pairs(m, qc, pc, q_rows, p_rows, 64, 16)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), (1000.0 * q_rows + p_rows).astype(np.float32))
    _, _, lengths, _ = pair_lengths(qc.lens[q_rows] - 2, pc.lens[p_rows] - 2, 64)
    want = R.length_batches(lengths, 16)
    assert len(m.batches) == len(want) == 7
    for (bq, bp, kw), b in zip(m.batches, want):
        assert np.array_equal(bq, q_rows[b]) and np.array_equal(bp, p_rows[b]) and kw == {}
    m2 = _Model()
    R.score_pairs(m2, qc, pc, q_rows[:5], p_rows[:5], 64, 16, fp32=True)
    assert m2.batches[0][2] == {"fp32": True}


def test_write_ranked_run_takes_a_given_order(tmp_path, monkeypatch):
    from cldrd_amd.retriever import rerank_top_passages as R
    rng = np.random.default_rng(6)
    nq, k = 5, 7
    qids, group = np.repeat(np.arange(100, 100 + nq), k), np.repeat(np.arange(nq), k)
    pids = rng.permutation(nq * k).astype(np.int64)
    scores = rng.choice(np.array([0.5, 1.5, -2.0], dtype=np.float32), nq * k)
    starts = np.arange(nq + 1, dtype=np.int64) * k
    a, b = tmp_path / "a.run", tmp_path / "b.run"
    assert R.write_ranked_run(str(a), qids, pids, group, starts, scores) == nq * k
    order = R.rank_order(group, scores)
    monkeypatch.setattr(R, "rank_order", lambda *args: pytest.fail("the given order must be used"))
    assert R.write_ranked_run(str(b), qids, pids, group, starts, scores, order=order) == nq * k
    assert a.read_bytes() == b.read_bytes()


def test_entry_point_is_declared_bound_and_checks_its_arguments():
    """cldrd_curriculum_select: in the header, in SIGNATURES at ABI 106, and every call below is rejected in front of any HIP call (small
    integers stand in for the device pointers, as in tests/test_capi.py)."""
    import os
    from cldrd_amd import _lib
    from conftest import ROOT
    assert _lib.ABI_VERSION == 106 and "cldrd_curriculum_select" in _lib.SIGNATURES
    assert "int cldrd_curriculum_select(" in open(os.path.join(ROOT, "include", "cldrd_hip.h")).read()
    lib = _lib.load()
    assert lib.cldrd_version() == 106
    P = 64

    def select(nq=4, K=64, n_rel=10, n_most=10, most=(11, 30), n_semi=10, semi=(31, 64), order=P):
        return lib.cldrd_curriculum_select(P, P, P, P, nq, K, n_rel, n_most, most[0], most[1], n_semi, semi[0], semi[1], 5, order, P, P, P, None)

    cases = [lambda: select(K=1025), lambda: select(K=0), lambda: select(nq=0), lambda: select(order=None),
             lambda: select(most=(10, 30)), lambda: select(most=(11, 19)), lambda: select(semi=(30, 64)), lambda: select(semi=(31, 30)),
             lambda: select(n_rel=0, n_most=0, n_semi=0), lambda: select(n_rel=-1)]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)
        rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0 and msg.startswith("curriculum_select:"), f"case {i}: {rc} {msg!r}"
    lib.cldrd_set_tuning(None, 0)
    assert select(K=1025) != 0 and "1024" in lib.cldrd_last_error().decode()
