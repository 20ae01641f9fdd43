"""The teacher score store on the GPU (retriever/score_store.py, csrc/pairstore.hip): ``hip_ops.pair_lookup`` against a dict,
``hip_ops.pair_merge`` against ``np.lexsort``, the store's append / compact / reopen, and the two programs with ``--score_store`` against
their own store-less output.  Every comparison is exact: score bits and file bytes."""
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd import hip_ops as ops
from test_gpu_curriculum import N_Q, TOP
from test_gpu_rerank import _hf_model, _save, _toy_files
from test_gpu_stage_file import stage  # noqa: F401  (the fixture of the one-job tests)
from test_rerank_host import make_pair_tokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
HI = 1 << 32
SENTINEL = 0x7FC12345           # a NaN pattern no score has
IDENTITY = {"teacher_sha256": "cd" * 32, "num_labels": 1, "max_len": 96, "arithmetic": "fp16"}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)       # (a copy: a one-entry column slice keeps its row stride)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def make_keys(rng, n, one_qid=False):
    """n distinct keys [n, 2] int64 in (qid, pid) order: ~40 pids per qid, ids above 2^40, qids and pids that differ only above bit 32
    (x and x + 2^32), one negative qid.  Every pid is 7 mod 3, so pid - 1 and pid + 1 are never in the set."""
    n_q = 1 if one_qid else n // 40 + 2
    base = rng.choice(1 << 20, size=n_q // 2 + 1, replace=False).astype(np.int64) * 4 + (1 << 41)
    qs = np.concatenate([base, base + HI])[:n_q]
    if n_q >= 3:
        qs[2] = -qs[2]
    m = 3 * n + 64
    q = qs[rng.integers(0, n_q, m)]
    p = rng.integers(0, max(5000, 2 * n), m).astype(np.int64) * 3 + 7 + rng.integers(0, 2, m) * HI + rng.integers(0, 2, m) * (1 << 40)
    k = np.unique(np.stack([q, p], 1), axis=0)
    k = k[np.sort(rng.choice(k.shape[0], n, replace=False))]
    k = k[np.lexsort((k[:, 1], k[:, 0]))]
    assert k.shape == (n, 2)
    return k


def make_scores(rng, n):
    s = rng.standard_normal(n).astype(np.float32)
    special = np.array([-0.0, 1e-42, 0.0], dtype=np.float32)        # -0.0, a denormal, +0.0: the bits are what is stored
    s[:min(n, 3)] = special[:min(n, 3)]
    return s


def oracle_of(keys, scores):
    return {(int(q), int(p)): int(b) for (q, p), b in zip(keys, scores.view(np.uint32))}


def lookup_batch(rng, keys):
    """Rows (qid, pids) that meet every case of the search for the segment ``keys``."""
    present = set(map(tuple, keys.tolist()))
    qids = np.unique(keys[:, 0])

    def pids_of(q):
        return keys[keys[:, 0] == q, 1]

    def absent_qid(q):
        assert not (keys[:, 0] == q).any()
        return int(q)
    rows = []
    for length in (0, 1, 64, 65, 200, 1024, 1500):                 # half of a row from the query's stored pids, half next to them
        q = int(qids[rng.integers(qids.shape[0])])
        own = pids_of(q)
        p = own[rng.integers(0, own.shape[0], length)] + rng.integers(0, 2, length)
        rows.append((q, p))
    first, last = int(keys[0, 0]), int(keys[-1, 0])
    rows.append((absent_qid(first - 1), pids_of(first)))           # a qid below the first key, above the last, absent in the middle
    rows.append((absent_qid(last + 1), pids_of(last)))
    mid = int(qids[qids.shape[0] // 2])
    rows.append((absent_qid(mid + 1), pids_of(mid)))
    for q in (int(qids[0]), int(qids[-1]), mid):
        if (q + HI) not in qids:
            rows.append((q + HI, pids_of(q)))                      # equal in the low 32 bits only
        own = pids_of(q)
        rows.append((q, np.concatenate([own[:1] - 1, own[:1] + 1, own[-1:] + 1, own[-1:] + HI, own[:1] - HI, own])))      # below, between, above
    for q in qids[:50]:
        if (int(q) + HI) in qids:                                  # x and x + 2^32 both stored: each row finds its own entries
            rows.append((int(q), np.concatenate([pids_of(q), pids_of(q + HI)])))
            rows.append((int(q) + HI, np.concatenate([pids_of(q), pids_of(q + HI)])))
            break
    rows.append((mid, np.zeros(0, dtype=np.int64)))                # an empty row at the end
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    qid = np.array([r[0] for r in rows], dtype=np.int64)
    starts = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r[1]) for r in rows], out=starts[1:])
    pid = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in rows])
    assert any((int(q), int(p)) in present for q, ps in rows for p in ps)
    return qid, starts, pid


def all_rows(keys):
    """the segment's own keys as a CSR batch: every pair hits"""
    qid, first = np.unique(keys[:, 0], return_index=True)
    return qid, np.append(first, keys.shape[0]).astype(np.int64), keys[:, 1].copy()


def expect_lookup(oracle, qid, starts, pid, score_bits, hit):
    score_bits, hit = score_bits.copy(), hit.copy()
    for r in range(qid.shape[0]):
        for i in range(int(starts[r]), int(starts[r + 1])):
            b = oracle.get((int(qid[r]), int(pid[i])))
            if b is not None:
                score_bits[i], hit[i] = b, 1
    return score_bits, hit


def run_lookup(segments, qid, starts, pid, rng):
    """the lookup over ``segments`` in turn, on outputs prefilled with a sentinel and a few hit bytes already 1 -> (score bits, hit, the
    prefilled two)"""
    total = pid.shape[0]
    bits0 = np.full(total, SENTINEL, dtype=np.uint32)
    hit0 = (rng.random(total) < 0.1).astype(np.uint8)
    score, hit = _dev(bits0.view(np.float32)), _dev(hit0)
    for keys, scores in segments:
        out = ops.pair_lookup(_dev(keys[:, 0]), _dev(keys[:, 1]), _dev(scores), _dev(qid), _dev(starts), _dev(pid), score, hit)
        assert out[0] is score and out[1] is hit
    return _bits(score), hit.cpu().numpy(), bits0, hit0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 100003])
def test_pair_lookup_equals_a_dict(n):
    rng = np.random.default_rng(n)
    keys, scores = make_keys(rng, n), make_scores(rng, n)
    oracle = oracle_of(keys, scores)
    qid, starts, pid = lookup_batch(rng, keys)
    got_s, got_h, bits0, hit0 = run_lookup([(keys, scores)], qid, starts, pid, rng)
    want_s, want_h = expect_lookup(oracle, qid, starts, pid, bits0, hit0)
    assert 0 < int((want_s != SENTINEL).sum()) < pid.shape[0]      # the batch has hits and misses
    assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s)
    # all hit: the segment's own keys, special scores included
    qid, starts, pid = all_rows(keys)
    got_s, got_h, _, _ = run_lookup([(keys, scores)], qid, starts, pid, rng)
    assert (got_h == 1).all() and np.array_equal(got_s, scores.view(np.uint32))
    # none hit: every pid moved by one; nothing is written
    got_s, got_h, bits0, hit0 = run_lookup([(keys, scores)], qid, starts, pid + 1, rng)
    assert np.array_equal(got_h, hit0) and np.array_equal(got_s, bits0)


def test_pair_lookup_over_two_segments_gives_the_union():
    rng = np.random.default_rng(7)
    keys, scores = make_keys(rng, 3000), make_scores(rng, 3000)
    side = rng.random(3000) < 0.5
    qid, starts, pid = lookup_batch(rng, keys)
    got_s, got_h, bits0, hit0 = run_lookup([(keys[side], scores[side]), (keys[~side], scores[~side])], qid, starts, pid, rng)
    want_s, want_h = expect_lookup(oracle_of(keys, scores), qid, starts, pid, bits0, hit0)
    assert np.array_equal(got_h, want_h) and np.array_equal(got_s, want_s)
    # the wrapper's own outputs: zeroed (the stored pids moved by one: no pair hits)
    qid, starts, pid = all_rows(keys)
    score, hit = ops.pair_lookup(_dev(keys[:, 0]), _dev(keys[:, 1]), _dev(scores), _dev(qid), _dev(starts), _dev(pid + 1))
    assert not hit.any().item() and not _bits(score).any()
    # no queries, no pairs: no launch
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    score, hit = ops.pair_lookup(_dev(keys[:, 0]), _dev(keys[:, 1]), _dev(scores), empty, torch.zeros(1, dtype=torch.int64, device=DEV), empty)
    assert score.shape == (0,) and hit.shape == (0,)


# ---------------------------------------------------------------- merge
def split_mask(rng, n_a, n_b, pattern):
    """which of the n_a + n_b sorted keys go to a (exactly n_a of them)"""
    n = n_a + n_b
    if pattern == "a_first":
        return np.arange(n) < n_a
    if pattern == "b_first":
        return np.arange(n) >= n_b
    if pattern == "alternating":                                    # strictly alternating while both last
        m = min(n_a, n_b)
        mask = np.zeros(n, dtype=bool)
        mask[0:2 * m:2] = True
        mask[2 * m:] = n_a > n_b
        return mask
    if pattern == "runs":                                           # long runs of one side
        want = np.zeros(n, dtype=bool)
        at, side = 0, True
        while at < n:
            run = int(rng.integers(1, 5000))
            want[at:at + run] = side
            at, side = at + run, not side
    else:
        want = rng.random(n) < 0.5
    # repair the count: flip random entries of the side that has too many
    extra = int(want.sum()) - n_a
    flip = rng.choice(np.flatnonzero(want if extra > 0 else ~want), abs(extra), replace=False)
    want[flip] = extra < 0
    return want


def check_merge(keys, scores, mask):
    a_k, a_s, b_k, b_s = keys[mask], scores[mask], keys[~mask], scores[~mask]
    q, p, s = ops.pair_merge(_dev(a_k[:, 0]), _dev(a_k[:, 1]), _dev(a_s), _dev(b_k[:, 0]), _dev(b_k[:, 1]), _dev(b_s))
    cat_k, cat_s = np.concatenate([a_k, b_k]), np.concatenate([a_s, b_s])
    order = np.lexsort((cat_k[:, 1], cat_k[:, 0]))
    assert np.array_equal(q.cpu().numpy(), cat_k[order, 0]) and np.array_equal(p.cpu().numpy(), cat_k[order, 1])
    assert np.array_equal(_bits(s), cat_s[order].view(np.uint32))


SIZES = [(1, 1), (2048, 1), (1, 2048), (2047, 2049), (100003, 70001)]


@pytest.mark.parametrize("pattern", ["a_first", "b_first", "alternating", "runs", "random"])
@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_pair_merge_equals_lexsort(n_a, n_b, pattern):
    """Mixed keys: ~40 pids per qid, so a qid's run lies in both inputs with interleaved pids under every pattern but the two ``first``
    ones, and runs straddle the tile boundaries; ids that differ only above bit 32."""
    rng = np.random.default_rng(n_a * 7 + n_b)
    keys, scores = make_keys(rng, n_a + n_b), make_scores(rng, n_a + n_b)
    check_merge(keys, scores, split_mask(rng, n_a, n_b, pattern))


@pytest.mark.parametrize("n_a,n_b", [(2047, 2049), (100003, 70001)])
def test_pair_merge_one_qid_in_both_inputs(n_a, n_b):
    """One qid throughout: the run straddles every partition boundary and only the pids (some equal in their low 32 bits) order the merge."""
    rng = np.random.default_rng(n_a)
    keys, scores = make_keys(rng, n_a + n_b, one_qid=True), make_scores(rng, n_a + n_b)
    assert np.unique(keys[:, 0]).shape[0] == 1
    for pattern in ("alternating", "random"):
        check_merge(keys, scores, split_mask(rng, n_a, n_b, pattern))


def test_pair_merge_with_an_empty_side_is_a_copy():
    rng = np.random.default_rng(3)
    keys, scores = make_keys(rng, 500), make_scores(rng, 500)
    check_merge(keys, scores, np.ones(500, dtype=bool))
    check_merge(keys, scores, np.zeros(500, dtype=bool))


@pytest.mark.parametrize("at", [0, 1000, 2047, 4999])
def test_pair_merge_raises_on_a_key_in_both_inputs(at):
    """a = keys[:5000], b = a's key ``at`` and 3000 later keys: the merged copy lands right behind the original - at 2047 as the first entry
    of the second tile."""
    rng = np.random.default_rng(11)
    keys, scores = make_keys(rng, 8000), make_scores(rng, 8000)
    a = (keys[:5000], scores[:5000])
    b = (np.concatenate([keys[at:at + 1], keys[5000:]]), np.concatenate([scores[at:at + 1], scores[5000:]]))
    with pytest.raises(ValueError, match="both inputs"):
        ops.pair_merge(_dev(a[0][:, 0]), _dev(a[0][:, 1]), _dev(a[1]), _dev(b[0][:, 0]), _dev(b[0][:, 1]), _dev(b[1]))
    with pytest.raises(ValueError, match="both inputs"):
        ops.pair_merge(_dev(b[0][:, 0]), _dev(b[0][:, 1]), _dev(b[1]), _dev(a[0][:, 0]), _dev(a[0][:, 1]), _dev(a[1]))


# ---------------------------------------------------------------- store
def _store(path):
    from cldrd_amd.retriever.score_store import TeacherScoreStore
    return TeacherScoreStore(str(path), IDENTITY, DEV)


def _append(store, keys, scores, order):
    store.append(_dev(keys[order, 0]), _dev(keys[order, 1]), _dev(scores[order]))


def _snapshot(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


def test_store_append_compact_reopen(tmp_path):
    rng = np.random.default_rng(5)
    keys, scores = make_keys(rng, 9000), make_scores(rng, 9000)
    oracle = oracle_of(keys, scores)
    part = rng.integers(0, 3, 9000)
    qid, starts, pid = lookup_batch(rng, keys)

    def check(store):
        score, hit = store.lookup(_dev(qid), _dev(starts), _dev(pid))
        want_s, want_h = expect_lookup(oracle, qid, starts, pid, np.zeros(pid.shape[0], np.uint32), np.zeros(pid.shape[0], np.uint8))
        assert np.array_equal(hit.cpu().numpy(), want_h) and np.array_equal(_bits(score), want_s)

    store = _store(tmp_path / "s")
    for i in range(3):
        at = np.flatnonzero(part == i)
        _append(store, keys, scores, rng.permutation(at))           # a chunk arrives in any order
    assert len(store.segments) == 3 and len(store) == 9000
    check(store)
    store.compact()
    assert len(store.segments) == 1
    _, q, p, s = store.segments[0]
    assert np.array_equal(q.cpu().numpy(), keys[:, 0]) and np.array_equal(p.cpu().numpy(), keys[:, 1])
    assert np.array_equal(_bits(s), scores.view(np.uint32))
    check(store)
    store.close()
    files = sorted(os.listdir(tmp_path / "s"))
    assert len(files) == 4 and "meta.json" in files and ".lock" not in files          # the three merged segments' files are gone
    store = _store(tmp_path / "s")
    assert len(store.segments) == 1 and len(store) == 9000
    check(store)
    store.close()


def test_store_duplicates_inside_a_chunk(tmp_path):
    from cldrd_amd.retriever.score_store import ScoreStoreError
    rng = np.random.default_rng(6)
    keys, scores = make_keys(rng, 300), make_scores(rng, 300)
    store = _store(tmp_path / "s")
    twice = np.concatenate([rng.permutation(300), [0, 1, 2, 150, 299]])               # -0.0, the denormal and +0.0 among the repeats
    _append(store, keys, scores, twice)
    assert len(store.segments) == 1 and len(store) == 300
    _, q, p, s = store.segments[0]
    assert np.array_equal(q.cpu().numpy(), keys[:, 0]) and np.array_equal(_bits(s), scores.view(np.uint32))
    other = make_keys(rng, 100)
    other[:, 0] += 1
    bad_scores = np.concatenate([np.zeros(100, np.float32), np.array([-0.0], np.float32)])      # 0.0 and -0.0: equal values, other bits
    before = _snapshot(tmp_path / "s")
    with pytest.raises(ScoreStoreError, match="different scores"):
        store.append(_dev(np.append(other[:, 0], other[0, 0])), _dev(np.append(other[:, 1], other[0, 1])), _dev(bad_scores))
    assert _snapshot(tmp_path / "s") == before and len(store.segments) == 1
    store.close()


def test_store_compaction_refuses_a_key_in_two_segments_and_changes_nothing(tmp_path):
    rng = np.random.default_rng(8)
    keys, scores = make_keys(rng, 6000), make_scores(rng, 6000)
    store = _store(tmp_path / "s")
    _append(store, keys, scores, np.arange(0, 4000))
    _append(store, keys, scores, np.arange(3999, 6000))             # key 3999 again: a caller that appended a pair that had not missed
    before = _snapshot(tmp_path / "s")
    with pytest.raises(ValueError, match="both inputs"):
        store.compact()
    assert _snapshot(tmp_path / "s") == before and len(store.segments) == 2
    store.close(compact=False)
    after = _snapshot(tmp_path / "s")
    before.pop(".lock")
    assert after == before


def test_store_compacts_at_close_above_eight_segments(tmp_path):
    rng = np.random.default_rng(9)
    keys, scores = make_keys(rng, 900), make_scores(rng, 900)
    store = _store(tmp_path / "s")
    for i in range(9):
        _append(store, keys, scores, np.arange(i, 900, 9))
    assert len(store.segments) == 9
    store.close()
    meta = json.loads((tmp_path / "s" / "meta.json").read_text())
    assert [s["entries"] for s in meta["segments"]] == [900]
    store = _store(tmp_path / "s")
    _, q, p, s = store.segments[0]
    assert np.array_equal(q.cpu().numpy(), keys[:, 0]) and np.array_equal(p.cpu().numpy(), keys[:, 1])
    assert np.array_equal(_bits(s), scores.view(np.uint32))
    store.close()


def test_store_refuses_a_damaged_segment(tmp_path):
    from cldrd_amd.retriever.score_store import ScoreStoreError
    rng = np.random.default_rng(10)
    keys, scores = make_keys(rng, 100), make_scores(rng, 100)
    store = _store(tmp_path / "s")
    _append(store, keys, scores, np.arange(100))
    name = store.segments[0][0]
    store.close()
    for part in "qp":                                               # entry 41 becomes a copy of entry 40's key: not STRICTLY ascending
        a = np.load(tmp_path / "s" / f"{name}.{part}.npy")
        a[41] = a[40]
        np.save(tmp_path / "s" / f"{name}.{part}.npy", a)
    with pytest.raises(ScoreStoreError, match=name):
        _store(tmp_path / "s")
    assert not (tmp_path / "s" / ".lock").exists()


# ---------------------------------------------------------------- rerank_top_passages --score_store
class Counter:
    """counts the pairs that reach CrossEncoder.score_cached"""

    def __init__(self, monkeypatch):
        from cldrd_amd.models.cross_encoder import CrossEncoder
        self.pairs = 0
        inner = CrossEncoder.score_cached

        def counted(model, q_cache, p_cache, q_rows, p_rows, *a, **kw):
            self.pairs += len(q_rows)
            return inner(model, q_cache, p_cache, q_rows, p_rows, *a, **kw)
        monkeypatch.setattr(CrossEncoder, "score_cached", counted)

    def take(self):
        n, self.pairs = self.pairs, 0
        return n


def _entries(store_dir):
    return sum(s["entries"] for s in json.loads((store_dir / "meta.json").read_text())["segments"])


@pytest.fixture(scope="module")
def rerank(tmp_path_factory):
    """The fixture shape of tests/test_gpu_rerank.py's full-size command-line test (a d = 768, 2-layer teacher, 40 queries x 60, --max_len
    96), file A of the run without a store, and a second run file that keeps each query's first 30 candidates and replaces the other 30."""
    from cldrd_amd.retriever import rerank_top_passages as R
    tmp = tmp_path_factory.mktemp("rerank_store")
    tok = make_pair_tokenizer()
    tok_dir = str(tmp / "tok")
    tok.save_pretrained(tok_dir)
    model_dir = _save(_hf_model("bert", 768, 2, 1, seed=13, vocab=tok.vocab_size + 4), tmp, "teacher")
    other_dir = _save(_hf_model("bert", 768, 2, 1, seed=14, vocab=tok.vocab_size + 4), tmp, "other_teacher")
    q_path, c_path, run_path = _toy_files(tmp, n_q=40, n_p=400, per_q=60)
    by_q = {}
    for line in run_path.read_text().splitlines():
        q, p = line.split("\t")[:2]
        if int(p) not in by_q.setdefault(int(q), []):
            by_q[int(q)].append(int(p))
    rng = np.random.default_rng(77)
    lines = []
    for q, ps in by_q.items():
        assert len(ps) == 60
        fresh = rng.choice(np.setdiff1d(np.arange(5000, 5400), ps), 30, replace=False)
        lines += [f"{q}\t{p}\t{r + 1}\t0.0\n" for r, p in enumerate(ps[:30] + fresh.tolist())]
    run2 = tmp / "run2.tsv"
    run2.write_text("".join(lines))

    def run(out, run_file=run_path, store=None, model=model_dir, max_len=96, extra=(), on_batch=None):
        argv = ["--run_path", str(run_file), "--queries_path", str(q_path), "--collection_path", str(c_path), "--model_name_or_path", model,
                "--tokenizer_name_or_path", tok_dir, "--max_len", str(max_len), "--token_cache_dir", str(tmp / "cache"),
                "--output_path", str(tmp / out)] + (["--score_store", str(store)] if store else []) + list(extra)
        R.main(R.get_args(argv), on_batch=on_batch)
        return (tmp / out).read_bytes()
    file_a = run("a.tsv")
    assert len(file_a.splitlines()) == 2400
    return dict(tmp=tmp, run=run, a=file_a, run2=run2, other=other_dir)


def test_rerank_cold_warm_and_partial(rerank, monkeypatch, capsys):
    count = Counter(monkeypatch)
    tmp, run = rerank["tmp"], rerank["run"]
    store = tmp / "store"
    assert run("cold.tsv", store=store) == rerank["a"]                                  # (b) cold
    assert count.take() == 2400 and _entries(store) == 2400
    assert "2400 pairs, 0 hits, 2400 scored, 1 segments" in capsys.readouterr().out
    assert run("warm.tsv", store=store) == rerank["a"]                                  # (c) warm
    assert count.take() == 0 and _entries(store) == 2400
    assert "2400 pairs, 2400 hits, 0 scored, 1 segments" in capsys.readouterr().out
    want = run("run2.plain.tsv", run_file=rerank["run2"])                               # (d) half of every query's candidates are new
    assert count.take() == 2400
    assert run("run2.store.tsv", run_file=rerank["run2"], store=store) == want
    assert count.take() == 1200 and _entries(store) == 3600
    assert not (store / ".lock").exists()


def test_rerank_restarts_after_a_flush(rerank, monkeypatch):
    """(e) the job stopped between two batches after its first flush: what it flushed is kept, the re-run scores exactly the rest"""
    count = Counter(monkeypatch)
    tmp, run = rerank["tmp"], rerank["run"]
    store = tmp / "store_restart"
    calls = []

    class Stop(Exception):
        pass

    def on_batch(n):
        calls.append(n)
        if len(calls) == 2:          # the first chunk of 500 is flushed before the second chunk's batch is scored
            raise Stop
    with pytest.raises(Stop):
        run("never.tsv", store=store, extra=["--score_store_flush_pairs", "500"], on_batch=on_batch)
    assert not (tmp / "never.tsv").exists() and not (store / ".lock").exists()
    kept = _entries(store)
    assert 500 <= kept < 2400
    count.take()
    assert run("restart.tsv", store=store, extra=["--score_store_flush_pairs", "500"]) == rerank["a"]
    assert count.take() == 2400 - kept and _entries(store) == 2400
    assert len(json.loads((store / "meta.json").read_text())["segments"]) <= 8          # 5 segments: below the compaction threshold


def test_rerank_refuses_another_teacher_and_another_max_len(rerank, monkeypatch):
    """(f) refused before a pair is scored"""
    from cldrd_amd.retriever.score_store import ScoreStoreError
    count = Counter(monkeypatch)
    tmp, run = rerank["tmp"], rerank["run"]
    store = tmp / "store_identity"
    assert run("id.tsv", store=store) == rerank["a"]
    count.take()
    before = _snapshot(store)
    with pytest.raises(ScoreStoreError, match="teacher_sha256="):
        run("id2.tsv", store=store, model=rerank["other"])
    with pytest.raises(ScoreStoreError, match="max_len="):
        run("id3.tsv", store=store, max_len=80)
    assert count.take() == 0 and _snapshot(store) == before


# ---------------------------------------------------------------- build_stage_file --score_store
def test_stage_job_with_store_writes_the_same_files(stage, monkeypatch, capsys):  # noqa: F811
    """Cold and fully warm (the fixture's teacher is tiny, d = 128: partial hits are covered at d = 768 above), and the store the job
    filled serves rerank_top_passages."""
    from cldrd_amd.retriever import build_stage_file as B
    from cldrd_amd.retriever import rerank_top_passages as R
    count = Counter(monkeypatch)
    tmp = stage["tmp"]
    store = tmp / "score_store"
    cut = ["--label_mode", "9", "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "5", "--with_scores"]

    def job(tag, extra=()):
        out = [tmp / f"ss.{tag}.json", tmp / f"ss.{tag}.student.run", tmp / f"ss.{tag}.teacher.run"]
        assert B.main(B.get_args(stage["job"] + cut + ["--output_path", str(out[0]), "--student_run_path", str(out[1]),
                                                       "--teacher_run_path", str(out[2])] + list(extra))) == (N_Q, 0)
        return [f.read_bytes() for f in out]
    want = job("plain")
    assert count.take() == N_Q * TOP and "score_store_lookup_s" not in B.main.last_timings
    assert want[2] == stage["teacher_run"].read_bytes()
    assert job("cold", ["--score_store", str(store)]) == want
    assert count.take() == N_Q * TOP and _entries(store) == N_Q * TOP
    assert {"score_store_lookup_s", "score_store_append_s", "teacher_score_s"} <= set(B.main.last_timings)
    assert job("warm", ["--score_store", str(store)]) == want
    assert count.take() == 0
    assert f"{N_Q * TOP} pairs, {N_Q * TOP} hits, 0 scored, 1 segments" in capsys.readouterr().out
    # the other program, same teacher, max_len and tables: every pair is in the store
    out = tmp / "ss.rerank.run"
    R.main(R.get_args(["--run_path", str(stage["run"]), "--queries_path", str(stage["q_path"]), "--collection_path", str(stage["c_path"]),
                       "--model_name_or_path", stage["job"][stage["job"].index("--teacher_name_or_path") + 1],
                       "--tokenizer_name_or_path", stage["job"][stage["job"].index("--teacher_tokenizer_name_or_path") + 1],
                       "--max_len", "64", "--output_path", str(out), "--score_store", str(store)]))
    assert count.take() == 0 and out.read_bytes() == stage["teacher_run"].read_bytes()
