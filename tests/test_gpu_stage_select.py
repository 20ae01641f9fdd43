"""The device selection of a curriculum stage (``cldrd_curriculum_select`` through ``dataset.curriculum_file.select_examples_device``)
against the host selection (``select_examples``) on the equivalent in-memory ``TeacherRun``: every array of ``CurriculumExamples`` equal,
``n_skipped`` equal, ``order`` equal to the host lexsort.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd.dataset import curriculum_file as C

pytestmark = pytest.mark.gpu

NQ = 37
DEV = "cuda"


def _spec(n_rel, n_most, n_semi, most, semi):
    return C.CurriculumSpec("test", n_rel, n_most, n_semi, most, semi)


# per K: the label modes 9, 8 (12 + 13), 3 (no semi-hard) and 6 (no negatives) where K holds them; every K has a window that ends exactly
# at K and one of exactly n ranks.  K = 1 holds no label mode: a one-relT spec, and mode 6 there skips every query.
SPECS = {
    1: [_spec(1, 0, 0, (2, 2), (3, 3)), C.curriculum_spec("6")],
    63: [C.curriculum_spec("9", "11:20", "21:63"), C.curriculum_spec("8", "6:30", "51:63"), C.curriculum_spec("3", "11:63"),
         C.curriculum_spec("6")],
    64: [C.curriculum_spec("9", "11:20", "21:64"), C.curriculum_spec("8", "6:17", "18:64"), C.curriculum_spec("3", "45:64"),
         C.curriculum_spec("6")],
    65: [C.curriculum_spec("9", "56:65", "11:40"), C.curriculum_spec("8", "6:40", "41:65"), C.curriculum_spec("3", "11:65"),
         C.curriculum_spec("6")],
    200: [C.curriculum_spec("9"), C.curriculum_spec("8", "6:100", "188:200"), C.curriculum_spec("3", "11:200", "201:300"),
          C.curriculum_spec("6")],
    1024: [C.curriculum_spec("9", "11:500", "501:1024"), C.curriculum_spec("8", "1000:1011", "6:999"), C.curriculum_spec("3", "300:1024"),
           C.curriculum_spec("6")],
}
CASES = [(K, i) for K in SPECS for i in range(len(SPECS[K]))]


def _ids(K, rng):
    """qid int64 [NQ], pid int64 [NQ, K]: negative ids and ids above 2^40, the pids of a row distinct, in no order"""
    qid = np.arange(NQ, dtype=np.int64) * 13 - 100 + (np.arange(NQ) % 3 == 1) * (1 << 42)
    pid = np.stack([rng.permutation(K) for _ in range(NQ)]).astype(np.int64) * 7919 - 3000
    pid += (np.arange(NQ)[:, None] % 2) * (1 << 41) + (rng.integers(0, 2, (NQ, K)) * (1 << 43))
    return qid, pid


def _scores(kind, K, rng):
    if kind == "ties4":
        return rng.choice(np.array([-1.5, 0.25, 0.75, 3.0], dtype=np.float32), (NQ, K))
    if kind == "equal":
        return np.full((NQ, K), 1.5, dtype=np.float32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 0.5, -0.5], dtype=np.float32), (NQ, K))
    return rng.standard_normal((NQ, K)).astype(np.float32)


def _counts(kind, K, need, rng):
    full = np.full(NQ, K, dtype=np.int32)
    if kind == "full":
        return full
    if kind == "min":
        return np.full(NQ, min(need, K), dtype=np.int32)
    if kind == "below":
        return np.full(NQ, max(0, min(need, K + 1) - 1), dtype=np.int32)
    if kind == "zero":
        return np.zeros(NQ, dtype=np.int32)
    pool = np.array([K, min(need, K), max(0, min(need, K + 1) - 1), 0, int(rng.integers(0, K + 1))], dtype=np.int32)
    return pool[rng.integers(0, pool.shape[0], NQ)]


def _garbage(pid, score, count):
    """positions >= count: NaN scores, ids that repeat a live pid and each other"""
    pid, score = pid.copy(), score.copy()
    dead = np.arange(pid.shape[1])[None, :] >= count[:, None]
    score[dead] = np.nan
    pid[dead] = np.broadcast_to(pid[:, :1], pid.shape)[dead]
    return pid, score


def _host(qid, pid, score, count, spec, seed, with_scores):
    """select_examples on the equivalent TeacherRun (lines in row order, rank column 1 .. count) and the host lexsort as [NQ, K] positions"""
    K = pid.shape[1]
    live = np.arange(K)[None, :] < count[:, None]
    at_q, at_j = np.nonzero(live)
    run = C.TeacherRun(qid[at_q], pid[at_q, at_j], at_j.astype(np.int64) + 1, score[at_q, at_j].astype(np.float64))
    ex = C.select_examples(run, spec, seed, with_scores=with_scores)
    line = np.lexsort((run.rank, -run.score, at_q))
    starts = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    order = np.full(pid.shape, -1, dtype=np.int32)
    order[at_q, at_j] = line - starts[at_q]
    return ex, order


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _assert_examples_equal(got, want, with_scores):
    assert got.n_skipped == want.n_skipped
    names = ("qid", "relT", "most_hard", "semi_hard") + (("relT_scores", "most_hard_scores", "semi_hard_scores") if with_scores else ())
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name
    if not with_scores:
        assert got.relT_scores is None and got.most_hard_scores is None and got.semi_hard_scores is None


@pytest.mark.parametrize("K,which", CASES)
def test_device_selection_equals_host_selection(K, which):
    spec = SPECS[K][which]
    rng = np.random.default_rng(1000 * K + which)
    qid, pid = _ids(K, rng)
    kept_somewhere = False
    for s_kind in ("ties4", "equal", "zeros", "normal"):
        score = _scores(s_kind, K, rng)
        for c_kind in ("full", "min", "below", "zero", "mix"):
            count = _counts(c_kind, K, spec.min_candidates, rng)
            with_scores = c_kind in ("full", "mix")
            want, want_order = _host(qid, pid, score, count, spec, 5, with_scores)
            pid_g, score_g = _garbage(pid, score, count)
            got, order = C.select_examples_device(*_dev(qid, pid_g, score_g, count), spec, seed=5, with_scores=with_scores)
            _assert_examples_equal(got, want, with_scores)
            assert order.dtype == torch.int32 and order.is_cuda
            assert np.array_equal(order.cpu().numpy(), want_order), (s_kind, c_kind)
            kept_somewhere |= want.qid.shape[0] > 0
    assert kept_somewhere == (spec.min_candidates <= K)


def test_seed_changes_the_negatives_and_nothing_else():
    spec = C.curriculum_spec("9")
    rng = np.random.default_rng(3)
    qid, pid = _ids(200, rng)
    t = _dev(qid, pid, _scores("normal", 200, rng), np.full(NQ, 200, dtype=np.int32))
    a, order_a = C.select_examples_device(*t, spec, seed=1)
    b, order_b = C.select_examples_device(*t, spec, seed=2)
    a2, _ = C.select_examples_device(*t, spec, seed=1)
    assert np.array_equal(a.relT, b.relT) and torch.equal(order_a, order_b)
    assert not np.array_equal(a.most_hard, b.most_hard) and not np.array_equal(a.semi_hard, b.semi_hard)
    assert np.array_equal(a.most_hard, a2.most_hard) and np.array_equal(a.semi_hard, a2.semi_hard)
    want, _ = _host(qid, pid, t[2].cpu().numpy(), np.full(NQ, 200, dtype=np.int32), spec, 2, False)
    assert np.array_equal(b.most_hard, want.most_hard) and np.array_equal(b.semi_hard, want.semi_hard)


def test_dead_positions_and_skipped_rows_are_isolated():
    """positions >= count change no output; rows with keep == 0 leave sel_pid / sel_score as they were"""
    from cldrd_amd import hip_ops as ops
    spec = C.curriculum_spec("8", "6:30", "31:65")
    rng = np.random.default_rng(11)
    K = 65
    qid, pid = _ids(K, rng)
    score = _scores("ties4", K, rng)
    count = _counts("mix", K, spec.min_candidates, rng)
    count[:4] = [K, spec.min_candidates - 1, 0, K]
    pid_g, score_g = _garbage(pid, score, count)
    outs = []
    for p, s in ((pid, score), (pid_g, score_g)):
        sel_pid = torch.full((NQ, 30), -77, dtype=torch.int64, device=DEV)
        sel_score = torch.full((NQ, 30), -7.5, dtype=torch.float32, device=DEV)
        outs.append(ops.curriculum_select(*_dev(qid, p, s, count), spec.n_rel, spec.n_most_hard, spec.most_hard_ranks, spec.n_semi_hard,
                                          spec.semi_hard_ranks, 9, sel_pid=sel_pid, sel_score=sel_score))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    order, keep, sel_pid, sel_score = outs[1]
    keep_h = keep.cpu().numpy()
    assert np.array_equal(keep_h, (count >= spec.min_candidates).astype(np.int32)) and 0 < keep_h.sum() < NQ
    assert (sel_pid.cpu().numpy()[keep_h == 0] == -77).all() and (sel_score.cpu().numpy()[keep_h == 0] == -7.5).all()
    assert (sel_pid.cpu().numpy()[keep_h == 1] != -77).all()
    assert (order.cpu().numpy()[np.arange(K)[None, :] >= count[:, None]] == -1).all()


def test_long_lists_take_the_host_path():
    spec = C.curriculum_spec("9", "11:100", "101:1100")
    rng = np.random.default_rng(17)
    K = 1100
    qid, pid = _ids(K, rng)
    score = _scores("ties4", K, rng)
    count = _counts("mix", K, spec.min_candidates, rng)
    count[0] = K
    want, want_order = _host(qid, pid, score, count, spec, 4, True)
    pid_g, score_g = _garbage(pid, score, count)
    got, order = C.select_examples_device(*_dev(qid, pid_g, score_g, count), spec, seed=4, with_scores=True)
    _assert_examples_equal(got, want, True)
    assert order.is_cuda and order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), want_order)


def test_refusals():
    from cldrd_amd import hip_ops as ops
    from cldrd_amd._lib import CldrdError
    spec = C.curriculum_spec("9", "11:30", "31:64")
    rng = np.random.default_rng(19)
    qid, pid = _ids(64, rng)
    score = _scores("normal", 64, rng)
    count = np.full(NQ, 64, dtype=np.int32)
    bad = score.copy()
    bad[5, 63] = np.nan
    bad[9, 0] = np.inf
    with pytest.raises(ValueError, match=f"qid {qid[5]}"):
        C.select_examples_device(*_dev(qid, pid, bad, count), spec)
    short = count.copy()
    short[5] = 63                    # the NaN is no longer live; the inf of row 9 is
    with pytest.raises(ValueError, match=f"qid {qid[9]}"):
        C.select_examples_device(*_dev(qid, pid, bad, short), spec)

    def select(q, p, s, c):
        return ops.curriculum_select(q, p, s, c, spec.n_rel, spec.n_most_hard, spec.most_hard_ranks, spec.n_semi_hard, spec.semi_hard_ranks, 0)

    q, p, s, c = _dev(qid, pid, score, count)
    with pytest.raises(RuntimeError):
        select(q.cpu(), p, s, c)
    with pytest.raises(RuntimeError):
        select(q, p, s.cpu(), c)
    with pytest.raises(RuntimeError):
        C.select_examples_device(q, p.cpu(), s, c, spec)
    with pytest.raises(TypeError):
        select(q.int(), p, s, c)
    with pytest.raises(TypeError):
        select(q, p, s.double(), c)
    with pytest.raises(TypeError):
        select(q, p, s, c.long())
    with pytest.raises(ValueError):
        select(q, p.t().contiguous().t(), s, c)
    with pytest.raises(ValueError):
        select(q[:-1], p, s, c)
    qid2, pid2 = _ids(1025, rng)
    with pytest.raises(CldrdError, match="1024"):
        select(*_dev(qid2, pid2, _scores("normal", 1025, rng), np.full(NQ, 1025, dtype=np.int32)))
