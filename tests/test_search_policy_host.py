"""The host arithmetic of ``FlatIPIndex.search_device`` - what a failed proof does to a threshold (``_retry_step``), the kept-set buffer after
the probe pass (``_cap2_after_probe``) - and the states of an index that is not on a GPU.  No GPU needed."""
import numpy as np
import pytest

from cldrd_amd.retriever import retrieval_utils as RU

CAP = RU.CAND_CAP


def _cases(seed, n):
    """random finite inputs: status 0..31, thresholds and k-th scores of either sign over six decades, eps > 0"""
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 32, n).astype(np.int32)
    thr = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
    khat = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
    khat[rng.random(n) < 0.05] = -np.inf                      # a list shorter than k has no k-th score
    eps = 10.0 ** rng.uniform(-6, 0, n)
    return status, thr, eps, khat


@pytest.mark.parametrize("attempt", range(1, 13))
def test_retry_step(attempt):
    """The "lowered by no more than" bar holds for the step the policy computes.  The test sees ``t_old - t_new``: the policy's subtraction and
    the test's own each round once in fp64 (half an ulp of the larger of |t_old|, |t_new| each), so that difference may sit up to ONE such
    ulp above the bar (2^-52 relative; measured: at most 1.0 ulp, on the queries whose step is the cap itself) - that much room and no more."""
    status, thr, eps, khat = _cases(100 + attempt, 20000)
    before = (status.copy(), thr.copy(), eps.copy(), khat.copy())
    t, tiled, full = RU._retry_step(status, thr, eps, khat, attempt)
    for a, b in zip(before, (status, thr, eps, khat)):
        assert np.array_equal(a, b)                           # a pure function
    assert t.dtype == np.float64 and t.shape == thr.shape
    over = (status & 2) != 0
    few = ((status & 1) != 0) & ~over                         # precedence: overflow over too-few over too-high
    high = ((status & 8) != 0) & ~over & ~few
    keep = ~(over | few | high)                               # only bit 4 and / or bit 16 (or nothing)
    assert over.any() and few.any() and high.any() and keep.any()
    finite = np.isfinite(khat)
    # too high only: as the float32 the device gets, strictly below khat - 2 eps
    hf = high & finite
    assert np.all(t[hf].astype(np.float32).astype(np.float64) < khat[hf] - 2.0 * eps[hf])
    # too few: strictly lower, by no more than 8 eps attempt + 0.2 |t| + 1e-3
    assert np.all(t[few] < thr[few])
    ulp = np.spacing(np.maximum(np.abs(thr[few]), np.abs(t[few])))
    assert np.all(thr[few] - t[few] <= 8.0 * eps[few] * attempt + 0.2 * np.abs(thr[few]) + 1e-3 + ulp)
    # overflow: strictly higher, and at least khat - 2 eps when there is a k-th score
    assert np.all(t[over] > thr[over])
    of = over & finite
    assert np.all(t[of] >= khat[of] - 2.0 * eps[of])
    # only bit 4 / 16: the threshold stays
    assert np.array_equal(t[keep], thr[keep])
    assert tiled is True and full is True                     # 20 000 random status words: both bits occur
    for bits, want in ((np.array([1, 2, 8, 11, 16, 27]), (False, True)), (np.array([4, 1, 9]), (True, False)), (np.array([1, 2, 8]), (False, False)),
                       (np.array([20]), (True, True))):
        m = bits.size
        _, tiled, full = RU._retry_step(bits.astype(np.int32), thr[:m], eps[:m], khat[:m], attempt)
        assert (tiled, full) == want, bits


def test_retry_step_precedence_on_one_query():
    thr, eps, khat = np.array([5.0]), np.array([0.01]), np.array([4.0])
    one = lambda s: float(RU._retry_step(np.array([s], dtype=np.int32), thr, eps, khat, 1)[0][0])
    assert one(2) == one(3) == one(2 | 8) == one(1 | 2 | 8) > 5.0          # overflow wins
    assert one(1) == one(1 | 8) < 5.0 and one(1) != one(8)                  # then too few
    assert one(8) < 4.0 - 0.02                                              # then too high: below khat - 2 eps
    assert one(4) == one(16) == one(20) == one(0) == 5.0


def test_cap2_after_probe():
    """The headroom bar is ``int(1.25 need) + 64``, the formula's own truncation: at need = 3226 that is 4096, half a slot under
    1.25 need + 64 = 4096.5, and 4096 slots is what the search has always taken there."""
    rng = np.random.default_rng(7)
    clean = np.zeros(128, dtype=np.int32)
    for cap2 in (1024, 2048, 4096, CAP):
        needs = np.unique(np.concatenate([rng.integers(0, CAP + 1, 300), [0, 1, 767, 768, 769, 1586, 1587, 3225, 3226, 3227, 6502, 6503, CAP]]))
        for need in needs.tolist():
            kept = rng.integers(0, need + 1, 128).astype(np.int32)
            kept[int(rng.integers(0, 128))] = need
            got = RU._cap2_after_probe(cap2, clean, kept)
            ratio = got // cap2
            assert got % cap2 == 0 and ratio & (ratio - 1) == 0 and ratio >= 1                 # a power-of-two multiple of the input
            assert min(CAP, int(1.25 * need) + 64) <= got <= CAP
            if int(1.25 * need) + 64 <= cap2:
                assert got == cap2                                                          # the need already fits
            elif got < CAP:
                assert got // 2 < int(1.25 * need) + 64                                     # and no larger than it has to be
            st = clean.copy()
            st[5] = 16 | int(rng.integers(0, 16))                                              # one kept set did not fit
            assert RU._cap2_after_probe(cap2, st, kept) == CAP
            st[5] = int(rng.integers(0, 16))                                                   # other bits do not size the buffer
            assert RU._cap2_after_probe(cap2, st, kept) == got


def test_multi_device_index_without_rows_answers_all_missing():
    d, nq = 16, 3
    index = RU.FlatIPIndex(d)
    index.add(np.zeros((0, d), dtype=np.float32))
    multi = RU.MultiDeviceFlatIPIndex(index, [0, 0])
    assert multi.ntotal == 0 and all(sh.device is None for sh in multi.shards)
    D, I = multi.search(np.ones((nq, d), dtype=np.float32), 5)
    assert D.shape == I.shape == (nq, 5) and D.dtype == np.float32 and I.dtype == np.int64
    assert np.all(np.isneginf(D)) and np.all(I == -1)
    D0, I0 = multi.search(np.ones((0, d), dtype=np.float32), 5)
    assert D0.shape == I0.shape == (0, 5)


def test_host_index_has_no_resident_state():
    d = 16
    index = RU.FlatIPIndex(d)
    rows = np.random.default_rng(1).standard_normal((10, d)).astype(np.float32)
    for _ in range(2):
        assert index.device is None and index.row_dtype == "float32" and index.mu is None
        with pytest.raises(RuntimeError, match="not on a GPU"):
            index.search(rows[:2], 3)
        index.add(rows)
