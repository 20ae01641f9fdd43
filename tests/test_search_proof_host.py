"""The corpora of tests/test_gpu_search_proof.py held to their own claims, with numpy alone (no kernel runs here): the symmetric families have
a column mean of exactly 0, the emulated fp16 scan (fp16 operands, exact products, fp32 running sum) stays inside ``eps_ref`` on every family
and spends more than half of it on the aligned one, and on the inversion corpus the exact top-64 is group A while the emulated scan ranks
every B row above every A row by MORE than one eps - so a select with a one-eps band would lose A.

Both inversion widths are the ones the issue names first, d = 128 and d = 768: the trim construction keeps the gap above 1.0 at d = 768
(1.1; the bound's accumulation term d 2^-22 grows with d and takes the rest), so the d = 256 substitute is not needed."""
import numpy as np
import pytest

from test_gpu_search_proof import (FAMILIES, INVERSION_WIDTHS, N_A, N_B, SYMMETRIC, corpus, eps_ref, host_premise, inversion_corpus,
                                   inversion_figures, max_norm_ref, scan_emulated)


def test_restatements_on_hand_values():
    # eps_ref, term by term, at |q| = 2, pmax = 3, d = 256 (every factor a power of two or a small integer: exact in fp64)
    e = 6.0 * (2.0 ** -10 + 2.0 ** -22 + 256 * 2.0 ** -22) + 2.0 ** -14 * 16.0 * 5.0 + 256 * 2.0 ** -28
    assert eps_ref(2.0, 3.0, 256)[0] == np.float32(e * (1.0 + 1e-6))
    assert eps_ref(np.float32([2.0, 2.0]), 3.0, 256).shape == (2,)
    assert eps_ref(0.0, 0.0, 4)[0] == np.float32(4 * 2.0 ** -28 * (1.0 + 1e-6)) + np.float32(1e-30)
    # max_norm_ref: rows (3, 4, 0, 0) and (0, 0, 0, 1), mu = (0, 0, 0, 1): centred norms 5.099.. and 0, raw norms 5 and 1
    P = np.float32([[3, 4, 0, 0], [0, 0, 0, 1]])
    mu = np.float32([0, 0, 0, 1])
    assert max_norm_ref(P, mu) == np.sqrt(float(np.float32(26.0))) * (1.0 + 1e-6) + 5.0 * 2.0 ** -12
    # scan_emulated: operands rounded to fp16 (1 + 2^-11 is a tie -> even: 1; 1 + 3 2^-11 -> 1 + 2^-9), the running sum in fp32 (2^24 + 1 is lost)
    s = scan_emulated(np.float32([1 + 2.0 ** -11, 1.0]), np.float32([[1.0, 1 + 3 * 2.0 ** -11], [4096.0, 1.0]]))
    assert s.dtype == np.float32 and s[0, 0] == np.float32(2 + 2.0 ** -9)
    assert scan_emulated(np.float32([4096.0, 1.0, 1.0]), np.float32([[4096.0, 1.0, 1.0]]))[0, 0] == np.float32(2.0 ** 24)


@pytest.mark.parametrize("d", [128, 384, 768, 1024])
@pytest.mark.parametrize("family", FAMILIES)
def test_emulated_scan_stays_inside_eps(family, d):
    P, Q = corpus(family, 2048, d, 16)
    assert P.dtype == np.float32 and Q.dtype == np.float32 and P.shape == (2048, d)
    mu, eps, ratio = host_premise(P, Q)
    if family in SYMMETRIC:
        assert np.array_equal(P[0::2], -P[1::2])
        assert np.all(P.astype(np.float64).sum(axis=0) == 0.0) and np.all(mu == 0)          # exactly: no rounding anywhere in the sum
    else:
        assert np.linalg.norm(mu) > 39.0
    print(f"emulated scan, {family} d={d}: max |scan - exact| / eps = {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    if family in ("aligned",):
        assert ratio.max() >= 0.5              # or the builder has turned into a Gaussian one (those reach 0.01 - 0.07)


def test_below_normal_family_is_below_the_fp16_normal_range():
    """every row element is an fp16 subnormal; flushed to zero, the whole score is the error, and it is 0.90 of eps"""
    P, Q = corpus("below_normal", 2048, 128, 16)
    p16 = P.astype(np.float16)
    assert np.all(np.abs(p16.astype(np.float32)) < 2.0 ** -14) and np.all(p16 != 0)
    mu, eps, _ = host_premise(P, Q)
    flushed = np.abs(Q.astype(np.float64) @ P.astype(np.float64).T).max() / float(eps[0])
    print(f"below-normal family: ratio if the scan flushes the rows to zero = {flushed:.4f}")
    assert 0.85 <= flushed <= 1.0


@pytest.mark.parametrize("d", INVERSION_WIDTHS)
def test_inversion_corpus_inverts_the_scan_by_more_than_one_eps(d):
    inv = inversion_corpus(d)
    P, q, A, B, eps = inv["P"], inv["q"], inv["A"], inv["B"], inv["eps"]
    n = P.shape[0]
    assert n == 16384 and P.dtype == np.float32 and len(A) == N_A and len(B) == N_B
    assert np.all(P.astype(np.float64).sum(axis=0) == 0.0)                           # mu == 0 exactly
    h = d // 2
    for g, lo in ((A, 0), (B, h)):                                                   # a group lives on its half; trim positions are fp16 values
        assert np.all(P[g][:, h - lo:d - lo] == 0) and np.all(P[g][:, lo:lo + h - 4] != 0)
        t = P[g][:, lo + h - 4:lo + h]
        assert np.array_equal(t.astype(np.float16).astype(np.float32), t) and np.all((np.abs(t) >= 2.0 ** -14) | (t == 0))
    tq = np.concatenate([q[h - 4:h], q[d - 4:]])
    assert np.array_equal(tq.astype(np.float16).astype(np.float32), tq) and np.all(np.abs(tq) >= 2.0 ** -14)
    exact, scan, (gap_exact, gap_scan, gap_err) = inversion_figures(inv)
    top = np.lexsort((np.arange(n), -exact))[:N_A]
    assert np.array_equal(top, A)                                                    # the exact top-64 is A, in A's order
    assert 0.01 <= gap_exact <= 0.05
    assert np.all(np.diff(exact[A].astype(np.float32)) < 0)                          # distinct as fp32 scores too: the oracle's order is strict
    top_scan = np.argsort(-scan, kind="stable")[:N_A]
    assert len(np.intersect1d(top_scan, A)) == 0 and np.all(np.isin(top_scan, B))    # the scan's top-64: B rows only
    worst = np.abs(scan - exact).max() / eps
    _, _, (_, gap16_scan, gap16_err) = inversion_figures(inv, fp16_rows=True)
    print(f"inversion corpus d={d}: eps = {eps:.4f}, least exact A - B gap = {gap_exact:.4f} eps, max |scan - exact| = {worst:.4f} eps, "
          f"inversion gap min scan(B) - max scan(A) = {gap_scan:.4f} eps (min err B - max err A = {gap_err:.4f} eps); "
          f"fp16-row mode (only q rounds): min err B - max err A = {gap16_err:.4f} eps")
    assert worst <= 1.0
    assert gap_scan > 1.0 and gap_err > 1.0                                          # a one-eps band under t^ (a B score) holds no A row
    assert gap_scan < 2.0                                                            # and the two-eps band holds them all
