"""int8-row index mode on the MI355X (``to_gpu(dev, int8_rows=True)`` / int8-row files / ``--index_int8`` / ``--use_int8``).

The oracle is the mode's definition restated in numpy (tests/test_index_int8_host.py): the quantiser, the query digits and the pinned scan score
``s^ = fmaf(128, (float)H, (float)L) * (sq * a_r)`` are compared BIT FOR BIT, the search against the definition's top-k from the index's own
``mu`` with the bars of tests/test_gpu_retrieval.py (``same_ranking``).  Integer products go through float64 matmul (exact here)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops
import selftest
from cldrd_amd.retriever import retrieval_utils as RU
from test_gpu_retrieval import same_ranking, _run_cli
from test_index_int8_host import (F32, adversarial_queries, bound_norms_ref, centred_exact, cls_like_rows, digits_ref, eps_ref, heavy_rows, oracle8,
                                  qnorm_ref, quantize_ref, scan_ref, special_rows)

DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_mu(index, P):
    mu64 = np.asarray(P, dtype=np.float64).mean(axis=0)
    mu = np.asarray(index.mu)
    assert mu.dtype == np.float32 and not index.mu.flags.writeable
    assert np.max(np.abs(mu.astype(np.float64) - mu64)) <= 1e-6 * np.max(np.abs(mu64))
    return mu


def attach8(P, ids=None, id_offset=0, **hooks):
    index = RU.FlatIPIndex(P.shape[1])
    index.add_with_ids(P, ids)
    index.id_offset = id_offset
    for k_, v_ in hooks.items():
        setattr(index, k_, v_)
    out = index.to_gpu(0, int8_rows=True)
    assert out is index and index.row_dtype == "int8" and index._p32 is None and index._p16 is None          # no fp32 or fp16 row tensor
    assert index._res.r8.dtype == torch.int8 and index._res.scale.shape == (P.shape[0],)
    return index


def run_scan(h, l, sq, thr, r8, a, cap):
    """cldrd_topk_scan_i8 -> (counts [nq], dropped, cand_rows [nq, cap], cand_scores [nq, cap]) on the host"""
    nq = h.shape[0]
    qd = dev(np.stack([h, l]).astype(np.int8))
    counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    rows = torch.full((nq, cap), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((nq, cap), 12345.0, device=DEV)
    ops.topk_scan_i8(qd, dev(sq.astype(F32)), dev(thr.astype(F32)), dev(r8), dev(a.astype(F32)), counts, rows, scores)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    return c[:nq], int(c[nq]), rows.cpu().numpy(), scores.cpu().numpy()


# ---- 1. the lane map of v_mfma_i32_16x16x64_i8 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [16, 17])
@pytest.mark.parametrize("d", [64, 128])
def test_lane_map(nq, d):
    """Asymmetric integers: row r is non-zero only at column (7 r + 3) mod d, value (r mod 127) + 1; the query digits differ in every column
    and query.  With sq = a = 1 the scan score is fmaf(128, H, L) exactly (|128 H + L| < 2^24): H alone (l = 0), L alone (h = 0) and both."""
    n = 64
    r8 = np.zeros((n, d), dtype=np.int8)
    r = np.arange(n)
    r8[r, (7 * r + 3) % d] = (r % 127) + 1
    j, q = np.arange(d)[None, :], np.arange(nq)[:, None]
    h = ((3 * q + 5 * j) % 255 - 127).astype(np.int8)
    l = ((7 * q + 11 * j) % 128 - 64).astype(np.int8)
    one, ninf = np.ones(nq, dtype=F32), np.full(nq, -np.inf, dtype=F32)
    H = h.astype(np.int64) @ r8.astype(np.int64).T
    L = l.astype(np.int64) @ r8.astype(np.int64).T
    assert len(np.unique(H)) > 100 and np.abs(128 * H + L).max() < 2 ** 24
    for hh, ll, want in ((h, np.zeros_like(l), 128 * H), (np.zeros_like(h), l, L), (h, l, 128 * H + L)):
        counts, dropped, rows, scores = run_scan(hh, ll, one, ninf, r8, np.ones(n, dtype=F32), n)
        assert dropped == 0 and np.all(counts == n)
        got = np.full((nq, n), np.nan)
        for qi in range(nq):
            assert sorted(rows[qi].tolist()) == list(range(n))
            got[qi, rows[qi]] = scores[qi]
        assert np.array_equal(got, want.astype(np.float64))


# ---- 2. the quantiser and the query prep, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 768, 1024])
def test_quantize_kernel_equals_the_definition(d):
    mu = ((np.arange(d) % 8 - 4) * 0.25).astype(F32)
    c_special, p_special = special_rows(d, mu)
    P = np.concatenate([heavy_rows(31 + d, 3000, d) + mu, p_special]).astype(F32)
    n = P.shape[0]
    r8_ref, a_ref = quantize_ref(P, mu)
    assert a_ref[3000] == 0 and np.count_nonzero(r8_ref[3001]) == 1 and r8_ref[3002, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]
    s_stride, s_rows = 7, (n + 6) // 7
    r8 = torch.full((n, d), 99, dtype=torch.int8, device=DEV)
    a = torch.full((n,), -1.0, device=DEV)
    sample = torch.zeros((s_rows + 7) // 8 * 8, d, dtype=torch.bfloat16, device=DEV)
    flag, b1, c2 = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
    Pd, mud = dev(P), dev(mu)
    for lo, hi in ((0, 1001), (1001, n)):                              # two chunks: the maxima and the sample accumulate
        ops.index_quantize_i8(Pd[lo:hi], mud, r8[lo:hi], a[lo:hi], sample, s_stride, s_rows, flag, b1, c2, row0=lo)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert np.array_equal(r8.cpu().numpy(), r8_ref)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), a_ref.view(np.uint32))
    b1_ref, c2_ref = bound_norms_ref(r8_ref, a_ref)
    assert b1.view(torch.float32).item() == b1_ref and c2.view(torch.float32).item() == c2_ref
    want = (torch.from_numpy(a_ref[::s_stride, None] * r8_ref[::s_stride].astype(F32))).to(torch.bfloat16)
    assert torch.equal(sample[:s_rows].cpu(), want) and not sample[s_rows:].any()
    bad = P.copy()
    bad[17, 3] = np.inf
    ops.index_quantize_i8(dev(bad), mud, r8, a, None, 1, 0, flag, b1, c2)
    assert int(flag.item()) == 1


@pytest.mark.parametrize("d", [64, 128, 768, 1024])
def test_prep_queries_i8_equals_the_definition(d):
    q = heavy_rows(41 + d, 40, d)
    q[0] = 0.0                                                         # the zero query: sq = 0, no digits
    q[1] = F32(1e-35)                                                  # below 2^-100: no digits, sq = 2 max|q|
    q[2, :8] = (np.array([16256, -16255, 64, -64, 63, -63, 0, 5]) * 2.0 ** -10).astype(F32)
    q[2, 8:] = 0.0
    q[3] = np.round(q[3] * 64) / 64                                    # many quotients near half steps
    h, l, sq = digits_ref(q)
    nq = q.shape[0]
    qd = torch.full((2, nq, d), 99, dtype=torch.int8, device=DEV)
    qb = torch.empty(nq, d, dtype=torch.bfloat16, device=DEV)
    sqd, qn, flag = torch.empty(nq, device=DEV), torch.empty(nq, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    qdev = dev(q)
    ops.topk_prep_queries_i8(qdev, qd, qb, sqd, qn, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert np.array_equal(sqd.cpu().numpy().view(np.uint32), sq.view(np.uint32))
    assert np.array_equal(qd[0].cpu().numpy(), h) and np.array_equal(qd[1].cpu().numpy(), l)
    assert torch.equal(qb.cpu(), torch.from_numpy(q).to(torch.bfloat16))
    ref = qnorm_ref(q)
    got = qn.cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(ref)) and got[0] == 0            # fp32 of an fp64 sum: one ulp for the order
    q[5, 1] = np.nan
    ops.topk_prep_queries_i8(dev(q), qd, qb, sqd, qn, flag)
    assert int(flag.item()) == 1


# ---- 3. the scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,n,d", [(1, 64, 64), (37, 5003, 128), (128, 4113, 768), (130, 9000, 1024), (256, 40000, 768), (70, 3001, 2048)])
def test_scan_emits_exactly_the_rows_above_the_threshold(nq, n, d):
    """Every query's candidate set is {r : s^ >= thr} with thr passing about 1 % of the rows, every score bit-equal to the numpy emulation;
    a cap below the hit count raises the dropped-hit counter, keeps counting, and fills the first cap slots with true hits."""
    g = np.random.default_rng(1000 + n)
    P = (g.standard_normal((n, d)) * np.exp(0.5 * g.standard_normal((n, 1)))).astype(F32)
    r8, a = quantize_ref(P, np.zeros(d, dtype=F32))
    q = g.standard_normal((nq, d)).astype(F32)
    h, l, sq = digits_ref(q)
    s = scan_ref(h, l, sq, r8, a)
    kth = max(1, n // 100)
    thr = np.partition(s, n - kth, axis=1)[:, n - kth].astype(F32)
    want = s >= thr[:, None]
    nhit = want.sum(axis=1)
    cap = int(nhit.max()) + 8
    counts, dropped, rows, scores = run_scan(h, l, sq, thr, r8, a, cap)
    assert dropped == 0 and np.array_equal(counts, nhit)
    for qi in range(nq):
        c = counts[qi]
        order = np.argsort(rows[qi, :c])
        assert np.array_equal(rows[qi, :c][order], np.nonzero(want[qi])[0])
        assert np.array_equal(scores[qi, :c][order].view(np.uint32), s[qi, want[qi]].view(np.uint32))
        assert np.all(rows[qi, c:] == -7)                              # nothing written past the list
    if nhit.max() > 4:
        small = int(nhit.max()) // 2
        counts, dropped, rows, scores = run_scan(h, l, sq, thr, r8, a, small)
        assert np.array_equal(counts, nhit) and dropped == int(np.maximum(nhit - small, 0).sum()) and dropped > 0
        for qi in range(nq):
            c = min(int(counts[qi]), small)
            assert len(set(rows[qi, :c].tolist())) == c and want[qi, rows[qi, :c]].all()
            assert np.array_equal(scores[qi, :c].view(np.uint32), s[qi, rows[qi, :c]].view(np.uint32))


# ---- 4. the re-score -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 768, 1024])
def test_rescore_i8_is_the_rounded_fp64_sum(d):
    """cldrd_topk_rescore_i8 + cldrd_query_dot64 against fp32(q.mu + a_r q.R8[row]) in numpy fp64 on ragged lists (counts 0, 1 and cap among them).
    Bit for bit except where the fp64 value lies within 1e-9 relative of an fp32 rounding boundary (the summation orders differ): at most 1 entry
    in 10 000, one ulp off - the condition of test_rescore16_is_the_rounded_fp64_sum.  First, in numpy alone: two summation orders of the
    chosen inputs differ only inside that condition."""
    n, nq, cap = 6000, 9, 1500
    g = np.random.default_rng(200 + d)
    r8, a = quantize_ref(heavy_rows(201 + d, n, d), np.zeros(d, dtype=F32))
    mu = g.standard_normal(d).astype(F32)
    q = g.standard_normal((nq, d)).astype(F32)
    cnt = g.integers(1, cap, nq).astype(np.int32)
    cnt[0], cnt[1], cnt[2] = 0, cap, 1
    cand = g.integers(0, n, (nq, cap)).astype(np.int32)
    cand[1, 0], cand[1, 1] = n - 1, 0
    q64, r64, a64 = q.astype(np.float64), r8.astype(np.float64), a.astype(np.float64)
    qmu_ref = (q64 * mu.astype(np.float64)).sum(axis=1)

    def ref64(qi, reverse):
        rows = cand[qi, :cnt[qi]]
        prod = r64[rows] * q64[qi]
        return qmu_ref[qi] + a64[rows] * (prod[:, ::-1] if reverse else prod).sum(axis=1)

    def compare(got, want64):
        """-> (entries, entries one ulp off at a boundary); anything else fails"""
        want32 = want64.astype(F32)
        bad = np.nonzero(got != want32)[0]
        for j in bad:
            g32, r32 = got[j], want32[j]
            assert g32 in (np.nextafter(r32, F32(np.inf)), np.nextafter(r32, F32(-np.inf))), (j, g32, r32)
            assert abs(want64[j] - 0.5 * (float(g32) + float(r32))) <= 1e-9 * abs(want64[j]), (j, want64[j])
        return len(want32), len(bad)
    tot = exc = 0
    for qi in range(nq):
        t_, e_ = compare(ref64(qi, True).astype(F32), ref64(qi, False))
        tot, exc = tot + t_, exc + e_
    assert exc * 10000 <= tot                                          # the inputs stay inside the condition under a change of order
    scores = torch.full((nq, cap), 12345.0, device=DEV)
    qd_ = dev(q)
    qmu = ops.query_dot64(qd_, dev(mu))
    ops.topk_rescore_i8(qd_, dev(r8), dev(a), qmu, dev(cnt), dev(cand), scores)
    torch.cuda.synchronize()
    got = scores.cpu().numpy()
    tot = exc = 0
    for qi in range(nq):
        assert np.all(got[qi, cnt[qi]:] == 12345.0)
        t_, e_ = compare(got[qi, :cnt[qi]], ref64(qi, False))
        tot, exc = tot + t_, exc + e_
    print(f"rescore_i8 d={d}: {exc} of {tot} entries one ulp off at a rounding boundary")
    assert exc * 10000 <= tot


# ---- 5. the search against the definition -----------------------------------------------------------------------------------------
def _corpus(n, d, nq, seed):
    emb = syn.corpus_embeddings(seed, n, d) + F32(0.125)
    emb[n // 2] = emb[n // 3]                                          # duplicated rows: equal stored rows, ties broken by row position
    emb[n - 1] = emb[5]
    q = syn.corpus_embeddings(seed + 1, nq, d)
    q[0] = emb[n // 3]
    if nq > 2:
        q[2] = 0.0                                                     # the zero query: every score is 0 (and <q, mu> = 0), rows 0 .. k-1
    return emb, q


@pytest.mark.parametrize("nq,n,d,with_ids", [(37, 5003, 768, True), (16, 9000, 128, False), (129, 40000, 768, True), (257, 70001, 256, False),
                                             (600, 40000, 768, False), (130, 3000, 128, False)])          # the last: exhaustive, two query tiles
def test_search_equals_the_definition(nq, n, d, with_ids):
    emb, q = _corpus(n, d, nq, 300 + nq)
    ids = np.arange(n, dtype=np.int64) * 3 + 5 if with_ids else None
    index = attach8(emb, ids, id_offset=0 if with_ids else 1000)
    assert index.query_tile == 128
    mu = check_mu(index, emb)
    r8, a = quantize_ref(emb, mu)
    res = index._res
    assert np.array_equal(res.r8.cpu().numpy(), r8) and np.array_equal(res.scale.cpu().numpy().view(np.uint32), a.view(np.uint32))
    b1, c2 = bound_norms_ref(r8, a)
    assert res.b1 == float(b1) and res.cnorm == float(np.sqrt(np.float64(c2)))
    Dr, Ir = oracle8(mu, r8, a, q, 1000, ids=ids, id_offset=1000)
    for k in (1000, 100, 10, 1):
        D, I = index.search(q, k)
        st = index.last_stats
        same_ranking(D, I, Dr[:, :k], Ir[:, :k])
        assert np.all(np.diff(D, axis=1) <= 0)
        # the zero query scores every row 0: more ties than any candidate list holds, so a scanned search serves it by the exact fallback
        assert st["exhaustive"] == (n <= RU.CAND_CAP) and st["fallback_queries"] <= (0 if st["exhaustive"] or nq <= 2 else 1), st
        if nq > 2 * 128 and not st["exhaustive"]:
            assert "cap2" in st                                        # the probe pass ran
    D, I = index.search(q, 10)
    first, second = (ids[n // 3], ids[n // 2]) if with_ids else (n // 3 + 1000, n // 2 + 1000)
    assert I[0, 0] == first and I[0, 1] == second and D[0, 0] == D[0, 1]          # exact tie: lower row first
    if nq > 2:
        assert np.all(D[2] == 0) and np.array_equal(I[2], Ir[2, :10])


def test_from_device_rows_and_width_refusals():
    n, d = 70000, 128
    P, u = syn.cls_like_corpus(n, d, 91, DEV)
    q = syn.cls_like_queries(12, u, 92).cpu().numpy()
    index = RU.FlatIPIndex.from_device_rows(P, id_offset=11, int8_rows=True)
    assert index.row_dtype == "int8" and index._p32 is None and index._p16 is None
    Ph = P.cpu().numpy()
    mu = check_mu(index, Ph)
    r8, a = quantize_ref(Ph, mu)
    D, I = index.search(q, 100)
    same_ranking(D, I, *oracle8(mu, r8, a, q, 100, id_offset=11))
    host = attach8(Ph, None, id_offset=11)                            # the same rows through the host staging buffers
    assert np.array_equal(host.mu, index.mu) and torch.equal(host._res.r8, index._res.r8) and torch.equal(host._sample, index._sample)
    for d_bad in (132, 2112):
        bad = RU.FlatIPIndex(d_bad)
        bad.add(np.ones((8, d_bad), dtype=F32))
        with pytest.raises(ValueError, match=str(d_bad)):
            bad.to_gpu(0, int8_rows=True)
        with pytest.raises(ValueError, match=str(d_bad)):
            RU.FlatIPIndex.from_device_rows(torch.ones(8, d_bad, device=DEV), int8_rows=True)
    with pytest.raises(ValueError):
        RU.FlatIPIndex.from_device_rows(P, fp16_rows=True, int8_rows=True)


def test_resident_bytes_are_d_plus_4_per_row():
    n, d = 300000, 768
    P = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) + F32(0.5)
    MB = 1 << 20
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    index = attach8(P)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    bound = n * (d + 4) + index._sample.numel() * 2 + 8 * MB
    print(f"int8-row mode: resident {grown / MB:.1f} MB (bound {bound / MB:.1f})")
    assert grown <= bound
    D, I = index.search(P[:4] * F32(0.1), 10)
    assert I[:, 0].tolist() == [0, 1, 2, 3]


# ---- 6. the proof ------------------------------------------------------------------------------------------------------------------------
def test_proof_on_near_ties_and_adversarial_queries():
    """CLS-like rows with 600 near-ties around the k-th score (k = 100 cuts through them), plus the queries built to spend the bound: the measured
    |s^ - a_r <q, R8[r]>| stays inside eps for every candidate the scan emits, every query ends proven or served by the exact fallback and equals
    the oracle, and last_stats says which."""
    n, d, k = 30000, 256, 100
    P, u = cls_like_rows(61, n, d)
    g = np.random.default_rng(62)
    base = P[7].copy()
    P[100:150] = base * F32(1.05) + (1e-3 * g.standard_normal((50, d))).astype(F32)
    P[1000:1600] = base + (2e-5 * g.standard_normal((600, d))).astype(F32)
    index = attach8(P)
    mu = check_mu(index, P)
    r8, a = quantize_ref(P, mu)
    q_adv, _ = adversarial_queries(r8, a, 8, 63)
    q = np.concatenate([(base - mu)[None, :] * F32(3.0), (4.0 * u[None, :] + 0.1 * g.standard_normal((7, d))).astype(F32), q_adv]).astype(F32)
    # the scan as the search runs it: thresholds from the index, candidates checked against eps
    res = index._res
    h, l, sq = digits_ref(q)
    eps = eps_ref(sq, qnorm_ref(q), res.b1, res.max_norm, d)
    qb, qn, sqd = torch.empty(len(q), d, dtype=torch.bfloat16, device=DEV), torch.empty(len(q), device=DEV), torch.empty(len(q), device=DEV)
    qd = torch.empty(2, len(q), d, dtype=torch.int8, device=DEV)
    ops.topk_prep_queries_i8(dev(q), qd, qb, sqd, qn, torch.zeros(1, dtype=torch.int32, device=DEV))
    thr_d, eps_d = index._estimate_thresholds(qb, qn, k, False, sq=sqd)
    eps_got = eps_d.cpu().numpy()
    assert np.all(np.abs(eps_got.astype(np.float64) - eps) <= 2 * np.spacing(eps)), (eps_got, eps)
    counts, dropped, rows, scores = run_scan(h, l, sq, thr_d.cpu().numpy(), r8, a, RU.CAND_CAP)
    exact = centred_exact(q, r8, a)
    worst = 0.0
    for qi in range(len(q)):
        c = min(int(counts[qi]), RU.CAND_CAP)
        err = np.abs(scores[qi, :c].astype(np.float64) - exact[qi, rows[qi, :c]])
        assert np.all(err <= eps_got[qi]), (qi, err.max(), eps_got[qi])
        worst = max(worst, float(err.max(initial=0.0)) / float(eps_got[qi]))
    print(f"int8 proof: {int(counts.sum())} candidates, max |s^ - exact| / eps = {worst:.3f}")
    D, I = index.search(q, k)
    st = index.last_stats
    print(f"int8 proof: unproven after the first pass {st['unproven_first_pass']}, rescans {st['rescans']}, exact fallback {st['fallback_queries']}, "
          f"status bits {st['status_bits_first_pass']}")
    same_ranking(D, I, *oracle8(mu, r8, a, q, k))
    assert set(I[0, 50:].tolist()) <= set(range(1000, 1600)) | {7}    # the cut runs through the block of near-ties (row 7 is their base)
    assert st["fallback_queries"] <= len(q) and st["unproven_first_pass"] <= len(q)


# ---- 7. files -----------------------------------------------------------------------------------------------------------------------------
def test_int8_file_attach_equals_the_attached_index(tmp_path):
    n, d, nq, k = 70001, 256, 40, 100
    emb = syn.corpus_embeddings(78, n, d) + F32(0.25)
    q = syn.corpus_embeddings(79, nq, d)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    a = attach8(emb, ids)
    D, I = a.search(q, k)
    path = str(tmp_path / "dev.index")
    RU.write_index(a, path, int8=True)                                 # the attached index's own mu, rows and scales
    f = RU.read_index(path)
    assert f.row_dtype == "int8" and f.embeddings is None and np.array_equal(f.mu, a.mu)
    with pytest.raises(RuntimeError):
        f.search(q, k)
    RU.convert_index_to_gpu(f, 0, True)                                # an int8-row file is searched in int8-row mode whatever the flag
    assert f.row_dtype == "int8" and f._p32 is None and f._p16 is None
    assert torch.equal(f._res.r8, a._res.r8) and torch.equal(f._res.scale, a._res.scale) and torch.equal(f._sample, a._sample)
    assert f._res.b1 == a._res.b1 and f._max_norm == a._max_norm
    Df, If = f.search(q, k)
    assert np.array_equal(D, Df) and np.array_equal(I, If)
    with pytest.raises(ValueError):
        RU.write_index(f, str(tmp_path / "no"), fp16=True)
    # a file written on the host from the same rows: its own mu (may differ in the last bit), held to the oracle of ITS rows
    hpath = str(tmp_path / "host.index")
    RU.write_index(RU.construct_flatindex_from_embeddings(emb, ids), hpath, int8=True)
    hidx = RU.read_index(hpath).to_gpu(0)
    r8h, ah = np.load(hpath + ".emb8.npy"), np.load(hpath + ".scale.npy")
    r8_ref, a_ref = quantize_ref(emb, hidx.mu)
    assert np.array_equal(r8h, r8_ref) and np.array_equal(ah.view(np.uint32), a_ref.view(np.uint32))
    Dh, Ih = hidx.search(q, k)
    same_ranking(Dh, Ih, *oracle8(hidx.mu, r8h, ah, q, k, ids=ids))
    assert os.path.getsize(hpath + ".emb8.npy") + os.path.getsize(hpath + ".scale.npy") < 0.26 * n * d * 4


# ---- 8. command lines -----------------------------------------------------------------------------------------------------------------
def test_clis_index_int8_and_use_int8(tmp_path):
    """index_text --index_int8 -> retrieve_top_passages writes the run file the Python API writes from the same index file; --use_int8 on an
    fp32-format file writes what to_gpu(int8_rows=True) gives; a refused flag pair exits before anything is loaded."""
    from cldrd_amd.dataset import SyntheticSequenceDataset
    from cldrd_amd.models.nway_dual_encoder import NwayDualEncoder
    from cldrd_amd.retriever.index_text import load_checkpoint_into
    from cldrd_amd.retriever.retrieve_top_passages import write_run_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = selftest.tiny_config()
    model = selftest.build_tiny_model(cfg).cuda().eval()
    mdir = tmp_path / "model"
    model.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp_path / "checkpoint_10.pth.tar"
    torch.save({"state_dict": {"module." + k_: v.cpu() for k_, v in model.state_dict().items()}, "scheduler": {"last_epoch": 3}}, ckpt)
    rows, nq, k = 1301, 45, 20
    common = ["--resume", str(ckpt), "--model_name_or_path", str(mdir)]

    def run(mod, argv, code=0):
        p = _run_cli(mod, common + argv, {}, root)
        out, _ = p.communicate(timeout=600)
        assert p.returncode == code, out[-2000:]
        return out

    out = run("cldrd_amd.retriever.retrieve_top_passages", ["--index_path", str(tmp_path / "missing.index"), "--use_int8", "--use_float16"], code=2)
    assert "exclude one another" in out
    for name, extra in (("f32", []), ("i8", ["--index_int8"])):
        run("cldrd_amd.retriever.index_text", ["--index_dir", str(tmp_path / name), "--max_length", "32", "--synthetic_rows", str(rows)] + extra)
    f32_index, i8_index = str(tmp_path / "f32" / "checkpoint_10.index"), str(tmp_path / "i8" / "checkpoint_10.index")
    assert os.path.exists(i8_index + ".emb8.npy") and os.path.exists(i8_index + ".scale.npy") and not os.path.exists(i8_index + ".emb.npy")
    runs = {}
    for name, index_path, extra in (("use_int8", f32_index, ["--use_int8"]), ("file8", i8_index, [])):
        runs[name] = str(tmp_path / (name + ".dev.run"))
        run("cldrd_amd.retriever.retrieve_top_passages", ["--index_path", index_path, "--max_length", "16", "--top_k", str(k), "--synthetic_queries", str(nq),
                                                          "--output_path", runs[name]] + extra)
    m2 = NwayDualEncoder(str(mdir), share_weights=False)
    load_checkpoint_into(m2, str(ckpt), True)
    m2.cuda()
    q, qids = RU.get_embeddings_from_scratch(m2, SyntheticSequenceDataset(nq, 16, seed=4242).loader(), use_fp16=True, is_query=True)
    for name, index in (("use_int8", RU.read_index(f32_index).to_gpu(0, int8_rows=True)), ("file8", RU.convert_index_to_gpu(RU.read_index(i8_index), 0, False))):
        assert index.row_dtype == "int8"
        s_, i_ = RU.index_retrieve(index, q, k, batch=128, as_arrays=True)
        mine = str(tmp_path / (name + ".inproc.run"))
        write_run_file(mine, qids, i_, s_)
        assert open(runs[name], "rb").read() == open(mine, "rb").read()
    # and the file's rows are the definition's
    f32 = RU.read_index(f32_index)
    f8 = RU.read_index(i8_index)
    r8, a = quantize_ref(np.asarray(f32.embeddings), f8.mu)
    assert np.array_equal(np.load(i8_index + ".emb8.npy"), r8) and np.array_equal(np.load(i8_index + ".scale.npy"), a)
