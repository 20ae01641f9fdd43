"""fp16-row index mode on the MI355X (``to_gpu(dev, fp16_rows=True)`` / ``convert_index_to_gpu(..., useFloat16=True)`` / fp16-row files).

The oracle is the mode's definition restated with numpy in fp64 from the INDEX'S OWN ``mu``: ``R16 = fp16(P - mu)`` (fp32 subtraction, round to
nearest even), ``s(q, r) = fp32(<q, mu> + <q, R16[r]>)`` with both sums in fp64 and one rounding, top-k by (s desc, row position asc).  ``mu``
itself is held to the fp64 column mean of P within 1e-6 of max|mu| (fp32 rounding of a mean).  Bars of the search checks: those of
tests/test_gpu_retrieval.py (``same_ranking``: identical ids and ranks wherever adjacent oracle scores differ by more than 1e-5 |score|,
scores to 1e-5 relative)."""
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

DEV = "cuda"


def centred16(P, mu):
    return (np.asarray(P, dtype=np.float32) - np.asarray(mu, dtype=np.float32)).astype(np.float16)


def oracle16(mu, r16, q, k, ids=None, id_offset=0, chunk=32768):
    """The definition: (D fp32 [nq, k], I int64 [nq, k]) over the stored rows mu + r16; missing -> (-inf, -1)."""
    n, nq = r16.shape[0], q.shape[0]
    q64 = q.astype(np.float64)
    qmu = q64 @ np.asarray(mu, dtype=np.float64)
    s = np.empty((nq, n), dtype=np.float32)
    for lo in range(0, n, chunk):
        s[:, lo:lo + chunk] = (qmu[:, None] + q64 @ r16[lo:lo + chunk].astype(np.float64).T).astype(np.float32)
    kk = min(k, n)
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]            # stable: equal scores keep row position ascending
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    D[:, :kk] = np.take_along_axis(s, order, 1)
    I[:, :kk] = order + id_offset if ids is None else np.asarray(ids, dtype=np.int64)[order]
    return D, I


def check_mu(index, P):
    mu64 = np.asarray(P, dtype=np.float64).mean(axis=0)
    mu = np.asarray(index.mu)
    assert mu.dtype == np.float32 and not index.mu.flags.writeable
    assert np.max(np.abs(mu.astype(np.float64) - mu64)) <= 1e-6 * np.max(np.abs(mu64))
    return mu


def attach16(P, ids=None, id_offset=0, **hooks):
    index = RU.FlatIPIndex(P.shape[1])
    index.add_with_ids(P, ids)
    index.id_offset = id_offset
    for k_, v_ in hooks.items():
        setattr(index, k_, v_)
    out = RU.convert_index_to_gpu(index, 0, True)
    assert out is index and index.row_dtype == "float16" and index._p32 is None
    return index


# ---- 1. the re-score kernel alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 768, 1024, 132])
def test_rescore16_is_the_rounded_fp64_sum(d):
    """cldrd_topk_rescore on fp16 rows + cldrd_query_dot64 against fp32(q.mu + q.R16[row]) in numpy fp64 on ragged candidate lists (counts 0 and cap among
    them), heavy-tailed row norms.  Equal BIT FOR BIT, except where the fp64 sum lies within 1e-9 relative of an fp32 rounding boundary (the
    device's summation order differs from numpy's): at most 1 in 10 000 such entries, each one ulp off.  d = 132 takes the 8-byte-load form."""
    rows, nq, cap = 6000, 9, 1500
    g = torch.Generator(device=DEV).manual_seed(100 + d)
    P = torch.randn(rows, d, device=DEV, generator=g) * torch.exp(1.5 * torch.randn(rows, 1, device=DEV, generator=g))
    R16 = P.half().contiguous()
    assert torch.isfinite(R16).all()
    mu = torch.randn(d, device=DEV, generator=g)
    Q = torch.randn(nq, d, device=DEV, generator=g)
    counts = torch.randint(1, cap, (nq,), device=DEV, generator=g, dtype=torch.int32)
    counts[0], counts[1], counts[2] = 0, cap, 1
    cand = torch.randint(0, rows, (nq, cap), device=DEV, generator=g, dtype=torch.int32)
    cand[1, 0], cand[1, 1] = rows - 1, 0
    scores = torch.full((nq, cap), 12345.0, device=DEV)
    qmu = ops.query_dot64(Q, mu)
    ops.topk_rescore(Q, R16, counts, cand, scores, qmu=qmu)
    torch.cuda.synchronize()
    q64, mu64, r64 = Q.cpu().numpy().astype(np.float64), mu.cpu().numpy().astype(np.float64), R16.cpu().numpy().astype(np.float64)
    qmu_ref = (q64 * mu64).sum(axis=1)
    assert np.allclose(qmu.cpu().numpy(), qmu_ref, rtol=1e-13, atol=1e-13)
    got, cnt, cr = scores.cpu().numpy(), counts.cpu().numpy(), cand.cpu().numpy()
    total = exceptions = 0
    for qi in range(nq):
        c = int(cnt[qi])
        assert np.all(got[qi, c:] == 12345.0)                      # nothing written past the list
        ref64 = qmu_ref[qi] + (r64[cr[qi, :c]] * q64[qi]).sum(axis=1)
        ref32 = ref64.astype(np.float32)
        bad = np.nonzero(got[qi, :c] != ref32)[0]
        total += c
        for j in bad:
            g32, r32 = got[qi, j], ref32[j]
            assert g32 in (np.nextafter(r32, np.float32(np.inf)), np.nextafter(r32, np.float32(-np.inf))), (qi, j, g32, r32)
            boundary = 0.5 * (float(g32) + float(r32))
            assert abs(ref64[j] - boundary) <= 1e-9 * abs(ref64[j]), (qi, j, ref64[j], boundary)
            exceptions += 1
    print(f"rescore16 d={d}: {exceptions} of {total} entries one ulp off at a rounding boundary")
    assert exceptions * 10000 <= total


# ---- 2. search parity ---------------------------------------------------------------------------------------------------------
def _iso_with_ties(n, d, nq):
    emb = syn.corpus_embeddings(71, n, d)
    emb[n // 2] = emb[n // 3]                                         # exact ties, broken by row position
    emb[n - 1] = emb[5]
    emb[101] = emb[100] * np.float32(1.0 + 2e-7)                      # near-ties (may or may not survive the fp16 rounding)
    emb[203] = emb[200] + np.float32(1e-6)
    q = syn.corpus_embeddings(72, nq, d)
    q[0] = emb[n // 3]
    q[1] = emb[100] * np.float32(0.5)
    return emb, q


def test_search_parity_isotropic_with_ties():
    n, d, nq = 20000, 768, 24
    emb, q = _iso_with_ties(n, d, nq)
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    index = attach16(emb, ids)
    mu = check_mu(index, emb)
    r16 = centred16(emb, mu)
    assert np.array_equal(index._p16.cpu().numpy().view(np.uint16), r16.view(np.uint16))          # R16 = fp16(P - mu), round to nearest even
    for k in (1, 10, 1000):
        D, I = index.search(q, k)
        st = index.last_stats
        Dr, Ir = oracle16(mu, r16, q, k, ids=ids)
        same_ranking(D, I, Dr, Ir)
        assert np.all(np.diff(D, axis=1) <= 0)
        assert not st["exhaustive"] and st["fallback_queries"] == 0, st
    D, I = index.search(q, 10)
    assert I[0, 0] == ids[n // 3] and I[0, 1] == ids[n // 2] and D[0, 0] == D[0, 1]             # exact tie: lower row first


def test_search_parity_query_tile_128_multi_pass():
    n, d, nq, k = 20000, 768, 300, 10
    emb, q = _iso_with_ties(n, d, nq)
    index = attach16(emb, None, id_offset=1000, query_tile_request=128)
    assert index.query_tile == 128
    mu = check_mu(index, emb)
    D, I = index.search(q, k)
    assert index.last_stats["scans"] >= 3 and index.last_stats["fallback_queries"] == 0
    sel = np.arange(0, nq, 7)
    Dr, Ir = oracle16(mu, centred16(emb, mu), q[sel], k, id_offset=1000)
    same_ranking(D[sel], I[sel], Dr, Ir)
    index2 = attach16(emb, None, id_offset=1000)                      # 256-query tiles: same answer
    D2, I2 = index2.search(q, k)
    assert index2.query_tile == 256 and np.array_equal(D, D2) and np.array_equal(I, I2)


@pytest.fixture(scope="module")
def cls200k():
    P, u = syn.cls_like_corpus(200000, 768, 777, DEV)
    Q = syn.cls_like_queries(128, u, 778)
    return P.cpu().numpy(), Q.cpu().numpy()


@pytest.fixture(scope="module")
def iso200k():
    return syn.corpus_embeddings(81, 200000, 768), syn.corpus_embeddings(82, 128, 768)


def test_search_parity_cls_like_200k(cls200k):
    P, Q = cls200k
    q = Q[:16]
    index = attach16(P, None, id_offset=17)
    mu = check_mu(index, P)
    r16 = centred16(P, mu)
    for k in (1000, 10, 1):
        D, I = index.search(q, k)
        st = index.last_stats
        Dr, Ir = oracle16(mu, r16, q, k, id_offset=17)
        same_ranking(D, I, Dr, Ir)
        assert st["fallback_queries"] == 0, st


@pytest.mark.parametrize("n,d,nq", [(3000, 128, 6), (500, 64, 6), (RU.CAND_CAP, 768, 6), (3000, 128, 130)],
                         ids=["3000-128", "500-64", f"{RU.CAND_CAP}-768", "3000-128-nq130"])          # 130 queries: two query tiles through the chain
def test_search_parity_exhaustive_form(n, d, nq):
    emb = syn.corpus_embeddings(73, n, d)
    emb[n // 2] = emb[n // 3]
    q = syn.corpus_embeddings(74, nq, d)
    ids = np.arange(n, dtype=np.int64) + 9
    index = attach16(emb, ids)
    mu = check_mu(index, emb)
    r16 = centred16(emb, mu)
    for k in (1, 10, 1000):
        D, I = index.search(q, k)
        assert index.last_stats["exhaustive"]
        Dr, Ir = oracle16(mu, r16, q, k, ids=ids)
        same_ranking(D, I, Dr, Ir)
        if k > n:
            assert np.all(I[:, n:] == -1) and np.all(np.isneginf(D[:, n:]))


# ---- 3. the last-resort path, the width limit -----------------------------------------------------------------------------------
def test_exhaustive_chunks_on_fp16_rows():
    n, d, nq, k = 30000, 128, 5, 1000
    emb = syn.corpus_embeddings(75, n, d)
    emb[n - 5] = emb[11]                              # a tie across chunks: lower row first
    q = syn.corpus_embeddings(76, nq, d)
    index = attach16(emb)
    mu = check_mu(index, emb)
    Dd, Id = index._search_exhaustive_chunks(torch.from_numpy(q).to(DEV), k)
    Dr, Ir = oracle16(mu, centred16(emb, mu), q, k)
    same_ranking(Dd.cpu().numpy(), Id.cpu().numpy().astype(np.int64), Dr, Ir)


def test_width_above_2048_is_refused_in_fp16_row_mode():
    emb = syn.corpus_embeddings(77, 64, 2052)
    index = RU.FlatIPIndex(2052)
    index.add(emb)
    with pytest.raises(ValueError, match="2048"):
        index.to_gpu(0, fp16_rows=True)
    with pytest.raises(ValueError, match="2048"):
        RU.FlatIPIndex.from_device_rows(torch.from_numpy(emb).to(DEV), fp16_rows=True)


# ---- 4. memory: the point of the mode ---------------------------------------------------------------------------------------------
def test_resident_bytes_and_attach_peak():
    """400 k x 768 rows.  fp16-row mode: resident growth <= 2 n d (the fp16 rows) + the bf16 threshold sample + 8 MB (mu, flags, allocator
    rounding); the peak during attach exceeds that by at most the two fp32 staging chunks; no fp32 rows.  fp32 mode: >= 6 n d."""
    n, d = 400000, 768
    P = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32)
    P += np.float32(0.5)
    MB = 1 << 20

    def measure(fp16_rows):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        index = RU.FlatIPIndex(d)
        index.add(P)
        index.to_gpu(0, fp16_rows=fp16_rows)
        torch.cuda.synchronize()
        return index, torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before

    index, grown, peak = measure(True)
    assert index._p32 is None and index.row_dtype == "float16"
    assert n > 2 * RU.ATTACH_CHUNK_ROWS                   # several chunks, both staging buffers in use
    bound = 2 * n * d + index._sample.numel() * 2 + 8 * MB
    print(f"fp16-row mode: resident {grown / MB:.1f} MB (bound {bound / MB:.1f}), attach peak {peak / MB:.1f} MB "
          f"(bound {(bound + 2 * RU.ATTACH_CHUNK_ROWS * d * 4) / MB:.1f})")
    assert grown <= bound
    assert peak <= bound + 2 * RU.ATTACH_CHUNK_ROWS * d * 4
    D, I = index.search(P[:4] * np.float32(0.1), 10)
    assert I[:, 0].tolist() == [0, 1, 2, 3]
    del index
    index32, grown32, _ = measure(False)
    print(f"fp32 mode: resident {grown32 / MB:.1f} MB")
    assert index32._p32 is not None and index32.row_dtype == "float32"
    assert grown32 >= 6 * n * d


# ---- 5. equivalences --------------------------------------------------------------------------------------------------------------
def test_fp16_file_attach_equals_attach_of_the_fp32_rows(tmp_path):
    n, d, nq, k = 70001, 256, 40, 100
    emb = syn.corpus_embeddings(78, n, d) + np.float32(0.25)
    q = syn.corpus_embeddings(79, nq, d)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    a = attach16(emb, ids)
    D, I = a.search(q, k)
    path = str(tmp_path / "dev.index")
    RU.write_index(a, path, fp16=True)                    # the attached index's own mu and rows
    f = RU.read_index(path)
    assert f.row_dtype == "float16" and f.embeddings is None and np.array_equal(f.mu, a.mu)
    RU.convert_index_to_gpu(f, 0, False)                  # an fp16-row file is searched in fp16-row mode whatever the flag
    assert f.row_dtype == "float16" and f._p32 is None
    assert torch.equal(f._p16, a._p16)
    assert f._max_norm == a._max_norm
    Df, If = f.search(q, k)
    assert np.array_equal(D, Df) and np.array_equal(I, If)
    assert f.last_stats["fallback_queries"] == 0
    mu = check_mu(a, emb)
    Dr, Ir = oracle16(mu, centred16(emb, mu), q, k, ids=ids)
    same_ranking(Df, If, Dr, Ir)
    # a file written on the host from the same rows: its own mu (may differ in the last bit), held to the oracle of ITS rows
    hpath = str(tmp_path / "host.index")
    RU.write_index(RU.construct_flatindex_from_embeddings(emb, ids), hpath, fp16=True)
    h = RU.read_index(hpath).to_gpu(0)
    Dh, Ih = h.search(q, k)
    r16h = np.load(hpath + ".emb16.npy")
    assert np.array_equal(r16h.view(np.uint16), centred16(emb, h.mu).view(np.uint16))
    same_ranking(Dh, Ih, *oracle16(h.mu, r16h, q, k, ids=ids))


@pytest.mark.parametrize("with_ids", [True, False])
def test_device_list_shards_in_fp16_row_mode(with_ids):
    n, d, nq, k = 30001, 128, 12, 50
    emb = syn.corpus_embeddings(83, n, d) + np.float32(0.3) * (np.arange(n, dtype=np.float32)[:, None] / n)      # shard means differ
    q = syn.corpus_embeddings(84, nq, d)
    ids = np.arange(n, dtype=np.int64) * 7 + 2 if with_ids else None
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    index.id_offset = 0 if with_ids else 500
    multi = RU.convert_index_to_gpu(index, [0, 0], True)
    assert isinstance(multi, RU.MultiDeviceFlatIPIndex) and multi.row_dtype == "float16"
    D, I = multi.search(q, k)
    s_all = []
    for s_, sh in enumerate(multi.shards):
        lo, hi = RU.ShardedFlatIPIndex.shard_bounds(n, 2, s_)
        assert sh.row_dtype == "float16" and sh._p32 is None
        mu = check_mu(sh, emb[lo:hi])
        Ds, Is = oracle16(mu, centred16(emb[lo:hi], mu), q, hi - lo)           # every row of the shard, scored by the shard's own mu
        back = np.empty_like(Ds)
        np.put_along_axis(back, Is, Ds, axis=1)
        s_all.append(back)
    s_all = np.concatenate(s_all, axis=1)
    order = np.argsort(-s_all, axis=1, kind="stable")[:, :k]
    Dr = np.take_along_axis(s_all, order, 1)
    Ir = ids[order] if with_ids else order + 500
    same_ranking(D, I, Dr, Ir)
    assert not np.array_equal(multi.shards[0].mu, multi.shards[1].mu)


def test_from_device_rows_in_fp16_row_mode():
    n, d, nq, k = 150000, 768, 10, 100                    # three chunks of device rows, the last one ragged
    P, u = syn.cls_like_corpus(n, d, 91, DEV)
    Q = syn.cls_like_queries(nq, u, 92)
    index = RU.FlatIPIndex.from_device_rows(P, id_offset=11, fp16_rows=True)
    assert index.row_dtype == "float16" and index._p32 is None
    Ph, q = P.cpu().numpy(), Q.cpu().numpy()
    mu = check_mu(index, Ph)
    D, I = index.search(q, k)
    same_ranking(D, I, *oracle16(mu, centred16(Ph, mu), q, k, id_offset=11))
    assert index.last_stats["fallback_queries"] == 0
    host = attach16(Ph, None, id_offset=11)               # the same rows through the host staging buffers: same mu, same rows, same answer
    assert np.array_equal(host.mu, index.mu) and torch.equal(host._p16, index._p16) and torch.equal(host._sample, index._sample)
    Dh, Ih = host.search(q, k)
    assert np.array_equal(D, Dh) and np.array_equal(I, Ih)


def test_default_mode_is_untouched():
    """fp32 rows: the argument omitted, passed as False, and both forms of convert_index_to_gpu give bit-identical results, and those are
    what the mode has always returned - the fp64 inner products rounded once, (score desc, row asc) - on a heavy-tailed corpus."""
    rows, d, nq, k = 20000, 128, 32, 100
    g = torch.Generator(device=DEV).manual_seed(3)
    P = (torch.randn(rows, d, device=DEV, generator=g) * torch.exp(1.5 * torch.randn(rows, 1, device=DEV, generator=g))).cpu().numpy()
    q = torch.randn(nq, d, device=DEV, generator=g).cpu().numpy()
    outs = []
    for how in ("omitted", "false", "convert", "convert_false"):
        index = RU.FlatIPIndex(d)
        index.add(P)
        if how == "omitted":
            index.to_gpu(0)
        elif how == "false":
            index.to_gpu(0, fp16_rows=False)
        elif how == "convert":
            RU.convert_index_to_gpu(index, 0)
        else:
            RU.convert_index_to_gpu(index, [0], False)
        assert index.row_dtype == "float32" and index._p32 is not None
        outs.append(index.search(q, k))
    for D, I in outs[1:]:
        assert np.array_equal(D, outs[0][0]) and np.array_equal(I, outs[0][1])
    s = (q.astype(np.float64) @ P.astype(np.float64).T).astype(np.float32)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    assert np.array_equal(outs[0][1], order)
    assert np.array_equal(outs[0][0], np.take_along_axis(s, order, 1))


# ---- 6. quality sanity ------------------------------------------------------------------------------------------------------------
def _overlap(Ia, Ib):
    return float(np.mean([len(np.intersect1d(Ia[j], Ib[j])) / Ia.shape[1] for j in range(Ia.shape[0])]))


@pytest.mark.parametrize("corpus", ["cls_like", "isotropic"])
def test_top100_overlap_with_the_fp32_mode(corpus, request):
    """A condition, not a tolerance: the top-100 of the fp16-row mode and of the fp32 mode share >= 0.995 of their rows (the numpy restatement
    of the definition gives 0.9997 / 0.9993 on these two corpora)."""
    P, Q = request.getfixturevalue("cls200k" if corpus == "cls_like" else "iso200k")
    a = attach16(P)
    _, I16 = a.search(Q, 100)
    del a
    b = RU.FlatIPIndex(P.shape[1])
    b.add(P)
    b.to_gpu(0)
    _, I32 = b.search(Q, 100)
    ov = _overlap(I16, I32)
    print(f"top-100 overlap fp16-row vs fp32 mode, {corpus} 200 k x 768, {Q.shape[0]} queries: {ov:.4f}")
    assert ov >= 0.995


# ---- 7. command lines -------------------------------------------------------------------------------------------------------------
def _read_run(path, nq, k):
    D = np.empty((nq, k), dtype=np.float32)
    I = np.empty((nq, k), dtype=np.int64)
    qids = []
    with open(path) as fh:
        for line in fh:
            qid, docid, rank, score = line.rstrip("\n").split("\t")
            if not qids or qids[-1] != int(qid):
                qids.append(int(qid))
            D[len(qids) - 1, int(rank) - 1] = np.float32(float(score))
            I[len(qids) - 1, int(rank) - 1] = int(docid)
    assert len(qids) == nq
    return qids, D, I


def test_clis_index_fp16_and_use_float16(tmp_path):
    """index_text --index_fp16 -> retrieve_top_passages, and index_text -> retrieve_top_passages --use_float16: each run file against the oracle
    of the rows THAT index stores (its own mu); without either flag the run file is the default path's, byte for byte."""
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

    def run(mod, argv):
        p = _run_cli(mod, common + argv, {}, root)
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out[-2000:]

    for name, extra in (("f32", []), ("f16", ["--index_fp16"])):
        run("cldrd_amd.retriever.index_text", ["--index_dir", str(tmp_path / name), "--max_length", "32", "--synthetic_rows", str(rows)] + extra)
    f32_index, f16_index = str(tmp_path / "f32" / "checkpoint_10.index"), str(tmp_path / "f16" / "checkpoint_10.index")
    assert os.path.exists(f16_index + ".emb16.npy") and not os.path.exists(f16_index + ".emb.npy")
    assert os.path.exists(f32_index + ".emb.npy") and not os.path.exists(f32_index + ".emb16.npy")
    assert os.path.getsize(f16_index + ".emb16.npy") < 0.51 * os.path.getsize(f32_index + ".emb.npy")
    runs = {}
    for name, index_path, extra in (("default", f32_index, []), ("use_float16", f32_index, ["--use_float16"]), ("file16", f16_index, [])):
        out_path = str(tmp_path / (name + ".dev.run"))
        run("cldrd_amd.retriever.retrieve_top_passages", ["--index_path", index_path, "--max_length", "16", "--top_k", str(k), "--synthetic_queries", str(nq),
                                                          "--output_path", out_path] + extra)
        runs[name] = out_path

    # the queries, encoded here as the command line encodes them
    m2 = NwayDualEncoder(str(mdir), share_weights=False)
    load_checkpoint_into(m2, str(ckpt), True)
    m2.cuda()
    q, qids = RU.get_embeddings_from_scratch(m2, SyntheticSequenceDataset(nq, 16, seed=4242).loader(), use_fp16=True, is_query=True)
    f32 = RU.read_index(f32_index)
    P, ids = np.asarray(f32.embeddings), np.asarray(f32.ids)

    # without the flags: the untouched default path
    dflt = RU.convert_index_to_gpu(RU.read_index(f32_index), 0, False)
    assert dflt.row_dtype == "float32"
    s_d, i_d = RU.index_retrieve(dflt, q, k, batch=128, as_arrays=True)
    write_run_file(str(tmp_path / "inproc.dev.run"), qids, i_d, s_d)
    assert open(runs["default"], "rb").read() == open(str(tmp_path / "inproc.dev.run"), "rb").read()

    # --use_float16: mu as the device computes it from the fp32 file (it depends neither on the device nor on timing)
    dev16 = RU.read_index(f32_index).to_gpu(0, fp16_rows=True)
    mu = check_mu(dev16, P)
    rq, D, I = _read_run(runs["use_float16"], nq, k)
    assert rq == list(qids)
    same_ranking(D, I, *oracle16(mu, centred16(P, mu), q, k, ids=ids))

    # --index_fp16: the file's own mu and rows
    f16 = RU.read_index(f16_index)
    assert f16.row_dtype == "float16" and np.array_equal(np.asarray(f16.ids), ids)
    mu_f = check_mu(f16, P)
    r16 = np.load(f16_index + ".emb16.npy")
    assert np.array_equal(r16.view(np.uint16), centred16(P, mu_f).view(np.uint16))
    rq, D, I = _read_run(runs["file16"], nq, k)
    assert rq == list(qids)
    same_ranking(D, I, *oracle16(mu_f, r16, q, k, ids=ids))
