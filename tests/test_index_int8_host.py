"""int8-row index mode, the parts that need no GPU: the mode's definition restated in numpy (the functions below are the oracle of
tests/test_gpu_index_int8.py too), the host writer against it bit for bit, the file format and its refusals, the command-line flags, the
query digits, and the scan bound - the pinned scan-score formula emulated in numpy against the exact centred score on four kinds of data.

The definition (include/cldrd_hip.h, csrc/topk_i8.hip):
    c = p - mu (fp32), a_r = max|c| / 127 (fp32), R8 = clamp(rint(c / a_r), -127, 127); stored row mu + a_r R8[r];
    s(q, r) = fp32(<q, mu> + a_r <q, R8[r]>) with the sums and the product in fp64;
    sq = max|q| / 16256, t = rint(q / sq), l = ((t + 64) mod 128) - 64, h = (t - l) / 128;
    s^ = fmaf(128.0f, (float)H, (float)L) * (sq * a_r),  H = <h, R8[r]>, L = <l, R8[r]> exact.
Integer products go through float64 matmul: exact for these magnitudes (|H| <= 127 127 2048 < 2^53) and fast."""
import inspect
import os
import pickle

import numpy as np
import pytest

from cldrd_amd.retriever import retrieval_utils as RU

F32 = np.float32


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def quantize_ref(P, mu):
    """-> (R8 int8 [n, d], a fp32 [n]) of fp32 rows P and the mean row mu"""
    c = np.asarray(P, dtype=F32) - np.asarray(mu, dtype=F32)
    a = np.abs(c).max(axis=1) / F32(127.0)
    assert a.dtype == F32
    r8 = np.zeros(c.shape, dtype=np.int8)
    live = a > 0
    r8[live] = np.clip(np.rint(c[live] / a[live, None]), -127, 127).astype(np.int8)
    return r8, a


def bound_norms_ref(r8, a):
    """-> (B1 = max a_r |R8[r]|_1, max a_r^2 |R8[r]|_2^2) as the fp32 values of the fp64 products with the exact integer sums"""
    r = r8.astype(np.int64)
    a64 = a.astype(np.float64)
    return (a64 * np.abs(r).sum(axis=1)).astype(F32).max(), ((a64 * a64) * (r * r).sum(axis=1)).astype(F32).max()


def digits_of_t(t):
    t = np.asarray(t, dtype=np.int64)
    l = ((t + 64) % 128) - 64
    h = (t - l) // 128
    return h, l


def digits_ref(q):
    """-> (h int8 [nq, d], l int8 [nq, d], sq fp32 [nq]); a query with max|q| < 2^-100 has zero digits and sq = 2 max|q|"""
    q = np.asarray(q, dtype=F32)
    amax = np.abs(q).max(axis=1)
    live = amax >= F32(2.0 ** -100)
    sq = np.where(live, amax / F32(16256.0), F32(2.0) * amax).astype(F32)
    t = np.zeros(q.shape, dtype=np.int64)
    t[live] = np.clip(np.rint(q[live] / sq[live, None]), -16256, 16256).astype(np.int64)
    h, l = digits_of_t(t)
    assert np.abs(h).max(initial=0) <= 127 and l.min(initial=0) >= -64 and l.max(initial=0) <= 63
    return h.astype(np.int8), l.astype(np.int8), sq


def scan_ref(h, l, sq, r8, a):
    """The pinned scan score, fp32 [nq, n]: every step rounds as the kernel's does."""
    r = r8.astype(np.float64).T
    H = h.astype(np.float64) @ r                                       # exact integers
    L = l.astype(np.float64) @ r
    Hf, Lf = H.astype(F32), L.astype(F32)                              # (float)int: round to nearest even
    F = (128.0 * Hf.astype(np.float64) + Lf.astype(np.float64)).astype(F32)      # the fp64 sum is exact: one rounding, as fmaf
    w = sq.astype(F32)[:, None] * a.astype(F32)[None, :]               # fp32 product
    return F * w


def qnorm_ref(q):
    return np.sqrt((np.asarray(q, dtype=np.float64) ** 2).sum(axis=1)).astype(F32)


def eps_ref(sq, qnorm, b1, cnorm, d):
    """thresholds_i8_kernel restated (csrc/topk_i8.hip derives it): query digits + the five fp32 roundings of s^"""
    s, qn = sq.astype(np.float64), qnorm.astype(np.float64)
    e = s * (0.5 + 2.0 ** -9) * float(b1) + 5.0 * 2.0 ** -24 * (qn + 65.0 * s * np.sqrt(float(d))) * float(cnorm) * (1.0 + 2.0 ** -22)
    return (e * (1.0 + 1e-6)).astype(F32) + F32(1e-30)


def centred_exact(q, r8, a):
    """a_r <q, R8[r]> in fp64 [nq, n]"""
    return (np.asarray(q, dtype=np.float64) @ r8.astype(np.float64).T) * a.astype(np.float64)[None, :]


def oracle8(mu, r8, a, q, k, ids=None, id_offset=0):
    """The definition's top-k: (D fp32 [nq, k], I int64 [nq, k]); missing -> (-inf, -1)."""
    n, nq = r8.shape[0], q.shape[0]
    q64 = np.asarray(q, dtype=np.float64)
    s = ((q64 @ np.asarray(mu, dtype=np.float64))[:, None] + centred_exact(q, r8, a)).astype(F32)
    kk = min(k, n)
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    D = np.full((nq, k), -np.inf, dtype=F32)
    I = np.full((nq, k), -1, dtype=np.int64)
    D[:, :kk] = np.take_along_axis(s, order, 1)
    I[:, :kk] = order + id_offset if ids is None else np.asarray(ids, dtype=np.int64)[order]
    return D, I


def special_rows(d, mu):
    """rows whose centred form is: all zero; one non-zero; exact half steps (round to even); the extremes +-127"""
    mu = np.asarray(mu, dtype=F32)
    c = np.zeros((4, d), dtype=F32)
    c[1, 5] = F32(-3.25)
    c[2, :8] = np.array([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5], dtype=F32)      # a = 1: quotients on the half steps
    c[3, 0], c[3, 1], c[3, 2:] = F32(2.0), F32(-2.0), F32(0.75)
    return c, c + mu


def heavy_rows(seed, n, d):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, d)) * np.exp(1.5 * g.standard_normal((n, 1)))).astype(F32)


def cls_like_rows(seed, n, d):
    g = np.random.default_rng(seed)
    u = g.standard_normal(d)
    u /= np.linalg.norm(u)
    return (4.0 * u[None, :] + 0.1 * g.standard_normal((n, d))).astype(F32), u      # one dominant common component


def adversarial_queries(r8, a, nq, seed):
    """Queries built to spend the digit term of the bound on the rows with the largest a_r |R8[r]|_1: q_j = sq (t_j + 0.499 sign(R8[r, j]))
    with sq = 2^-10 exactly (one coordinate sits at t = 16256 without an offset)."""
    g = np.random.default_rng(seed)
    d = r8.shape[1]
    l1 = a.astype(np.float64) * np.abs(r8.astype(np.int64)).sum(axis=1)
    rows = np.argsort(-l1)[:nq]
    t = g.integers(-8000, 8001, size=(nq, d)).astype(np.float64)
    off = 0.499 * np.sign(r8[rows].astype(np.float64))
    pin = np.argmin(np.abs(r8[rows].astype(np.int64)), axis=1)         # pinning a coordinate where R8 is smallest loses the least of the bound
    t[np.arange(nq), pin], off[np.arange(nq), pin] = 16256.0, 0.0
    return ((t + off) * 2.0 ** -10).astype(F32), rows


# ---- 1. the host writer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 768])
def test_host_writer_equals_the_definition(tmp_path, d):
    P = heavy_rows(11 + d, 3000, d) + F32(0.25)
    index = RU.construct_flatindex_from_embeddings(P, np.arange(P.shape[0]) * 2 + 1)
    path = str(tmp_path / "h.index")
    RU.write_index(index, path, int8=True)
    meta = pickle.load(open(path + ".meta.pkl", "rb"))
    assert meta["format"] == RU.FORMAT_I8 == "cldrd-flatip-i8-v1"
    mu = (P.astype(np.float64).sum(axis=0) / P.shape[0]).astype(F32)
    assert meta["mu"].dtype == F32 and np.array_equal(meta["mu"], mu)
    r8, a = quantize_ref(P, mu)
    r8_f, a_f = np.load(path + ".emb8.npy", mmap_mode="r"), np.load(path + ".scale.npy")
    assert r8_f.dtype == np.int8 and a_f.dtype == F32
    assert np.array_equal(r8_f, r8) and np.array_equal(a_f.view(np.uint32), a.view(np.uint32))
    b1, c2 = bound_norms_ref(r8, a)
    assert meta["bound_l1"] == float(b1) and meta["max_centred_norm"] == float(np.sqrt(np.float64(c2)))
    assert abs(meta["raw_max_norm"] - np.sqrt((P.astype(np.float64) ** 2).sum(axis=1).max())) <= 1e-6 * meta["raw_max_norm"]
    assert np.abs(r8).max() == 127 and not os.path.exists(path + ".emb.npy")


def test_quantiser_special_rows():
    d = 64
    mu = ((np.arange(d) % 8 - 4) * 0.25).astype(F32)                          # quarter steps: c + mu and back are exact
    c, P = special_rows(d, mu)
    assert np.array_equal(P - mu, c)                                                     # chosen so that the fp32 subtraction gives c back
    for r8, a in (quantize_ref(P, mu), RU.FlatIPIndex.quantize_rows_i8(P, mu)[:2]):
        assert a[0] == 0 and not r8[0].any()
        assert a[1] == F32(3.25) / F32(127) and r8[1, 5] == -127 and np.count_nonzero(r8[1]) == 1
        assert a[2] == 1 and r8[2, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]           # halves go to the even neighbour
        assert r8[3, 0] == 127 and r8[3, 1] == -127 and np.all(r8[3, 2:] == np.rint(F32(0.75) / a[3]))
    r8, a, l1, l2sq = RU.FlatIPIndex.quantize_rows_i8(P, mu)
    r8_ref, a_ref = quantize_ref(P, mu)
    assert np.array_equal(r8, r8_ref) and np.array_equal(a, a_ref)
    assert (l1.max(), l2sq.max()) == bound_norms_ref(r8_ref, a_ref)


# ---- 2. the file format and its refusals -----------------------------------------------------------------------------------------
def test_file_round_trip_and_refusals(tmp_path):
    P = heavy_rows(5, 500, 128)
    ids = np.arange(500, dtype=np.int64) * 3 + 7
    path = str(tmp_path / "a.index")
    RU.write_index(RU.construct_flatindex_from_embeddings(P, ids), path, int8=True)
    f = RU.read_index(path)
    assert f.row_dtype == "int8" and f.embeddings is None and f.ntotal == 500 and f.d == 128
    assert np.array_equal(np.asarray(f.ids), ids) and f.mu.dtype == F32 and not f.mu.flags.writeable
    with pytest.raises(ValueError, match="int8-row file"):
        f.add(P[:3])
    with pytest.raises(ValueError):
        RU.write_index(f, str(tmp_path / "b"))
    with pytest.raises(ValueError):
        RU.write_index(f, str(tmp_path / "b"), fp16=True)
    with pytest.raises(RuntimeError):
        f.search(P[:2], 3)
    assert not list(tmp_path.glob("b*"))
    # a file index writes itself back unchanged
    path2 = str(tmp_path / "c.index")
    RU.write_index(f, path2, int8=True)
    for ext in (".emb8.npy", ".scale.npy"):
        assert np.array_equal(np.load(path + ext), np.load(path2 + ext))
    m1, m2 = (pickle.load(open(p_ + ".meta.pkl", "rb")) for p_ in (path, path2))
    assert sorted(m1) == sorted(m2) == sorted(["d", "ids", "id_offset", "format", "mu", "bound_l1", "max_centred_norm", "raw_max_norm"])
    assert all(np.array_equal(m1[k_], m2[k_]) for k_ in m1)


def test_flags_exclude_one_another_and_write_nothing(tmp_path):
    index = RU.construct_flatindex_from_embeddings(heavy_rows(6, 50, 64), None)
    for kw in ({"int8": True, "fp16": True}, {"int8": True, "faiss_format": True}):
        with pytest.raises(ValueError):
            RU.write_index(index, str(tmp_path / "x"), **kw)
    with pytest.raises(ValueError):
        index.write(str(tmp_path / "x"), fp16=True, int8=True)
    with pytest.raises(ValueError):
        index.to_gpu(0, fp16_rows=True, int8_rows=True)
    assert not list(tmp_path.iterdir())
    sig = inspect.signature(RU.write_index)
    assert list(sig.parameters) == ["index", "path", "faiss_format", "fp16", "int8"] and sig.parameters["int8"].default is False
    assert inspect.signature(RU.FlatIPIndex.to_gpu).parameters["int8_rows"].default is False
    assert inspect.signature(RU.FlatIPIndex.from_device_rows).parameters["int8_rows"].default is False
    assert list(inspect.signature(RU.convert_index_to_gpu).parameters) == ["index", "faiss_gpu_index", "useFloat16"]


@pytest.mark.parametrize("d", [132, 96, 2112])
def test_unsupported_width_is_named(tmp_path, d):
    index = RU.construct_flatindex_from_embeddings(np.ones((4, d), dtype=F32), None)
    with pytest.raises(ValueError, match=str(d)):
        RU.write_index(index, str(tmp_path / "w"), int8=True)
    assert not list(tmp_path.glob("w*.npy"))


# ---- 3. command-line flags ----------------------------------------------------------------------------------------------------------
def test_command_line_flags_default_off_and_exclude(tmp_path, capsys):
    from cldrd_amd.retriever import build_stage_file, index_text, retrieve_top_passages
    a = index_text.get_args(["--index_dir", str(tmp_path / "i")])
    assert a.index_int8 is False and a.index_fp16 is False
    assert index_text.get_args(["--index_dir", str(tmp_path / "i"), "--index_int8"]).index_int8 is True
    r = retrieve_top_passages.get_args([])
    assert r.use_int8 is False and r.use_float16 is False
    assert retrieve_top_passages.get_args(["--use_int8"]).use_int8 is True
    need = ["--index_path", "x", "--queries_path", "q", "--collection_path", "c", "--teacher_name_or_path", "t", "--label_mode", "9", "--output_path", "o"]
    b = build_stage_file.get_args(need)
    assert b.use_int8 is False and b.use_float16 is False
    assert build_stage_file.get_args(need + ["--use_int8"]).use_int8 is True
    for fn, argv in ((index_text.get_args, ["--index_dir", str(tmp_path / "never"), "--index_int8", "--index_fp16"]),
                     (retrieve_top_passages.get_args, ["--use_int8", "--use_float16"]),
                     (build_stage_file.get_args, need + ["--use_int8", "--use_float16"])):
        with pytest.raises(SystemExit) as e:
            fn(argv)
        assert e.value.code == 2
    assert "exclude one another" in capsys.readouterr().err
    assert not (tmp_path / "never").exists()                           # refused before anything is created or loaded


# ---- 4. the query digits --------------------------------------------------------------------------------------------------------------
def test_digits_are_exact_and_in_range():
    t = np.array([16256, -16256, 16255, -16255, 64, -64, 63, -63, 0, 1, -1, 127, 128, -128, -129, 8191], dtype=np.int64)
    h, l = digits_of_t(t)
    assert np.array_equal(128 * h + l, t)
    assert np.abs(h).max() == 127 and l.min() >= -64 and l.max() <= 63
    assert dict(zip(t.tolist(), zip(h.tolist(), l.tolist())))[16256] == (127, 0)
    assert dict(zip(t.tolist(), zip(h.tolist(), l.tolist())))[16255] == (127, -1)
    assert dict(zip(t.tolist(), zip(h.tolist(), l.tolist())))[64] == (1, -64)
    assert dict(zip(t.tolist(), zip(h.tolist(), l.tolist())))[-64] == (0, -64)
    assert dict(zip(t.tolist(), zip(h.tolist(), l.tolist())))[63] == (0, 63)
    every = np.arange(-16256, 16257)
    h, l = digits_of_t(every)
    assert np.array_equal(128 * h + l, every) and np.abs(h).max() == 127 and l.min() == -64 and l.max() == 63
    # through the query: sq = 2^-10 makes t the stated integers
    q = (np.array([[16256, -16255, 64, -64, 63, -63, 0, 5]], dtype=np.float64) * 2.0 ** -10).astype(F32)
    hq, lq, sq = digits_ref(q)
    assert sq[0] == F32(2.0 ** -10)
    assert np.array_equal(128 * hq.astype(np.int64) + lq, np.array([[16256, -16255, 64, -64, 63, -63, 0, 5]]))
    hz, lz, sz = digits_ref(np.zeros((1, 8), dtype=F32))
    assert sz[0] == 0 and not hz.any() and not lz.any()
    ht, lt, st = digits_ref(np.full((1, 8), 1e-35, dtype=F32))
    assert st[0] == F32(2e-35) and not ht.any() and not lt.any()


# ---- 5. the bound -----------------------------------------------------------------------------------------------------------------------
def _bound_case(name):
    n, d, nq = 20000, 768, 16
    g = np.random.default_rng(17)
    if name == "isotropic":
        P = g.standard_normal((n, d)).astype(F32) / F32(np.sqrt(d))
        Q = g.standard_normal((nq, d)).astype(F32) / F32(np.sqrt(d))
    elif name == "cls_like":
        P, u = cls_like_rows(18, n, d)
        Q = (4.0 * u[None, :] + 0.1 * g.standard_normal((nq, d))).astype(F32)
    elif name == "heavy_tailed":
        P = heavy_rows(19, n, d)
        Q = heavy_rows(20, nq, d)
    else:
        P, _ = cls_like_rows(21, 5000, 256)
        Q = None
    mu = (P.astype(np.float64).sum(axis=0) / P.shape[0]).astype(F32)
    r8, a = quantize_ref(P, mu)
    rows = None
    if Q is None:
        Q, rows = adversarial_queries(r8, a, nq, 22)
    return r8, a, Q, rows


@pytest.mark.parametrize("name", ["isotropic", "cls_like", "heavy_tailed", "adversarial"])
def test_scan_error_is_inside_eps(name):
    """|s^ - a_r <q, R8[r]>| <= eps for every (query, row); the adversarial queries must actually spend the bound (ratio >= 0.9)."""
    r8, a, Q, rows = _bound_case(name)
    d = r8.shape[1]
    h, l, sq = digits_ref(Q)
    b1, c2 = bound_norms_ref(r8, a)
    eps = eps_ref(sq, qnorm_ref(Q), b1, np.sqrt(np.float64(c2)), d)
    err = np.abs(scan_ref(h, l, sq, r8, a).astype(np.float64) - centred_exact(Q, r8, a))
    ratio = err / eps.astype(np.float64)[:, None]
    spread = centred_exact(Q, r8, a).std(axis=1)
    print(f"int8 scan bound, {name} {r8.shape[0]} x {d}: max |s^ - exact| / eps = {ratio.max():.3f}; eps / score spread = "
          f"{float((eps / spread).min()):.2e} .. {float((eps / spread).max()):.2e}")
    assert np.all(err <= eps.astype(np.float64)[:, None])
    if rows is not None:
        assert ratio[np.arange(len(rows)), rows].max() >= 0.9
