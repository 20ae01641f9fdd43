"""fp16-row index mode, the parts that need no GPU: the fp16-row file format (``write_index(..., fp16=True)`` / ``read_index``), the two
command-line flags, and the unchanged call surface.

Definition the checks restate with numpy: ``mu`` = fp32 of the fp64 column mean, ``R16 = fp16(P - mu)`` (fp32 subtraction, round to nearest
even), ``max_centred_norm`` = sqrt of the fp32 value of max_r |P[r] - mu|^2 (fp64 row sums), ``raw_max_norm`` likewise for P."""
import inspect
import math
import os
import pickle

import numpy as np
import pytest

import cldrd_amd.synthetic as syn
from cldrd_amd.retriever import retrieval_utils as RU


def _restate(P):
    mu = P.astype(np.float64).mean(axis=0).astype(np.float32)
    c = P - mu
    r16 = c.astype(np.float16)
    cn = math.sqrt(float(np.float32((c.astype(np.float64) ** 2).sum(axis=1).max())))
    rn = math.sqrt(float(np.float32((P.astype(np.float64) ** 2).sum(axis=1).max())))
    return mu, r16, cn, rn


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("with_ids,id_offset", [(True, 0), (False, 0), (False, 4321)])
def test_fp16_file_round_trip(tmp_path, monkeypatch, d, with_ids, id_offset):
    n = 3001
    monkeypatch.setattr(RU, "HOST_CHUNK_ROWS", 1000)          # several chunks and a ragged last one
    P = syn.corpus_embeddings(61, n, d) + (np.arange(d, dtype=np.float32) % 7 - 2.0) * 0.5      # a common component: mu is not ~0
    ids = np.arange(n, dtype=np.int64) * 5 + 3 if with_ids else None
    index = RU.construct_flatindex_from_embeddings(P, ids)
    index.id_offset = id_offset
    path = str(tmp_path / "h.index")
    RU.write_index(index, path, fp16=True)
    assert os.path.exists(path + ".emb16.npy") and not os.path.exists(path + ".emb.npy")
    with open(path + ".meta.pkl", "rb") as fh:
        meta = pickle.load(fh)
    assert meta["format"] == "cldrd-flatip-f16-v1" and meta["d"] == d and meta["id_offset"] == id_offset
    back = RU.read_index(path)
    assert back.row_dtype == "float16" and back.embeddings is None and back.ntotal == n and back.d == d
    assert back.id_offset == id_offset
    assert (back.ids is None) if ids is None else np.array_equal(back.ids, ids)
    # mu: fp32 rounding of a mean (relative 2^-24 of the mean's own size, far inside 1e-6 of max|mu|); the chunked fp64 sum may differ from
    # numpy's pairwise one in the last bits of the fp64 value
    mu64 = P.astype(np.float64).mean(axis=0)
    mu = np.asarray(back.mu)
    assert mu.dtype == np.float32 and mu.shape == (d,)
    assert np.max(np.abs(mu.astype(np.float64) - mu64)) <= 1e-6 * np.max(np.abs(mu64))
    assert not back.mu.flags.writeable
    # R16 is fp16(P - mu) for the STORED mu, exactly
    r16 = np.load(path + ".emb16.npy", mmap_mode="r")
    assert r16.dtype == np.float16 and r16.shape == (n, d)
    assert np.array_equal(np.asarray(r16).view(np.uint16), (P - mu).astype(np.float16).view(np.uint16))
    c = P - mu
    assert meta["max_centred_norm"] == math.sqrt(float(np.float32((c.astype(np.float64) ** 2).sum(axis=1).max())))
    assert meta["raw_max_norm"] == math.sqrt(float(np.float32((P.astype(np.float64) ** 2).sum(axis=1).max())))
    assert np.array_equal(meta["mu"], mu)
    # when the chunked sum rounds like numpy's, everything equals the one-shot restatement
    mu_r, r16_r, cn_r, rn_r = _restate(P)
    if np.array_equal(mu_r, mu):
        assert np.array_equal(r16_r.view(np.uint16), np.asarray(r16).view(np.uint16)) and meta["max_centred_norm"] == cn_r and meta["raw_max_norm"] == rn_r
    # an fp16-row index written again is the same pair of files; it has no fp32 form
    path2 = str(tmp_path / "h2.index")
    RU.write_index(back, path2, fp16=True)
    assert open(path + ".emb16.npy", "rb").read() == open(path2 + ".emb16.npy", "rb").read()
    with open(path2 + ".meta.pkl", "rb") as fh:
        meta2 = pickle.load(fh)
    assert meta2["max_centred_norm"] == meta["max_centred_norm"] and np.array_equal(meta2["mu"], meta["mu"])
    with pytest.raises(ValueError):
        RU.write_index(back, str(tmp_path / "no.index"))
    with pytest.raises(ValueError):
        back.add(P[:3])
    with pytest.raises(RuntimeError):
        back.search(P[:2], 5)                       # not on a GPU: refuses, as the fp32 form does


def test_v1_file_is_the_same_bytes_as_before(tmp_path):
    """The fp32 format is written as the parent commit wrote it: np.save of the rows + the four-key pickle."""
    P = syn.corpus_embeddings(62, 500, 64)
    ids = np.arange(500, dtype=np.int64) + 9
    index = RU.construct_flatindex_from_embeddings(P, ids)
    for name, kw in (("a", {}), ("b", {"fp16": False}), ("c", {"faiss_format": False, "fp16": False})):
        RU.write_index(index, str(tmp_path / name), **kw)
    np.save(str(tmp_path / "ref.emb.npy"), P)
    with open(tmp_path / "ref.meta.pkl", "wb") as fh:
        pickle.dump({"d": 64, "ids": ids, "id_offset": 0, "format": "cldrd-flatip-v1"}, fh)
    for name in "abc":
        assert (tmp_path / (name + ".emb.npy")).read_bytes() == (tmp_path / "ref.emb.npy").read_bytes()
        assert (tmp_path / (name + ".meta.pkl")).read_bytes() == (tmp_path / "ref.meta.pkl").read_bytes()
        assert not os.path.exists(str(tmp_path / (name + ".emb16.npy")))
    back = RU.read_index(str(tmp_path / "a"))
    assert back.row_dtype == "float32" and np.array_equal(back.embeddings, P) and back.mu is None


def test_fp16_and_faiss_format_exclude_each_other(tmp_path):
    index = RU.construct_flatindex_from_embeddings(syn.corpus_embeddings(63, 10, 64), None)
    with pytest.raises(ValueError):
        RU.write_index(index, str(tmp_path / "x"), faiss_format=True, fp16=True)
    assert os.listdir(tmp_path) == []


def test_fp16_file_refuses_rows_outside_the_fp16_range(tmp_path):
    P = syn.corpus_embeddings(64, 100, 64)
    P[7, 3] = 1.0e5
    with pytest.raises(ValueError):
        RU.write_index(RU.construct_flatindex_from_embeddings(P, None), str(tmp_path / "x"), fp16=True)
    P[7, 3] = np.nan
    with pytest.raises(ValueError):
        RU.write_index(RU.construct_flatindex_from_embeddings(P, None), str(tmp_path / "y"), fp16=True)


def test_command_lines_have_the_new_flags_default_off(tmp_path):
    from cldrd_amd.retriever import index_text, retrieve_top_passages
    a = index_text.get_args(["--index_dir", str(tmp_path / "i")])
    assert a.index_fp16 is False
    assert index_text.get_args(["--index_dir", str(tmp_path / "i"), "--index_fp16"]).index_fp16 is True
    b = retrieve_top_passages.get_args([])
    assert b.use_float16 is False
    assert retrieve_top_passages.get_args(["--use_float16"]).use_float16 is True


def test_call_surface():
    sig = inspect.signature(RU.convert_index_to_gpu)
    assert list(sig.parameters) == ["index", "faiss_gpu_index", "useFloat16"] and sig.parameters["useFloat16"].default is False
    assert inspect.signature(RU.FlatIPIndex.to_gpu).parameters["fp16_rows"].default is False
    assert inspect.signature(RU.FlatIPIndex.from_device_rows).parameters["fp16_rows"].default is False
    assert inspect.signature(RU.MultiDeviceFlatIPIndex.__init__).parameters["fp16_rows"].default is False
    assert 0 < RU.ATTACH_CHUNK_ROWS <= 1 << 20
    index = RU.FlatIPIndex(64)
    assert index.row_dtype == "float32" and index.mu is None
    for name in ("row_dtype", "mu"):
        with pytest.raises(AttributeError):
            setattr(index, name, None)


def test_sharded_index_carries_the_row_mode_of_its_local_index(tmp_path):
    """ShardedFlatIPIndex only exchanges and merges (scores, ids) lists; it reports what its local index holds and searches through it."""
    P = syn.corpus_embeddings(65, 40, 64)
    host = RU.construct_flatindex_from_embeddings(P, None)
    assert RU.ShardedFlatIPIndex(host).row_dtype == "float32"
    RU.write_index(host, str(tmp_path / "s"), fp16=True)
    assert RU.ShardedFlatIPIndex(RU.read_index(str(tmp_path / "s")), 0, 1).row_dtype == "float16"

    class Local:
        row_dtype, ntotal = "float16", 40

        def search(self, q, k):
            return "D", "I"
    sh = RU.ShardedFlatIPIndex(Local())
    assert sh.row_dtype == "float16" and sh.search(P[:2], 3) == ("D", "I")
