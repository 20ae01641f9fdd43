"""The row mode of the flat index as a value (retriever.retrieval_utils): the flags -> requested mode helper and its refusal, the attach
decision of ``to_gpu`` over its whole table, and the single writer of stored rows fed from a file.  No GPU."""
import os

import numpy as np
import pytest

from cldrd_amd.retriever import retrieval_utils as RU

F32 = np.float32
FP16_ONLY = "this index holds fp16 rows only (read from an fp16-row file): int8 rows are quantised from fp32 rows"
NO_ROWS = "the index holds no rows"
# what the index holds on the host -> {requested mode: attached mode, or the text of the refusal}
TABLE = {"float32": {"float32": "float32", "float16": "float16", "int8": "int8"},             # host fp32 rows attach as asked
         "float16": {"float32": "float16", "float16": "float16", "int8": FP16_ONLY},          # an fp16-row file: fp16 rows, whatever is asked
         "int8": {"float32": "int8", "float16": "int8", "int8": "int8"},                      # an int8-row file: int8 rows, whatever is asked
         None: {"float32": "float32", "float16": NO_ROWS, "int8": NO_ROWS}}                   # nothing: the fp32 upload fails by itself, as before


@pytest.mark.parametrize("holds", list(TABLE), ids=str)
@pytest.mark.parametrize("requested", ["float32", "float16", "int8"])
def test_attach_decision_table(holds, requested):
    want = TABLE[holds][requested]
    if want in ("float32", "float16", "int8"):
        assert RU._attach_mode(holds, requested) == want
    else:
        with pytest.raises(ValueError) as e:
            RU._attach_mode(holds, requested)
        assert want in str(e.value) and str(e.value).startswith("FlatIPIndex.to_gpu:")


def test_to_gpu_decides_before_it_touches_a_device(tmp_path):
    """the refusals of the table reach the caller of ``to_gpu`` itself (device "cuda" is only parsed, never opened)"""
    P = (np.arange(300 * 64, dtype=F32).reshape(300, 64) % 17) - F32(8)
    path = str(tmp_path / "f16.index")
    RU.write_index(RU.construct_flatindex_from_embeddings(P, None), path, fp16=True)
    with pytest.raises(ValueError, match="holds fp16 rows only"):
        RU.read_index(path).to_gpu(0, int8_rows=True)
    for kw in ({"fp16_rows": True}, {"int8_rows": True}):
        with pytest.raises(ValueError, match=NO_ROWS):
            RU.FlatIPIndex(64).to_gpu(0, **kw)


@pytest.mark.parametrize("who,text", [("FlatIPIndex.to_gpu", "fp16_rows and int8_rows exclude one another"),
                                      ("FlatIPIndex.from_device_rows", "fp16_rows and int8_rows exclude one another"),
                                      ("FlatIPIndex.write", "fp16 and int8 exclude one another"),
                                      ("write_index", "int8=True excludes faiss_format=True and fp16=True")])
def test_exclusion_helper_names_its_caller(who, text):
    with pytest.raises(ValueError) as e:
        RU._requested_mode(True, True, who)
    assert str(e.value).startswith(who + ": ") and text in str(e.value)
    assert [RU._requested_mode(f, i, who) for f, i in ((False, False), (True, False), (False, True))] == ["float32", "float16", "int8"]


@pytest.mark.parametrize("mode", ["float32", "float16", "int8"])
def test_stored_rows_round_trip_is_byte_equal(tmp_path, mode):
    """write, read, write the read-back index again: the single writer fed from a file gives the bytes the encoder gave"""
    n, d = 300, 64
    g = np.random.default_rng(17)
    P = (g.standard_normal((n, d)) * g.uniform(0.2, 3.0, (n, 1)) + 0.25).astype(F32)
    kw = {"float32": {}, "float16": {"fp16": True}, "int8": {"int8": True}}[mode]
    first, second = str(tmp_path / "a.index"), str(tmp_path / "b.index")
    RU.write_index(RU.construct_flatindex_from_embeddings(P, np.arange(n, dtype=np.int64) * 5 + 2), first, **kw)
    back = RU.read_index(first)
    assert back.row_dtype == mode and back.ntotal == n and (back.embeddings is None) == (mode != "float32")
    RU.write_index(back, second, **kw)
    names = sorted(f[len("a.index"):] for f in os.listdir(tmp_path) if f.startswith("a.index"))
    assert names == {"float32": [".emb.npy", ".meta.pkl"], "float16": [".emb16.npy", ".meta.pkl"], "int8": [".emb8.npy", ".meta.pkl", ".scale.npy"]}[mode]
    assert sorted(f[len("b.index"):] for f in os.listdir(tmp_path) if f.startswith("b.index")) == names
    for ext in names:
        with open(first + ext, "rb") as fa, open(second + ext, "rb") as fb:
            assert fa.read() == fb.read(), ext
