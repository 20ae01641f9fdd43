"""Host side of the teacher score store (retriever/score_store.py, csrc/pairstore.hip): the two new entry points in the C ABI and their
argument checks, the missing-symbol guard of ``_lib.load``, and the store's metadata rules - commit order, lock, identity.  No GPU: the
stores here hold no segment, and every C call below is rejected in front of any HIP call."""
import json
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cldrd_hip.h")
NEW = ("cldrd_pair_lookup", "cldrd_pair_merge")

IDENTITY = {"teacher_sha256": "ab" * 32, "num_labels": 1, "max_len": 96, "arithmetic": "fp16",
            "query_cache.source_bytes": 1234, "query_cache.max_length": 96, "query_cache.tokenizer": "tok", "query_cache.vocab_size": 64,
            "passage_cache.source_bytes": 99999, "passage_cache.max_length": 96, "passage_cache.tokenizer": "tok",
            "passage_cache.vocab_size": 64}


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays():
    from cldrd_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/cldrd_hip.h"
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 106
    lib = _lib.load()
    assert lib.cldrd_version() == 106
    for name in NEW:
        assert hasattr(lib, name)


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """Small integers stand in for the device pointers: no call here may pass the checks."""
    from cldrd_amd import _lib
    lib = _lib.load()
    P, BIG = 64, 2 ** 31

    def lookup(seg=(P, P, P), n=10, qid=P, starts=P, pid=P, nq=4, total=40, out=P, hit=P):
        return "pair_lookup", lib.cldrd_pair_lookup(*seg, n, qid, starts, pid, nq, total, out, hit, None)

    def merge(a=(P, P, P), na=10, b=(P, P, P), nb=10, out=(P, P, P), flag=P):
        return "pair_merge", lib.cldrd_pair_merge(*a, na, *b, nb, *out, flag, None)

    cases = [
        lambda: lookup(seg=(None, P, P)), lambda: lookup(seg=(P, None, P)), lambda: lookup(seg=(P, P, None)), lambda: lookup(qid=None),
        lambda: lookup(starts=None), lambda: lookup(pid=None), lambda: lookup(out=None), lambda: lookup(hit=None),
        lambda: lookup(n=-1), lambda: lookup(n=0), lambda: lookup(n=BIG), lambda: lookup(nq=0), lambda: lookup(nq=-3), lambda: lookup(nq=BIG),
        lambda: lookup(total=-1),
        lambda: merge(a=(None, P, P)), lambda: merge(a=(P, None, P)), lambda: merge(a=(P, P, None)), lambda: merge(b=(None, P, P)),
        lambda: merge(b=(P, None, P)), lambda: merge(b=(P, P, None)), lambda: merge(out=(None, P, P)), lambda: merge(out=(P, None, P)),
        lambda: merge(out=(P, P, None)), lambda: merge(flag=None),
        lambda: merge(na=-1), lambda: merge(nb=-1), lambda: merge(na=0), lambda: merge(nb=0), lambda: merge(na=BIG), lambda: merge(nb=BIG),
        lambda: merge(na=BIG - 1, nb=1), lambda: merge(na=2 ** 30, nb=2 ** 30),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"


def test_a_build_that_lacks_a_symbol_is_named(monkeypatch):
    """Entry points are added under one ABI version: a CLDRD_LIB build without one of them raises CldrdError naming it."""
    import ctypes as C
    from cldrd_amd import _lib
    _lib.load()
    sigs = dict(_lib.SIGNATURES)
    sigs["cldrd_no_such_entry_point"] = (C.c_int, [C.c_void_p])
    monkeypatch.setattr(_lib, "SIGNATURES", sigs)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.CldrdError, match="cldrd_no_such_entry_point"):
        _lib.load()


def _open(path, identity=IDENTITY, **kw):
    from cldrd_amd.retriever.score_store import TeacherScoreStore
    return TeacherScoreStore(str(path), identity, "cpu", **kw)


def test_meta_is_the_commit_point(tmp_path):
    """Segment files that meta.json does not name are leftovers of an interrupted append: ignored and removed on open."""
    import numpy as np
    d = tmp_path / "store"
    _open(d).close()
    meta = json.loads((d / "meta.json").read_text())
    assert meta["segments"] == [] and meta["identity"] == IDENTITY and meta["format"] == 1 and len(meta["library_sha256"]) == 64
    assert not (d / ".lock").exists()
    for part, dt in (("q", np.int64), ("p", np.int64), ("s", np.float32)):
        np.save(d / f"seg-000000.{part}.npy", np.arange(3).astype(dt))
    (d / "meta.json.tmp").write_text("{")
    store = _open(d)
    assert store.segments == [] and len(store) == 0
    assert sorted(os.listdir(d)) == [".lock", "meta.json"]
    store.close()
    assert sorted(os.listdir(d)) == ["meta.json"]
    assert json.loads((d / "meta.json").read_text()) == meta


def test_a_lock_file_is_refused(tmp_path):
    from cldrd_amd.retriever.score_store import ScoreStoreError
    d = tmp_path / "store"
    store = _open(d)
    with pytest.raises(ScoreStoreError, match=re.escape(str(d / ".lock"))):
        _open(d)
    assert (d / ".lock").exists()           # the refused open did not take the first writer's lock away
    store.close()
    _open(d).close()


@pytest.mark.parametrize("field", sorted(IDENTITY))
def test_every_identity_field_is_checked(tmp_path, field):
    from cldrd_amd.retriever.score_store import ScoreStoreError
    d = tmp_path / "store"
    _open(d).close()
    other = dict(IDENTITY)
    other[field] = other[field] + 1 if isinstance(other[field], int) else ("bf16" if field == "arithmetic" else other[field] + "x")
    with pytest.raises(ScoreStoreError, match=re.escape(field + "=")):
        _open(d, other)
    assert not (d / ".lock").exists()       # a refused open leaves the store free
    _open(d).close()


def test_another_library_build_only_prints(tmp_path, capsys):
    d = tmp_path / "store"
    other_lib = tmp_path / "other.so"
    other_lib.write_bytes(b"another build")
    _open(d, library_path=str(other_lib)).close()
    assert "another build" not in capsys.readouterr().out
    store = _open(d)                        # this build's library against the recorded digest
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "another build of the kernel library" in out
    assert store.segments == []
    store.close()


def test_score_store_is_refused_with_dual_encoder(capsys):
    from cldrd_amd.retriever import rerank_top_passages as R
    base = ["--run_path", "r", "--queries_path", "q", "--collection_path", "c", "--model_name_or_path", "m", "--output_path", "o"]
    args = R.get_args(base + ["--score_store", "dir"])
    assert args.score_store == "dir" and args.score_store_flush_pairs >= 1
    assert R.get_args(base).score_store == ""
    with pytest.raises(SystemExit):
        R.get_args(base + ["--score_store", "dir", "--dual_encoder"])
    assert "--dual_encoder" in capsys.readouterr().err
    args = R.get_args(base + ["--dual_encoder"])
    args.score_store = "dir"
    with pytest.raises(ValueError, match="--score_store"):
        R.main(args)
