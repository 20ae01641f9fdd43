"""Cosine-similarity scoring without a GPU: the three C entry points are declared, bound and exported and reject bad arguments in front of any
HIP call (small integers stand in for device pointers), the command-line flags, the (checkpoint, flag) helper, what a checkpoint carries with
and without the mode, the refusal of an exact resume across the two modes, and the refusal of a cosine model on an index of raw rows."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import selftest
from cldrd_amd import _lib
from cldrd_amd import hip_ops as ops
from cldrd_amd.models import NwayDualEncoder
from cldrd_amd.retriever import retrieval_utils as RU
from cldrd_amd.trainer import nway_listwise as T

NEW = ("cldrd_score_cos_fwd", "cldrd_score_cos_bwd", "cldrd_l2_normalize_rows")


def test_the_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cldrd_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("score_cos_fwd", "score_cos_bwd", "l2_normalize_rows"):
        assert callable(getattr(ops, name))
    assert ops.COSINE_EPS == 1e-8
    from cldrd_amd import torch_ops
    assert "nway_score_cos" in torch_ops.OPS and hasattr(torch.ops.cldrd, "nway_score_cos")


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    P, B, N, d = 64, 2, 3, 8            # P: any non-null "pointer"
    nan, inf = float("nan"), float("inf")

    def fwd(q=P, p=P, logits=P, inv=P, d=d, mode=0, scale=1.0, eps=1e-8, B=B, N=N):
        return "score_cos_fwd", lib.cldrd_score_cos_fwd(q, p, logits, inv, B, N, d, mode, scale, eps, None)

    def bwd(dl=P, lg=P, q=P, p=P, inv=P, dq=P, dp=P, d=d, mode=0, scale=1.0, B=B, N=N):
        return "score_cos_bwd", lib.cldrd_score_cos_bwd(dl, lg, q, p, inv, dq, dp, B, N, d, mode, scale, None)

    def l2(x=P, ld=d, out=P + 4096, n=4, d=d, eps=1e-8):
        return "l2_normalize_rows", lib.cldrd_l2_normalize_rows(x, ld, out, n, d, eps, None)

    cases = [
        lambda: fwd(d=0), lambda: fwd(d=-4), lambda: fwd(d=6), lambda: bwd(d=0), lambda: bwd(d=6), lambda: l2(d=0, ld=0), lambda: l2(d=6, ld=8),
        lambda: fwd(eps=0.0), lambda: fwd(eps=-1e-8), lambda: fwd(eps=nan), lambda: l2(eps=0.0), lambda: l2(eps=-1.0), lambda: l2(eps=nan),
        lambda: fwd(scale=0.0), lambda: fwd(scale=-1.0), lambda: fwd(scale=nan), lambda: fwd(scale=inf),
        lambda: bwd(scale=0.0), lambda: bwd(scale=-20.0), lambda: bwd(scale=nan), lambda: bwd(scale=inf),
        lambda: fwd(mode=-1), lambda: fwd(mode=3), lambda: bwd(mode=-1), lambda: bwd(mode=3),
        lambda: fwd(q=None), lambda: fwd(p=None), lambda: fwd(logits=None), lambda: fwd(inv=None),
        lambda: bwd(dl=None), lambda: bwd(lg=None), lambda: bwd(q=None), lambda: bwd(p=None), lambda: bwd(inv=None), lambda: bwd(dq=None),
        lambda: bwd(dp=None), lambda: l2(x=None), lambda: l2(out=None),
        lambda: l2(ld=d - 4), lambda: l2(ld=d + 2), lambda: l2(out=P, ld=d + 4),            # a short, an unaligned stride; in place over padded rows
        lambda: fwd(B=0), lambda: fwd(N=0), lambda: bwd(B=0),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"
    # the wrappers refuse host tensors and a short inv_norms before the library is asked
    with pytest.raises(RuntimeError, match="GPU"):
        ops.l2_normalize_rows(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.score_cos_fwd(torch.zeros(2, 8), torch.zeros(6, 8), torch.zeros(2, 3), torch.zeros(8), 2, 3)


def test_command_line_flags(capsys):
    a = T.get_args([])
    assert a.apply_consine_similarity is False and a.cosine_scale is None and T._cosine_kw(a) == {}
    for flag in ("--apply_consine_similarity", "--apply_cosine_similarity"):          # the reference's spelling and the dictionary's
        b = T.get_args([flag])
        assert b.apply_consine_similarity is True and T._cosine_kw(b) == {"cosine": True, "cosine_scale": 1.0}
        c = T.get_args([flag, "--cosine_scale", "20"])
        assert T._cosine_kw(c) == {"cosine": True, "cosine_scale": 20.0}
    with pytest.raises(SystemExit):
        T.get_args(["--cosine_scale", "20"])
    assert "--apply_consine_similarity" in capsys.readouterr().err                    # the error names the flag
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            T.get_args(["--apply_consine_similarity", "--cosine_scale", bad])
    from cldrd_amd.evaluation import continue_rerank_evaluator as C
    from cldrd_amd.retriever import build_stage_file as B, index_text as I, rerank_top_passages as R, retrieve_top_passages as S
    for flag in ("--apply_consine_similarity", "--apply_cosine_similarity"):
        assert I.get_args(["--index_dir", os.path.join(ROOT, "tests"), flag]).apply_consine_similarity is True
        assert S.get_args([flag]).apply_consine_similarity is True
        assert R.get_args(["--run_path", "r", "--queries_path", "q", "--collection_path", "c", "--model_name_or_path", "m", "--output_path", "o",
                           "--dual_encoder", flag]).apply_consine_similarity is True
        assert C.get_args(["--resume_folder", "f", "--dev_path", "d", "--dev_queries_path", "q", "--dev_qrels_path", "r", "--collection_path", "c",
                           "--output_path", "o", flag]).apply_consine_similarity is True
    assert S.get_args([]).apply_consine_similarity is False
    import inspect
    assert "apply_consine_similarity" in inspect.getsource(B.get_args)


def test_cosine_of_checkpoint_and_flag():
    score = {"kind": "cosine", "scale": 20.0, "eps": 1e-8}
    assert RU.cosine_of(None, False) is False and RU.cosine_of({"state_dict": {}}, False) is False          # neither
    assert RU.cosine_of({"score": score}, False) is True                                                     # the checkpoint says so
    assert RU.cosine_of(None, True) is True and RU.cosine_of({"state_dict": {}}, True) is True               # the flag says so
    assert RU.cosine_of({"score": score}, True) is True                                                      # both
    assert RU.cosine_of({"score": {"kind": "dot"}}, False) is False

    class M:
        cosine, cosine_scale = False, 1.0
    m = M()
    assert RU.set_score_mode(m, {"score": score}) is True and m.cosine is True and m.cosine_scale == 20.0
    m = M()
    assert RU.set_score_mode(m, None, True) is True and m.cosine_scale == 1.0
    m = M()
    assert RU.set_score_mode(m, {"state_dict": {}}) is False and m.cosine is False


def test_model_keywords_are_keyword_only_and_default_off():
    cfg = selftest.tiny_config()
    m = NwayDualEncoder(cfg, False)
    assert m.cosine is False and m.cosine_scale == 1.0
    m = NwayDualEncoder(cfg, False, False, True, cosine=True, cosine_scale=20)
    assert m.cosine is True and m.cosine_scale == 20.0
    with pytest.raises(TypeError):
        NwayDualEncoder(cfg, False, False, True, True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cosine_scale"):
            NwayDualEncoder(cfg, False, cosine=True, cosine_scale=bad)
    assert sorted(m.state_dict()) == sorted(NwayDualEncoder(cfg, False).state_dict())          # no new parameter or buffer


def _cpu_trainer(cosine=False, scale=1.0):
    """What state_dict / resume_state / the exact-resume check read of a trainer, on a CPU model (the constructor needs a GPU)."""
    model = NwayDualEncoder(selftest.tiny_config(), share_weights=False, cosine=cosine, cosine_scale=scale)
    tr = T.NwayTrainer.__new__(T.NwayTrainer)
    tr.model, tr.cosine, tr.cosine_scale = model, model.cosine, model.cosine_scale
    tr.amp16, tr._scale_state, tr.global_step, tr.adam_step = False, None, 0, 0
    tr.lr0, tr.wd, tr.eps, tr.betas, tr.warmup_steps, tr.total_steps = 1e-3, 0.01, 1e-8, (0.9, 0.999), 1, 10
    return tr


def test_checkpoint_keys_with_and_without_the_mode():
    plain = _cpu_trainer()
    ckpt = plain.state_dict()
    assert sorted(ckpt) == ["global_step", "optimizer", "resume_state", "scheduler", "state_dict"]           # exactly today's keys
    assert "score" not in ckpt["resume_state"] and plain.score_state() is None
    assert sorted(ckpt["resume_state"]) == sorted(["version", "step_seeds", "loss_scale", "skipped_steps", "adam_step", "global_step", "amp",
                                                   "share_weights", "n_towers"])
    cos = _cpu_trainer(True, 20.0)
    ckpt = cos.state_dict()
    want = {"kind": "cosine", "scale": 20.0, "eps": 1e-8}
    assert ckpt["score"] == want and ckpt["resume_state"]["score"] == want
    assert sorted(set(ckpt) - {"score"}) == ["global_step", "optimizer", "resume_state", "scheduler", "state_dict"]
    assert RU.cosine_of(ckpt) is True and RU.cosine_of(plain.state_dict()) is False


def test_exact_resume_is_refused_across_the_two_modes():
    plain, cos, cos5 = _cpu_trainer(), _cpu_trainer(True, 20.0), _cpu_trainer(True, 5.0)
    for saver, loader in ((cos, plain), (plain, cos), (cos, cos5)):
        with pytest.raises(ValueError, match="'score'"):
            loader._checked_resume_state({"resume_state": saver.resume_state()})
    for tr in (plain, cos):
        assert tr._checked_resume_state({"resume_state": tr.resume_state()})["global_step"] == 0


def test_index_mark_and_the_refusal_of_raw_rows(tmp_path):
    rows = np.random.default_rng(0).standard_normal((5, 64)).astype(np.float32)
    raw = RU.FlatIPIndex(64)
    raw.add_with_ids(rows, np.arange(5, dtype=np.int64))
    assert raw.normalized is False
    raw.write(str(tmp_path / "raw"))
    with open(tmp_path / "raw.meta.pkl", "rb") as fh:
        assert sorted(pickle.load(fh)) == ["d", "format", "id_offset", "ids"]                # a raw index: the keys it always had
    unit = RU.FlatIPIndex(64)
    unit.add_with_ids(rows / np.linalg.norm(rows, axis=1, keepdims=True), np.arange(5, dtype=np.int64))
    unit.normalized = True
    for name, kw in (("unit", {}), ("unit16", {"fp16": True}), ("unit8", {"int8": True})):
        unit.write(str(tmp_path / name), **kw)
        with open(tmp_path / (name + ".meta.pkl"), "rb") as fh:
            assert pickle.load(fh)["normalized"] is True
        assert RU.read_index(str(tmp_path / name)).normalized is True
    back = RU.read_index(str(tmp_path / "raw"))
    assert back.normalized is False
    RU.check_index_normalized(back, False, "raw")                   # a dot-product model: any index
    RU.check_index_normalized(unit, False, "unit")                  # ... also one of unit rows
    RU.check_index_normalized(unit, True, "unit")
    with pytest.raises(ValueError, match="raw rows.*rebuil"):
        RU.check_index_normalized(back, True, str(tmp_path / "raw"))
