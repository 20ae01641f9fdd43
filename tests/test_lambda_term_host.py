"""``cldrd_lambda_term`` and ``--loss lambda_loss`` without a GPU: the header, the ctypes table and the built library agree on the entry
point, the ABI version stays, every argument error is refused in front of any HIP call with a ``lambda_term:`` message, and the trainer's
command line takes the new flags and refuses the combinations that mean nothing with a ``ValueError`` that names the flag."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
from cldrd_amd import _lib, hip_ops, torch_ops
from cldrd_amd.trainer import nway_listwise as T

N_ARGS = 24


def test_the_entry_point_is_declared_bound_and_exported():
    text = open(os.path.join(conftest.ROOT, "include", "cldrd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+cldrd_lambda_term\s*\(([^)]*)\)", text)
    assert m, "include/cldrd_hip.h does not declare cldrd_lambda_term"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == N_ARGS
    res, argtypes = _lib.SIGNATURES["cldrd_lambda_term"]
    assert res is _lib.ci and len(argtypes) == N_ARGS
    for p, a in zip(params, argtypes):          # pointer <-> void*, int <-> c_int, float <-> c_float, position by position
        want = _lib.vp if "*" in p else (_lib.cf if p.startswith("float") else _lib.ci)
        assert a is want, (p, a)
    assert hasattr(_lib.load(), "cldrd_lambda_term")
    assert _lib.ABI_VERSION == 106 and _lib.load().cldrd_version() == 106
    assert "lambda_term" in torch_ops.OPS and hasattr(torch.ops.cldrd, "lambda_term")
    assert hip_ops.LAMBDA_LABEL_FLAGS == {"mean": 1, "row_min": 2}
    # the neighbours this change must not touch
    assert len(_lib.SIGNATURES["cldrd_distill_term"][1]) == 12 and len(_lib.SIGNATURES["cldrd_lambda_loss_fwd_bwd"][1]) == 17
    assert hip_ops.DISTILL_KINDS == {"kl_div": 0, "margin_mse": 1} and T.DISTILL_KINDS == ("kl_div", "margin_mse")


def _call(**over):
    """cldrd_lambda_term on fake non-null pointers: every case below must be refused before the library touches the GPU."""
    p = C.c_void_p(64)
    a = dict(logits=p, B=2, Np=8, labels=p, Ns=6, label_flags=0, n_rel=6, label_offset=0.0, scheme=1, k=0, eps=1e-4, sigma=1.0, mu=10.0,
             pad=-1.0, mean=1, log2=0, linear=0, alpha=1.0, accumulate=0, loss_out=p, grad=p, term_out=None, workspace=p, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    lib = _lib.load()
    rc = lib.cldrd_lambda_term(*a.values())
    return rc, lib.cldrd_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(logits=None), "null"), (dict(labels=None), "null"), (dict(loss_out=None), "null"), (dict(grad=None), "null"),
    (dict(workspace=None), "null"),
    (dict(Ns=9), "Ns <= Np"), (dict(Ns=0), "1 <= Ns"), (dict(B=0), "B > 0"),
    (dict(Np=5000, Ns=4097, n_rel=0), "4096"),
    (dict(scheme=8), "scheme"), (dict(scheme=-1), "scheme"),
    (dict(alpha=-0.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
    (dict(n_rel=7), "n_rel"), (dict(n_rel=-1), "n_rel"),
    (dict(label_flags=4), "label_flags"), (dict(accumulate=2), "accumulate"),
])
def test_bad_arguments_are_refused_without_a_gpu(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("lambda_term:") and word in msg, (over, rc, msg)


def test_the_wrapper_checks_shapes_before_the_library():
    z = torch.zeros
    with pytest.raises(KeyError):
        hip_ops.lambda_term(z(2, 6), z(2, 6), z(2), z(2, 6), weighing_scheme="ndcg")
    with pytest.raises(ValueError):
        hip_ops.lambda_term(z(2, 6), z(2, 6), z(2), z(2, 6), gain="cubic")
    with pytest.raises(ValueError):
        hip_ops.lambda_term(z(2, 6), z(2, 6), z(2), z(2, 6), reduction="max")
    with pytest.raises(RuntimeError):               # CPU tensors: no kernel, no fallback
        hip_ops.lambda_term(z(2, 6), z(2, 6), z(2), z(2, 6))


def test_the_golden_file_has_the_cases_the_kernel_is_held_to():
    G = np.load(os.path.join(conftest.GOLDEN, "lambda_term.npz"))
    meta = json.loads(str(G["meta"]))
    shapes = {(G[n + ".logits"].shape[0], G[n + ".labels"].shape[1], G[n + ".logits"].shape[1] - G[n + ".labels"].shape[1]) for n in meta}
    assert {s[1] for s in shapes} == {2, 3, 30, 31, 255, 256, 257} and {s[0] for s in shapes} == {1, 3} and {s[2] for s in shapes} == {0, 5}
    assert {m["weighing_scheme"] for m in meta.values()} == set(hip_ops.LAMBDA_SCHEMES)
    assert {m["k"] for m in meta.values()} == {None, 1, 10} and {m["sigma"] for m in meta.values()} == {1.0, 2.0}
    assert {(m["gain"], m["reduction_log"], m["reduction"]) for m in meta.values()} >= {
        ("power", "natural", "mean"), ("power", "binary", "sum"), ("linear", "natural", "sum"), ("linear", "binary", "mean")}
    assert {(m["neg_mean"], m["row_min"]) for m in meta.values()} == {(False, False), (True, False), (False, True), (True, True)}
    assert {m["pad"] for m in meta.values()} == {-1.0, "-inf"}
    live = [int((G[n + ".labels"][b] != -1.0).sum()) for n, m in meta.items() if m["pad"] == -1.0 for b in range(G[n + ".labels"].shape[0])]
    assert 2 in live                                                                       # a row with only two live items
    assert any((G[n + ".labels"] < 0).all() for n, m in meta.items() if m["pad"] == "-inf")  # teacher-like labels, all negative
    assert all(np.isfinite(G[n + ".value"]) and np.isfinite(G[n + ".grad"]).all() for n in meta)


# ---------------------------------------------------------------------------------------------------------------- command line
LAMBDA_FLAGS = ["--weighing_scheme", "ndcgLoss1_scheme", "--lambda_k", "10", "--lambda_sigma", "2", "--lambda_mu", "5", "--lambda_gain", "linear",
                "--lambda_log", "binary"]


def test_the_command_line_takes_every_new_flag():
    args = T.get_args([])
    assert args.loss == "lambda_mrr" and args.label_source == "rank"
    assert all(getattr(args, k) is None for k in (*T.LAMBDA_DEFAULTS, *T.TEACHER_LABEL_DEFAULTS))
    assert T.LOSS_KINDS == ("lambda_mrr", "ranknet", "kl_div", "margin_mse", "lambda_loss")
    assert T.LAMBDA_DEFAULTS == {"weighing_scheme": "none", "lambda_k": 0, "lambda_sigma": 1.0, "lambda_mu": 10.0, "lambda_gain": "power",
                                 "lambda_log": "natural"}
    args = T.get_args(["--loss", "lambda_loss"] + LAMBDA_FLAGS)
    assert (args.weighing_scheme, args.lambda_k, args.lambda_sigma, args.lambda_mu, args.lambda_gain, args.lambda_log) == \
        ("ndcgLoss1_scheme", 10, 2.0, 5.0, "linear", "binary")
    for name in list(hip_ops.LAMBDA_SCHEMES)[1:] + ["none"]:
        assert T.get_args(["--loss", "lambda_loss", "--weighing_scheme", name]).weighing_scheme == name
    # the reference's four ndcg scripts
    for mode in ("original", "mean"):
        args = T.get_args(["--loss", "lambda_loss", "--weighing_scheme", "ndcgLoss1_scheme", "--label_source", "teacher", "--neg_score_mode", mode,
                           "--teacher_label_shift", "row_min", "--label_mode", "9"])
        assert (args.label_source, args.neg_score_mode, args.teacher_label_shift) == ("teacher", mode, "row_min")
    # they compose with the regulariser and the distillation term, and run on synthetic batches
    args = T.get_args(["--loss", "lambda_loss", "--label_source", "teacher", "--reg_lambda", "0.1", "--distill_loss", "margin_mse",
                       "--synthetic_steps", "2", "--label_mode", "1"])
    assert args.distill_loss == "margin_mse" and args.reg_lambda == 0.1
    args.rank, args.nranks, args.synthetic_vocab, args.synthetic_nway, args.train_batch_size = 0, 1, 512, 4, 2
    args.query_max_len, args.passage_max_len = 8, 16
    assert "teacher_scores" in T._SyntheticBatches(args)[0]
    assert T._n_rel(args) == 1
    args = T.get_args(["--loss", "lambda_loss", "--label_source", "teacher", "--synthetic_steps", "2", "--label_mode", "9", "--synthetic_nway", "6"])
    assert T._n_rel(args) == 6 and T._n_rel(T.get_args(["--label_mode", "9"])) == 10


@pytest.mark.parametrize("argv,flag", [
    (["--label_source", "teacher"], "--label_source"),                                                   # the default --loss lambda_mrr
    (["--loss", "ranknet", "--label_source", "teacher"], "--label_source"),
    (["--loss", "lambda_loss", "--label_source", "teacher", "--in_batch_loss"], "--in_batch_loss"),
    (["--loss", "lambda_loss", "--label_source", "teacher", "--label_mode", "1"], "--label_mode"),
    (["--weighing_scheme", "ndcgLoss1_scheme"], "--weighing_scheme"),
    (["--loss", "ranknet", "--lambda_k", "10"], "--lambda_k"),
    (["--loss", "kl_div", "--lambda_sigma", "2"], "--lambda_sigma"),
    (["--lambda_mu", "5"], "--lambda_mu"),
    (["--lambda_gain", "linear"], "--lambda_gain"),
    (["--lambda_log", "binary"], "--lambda_log"),
    (["--loss", "lambda_loss", "--neg_score_mode", "mean"], "--neg_score_mode"),
    (["--loss", "lambda_loss", "--teacher_label_shift", "row_min"], "--teacher_label_shift"),
    (["--loss", "lambda_loss", "--lambda_k", "-1"], "--lambda_k"),
])
def test_the_command_line_refuses_what_means_nothing_and_names_the_flag(argv, flag):
    with pytest.raises(ValueError, match=flag):
        T.get_args(argv)


def test_unknown_choices_are_argparse_errors(capsys):
    for argv in (["--loss", "ndcg"], ["--loss", "lambda_loss", "--weighing_scheme", "ndcgLoss3_scheme"], ["--label_source", "student"],
                 ["--loss", "lambda_loss", "--label_source", "teacher", "--neg_score_mode", "median"]):
        with pytest.raises(SystemExit):
            T.get_args(argv)
    capsys.readouterr()


def test_build_dataloader_refuses_teacher_labels_from_a_label_mode_1_file():
    args = T.get_args(["--loss", "lambda_loss", "--label_source", "teacher", "--label_mode", "9", "--queries_path", "q", "--collection_path", "c",
                       "--training_path", "t"])
    args.label_mode, args.distributed, args.rank, args.nranks = "1", False, 0, 1
    with pytest.raises(ValueError, match="--label_mode 1"):          # before the tokenizer or any file is opened
        T.build_dataloader(args)
