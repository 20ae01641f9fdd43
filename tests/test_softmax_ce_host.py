"""``cldrd_softmax_ce`` and ``--loss softmax_ce`` without a GPU: the header, the ctypes table and the built library agree on the entry
point, every argument error is refused in front of any HIP call with a ``softmax_ce:`` message, the trainer's command line takes the new
flags and refuses the combinations that mean nothing with a ``ValueError`` that names the flag, and the captured step gains its one more
input only with ``--ce_mask_duplicate_pids``.

The ABI version: the entry point is added the way cldrd_lambda_term and the cosine scorer were, without a new number - three test files
pin 106 (test_lambda_term_host.py, test_score_store_host.py, test_stage_file_host.py) and `_lib.load` names a missing entry point itself."""
import ctypes as C
import os
import re

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
from cldrd_amd import _lib, hip_ops, losses, torch_ops
from cldrd_amd.trainer import nway_listwise as T

N_ARGS = 16


def test_the_entry_point_is_declared_bound_and_exported():
    text = open(os.path.join(conftest.ROOT, "include", "cldrd_hip.h")).read()
    assert "L_b  = (1/|P|) * sum_{i in P} [ log(exp(z_i) + Z) - z_i ]" in text           # the definition is in the header comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+cldrd_softmax_ce\s*\(([^)]*)\)", text)
    assert m, "include/cldrd_hip.h does not declare cldrd_softmax_ce"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == N_ARGS
    res, argtypes = _lib.SIGNATURES["cldrd_softmax_ce"]
    assert res is _lib.ci and len(argtypes) == N_ARGS
    for p, a in zip(params, argtypes):          # pointer <-> void*, int <-> c_int, float <-> c_float, position by position
        want = _lib.vp if "*" in p else (_lib.cf if p.startswith("float") else _lib.ci)
        assert a is want, (p, a)
    assert hasattr(_lib.load(), "cldrd_softmax_ce")
    assert _lib.load().cldrd_version() == _lib.ABI_VERSION
    assert "softmax_ce" in torch_ops.OPS and hasattr(torch.ops.cldrd, "softmax_ce")
    assert "cldrd::softmax_ce" in str(torch.ops.cldrd.softmax_ce.default._schema)
    assert losses.SoftmaxCE.__name__ == "SoftmaxCE"
    # it is an entry point of its own, not a sixth kind of cldrd_loss_fwd_bwd
    assert hip_ops.LOSS_KINDS == {"kl_div": 0, "margin_mse": 1, "ranknet": 2, "lambda_mrr": 3, "weighted_pointwise": 4}
    p = C.c_void_p(64)
    assert _lib.load().cldrd_loss_fwd_bwd(5, p, p, None, p, p, p, 2, 4, 1.0, -1.0, 1, None) != 0


def _call(**over):
    """cldrd_softmax_ce on fake non-null pointers: every case below must be refused before the library touches the GPU."""
    p = C.c_void_p(64)
    a = dict(logits=p, labels=p, B=2, Np=8, pids=None, N=0, mode=0, tau=0.05, pos_min=0.0, has_pos_min=0, neg_max=0.0, mean=1, loss_out=p,
             grad=p, workspace=p, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    lib = _lib.load()
    rc = lib.cldrd_softmax_ce(*a.values())
    return rc, lib.cldrd_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(logits=None), "null"), (dict(labels=None), "null"), (dict(loss_out=None), "null"), (dict(grad=None), "null"),
    (dict(workspace=None), "null"),
    (dict(tau=0.0), "tau"), (dict(tau=-1.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=float("inf")), "tau"),
    (dict(Np=0), "Np"), (dict(Np=8193), "Np"), (dict(B=0), "B > 0"),
    (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
    (dict(pids=C.c_void_p(64), N=4, mode=0), "Np does not match"),            # mode 0 needs Np == N
    (dict(pids=C.c_void_p(64), N=8, mode=1), "Np does not match"),            # mode 1 needs Np == B * N
    (dict(pids=C.c_void_p(64), N=8, mode=2), "Np does not match"),            # mode 2 needs Np == 2 * N
    (dict(pids=C.c_void_p(64), N=0, mode=0), "N >= 1"),
    (dict(has_pos_min=1, pos_min=0.0, neg_max=0.0), "pos_min > neg_max"), (dict(has_pos_min=1, pos_min=-1.0), "pos_min > neg_max"),
    (dict(has_pos_min=1, pos_min=float("nan")), "pos_min > neg_max"), (dict(neg_max=float("nan")), "neg_max"),
    (dict(has_pos_min=2), "0 or 1"), (dict(mean=2), "0 or 1"),
])
def test_bad_arguments_are_refused_without_a_gpu(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("softmax_ce:") and word in msg, (over, rc, msg)


def test_the_wrappers_check_before_the_library():
    z = torch.zeros
    with pytest.raises(ValueError, match="sum or mean"):
        hip_ops.softmax_ce(z(2, 6), z(2, 6), z(2), z(2, 6), reduction="max")
    with pytest.raises(ValueError, match="temperature"):
        hip_ops.softmax_ce(z(2, 6), z(2, 6), z(2), z(2, 6), temperature=0.0)
    with pytest.raises(ValueError, match="pos_min"):
        hip_ops.softmax_ce(z(2, 6), z(2, 6), z(2), z(2, 6), pos_min=0.0)
    with pytest.raises(RuntimeError):               # CPU tensors: no kernel, no fallback
        hip_ops.softmax_ce(z(2, 6), z(2, 6), z(2), z(2, 6))
    with pytest.raises(RuntimeError):
        losses.SoftmaxCE(0.05)(z(2, 6), z(2, 6))
    for kw in (dict(temperature=0.0), dict(pos_min=0.0), dict(pos_min=-0.1, neg_max=-0.1), dict(reduction="max")):
        with pytest.raises(ValueError):
            losses.SoftmaxCE(**kw)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out, grad = torch.ops.cldrd.softmax_ce(torch.empty(4, 8), torch.empty(4, 8), None, 0, 0.05, None, 0.0, True)
        assert out.shape == (2,) and grad.shape == (4, 8)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_the_command_line_takes_every_new_flag_and_the_defaults_stay():
    args = T.get_args([])
    assert args.loss == "lambda_mrr" and args.label_source == "rank"
    assert (args.ce_temperature, args.ce_pos_min, args.ce_neg_max, args.ce_mask_duplicate_pids) == (None, None, None, False)
    assert T.LOSS_KINDS == ("lambda_mrr", "ranknet", "kl_div", "margin_mse", "lambda_loss") and T.CONTRASTIVE_KINDS == ("softmax_ce",)
    assert T.CE_DEFAULTS == {"ce_temperature": 1.0, "ce_pos_min": None, "ce_neg_max": 0.0}
    args = T.get_args(["--loss", "softmax_ce", "--ce_temperature", "0.05", "--ce_pos_min", "0.3", "--ce_neg_max", "-0.2", "--ce_mask_duplicate_pids"])
    assert (args.loss, args.ce_temperature, args.ce_pos_min, args.ce_neg_max, args.ce_mask_duplicate_pids) == ("softmax_ce", 0.05, 0.3, -0.2, True)
    # with the in-batch columns, cosine scoring, the regulariser and the distillation term
    args = T.get_args(["--loss", "softmax_ce", "--in_batch_loss", "--all_in_batch_neg", "--apply_consine_similarity", "--cosine_scale", "20",
                       "--reg_lambda", "0.1", "--distill_loss", "margin_mse", "--label_mode", "6"])
    assert args.in_batch_loss and args.distill_loss == "margin_mse" and args.cosine_scale == 20.0
    for mode in ("1", "2", "3", "5", "7", "8", "9", "10"):          # every label mode with a negative column of its own
        assert T.get_args(["--loss", "softmax_ce", "--label_mode", mode]).label_mode == mode
    # synthetic batches carry the rank labels, as for lambda_mrr, and no teacher scores
    args = T.get_args(["--loss", "softmax_ce", "--synthetic_steps", "2", "--synthetic_nway", "4", "--label_mode", "6"])
    args.rank, args.nranks, args.synthetic_vocab, args.train_batch_size, args.query_max_len, args.passage_max_len = 0, 1, 512, 2, 8, 16
    batch = T._SyntheticBatches(args)[0]
    assert "teacher_scores" not in batch and float(batch["labels"].max()) == 1.0 and float(batch["labels"].min()) < 0.0


@pytest.mark.parametrize("argv,flag", [
    (["--ce_temperature", "0.05"], "--ce_temperature"),                                                   # the default --loss lambda_mrr
    (["--loss", "ranknet", "--ce_pos_min", "0.3"], "--ce_pos_min"),
    (["--loss", "lambda_loss", "--ce_neg_max", "-0.1"], "--ce_neg_max"),
    (["--loss", "kl_div", "--ce_mask_duplicate_pids"], "--ce_mask_duplicate_pids"),
    (["--loss", "softmax_ce", "--ce_temperature", "0"], "--ce_temperature"),
    (["--loss", "softmax_ce", "--ce_temperature", "-0.05"], "--ce_temperature"),
    (["--loss", "softmax_ce", "--ce_temperature", "nan"], "--ce_temperature"),
    (["--loss", "softmax_ce", "--ce_pos_min", "0"], "--ce_pos_min"),                                       # <= the default --ce_neg_max 0
    (["--loss", "softmax_ce", "--ce_pos_min", "0.3", "--ce_neg_max", "0.3"], "--ce_pos_min"),
    (["--loss", "softmax_ce", "--ce_pos_min", "0.3", "--ce_neg_max", "0.5"], "--ce_neg_max"),
    (["--loss", "softmax_ce", "--label_mode", "6"], "--in_batch_loss"),
    (["--loss", "softmax_ce", "--label_mode", "6"], "--label_mode 6"),
    (["--loss", "softmax_ce", "--label_mode", "7", "--ce_neg_max", "-0.1"], "--label_mode 7"),             # zeros are no negatives then
    (["--loss", "softmax_ce", "--ce_mask_duplicate_pids", "--synthetic_steps", "2"], "--ce_mask_duplicate_pids"),
])
def test_the_command_line_refuses_what_means_nothing_and_names_the_flag(argv, flag):
    with pytest.raises(ValueError, match=flag):
        T.get_args(argv)


def test_teacher_labels_are_refused_with_the_message_they_had():
    with pytest.raises(ValueError, match="--label_source teacher needs --loss lambda_loss .* got --loss softmax_ce"):
        T.get_args(["--loss", "softmax_ce", "--label_source", "teacher", "--ce_temperature", "0.05"])


def test_check_loss_options_gained_keyword_arguments_only():
    import inspect
    sig = inspect.signature(T.check_loss_options)
    names = list(sig.parameters)
    assert names[:6] == ["loss", "label_source", "in_batch_loss", "label_mode", "synthetic", "given"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[6:])
    assert names[6:] == ["ce_temperature", "ce_pos_min", "ce_neg_max", "ce_mask_duplicate_pids"]
    T.check_loss_options("lambda_mrr")                                                         # the old calls mean what they meant
    T.check_loss_options("lambda_loss", "teacher", False, "9", False, given=["neg_score_mode"])


def test_build_dataloader_refuses_a_label_mode_without_negatives_before_anything_is_loaded():
    args = T.get_args(["--loss", "softmax_ce", "--label_mode", "9", "--queries_path", "q", "--collection_path", "c", "--training_path", "t"])
    args.label_mode, args.distributed, args.rank, args.nranks = "6", False, 0, 1
    with pytest.raises(ValueError, match="--in_batch_loss"):          # before the tokenizer or any file is opened
        T.build_dataloader(args)


# ---------------------------------------------------------------------------------------------------------------- the captured step's inputs
def _cpu_trainer(mask, distill=None, distill_only=False):
    """What `_step_inputs` reads of a trainer (the constructor needs a GPU)."""
    tr = T.NwayTrainer.__new__(T.NwayTrainer)
    tr.distill, tr.distill_only, tr.label_source, tr.ce_mask_duplicate_pids = distill, distill_only, "rank", mask
    return tr


def _batch(B=3, N=4, with_pids=True):
    z = torch.zeros
    b = {"query": {"input_ids": z(B, 8, dtype=torch.int64), "attention_mask": z(B, 8, dtype=torch.int64)},
         "nway_passages": {"input_ids": z(B, N, 16, dtype=torch.int64), "attention_mask": z(B, N, 16, dtype=torch.int64)},
         "labels": z(B, N), "teacher_scores": z(B, N)}
    if with_pids:
        b["nway_pids"] = (torch.arange(B * N, dtype=torch.int64).view(B, N) + (1 << 40)).numpy()      # collate_fn returns a numpy array
    return b


def test_the_step_has_the_extra_input_only_with_the_duplicate_flag():
    plain = [w for w, _, _ in _cpu_trainer(False)._step_inputs(_batch())]
    assert plain == [("query", "input_ids"), ("nway_passages", "input_ids"), ("nway_passages", "attention_mask"), ("labels",),
                     ("query", "attention_mask")]
    assert [w for w, _, _ in _cpu_trainer(False)._step_inputs(_batch(with_pids=False))] == plain       # the key is not even looked at
    masked = _cpu_trainer(True)._step_inputs(_batch())
    assert [w for w, _, _ in masked] == plain + [("nway_pids",)]
    where, t, dtype = masked[-1]
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int64 and tuple(t.shape) == (3, 4) and dtype is None and int(t[0, 0]) == 1 << 40
    full = _cpu_trainer(True, distill="kl_div")._step_inputs(_batch())
    assert [w for w, _, _ in full] == plain + [("teacher_scores",), ("nway_pids",)] and len(full) == 7 <= 8
    assert [w for w, _, _ in _cpu_trainer(True, distill="kl_div", distill_only=True)._step_inputs(_batch())] == plain + [("teacher_scores",)]
    with pytest.raises(ValueError, match="nway_pids"):                                             # synthetic batches have none
        _cpu_trainer(True)._step_inputs(_batch(with_pids=False))
    bad = _batch()
    bad["nway_pids"] = bad["nway_pids"][:, :3]
    with pytest.raises(ValueError, match="nway_pids"):
        _cpu_trainer(True)._step_inputs(bad)
