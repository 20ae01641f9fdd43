"""Exact resume of a training run (NwayTrainer.load_state_dict(exact=True), --resume_exact): a run that is saved, rebuilt from nothing and
continued equals the run that was never interrupted - parameters, Adam moments, the loss-scale block, dropout step counters, the step
counters, lr and the loss of every later step.  With ``deterministic=True`` the equality is of bits, so every comparison here is
``torch.equal`` on the bit patterns (float buffers are compared as int32 words: a NaN in the loss-scale block's scratch words must not make equal
blocks unequal) or ``==``; there is no tolerance anywhere in this file.

Set-up shared by the trainer tests: the 2-layer width-128 towers of the other trainer tests with dropout ON (0.1: with the tiny config's 0.0 the
dropout seeds would not matter), B = 2, N = 3, Lq = 8 batches that differ every step, and a save after step 6 - behind the graph capture at step 4,
so the resumed trainer goes through its eager warm-up and a capture of its own while the uninterrupted one replays."""
import io
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import cldrd_amd.synthetic as syn
import selftest
from cldrd_amd.encoder import EncoderConfig
from cldrd_amd.trainer import nway_listwise as T

N_SAVE, N_STEPS = 6, 12
LAYOUTS = ("padded", "packed16", "packed160")
LONG = torch.tensor([20, 140, 60, 160, 129, 100])       # passage lengths on both sides of 128: 63 % token fill, the encoder packs the batch


def _cfg():
    return EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=192,
                         dropout=0.1, attention_dropout=0.1)


def _trainer(seed, distill=None, deterministic=True):
    model = selftest.build_tiny_model(_cfg(), seed=seed).cuda().train()
    return T.NwayTrainer(model, loss="kl_div", learning_rate=1e-3, warmup_steps=2, total_steps=40, distill=distill, distill_alpha=0.5,
                         deterministic=deterministic)


def _batch(i, layout="padded", distill=False, poison=False):
    Lp = 160 if layout == "packed160" else 16
    b = syn.nway_batch(4680 + i, 2, 3, 8, Lp, vocab=512, ragged=False, label_kind="teacher", with_teacher_scores=distill)
    if layout != "padded":      # another assignment of lengths every step
        lens = LONG.roll(i) if Lp == 160 else 4 + (torch.arange(6) * 5 + i) % 13
        mask = (torch.arange(Lp)[None, :] < lens[:, None]).to(torch.int64).view(2, 3, Lp)
        b["nway_passages"]["attention_mask"] = mask
        b["nway_passages"]["input_ids"] = b["nway_passages"]["input_ids"] * mask
    if poison:
        b["labels"][1, 2] = float("inf")                 # a non-finite teacher score: every gradient is NaN, the safety net skips the step
    return T.batch_to_device(b, torch.device("cuda"))


def _batches(layout="padded", distill=False, poison_at=None, n=N_STEPS):
    return [_batch(i, layout, distill, poison=i == poison_at) for i in range(n)]


def _steps(tr, batches):
    return [tr.train_step(b).clone() for b in batches]


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(tr):
    torch.cuda.synchronize()
    return {"flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
            "loss_scale": tr._scale_state.clone() if tr._scale_state is not None else None,
            "step_seeds": [t.step_seed for t in tr.model.towers()], "global_step": tr.global_step, "adam_step": tr.adam_step, "lr": tr.lr(),
            "skipped_steps": tr.skipped_steps()}


def _same(a, b, where=""):
    """recursive equality of checkpoints / snapshots: tensors by their bits, containers item by item, everything else by =="""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape, where
        assert torch.equal(_bits(a), _bits(b)), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    else:
        assert a == b, (where, a, b)


def _through_a_file(ckpt):
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=False)


def _resumed_against_uninterrupted(layout, distill, poison_at=None, exact=True):
    """-> (snapshot, losses of steps 7..12, trainer) of the uninterrupted run and of the run saved after step 6 and continued by a model built from
    ANOTHER init seed under a fresh trainer"""
    batches = _batches(layout, distill is not None, poison_at)
    nw = batches[0]["nway_passages"]
    probe = _trainer(3, distill)
    assert probe.model.passage_encoder.would_pack(nw["lengths"], 6, nw["input_ids"].shape[-1]) == (layout != "padded"), "not the layout this case is about"
    a = probe
    la = _steps(a, batches)
    b = _trainer(3, distill)
    _steps(b, batches[:N_SAVE])
    if poison_at is not None:
        assert b.skipped_steps() == 1
    ckpt = _through_a_file(b.state_dict())
    del b
    c = _trainer(5, distill)
    assert not torch.equal(c.flat_p, a.flat_p)
    c.load_state_dict(ckpt, exact=exact)
    lc = _steps(c, batches[N_SAVE:])
    graphs = [sum(e["graph"] is not None for e in t._graphs.values()) for t in (a, c)]
    assert graphs == ([1, 1] if layout == "padded" else [0, 0]), graphs         # both went through a capture of their own (padded) / stayed eager
    return (_snapshot(a), la[N_SAVE:], a), (_snapshot(c), lc, c)


@pytest.mark.parametrize("distill", [None, "margin_mse"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_resumed_run_equals_the_uninterrupted_one(amp, layout, distill, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", amp)
    (sa, la, a), (sc, lc, _) = _resumed_against_uninterrupted(layout, distill)
    assert a.amp16 == (amp == "fp16") and sa["global_step"] == sa["adam_step"] == N_STEPS and sa["skipped_steps"] == 0
    assert (sa["loss_scale"] is not None) == (amp == "fp16")
    _same(sa, sc, "trainer")
    _same(la, lc, "loss")
    assert all(torch.isfinite(l).all().item() for l in la)


def test_resumed_run_with_a_skipped_step_keeps_both_counts(monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    (sa, la, a), (sc, lc, c) = _resumed_against_uninterrupted("padded", None, poison_at=2)
    assert sa["skipped_steps"] == 1 and sa["adam_step"] == N_STEPS
    _same(sa, sc, "trainer")
    _same(la, lc, "loss")
    oa, oc = a.optimizer_state_dict(), c.optimizer_state_dict()
    assert {int(st["step"]) for st in oa["state"].values()} == {N_STEPS - 1}      # scaler.step semantics: the skipped step is not in it
    _same(oa, oc, "optimizer")


def test_state_is_restored_without_the_deterministic_mode(monkeypatch):
    """Float atomics make the steps themselves unrepeatable here, so nothing computed is compared: what was saved is back, and the dropout seeds
    the two trainers write for their next steps - integers, a function of the restored counters - are the same."""
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    batches = _batches(n=N_SAVE + 4)
    b = _trainer(3, deterministic=False)
    _steps(b, batches[:N_SAVE])
    saved = _snapshot(b)
    c = _trainer(5, deterministic=False)
    c.load_state_dict(_through_a_file(b.state_dict()), exact=True)
    got = _snapshot(c)
    for k in ("loss_scale", "step_seeds", "global_step", "adam_step", "lr", "skipped_steps", "flat_p", "m", "v"):
        _same(saved[k], got[k], k)
    assert saved["step_seeds"] == [N_SAVE] * 2
    for tr in (b, c):
        tr.train_step(batches[N_SAVE])
    assert [t.step_seed for t in b.model.towers()] == [t.step_seed for t in c.model.towers()] == [N_SAVE + 1] * 2
    assert b._state is not None and c._state is None            # the saved trainer replays; the resumed one is in its eager warm-up ...
    for tr in (b, c):
        _steps(tr, batches[N_SAVE + 1:])
    torch.cuda.synchronize()
    assert c._state is not None                                 # ... and from its own capture on writes the seeds where `b` writes them
    assert torch.equal(b._state["seeds"], c._state["seeds"]) and int(b._state["seeds"][0]) == b.model.towers()[0].step_seed * 0x9E3779B1 & 0x7FFFFFFFFFFF


def test_loading_into_a_trainer_that_has_captured_a_graph(monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    batches = _batches(n=9)
    a = _trainer(3)
    _steps(a, batches[:3])
    ckpt = _through_a_file(a.state_dict())
    _steps(a, batches[3:5])                                     # capture at step 4, a replay at step 5
    assert len(a._graphs) == 1
    block = a._scale_state.data_ptr()
    a.load_state_dict(ckpt, exact=True)
    assert a._scale_state.data_ptr() == block and a.global_step == 3
    la = _steps(a, batches[3:])                                 # replays of the graph captured before the load
    d = _trainer(5)
    d.load_state_dict(ckpt, exact=True)
    ld = _steps(d, batches[3:])
    _same(_snapshot(a), _snapshot(d), "trainer")
    _same(la, ld, "loss")


def test_exact_load_refuses_what_it_cannot_continue(monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    src = _trainer(3)
    _steps(src, _batches(n=1))
    ckpt = _through_a_file(src.state_dict())
    assert ckpt["resume_state"]["version"] == 1 and ckpt["resume_state"]["amp"] == "fp16" and ckpt["resume_state"]["n_towers"] == 2
    assert set(ckpt) == {"global_step", "state_dict", "optimizer", "scheduler", "resume_state"}
    no_key = {k: v for k, v in ckpt.items() if k != "resume_state"}
    other_version = dict(ckpt, resume_state=dict(ckpt["resume_state"], version=99))
    fp16_tr = _trainer(5)
    monkeypatch.setenv("CLDRD_AMP", "bf16")
    bf16_tr = _trainer(5)
    assert not bf16_tr.amp16
    for tr, bad, field in ((fp16_tr, no_key, "resume_state"), (fp16_tr, other_version, "version"), (bf16_tr, ckpt, "amp")):
        before = tr.flat_p.clone()
        with pytest.raises(ValueError, match=f"'{field}'"):
            tr.load_state_dict(bad, exact=True)
        assert torch.equal(tr.flat_p, before) and tr.global_step == 0          # refused before anything was loaded
    for tr, bad in ((fp16_tr, no_key), (fp16_tr, other_version), (bf16_tr, ckpt)):
        tr.load_state_dict(bad)                                                # exact=False: as before, the key is not looked at
        assert torch.equal(tr.flat_p, src.flat_p) and tr.global_step == 1 and [t.step_seed for t in tr.model.towers()] == [0, 0]


# ---------------------------------------------------------------------------------------------------------- the command line
def _cli(folder, run, extra=()):
    return ["--experiment_folder", folder, "--run_folder", run, "--synthetic_steps", "8", "--synthetic_model", "tiny", "--num_train_epochs", "2",
            "--evaluate_steps", "5", "--deterministic", "--synthetic_nway", "4", "--label_mode", "9", "--passage_max_len", "32", "--query_max_len", "8",
            "--train_batch_size", "4", "--logging_steps", "2", "--warmup_steps", "2", "--learning_rate", "1e-3", "--loader_workers", "2"] + list(extra)


def _train(argv):
    """train() in process, as tests/test_trainer_cli.py runs it -> (trainer, train_step calls)"""
    calls = []
    real = T.NwayTrainer.train_step

    def counted(self, batch):
        calls.append(1)
        return real(self, batch)
    T.NwayTrainer.train_step = counted
    try:
        return T.train(T.set_env(T.get_args(argv))), len(calls)
    finally:
        T.NwayTrainer.train_step = real


@pytest.fixture(scope="module")
def run1(tmp_path_factory):
    """the uninterrupted run: two epochs of eight generated batches, checkpoints after steps 5, 10 (in the second epoch) and 15"""
    folder = str(tmp_path_factory.mktemp("resume_cli"))
    tr, n = _train(_cli(folder, "run1"))
    assert n == 16 and tr.global_step == 16
    return folder


def _ckpt(folder, run, step):
    return torch.load(os.path.join(folder, run, "models", f"checkpoint_{step}.pth.tar"), map_location="cpu", weights_only=False)


@pytest.mark.parametrize("k", [5, 10])
def test_command_line_resumes_where_the_checkpoint_was_written(run1, k):
    run = f"from{k}"
    tr, n = _train(_cli(run1, run, ["--resume", os.path.join(run1, "run1", "models", f"checkpoint_{k}.pth.tar"), "--resume_exact"]))
    assert n == 16 - k and tr.global_step == 16
    later = [s for s in (10, 15) if s > k]
    assert sorted(os.listdir(os.path.join(run1, run, "models"))) == [f"checkpoint_{s}.pth.tar" for s in later]
    for s in later:
        want, got = _ckpt(run1, "run1", s), _ckpt(run1, run, s)
        assert got["resume_state"]["epoch"] == (s - 1) // 8 and got["resume_state"]["step_in_epoch"] == (s - 1) % 8 + 1 and got["epoch"] == want["epoch"]
        for key in ("state_dict", "optimizer", "resume_state"):
            _same(want[key], got[key], f"checkpoint_{s}.{key}")


@pytest.mark.parametrize("flag,value", [("train_batch_size", "8"), ("seed", "1")])
def test_command_line_refuses_another_data_position(run1, flag, value):
    argv = _cli(run1, "refused", ["--resume", os.path.join(run1, "run1", "models", "checkpoint_5.pth.tar"), "--resume_exact"])
    argv[argv.index("--train_batch_size") + 1] = "8" if flag == "train_batch_size" else "4"
    with pytest.raises(ValueError, match=rf"{flag} was \d+ when the checkpoint was written and is {value} now"):
        _train(argv + (["--seed", value] if flag == "seed" else []))
    assert not os.path.exists(os.path.join(run1, "refused", "models", "checkpoint_10.pth.tar"))       # refused before the first step


def test_checkpoints_are_moved_into_place(run1):
    models = os.path.join(run1, "run1", "models")
    names = sorted(os.listdir(models))
    assert names == ["checkpoint_10.pth.tar", "checkpoint_15.pth.tar", "checkpoint_5.pth.tar"]      # and no temporary name
    assert all(re.fullmatch(r"checkpoint_\d+\.pth\.tar", n) for n in names)
    for s in (5, 10, 15):
        assert _ckpt(run1, "run1", s)["global_step"] == s
