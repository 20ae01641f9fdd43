"""Host side of teacher-score distillation: ``curriculum_file --with_scores`` writes the teacher's scores next to the pids,
``NwayDataset(..., teacher_scores=True)`` collates them into ``batch["teacher_scores"]``, the trainer's command line and the synthetic
loader carry the new options, and the C entry point is declared and bound.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
from cldrd_amd.dataset import curriculum_file as C
from cldrd_amd.dataset.nway_dataset import NwayDataset

SCORE_KEYS = {"relT_pids": "relT_scores", "most_hard_pids": "most_hard_scores", "semi_hard_pids": "semi_hard_scores"}
WINDOWS = dict(most_hard_ranks="11:30", semi_hard_ranks="31:60")


def scored_run(path, n_q=12, k=60, seed=31):
    """n_q queries x k candidates with distinct scores that do not round-trip through float32 (many digits), lines shuffled.
    Returns {qid: {pid: score as parsed from the written text}}."""
    rng = np.random.default_rng(seed)
    qids = rng.choice(10 ** 6, n_q, replace=False)
    rows, table = [], {}
    for q in qids:
        sc = rng.normal(0.0, 4.0, k)
        for r, (p, s) in enumerate(zip(rng.choice(10 ** 5, k, replace=False), sc)):
            text = repr(float(s))
            rows.append(f"{q}\t{p}\t{r + 1}\t{text}\n")
            table.setdefault(int(q), {})[int(p)] = float(text)
    with open(path, "w") as fh:
        fh.write("".join(rows[i] for i in rng.permutation(len(rows))))
    return table


def read_lines(path):
    with open(path) as fh:
        return [json.loads(line) for line in fh]


def test_with_scores_writes_the_run_scores_next_to_the_pids(tmp_path):
    run = tmp_path / "teacher.run"
    table = scored_run(run)
    plain, scored = tmp_path / "plain.json", tmp_path / "scored.json"
    assert C.build_curriculum_file(str(run), str(plain), "9", seed=3, **WINDOWS) == (12, 0)
    assert C.build_curriculum_file(str(run), str(scored), "9", seed=3, with_scores=True, **WINDOWS) == (12, 0)
    a, b = read_lines(plain), read_lines(scored)
    assert len(a) == len(b) == 12
    for ex0, ex in zip(a, b):
        assert set(ex0) == {"qid", "relT_pids", "most_hard_pids", "semi_hard_pids"}          # without the flag: the four present keys
        assert set(ex) == set(ex0) | set(SCORE_KEYS.values())
        assert {k: ex[k] for k in ex0} == ex0                                                # the pids do not depend on the flag
        for pk, sk in SCORE_KEYS.items():
            assert len(ex[sk]) == len(ex[pk])
            want = np.array([table[ex["qid"]][p] for p in ex[pk]], dtype=np.float64).astype(np.float32)
            assert np.array_equal(np.array(ex[sk], dtype=np.float64).astype(np.float32), want)
        rel = ex["relT_scores"]
        assert all(x >= y for x, y in zip(rel, rel[1:]))
        assert min(rel) >= max(ex["most_hard_scores"]) >= min(ex["most_hard_scores"]) >= max(ex["semi_hard_scores"])
    # the library pieces: select_examples carries the scores, write_examples refuses examples without them
    spec = C.curriculum_spec("9", **WINDOWS)
    ex = C.select_examples(C.read_teacher_run(str(run)), spec, 3, with_scores=True)
    assert ex.relT_scores.shape == ex.relT.shape and ex.most_hard_scores.shape == ex.most_hard.shape
    assert ex.semi_hard_scores.shape == ex.semi_hard.shape and ex.relT_scores.dtype == np.float64
    ex0 = C.select_examples(C.read_teacher_run(str(run)), spec, 3)
    assert ex0.relT_scores is None and np.array_equal(ex0.relT, ex.relT)
    with pytest.raises(ValueError, match="with_scores"):
        C.write_examples(str(tmp_path / "x.json"), ex0, with_scores=True)


def test_with_scores_command_line_and_default_output_bytes(tmp_path):
    run = tmp_path / "teacher.run"
    scored_run(run, n_q=5)
    base = ["--run_path", str(run), "--label_mode", "9", "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "4"]
    args = C.get_args(base + ["--output_path", str(tmp_path / "cli_plain.json")])
    assert args.with_scores is False
    C.main(args)
    C.main(C.get_args(base + ["--output_path", str(tmp_path / "cli_scored.json"), "--with_scores"]))
    C.build_curriculum_file(str(run), str(tmp_path / "lib_plain.json"), "9", "11:30", "31:60", None, 4)
    C.build_curriculum_file(str(run), str(tmp_path / "lib_scored.json"), "9", "11:30", "31:60", None, 4, with_scores=True)
    assert (tmp_path / "cli_plain.json").read_bytes() == (tmp_path / "lib_plain.json").read_bytes()
    assert (tmp_path / "cli_scored.json").read_bytes() == (tmp_path / "lib_scored.json").read_bytes()
    # byte for byte the format of a file without scores: json.dumps of the four keys in their order
    for line, ex in zip((tmp_path / "cli_plain.json").read_text().splitlines(), read_lines(tmp_path / "cli_plain.json")):
        assert line == json.dumps({k: ex[k] for k in ("qid", "relT_pids", "most_hard_pids", "semi_hard_pids")})
    assert all("relT_scores" in ex for ex in read_lines(tmp_path / "cli_scored.json"))


def test_a_non_finite_selected_score_is_refused_with_the_qid(tmp_path):
    run = tmp_path / "teacher.run"
    rows = [f"7\t{100 + r}\t{r + 1}\t{60.0 - r}\n" for r in range(60)] + [f"8\t{100 + r}\t{r + 1}\t{60.0 - r}\n" for r in range(60)]
    rows[60 + 3] = "8\t103\t4\tinf\n"           # sorts first: a relT position of qid 8
    run.write_text("".join(rows))
    with pytest.raises(ValueError, match="qid 8"):
        C.build_curriculum_file(str(run), str(tmp_path / "o.json"), "9", with_scores=True, **WINDOWS)
    assert C.build_curriculum_file(str(run), str(tmp_path / "o.json"), "9", **WINDOWS) == (2, 0)          # without scores: as before


def _tables(tmp_path, pids, qids):
    from toy_tokenizer import WORDS
    q_path, c_path = tmp_path / "queries.tsv", tmp_path / "collection.tsv"
    q_path.write_text("".join(f"{q}\t{' '.join(WORDS[(q + i) % len(WORDS)] for i in range(3))}\n" for q in qids))
    c_path.write_text("".join(f"{p}\t{' '.join(WORDS[(p * 7 + i) % len(WORDS)] for i in range(1 + p % 9))}\n" for p in pids))
    return q_path, c_path


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if hasattr(a, "keys"):
        return sorted(a.keys()) == sorted(b.keys()) and all(_same(a[k], b[k]) for k in a.keys())
    return a == b


@pytest.mark.parametrize("mode,ctor", [("9", "create_from_10relT_20neg_file"), ("8", "create_from_5relT_25neg_file"),
                                       ("9", "create_from_relT_most_semi_hard_file")])
def test_dataset_collates_the_teacher_scores(mode, ctor, tmp_path):
    from toy_tokenizer import make_tokenizer
    run = tmp_path / "teacher.run"
    table = scored_run(run, n_q=6)
    out = tmp_path / "train.json"
    C.build_curriculum_file(str(run), str(out), mode, seed=2, with_scores=True,
                            most_hard_ranks="11:30" if mode == "9" else "6:30", semi_hard_ranks="31:60")
    q_path, c_path = _tables(tmp_path, sorted({p for t in table.values() for p in t}), list(table))
    a = (str(q_path), str(c_path), str(out), make_tokenizer(), 8, 12, mode)
    ds = getattr(NwayDataset, ctor)(*a, teacher_scores=True)
    ds0 = getattr(NwayDataset, ctor)(*a)
    items = [ds[i] for i in range(4)]
    assert all(len(it["teacher_scores"]) == 30 for it in items) and "teacher_scores" not in ds0[0]
    batch, batch0 = ds.collate_fn(items), ds0.collate_fn([ds0[i] for i in range(4)])
    ts = batch["teacher_scores"]
    assert ts.dtype == torch.float32 and tuple(ts.shape) == (4, 30) and tuple(batch["nway_pids"].shape) == (4, 30)
    for b in range(4):
        want = np.array([table[int(batch["qid"][b])][int(p)] for p in batch["nway_pids"][b]], dtype=np.float64).astype(np.float32)
        assert np.array_equal(ts[b].numpy(), want)
    assert "teacher_scores" not in batch0
    assert sorted(batch0) == sorted(k for k in batch if k != "teacher_scores")
    assert all(_same(batch[k], batch0[k]) for k in batch0)
    # the token-cache path gives the same batch, scores included
    dsc = getattr(NwayDataset, ctor)(*a, teacher_scores=True).with_token_cache(str(tmp_path / "cache"))
    batch_c = dsc.collate_fn([dsc[i] for i in range(4)])
    assert "query" not in dsc[0] and sorted(batch_c) == sorted(batch)
    assert all(_same(batch[k], batch_c[k]) for k in batch)


def test_dataset_refusals_at_load_time(tmp_path):
    from toy_tokenizer import make_tokenizer
    run = tmp_path / "teacher.run"
    table = scored_run(run, n_q=4)
    plain, scored = tmp_path / "plain.json", tmp_path / "scored.json"
    C.build_curriculum_file(str(run), str(plain), "9", **WINDOWS)
    C.build_curriculum_file(str(run), str(scored), "9", with_scores=True, **WINDOWS)
    q_path, c_path = _tables(tmp_path, sorted({p for t in table.values() for p in t}), list(table))
    tok = make_tokenizer()
    first_qid = read_lines(plain)[0]["qid"]
    with pytest.raises(ValueError, match=f"qid {first_qid}.*relT_scores"):          # a file without the score keys
        NwayDataset.create_from_10relT_20neg_file(str(q_path), str(c_path), str(plain), tok, 8, 12, "9", teacher_scores=True)
    lines = read_lines(scored)
    lines[2]["semi_hard_scores"] = lines[2]["semi_hard_scores"][:-1]
    short = tmp_path / "short.json"
    short.write_text("".join(json.dumps(ex) + "\n" for ex in lines))
    with pytest.raises(ValueError, match=f"qid {lines[2]['qid']}.*semi_hard_scores"):
        NwayDataset.create_from_10relT_20neg_file(str(q_path), str(c_path), str(short), tok, 8, 12, "9", teacher_scores=True)
    del lines[2]["semi_hard_scores"]
    short.write_text("".join(json.dumps(ex) + "\n" for ex in lines))
    with pytest.raises(ValueError, match=f"qid {lines[2]['qid']}"):
        NwayDataset.create_from_relT_most_semi_hard_file(str(q_path), str(c_path), str(short), tok, 8, 12, "9", teacher_scores=True)
    # label mode 1: that file format has no scores
    ex1 = [{"qid": 1, "relT_pids": [5], "neg_pids": [6, 7, 8, 9, 10]}]
    with pytest.raises(ValueError, match="label mode 1"):
        NwayDataset({1: "alpha"}, {p: "beta" for p in range(5, 11)}, ex1, tok, 8, 12, label_mode="1", teacher_scores=True)
    assert len(NwayDataset({1: "alpha"}, {p: "beta" for p in range(5, 11)}, ex1, tok, 8, 12, label_mode="1")) == 1
    # a scored file read without the flag is an ordinary file
    ds = NwayDataset.create_from_10relT_20neg_file(str(q_path), str(c_path), str(scored), tok, 8, 12, "9")
    assert "teacher_scores" not in ds.collate_fn([ds[0], ds[1]])


def test_trainer_command_line_defaults_and_refusals(capsys):
    from cldrd_amd.trainer import nway_listwise as T
    args = T.get_args([])
    assert args.distill_loss is None and args.distill_alpha == 1.0 and args.distill_T == 1.0 and args.distill_only is False
    args = T.get_args(["--distill_loss", "margin_mse", "--distill_alpha", "0.5", "--label_mode", "9"])
    assert (args.distill_loss, args.distill_alpha, args.distill_T, args.loss) == ("margin_mse", 0.5, 1.0, "lambda_mrr")
    assert T.get_args(["--distill_loss", "kl_div", "--distill_T", "2", "--distill_only"]).distill_only is True
    for bad in (["--distill_loss", "ranknet"], ["--distill_only"], ["--distill_loss", "kl_div", "--label_mode", "1"],
                ["--distill_loss", "kl_div", "--distill_T", "0"], ["--distill_loss", "kl_div", "--distill_alpha", "-1"]):
        with pytest.raises(SystemExit):
            T.get_args(bad)
    capsys.readouterr()
    assert T.DISTILL_KINDS == ("kl_div", "margin_mse")


def test_build_dataloader_refuses_label_mode_1_with_a_distillation_loss(tmp_path, monkeypatch):
    import transformers
    from cldrd_amd.trainer import nway_listwise as T
    from toy_tokenizer import make_tokenizer
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: make_tokenizer()))
    args = T.get_args(["--distill_loss", "kl_div", "--label_mode", "9", "--queries_path", "q", "--collection_path", "c", "--training_path", "t"])
    args.label_mode, args.distributed, args.rank, args.nranks = "1", False, 0, 1
    with pytest.raises(ValueError, match="label mode 1"):
        T.build_dataloader(args)


def test_build_dataloader_asks_the_dataset_for_teacher_scores(tmp_path, monkeypatch):
    import transformers
    from cldrd_amd.trainer import nway_listwise as T
    from toy_tokenizer import make_tokenizer
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: make_tokenizer()))
    run = tmp_path / "teacher.run"
    table = scored_run(run, n_q=6)
    out = tmp_path / "train.json"
    C.build_curriculum_file(str(run), str(out), "9", with_scores=True, **WINDOWS)
    q_path, c_path = _tables(tmp_path, sorted({p for t in table.values() for p in t}), list(table))
    base = ["--label_mode", "9", "--queries_path", str(q_path), "--collection_path", str(c_path), "--training_path", str(out),
            "--train_batch_size", "2", "--loader_workers", "0", "--query_max_len", "8", "--passage_max_len", "12"]
    for extra, want in ((["--distill_loss", "margin_mse"], True), ([], False)):
        args = T.get_args(base + extra)
        args.distributed, args.rank, args.nranks = False, 0, 1
        ds, loader = T.build_dataloader(args)
        assert ds.teacher_scores is want
        batch = next(iter(loader))
        assert ("teacher_scores" in batch) is want
        if want:
            assert tuple(batch["teacher_scores"].shape) == (2, 30) and batch["teacher_scores"].dtype == torch.float32


def test_synthetic_batches_have_teacher_scores_only_when_asked():
    import cldrd_amd.synthetic as syn
    plain = syn.nway_batch(5, 3, 6, 8, 16, vocab=512, label_kind="mode9")
    asked = syn.nway_batch(5, 3, 6, 8, 16, vocab=512, label_kind="mode9", with_teacher_scores=True)
    assert "teacher_scores" not in plain and sorted(asked) == sorted(list(plain) + ["teacher_scores"])
    ts = asked["teacher_scores"]
    assert ts.dtype == torch.float32 and tuple(ts.shape) == (3, 6) and torch.isfinite(ts).all()
    assert torch.equal(ts, syn.nway_batch(5, 3, 6, 8, 16, vocab=512, label_kind="mode9", with_teacher_scores=True)["teacher_scores"])
    assert not torch.equal(ts, syn.nway_batch(6, 3, 6, 8, 16, vocab=512, label_kind="mode9", with_teacher_scores=True)["teacher_scores"])
    assert 2.0 < float(ts.max() - ts.min()) < 60.0                     # cross-encoder-like spread, not labels in [-0.5, 1]
    assert all(_same(plain[k], asked[k]) for k in plain)
    # the command line's synthetic loader asks for them exactly when a distillation loss is set
    from cldrd_amd.trainer import nway_listwise as T
    for extra, want in ((["--distill_loss", "kl_div"], True), ([], False)):
        args = T.get_args(["--synthetic_steps", "2", "--synthetic_nway", "4", "--train_batch_size", "2", "--query_max_len", "8",
                           "--passage_max_len", "16"] + extra)
        args.rank, args.nranks, args.synthetic_vocab = 0, 1, 512
        assert ("teacher_scores" in T._SyntheticBatches(args)[0]) is want


def test_the_entry_point_is_declared_and_bound():
    from cldrd_amd import _lib, hip_ops, torch_ops
    text = open(os.path.join(conftest.ROOT, "include", "cldrd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "cldrd_distill_term" in set(re.findall(r"\b(cldrd_[a-z0-9_]+)\s*\(", text))
    res, argtypes = _lib.SIGNATURES["cldrd_distill_term"]
    assert res is _lib.ci and len(argtypes) == 12
    m = re.search(r"int\s+cldrd_distill_term\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 12
    assert hip_ops.DISTILL_KINDS == {"kl_div": 0, "margin_mse": 1}
    assert "distill_term" in torch_ops.OPS and hasattr(torch.ops.cldrd, "distill_term")
    from cldrd_amd.losses import DistillLoss
    with pytest.raises(ValueError):
        DistillLoss(kd="ranknet")
    with pytest.raises(ValueError):
        DistillLoss(rank="kl_div")
    with pytest.raises(RuntimeError, match="GPU"):
        DistillLoss()(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4))
