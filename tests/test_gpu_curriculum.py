"""One CL-DRD iteration end to end on tiny models, with this package's command lines only: index a toy collection with a student
checkpoint, retrieve the top 60 of the training queries, re-score them with a cross-encoder teacher, cut a mode-9 curriculum file from the
teacher's run, and train the student on it."""
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
import selftest
from test_rerank_host import make_pair_tokenizer, words

pytestmark = pytest.mark.gpu

N_P, N_Q, TOP = 300, 16, 60


def _teacher(tmp_path, vocab):
    from transformers import BertConfig, BertForSequenceClassification
    torch.manual_seed(17)
    cfg = BertConfig(vocab_size=vocab, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                     max_position_embeddings=512, num_labels=1, initializer_range=0.05)
    m = BertForSequenceClassification(cfg).eval()
    with torch.no_grad():       # spread the random logits (see tests/test_gpu_rerank.py: _hf_model)
        m.classifier.weight.mul_(10.0)
    path = str(tmp_path / "teacher")
    m.save_pretrained(path)
    return path


def test_one_curriculum_iteration_end_to_end(tmp_path):
    from cldrd_amd.dataset import curriculum_file as C
    from cldrd_amd.retriever import index_text, rerank_top_passages, retrieve_top_passages
    from cldrd_amd.trainer import nway_listwise as T
    rng = np.random.default_rng(23)
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    c_path, q_path = tmp_path / "collection.tsv", tmp_path / "queries.train.tsv"
    c_path.write_text("".join(f"{9000 + j}\t{words(int(rng.integers(3, 24)), 5 * j)}\n" for j in range(N_P)))
    qids = [int(q) for q in rng.choice(100000, N_Q, replace=False)]
    q_path.write_text("".join(f"{q}\t{words(int(rng.integers(2, 7)), 3 * i)}\n" for i, q in enumerate(qids)))

    # 0. a student checkpoint in the trainer's layout
    cfg = selftest.tiny_config()
    student = selftest.build_tiny_model(cfg)
    mdir = tmp_path / "student"
    student.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp_path / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt)
    common = ["--resume", str(ckpt), "--model_name_or_path", str(mdir), "--tokenizer_name_or_path", tok_dir]

    # 1. index, 2. retrieve the top 60 of every training query
    index_path = index_text.main(index_text.get_args(common + ["--passages_path", str(c_path), "--index_dir", str(tmp_path / "index"),
                                                               "--max_length", "32"]))
    run_path = tmp_path / "runs" / "train.top60.run"
    retrieve_top_passages.main(retrieve_top_passages.get_args(common + ["--queries_path", str(q_path), "--index_path", index_path,
                                                                        "--max_length", "16", "--top_k", str(TOP),
                                                                        "--output_path", str(run_path)]))
    assert len(run_path.read_text().splitlines()) == N_Q * TOP

    # 3. teacher re-scoring
    teacher_run = tmp_path / "runs" / "train.top60.teacher.run"
    rerank_top_passages.main(rerank_top_passages.get_args([
        "--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path),
        "--model_name_or_path", _teacher(tmp_path, tok.vocab_size + 4), "--tokenizer_name_or_path", tok_dir, "--max_len", "64",
        "--output_path", str(teacher_run)]))
    scores = {}
    for line in teacher_run.read_text().splitlines():
        q, p, _, s = line.split("\t")
        scores.setdefault(int(q), {})[int(p)] = float(s)
    assert sorted(scores) == sorted(qids) and all(len(v) == TOP for v in scores.values())

    # 4. the mode-9 curriculum file
    train_path = tmp_path / "train.10relT_20neg.json"
    n, skipped = C.main(C.get_args(["--run_path", str(teacher_run), "--label_mode", "9", "--output_path", str(train_path),
                                    "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "5"]))
    assert (n, skipped) == (N_Q, 0)
    examples = [json.loads(line) for line in train_path.read_text().splitlines()]
    assert sorted(ex["qid"] for ex in examples) == sorted(qids) and len(examples) == N_Q
    for ex in examples:
        sc = scores[ex["qid"]]
        by_score = sorted(sc.values(), reverse=True)
        assert [sc[p] for p in ex["relT_pids"]] == by_score[:10]
        assert all(by_score[29] <= sc[p] <= by_score[10] for p in ex["most_hard_pids"])
        assert all(by_score[59] <= sc[p] <= by_score[30] for p in ex["semi_hard_pids"])
        every = ex["relT_pids"] + ex["most_hard_pids"] + ex["semi_hard_pids"]
        assert len(every) == 30 and len(set(every)) == 30

    # 5. two epochs of the trainer command line on it, from the student checkpoint
    args = T.set_env(T.get_args([
        "--experiment_folder", str(tmp_path), "--run_folder", "stage2", "--queries_path", str(q_path), "--collection_path", str(c_path),
        "--training_path", str(train_path), "--label_mode", "9", "--model_name_or_path", str(mdir), "--model_checkpoint", str(ckpt),
        "--tokenizer_name_or_path", tok_dir, "--query_max_len", "16", "--passage_max_len", "32", "--train_batch_size", "4",
        "--logging_steps", "1", "--evaluate_steps", "4", "--warmup_steps", "1", "--num_train_epochs", "2", "--learning_rate", "1e-3",
        "--loader_workers", "2"]))
    tr = T.train(args)
    assert tr.global_step == 2 * N_Q // 4 and tr.skipped_steps() == 0
    assert torch.isfinite(tr.flat_p).all().item()
    log = (tmp_path / "stage2" / "log" / "train_logs.log").read_text().splitlines()
    losses = [float(line.split("\t")[2]) for line in log[1:]]
    assert len(losses) == tr.global_step - 1 and all(np.isfinite(losses))           # the first logging call only writes the header
    assert os.path.exists(tmp_path / "stage2" / "models" / f"checkpoint_{tr.global_step}.pth.tar")
