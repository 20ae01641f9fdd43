"""``retriever.build_stage_file`` against the three programs it replaces, on tiny models and the fixture shape of
tests/test_gpu_curriculum.py (300 passages, 16 queries, top 60, windows 11:30 and 31:60): the student run, the teacher run and the training
file of the one job are byte for byte the files of ``retrieve_top_passages`` -> ``rerank_top_passages`` -> ``curriculum_file``."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
import selftest
from test_gpu_curriculum import N_P, N_Q, TOP, _teacher
from test_rerank_host import make_pair_tokenizer, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """collection, queries, a student checkpoint with its index, a teacher - and the run files of the first two of the three programs"""
    from cldrd_amd.retriever import index_text, rerank_top_passages, retrieve_top_passages
    tmp = tmp_path_factory.mktemp("stage")
    rng = np.random.default_rng(23)
    tok = make_pair_tokenizer()
    tok_dir = str(tmp / "tok")
    tok.save_pretrained(tok_dir)
    c_path, q_path = tmp / "collection.tsv", tmp / "queries.train.tsv"
    c_path.write_text("".join(f"{9000 + j}\t{words(int(rng.integers(3, 24)), 5 * j)}\n" for j in range(N_P)))
    qids = [int(q) for q in rng.choice(100000, N_Q, replace=False)]
    q_path.write_text("".join(f"{q}\t{words(int(rng.integers(2, 7)), 3 * i)}\n" for i, q in enumerate(qids)))
    student = selftest.build_tiny_model(selftest.tiny_config())
    mdir = tmp / "student"
    student.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt)
    common = ["--resume", str(ckpt), "--model_name_or_path", str(mdir), "--tokenizer_name_or_path", tok_dir]
    index_path = index_text.main(index_text.get_args(common + ["--passages_path", str(c_path), "--index_dir", str(tmp / "index"),
                                                               "--max_length", "32"]))
    run_path = tmp / "runs" / "train.top60.run"
    retrieve_top_passages.main(retrieve_top_passages.get_args(common + ["--queries_path", str(q_path), "--index_path", index_path,
                                                                        "--max_length", "16", "--top_k", str(TOP),
                                                                        "--output_path", str(run_path)]))
    teacher = _teacher(tmp, tok.vocab_size + 4)
    teacher_run = tmp / "runs" / "train.top60.teacher.run"
    rerank_top_passages.main(rerank_top_passages.get_args([
        "--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path), "--model_name_or_path", teacher,
        "--tokenizer_name_or_path", tok_dir, "--max_len", "64", "--output_path", str(teacher_run)]))
    assert len(teacher_run.read_text().splitlines()) == N_Q * TOP
    job = common + ["--index_path", index_path, "--queries_path", str(q_path), "--collection_path", str(c_path), "--query_max_len", "16",
                    "--top_k", str(TOP), "--teacher_name_or_path", teacher, "--teacher_tokenizer_name_or_path", tok_dir,
                    "--teacher_max_len", "64"]
    return dict(tmp=tmp, tok=tok, q_path=q_path, c_path=c_path, run=run_path, teacher_run=teacher_run, job=job, index_path=index_path)


@pytest.mark.parametrize("mode,with_scores", [("9", True), ("9", False), ("8", False)])
def test_one_job_writes_the_files_of_the_three_programs(stage, mode, with_scores):
    from cldrd_amd.dataset import curriculum_file as C
    from cldrd_amd.dataset.nway_dataset import NwayDataset
    from cldrd_amd.retriever import build_stage_file as B
    tmp = stage["tmp"]
    tag = f"mode{mode}{'s' if with_scores else ''}"
    cut = ["--label_mode", mode, "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "5"] + (["--with_scores"] if with_scores else [])
    want = tmp / f"three.{tag}.json"
    assert C.main(C.get_args(["--run_path", str(stage["teacher_run"]), "--output_path", str(want)] + cut)) == (N_Q, 0)
    got, s_run, t_run = tmp / f"job.{tag}.json", tmp / f"job.{tag}.train.student.run", tmp / f"job.{tag}.train.teacher.run"
    assert B.main(B.get_args(stage["job"] + cut + ["--output_path", str(got), "--student_run_path", str(s_run),
                                                   "--teacher_run_path", str(t_run)])) == (N_Q, 0)
    assert s_run.read_bytes() == stage["run"].read_bytes()
    assert t_run.read_bytes() == stage["teacher_run"].read_bytes()
    assert got.read_bytes() == want.read_bytes() and len(got.read_text().splitlines()) == N_Q
    assert set(B.main.last_timings) >= {"encode_queries_s", "search_s", "teacher_score_s", "select_s", "training_file_s"}
    if with_scores:
        ds = NwayDataset.create_from_relT_most_semi_hard_file(str(stage["q_path"]), str(stage["c_path"]), str(got), stage["tok"], 16, 32, mode,
                                                              teacher_scores=True)
        assert len(ds) == N_Q
        batch = ds.collate_fn([ds[0], ds[N_Q - 1]])
        assert tuple(batch["teacher_scores"].shape) == (2, 30) and torch.isfinite(batch["teacher_scores"]).all().item()


def test_the_job_refuses_what_the_three_programs_fail_on_later(stage):
    from cldrd_amd.retriever import build_stage_file as B
    tmp = stage["tmp"]
    cut = ["--label_mode", "9", "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--output_path", str(tmp / "never.json")]
    job = list(stage["job"])
    job[job.index("--top_k") + 1] = str(N_P + 1)
    with pytest.raises(ValueError, match="fewer than --top_k"):
        B.main(B.get_args(job + cut))
    assert not (tmp / "never.json").exists()
