"""Topic-aware batches end to end on the committed dataset fixture (12 queries) with the tiny model of selftest: query_clusters writes its
three files and its assignments are the nearest centroids of the embeddings; training under --tas_clusters runs the predicted pure
batches; an exact resume under the flag continues bit for bit and is refused under another cluster file."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest
import selftest
from cldrd_amd.dataset import query_clusters as Q
from cldrd_amd.trainer import nway_listwise as T
from test_gpu_kmeans import _check_assign

FIX = os.path.join(conftest.GOLDEN, "nway_dataset_fixture")
QUERIES, COLLECTION, TRAIN = (os.path.join(FIX, n) for n in ("queries.tsv", "collection.tsv", "train_10relT_20neg.jsonl"))
K = 3


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from toy_tokenizer import make_tokenizer
    d = tmp_path_factory.mktemp("tas")
    tok_dir, mdir = str(d / "tok"), str(d / "student")
    make_tokenizer().save_pretrained(tok_dir)
    student = selftest.build_tiny_model(selftest.tiny_config(), std=0.05)
    student.query_encoder.save_pretrained(mdir)
    ckpt0 = str(d / "checkpoint_0.pth.tar")
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt0)
    out = str(d / "clusters" / "queries.clusters.tsv")
    model_flags = ["--resume", ckpt0, "--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir]
    meta = Q.main(Q.get_args(model_flags + ["--queries_path", QUERIES, "--training_path", TRAIN, "--n_clusters", str(K), "--output_path", out,
                                            "--iters", "5", "--seed", "1", "--max_length", "8", "--fp32_encode"]))
    return {"dir": d, "tok": tok_dir, "mdir": mdir, "ckpt0": ckpt0, "out": out, "meta": meta, "model_flags": model_flags}


def _lines(path):
    return [tuple(int(v) for v in ln.split("\t")) for ln in open(path).read().splitlines()]


def test_query_clusters_writes_its_three_files(stage):
    lines = _lines(stage["out"])
    file_qids = [int(ln.split("\t")[0]) for ln in open(QUERIES) if len(ln.strip().split("\t")) >= 2]
    assert len(lines) == 12 and [q for q, _ in lines] == file_qids and all(0 <= c < K for _, c in lines)
    cent = np.load(stage["out"] + ".centroids.npy")
    meta = json.load(open(stage["out"] + ".meta.json"))
    assert cent.shape == (K, 128) and cent.dtype == np.float32 and meta == stage["meta"]
    assert {k: meta[k] for k in ("k", "iters", "seed", "n", "d")} == {"k": K, "iters": 5, "seed": 1, "n": 12, "d": 128}
    assert len(meta["moved"]) == 5 and meta["moved"][0] == 12 and 0 <= meta["n_empty"] < K
    sizes = np.bincount([c for _, c in lines], minlength=K)
    assert (meta["size_min"], meta["size_max"]) == (int(sizes.min()), int(sizes.max())) and meta["size_min"] <= meta["size_median"] <= meta["size_max"]
    with pytest.raises(ValueError, match="--n_clusters 13 is larger than the number of queries"):          # before any model is built
        Q.main(Q.get_args(["--model_name_or_path", "/nonexistent/model", "--tokenizer_name_or_path", stage["tok"], "--queries_path", QUERIES,
                           "--n_clusters", "13", "--output_path", str(stage["dir"] / "never.tsv")]))
    assert not os.path.exists(str(stage["dir"] / "never.tsv"))


def test_assignments_are_the_nearest_centroids_of_the_embeddings(stage):
    from transformers import AutoTokenizer
    from cldrd_amd.dataset import SequenceDataset
    from cldrd_amd.models.nway_dual_encoder import NwayDualEncoder
    from cldrd_amd.retriever.index_text import load_checkpoint_into
    from cldrd_amd.retriever.retrieval_utils import get_embeddings_from_scratch
    model = NwayDualEncoder(stage["mdir"], share_weights=False)
    load_checkpoint_into(model, stage["ckpt0"], True)
    model.cuda()
    ds = SequenceDataset.create_from_seqs_file(QUERIES, AutoTokenizer.from_pretrained(stage["tok"]), 8, is_query=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=512, shuffle=False, num_workers=0, collate_fn=ds.collate_fn)
    embs, ids = get_embeddings_from_scratch(model, loader, use_fp16=False, is_query=True)
    lines = _lines(stage["out"])
    assert list(ids) == [q for q, _ in lines]
    cent = torch.from_numpy(np.load(stage["out"] + ".centroids.npy"))
    _check_assign(torch.from_numpy(np.asarray(embs, dtype=np.float32)), cent, torch.tensor([c for _, c in lines]))


def _common(stage):
    return ["--experiment_folder", str(stage["dir"]), "--queries_path", QUERIES, "--collection_path", COLLECTION, "--training_path", TRAIN,
            "--label_mode", "9", "--model_name_or_path", stage["mdir"], "--tokenizer_name_or_path", stage["tok"], "--query_max_len", "8",
            "--passage_max_len", "24", "--train_batch_size", "4", "--logging_steps", "3", "--evaluate_steps", "3", "--warmup_steps", "1",
            "--num_train_epochs", "2", "--learning_rate", "1e-3", "--loader_workers", "0", "--loss", "softmax_ce", "--in_batch_loss",
            "--deterministic"]


def _train(argv):
    """train() in process -> (trainer, the qids of every batch a step saw)"""
    seen = []
    real = T.NwayTrainer.train_step

    def recorded(self, batch):
        q = batch["qid"]
        seen.append(np.asarray(q.cpu() if isinstance(q, torch.Tensor) else q).tolist())
        return real(self, batch)
    T.NwayTrainer.train_step = recorded
    try:
        return T.train(T.set_env(T.get_args(argv))), seen
    finally:
        T.NwayTrainer.train_step = real


def _ckpt(stage, run, step):
    return torch.load(os.path.join(str(stage["dir"]), run, "models", f"checkpoint_{step}.pth.tar"), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def run_a(stage):
    """the uninterrupted run: two epochs of three batches under --tas_clusters, checkpoints after steps 3 and 6"""
    tr, seen = _train(_common(stage) + ["--run_folder", "tas_a", "--tas_clusters", stage["out"]])
    torch.cuda.synchronize()
    return {"global_step": tr.global_step, "finite": bool(torch.isfinite(tr.flat_p).all()), "seen": seen,
            "state": [t.detach().cpu().clone() for t in (tr.flat_p, tr.m, tr.v)]}


def test_training_runs_the_predicted_pure_batches(stage, run_a):
    assert run_a["global_step"] == 6 and run_a["finite"]
    cof = dict(_lines(stage["out"]))
    sizes = np.bincount(list(cof.values()), minlength=K)
    pure_per_epoch = int((sizes // 4).sum())
    seen = run_a["seen"]
    assert len(seen) == 6 and all(len(b) == 4 for b in seen)
    for epoch in (seen[:3], seen[3:]):
        assert sorted(q for b in epoch for q in b) == sorted(cof)          # every example once per epoch
        assert sum(len({cof[q] for q in b}) == 1 for b in epoch) == pure_per_epoch
    rs = _ckpt(stage, "tas_a", 3)["resume_state"]
    assert rs["tas_clusters"] == stage["out"] and rs["tas_clusters_digest"] == T.read_query_clusters(stage["out"])[1]
    assert (rs["epoch"], rs["step_in_epoch"]) == (0, 3)


def test_exact_resume_under_the_flag_and_its_refusals(stage, run_a):
    ckpt3 = os.path.join(str(stage["dir"]), "tas_a", "models", "checkpoint_3.pth.tar")
    resume = ["--resume", ckpt3, "--resume_exact"]
    tr, seen = _train(_common(stage) + ["--run_folder", "tas_b", "--tas_clusters", stage["out"]] + resume)
    torch.cuda.synchronize()
    assert tr.global_step == 6 and seen == run_a["seen"][3:]
    for got, want in zip((tr.flat_p, tr.m, tr.v), run_a["state"]):
        assert torch.equal(got.detach().cpu().view(torch.int32), want.view(torch.int32))
    a6, b6 = _ckpt(stage, "tas_a", 6), _ckpt(stage, "tas_b", 6)
    assert list(a6["resume_state"]) == list(b6["resume_state"])
    for k, v in a6["state_dict"].items():
        assert torch.equal(v, b6["state_dict"][k]), k
    # another cluster file, the flag dropped, the flag added: refused by field name before the first step
    other = str(stage["dir"] / "other.clusters.tsv")
    open(other, "w").write("".join(f"{q}\t{(c + 1) % K}\n" for q, c in _lines(stage["out"])))
    with pytest.raises(ValueError, match="--resume_exact: tas_clusters"):
        _train(_common(stage) + ["--run_folder", "tas_refused", "--tas_clusters", other] + resume)
    with pytest.raises(ValueError, match="--resume_exact: tas_clusters"):
        _train(_common(stage) + ["--run_folder", "tas_refused"] + resume)
    assert not os.path.exists(os.path.join(str(stage["dir"]), "tas_refused", "models", "checkpoint_6.pth.tar"))
    # a run without the flag writes exactly the keys it wrote before the flag existed
    plain_argv = _common(stage) + ["--run_folder", "plain"]
    plain_argv[plain_argv.index("--num_train_epochs") + 1] = "1"
    _train(plain_argv)
    plain = _ckpt(stage, "plain", 3)["resume_state"]
    assert set(a6["resume_state"]) - set(plain) == set(T.TAS_POSITION_FIELDS) and not set(plain) - set(a6["resume_state"])
    with pytest.raises(ValueError, match="--resume_exact: tas_clusters"):
        _train(plain_argv + ["--tas_clusters", stage["out"], "--resume", os.path.join(str(stage["dir"]), "plain", "models", "checkpoint_3.pth.tar"),
                             "--resume_exact"])
