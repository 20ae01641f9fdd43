"""Validation on a dev run while training, on the GPU: the student score against the flat search, the dataloader path against the pool path,
NwayTrainer.validate between replayed steps, the command lines end to end, and the cross-encoder through the dataloader path.
Tiny towers (d = 128, 2 heads, 2 layers, vocabulary 512, 64 positions, std-0.05 init) on tiny files."""
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
import selftest
from cldrd_amd import synthetic as syn
from cldrd_amd.evaluation import DevPool, RerankingEvaluator
from cldrd_amd.evaluation import dev_pool as DP
from test_rerank_host import make_pair_tokenizer, words

pytestmark = pytest.mark.gpu

N_P, Q_LEN, P_LEN = 120, 16, 48
# dev query -> candidates in run order: 1 to 9 candidates, passage 9007 shared by three queries
DEV = {501: [9007], 502: [9011, 9007, 9040, 9003], 503: [9090, 9007, 9001, 9002, 9005, 9006, 9008, 9009, 9010],
       504: [9100, 9000], 505: [9055, 9056, 9057, 9058, 9059, 9060], 506: [9070, 9071, 9072]}
QRELS = {501: [9007], 502: [9040], 503: [9005, 9010], 504: [9119], 506: [9071]}           # 504: no relevant candidate; 505: no qrels


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """collection / dev queries / dev run / qrels + the tokenizer directory, written once for the module"""
    d = tmp_path_factory.mktemp("dev")
    rng = np.random.default_rng(77)
    tok = make_pair_tokenizer()
    tok.save_pretrained(str(d / "tok"))
    plens = rng.integers(3, 39, N_P)                     # 5 to 40 tokens with [CLS] / [SEP]
    plens[:4] = [3, 38, 38, 20]
    (d / "collection.tsv").write_text("".join(f"{9000 + j}\t{words(int(plens[j]), 5 * j)}\n" for j in range(N_P)))
    (d / "queries.dev.tsv").write_text("".join(f"{q}\t{words(1 + i, 7 * i)}\n" for i, q in enumerate(DEV)))
    lines = [f"{q}\t{p}\t{r + 1}\t{10.0 - r}\n" for q, ps in DEV.items() for r, p in enumerate(ps)]
    lines.insert(4, lines[1])                            # a duplicated run line: scored once
    (d / "dev.run.tsv").write_text("".join(lines))
    (d / "qrels.dev.tsv").write_text("".join(f"{q}\t0\t{p}\t1\n" for q, ps in QRELS.items() for p in ps))
    paths = dict(dir=d, tok_dir=str(d / "tok"), collection=str(d / "collection.tsv"), queries=str(d / "queries.dev.tsv"),
                 run=str(d / "dev.run.tsv"), qrels=str(d / "qrels.dev.tsv"))
    paths["pool"] = DevPool(paths["run"], paths["queries"], paths["collection"], tok, Q_LEN, P_LEN)
    return paths


def _student(seed=3):
    return selftest.build_tiny_model(selftest.tiny_config(), seed=seed, std=0.05).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- (a) the student score IS the flat search's score
def test_pool_scores_equal_the_flat_search_bit_for_bit(tmp_path, monkeypatch):
    from cldrd_amd.retriever.retrieval_utils import FlatIPIndex
    nq, n_p, d = 5, 37, 128
    (tmp_path / "q.tsv").write_text("".join(f"{i}\tw{i}\n" for i in range(nq)))
    (tmp_path / "c.tsv").write_text("".join(f"{100 + j}\tw{j}\n" for j in range(n_p)))
    rng = np.random.default_rng(3)
    (tmp_path / "run.tsv").write_text("".join(f"{i}\t{100 + j}\n" for i in range(nq) for j in rng.permutation(n_p)))
    pool = DevPool(str(tmp_path / "run.tsv"), str(tmp_path / "q.tsv"), str(tmp_path / "c.tsv"), make_pair_tokenizer(), 8, 8)
    assert pool.n_pairs == nq * n_p and pool.cand_rows.shape == (nq, n_p)
    g = torch.Generator().manual_seed(9)
    common = torch.randn(1, d, generator=g) * 2.0            # CLS-like: a large common component
    q = (common + torch.randn(nq, d, generator=g)).contiguous()
    p = (common + torch.randn(n_p, d, generator=g)).contiguous()
    got = pool.score_embeddings(q.cuda(), p.cuda())
    monkeypatch.setattr(DP, "RESCORE_CHUNK", 2)              # three launches instead of one
    assert np.array_equal(_bits(pool.score_embeddings(q.cuda(), p.cuda())), _bits(got))
    index = FlatIPIndex(d)
    index.add_with_ids(p.numpy(), pool.passage_ids)
    D, I = index.to_gpu(0).search(q.numpy(), n_p)
    by_pid = [dict(zip(I[i].tolist(), D[i])) for i in range(nq)]
    want = np.array([by_pid[gq][pid] for gq, pid in zip(pool.group.tolist(), pool.pids.tolist())], dtype=np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    exact = (q.numpy().astype(np.float64)[pool.group] * p.numpy().astype(np.float64)[pool.p_pos]).sum(1)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - exact) <= ulp).all()


# ---------------------------------------------------------------- (b) dataloader path == pool path
def test_dataloader_path_equals_pool_path(files):
    from cldrd_amd.dataset import RerankingDataset
    tok = make_pair_tokenizer()
    pool = files["pool"]
    assert sorted(np.diff(pool.starts).tolist()) == [1, 2, 3, 4, 6, 9] and pool.n_passages == pool.n_pairs - 2
    assert pool.p_lens.min() == 5 and pool.p_lens.max() == 40
    model = _student().train()
    seeds = [t.step_seed for t in model.towers()]
    ev = RerankingEvaluator(files["qrels"])
    ds = RerankingDataset(files["run"], files["queries"], files["collection"], tok, False, query_max_len=Q_LEN, passage_max_len=P_LEN)
    assert len(ds) == pool.n_pairs + 1                                       # the duplicated line is still in the dataset
    loader = torch.utils.data.DataLoader(ds, batch_size=7, shuffle=False, collate_fn=ds.collate_fn)
    model.eval_fp32 = True                                                   # the batch-invariant pass
    m_loader = ev.compute_metrics(model, loader)
    s_loader = ev.last_scores.copy()
    m_pool = ev.compute_metrics_pool(model, pool)
    s_pool = ev.last_scores.copy()
    assert s_pool.shape == (pool.n_pairs,) and np.isfinite(s_pool).all() and np.unique(s_pool).shape[0] > pool.n_pairs // 2
    assert np.array_equal(_bits(s_loader), _bits(s_pool))
    assert list(m_loader) == list(m_pool) and all(float(m_loader[k]) == float(m_pool[k]) for k in m_pool)
    assert m_pool["QueriesRanked"] == 5 and m_pool["QueriesWithNoRelevant@10"] == 2 and m_pool["QueriesWithRelevant@10"] == 4
    ev.compute_metrics_pool(model, pool, batch_size=5)
    assert np.array_equal(_bits(ev.last_scores), _bits(s_pool))             # fp32 pass: not a function of the batch size either
    model.eval_fp32 = False                                                  # the 16-bit pass: the same call twice
    ev.compute_metrics_pool(model, pool)
    s1 = ev.last_scores.copy()
    ev.compute_metrics_pool(model, pool)
    assert np.array_equal(_bits(s1), _bits(ev.last_scores))
    assert np.abs(s1 - s_pool).max() <= 2e-2 * np.abs(s_pool).max()          # and it is the same model (the small-model 16-bit bar)
    # the state the evaluator found
    assert model.training and all(m.training for m in model.modules()) and [t.step_seed for t in model.towers()] == seeds


# ---------------------------------------------------------------- (c) training is untouched
def test_validate_leaves_training_untouched(files, monkeypatch):
    from cldrd_amd.models import NwayDualEncoder
    from cldrd_amd.trainer.nway_listwise import NwayTrainer
    cfg = selftest.tiny_config()
    cfg.dropout, cfg.attention_dropout = 0.1, 0.1
    monkeypatch.setenv("CLDRD_GRAPH", "1")
    model = NwayDualEncoder(cfg, share_weights=False).cuda().train()
    with torch.no_grad():
        for seed, tower in ((11, model.query_encoder), (12, model.passage_encoder)):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed, name, tuple(p.shape), std=0.05, perturb=True))
    tr = NwayTrainer(model, loss="kl_div", learning_rate=3e-3, warmup_steps=5, total_steps=40)
    towers = model.towers()
    emb = torch.zeros(tr.flat_p.numel(), dtype=torch.bool, device="cuda")
    for t, toff in zip(towers, model._tower_offsets):
        for n in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight"):
            off, shape = t.layout.entries[n]
            emb[toff + off:toff + off + shape[0] * shape[1]] = True
    pool, ev = files["pool"], RerankingEvaluator(files["qrels"])

    def snapshot():
        return (tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.global_step, tr.adam_step, [t.step_seed for t in towers])

    def restore(sn):
        tr.flat_p.copy_(sn[0]); tr.m.copy_(sn[1]); tr.v.copy_(sn[2])
        tr.global_step, tr.adam_step = sn[3], sn[4]
        for t, ss in zip(towers, sn[5]):
            t.step_seed = ss
            t.refresh_shadows(need_transposed=True)

    def dev(batch):
        return {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}

    def state():
        scale = None if tr._scale_state is None else tr._scale_state.clone()
        return ([tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.flat_g.clone()] + ([scale] if scale is not None else []),
                (tr.global_step, tr.adam_step, [t.step_seed for t in towers], model.training, [m.training for m in model.modules()]))

    shape = (3, 4, 8, 16)
    for i in range(5):                                    # three eager steps, the capture, one replay
        tr.train_step(dev(syn.nway_batch(100 + i, *shape, vocab=cfg.vocab_size, ragged=True, label_kind="teacher")))
    batch = dev(syn.nway_batch(200, *shape, vocab=cfg.vocab_size, ragged=True, label_kind="teacher"))
    key = tr._batch_key(batch)
    assert tr._graphs[key]["graph"] is not None
    graphs = {k: id(e["graph"]) for k, e in tr._graphs.items()}
    replays, real_replay = [], torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real_replay(self))[1])
    monkeypatch.setattr(tr, "_capture", lambda b: pytest.fail("validate() made the trainer capture again"))
    sn = snapshot()
    # validate, then the step
    tensors0, host0 = state()
    metrics = tr.validate(pool, ev)
    tensors1, host1 = state()
    assert host0 == host1 and all(torch.equal(a, b) for a, b in zip(tensors0, tensors1))
    assert list(metrics)[0] == "MRR@10" and metrics["QueriesRanked"] == 5 and not replays
    l1 = tr.train_step(batch).clone()
    lg1, g1, p1 = tr.last_logits.clone(), tr.flat_g.clone(), tr.flat_p.clone()
    assert replays == [graphs[key]] and {k: id(e["graph"]) for k, e in tr._graphs.items()} == graphs
    # the step alone, from the same snapshot
    restore(sn)
    l0 = tr.train_step(batch).clone()
    torch.cuda.synchronize()
    assert len(replays) == 2
    assert torch.equal(l1, l0) and torch.equal(lg1, tr.last_logits)
    assert torch.equal(g1[~emb], tr.flat_g[~emb])
    ge = (g1[emb] - tr.flat_g[emb]).abs().max().item()                       # float atomics in the embedding tables
    assert ge <= 1e-5 * max(1.0, g1[emb].abs().max().item())
    assert (p1 - tr.flat_p).abs().max().item() <= 1e-6
    # a second validation sees the weights of the step in between (the shadows were marked stale by the replay)
    m2 = tr.validate(pool, ev)
    s2 = ev.last_scores.copy()
    for t in towers:
        t.refresh_shadows(need_transposed=True)
    tr.validate(pool, ev)
    assert np.array_equal(_bits(s2), _bits(ev.last_scores)) and list(m2) == list(metrics)


# ---------------------------------------------------------------- (d) the command lines end to end
def _row(line, header):
    cols = line.split("\t")
    return {k: (float(v) if "." in v or "e" in v or "n" in v else int(v)) for k, v in zip(header, cols)}


def _run_metrics(path, ev):
    ranking = {}
    for line in open(path).read().splitlines():
        q, p = line.split("\t")[:2]
        ranking.setdefault(int(q), []).append(int(p))
    return ev.direct_compute_metric(ranking)


def test_command_lines_end_to_end(files, tmp_path):
    from cldrd_amd.evaluation import continue_rerank_evaluator as C
    from cldrd_amd.retriever import rerank_top_passages as R
    from cldrd_amd.trainer import nway_listwise as T
    rng = np.random.default_rng(5)
    n_q = 16
    q_path, train_path = tmp_path / "queries.train.tsv", tmp_path / "train.10relT_20neg.json"
    q_path.write_text("".join(f"{3000 + i}\t{words(int(rng.integers(2, 7)), 3 * i)}\n" for i in range(n_q)))
    with open(train_path, "w") as fh:
        for i in range(n_q):
            pids = (9000 + rng.choice(N_P, 30, replace=False)).tolist()
            fh.write(json.dumps({"qid": 3000 + i, "relT_pids": pids[:10], "most_hard_pids": pids[10:20], "semi_hard_pids": pids[20:]}) + "\n")
    student = selftest.build_tiny_model(selftest.tiny_config(), std=0.05)
    mdir = tmp_path / "student"
    student.query_encoder.save_pretrained(str(mdir))
    ckpt0 = tmp_path / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt0)
    common = ["--experiment_folder", str(tmp_path), "--queries_path", str(q_path), "--collection_path", files["collection"],
              "--training_path", str(train_path), "--label_mode", "9", "--model_name_or_path", str(mdir), "--model_checkpoint", str(ckpt0),
              "--tokenizer_name_or_path", files["tok_dir"], "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN),
              "--train_batch_size", "4", "--logging_steps", "4", "--evaluate_steps", "4", "--warmup_steps", "1", "--num_train_epochs", "2",
              "--learning_rate", "1e-3", "--loader_workers", "0"]
    dev_flags = ["--dev_path", files["run"], "--dev_queries_path", files["queries"], "--dev_qrels_path", files["qrels"]]
    tr = T.train(T.set_env(T.get_args(common + ["--run_folder", "with_dev"] + dev_flags)))
    assert tr.global_step == 8 and tr.model.training
    run_dir = tmp_path / "with_dev"
    log = (run_dir / "log" / "dev_logs.log").read_text().splitlines()
    header = log[0].split("\t")
    ev = RerankingEvaluator(files["qrels"])
    assert header == ["epoch", "step"] + list(_run_metrics(files["run"], ev)) + ["seconds"] and header[2] == "MRR@10"
    rows = [_row(line, header) for line in log[1:]]
    assert [(r["epoch"], r["step"]) for r in rows] == [(1, 4), (2, 8)]
    best = json.loads((run_dir / "dev_best.json").read_text())
    assert sorted(best) == ["checkpoint", "epoch", "metric", "step", "value"] and best["metric"] == "MRR@10"
    assert os.path.exists(best["checkpoint"]) and best["checkpoint"].endswith(f"checkpoint_{best['step']}.pth.tar")
    want = max(rows, key=lambda r: (r["MRR@10"], -r["step"]))
    assert (best["step"], best["value"], best["epoch"]) == (want["step"], want["MRR@10"], want["epoch"])
    metric_keys = header[2:-1]
    # the student mode of rerank_top_passages on checkpoint_4: the run whose metrics are the step-4 row
    out = tmp_path / "dev.rerank.step4.tsv"
    R.main(R.get_args(["--dual_encoder", "--resume", str(run_dir / "models" / "checkpoint_4.pth.tar"), "--model_name_or_path", str(mdir),
                       "--tokenizer_name_or_path", files["tok_dir"], "--run_path", files["run"], "--queries_path", files["queries"],
                       "--collection_path", files["collection"], "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN),
                       "--output_path", str(out)]))
    lines = [ln.split("\t") for ln in out.read_text().splitlines()]
    assert len(lines) == files["pool"].n_pairs and list(dict.fromkeys(int(c[0]) for c in lines)) == list(DEV)
    for q, ps in DEV.items():
        mine = [c for c in lines if int(c[0]) == q]
        assert sorted(int(c[1]) for c in mine) == sorted(ps) and [int(c[2]) for c in mine] == list(range(1, len(ps) + 1))
        assert all(float(a[3]) >= float(b[3]) for a, b in zip(mine, mine[1:]))
    m4 = _run_metrics(out, ev)
    assert {k: float(m4[k]) for k in metric_keys} == {k: float(rows[0][k]) for k in metric_keys}
    # every checkpoint of the folder after the fact: the same table
    table = tmp_path / "continue.log"
    best2 = C.main(C.get_args(["--resume_folder", str(run_dir / "models"), "--dev_path", files["run"], "--dev_queries_path", files["queries"],
                               "--dev_qrels_path", files["qrels"], "--collection_path", files["collection"], "--model_name_or_path", str(mdir),
                               "--tokenizer_name_or_path", files["tok_dir"], "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN),
                               "--output_path", str(table)]))
    log2 = table.read_text().splitlines()
    assert log2[0] == log[0] and [ln.split("\t")[:-1] for ln in log2[1:]] == [ln.split("\t")[:-1] for ln in log[1:]]
    assert (best2["step"], best2["value"]) == (best["step"], best["value"])
    # without the dev flags: neither file
    T.train(T.set_env(T.get_args(common + ["--run_folder", "without_dev"])))
    plain = tmp_path / "without_dev"
    assert os.path.exists(plain / "models" / "checkpoint_8.pth.tar")
    assert not os.path.exists(plain / "log" / "dev_logs.log") and not os.path.exists(plain / "dev_best.json")
    assert sorted(os.listdir(plain)) == ["log", "models"] and sorted(os.listdir(plain / "log")) == ["train_logs.log"]


# ---------------------------------------------------------------- (e) a cross-encoder through the dataloader path
def test_cross_encoder_through_the_dataloader_path(files, tmp_path):
    from cldrd_amd.dataset import RerankingDataset
    from cldrd_amd.models.cross_encoder import CrossEncoder
    from cldrd_amd.retriever import rerank_top_passages as R
    from test_gpu_rerank import _hf_model, _save
    tok = make_pair_tokenizer()
    hf = _hf_model("bert", 128, 2, 1, seed=12, vocab=tok.vocab_size + 4)
    model_dir = _save(hf, tmp_path, "teacher")
    teacher_run = tmp_path / "teacher.tsv"
    R.main(R.get_args(["--run_path", files["run"], "--queries_path", files["queries"], "--collection_path", files["collection"],
                       "--model_name_or_path", model_dir, "--tokenizer_name_or_path", files["tok_dir"], "--max_len", "48",
                       "--output_path", str(teacher_run)]))
    want = [ln.split("\t") for ln in teacher_run.read_text().splitlines()]
    t_score = {(int(c[0]), int(c[1])): float(c[3]) for c in want}
    model = CrossEncoder.from_pretrained(model_dir, max_len=48).cuda()
    ds = RerankingDataset(files["run"], files["queries"], files["collection"], tok, True, max_len=48)
    loader = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False, collate_fn=ds.collate_fn)
    ev = RerankingEvaluator(files["qrels"])
    mine_run = tmp_path / "mine.tsv"
    metrics = ev.compute_metrics(model, loader, output_rerank_path=str(mine_run), is_cross_encoder=True)
    got = [ln.split("\t") for ln in mine_run.read_text().splitlines()]
    assert sorted((int(c[0]), int(c[1])) for c in got) == sorted(t_score) and len(got) == len(want)
    assert list(dict.fromkeys(c[0] for c in got)) == list(dict.fromkeys(c[0] for c in want))
    # the padded batch path against the cached pair path: the bar of test_padded_forward_matches_score_cached (2e-3 of max|score|); the two
    # rankings agree wherever the teacher run's scores are further apart than that
    bar = 2e-3 * max(abs(v) for v in t_score.values())
    assert max(abs(float(c[3]) - t_score[(int(c[0]), int(c[1]))]) for c in got) <= bar
    for a, b in zip(got, got[1:]):
        if a[0] == b[0]:
            assert int(b[2]) == int(a[2]) + 1 and float(a[3]) >= float(b[3])
            assert t_score[(int(a[0]), int(a[1]))] >= t_score[(int(b[0]), int(b[1]))] - 2 * bar
    assert {k: float(v) for k, v in metrics.items()} == {k: float(v) for k, v in _run_metrics(mine_run, ev).items()}
