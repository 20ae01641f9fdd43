"""Teacher-score distillation on the GPU: the ``cldrd_distill_term`` kernel and ``losses.DistillLoss`` against goldens recorded from the
reference's ``KLDiv`` / ``MarginMSE`` / ``lambda_mrr_loss`` / ``ranknet_loss`` (tests/golden/make_distill_golden.py), the column mask and
determinism of the kernel, the trainer's fused step with the term (eager, graph replay, all score modes, both AMP modes), and the command
lines end to end: teacher run -> ``curriculum_file --with_scores`` -> ``trainer.nway_listwise --distill_loss``."""
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd.synthetic as syn
import selftest
from cldrd_amd import hip_ops as ops
from cldrd_amd.encoder import EncoderConfig
from cldrd_amd.models import NwayDualEncoder
from cldrd_amd.trainer import NwayTrainer
from oracle import losses_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"

G = np.load(os.path.join(conftest.GOLDEN, "distill_losses.npz"))
NAMES = [str(n) for n in G["names"]]


def _case(name):
    shape, kd, T, rank = name.split(".")[0], name.split(".")[1], float(G[name + "/T"]), name.rsplit(".", 1)[1]
    return (G[shape + "/y_pred"], G[shape + "/y_true"], G[shape + "/teacher"], kd, float(G[name + "/alpha"]), T,
            None if rank == "none" else rank)


def _close(value, grad, name):
    """The bars of tests/test_gpu_kernels.py::test_losses_match_reference_goldens (fp32 kernel against the reference's fp32)."""
    ref_v, ref_g = float(G[name + "/value"]), G[name + "/grad"]
    scale = float(np.abs(ref_g).max())
    err_v = abs(value - ref_v) / abs(ref_v)
    err_g = float(np.abs(grad - ref_g).max()) / scale
    print(f"{name}: value {value:.8g} (reference {ref_v:.8g}, rel {err_v:.1e}), gradient max error {err_g:.1e} of max|grad|")
    assert value == pytest.approx(ref_v, rel=3e-5, abs=1e-6)
    assert np.allclose(grad, ref_g, rtol=5e-4, atol=3e-5 * scale + 1e-9)


def test_the_golden_file_has_every_case():
    assert len(NAMES) == 5 * 2 * 3 * 3
    assert {n.split(".")[0] for n in NAMES} == {"8x30x30", "2x200x200", "4x120x30", "8x60x30", "1x7x3"}


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_reference_goldens(name):
    """cldrd_loss_fwd_bwd (when the case has a rank term) then cldrd_distill_term on the same buffers, as the trainer chains them."""
    y_pred, y_true, teacher, kd, alpha, T, rank = _case(name)
    yp, yt, te = (torch.tensor(a, device=DEV) for a in (y_pred, y_true, teacher))
    if rank is None:
        loss_out, grad = torch.zeros(2, device=DEV), torch.zeros_like(yp)
    else:
        loss_out, grad = ops.loss_fwd_bwd(rank, yp, yt)
    term = torch.full((1,), float("nan"), device=DEV)
    ops.distill_term(kd, yp, te, alpha, T, loss_out, grad, term)
    torch.cuda.synchronize()
    _close(loss_out[0].item(), grad.cpu().numpy(), name)
    assert term.item() == pytest.approx(float(G[name + "/kd"]), rel=3e-5, abs=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_distill_loss_module_matches_the_reference_goldens(name):
    """The reference-style loop: loss = crit(y_pred, labels, teacher); loss.backward()."""
    from cldrd_amd.losses import DistillLoss
    y_pred, y_true, teacher, kd, alpha, T, rank = _case(name)
    yp = torch.tensor(y_pred, device=DEV, requires_grad=True)
    crit = DistillLoss(rank=rank, kd=kd, alpha=alpha, T=T)
    loss = crit(yp, torch.tensor(y_true, device=DEV) if rank is not None else None, torch.tensor(teacher, device=DEV))
    loss.backward()
    _close(loss.item(), yp.grad.cpu().numpy(), name)
    assert crit.last_kd.item() == pytest.approx(float(G[name + "/kd"]), rel=3e-5, abs=1e-6)


@pytest.mark.parametrize("kd", ["kl_div", "margin_mse"])
@pytest.mark.parametrize("shape", [(4, 120, 30), (8, 60, 30), (1, 7, 3), (8, 30, 30), (11, 70, 67)])
def test_column_mask_alpha_zero_and_determinism(kd, shape):
    B, Np, Nt = shape
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + Np)
    logits = 100.0 + 5.0 * torch.randn(B, Np, device=DEV, generator=gen)
    teacher = 4.0 * torch.randn(B, Nt, device=DEV, generator=gen)
    grad0 = torch.randn(B, Np, device=DEV, generator=gen)
    grad0[0, 0] = -0.0
    loss0 = torch.tensor([1.25, 7.0], device=DEV)

    def run(alpha):
        loss, grad, term = loss0.clone(), grad0.clone(), torch.zeros(1, device=DEV)
        ops.distill_term(kd, logits, teacher, alpha, 2.0, loss, grad, term)
        torch.cuda.synchronize()
        return loss, grad, term

    loss, grad, term = run(0.75)
    # columns >= Nt (the in-batch negatives): bit-identical before and after the call
    assert torch.equal(grad[:, Nt:].view(torch.int32), grad0[:, Nt:].view(torch.int32))
    assert not torch.equal(grad[:, :Nt], grad0[:, :Nt]) and loss[1].item() == 7.0 and loss[0].item() != 1.25
    ref_v, ref_g = (LR.kl_div(logits[:, :Nt].cpu().numpy(), teacher.cpu().numpy(), 2.0) if kd == "kl_div"
                    else LR.margin_mse(logits[:, :Nt].cpu().numpy(), teacher.cpu().numpy()))
    # Random rows can have a KL of 0.01 that is a sum of +-0.3 terms p_t (log p_t - log p_s); a log-softmax entry of fp32 logits / T ~ 50 is
    # only known to one fp32 spacing at that magnitude (2^-18 = 3.8e-6), and the KL is a p_t-weighted mean of differences of such entries:
    # the value bar gets two spacings of max|logits / T| as its absolute part (the float64 oracle is the reference here, not fp32 torch).
    ulp = 2.0 * float(np.spacing(np.float32(logits.abs().max().item() / 2.0)))
    assert term.item() == pytest.approx(ref_v, rel=3e-5, abs=1e-6 + ulp)
    assert loss[0].item() == pytest.approx(1.25 + 0.75 * ref_v, rel=3e-5, abs=1e-6 + ulp)
    got = (grad[:, :Nt] - grad0[:, :Nt]).double().cpu().numpy()
    scale = float(np.abs(0.75 * ref_g).max())
    # (the difference of two fp32 gradients: on top of the kernel bar, the rounding of grad0 + term at grad0's magnitude, 2^-23 relative each way)
    assert np.allclose(got, 0.75 * ref_g, rtol=5e-4, atol=3e-5 * scale + 1e-6 * float(grad0.abs().max()))
    # two calls on the same inputs: the same bits
    loss2, grad2, term2 = run(0.75)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    assert torch.equal(term.view(torch.int32), term2.view(torch.int32))
    # alpha = 0: loss_out and grad bit-identical (a -0 stays a -0), the unweighted term still reported
    lossz, gradz, termz = run(0.0)
    assert torch.equal(lossz.view(torch.int32), loss0.view(torch.int32)) and torch.equal(gradz.view(torch.int32), grad0.view(torch.int32))
    assert torch.equal(termz.view(torch.int32), term.view(torch.int32))


def test_wrapper_and_entry_point_refusals():
    from cldrd_amd._lib import CldrdError
    lg, te, lo, gr = (torch.zeros(2, 6, device=DEV), torch.zeros(2, 4, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, 6, device=DEV))
    with pytest.raises(ValueError):
        ops.distill_term("ranknet", lg, te, 1.0, 1.0, lo, gr)
    with pytest.raises(ValueError):
        ops.distill_term("kl_div", lg, torch.zeros(2, 7, device=DEV), 1.0, 1.0, lo, gr)          # Nt > Np
    with pytest.raises(ValueError):
        ops.distill_term("kl_div", lg, torch.zeros(3, 4, device=DEV), 1.0, 1.0, lo, gr)
    with pytest.raises(ValueError):
        ops.distill_term("kl_div", lg, te, 1.0, 1.0, lo, torch.zeros(2, 5, device=DEV))
    with pytest.raises(CldrdError, match="alpha"):
        ops.distill_term("kl_div", lg, te, -1.0, 1.0, lo, gr)
    with pytest.raises(CldrdError, match="T > 0"):
        ops.distill_term("kl_div", lg, te, 1.0, 0.0, lo, gr)
    with pytest.raises(RuntimeError):
        ops.distill_term("kl_div", lg.cpu(), te, 1.0, 1.0, lo, gr)


# ---------------------------------------------------------------------------------------------------------------- trainer
def _model(mode, cfg=None, seed=3):
    model = selftest.build_tiny_model(cfg or selftest.tiny_config(), seed=seed)
    model.in_batch_loss, model.all_in_batch_neg = mode != 0, mode == 1
    return model.cuda().train()


def _dev(batch):
    return {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}


def _not_embedding(tr):
    emb = torch.zeros(tr.flat_p.numel(), dtype=torch.bool, device=DEV)
    for t, toff in zip(tr.model.towers(), tr.model._tower_offsets):
        for n in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight"):
            off, shape = t.layout.entries[n]
            emb[toff + off:toff + off + shape[0] * shape[1]] = True
    return ~emb


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kd,alpha,T", [("margin_mse", 0.5, 1.0), ("kl_div", 2.0, 2.0)])
def test_trainer_loss_is_rank_plus_alpha_kd_of_its_own_logits(amp, mode, kd, alpha, T, monkeypatch):
    """loss_out[0] of forward_backward against oracle/losses_ref.py (float64) on the logits the step returned: the rank loss over all Np
    columns (in-batch columns labelled -0.5) plus alpha times the distillation term over the row's own nway columns."""
    monkeypatch.setenv("CLDRD_AMP", amp)
    B, N = 4, 6
    batch = syn.nway_batch(77 + mode, B, N, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True)
    tr = NwayTrainer(_model(mode), loss="lambda_mrr", distill=kd, distill_alpha=alpha, distill_T=T)
    assert tr.amp16 == (amp == "fp16")
    loss_out, logits = tr.forward_backward(batch)
    torch.cuda.synchronize()
    Np = {0: N, 1: B * N, 2: 2 * N}[mode]
    assert tuple(logits.shape) == (B, Np)
    lg = logits.double().cpu().numpy()
    labels = np.concatenate([batch["labels"].numpy(), np.full((B, Np - N), -0.5, np.float32)], axis=1)
    rank_v, _ = LR.lambda_mrr(lg, labels)
    te = batch["teacher_scores"].numpy()
    kd_v, _ = LR.kl_div(lg[:, :N], te, T) if kd == "kl_div" else LR.margin_mse(lg[:, :N], te)
    print(f"amp {amp} mode {mode} {kd}: loss {loss_out[0].item():.8g}, oracle rank {rank_v:.8g} + {alpha} * kd {kd_v:.8g}")
    assert loss_out[0].item() == pytest.approx(rank_v + alpha * kd_v, rel=3e-5, abs=1e-6)
    assert tr.last_kd.item() == pytest.approx(kd_v, rel=3e-5, abs=1e-6)
    assert torch.isfinite(tr.flat_g).all().item()
    # distill_only drops the rank term
    tr2 = NwayTrainer(_model(mode), loss="lambda_mrr", distill=kd, distill_alpha=alpha, distill_T=T, distill_only=True)
    loss2, logits2 = tr2.forward_backward(batch)
    torch.cuda.synchronize()
    lg2 = logits2.double().cpu().numpy()
    kd2, _ = LR.kl_div(lg2[:, :N], te, T) if kd == "kl_div" else LR.margin_mse(lg2[:, :N], te)
    assert loss2[0].item() == pytest.approx(alpha * kd2, rel=3e-5, abs=1e-6) and loss2[1].item() == 0.0


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_alpha_zero_gives_the_gradient_of_a_trainer_without_distillation(amp, mode, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", amp)
    batch = syn.nway_batch(91, 3, 5, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True)
    res = []
    for distill in (None, "margin_mse", "kl_div"):
        tr = NwayTrainer(_model(mode), loss="lambda_mrr", distill=distill, distill_alpha=0.0)
        loss_out, logits = tr.forward_backward(batch)          # a trainer without `distill` ignores the teacher_scores key
        torch.cuda.synchronize()
        res.append((loss_out.clone(), logits.clone(), tr.flat_g[_not_embedding(tr)].clone()))
        assert (tr.last_kd is None) == (distill is None)
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
        assert torch.equal(res[0][2].view(torch.int32), other[2].view(torch.int32))
    assert res[0][2].abs().max().item() > 0.0


def test_a_distilling_trainer_needs_teacher_scores_and_checks_their_shape():
    batch = syn.nway_batch(5, 2, 4, 8, 16, vocab=512, label_kind="mode9")
    tr = NwayTrainer(_model(0), distill="kl_div")
    with pytest.raises(ValueError, match="teacher_scores"):
        tr.forward_backward(batch)
    with pytest.raises(ValueError, match="teacher_scores"):
        tr.train_step(batch)
    bad = dict(batch)
    bad["teacher_scores"] = torch.zeros(2, 5)
    with pytest.raises(ValueError, match=r"\[2, 4\]"):
        tr.forward_backward(bad)
    with pytest.raises(ValueError):
        NwayTrainer(tr.model, distill="ranknet")
    with pytest.raises(ValueError):
        NwayTrainer(tr.model, distill_only=True)
    with pytest.raises(ValueError):
        NwayTrainer(tr.model, distill="kl_div", distill_T=0.0)


def test_graph_replay_of_the_distilling_step_equals_the_eager_step(monkeypatch):
    """The comparison of tests/test_gpu_model.py::test_graph_replay_of_the_training_step_equals_the_eager_step with a distillation term and
    DIFFERENT teacher scores every step: from identical state (snapshot / restore of parameters, moments, counters) the replayed step and
    the plain eager step must agree - loss, the distillation term, logits and every gradient outside the embedding tables bit for bit
    (dropout on), the embedding-table gradients (float atomics) and the updated parameters to rounding.  Teacher scores baked into the
    captured graph would give the first captured batch's term on every replay."""
    cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=64,
                        dropout=0.1, attention_dropout=0.1)
    monkeypatch.setenv("CLDRD_GRAPH", "1")
    torch.manual_seed(0)
    model = NwayDualEncoder(cfg, share_weights=False).cuda().train()
    with torch.no_grad():
        for seed, tower in ((11, model.query_encoder), (12, model.passage_encoder)):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed, name, tuple(p.shape), std=0.05, perturb=True))
    tr = NwayTrainer(model, loss="lambda_mrr", learning_rate=3e-3, warmup_steps=5, total_steps=40, distill="margin_mse", distill_alpha=0.5)
    towers = model.towers()
    keep = _not_embedding(tr)

    def snapshot():
        return (tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.global_step, tr.adam_step, [t.step_seed for t in towers])

    def restore(sn):
        tr.flat_p.copy_(sn[0]); tr.m.copy_(sn[1]); tr.v.copy_(sn[2])
        tr.global_step, tr.adam_step = sn[3], sn[4]
        for t, ss in zip(towers, sn[5]):
            t.step_seed = ss
            t.refresh_shadows(need_transposed=True)

    replays, kds = 0, []
    for i in range(11):
        shape = (3, 4, 8, 16) if i != 8 else (2, 3, 8, 16)
        batch = _dev(syn.nway_batch(100 + i, *shape, vocab=cfg.vocab_size, ragged=True, label_kind="mode9", with_teacher_scores=True))
        sn = snapshot()
        monkeypatch.setenv("CLDRD_GRAPH", "1")
        l1 = tr.train_step(batch).clone()
        kd1 = tr.last_kd.clone()
        lg1, g1, p1 = tr.last_logits.clone(), tr.flat_g.clone(), tr.flat_p.clone()
        key = tr._batch_key(batch)
        replayed = key in getattr(tr, "_graphs", {}) and tr._graphs[key]["graph"] is not None
        replays += int(replayed)
        # the plain eager step from the same state: no device-side step state at all
        restore(sn)
        state, ptrs = tr._state, [getattr(t, "seed_base_ptr", None) for t in towers]
        tr._state = None
        for t in towers:
            t.seed_base_ptr = None
        monkeypatch.setenv("CLDRD_GRAPH", "0")
        l0 = tr.train_step(batch).clone()
        kd0 = tr.last_kd.clone()
        tr._state = state
        for t, pp in zip(towers, ptrs):
            t.seed_base_ptr = pp
        torch.cuda.synchronize()
        assert torch.equal(l1, l0), (i, replayed, l1, l0)
        assert torch.equal(kd1, kd0), (i, replayed, kd1, kd0)
        assert torch.equal(lg1, tr.last_logits), (i, replayed)
        assert torch.equal(g1[keep], tr.flat_g[keep]), (i, replayed)
        ge = (g1[~keep] - tr.flat_g[~keep]).abs().max().item()
        assert ge <= 1e-5 * max(1.0, g1[~keep].abs().max().item()), (i, ge)
        assert (p1 - tr.flat_p).abs().max().item() <= 1e-6, i
        # the term is this step's: MarginMSE of the returned logits against THIS batch's teacher scores
        ref_kd, _ = LR.margin_mse(lg1.double().cpu().numpy(), batch["teacher_scores"].cpu().numpy())
        assert kd1.item() == pytest.approx(ref_kd, rel=3e-5, abs=1e-6), (i, replayed)
        kds.append(kd1.item())
    assert replays >= 6, replays                    # (at least three replayed steps after the capture)
    assert len(set(kds)) == len(kds)
    assert tr.global_step == tr.adam_step == 11


def test_pure_distillation_learns():
    """dropout 0, one fixed batch, distill_only, MarginMSE, 30 steps: the term after the last step is below its value at the first."""
    batch = _dev(syn.nway_batch(4680, 4, 6, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True))
    # learning rate 1e-3 (Adam, no warm-up), chosen once on an MI355X: MarginMSE 76.5221 at the first step, 0.0715872 after 30
    tr = NwayTrainer(_model(0), loss="lambda_mrr", learning_rate=1e-3, warmup_steps=0, total_steps=1000, distill="margin_mse",
                     distill_only=True)
    kd = []
    for _ in range(30):
        loss_out = tr.train_step(batch)
        kd.append(tr.last_kd.item())
        assert loss_out[0].item() == pytest.approx(kd[-1], rel=1e-6)
    print(f"pure distillation: MarginMSE {kd[0]:.6g} at the first step, {kd[-1]:.6g} after 30")
    assert np.isfinite(kd).all() and kd[-1] < kd[0]


# ------------------------------------------------------------------------------------------------------------ end to end
N_P, N_Q, TOP = 300, 16, 60


def _teacher(tmp_path, vocab):
    from transformers import BertConfig, BertForSequenceClassification
    torch.manual_seed(17)
    cfg = BertConfig(vocab_size=vocab, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                     max_position_embeddings=512, num_labels=1, initializer_range=0.05)
    m = BertForSequenceClassification(cfg).eval()
    with torch.no_grad():       # spread the random logits
        m.classifier.weight.mul_(10.0)
    path = str(tmp_path / "teacher")
    m.save_pretrained(path)
    return path


def test_teacher_run_to_scored_file_to_distilling_trainer_end_to_end(tmp_path):
    """Index, retrieve, teacher scoring (the steps of tests/test_gpu_curriculum.py, same tiny models and corpus), then
    ``curriculum_file --with_scores`` and two epochs of ``trainer.nway_listwise --distill_loss kl_div`` through the worker loader."""
    from cldrd_amd.dataset import curriculum_file as C
    from cldrd_amd.retriever import index_text, rerank_top_passages, retrieve_top_passages
    from cldrd_amd.trainer import nway_listwise as T
    from test_rerank_host import make_pair_tokenizer, words
    rng = np.random.default_rng(23)
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    c_path, q_path = tmp_path / "collection.tsv", tmp_path / "queries.train.tsv"
    c_path.write_text("".join(f"{9000 + j}\t{words(int(rng.integers(3, 24)), 5 * j)}\n" for j in range(N_P)))
    qids = [int(q) for q in rng.choice(100000, N_Q, replace=False)]
    q_path.write_text("".join(f"{q}\t{words(int(rng.integers(2, 7)), 3 * i)}\n" for i, q in enumerate(qids)))

    cfg = selftest.tiny_config()
    student = selftest.build_tiny_model(cfg)
    mdir = tmp_path / "student"
    student.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp_path / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt)
    common = ["--resume", str(ckpt), "--model_name_or_path", str(mdir), "--tokenizer_name_or_path", tok_dir]
    index_path = index_text.main(index_text.get_args(common + ["--passages_path", str(c_path), "--index_dir", str(tmp_path / "index"),
                                                               "--max_length", "32"]))
    run_path = tmp_path / "runs" / "train.top60.run"
    retrieve_top_passages.main(retrieve_top_passages.get_args(common + ["--queries_path", str(q_path), "--index_path", index_path,
                                                                        "--max_length", "16", "--top_k", str(TOP),
                                                                        "--output_path", str(run_path)]))
    teacher_run = tmp_path / "runs" / "train.top60.teacher.run"
    rerank_top_passages.main(rerank_top_passages.get_args([
        "--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path),
        "--model_name_or_path", _teacher(tmp_path, tok.vocab_size + 4), "--tokenizer_name_or_path", tok_dir, "--max_len", "64",
        "--output_path", str(teacher_run)]))
    scores = {}
    for line in teacher_run.read_text().splitlines():
        q, p, _, s = line.split("\t")
        scores.setdefault(int(q), {})[int(p)] = float(s)

    train_path = tmp_path / "train.10relT_20neg.scored.json"
    n, skipped = C.main(C.get_args(["--run_path", str(teacher_run), "--label_mode", "9", "--output_path", str(train_path),
                                    "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "5", "--with_scores"]))
    assert (n, skipped) == (N_Q, 0)
    for ex in (json.loads(line) for line in train_path.read_text().splitlines()):
        for pk, sk in (("relT_pids", "relT_scores"), ("most_hard_pids", "most_hard_scores"), ("semi_hard_pids", "semi_hard_scores")):
            assert ex[sk] == [scores[ex["qid"]][p] for p in ex[pk]]

    args = T.set_env(T.get_args([
        "--experiment_folder", str(tmp_path), "--run_folder", "stage2", "--queries_path", str(q_path), "--collection_path", str(c_path),
        "--training_path", str(train_path), "--label_mode", "9", "--model_name_or_path", str(mdir), "--model_checkpoint", str(ckpt),
        "--tokenizer_name_or_path", tok_dir, "--query_max_len", "16", "--passage_max_len", "32", "--train_batch_size", "4",
        "--logging_steps", "1", "--evaluate_steps", "4", "--warmup_steps", "1", "--num_train_epochs", "2", "--learning_rate", "1e-3",
        "--loader_workers", "2", "--distill_loss", "kl_div", "--distill_alpha", "0.5"]))
    tr = T.train(args)
    assert tr.distill == "kl_div" and tr.distill_alpha == 0.5
    assert tr.global_step == 2 * N_Q // 4 and tr.skipped_steps() == 0
    assert torch.isfinite(tr.flat_p).all().item()
    log = (tmp_path / "stage2" / "log" / "train_logs.log").read_text().splitlines()
    header = log[0].split("\t")
    assert "kd_loss" in header
    col = header.index("kd_loss")
    kd = [float(line.split("\t")[col]) for line in log[1:]]
    losses = [float(line.split("\t")[2]) for line in log[1:]]
    assert len(kd) == tr.global_step - 1 and np.isfinite(kd).all() and np.isfinite(losses).all()          # the first logging call only writes the header
    assert tr.last_kd.item() > 0.0
    assert os.path.exists(tmp_path / "stage2" / "models" / f"checkpoint_{tr.global_step}.pth.tar")
