"""``cldrd_lambda_term`` and ``--loss lambda_loss`` on the GPU: the kernel against goldens recorded from the reference's ``lambda_loss``
(tests/golden/make_lambda_term_golden.py) and the float64 oracle, bit equality with ``cldrd_lambda_loss_fwd_bwd`` where the two compute
the same thing, the accumulate form, determinism; then the trainer's fused step with the term (against the oracle, graph replay against
the eager step with teacher labels that change every step, --deterministic, learning) and the command lines end to end: teacher run ->
``curriculum_file --with_scores`` -> ``trainer.nway_listwise --loss lambda_loss --label_source teacher``."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd.synthetic as syn
import test_gpu_distill as D            # its tiny models, batch mover and teacher (helpers only)
from cldrd_amd import hip_ops as ops
from cldrd_amd.encoder import EncoderConfig
from cldrd_amd.models import NwayDualEncoder
from cldrd_amd.trainer import NwayTrainer
from oracle import losses_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"

G = np.load(os.path.join(conftest.GOLDEN, "lambda_term.npz"))
META = json.loads(str(G["meta"]))
NAMES = sorted(META, key=lambda s: int(s[4:]))
_spec = importlib.util.spec_from_file_location("make_lambda_term_golden", os.path.join(conftest.GOLDEN, "make_lambda_term_golden.py"))
_gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gold)
transform = _gold.transform             # the label transform in fp32, as the goldens were made


def _bits(t):
    return t.contiguous().view(torch.int32)


def _kw(name):
    kw = dict(META[name])
    pad = kw.pop("pad")
    kw["padded_value_indicator"] = float("-inf") if pad == "-inf" else pad
    return kw


def _term(logits, labels, loss=None, grad=None, **kw):
    """ops.lambda_term on fresh (NaN-filled) or given outputs -> (loss_out, grad, term)."""
    loss = torch.full((2,), float("nan"), device=DEV) if loss is None else loss.clone()
    grad = torch.full_like(logits, float("nan")) if grad is None else grad.clone()
    term = torch.full((1,), float("nan"), device=DEV)
    ops.lambda_term(logits, labels, loss, grad, term, **kw)
    torch.cuda.synchronize()
    return loss, grad, term


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_reference_goldens(name):
    """The bars of tests/test_gpu_kernels.py::test_lambda_loss_kernel_against_reference_goldens: 2e-4 relative (+ 1e-6) on the value, 2e-4
    of the largest gradient entry on the gradient."""
    logits, labels = torch.tensor(G[name + ".logits"], device=DEV), torch.tensor(G[name + ".labels"], device=DEV)
    Ns = labels.shape[1]
    loss, grad, term = _term(logits, labels, **_kw(name))
    ref_v, ref_g = float(G[name + ".value"]), G[name + ".grad"]
    got_g = grad[:, :Ns].cpu().numpy()
    print(f"{name}: value {loss[0].item():.8g} (reference {ref_v:.8g}), gradient max error {np.abs(got_g - ref_g).max():.3g} "
          f"of max|grad| {np.abs(ref_g).max():.3g}, pairs {loss[1].item():.0f}")
    assert abs(loss[0].item() - ref_v) <= 2e-4 * abs(ref_v) + 1e-6, (META[name], loss[0].item(), ref_v)
    assert np.abs(got_g - ref_g).max() <= 2e-4 * np.abs(ref_g).max() + 1e-7, META[name]
    assert torch.equal(_bits(term), _bits(loss[0:1]))                                   # alpha = 1: the weighted term is the term
    assert loss[1].item() >= 0 and loss[1].item() == int(loss[1].item())                # (k = 1 under a pairwise scheme: no pair, sum 0)
    assert (grad[:, Ns:] == 0).all().item()                                             # the overwrite form zeroes the columns behind the slate


def _oracle_case():
    B, N = 8, 200                                              # the slates of tests/test_gpu_kernels.py's oracle test
    yp = (syn.normal(50, B * N).reshape(B, N) * 3.0).astype(np.float32)
    yt = np.tile(syn.labels_mode9(B, 30), (1, 7))[:, :N].copy()
    yt[:, 190:] = -1.0
    return yp, yt


@pytest.mark.parametrize("sch", [None, "ndcgLoss2PP_scheme", "lambdaRank_scheme", "rankNetWeightedByGTDiffPowed_scheme", "ndcgLoss1_scheme"])
def test_kernel_matches_the_oracle_on_bigger_slates(sch):
    """[8, 200], k = 50, against oracle/losses_ref.py at the bars of test_lambda_loss_demo_and_bigger_slate_vs_oracle."""
    yp, yt = _oracle_case()
    v, g = LR.lambda_loss(yp, yt, weighing_scheme=sch, k=50)
    for extra in (0, 5):
        logits = torch.tensor(np.concatenate([yp, np.full((8, extra), 7.0, np.float32)], axis=1), device=DEV)
        loss, grad, _ = _term(logits, torch.tensor(yt, device=DEV), weighing_scheme=sch, k=50)
        err = np.abs(grad[:, :200].cpu().numpy() - g).max()
        print(f"{sch} Np = {200 + extra}: value {loss[0].item():.8g} (oracle {v:.8g}), gradient max error {err:.3g} of max|grad| {np.abs(g).max():.3g}")
        assert abs(loss[0].item() - v) <= 2e-4 * abs(v) + 1e-6
        assert err <= 5e-4 * np.abs(g).max() + 1e-8


def test_the_degenerate_configuration_equals_lambda_loss_fwd_bwd_bit_for_bit():
    """accumulate 0, alpha 1, Ns == Np, no label transform: the bits of cldrd_lambda_loss_fwd_bwd - value, pair count and gradient."""
    cases = [(torch.tensor(G[n + ".logits"], device=DEV), torch.tensor(G[n + ".labels"], device=DEV), _kw(n)) for n in NAMES
             if G[n + ".logits"].shape[1] == G[n + ".labels"].shape[1] and not (META[n]["neg_mean"] or META[n]["row_min"] or META[n]["label_offset"])]
    yp, yt = _oracle_case()
    cases += [(torch.tensor(yp, device=DEV), torch.tensor(yt, device=DEV), dict(weighing_scheme=s, k=50, reduction=r))
              for s in (None, "ndcgLoss2PP_scheme") for r in ("mean", "sum")]
    assert len(cases) >= 20
    for logits, labels, kw in cases:
        kw = {k: v for k, v in kw.items() if k not in ("neg_mean", "row_min", "n_rel", "label_offset")}
        out, g = ops.lambda_loss_fwd_bwd(logits, labels, **kw)
        loss, grad, term = _term(logits, labels, **kw)
        assert torch.equal(_bits(loss), _bits(out)), (kw, loss, out)
        assert torch.equal(_bits(grad), _bits(g)), kw
        assert torch.equal(_bits(term), _bits(out[0:1]))


@pytest.mark.parametrize("shape", [(3, 35, 30), (11, 70, 67), (1, 7, 3), (5, 300, 257), (4, 31, 31)])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_accumulate_form_column_mask_alpha_and_determinism(shape, reduction):
    B, Np, Ns = shape
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + Np)
    logits = 100.0 + 5.0 * torch.randn(B, Np, device=DEV, generator=gen)
    labels = 8.0 + 4.0 * torch.randn(B, Ns, device=DEV, generator=gen)
    grad0 = torch.randn(B, Np, device=DEV, generator=gen)
    grad0[:, Ns:] = float("nan")                      # the columns behind the slate: neither read nor written
    grad0[0, 0] = -0.0
    loss0 = torch.tensor([1.25, 7.0], device=DEV)
    kw = dict(weighing_scheme="ndcgLoss1_scheme", padded_value_indicator=float("-inf"), neg_mean=True, row_min=True, n_rel=Ns // 3,
              reduction=reduction)
    over_loss, over_grad, over_term = _term(logits, labels, **kw)                    # the overwrite form: what gets added
    assert torch.isfinite(over_grad).all().item() and over_grad[:, :Ns].abs().max().item() > 0 and (over_grad[:, Ns:] == 0).all().item()
    for alpha in (1.0, 2.0):
        loss, grad, term = _term(logits, labels, loss0, grad0, alpha=alpha, accumulate=True, **kw)
        assert torch.equal(_bits(grad[:, Ns:]), _bits(grad0[:, Ns:]))
        # alpha * x is exact for alpha = 1, 2, so the sum is the one fp32 addition whether or not the kernel fuses it: alpha = 2 doubles the added part
        assert torch.equal(_bits(grad[:, :Ns]), _bits(grad0[:, :Ns] + alpha * over_grad[:, :Ns]))
        assert torch.equal(_bits(loss), _bits(torch.stack([loss0[0] + alpha * over_term[0], loss0[1]])))
        assert torch.equal(_bits(term), _bits(over_term))
        loss2, grad2, term2 = _term(logits, labels, loss0, grad0, alpha=alpha, accumulate=True, **kw)          # two launches: the same bits
        assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(grad), _bits(grad2)) and torch.equal(_bits(term), _bits(term2))
    lossz, gradz, termz = _term(logits, labels, loss0, grad0, alpha=0.0, accumulate=True, **kw)
    assert torch.equal(_bits(lossz), _bits(loss0)) and torch.equal(_bits(gradz), _bits(grad0))      # bit for bit: the -0 stays a -0
    assert torch.equal(_bits(termz), _bits(over_term))
    over2 = _term(logits, labels, **kw)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((over_loss, over_grad, over_term), over2))


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_forty_calls_in_a_row_give_the_bits_of_the_first(B, streams):
    """More launches than the kernel has arrival slots, back to back on one stream or alternating over two: every launch finds its slot at
    zero and leaves it at zero, and the workgroup that arrives last (B = 1: the first ticket is the last) adds the rows of its own launch.
    The first call at the bars of test_kernel_matches_the_oracle_on_bigger_slates."""
    yp, yt = _oracle_case()
    yp, yt = yp[:B], yt[:B]
    v, g = LR.lambda_loss(yp, yt, weighing_scheme="ndcgLoss2PP_scheme", k=50)
    logits, labels = torch.tensor(yp, device=DEV), torch.tensor(yt, device=DEV)
    outs = [(torch.full((2,), float("nan"), device=DEV), torch.full_like(logits, float("nan"))) for _ in range(40)]
    lanes = [torch.cuda.Stream() for _ in range(streams)]
    for s in lanes:
        s.wait_stream(torch.cuda.current_stream())
    for i, (loss, grad) in enumerate(outs):
        with torch.cuda.stream(lanes[i % streams]):
            ops.lambda_term(logits, labels, loss, grad, weighing_scheme="ndcgLoss2PP_scheme", k=50)
    for s in lanes:
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    loss0, grad0 = outs[0]
    assert abs(loss0[0].item() - v) <= 2e-4 * abs(v) + 1e-6
    assert np.abs(grad0.cpu().numpy() - g).max() <= 5e-4 * np.abs(g).max() + 1e-8
    for i, (loss, grad) in enumerate(outs[1:], 1):
        assert torch.equal(_bits(loss), _bits(loss0)) and torch.equal(_bits(grad), _bits(grad0)), i


def test_wrapper_and_entry_point_refusals():
    from cldrd_amd._lib import CldrdError
    z = lambda *s: torch.zeros(*s, device=DEV)          # noqa: E731
    with pytest.raises(ValueError):
        ops.lambda_term(z(2, 6), z(2, 7), z(2), z(2, 6))          # Ns > Np
    with pytest.raises(ValueError):
        ops.lambda_term(z(2, 6), z(3, 4), z(2), z(2, 6))
    with pytest.raises(ValueError):
        ops.lambda_term(z(2, 6), z(2, 4), z(2), z(2, 5))
    with pytest.raises(CldrdError, match="lambda_term: need alpha"):
        ops.lambda_term(z(2, 6), z(2, 4), z(2), z(2, 6), alpha=-1.0)
    with pytest.raises(CldrdError, match="lambda_term: need 0 <= n_rel"):
        ops.lambda_term(z(2, 6), z(2, 4), z(2), z(2, 6), n_rel=5)


def test_torch_op_value_and_autograd():
    name = "case0"
    logits = torch.tensor(G[name + ".logits"], device=DEV, requires_grad=True)
    labels = torch.tensor(G[name + ".labels"], device=DEV)
    m = META[name]
    out, _ = torch.ops.cldrd.lambda_term(logits, labels, 0.5, 0, labels.shape[1], 0.0, ops.LAMBDA_SCHEMES[m["weighing_scheme"]], m["k"] or 0, 1e-4,
                                         m["sigma"], m["mu"], -1.0, m["reduction"] == "mean", m["reduction_log"] == "binary", m["gain"] == "linear")
    out[0].backward()
    ref_v, ref_g = float(G[name + ".value"]), G[name + ".grad"]
    assert out[2].item() == pytest.approx(ref_v, rel=2e-4, abs=1e-6) and out[0].item() == pytest.approx(0.5 * ref_v, rel=2e-4, abs=1e-6)
    Ns = labels.shape[1]
    assert np.abs(logits.grad[:, :Ns].cpu().numpy() - 0.5 * ref_g).max() <= 2e-4 * np.abs(0.5 * ref_g).max() + 1e-7


# ---------------------------------------------------------------------------------------------------------------- trainer
def _oracle_loss(tr, logits, batch, N):
    """float64 lambda_loss of the logits a step returned, under the trainer's options (the label transform in fp32, as the kernel's)."""
    lg = logits.double().cpu().numpy()
    kw = tr._lambda_kw
    okw = dict(weighing_scheme=kw["weighing_scheme"], k=kw["k"], sigma=kw["sigma"], mu=kw["mu"], gain=kw["gain"], reduction_log=kw["reduction_log"])
    if tr.label_source == "teacher":
        lab = transform(batch["teacher_scores"].cpu().numpy(), -np.inf, kw["neg_mean"], kw["row_min"], kw["n_rel"], 0.0)
        return LR.lambda_loss(lg[:, :N], lab.astype(np.float64), padded_value_indicator=-np.inf, **okw)[0]
    labels = np.concatenate([batch["labels"].cpu().numpy(), np.full((lg.shape[0], lg.shape[1] - N), -0.5, np.float32)], axis=1)
    return LR.lambda_loss(lg, labels, **okw)[0]


TRAINER_CASES = {
    "rank": dict(weighing_scheme="ndcgLoss1_scheme"),
    "rank-ndcg2pp-k4": dict(weighing_scheme="ndcgLoss2PP_scheme", lambda_k=4, lambda_sigma=2.0, lambda_log="binary"),
    "teacher-original": dict(weighing_scheme="ndcgLoss1_scheme", label_source="teacher"),
    "teacher-mean-row_min": dict(weighing_scheme="ndcgLoss1_scheme", label_source="teacher", neg_score_mode="mean", teacher_label_shift="row_min", n_rel=2),
    "rank+margin_mse": dict(weighing_scheme="ndcgLoss1_scheme", distill="margin_mse", distill_alpha=0.5),
    "teacher+margin_mse": dict(weighing_scheme="lambdaRank_scheme", label_source="teacher", teacher_label_shift="row_min", distill="margin_mse",
                               distill_alpha=0.5),
}


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("case", list(TRAINER_CASES))
@pytest.mark.parametrize("mode", [0, 2])
def test_trainer_loss_is_lambda_loss_of_its_own_logits(amp, case, mode, monkeypatch):
    """loss_out[0] of forward_backward against oracle/losses_ref.py (float64) on the logits the step returned, at the bars of
    tests/test_gpu_distill.py::test_trainer_loss_is_rank_plus_alpha_kd_of_its_own_logits."""
    kw = TRAINER_CASES[case]
    if mode != 0 and kw.get("label_source") == "teacher":
        with pytest.raises(ValueError, match="--in_batch_loss"):
            NwayTrainer(D._model(mode), loss="lambda_loss", **kw)
        return
    monkeypatch.setenv("CLDRD_AMP", amp)
    B, N = 4, 6
    batch = syn.nway_batch(77 + mode, B, N, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True)
    tr = NwayTrainer(D._model(mode), loss="lambda_loss", **kw)
    loss_out, logits = tr.forward_backward(batch)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (B, {0: N, 2: 2 * N}[mode])
    want = _oracle_loss(tr, logits, batch, N)
    if tr.distill is not None:
        kd_v, _ = LR.margin_mse(logits.double().cpu().numpy()[:, :N], batch["teacher_scores"].numpy())
        assert tr.last_kd.item() == pytest.approx(kd_v, rel=3e-5, abs=1e-6)
        want += tr.distill_alpha * kd_v
    print(f"amp {amp} mode {mode} {case}: loss {loss_out[0].item():.8g}, oracle {want:.8g}, relative error {abs(loss_out[0].item() - want) / abs(want):.2e}")
    assert want > 0 and loss_out[0].item() == pytest.approx(want, rel=3e-5, abs=1e-6)
    assert torch.isfinite(tr.flat_g).all().item() and tr.flat_g.abs().max().item() > 0
    # train_metrics under teacher labels: the column with the highest teacher score is the relevant one
    lab = tr.metric_labels(D._dev(batch), logits.shape[1])
    assert tuple(lab.shape) == tuple(logits.shape) and (lab == 1).sum(dim=1).min().item() >= 1
    if tr.label_source == "teacher":
        assert torch.equal(lab.argmax(dim=1).cpu(), batch["teacher_scores"].argmax(dim=1)) and (lab == 1).sum().item() == B
    mrr, rec = tr.train_metrics(logits, lab)
    assert 0.0 <= mrr <= 1.0 and 0.0 <= rec <= 1.0


def test_constructor_refusals_name_the_option():
    model = D._model(0)
    for kw, word in ((dict(loss="ranknet", label_source="teacher"), "label_source"), (dict(loss="lambda_mrr", weighing_scheme="ndcgLoss1_scheme"), "weighing_scheme"),
                     (dict(loss="lambda_loss", neg_score_mode="mean"), "neg_score_mode"),
                     (dict(loss="lambda_loss", label_source="teacher", neg_score_mode="mean"), "n_rel"),
                     (dict(loss="lambda_loss", weighing_scheme="ndcg"), "weighing_scheme"), (dict(loss="lambda_loss", lambda_k=-1), "lambda_k")):
        with pytest.raises(ValueError, match=word):
            NwayTrainer(model, **kw)
    tr = NwayTrainer(model, loss="lambda_loss", label_source="teacher")
    with pytest.raises(ValueError, match="teacher_scores"):
        tr.train_step(syn.nway_batch(5, 2, 4, 8, 16, vocab=512, label_kind="mode9"))


def test_graph_replay_of_the_lambda_step_equals_the_eager_step(monkeypatch):
    """tests/test_gpu_distill.py::test_graph_replay_of_the_distilling_step_equals_the_eager_step with the teacher scores as the LABELS of
    lambda_loss, different every step: loss, logits and every gradient outside the embedding tables bit for bit.  Teacher scores baked into
    the captured graph would give the first captured batch's loss on every replay."""
    cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=64,
                        dropout=0.1, attention_dropout=0.1)
    monkeypatch.setenv("CLDRD_GRAPH", "1")
    torch.manual_seed(0)
    model = NwayDualEncoder(cfg, share_weights=False).cuda().train()
    with torch.no_grad():
        for seed, tower in ((11, model.query_encoder), (12, model.passage_encoder)):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed, name, tuple(p.shape), std=0.05, perturb=True))
    tr = NwayTrainer(model, loss="lambda_loss", learning_rate=3e-3, warmup_steps=5, total_steps=40, weighing_scheme="ndcgLoss1_scheme",
                     label_source="teacher", neg_score_mode="mean", teacher_label_shift="row_min", n_rel=2)
    towers = model.towers()
    keep = D._not_embedding(tr)

    def snapshot():
        return (tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.global_step, tr.adam_step, [t.step_seed for t in towers])

    def restore(sn):
        tr.flat_p.copy_(sn[0]); tr.m.copy_(sn[1]); tr.v.copy_(sn[2])
        tr.global_step, tr.adam_step = sn[3], sn[4]
        for t, ss in zip(towers, sn[5]):
            t.step_seed = ss
            t.refresh_shadows(need_transposed=True)

    replays, losses = 0, []
    for i in range(11):
        shape = (3, 4, 8, 16) if i != 8 else (2, 3, 8, 16)
        batch = D._dev(syn.nway_batch(100 + i, *shape, vocab=cfg.vocab_size, ragged=True, label_kind="mode9", with_teacher_scores=True))
        assert len(tr._step_inputs(batch)) <= 8 and sum(w == ("teacher_scores",) for w, _, _ in tr._step_inputs(batch)) == 1
        sn = snapshot()
        monkeypatch.setenv("CLDRD_GRAPH", "1")
        l1 = tr.train_step(batch).clone()
        lg1, g1, p1 = tr.last_logits.clone(), tr.flat_g.clone(), tr.flat_p.clone()
        key = tr._batch_key(batch)
        replayed = key in getattr(tr, "_graphs", {}) and tr._graphs[key]["graph"] is not None
        replays += int(replayed)
        restore(sn)
        state, ptrs = tr._state, [getattr(t, "seed_base_ptr", None) for t in towers]
        tr._state = None
        for t in towers:
            t.seed_base_ptr = None
        monkeypatch.setenv("CLDRD_GRAPH", "0")
        l0 = tr.train_step(batch).clone()
        tr._state = state
        for t, pp in zip(towers, ptrs):
            t.seed_base_ptr = pp
        torch.cuda.synchronize()
        assert torch.equal(l1, l0), (i, replayed, l1, l0)
        assert torch.equal(lg1, tr.last_logits), (i, replayed)
        assert torch.equal(g1[keep], tr.flat_g[keep]), (i, replayed)
        ge = (g1[~keep] - tr.flat_g[~keep]).abs().max().item()
        assert ge <= 1e-5 * max(1.0, g1[~keep].abs().max().item()), (i, ge)
        assert (p1 - tr.flat_p).abs().max().item() <= 1e-6, i
        # the loss is this step's: lambda_loss of the returned logits under THIS batch's teacher scores
        assert l1[0].item() == pytest.approx(_oracle_loss(tr, lg1, batch, shape[1]), rel=3e-5, abs=1e-6), (i, replayed)
        losses.append(l1[0].item())
    assert replays >= 6, replays
    assert len(set(losses)) == len(losses)
    assert tr.global_step == tr.adam_step == 11


def test_deterministic_runs_end_in_equal_parameters_and_moments():
    ends = []
    for _ in range(2):
        tr = NwayTrainer(D._model(0), loss="lambda_loss", learning_rate=1e-3, warmup_steps=0, total_steps=100, deterministic=True,
                         weighing_scheme="ndcgLoss1_scheme", label_source="teacher", teacher_label_shift="row_min")
        for i in range(6):
            tr.train_step(D._dev(syn.nway_batch(300 + i, 4, 6, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True)))
        torch.cuda.synchronize()
        ends.append((tr.flat_p.clone(), tr.m.clone(), tr.v.clone()))
    for a, b in zip(*ends):
        assert torch.equal(_bits(a), _bits(b))
    assert ends[0][1].abs().max().item() > 0


@pytest.mark.parametrize("source", ["rank", "teacher"])
def test_lambda_loss_learns(source):
    """dropout as configured, one fixed batch, 30 steps: the loss after the last step is below its value at the first."""
    batch = D._dev(syn.nway_batch(4680, 4, 6, 8, 24, vocab=512, ragged=True, label_kind="mode9", with_teacher_scores=True))
    kw = dict(label_source="teacher", neg_score_mode="mean", teacher_label_shift="row_min", n_rel=2) if source == "teacher" else {}
    tr = NwayTrainer(D._model(0), loss="lambda_loss", learning_rate=1e-3, warmup_steps=0, total_steps=1000, weighing_scheme="ndcgLoss1_scheme", **kw)
    losses = [tr.train_step(batch)[0].item() for _ in range(30)]
    print(f"lambda_loss ({source} labels): {losses[0]:.6g} at the first step, {losses[-1]:.6g} after 30")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------------------ end to end
def test_teacher_run_to_scored_file_to_lambda_trainer_end_to_end(tmp_path):
    """The command lines of tests/test_gpu_distill.py's end-to-end test (same tiny models and corpus) with the reference's ndcg script as
    ours: ``--loss lambda_loss --weighing_scheme ndcgLoss1_scheme --label_source teacher --neg_score_mode mean``, to a checkpoint."""
    from cldrd_amd.dataset import curriculum_file as C
    from cldrd_amd.retriever import index_text, rerank_top_passages, retrieve_top_passages
    from cldrd_amd.trainer import nway_listwise as T
    from test_rerank_host import make_pair_tokenizer, words
    import selftest
    N_P, N_Q, TOP = D.N_P, D.N_Q, D.TOP
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
        "--model_name_or_path", D._teacher(tmp_path, tok.vocab_size + 4), "--tokenizer_name_or_path", tok_dir, "--max_len", "64",
        "--output_path", str(teacher_run)]))
    train_path = tmp_path / "train.10relT_20neg.scored.json"
    n, skipped = C.main(C.get_args(["--run_path", str(teacher_run), "--label_mode", "9", "--output_path", str(train_path),
                                    "--most_hard_ranks", "11:30", "--semi_hard_ranks", "31:60", "--seed", "5", "--with_scores"]))
    assert (n, skipped) == (N_Q, 0)
    args = T.set_env(T.get_args([
        "--experiment_folder", str(tmp_path), "--run_folder", "ndcg", "--queries_path", str(q_path), "--collection_path", str(c_path),
        "--training_path", str(train_path), "--label_mode", "9", "--model_name_or_path", str(mdir), "--model_checkpoint", str(ckpt),
        "--tokenizer_name_or_path", tok_dir, "--query_max_len", "16", "--passage_max_len", "32", "--train_batch_size", "4",
        "--logging_steps", "1", "--evaluate_steps", "4", "--warmup_steps", "1", "--num_train_epochs", "2", "--learning_rate", "1e-3",
        "--loader_workers", "2", "--loss", "lambda_loss", "--weighing_scheme", "ndcgLoss1_scheme", "--label_source", "teacher",
        "--neg_score_mode", "mean", "--teacher_label_shift", "row_min"]))
    tr = T.train(args)
    assert tr.loss_kind == "lambda_loss" and tr.label_source == "teacher" and tr.distill is None
    assert tr._lambda_kw["n_rel"] == 10 and tr._lambda_kw["neg_mean"] and tr._lambda_kw["row_min"]
    assert tr.global_step == 2 * N_Q // 4 and tr.skipped_steps() == 0
    assert torch.isfinite(tr.flat_p).all().item()
    log = (tmp_path / "ndcg" / "log" / "train_logs.log").read_text().splitlines()
    header = log[0].split("\t")
    assert "kd_loss" not in header                                   # kd_loss logging is the distillation term's, unchanged
    losses = [float(line.split("\t")[2]) for line in log[1:]]
    assert len(losses) == tr.global_step - 1 and np.isfinite(losses).all() and min(losses) > 0.0
    assert os.path.exists(tmp_path / "ndcg" / "models" / f"checkpoint_{tr.global_step}.pth.tar")
