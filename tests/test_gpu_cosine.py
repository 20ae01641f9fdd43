"""Cosine-similarity scoring on the GPU: the scorer and its backward against float64, exact scale invariance, bit reproducibility, the
autograd op, row normalisation, one training step against the oracle towers, deterministic replay == eager, and the command lines end to end
(train with --apply_consine_similarity, index, retrieve, re-rank, validate).

The bar of the kernel tests: the formulas of the issue evaluated in fp32 with torch on the CPU are some distance from their float64 evaluation;
the kernel may be at most 4 times as far, and never has to be closer than 8 fp32 ulps of the tensor's largest magnitude.  A different
summation order passes, a wrong term does not."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
import cldrd_amd.synthetic as syn
import selftest
from cldrd_amd import hip_ops as ops
from cldrd_amd.models import NwayDualEncoder
from cldrd_amd.trainer import NwayTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-8


def _cols(B, N, mode):
    return N if mode == 0 else (B * N if mode == 1 else 2 * N)


def passage_index(B, N, mode):
    """int64 [B, N']: the passage row behind logit column j of query b (reference models/nway_dual_encoder.py:30-44)."""
    rows = []
    for b in range(B):
        own = list(range(b * N, (b + 1) * N))
        if mode == 1:
            own += [m for m in range(B * N) if m // N != b]
        elif mode == 2:
            nb = (b + 1) % B
            own += list(range(nb * N, (nb + 1) * N))
        rows.append(own)
    return torch.tensor(rows, dtype=torch.int64)


def restate(q, p, g, B, N, mode, scale, dtype):
    """The issue's formulas in ``dtype`` on the CPU -> (logits, dq, dp)."""
    q, p, g = q.to(dtype), p.to(dtype), g.to(dtype)
    idx = passage_index(B, N, mode)
    nq, npn = (q * q).sum(1).sqrt(), (p * p).sum(1).sqrt()
    iq, ip = 1.0 / nq.clamp_min(EPS), 1.0 / npn.clamp_min(EPS)
    P, ipj = p[idx], ip[idx]                                                   # [B, N', d], [B, N']
    logits = scale * (q[:, None, :] * P).sum(-1) * iq[:, None] * ipj
    live_q, live_p = (nq > EPS).to(dtype), (npn > EPS).to(dtype)
    dq = iq[:, None] * (scale * ((g * ipj)[:, :, None] * P).sum(1) - (g * logits).sum(1, keepdim=True) * iq[:, None] * q * live_q[:, None])
    A = torch.zeros_like(p).index_add_(0, idx.reshape(-1), ((g * iq[:, None])[:, :, None] * q[:, None, :]).reshape(-1, q.shape[1]))
    S = torch.zeros(p.shape[0], dtype=dtype).index_add_(0, idx.reshape(-1), (g * logits).reshape(-1))
    dp = ip[:, None] * (scale * A - S[:, None] * ip[:, None] * p * live_p[:, None])
    return logits, dq, dp


def autograd64(q, p, g, B, N, mode, scale):
    q, p = q.double().requires_grad_(True), p.double().requires_grad_(True)
    logits = scale * F.cosine_similarity(q[:, None, :], p[passage_index(B, N, mode)], dim=-1, eps=EPS)
    logits.backward(g.double())
    return logits.detach(), q.grad, p.grad


def run_kernels(q, p, g, B, N, mode, scale):
    qd, pd, gd = q.to(DEV), p.to(DEV), g.to(DEV)
    logits = torch.empty(B, _cols(B, N, mode), dtype=torch.float32, device=DEV)
    inv = torch.empty(B + B * N, dtype=torch.float32, device=DEV)
    ops.score_cos_fwd(qd, pd, logits, inv, B, N, mode, scale)
    dq, dp = torch.empty_like(qd), torch.empty_like(pd)
    ops.score_cos_bwd(gd, logits, qd, pd, inv, dq, dp, B, N, mode, scale)
    torch.cuda.synchronize()
    return logits.cpu(), dq.cpu(), dp.cpu()


def inputs(seed, B, N, d, mode):
    gen = torch.Generator().manual_seed(seed)
    common = torch.randn(1, d, generator=gen)                  # CLS-like: a common component
    q = (common + torch.randn(B, d, generator=gen)).contiguous()
    p = (common + torch.randn(B * N, d, generator=gen)).contiguous()
    g = torch.randn(B, _cols(B, N, mode), generator=gen).contiguous()
    return q, p, g


def check_against_float64(name, q, p, g, B, N, mode, scale, with_autograd):
    ref = restate(q, p, g, B, N, mode, scale, torch.float64)
    cpu32 = restate(q, p, g, B, N, mode, scale, torch.float32)
    got = run_kernels(q, p, g, B, N, mode, scale)
    refs = [ref] + ([autograd64(q, p, g, B, N, mode, scale)] if with_autograd else [])
    for what, g_, c_, *rs in zip(("logits", "dq", "dp"), got, cpu32, *refs):
        for which, r_ in zip(("formulas", "autograd"), rs):
            d_cpu = float((c_.double() - r_).abs().max())
            d_gpu = float((g_.double() - r_).abs().max())
            floor = 8.0 * float(np.spacing(np.float32(r_.abs().max())))
            print(f"cosine_parity {name} {what} vs float64 {which}: kernel {d_gpu:.3e} cpu-fp32 {d_cpu:.3e} bar {max(4.0 * d_cpu, floor):.3e}")
            assert d_gpu <= max(4.0 * d_cpu, floor), (name, what, which, d_gpu, d_cpu, floor)
    if with_autograd:            # the restated formulas ARE the derivative of scale * cosine_similarity
        for a, b in zip(ref, refs[1]):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ 1. scorer against float64
@pytest.mark.parametrize("scale", [1.0, 20.0])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,N,d", [(1, 1, 4), (3, 5, 128), (2, 3, 260), (2, 32, 768)])
def test_scorer_against_float64(B, N, d, mode, scale):
    q, p, g = inputs(1000 + 7 * B + N + d + mode, B, N, d, mode)
    check_against_float64(f"B{B}_N{N}_d{d}_mode{mode}_s{scale:g}", q, p, g, B, N, mode, scale, with_autograd=True)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d", [4, 260])
@pytest.mark.parametrize("N", [1, 5, 11])
@pytest.mark.parametrize("B", [1, 3])
def test_scorer_tails_in_every_mode(B, N, d, mode):
    """Column counts of 1 to 33 (a tail alone, eight plus a tail, four times eight plus one; B = 1 and 3 close the cycle of mode 2 on the
    row itself and on another row) and d of one float4 and of a second pass of the 256-wide loop."""
    q, p, g = inputs(2000 + 100 * B + 7 * N + d + mode, B, N, d, mode)
    check_against_float64(f"tails_B{B}_N{N}_d{d}_mode{mode}", q, p, g, B, N, mode, 20.0, with_autograd=False)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("zero", ["passage", "query"])
def test_scorer_with_a_clamped_row(zero, mode):
    """An all-zero row: its norm is clamped to eps and is a constant there - its logits are 0 and the second term of its gradient is dropped."""
    B, N, d, scale = 3, 5, 128, 20.0
    q, p, g = inputs(77 + mode, B, N, d, mode)
    if zero == "passage":
        p[7] = 0.0
    else:
        q[1] = 0.0
    check_against_float64(f"zero_{zero}_mode{mode}", q, p, g, B, N, mode, scale, with_autograd=False)
    logits, dq, dp = run_kernels(q, p, g, B, N, mode, scale)
    idx = passage_index(B, N, mode)
    if zero == "passage":
        assert (logits[idx == 7] == 0).all() and torch.isfinite(dp).all() and float(dp[7].abs().max()) > 0
    else:
        assert (logits[1] == 0).all() and torch.isfinite(dq).all() and float(dq[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. scale invariance, exact
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scaling_the_rows_by_powers_of_two_is_exact(mode):
    B, N, d, scale = 3, 5, 128, 20.0
    q, p, g = inputs(5 + mode, B, N, d, mode)
    l0, dq0, dp0 = run_kernels(q, p, g, B, N, mode, scale)
    l1, dq1, dp1 = run_kernels(q * 4.0, p * 0.5, g, B, N, mode, scale)
    assert torch.equal(l0, l1)
    assert torch.equal(dq1, dq0 * 0.25) and torch.equal(dp1, dp0 * 2.0)
    assert float(l0.abs().max()) <= scale * (1 + 1e-6) and float(dq0.abs().max()) > 0 and float(dp0.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. two calls, equal bits
def test_two_calls_give_the_same_bits():
    B, N, d, mode = 4, 8, 128, 1
    q, p, g = inputs(31, B, N, d, mode)
    a = run_kernels(q, p, g, B, N, mode, 20.0)
    b = run_kernels(q, p, g, B, N, mode, 20.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 4. autograd
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_autograd_op_equals_the_raw_pair(mode):
    B, N, d, scale = 3, 4, 128, 20.0
    q, p, g = inputs(9 + mode, B, N, d, mode)
    want = run_kernels(q, p, g, B, N, mode, scale)
    qd, pd = q.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    logits = torch.ops.cldrd.nway_score_cos(qd, pd, B, N, mode, scale)
    logits.backward(g.to(DEV))
    assert torch.equal(logits.detach().cpu(), want[0]) and torch.equal(qd.grad.cpu(), want[1]) and torch.equal(pd.grad.cpu(), want[2])
    torch.library.opcheck(torch.ops.cldrd.nway_score_cos, (q.to(DEV), p.to(DEV), B, N, mode, scale), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(Exception):
        torch.ops.cldrd.nway_score_cos(q, p, B, N, mode, scale)               # CPU tensors: no kernel, no fall-back


# ------------------------------------------------------------------------------------------------ 5. l2_normalize_rows
@pytest.mark.parametrize("layout", ["dense", "strided", "in_place"])
@pytest.mark.parametrize("d", [4, 128, 768])
@pytest.mark.parametrize("n", [1, 5, 513])
def test_l2_normalize_rows(n, d, layout):
    gen = torch.Generator().manual_seed(100 * n + d)
    x = (torch.randn(n, d, generator=gen) * torch.rand(n, 1, generator=gen) * 30.0 + 0.5).contiguous()
    if n > 1:
        x[n // 2] = 0.0                                         # a zero row stays zero
    ref = x.double() / (x.double() * x.double()).sum(1, keepdim=True).sqrt().clamp_min(EPS)
    if layout == "strided":
        buf = torch.full((n, d + 4), 7.0, device=DEV)
        buf[:, :d] = x.to(DEV)
        src = buf[:, :d]
        assert src.stride(0) == d + 4
        out = ops.l2_normalize_rows(src, torch.empty(n, d, device=DEV))
        assert torch.equal(buf[:, :d].cpu(), x) and (buf[:, d:] == 7.0).all()          # the source is untouched
    elif layout == "in_place":
        src = x.to(DEV)
        out = ops.l2_normalize_rows(src)
        assert out.data_ptr() == src.data_ptr()
    else:
        src = x.to(DEV)
        out = ops.l2_normalize_rows(src, torch.empty(n, d, device=DEV))
        assert torch.equal(src.cpu(), x)
    got = out.cpu()
    ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))
    assert ((got.double() - ref).abs() <= ulp).all(), float(((got.double() - ref).abs() / ulp).max())
    norms = (got.double() * got.double()).sum(1).sqrt()
    live = (x.abs().sum(1) > 0)
    assert ((norms[live] - 1.0).abs() <= 2.0 ** -22).all(), float((norms[live] - 1.0).abs().max())
    if n > 1:
        assert (got[n // 2] == 0).all()
    if n == 1:
        z = ops.l2_normalize_rows(torch.zeros(1, d, device=DEV), torch.full((1, d), 3.0, device=DEV))
        assert (z == 0).all()


# ------------------------------------------------------------------------------------------------ 6. one training step against the oracle
def _cosine_model(cfg, scale=20.0, seed=3, std=0.1, **kw):
    """selftest.build_tiny_model with the cosine scorer"""
    model = NwayDualEncoder(cfg, share_weights=False, cosine=True, cosine_scale=scale, **kw)
    with torch.no_grad():
        for ti, tower in enumerate(model.towers()):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed + ti, name, tuple(p.shape), std=std, perturb=True))
    return model


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def test_one_training_step_against_the_oracle_towers():
    """tests/test_gpu_model.py: test_small_model_forward_backward_vs_oracle (distilbert, margin_mse) with cosine=True, cosine_scale=20: the
    oracle's towers in float64, its scoring line replaced by 20 * F.cosine_similarity; that test's bars."""
    from oracle import encoder_ref as E
    from oracle import losses_ref as LR
    from test_gpu_model import small_cfg
    cfg = small_cfg("distilbert")
    model = _cosine_model(cfg).cuda()
    model.train()
    batch = syn.nway_batch(4680, 3, 5, 10, 40, vocab=cfg.vocab_size, ragged=True, label_kind="teacher")
    qp, pp = ({k: v.double().requires_grad_(True) for k, v in d_.items()} for d_ in selftest.oracle_params(model))
    ocfg = selftest.oracle_cfg(cfg)
    ref = 20.0 * F.cosine_similarity(E.cls_embs(qp, ocfg, batch["query"]).unsqueeze(1), E.nway_passage_embs(pp, ocfg, batch["nway_passages"]),
                                     dim=-1, eps=EPS)
    assert ref.dtype == torch.float64
    ref_logits = ref.detach().numpy()
    ref_loss, dl = LR.margin_mse(ref_logits, batch["labels"].numpy())
    ref.backward(torch.from_numpy(np.asarray(dl)).double())
    tr = NwayTrainer(model, loss="margin_mse", learning_rate=1e-3, warmup_steps=0, total_steps=100)
    assert tr.cosine and tr.cosine_scale == 20.0
    loss_out, logits = tr.forward_backward(batch)
    torch.cuda.synchronize()
    got = logits.cpu().numpy()
    scale = np.abs(ref_logits).max()
    print(f"cosine step: logits off {np.abs(got - ref_logits).max() / scale:.3e} of max |logit| {scale:.3f}; loss {loss_out[0].item():.5f} oracle {ref_loss:.5f}")
    assert np.abs(got).max() <= 20.0 * (1 + 1e-6)
    assert np.abs(got - ref_logits).max() <= 2e-2 * scale, f"logits off: {np.abs(got - ref_logits).max() / scale:.3e}"
    assert loss_out[0].item() == pytest.approx(ref_loss, rel=5e-2, abs=1e-3)
    checked = 0
    for tname, tower, ref_params in (("query_encoder", model.query_encoder, qp), ("passage_encoder", model.passage_encoder, pp)):
        tower.ensure_grads()
        all_g, all_r = [], []
        for name, p in tower.named_flat():
            gg, rr = p.grad.detach().cpu().numpy(), ref_params[name].grad.numpy()
            all_g.append(gg.ravel()), all_r.append(rr.ravel())
            if np.linalg.norm(rr) > 1e-3 * max(1.0, ref_loss):          # skip analytically-zero grads (k bias)
                thr = 0.99 if "token_type" in name else 0.995
                checked += 1
                assert _cos(gg, rr) > thr, f"{tname}.{name}: cosine {_cos(gg, rr):.5f}"
                assert np.linalg.norm(gg) == pytest.approx(np.linalg.norm(rr), rel=5e-2), f"{tname}.{name}"
        assert _cos(np.concatenate(all_g), np.concatenate(all_r)) > 0.999
    assert checked >= 20, checked
    # the reference-style loop takes the same scorer: model(...) gives the trainer's logits
    dev_batch = {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    assert torch.equal(model(dev_batch["query"], dev_batch["nway_passages"]).detach(), logits)


# ------------------------------------------------------------------------------------------------ 7. deterministic: replay == eager
@pytest.mark.parametrize("packed,in_batch", [(False, False), (True, False), (False, True)])
def test_deterministic_replayed_steps_equal_an_all_eager_run(packed, in_batch, monkeypatch):
    """fp16 mode, --deterministic: three eager steps, the capture and replays (a packed batch changes its row count every step and stays
    eager) against a run that never captures: parameters and both moments bit for bit."""
    from test_gpu_deterministic import _ragged, small_cfg
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    ends = []
    for graph in ("1", "0"):
        monkeypatch.setenv("CLDRD_GRAPH", graph)
        cfg = small_cfg()
        torch.manual_seed(0)
        model = _cosine_model(cfg, seed=11, std=0.05, in_batch_loss=in_batch, all_in_batch_neg=True).cuda().train()
        tr = NwayTrainer(model, loss="kl_div" if not in_batch else "lambda_mrr", learning_rate=3e-3, warmup_steps=5, total_steps=40,
                         deterministic=True)
        assert tr.cosine and tr.amp16
        for i in range(8):
            tr.train_step(_ragged(cfg, 300 + i, 3, 4, 8, 16, packed))
        torch.cuda.synchronize()
        assert bool(tr._graphs) == (graph == "1" and not packed)
        assert torch.isfinite(tr.flat_p).all().item() and float(tr.m.abs().max()) > 0
        ends.append((tr.flat_p.clone(), tr.m.clone(), tr.v.clone()))
    for a, b, name in zip(ends[0], ends[1], ("flat_p", "m", "v")):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ 8. the command lines end to end
N_P, Q_LEN, P_LEN = 120, 16, 48
DEV_RUN = {501: [9007], 502: [9011, 9007, 9040, 9003], 503: [9090, 9007, 9001, 9002, 9005, 9006, 9008, 9009, 9010],
           504: [9100, 9000], 505: [9055, 9056, 9057, 9058, 9059, 9060], 506: [9070, 9071, 9072]}
QRELS = {501: [9007], 502: [9040], 503: [9005, 9010], 504: [9119], 506: [9071]}


def _read_run(path):
    """{(qid, pid): score string}, {qid: [pid in file order]}"""
    scores, order = {}, {}
    for line in open(path).read().splitlines():
        q, p, _, s = line.split("\t")
        scores[(int(q), int(p))] = s
        order.setdefault(int(q), []).append(int(p))
    return scores, order


def test_command_lines_end_to_end(tmp_path):
    from cldrd_amd.dataset import SequenceDataset
    from cldrd_amd.evaluation import continue_rerank_evaluator as C
    from cldrd_amd.retriever import build_stage_file as B, index_text as I, rerank_top_passages as R, retrieve_top_passages as S
    from cldrd_amd.retriever.retrieval_utils import get_embeddings_from_scratch, read_index
    from cldrd_amd.trainer import nway_listwise as T
    from test_rerank_host import make_pair_tokenizer, words
    rng = np.random.default_rng(77)
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    plens = rng.integers(3, 39, N_P)
    collection, dev_q, dev_run, qrels = (str(tmp_path / n) for n in ("collection.tsv", "queries.dev.tsv", "dev.run.tsv", "qrels.dev.tsv"))
    open(collection, "w").write("".join(f"{9000 + j}\t{words(int(plens[j]), 5 * j)}\n" for j in range(N_P)))
    open(dev_q, "w").write("".join(f"{q}\t{words(1 + i, 7 * i)}\n" for i, q in enumerate(DEV_RUN)))
    open(dev_run, "w").write("".join(f"{q}\t{p}\t{r + 1}\t{10.0 - r}\n" for q, ps in DEV_RUN.items() for r, p in enumerate(ps)))
    open(qrels, "w").write("".join(f"{q}\t0\t{p}\t1\n" for q, ps in QRELS.items() for p in ps))
    n_q = 16
    q_path, train_path = tmp_path / "queries.train.tsv", tmp_path / "train.10relT_20neg.json"
    q_path.write_text("".join(f"{3000 + i}\t{words(int(rng.integers(2, 7)), 3 * i)}\n" for i in range(n_q)))
    with open(train_path, "w") as fh:
        for i in range(n_q):
            pids = (9000 + rng.choice(N_P, 30, replace=False)).tolist()
            fh.write(json.dumps({"qid": 3000 + i, "relT_pids": pids[:10], "most_hard_pids": pids[10:20], "semi_hard_pids": pids[20:]}) + "\n")
    student = selftest.build_tiny_model(selftest.tiny_config(), std=0.05)
    mdir = str(tmp_path / "student")
    student.query_encoder.save_pretrained(mdir)
    ckpt0 = tmp_path / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt0)

    # -- train with the flag, a few steps, with a dev run
    tr = T.train(T.set_env(T.get_args([
        "--experiment_folder", str(tmp_path), "--run_folder", "cos", "--queries_path", str(q_path), "--collection_path", collection,
        "--training_path", str(train_path), "--label_mode", "9", "--model_name_or_path", mdir, "--model_checkpoint", str(ckpt0),
        "--tokenizer_name_or_path", tok_dir, "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN), "--train_batch_size", "4",
        "--logging_steps", "4", "--evaluate_steps", "4", "--warmup_steps", "1", "--num_train_epochs", "2", "--learning_rate", "1e-3",
        "--loader_workers", "0", "--apply_consine_similarity", "--cosine_scale", "20",
        "--dev_path", dev_run, "--dev_queries_path", dev_q, "--dev_qrels_path", qrels])))
    assert tr.global_step == 8 and tr.cosine and tr.cosine_scale == 20.0 and float(tr.last_logits.abs().max()) <= 20.0 * (1 + 1e-6)
    run_dir = tmp_path / "cos"
    ckpt_path = str(run_dir / "models" / "checkpoint_8.pth.tar")
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    want_score = {"kind": "cosine", "scale": 20.0, "eps": 1e-8}
    assert ckpt["score"] == want_score and ckpt["resume_state"]["score"] == want_score
    dot_ckpt = str(tmp_path / "dot" / "checkpoint_8.pth.tar")          # the same weights as a dot-product checkpoint: no `score` key
    os.makedirs(os.path.dirname(dot_ckpt))
    torch.save({k: v for k, v in ckpt.items() if k != "score"}, dot_ckpt)

    # -- index_text with no flag: unit rows and the mark; the dot-product checkpoint: raw rows, no mark.  (--fp32_encode: the batch-invariant pass)
    model_flags = ["--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir, "--fp32_encode"]
    unit_path = I.main(I.get_args(model_flags + ["--resume", ckpt_path, "--passages_path", collection, "--index_dir", str(tmp_path / "unit"),
                                                 "--max_length", str(P_LEN)]))
    raw_path = I.main(I.get_args(model_flags + ["--resume", dot_ckpt, "--passages_path", collection, "--index_dir", str(tmp_path / "raw"),
                                                "--max_length", str(P_LEN)]))
    unit, raw = read_index(unit_path), read_index(raw_path)
    assert unit.normalized is True and raw.normalized is False and unit.ntotal == raw.ntotal == N_P
    rows, raw_rows = np.asarray(unit.embeddings, dtype=np.float64), np.asarray(raw.embeddings, dtype=np.float64)
    assert (np.abs(np.linalg.norm(rows, axis=1) - 1.0) <= 2.0 ** -22).all()
    assert np.abs(np.linalg.norm(raw_rows, axis=1) - 1.0).min() > 1e-3                     # the CLS rows themselves are no unit vectors
    pid_row = {int(p): i for i, p in enumerate(np.asarray(raw.ids).tolist())}

    # -- retrieve with no flag: plain cosines of the raw CLS rows
    run_unit = str(tmp_path / "dev.cos.run.tsv")
    S.main(S.get_args(model_flags + ["--resume", ckpt_path, "--queries_path", dev_q, "--index_path", unit_path, "--max_length", str(Q_LEN),
                                     "--top_k", str(N_P), "--output_path", run_unit]))
    dot_model = NwayDualEncoder(mdir, share_weights=False)
    I.load_checkpoint_into(dot_model, dot_ckpt)
    dot_model.cuda()
    ds = SequenceDataset.create_from_seqs_file(dev_q, tok, Q_LEN, is_query=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=512, shuffle=False, collate_fn=ds.collate_fn)
    q_raw, q_ids = get_embeddings_from_scratch(dot_model, loader, use_fp16=False, is_query=True)
    assert q_ids == list(DEV_RUN) and np.abs(np.linalg.norm(q_raw, axis=1) - 1.0).min() > 1e-3
    q64 = q_raw.astype(np.float64)
    ref = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (raw_rows / np.linalg.norm(raw_rows, axis=1, keepdims=True)).T       # [nq, N_P]
    q32, p32 = torch.from_numpy(q_raw), torch.from_numpy(np.asarray(raw.embeddings, dtype=np.float32))
    cpu32 = ((q32 / (q32 * q32).sum(1, keepdim=True).sqrt().clamp_min(EPS)) @ (p32 / (p32 * p32).sum(1, keepdim=True).sqrt().clamp_min(EPS)).T).numpy()
    d_cpu = float(np.abs(cpu32.astype(np.float64) - ref).max())
    bar = max(4.0 * d_cpu, 8.0 * float(np.spacing(np.float32(np.abs(ref).max()))))
    scores, order = _read_run(run_unit)
    assert len(scores) == len(DEV_RUN) * N_P
    d_gpu = max(abs(float(s) - ref[q_ids.index(q), pid_row[p]]) for (q, p), s in scores.items())
    print(f"cosine_parity retrieve scores vs float64 cosine of the raw CLS rows: search {d_gpu:.3e} cpu-fp32 {d_cpu:.3e} bar {bar:.3e}")
    assert d_gpu <= bar and max(abs(float(s)) for s in scores.values()) <= 1.0 + bar
    pids = np.asarray(raw.ids)
    for qi, q in enumerate(q_ids):
        by = np.argsort(-ref[qi], kind="stable")
        s = ref[qi][by]
        for r in range(N_P):
            if (r == 0 or s[r - 1] - s[r] > 2 * bar) and (r == N_P - 1 or s[r] - s[r + 1] > 2 * bar):
                assert order[q][r] == int(pids[by[r]]), (q, r)

    # -- the dev_logs.log rows are what the student mode of rerank_top_passages and continue_rerank_evaluator give for the checkpoints (no flag)
    from cldrd_amd.evaluation import RerankingEvaluator
    log = (run_dir / "log" / "dev_logs.log").read_text().splitlines()
    header = log[0].split("\t")
    metric_keys = header[2:-1]
    row8 = dict(zip(header, log[2].split("\t")))
    assert (row8["epoch"], row8["step"]) == ("2", "8")
    common = ["--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir, "--queries_path", dev_q, "--collection_path", collection,
              "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN)]
    rerank = str(tmp_path / "dev.rerank.step8.tsv")
    R.main(R.get_args(["--dual_encoder", "--resume", ckpt_path, "--run_path", dev_run, "--output_path", rerank] + common))
    r_scores, r_order = _read_run(rerank)
    assert max(abs(float(s)) for s in r_scores.values()) <= 1.0 + 1e-6                    # plain cosines: the scale is not applied
    m8 = RerankingEvaluator(qrels).direct_compute_metric(r_order)
    assert {k: float(m8[k]) for k in metric_keys} == {k: float(row8[k]) for k in metric_keys}
    table = tmp_path / "continue.log"
    C.main(C.get_args(["--resume_folder", str(run_dir / "models"), "--dev_path", dev_run, "--dev_queries_path", dev_q, "--dev_qrels_path", qrels,
                       "--collection_path", collection, "--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir,
                       "--query_max_len", str(Q_LEN), "--passage_max_len", str(P_LEN), "--output_path", str(table)]))
    log2 = table.read_text().splitlines()
    assert log2[0] == log[0] and [ln.split("\t")[:-1] for ln in log2[1:]] == [ln.split("\t")[:-1] for ln in log[1:]]
    # the same weights as a dot-product checkpoint, with the program's own flag: the cosine model again
    rerank_flag = str(tmp_path / "dev.rerank.flag.tsv")
    R.main(R.get_args(["--dual_encoder", "--resume", dot_ckpt, "--run_path", dev_run, "--output_path", rerank_flag,
                       "--apply_cosine_similarity"] + common))
    assert open(rerank_flag).read() == open(rerank).read()

    # -- a validation score IS the flat search's score of the pair (both through the batch-invariant fp32 pass)
    rerank32 = str(tmp_path / "dev.rerank.fp32.tsv")
    R.main(R.get_args(["--dual_encoder", "--resume", ckpt_path, "--run_path", dev_run, "--output_path", rerank32, "--fp32_encode"] + common))
    v_scores, _ = _read_run(rerank32)
    assert len(v_scores) == sum(len(v) for v in DEV_RUN.values())
    for pair, s in v_scores.items():
        assert np.float32(float(s)).view(np.uint32) == np.float32(float(scores[pair])).view(np.uint32), pair

    # -- the index of unit rows under a dot-product model: an ordinary search; a cosine model on the raw index: refused before any encoding
    S.main(S.get_args(model_flags + ["--resume", dot_ckpt, "--queries_path", dev_q, "--index_path", unit_path, "--max_length", str(Q_LEN),
                                     "--top_k", "10", "--output_path", str(tmp_path / "dev.dot_on_unit.tsv")]))
    assert len(_read_run(str(tmp_path / "dev.dot_on_unit.tsv"))[0]) == 10 * len(DEV_RUN)
    calls = []
    import cldrd_amd.retriever.retrieval_utils as RU
    real = RU._embeddings_from_scratch
    try:
        RU._embeddings_from_scratch = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        for resume, flag in ((ckpt_path, []), (dot_ckpt, ["--apply_consine_similarity"])):
            with pytest.raises(ValueError, match="raw rows.*rebuil"):
                S.main(S.get_args(model_flags + flag + ["--resume", resume, "--queries_path", dev_q, "--index_path", raw_path,
                                                        "--max_length", str(Q_LEN), "--top_k", "10", "--output_path", str(tmp_path / "no.dev.tsv")]))
            if flag:
                continue
            with pytest.raises(ValueError, match="raw rows.*rebuil"):
                B.main(B.get_args(flag + ["--resume", resume, "--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir,
                                          "--index_path", raw_path, "--queries_path", str(q_path), "--collection_path", collection,
                                          "--teacher_name_or_path", "unused", "--label_mode", "9", "--top_k", str(N_P),
                                          "--most_hard_ranks", "11:60", "--semi_hard_ranks", "61:120", "--output_path", str(tmp_path / "no.json")]))
    finally:
        RU._embeddings_from_scratch = real
    assert not calls and not os.path.exists(tmp_path / "no.dev.tsv") and not os.path.exists(tmp_path / "no.json")
