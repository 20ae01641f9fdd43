"""Head-dim-32 models end to end on the GPU (run with -m gpu): MiniLM-shaped cross-encoder teachers against HF fp32 on the CPU (16-bit pass and
fp32 pass, padded and cached), the MiniLM-L-6 shape against its head-dim-64 twin, batch invariance of score_cached at that shape, a head-dim-32
student tower through HipEncoder / NwayDualEncoder, the refusals of everything that would train, and the rerank_top_passages command line.

Set CLDRD_HD32_PARITY_OUT to a file name to get the measured ratios appended to it (profiles/hd32_parity.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import selftest
import cldrd_amd.synthetic as syn
from cldrd_amd.encoder import EncoderConfig, HipEncoder, encode_autograd
from cldrd_amd.models.cross_encoder import CrossEncoder
from oracle import encoder_ref as E
from test_gpu_rerank import TINY_BAR, _base_pairs, _hf_logits, _pairs, _save, _scores, _toy_files
from test_rerank_host import make_pair_tokenizer

pytestmark = pytest.mark.gpu


def _record(line):
    print(line)
    path = os.environ.get("CLDRD_HD32_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def _hf_model(arch, d, layers, nl, seed, heads, vocab=1000, ffn=None, init=None):
    """test_gpu_rerank._hf_model with the head count as an argument (there: d // 64)."""
    from transformers import BertConfig, BertForSequenceClassification, DistilBertConfig, DistilBertForSequenceClassification
    torch.manual_seed(seed)
    init = (0.05 if d < 384 else 0.02) if init is None else init          # small models: a wider init, see test_gpu_rerank._hf_model
    ffn = 4 * d if ffn is None else ffn
    if arch == "bert":
        cfg = BertConfig(vocab_size=vocab, hidden_size=d, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn,
                         max_position_embeddings=512, num_labels=nl, initializer_range=init)
        cls = BertForSequenceClassification
    else:
        cfg = DistilBertConfig(vocab_size=vocab, dim=d, n_layers=layers, n_heads=heads, hidden_dim=ffn, max_position_embeddings=512,
                               num_labels=nl, initializer_range=init)
        cls = DistilBertForSequenceClassification
    cfg._attn_implementation = "eager"
    m = cls(cfg).eval()
    with torch.no_grad():       # spread the classifier a little: random init gives logits of a few 1e-2
        m.classifier.weight.mul_(10.0)
    return m


# ---------------------------------------------------------------- tiny teachers against HF fp32
@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("arch,nl", [("bert", 1), ("bert", 2), ("distilbert", 1), ("distilbert", 2)])
def test_tiny_head_dim_32_teacher_matches_hf(arch, nl, amp, tmp_path, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", amp)
    hf = _hf_model(arch, 128, 2, nl, seed=7 + nl, heads=4)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m"), eval_only=True).cuda()
    assert model.cfg.head_dim == 32
    qc, pc, qr, pr = _pairs(3, 12, 40, 96, 1000, 256, 120)
    ref, batch = _hf_logits(hf, arch, qc, pc, qr, pr, 256)
    # passages of 256, 255, 3 and 2 tokens are among the pairs (_pairs puts them first); the longest pair fills the 256 tokens
    assert {256, 255, 3, 2} <= set(pc.lens[pr].tolist()) and int(batch["attention_mask"].sum(1).max()) == 256
    got = model(batch).cpu().numpy()
    spread = ref.max() - ref.min()
    err = np.abs(got - ref).max()
    sc = model.score_cached(qc, pc, qr, pr, 256).cpu().numpy()
    ref_s = _scores(ref, nl)
    err_c = np.abs(sc - ref_s).max()
    print(f"tiny head-dim-32 {arch} nl={nl} {amp}: max|dlogit| {err:.3e} = {err / spread:.2e} of the spread {spread:.3e}, "
          f"{err / np.abs(ref).max():.2e} of max|logit|; cached {err_c / (ref_s.max() - ref_s.min()):.2e} of the score spread")
    assert err <= TINY_BAR * np.abs(ref).max()
    assert err <= TINY_BAR * spread
    assert err_c <= TINY_BAR * (ref_s.max() - ref_s.min())


# ---------------------------------------------------------------- the MiniLM-L-6 shape against its head-dim-64 twin
_L6 = {}


def _l6(heads, tmp_path):
    """HF model, its fp32 logits and the saved directory of the MiniLM-L-6 shape with `heads` heads (12: head dim 32; 6: the head-dim-64 twin),
    on the same 64 pairs; computed once."""
    if "data" not in _L6:
        _L6["data"] = _pairs(9, 16, 80, 64, 30522, 256, 160)
    if heads not in _L6:
        torch.set_num_threads(16)
        hf = _hf_model("bert", 384, 6, 1, seed=21, heads=heads, vocab=30522, ffn=1536, init=0.02)
        ref, batch = _hf_logits(hf, "bert", *_L6["data"], 256)
        _L6[heads] = dict(ref=ref, batch=batch, path=_save(hf, tmp_path, f"l6h{heads}"))
    return _L6[heads]


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_minilm_l6_shape_is_as_close_to_hf_as_its_head_dim_64_twin(amp, tmp_path, monkeypatch):
    """d 384, 6 layers, FFN 1536, vocab 30522, init 0.02, classifier x 10, 64 pairs with one of exactly 256 tokens.  No bar has been measured for
    this shape, so the yardstick is the existing code: the twin with 6 heads (head dim 64) runs the existing kernels on the same seed, pairs and
    AMP mode; each model is compared with its own HF fp32 logits and head dim 32 may be at most twice as far, relative to the spread (the two are
    different random functions, and attention is one of several rounding sites per layer)."""
    monkeypatch.setenv("CLDRD_AMP", amp)
    ratios = {}
    for heads in (12, 6):
        c = _l6(heads, tmp_path)
        model = CrossEncoder.from_pretrained(c["path"], eval_only=True).cuda()
        assert model.cfg.head_dim == 384 // heads and int(c["batch"]["attention_mask"].sum(1).max()) == 256
        ref = c["ref"]
        spread = ref.max() - ref.min()
        got = model(c["batch"]).cpu().numpy()
        sc = model.score_cached(*_L6["data"], 256).cpu().numpy()
        ratios[heads] = (np.abs(got - ref).max() / spread, np.abs(sc - ref[:, 0]).max() / spread)
        del model
    (p32, c32), (p64, c64) = ratios[12], ratios[6]
    _record(f"MiniLM-L-6 shape {amp}: err / spread  head dim 32 padded {p32:.3e} cached {c32:.3e};  head-dim-64 twin padded {p64:.3e} cached {c64:.3e}")
    assert p32 <= 2 * p64 and c32 <= 2 * c64, ratios


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_score_cached_is_batch_invariant_at_the_minilm_shape(amp, monkeypatch):
    """40 pairs scored in a call of their own and inside a call of 1500 pairs in another order: bit for bit the same scores (the attention
    kernels' item independence, and the GEMM routes at N = 384, 1152 and 1536)."""
    monkeypatch.setenv("CLDRD_AMP", amp)
    cfg = EncoderConfig(arch="bert", vocab_size=30522, dim=384, n_heads=12, hidden_dim=1536, n_layers=6)
    model = CrossEncoder(cfg, num_labels=1, seed=5).cuda()
    qc, pc, qr, pr = _base_pairs(1500)
    perm = np.random.default_rng(2).permutation(len(qr))
    whole = model.score_cached(qc, pc, qr[perm], pr[perm], 256).cpu().numpy()
    assert np.isfinite(whole).all() and np.unique(whole).shape[0] > 700
    pick = np.concatenate([[0, 1, 2], np.random.default_rng(3).choice(np.arange(3, 1500), 37, replace=False)])      # with the 256-, 2- and 130-token passages
    few = model.score_cached(qc, pc, qr[pick], pr[pick], 256).cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    assert np.array_equal(few, whole[inv[pick]]), f"{np.mean(few != whole[inv[pick]]):.3f} of the scores differ"


# ---------------------------------------------------------------- the fp32 pass
def test_fp32_pass_of_a_head_dim_32_teacher(tmp_path, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    hf = _hf_model("bert", 128, 2, 1, seed=8, heads=4)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m"), eval_only=True).cuda()
    qc, pc, qr, pr = _pairs(3, 12, 40, 96, 1000, 256, 120)
    ref32, batch = _hf_logits(hf, "bert", qc, pc, qr, pr, 256)
    import copy
    hf64 = copy.deepcopy(hf).double()
    with torch.no_grad():
        ref64 = torch.cat([hf64(**{k: v[a:a + 16] for k, v in batch.items()}).logits for a in range(0, len(qr), 16)]).numpy()
    scale = np.abs(ref64).max()
    e32 = np.abs(ref32 - ref64).max() / scale
    with torch.no_grad():
        got = model(batch, fp32=True).cpu().numpy()
        cached = model.score_cached(qc, pc, qr, pr, 256, fp32=True).cpu().numpy()
        got16 = model(batch).cpu().numpy()
    e_gpu, e_c, e16 = np.abs(got - ref64).max() / scale, np.abs(cached - ref64[:, 0]).max() / scale, np.abs(got16 - ref64).max() / scale
    _record(f"tiny head-dim-32 teacher, fp32 pass: e32 = {e32:.3e}, e_gpu = {e_gpu:.3e} (cached {e_c:.3e}), e_gpu / e32 = {e_gpu / e32:.2f}, "
            f"16-bit pass e16 = {e16:.3e}")
    assert e_gpu <= 32 * e32 and e_c <= 32 * e32
    assert 100 * e_gpu <= e16 and 100 * e_c <= e16


# ---------------------------------------------------------------- a head-dim-32 student
def _student():
    cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=4, hidden_dim=256, n_layers=2, max_position_embeddings=64,
                        dropout=0.0, attention_dropout=0.0)
    return cfg, selftest.build_tiny_model(cfg).cuda().eval()


def test_head_dim_32_student_evaluation_passes():
    from cldrd_amd.dataset import SyntheticSequenceDataset
    from cldrd_amd.retriever import retrieval_utils as RU
    cfg, model = _student()
    batch = syn.nway_batch(4680, 4, 8, 16, 48, vocab=512, ragged=True)
    ids, mask = batch["nway_passages"]["input_ids"].reshape(32, 48), batch["nway_passages"]["attention_mask"].reshape(32, 48)
    _, pp = selftest.oracle_params(model)
    with torch.no_grad():
        ref = E.encoder_forward({k: v.double() for k, v in pp.items()}, selftest.oracle_cfg(cfg), ids, mask)[:, 0].numpy()
        enc = model.passage_encoder
        padded = enc.encode(ids.cuda(), mask.cuda(), train=False).cpu().numpy()
        packed = enc.encode(ids.cuda(), mask.cuda(), train=False, lengths=mask.sum(1).tolist()).cpu().numpy()
        q = model.query_embs({k: v.cuda() for k, v in batch["query"].items()}).cpu().numpy()          # the query tower's all-fp16 pass in the fp16 mode
        q_ref = E.encoder_forward({k: v.double() for k, v in selftest.oracle_params(model)[0].items()}, selftest.oracle_cfg(cfg),
                                  batch["query"]["input_ids"], batch["query"]["attention_mask"])[:, 0].numpy()
    scale = np.abs(ref).max()
    print(f"head-dim-32 student: padded {np.abs(padded - ref).max() / scale:.2e}, packed {np.abs(packed - ref).max() / scale:.2e}, "
          f"query tower {np.abs(q - q_ref).max() / np.abs(q_ref).max():.2e} of max|cls|")
    # the small-model bar of tests/test_gpu_model.py for evaluation CLS vectors
    assert np.abs(padded - ref).max() <= 2e-2 * scale and np.abs(packed - ref).max() <= 2e-2 * scale
    assert np.abs(q - q_ref).max() <= 2e-2 * np.abs(q_ref).max()
    for use_fp16 in (True, False):
        ds = SyntheticSequenceDataset(300, 32, vocab=cfg.vocab_size, batch_size=128)
        embs, out_ids = RU.get_embeddings_from_scratch(model, ds.loader(), use_fp16=use_fp16, is_query=False)
        assert embs.shape == (300, 128) and embs.dtype == np.float32 and np.isfinite(embs).all() and out_ids == list(range(300))


def test_head_dim_32_student_refuses_to_train():
    from cldrd_amd.trainer import NwayTrainer
    cfg, model = _student()
    enc = model.passage_encoder
    ids, mask = torch.ones(2, 8, dtype=torch.int64, device="cuda"), torch.ones(2, 8, dtype=torch.int64, device="cuda")
    for call in (lambda: enc.encode(ids, mask, save=True), lambda: enc.encode(ids, mask, train=True), lambda: encode_autograd(enc, ids, mask),
                 lambda: NwayTrainer(model, loss="margin_mse")):
        with pytest.raises(ValueError, match="head dim 32"):
            call()
    assert isinstance(enc, HipEncoder) and torch.isfinite(enc.encode(ids, mask, train=False)).all()


# ---------------------------------------------------------------- command line
def test_rerank_command_line_with_a_head_dim_32_teacher(tmp_path):
    from cldrd_amd.dataset import RerankingDataset
    from cldrd_amd.retriever import rerank_top_passages as R
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    hf = _hf_model("bert", 128, 2, 1, seed=12, heads=4, vocab=tok.vocab_size + 4)
    model_dir = _save(hf, tmp_path, "teacher")
    q_path, c_path, run_path = _toy_files(tmp_path)
    out = tmp_path / "out.tsv"
    R.main(R.get_args(["--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path),
                       "--model_name_or_path", model_dir, "--tokenizer_name_or_path", tok_dir, "--max_len", "48",
                       "--batch_size", "300", "--token_cache_dir", str(tmp_path / "cache"), "--output_path", str(out)]))
    rows = [ln.split("\t") for ln in out.read_text().splitlines()]
    # the order test_rerank_command_line checks: queries in the order of the run, ranks 1 .. n by descending score, every pair once
    ds = RerankingDataset(str(run_path), str(q_path), str(c_path), tok, True, max_len=48)
    pairs = list(dict.fromkeys(ds.qid_pid_pairs))
    q_order = list(dict.fromkeys(q for q, _ in pairs))
    assert list(dict.fromkeys(int(r[0]) for r in rows)) == q_order
    got = [(int(r[0]), int(r[1])) for r in rows]
    assert sorted(got) == sorted(pairs) and len(set(got)) == len(got)
    oracle = {}
    with torch.no_grad():
        for qid, pid in pairs:
            e = tok(ds.qid_to_query[qid], ds.pid_to_passage[pid], truncation="longest_first", max_length=48, return_tensors="pt")
            oracle[(qid, pid)] = hf(**e).logits[0, 0].item()
    bar = TINY_BAR * (max(oracle.values()) - min(oracle.values()))
    for q in q_order:
        mine = [r for r in rows if int(r[0]) == q]
        assert [int(r[2]) for r in mine] == list(range(1, len(mine) + 1))
        for a, b in zip(mine, mine[1:]):
            assert float(a[3]) >= float(b[3])
        for r in mine:
            assert abs(float(r[3]) - oracle[(q, int(r[1]))]) <= bar
    # ... and the scores are score_cached's: the command line's own token caches, the pairs of the run
    from cldrd_amd.dataset import SequenceTokenCache
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(tok_dir)
    q_cache = SequenceTokenCache.open_or_build(str(tmp_path / "cache"), str(q_path), tokenizer, 48)
    p_cache = SequenceTokenCache.open_or_build(str(tmp_path / "cache"), str(c_path), tokenizer, 48)
    q_row = {int(k): i for i, k in enumerate(np.asarray(q_cache.keys))}
    p_row = {int(k): i for i, k in enumerate(np.asarray(p_cache.keys))}
    model = CrossEncoder.from_pretrained(model_dir, max_len=48, eval_only=True).cuda()
    sc = model.score_cached(q_cache, p_cache, np.array([q_row[q] for q, _ in got]), np.array([p_row[p] for _, p in got]), 48).cpu().numpy()
    assert np.array_equal(np.array([float(r[3]) for r in rows], dtype=np.float32), sc.astype(np.float32))
