"""Cross-encoder teacher scoring on the GPU: pair assembly, typed embeddings, CrossEncoder against HF *ForSequenceClassification, the
padded against the cached path, and the rerank_top_passages command line."""
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd import hip_ops as ops
from cldrd_amd.models.cross_encoder import CrossEncoder, pair_lengths
from test_rerank_host import make_pair_tokenizer, pair_rows, random_cache, words

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_build_pairs_equals_host_restatement(dtype):
    rng = np.random.default_rng(5)
    W, max_len = 120, 64
    qlens = np.concatenate([[2, 3, 2 + 30, 2 + 80], rng.integers(2, W + 1, 12)])        # empty query content, single token, over budget
    plens = np.concatenate([[2, 3, 2 + 61, 2 + 100, 2 + 118], rng.integers(2, W + 1, 27)])  # empty passage, single token, budget hit, over
    qc = random_cache(rng, len(qlens), W, qlens, 60000, dtype)
    pc = random_cache(rng, len(plens), W, plens, 60000, dtype)
    qr = np.concatenate([[0, 1, 2, 3, 0, 2, 1, 3], rng.integers(0, len(qlens), 200)])
    pr = np.concatenate([[0, 1, 2, 3, 2, 3, 4, 0], rng.integers(0, len(plens), 200)])
    kq, kp, lengths, cu = pair_lengths(qc.lens[qr] - 2, pc.lens[pr] - 2, max_len)
    assert lengths.max() == max_len and lengths.min() == 2 and (kq[:8] + kp[:8] == max_len - 3).sum() >= 3
    tok = lambda c: torch.from_numpy(np.ascontiguousarray(c.ids).view(np.int16) if dtype == np.uint16 else np.ascontiguousarray(c.ids)).to(DEV)
    ids, types, pos = ops.build_pairs(tok(qc), _i32(qc.lens), tok(pc), _i32(pc.lens), _i32(qr), _i32(pr), _i32(kq), _i32(kp), _i32(cu),
                                      int(cu[-1]))
    want_i, want_t, want_p = [], [], []
    for m in range(len(qr)):
        i, t, p = pair_rows(qc.ids[qr[m], :qc.lens[qr[m]]], pc.ids[pr[m], :pc.lens[pr[m]]], int(kq[m]), int(kp[m]))
        assert len(i) == lengths[m]
        want_i += i
        want_t += t
        want_p += p
    assert ids.cpu().numpy().tolist() == want_i
    assert types.cpu().numpy().tolist() == want_t
    assert pos.cpu().numpy().tolist() == want_p


@pytest.mark.parametrize("d", [128, 768])
def test_embed_ln_fwd_typed(d):
    g = torch.Generator().manual_seed(d)
    V, P, T, L = 300, 64, 333, 37
    word, pos = torch.randn(V, d, generator=g).to(DEV), torch.randn(P, d, generator=g).to(DEV)
    typ = (torch.randn(2, d, generator=g) * 0.5).to(DEV)
    gam, bet = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ids = torch.randint(0, V, (T,), generator=g).to(DEV)
    posi = (torch.arange(T) % L).to(torch.int32).to(DEV)

    def run(types):
        out, o32 = torch.empty(T, d, dtype=torch.bfloat16, device=DEV), torch.empty(T, d, device=DEV)
        mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
        ops.embed_ln_fwd(ids, word, pos, typ, gam, bet, out, mean, rstd, T, L, 1e-12, out32=o32, pos_idx=posi, type_ids=types)
        return out, o32, mean, rstd
    zero = run(torch.zeros(T, dtype=torch.int32, device=DEV))
    base = run(None)
    for a, b in zip(zero, base):
        assert torch.equal(a, b)
    tt = torch.randint(0, 2, (T,), generator=g).to(torch.int32)
    _, o32, _, _ = run(tt.to(DEV))
    x = word.cpu()[ids.cpu()] + pos.cpu()[posi.cpu().long()] + typ.cpu()[tt.long()]
    ref = torch.nn.functional.layer_norm(x.double(), (d,), gam.cpu().double(), bet.cpu().double(), 1e-12)
    assert (o32.cpu().double() - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embed_ln_fwd_all_zero_type_ids_equal_no_type_ids(p):
    """include/cldrd_hip.h: with all-zero type_ids the typed form computes what type_ids = NULL does - bit for bit, with and without dropout
    (same seed); two sequences of 8 rows, a two-row token-type table."""
    g = torch.Generator().manual_seed(5)
    V, T, L, d = 50, 16, 8, 128
    word, pos, typ = torch.randn(V, d, generator=g).to(DEV), torch.randn(L, d, generator=g).to(DEV), torch.randn(2, d, generator=g).to(DEV)
    gam, bet = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    ids = torch.randint(0, V, (T,), generator=g).to(DEV)

    def run(types):
        out, o32 = torch.empty(T, d, dtype=torch.bfloat16, device=DEV), torch.empty(T, d, device=DEV)
        mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
        ops.embed_ln_fwd(ids, word, pos, typ, gam, bet, out, mean, rstd, T, L, 1e-12, dropout_p=p, seed=11, out32=o32, type_ids=types)
        return out, o32, mean, rstd
    for a, b in zip(run(torch.zeros(T, dtype=torch.int32, device=DEV)), run(None)):
        assert torch.equal(a, b)
    ones = run(torch.ones(T, dtype=torch.int32, device=DEV))
    assert not torch.equal(ones[2], run(None)[2])           # the type ids are read: row 1 of the table moves the means


# ---------------------------------------------------------------- CrossEncoder against HF
def _hf_model(arch, d, layers, nl, seed, vocab=1000):
    from transformers import BertConfig, BertForSequenceClassification, DistilBertConfig, DistilBertForSequenceClassification
    torch.manual_seed(seed)
    # the small models get a wider init (std 0.05): at 0.02 two layers of d = 128 leave the pooled CLS rows of different pairs nearly
    # alike, and a bar relative to the logit spread would then measure the 16-bit rounding of the common part
    init = 0.05 if d < 768 else 0.02
    if arch == "bert":
        cfg = BertConfig(vocab_size=vocab, hidden_size=d, num_hidden_layers=layers, num_attention_heads=d // 64, intermediate_size=4 * d,
                         max_position_embeddings=512, num_labels=nl, initializer_range=init)
        cls = BertForSequenceClassification
    else:
        cfg = DistilBertConfig(vocab_size=vocab, dim=d, n_layers=layers, n_heads=d // 64, hidden_dim=4 * d, max_position_embeddings=512,
                               num_labels=nl, initializer_range=init)
        cls = DistilBertForSequenceClassification
    cfg._attn_implementation = "eager"
    m = cls(cfg).eval()
    with torch.no_grad():       # spread the classifier a little: random init gives logits of a few 1e-2
        m.classifier.weight.mul_(10.0)
    return m


def _save(model, tmp_path, name):
    path = str(tmp_path / name)
    model.save_pretrained(path)
    return path


def _pairs(seed, n_q, n_p, n_pairs, vocab, max_len, plen_hi):
    rng = np.random.default_rng(seed)
    qc = random_cache(rng, n_q, max_len, rng.integers(3, 34, n_q), vocab)
    plens = np.clip(np.round(rng.lognormal(np.log(plen_hi / 2.5), 0.7, n_p)), 3, max_len).astype(np.int32)
    plens[:4] = [max_len, max_len - 1, 3, 2]
    pc = random_cache(rng, n_p, max_len, plens, vocab)
    qr, pr = rng.integers(0, n_q, n_pairs), rng.integers(0, n_p, n_pairs)
    pr[:4] = [0, 1, 2, 3]
    return qc, pc, qr, pr


def _hf_logits(hf, arch, qc, pc, qr, pr, max_len):
    kq, kp, lengths, _ = pair_lengths(qc.lens[qr] - 2, pc.lens[pr] - 2, max_len)
    L = int(lengths.max())
    ids = np.zeros((len(qr), L), np.int64)
    tts, mask = np.zeros_like(ids), np.zeros_like(ids)
    for m in range(len(qr)):
        i, t, _ = pair_rows(qc.ids[qr[m], :qc.lens[qr[m]]], pc.ids[pr[m], :pc.lens[pr[m]]], int(kq[m]), int(kp[m]))
        ids[m, :len(i)], tts[m, :len(i)], mask[m, :len(i)] = i, t, 1
    batch = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}
    if arch == "bert":
        batch["token_type_ids"] = torch.from_numpy(tts)
    out = []
    with torch.no_grad():
        for a in range(0, len(qr), 16):
            out.append(hf(**{k: v[a:a + 16] for k, v in batch.items()}).logits.float())
    return torch.cat(out).numpy(), batch


def _scores(logits, nl):
    t = torch.from_numpy(np.asarray(logits, np.float64))
    return (t[:, 0] if nl == 1 else torch.log_softmax(t, -1)[:, 1]).numpy()


# Bars, asserted both relative to the SPREAD (max - min) of the HF fp32 logits over the pairs and relative to max|logit| (the scale the
# existing bars of tests/test_gpu_model.py use); the tests print both:
#   d = 128, 2 layers: 2e-2, the bar of the small-model logits against the CPU oracle in tests/test_gpu_model.py; measured at most
#   1.3e-2 of the spread, 7.0e-3 of max|logit|;
#   BERT-base, 12 layers, pairs up to 256 tokens: CLDRD_AMP=fp16 5e-3, the full-size eval-mode bar of tests/test_gpu_model.py (5e-3 of
#   max|logit|), measured 3.7e-3 of the spread, 4.3e-3 of max|logit|; CLDRD_AMP=bf16 (every operand bf16, 8-bit significands) 2e-2, the
#   small-model bar, measured 1.6e-2 / 1.9e-2.
TINY_BAR = 2e-2
BASE_BAR = {"fp16": 5e-3, "bf16": 2e-2}


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("arch,nl", [("bert", 1), ("bert", 2), ("distilbert", 1), ("distilbert", 2)])
def test_cross_encoder_tiny_matches_hf(arch, nl, amp, tmp_path, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", amp)
    hf = _hf_model(arch, 128, 2, nl, seed=7 + nl)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m")).cuda()
    qc, pc, qr, pr = _pairs(3, 12, 40, 96, 1000, 256, 120)
    ref, batch = _hf_logits(hf, arch, qc, pc, qr, pr, 256)
    got = model(batch).cpu().numpy()
    spread = ref.max() - ref.min()
    err = np.abs(got - ref).max()
    print(f"tiny {arch} nl={nl} {amp}: max|dlogit| {err:.3e} = {err / spread:.2e} of the spread {spread:.3e}, "
          f"{err / np.abs(ref).max():.2e} of max|logit|")
    assert err <= TINY_BAR * np.abs(ref).max()
    assert err <= TINY_BAR * spread
    sc = model.score_cached(qc, pc, qr, pr, 256).cpu().numpy()
    ref_s = _scores(ref, nl)
    assert np.abs(sc - ref_s).max() <= TINY_BAR * (ref_s.max() - ref_s.min())


_BASE = {}


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_cross_encoder_bert_base_matches_hf(amp, tmp_path, monkeypatch):
    monkeypatch.setenv("CLDRD_AMP", amp)
    if "ref" not in _BASE:
        torch.set_num_threads(16)
        hf = _hf_model("bert", 768, 12, 1, seed=21, vocab=30522)
        qc, pc, qr, pr = _pairs(9, 16, 80, 64, 30522, 256, 160)
        ref, batch = _hf_logits(hf, "bert", qc, pc, qr, pr, 256)
        _BASE.update(ref=ref, batch=batch, data=(qc, pc, qr, pr), path=_save(hf, tmp_path, "base"))
    model = CrossEncoder.from_pretrained(_BASE["path"]).cuda()
    ref = _BASE["ref"]
    assert int(_BASE["batch"]["attention_mask"].sum(1).max()) == 256
    got = model(_BASE["batch"]).cpu().numpy()
    sc = model.score_cached(*_BASE["data"], 256).cpu().numpy()
    spread = ref.max() - ref.min()
    err, err_c = np.abs(got - ref).max(), np.abs(sc - ref[:, 0]).max()
    scale = np.abs(ref).max()
    print(f"BERT-base {amp}: max|dlogit| padded {err / spread:.2e}, cached {err_c / spread:.2e} of the spread {spread:.3e}; "
          f"{err / scale:.2e} / {err_c / scale:.2e} of max|logit| {scale:.3e}")
    assert err <= BASE_BAR[amp] * spread and err_c <= BASE_BAR[amp] * spread
    assert err <= BASE_BAR[amp] * scale and err_c <= BASE_BAR[amp] * scale


def test_padded_forward_matches_score_cached(tmp_path):
    """The two paths pack the same rows; bar: the packed-vs-padded bar of test_packed_index_encode_matches_padded (2e-3 of max|value|)."""
    hf = _hf_model("bert", 128, 3, 2, seed=4)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m")).cuda()
    qc, pc, qr, pr = _pairs(17, 20, 200, 300, 1000, 256, 140)
    _, batch = _hf_logits(hf, "bert", qc, pc, qr, pr, 256)
    a = model.scores(model(batch)).cpu().numpy()
    b = model.score_cached(qc, pc, qr, pr, 256).cpu().numpy()
    print(f"padded vs cached: identical {np.mean(a == b):.2f}, max diff {np.abs(a - b).max() / np.abs(a).max():.2e} of max|score|")
    assert np.abs(a - b).max() <= 2e-3 * np.abs(a).max()


def test_score_cached_refuses_a_short_cache(tmp_path):
    hf = _hf_model("distilbert", 128, 1, 1, seed=2)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m")).cuda()
    rng = np.random.default_rng(0)
    qc, pc = random_cache(rng, 2, 30, [5, 6], 1000), random_cache(rng, 2, 128, [40, 50], 1000)
    with pytest.raises(ValueError, match="max_length 30"):
        model.score_cached(qc, pc, [0, 1], [1, 0], 256)


# ---------------------------------------------------------------- command line
def _toy_files(tmp_path, n_q=6, n_p=40, per_q=12):
    rng = np.random.default_rng(31)
    q_path, c_path, run_path = tmp_path / "queries.tsv", tmp_path / "collection.tsv", tmp_path / "run.tsv"
    q_path.write_text("".join(f"{100 + i}\t{words(int(rng.integers(1, 9)), 3 * i)}\n" for i in range(n_q)))
    c_path.write_text("".join(f"{5000 + j}\t{words(int(rng.integers(1, 70)), 7 * j)}\n" for j in range(n_p)))
    lines = []
    for i in rng.permutation(n_q):
        for r, j in enumerate(rng.choice(n_p, per_q, replace=False)):
            lines.append(f"{100 + i}\t{5000 + j}\t{r + 1}\t{-0.1 * r:.2f}\n")
    lines.insert(5, lines[2])                    # a duplicated pair: written once
    run_path.write_text("".join(lines))
    return q_path, c_path, run_path


def test_rerank_command_line(tmp_path):
    from cldrd_amd.dataset import RerankingDataset
    from cldrd_amd.retriever import rerank_top_passages as R
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    hf = _hf_model("bert", 128, 2, 1, seed=12, vocab=tok.vocab_size + 4)
    model_dir = _save(hf, tmp_path, "teacher")
    q_path, c_path, run_path = _toy_files(tmp_path)
    outs = []
    for bs in (300, 2048):
        out = tmp_path / f"out{bs}.tsv"
        R.main(R.get_args(["--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path),
                           "--model_name_or_path", model_dir, "--tokenizer_name_or_path", tok_dir, "--max_len", "48",
                           "--batch_size", str(bs), "--token_cache_dir", str(tmp_path / "cache"), "--output_path", str(out)]))
        outs.append(out.read_text())
    rows = [ln.split("\t") for ln in outs[0].splitlines()]
    if outs[0] != outs[1]:
        b = [ln.split("\t") for ln in outs[1].splitlines()]
        d = max(abs(float(x[3]) - float(y[3])) for x, y in zip(rows, b))
        pytest.fail(f"run file depends on --batch_size (max score difference {d:.3e}; same order: {[x[:3] for x in rows] == [y[:3] for y in b]})")
    # oracle: HF on the host over the reference collate's pairs (single-pair tokenizer calls: an empty passage is the single sequence)
    ds = RerankingDataset(str(run_path), str(q_path), str(c_path), tok, True, max_len=48)
    pairs = list(dict.fromkeys(ds.qid_pid_pairs))
    oracle = {}
    with torch.no_grad():
        for qid, pid in pairs:
            e = tok(ds.qid_to_query[qid], ds.pid_to_passage[pid], truncation="longest_first", max_length=48, return_tensors="pt")
            oracle[(qid, pid)] = hf(**e).logits[0, 0].item()
    spread = max(oracle.values()) - min(oracle.values())
    bar = TINY_BAR * spread
    q_order = list(dict.fromkeys(q for q, _ in pairs))
    assert list(dict.fromkeys(int(r[0]) for r in rows)) == q_order
    got = [(int(r[0]), int(r[1])) for r in rows]
    assert sorted(got) == sorted(pairs) and len(set(got)) == len(got)
    for q in q_order:
        mine = [r for r in rows if int(r[0]) == q]
        assert [int(r[2]) for r in mine] == list(range(1, len(mine) + 1))
        for a, b in zip(mine, mine[1:]):
            assert float(a[3]) >= float(b[3])
            oa, ob = oracle[(q, int(a[1]))], oracle[(q, int(b[1]))]
            assert oa >= ob - bar, f"query {q}: {a[1]} above {b[1]} but the oracle has {oa:.5f} < {ob:.5f}"
        for r in mine:
            assert abs(float(r[3]) - oracle[(q, int(r[1]))]) <= bar


# ---------------------------------------------------------------- a pair's score does not depend on its batch
def _base_pairs(n_pairs, seed=41, vocab=30522, max_len=256):
    rng = np.random.default_rng(seed)
    n_q, n_p = 64, n_pairs
    qc = random_cache(rng, n_q, max_len, rng.integers(3, 34, n_q), vocab, np.uint16)
    plens = np.clip(np.round(rng.lognormal(np.log(74), 0.6, n_p)), 3, max_len).astype(np.int32)
    plens[:3] = [max_len, 2, 130]
    pc = random_cache(rng, n_p, max_len, plens, vocab, np.uint16)
    return qc, pc, rng.integers(0, n_q, n_pairs), rng.permutation(n_p)


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_score_cached_is_batch_invariant_at_full_size(amp, monkeypatch):
    """BERT-base shapes (d = 768, K up to 3072, 12 layers: the fp16 mode's QKV projection on fp16 operands too): the same 2600 pairs scored
    in one call, in calls of 2048, 1024 and 300 pairs (below 1024 the GEMMs would take the small-M / split-K kernels), and in a shuffled
    order - every score bit for bit the same."""
    from cldrd_amd.encoder import _KNOWN, EncoderConfig
    monkeypatch.setenv("CLDRD_AMP", amp)
    model = CrossEncoder(EncoderConfig(**_KNOWN["bert-base-uncased"]), num_labels=1, seed=5).cuda()
    qc, pc, qr, pr = _base_pairs(2600)
    whole = model.score_cached(qc, pc, qr, pr, 256).cpu().numpy()
    assert np.isfinite(whole).all() and np.unique(whole).shape[0] > 1000
    for bs in (2048, 1024, 300):
        got = np.concatenate([model.score_cached(qc, pc, qr[a:a + bs], pr[a:a + bs], 256).cpu().numpy() for a in range(0, len(qr), bs)])
        assert np.array_equal(got, whole), f"batch {bs}: {np.mean(got != whole):.3f} of the scores differ, max {np.abs(got - whole).max():.2e}"
    perm = np.random.default_rng(2).permutation(len(qr))
    got = model.score_cached(qc, pc, qr[perm], pr[perm], 256).cpu().numpy()
    assert np.array_equal(got, whole[perm])


def test_rerank_command_line_is_batch_invariant_at_full_size(tmp_path):
    """The command line with a d = 768 / dff = 3072 teacher on 2 400 pairs at --batch_size 300, 1024 and 2048: the same file."""
    from cldrd_amd.retriever import rerank_top_passages as R
    tok = make_pair_tokenizer()
    tok_dir = str(tmp_path / "tok")
    tok.save_pretrained(tok_dir)
    hf = _hf_model("bert", 768, 2, 1, seed=13, vocab=tok.vocab_size + 4)
    model_dir = _save(hf, tmp_path, "teacher")
    q_path, c_path, run_path = _toy_files(tmp_path, n_q=40, n_p=400, per_q=60)
    outs = []
    for bs in (300, 1024, 2048):
        out = tmp_path / f"out{bs}.tsv"
        R.main(R.get_args(["--run_path", str(run_path), "--queries_path", str(q_path), "--collection_path", str(c_path),
                           "--model_name_or_path", model_dir, "--tokenizer_name_or_path", tok_dir, "--max_len", "96",
                           "--batch_size", str(bs), "--token_cache_dir", str(tmp_path / "cache"), "--output_path", str(out)]))
        outs.append(out.read_text())
    assert len(outs[0].splitlines()) == 40 * 60
    assert outs[0] == outs[1] == outs[2]
