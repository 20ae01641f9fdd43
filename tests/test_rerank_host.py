"""Host-side checks of the cross-encoder teacher path: pair truncation against the HF fast tokenizer, RerankingDataset against direct
tokenizer calls, CrossEncoder checkpoint loading and its refusals."""
import json

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd.dataset import RerankingDataset
from cldrd_amd.models.cross_encoder import CrossEncoder, pair_lengths
from tokenizers import Tokenizer
from tokenizers.models import WordLevel
from tokenizers.pre_tokenizers import Whitespace
from tokenizers.processors import TemplateProcessing
from transformers import PreTrainedTokenizerFast

# ---------------------------------------------------------------- host restatements (tests/test_gpu_rerank.py imports them from here):
# a pair tokenizer (WordLevel vocabulary, BERT pair template, token types), packed pair rows built from token-cache rows with plain
# Python slicing, and random token caches
CLS, SEP = 2, 3


def make_pair_tokenizer(n_words=60):
    vocab = {"[PAD]": 0, "[UNK]": 1, "[CLS]": CLS, "[SEP]": SEP}
    for i in range(n_words):
        vocab[f"w{i}"] = len(vocab)
    tok = Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = Whitespace()
    tok.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                            special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    return PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="[PAD]", unk_token="[UNK]", cls_token="[CLS]", sep_token="[SEP]",
                                   model_input_names=["input_ids", "token_type_ids", "attention_mask"])


def words(n, offset=0, n_words=60):
    return " ".join(f"w{(offset + i) % n_words}" for i in range(n))


def pair_rows(q_row, p_row, kq, kp):
    """(ids, types, positions) of one pair from two cache rows ([CLS] content [SEP], trailing zeros allowed) and the kept counts."""
    q = [int(t) for t in q_row]
    p = [int(t) for t in p_row]
    lq = len(q)
    if kp == 0 and len(p) == 2:
        ids = q[:1 + kq] + [q[lq - 1]]
        return ids, [0] * len(ids), list(range(len(ids)))
    ids = q[:1 + kq] + [q[lq - 1]] + p[1:1 + kp] + [p[len(p) - 1]]
    types = [0] * (kq + 2) + [1] * (kp + 1)
    return ids, types, list(range(len(ids)))


def random_cache(rng, n, width, lens, vocab, dtype=np.int32, key0=0):
    """A SequenceTokenCache of n rows `[CLS] random ids [SEP]` (lens include the two specials), zero padded to width."""
    from cldrd_amd.dataset import SequenceTokenCache
    lens = np.asarray(lens, dtype=np.int32)
    ids = np.zeros((n, width), dtype=dtype)
    for r in range(n):
        ids[r, 0] = CLS
        ids[r, 1:lens[r] - 1] = rng.integers(5, vocab, lens[r] - 2)
        ids[r, lens[r] - 1] = SEP
    return SequenceTokenCache(np.arange(n, dtype=np.int64) + key0, ids, lens, {"rows": n, "max_length": width})


# ---------------------------------------------------------------- tests


@pytest.mark.parametrize("max_len", [8, 11, 12, 33, 64])
def test_pair_lengths_match_the_hf_fast_tokenizer(max_len):
    tok = make_pair_tokenizer()
    N = 41
    nq, npp = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    nq, npp = nq.ravel(), npp.ravel()
    kq, kp, lengths, cu = pair_lengths(nq, npp, max_len)
    assert cu[0] == 0 and (np.diff(cu) == lengths).all()
    q_texts = [words(int(a)) for a in nq]
    p_texts = [words(int(b), 30) for b in npp]
    single = {n: tok(words(n), truncation="longest_first", max_length=10 ** 6)["input_ids"] for n in range(N)}
    single_p = {n: tok(words(n, 30), truncation="longest_first", max_length=10 ** 6)["input_ids"] for n in range(N)}
    for m in range(nq.shape[0]):
        e = tok(q_texts[m], p_texts[m], truncation="longest_first", max_length=max_len)
        ids, types, _ = pair_rows(single[int(nq[m])], single_p[int(npp[m])], int(kq[m]), int(kp[m]))
        assert e["input_ids"] == ids, (nq[m], npp[m])
        assert e["token_type_ids"] == types, (nq[m], npp[m])
        assert len(ids) == lengths[m]


def test_pair_lengths_longest_first_examples():
    kq, kp, _, _ = pair_lengths([12, 13, 3, 6], [12, 12, 20, 20], 12)       # budget 9
    assert kq.tolist() == [4, 5, 3, 4] and kp.tolist() == [5, 4, 6, 5]
    kq, kp, lengths, _ = pair_lengths([5, 0], [0, 0], 6)
    assert kq.tolist() == [4, 0] and kp.tolist() == [0, 0] and lengths.tolist() == [6, 2]


def _files(tmp_path, ncol):
    q = tmp_path / "q.tsv"
    c = tmp_path / "c.tsv"
    r = tmp_path / "r.tsv"
    q.write_text("1\tw1 w2 w3\n2\tw4 w5\n3\tw7 w8 w9 w10 w11 w12 w13\n")
    c.write_text("".join(f"{10 + j}\t{words(3 + 4 * j, j)}\n" for j in range(6)) + "20\ttitle w1\tw2 w3 w4\n")
    extra = {2: "", 3: "\t0.5", 4: "\t3\t0.5"}[ncol]
    r.write_text("".join(f"{q}\t{p}{extra}\n" for q, p in [(2, 11), (1, 10), (1, 12), (3, 15), (3, 20), (2, 13)]))
    return q, c, r


@pytest.mark.parametrize("ncol", [2, 3, 4])
def test_reranking_dataset(tmp_path, ncol):
    tok = make_pair_tokenizer()
    q, c, r = _files(tmp_path, ncol)
    ds = RerankingDataset(str(r), str(q), str(c), tok, True, max_len=12)
    assert ds.qid_pid_pairs == [(2, 11), (1, 10), (1, 12), (3, 15), (3, 20), (2, 13)]
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert batch["qid"] == [2, 1, 1, 3, 3, 2] and batch["pid"] == [11, 10, 12, 15, 20, 13]
    texts_p = [ds.pid_to_passage[p] if isinstance(ds.pid_to_passage[p], str) else "title [SEP] w2 w3 w4" for p in batch["pid"]]
    assert ds[4]["passage"] == "title w1 [SEP] w2 w3 w4"
    texts_p[4] = ds[4]["passage"]
    want = tok([ds.qid_to_query[x] for x in batch["qid"]], texts_p, padding=True, truncation="longest_first", return_tensors="pt", max_length=12)
    for k in ("input_ids", "attention_mask", "token_type_ids"):
        assert torch.equal(batch["query_passage"][k], want[k])
    ds2 = RerankingDataset(str(r), str(q), str(c), tok, False, query_max_len=4, passage_max_len=9)
    b2 = ds2.collate_fn([ds2[i] for i in range(len(ds2))])
    wq = tok([ds2.qid_to_query[x] for x in b2["qid"]], padding=True, truncation="longest_first", return_tensors="pt", max_length=4)
    wp = tok(texts_p, padding=True, truncation="longest_first", return_tensors="pt", max_length=9)
    assert torch.equal(b2["query"]["input_ids"], wq["input_ids"]) and torch.equal(b2["passage"]["input_ids"], wp["input_ids"])


def test_reranking_dataset_passage_first(tmp_path):
    tok = make_pair_tokenizer()
    q, c, _ = _files(tmp_path, 2)
    r = tmp_path / "pf.tsv"
    r.write_text("10\t1\t1\t0.3\n13\t2\t2\t0.1\n")
    ds = RerankingDataset(str(r), str(q), str(c), tok, True, query_first=False, max_len=16)
    assert ds.qid_pid_pairs == [(1, 10), (2, 13)]
    assert ds[1] == {"qid": 2, "pid": 13, "query": "w4 w5", "passage": ds.pid_to_passage[13]}


def _hf(arch, nl, heads=2, d=128, tmp_path=None):
    from transformers import BertConfig, BertForSequenceClassification, DistilBertConfig, DistilBertForSequenceClassification
    torch.manual_seed(3 + nl)
    if arch == "bert":
        m = BertForSequenceClassification(BertConfig(vocab_size=100, hidden_size=d, num_hidden_layers=2, num_attention_heads=heads,
                                                     intermediate_size=256, max_position_embeddings=300, num_labels=nl))
    else:
        m = DistilBertForSequenceClassification(DistilBertConfig(vocab_size=100, dim=d, n_layers=2, n_heads=heads, hidden_dim=256,
                                                                 max_position_embeddings=300, num_labels=nl))
    path = str(tmp_path / f"{arch}{nl}{heads}")
    m.save_pretrained(path)
    return m, path


@pytest.mark.parametrize("arch,nl", [("bert", 1), ("bert", 2), ("distilbert", 1), ("distilbert", 2)])
def test_cross_encoder_from_pretrained_key_mapping(arch, nl, tmp_path):
    hf, path = _hf(arch, nl, tmp_path=tmp_path)
    model = CrossEncoder.from_pretrained(path)
    assert model.num_labels == nl and model.head_act == ("tanh" if arch == "bert" else "relu")
    sd = hf.state_dict()
    pre = "bert." if arch == "bert" else "distilbert."
    dense = "bert.pooler.dense" if arch == "bert" else "pre_classifier"
    assert torch.equal(model.head_w1, sd[dense + ".weight"]) and torch.equal(model.head_b1, sd[dense + ".bias"])
    assert torch.equal(model.head_w2, sd["classifier.weight"]) and torch.equal(model.head_b2, sd["classifier.bias"])
    own = dict(model.encoder.named_parameters())
    for name, p in own.items():
        assert torch.equal(p, sd[pre + name]), name
    if arch == "bert":
        assert "embeddings.token_type_embeddings.weight" in own
    with pytest.raises(RuntimeError, match="GPU"):         # the model is still on the host: no CPU path
        model({"input_ids": torch.ones(1, 4, dtype=torch.int64), "attention_mask": torch.ones(1, 4, dtype=torch.int64)})


def test_cross_encoder_refusals(tmp_path):
    from transformers import ElectraConfig
    e = tmp_path / "electra"
    e.mkdir()
    ElectraConfig(num_labels=1).to_json_file(str(e / "config.json"))
    with pytest.raises(ValueError, match="electra"):
        CrossEncoder.from_pretrained(str(e))
    _, path = _hf("bert", 1, heads=4, tmp_path=tmp_path)            # d = 128, 4 heads: head dim 32
    with pytest.raises(ValueError, match="head dim 32"):
        CrossEncoder.from_pretrained(path)
    _, path = _hf("distilbert", 1, tmp_path=tmp_path)
    with pytest.raises(ValueError, match="max_len 300"):
        CrossEncoder.from_pretrained(path, max_len=300)
    cfg = json.load(open(path + "/config.json"))
    cfg["id2label"] = {"0": "a", "1": "b", "2": "c"}
    json.dump(cfg, open(path + "/config.json", "w"))
    with pytest.raises(ValueError, match="num_labels 3"):
        CrossEncoder.from_pretrained(path)


def test_read_run_order_duplicates_and_top_k(tmp_path):
    from cldrd_amd.retriever.rerank_top_passages import read_run
    r = tmp_path / "run.tsv"
    r.write_text("7 70 1 0.9\n3 30\n7 71 2 0.8\n7 70 3 0.1\n3 31 0.5\n9 90\n3 32\n7 72\n")
    qids, pids, group, starts = read_run(str(r))
    assert qids.tolist() == [7, 7, 7, 3, 3, 3, 9] and pids.tolist() == [70, 71, 72, 30, 31, 32, 90]
    assert group.tolist() == [0, 0, 0, 1, 1, 1, 2] and starts.tolist() == [0, 3, 6, 7]
    qids, pids, group, starts = read_run(str(r), top_k=2)
    assert pids.tolist() == [70, 71, 30, 31, 90] and starts.tolist() == [0, 2, 4, 5]
