"""Cross-encoder teacher: re-scores (query, passage) pairs for the next curriculum iteration's training files.

A cross-encoder is a BERT / DistilBERT body that reads the query and the passage together (``[CLS] q [SEP] p [SEP]``, token types 0 / 1)
plus a sequence-classification head on the CLS row - HF ``BertForSequenceClassification`` (pooler dense + tanh, classifier) or
``DistilBertForSequenceClassification`` (pre_classifier + ReLU, classifier).  The reference carries only the input contract of such a
teacher (``dataset/reranking_dataset.py:14-87``, ``is_cross_encoder=True``) and runs the model through HF / torch; here the body is the
packed HIP encoder (evaluation pass, CLS-only last layer), the head is ``cldrd_cls_head_fwd`` and pairs are assembled on the device from
token caches (``cldrd_build_pairs``).  Inference only.

Score of a pair (the monoBERT convention): ``logits[:, 0]`` with one label, ``log_softmax(logits)[:, 1]`` with two."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn as nn

from .. import hip_ops as ops
from ..encoder import EncoderConfig, HipEncoder

MAX_PAIR_LEN = 256          # the encoder's sequence limit (attention kernels: L <= 256)
# score_cached runs at least this many pairs per encoder pass (fewer are padded with copies of the call's shortest pair): every GEMM of the
# pass then has M >= 1024 rows (M = pairs in the CLS-only last layer, tokens before it) and takes the one-pass large-M kernels.  Below
# 1024 rows hip_ops.gemm_nt picks the 64 x 64 / split-K kernels by M, whose K sums run in another order: a pair's score would depend on
# how many pairs share its batch.
MIN_PASS_PAIRS = 1024

_ARCHS = {"bert": "BertForSequenceClassification", "distilbert": "DistilBertForSequenceClassification"}
# HF key of (dense weight, dense bias, classifier weight, classifier bias) of the head
_HEAD_KEYS = {"bert": ("bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight", "classifier.bias"),
              "distilbert": ("pre_classifier.weight", "pre_classifier.bias", "classifier.weight", "classifier.bias")}


def pair_lengths(nq, np_, max_len: int):
    """How many content tokens of the query and of the passage a pair keeps, as the HF fast tokenizer's ``truncation='longest_first'``
    leaves them for ``tokenizer(query, passage, max_length=max_len)`` with a ``[CLS] $A [SEP] $B [SEP]`` template.

    ``nq`` / ``np_``: content lengths (tokens without [CLS] / [SEP]).  With budget B = max_len - 3 and n1 <= n2 the shorter / longer side:
    nothing is cut if n1 + n2 <= B; else the longer side is cut to max(n1, B - n1) (n1 if n1 > B), and if the two still exceed B both
    become B // 2 and B // 2 + B % 2 - the larger half going to the side that was longer (the query on a tie).  An empty passage text makes
    the single sequence ``[CLS] q [SEP]`` (budget max_len - 2), which is what the tokenizer returns for a pair with an empty second text.

    Returns int64 arrays (keep_q, keep_p, lengths, cu): ``lengths`` = pair token counts, ``cu`` = [0, cumsum(lengths)]."""
    if max_len < 3:
        raise ValueError("pair_lengths: max_len must leave room for [CLS] and two [SEP]")
    nq = np.maximum(np.asarray(nq, dtype=np.int64).reshape(-1), 0)
    npp = np.maximum(np.asarray(np_, dtype=np.int64).reshape(-1), 0)
    if nq.shape != npp.shape:
        raise ValueError("pair_lengths: one query and one passage length per pair")
    B = int(max_len) - 3
    swap = nq > npp
    n1, n2 = np.minimum(nq, npp), np.maximum(nq, npp)
    m2 = np.where(n1 > B, n1, np.maximum(n1, B - n1))
    halve = n1 + m2 > B
    s1 = np.where(halve, B // 2, n1)
    s2 = np.where(halve, B // 2 + B % 2, m2)
    over = nq + npp > B
    keep_q = np.where(over, np.where(swap, s2, s1), nq)
    keep_p = np.where(over, np.where(swap, s1, s2), npp)
    single = npp == 0
    keep_q = np.where(single, np.minimum(nq, int(max_len) - 2), keep_q)
    keep_p = np.where(single, 0, keep_p)
    lengths = np.where(single, keep_q + 2, keep_q + keep_p + 3)
    cu = np.zeros(lengths.shape[0] + 1, dtype=np.int64)
    np.cumsum(lengths, out=cu[1:])
    return keep_q, keep_p, lengths, cu


def _device_rows(cache, rows, dev):
    """The cache rows a batch reads, as a compact device table: (tokens [u, w] int32 or uint16-as-int16, lens int32 [u], row index into
    the table for every entry of ``rows``)."""
    uniq, inv = np.unique(rows, return_inverse=True)
    lens = np.asarray(cache.lens[uniq], dtype=np.int32)
    w = max(int(lens.max()), 1)
    tok = np.ascontiguousarray(np.asarray(cache.ids[uniq])[:, :w])
    if tok.dtype == np.uint16:
        tok = tok.view(np.int16)            # torch has no general uint16 tensor; the kernel reads the 16 bits unsigned
    elif tok.dtype != np.int32:
        tok = tok.astype(np.int32)
    return (torch.from_numpy(tok).to(dev), torch.from_numpy(lens).to(dev),
            torch.from_numpy(inv.reshape(-1).astype(np.int32)).to(dev))


class CrossEncoder(nn.Module):
    """BERT / DistilBERT sequence-classification model on the HIP encoder.  ``forward(batch)`` -> fp32 logits [M, num_labels];
    ``score_cached(...)`` -> fp32 scores [n] of pairs assembled on the device from token caches."""

    def __init__(self, cfg: EncoderConfig, num_labels: int = 1, seed: int | None = None, max_len: int = MAX_PAIR_LEN):
        super().__init__()
        if num_labels not in (1, 2):
            raise ValueError(f"num_labels must be 1 (a relevance logit) or 2 (monoBERT), got {num_labels}")
        if max_len > MAX_PAIR_LEN or max_len > cfg.max_position_embeddings or max_len < 3:
            raise ValueError(f"max_len {max_len}: pairs are at most {MAX_PAIR_LEN} tokens (and max_position_embeddings)")
        self.encoder = HipEncoder(cfg, seed=seed)
        self.cfg, self.num_labels, self.max_len = cfg, int(num_labels), int(max_len)
        self.head_act = "tanh" if cfg.arch == "bert" else "relu"
        d = cfg.dim
        g = torch.Generator().manual_seed(0 if seed is None else int(seed) + 1)
        std = cfg.initializer_range
        self.head_w1 = nn.Parameter(torch.randn(d, d, generator=g) * std)
        self.head_b1 = nn.Parameter(torch.zeros(d))
        self.head_w2 = nn.Parameter(torch.randn(self.num_labels, d, generator=g) * std)
        self.head_b2 = nn.Parameter(torch.zeros(self.num_labels))
        self.eval()

    # ------------------------------------------------------------------ loading
    @staticmethod
    def read_config(path: str, max_len: int = MAX_PAIR_LEN):
        """(EncoderConfig, num_labels) of an HF ``*ForSequenceClassification`` directory; ValueError names what is not supported."""
        with open(os.path.join(path, "config.json")) as fh:
            c = json.load(fh)
        mt = c.get("model_type")
        if mt not in _ARCHS:
            raise ValueError(f"{path}: model_type {mt!r} is not supported (a cross-encoder here is BERT or DistilBERT)")
        archs = c.get("architectures") or [_ARCHS[mt]]
        if _ARCHS[mt] not in archs:
            raise ValueError(f"{path}: architectures {archs} - expected {_ARCHS[mt]}")
        dim, heads = (c["hidden_size"], c["num_attention_heads"]) if mt == "bert" else (c["dim"], c["n_heads"])
        if dim % heads or not (dim // heads == 64 or (dim // heads == 32 and heads % 2 == 0)):
            raise ValueError(f"{path}: head dim {dim / heads:g} with {heads} heads is not supported (the attention kernels need head dim 64, or "
                             "head dim 32 with an even number of heads)")
        num_labels = len(c["id2label"]) if "id2label" in c else int(c.get("num_labels", 2))
        if num_labels not in (1, 2):
            raise ValueError(f"{path}: num_labels {num_labels} is not supported (1 or 2)")
        if max_len > MAX_PAIR_LEN:
            raise ValueError(f"max_len {max_len} is not supported: pairs are at most {MAX_PAIR_LEN} tokens")
        cfg = EncoderConfig.from_hf_dict(c)
        cfg.validate()
        if max_len > cfg.max_position_embeddings:
            raise ValueError(f"max_len {max_len} exceeds max_position_embeddings {cfg.max_position_embeddings}")
        return cfg, num_labels

    @classmethod
    def from_pretrained(cls, path: str, max_len: int = MAX_PAIR_LEN, eval_only: bool = False) -> "CrossEncoder":
        """An HF ``BertForSequenceClassification`` / ``DistilBertForSequenceClassification`` directory (``config.json`` and
        ``model.safetensors`` or ``pytorch_model.bin``).  The model stays on the host: move it with ``.to(device)``.
        ``eval_only=True`` (the scoring programs): the caller runs evaluation passes only, so a model whose encoder has no other pass - head
        dim 32, the MiniLM shapes - is accepted.  Without it such a directory is refused as before (tests/test_rerank_host.py pins that)."""
        cfg, num_labels = cls.read_config(path, max_len)
        if cfg.head_dim != 64 and not eval_only:
            raise ValueError(f"{path}: head dim {cfg.head_dim} runs the evaluation passes only: load it with from_pretrained(..., eval_only=True)")
        model = cls(cfg, num_labels=num_labels, max_len=max_len)
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
        model.load_hf_state_dict(sd)
        return model

    def load_hf_state_dict(self, sd: dict):
        keys = _HEAD_KEYS[self.cfg.arch]
        missing = [k for k in keys if k not in sd]
        if missing:
            raise KeyError(f"missing head keys in checkpoint: {missing}")
        self.encoder.load_hf_state_dict({k: v for k, v in sd.items() if k not in keys})
        with torch.no_grad():
            for p, k in zip((self.head_w1, self.head_b1, self.head_w2, self.head_b2), keys):
                if tuple(sd[k].shape) != tuple(p.shape):
                    raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {tuple(p.shape)}")
                p.copy_(sd[k].to(torch.float32))

    # ------------------------------------------------------------------ scoring
    def _device(self):
        dev = self.encoder.flat_p.device
        if dev.type != "cuda" or self.head_w1.device != dev:
            raise RuntimeError("CrossEncoder: the model must be on the GPU (cldrd_amd has no CPU path)")
        return dev

    def _head(self, cls):
        return ops.cls_head_fwd(cls.contiguous(), self.head_w1, self.head_b1, self.head_w2, self.head_b2, self.head_act)

    def scores(self, logits):
        """logits[:, 0] (one label) or log_softmax(logits)[:, 1] (two)."""
        return logits[:, 0] if self.num_labels == 1 else torch.log_softmax(logits, dim=-1)[:, 1]

    @torch.no_grad()
    def forward(self, batch, fp32: bool = False):
        """``fp32=True``: the body runs the exact fp32 evaluation pass (HipEncoder.encode(fp32=True)); the head is fp32 in both modes.
        ``batch``: the reference collate's ``query_passage`` dict - padded ``input_ids`` / ``attention_mask`` (right padding) and, for
        BERT, ``token_type_ids`` - on the host or the device.  Returns fp32 logits [M, num_labels].  The encoder packs the batch (token
        counts from the mask)."""
        dev = self._device()
        ids = batch["input_ids"]
        if ids.dim() != 2 or ids.shape[1] > self.max_len:
            raise ValueError(f"input_ids must be [M, L] with L <= max_len = {self.max_len}")
        mask = batch.get("attention_mask")
        if mask is None:
            mask = torch.ones_like(ids)
        lengths = mask.to("cpu").sum(1).tolist()
        tt = batch.get("token_type_ids") if self.cfg.arch == "bert" else None
        cls = self.encoder.encode(ids.to(dev), mask.to(dev), train=False, lengths=lengths,
                                  token_type_ids=None if tt is None else tt.to(dev), fp32=fp32)
        return self._head(cls)

    @torch.no_grad()
    def score_cached(self, q_cache, p_cache, q_rows, p_rows, max_len: int | None = None, fp32: bool = False):
        """Scores fp32 [n] of the pairs (query row q_rows[i] of ``q_cache``, passage row p_rows[i] of ``p_cache``); the caches are
        ``TokenCache`` / ``SequenceTokenCache`` tables (``[CLS] text [SEP]`` rows).  A cache built at a smaller max_length than the pairs'
        could have cut tokens a pair keeps: refused.  (Texts of more than max_length - 2 tokens on BOTH sides are seen at their cached
        length; with an odd budget the longer side's extra token can then go to the other side.)

        A pair's score does not depend on the other pairs of the call (bit for bit, for a given max_len): the pass runs at least
        MIN_PASS_PAIRS pairs (large-M GEMM kernels only) and chooses its attention kernels for sequences of max_len tokens, so that every
        pair's arithmetic depends on its own length only.  (``forward`` on a padded batch gives no such guarantee.)

        ``fp32=True``: the body runs the exact fp32 evaluation pass.  Its kernels have one schedule for every shape, so the same guarantee
        holds without padding pairs."""
        dev = self._device()
        max_len = self.max_len if max_len is None else int(max_len)
        if max_len > self.max_len:
            raise ValueError(f"max_len {max_len} > the model's {self.max_len}")
        for name, c in (("query", q_cache), ("passage", p_cache)):
            if int(c.ids.shape[1]) < max_len:
                raise ValueError(f"the {name} token cache was built at max_length {c.ids.shape[1]} < max_len {max_len}: it may have cut "
                                 f"tokens a pair keeps; build it at max_length {max_len}")
        q_rows = np.asarray(q_rows, dtype=np.int64).reshape(-1)
        p_rows = np.asarray(p_rows, dtype=np.int64).reshape(-1)
        if q_rows.shape != p_rows.shape:
            raise ValueError("score_cached: one query row and one passage row per pair")
        if q_rows.shape[0] == 0:
            return torch.empty(0, dtype=torch.float32, device=dev)
        n = q_rows.shape[0]
        nq = np.asarray(q_cache.lens[q_rows], dtype=np.int64) - 2
        npp = np.asarray(p_cache.lens[p_rows], dtype=np.int64) - 2
        if n < MIN_PASS_PAIRS and not fp32:
            fill = int(np.argmin(np.maximum(nq, 0) + np.maximum(npp, 0)))          # padding pairs: copies of the shortest one
            q_rows = np.concatenate([q_rows, np.full(MIN_PASS_PAIRS - n, q_rows[fill])])
            p_rows = np.concatenate([p_rows, np.full(MIN_PASS_PAIRS - n, p_rows[fill])])
            nq = np.concatenate([nq, np.full(MIN_PASS_PAIRS - n, nq[fill])])
            npp = np.concatenate([npp, np.full(MIN_PASS_PAIRS - n, npp[fill])])
        keep_q, keep_p, lengths, cu = pair_lengths(nq, npp, max_len)
        q_tok, q_lens, q_idx = _device_rows(q_cache, q_rows, dev)
        p_tok, p_lens, p_idx = _device_rows(p_cache, p_rows, dev)

        def i32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        ids, types, pos = ops.build_pairs(q_tok, q_lens, p_tok, p_lens, q_idx, p_idx, i32(keep_q), i32(keep_p), i32(cu), int(cu[-1]))
        cls = self.encoder.encode(None, None, train=False, lengths=lengths.tolist(), packed=(ids, types, pos, max_len), fp32=fp32)
        return self.scores(self._head(cls))[:n]
