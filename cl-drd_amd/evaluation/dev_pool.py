"""The dev run a student is validated on while it trains, prepared ONCE: the distinct ``(qid, pid)`` pairs of a ``qid pid [rank] [score]``
run file (``retriever.rerank_top_passages.read_run``: queries in order of first appearance, a query's first ``top_k`` distinct pids in run
order), the distinct queries and the distinct passages OF THE RUN tokenised once (not the collection: 1000 dev queries x 200 candidates
are ~190 k of 8.8 M passages), and the padded candidate table ``ops.topk_rescore`` takes.

Scoring a model against the pool (:meth:`DevPool.score`): every distinct query through ``model.query_embs``, every distinct passage through
``model.passage_embs`` with its token count (the batch is packed), both in ``(length, pool position)`` order in batches of a fixed
``batch_size``; the embeddings stay in HBM (1000 x 200 at width 768: ~0.6 GB) and the pairs are scored by the flat search's exact re-score,
so

    score(q, p) = fp32 of the fp64-accumulated inner product of the two fp32 CLS embeddings
                  (of a cosine model, ``model.cosine``: of the two unit vectors ``x / max(||x||, 1e-8)``, ``cldrd_l2_normalize_rows``)

is the number ``FlatIPIndex.search`` returns for the same vectors, bit for bit: a student re-rank of the student's own retrieval run
reproduces that run's scores.  There is one implementation of that sum in the package (``cldrd_topk_rescore``), on purpose.  The result is a
function of (weights, pool files, ``top_k``, ``batch_size``, the model's arithmetic mode) - no loader workers, no state of earlier calls."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import hip_ops as ops
from ..dataset.sequence_dataset import SequenceTokenCache
from ..retriever.rerank_top_passages import group_pairs, length_batches, read_run

RESCORE_CHUNK = 65535        # queries per cldrd_topk_rescore launch: the kernel's grid has the query on blockIdx.y


def candidate_table(group, starts, p_pos):
    """(counts int32 [nq], cand_rows int32 [nq, cap]): row g holds the passage positions of query g's pairs in run order, -1 behind them."""
    counts = np.diff(starts).astype(np.int32)
    cap = max(int(counts.max()) if counts.shape[0] else 0, 1)
    table = np.full((counts.shape[0], cap), -1, dtype=np.int32)
    table[group, np.arange(group.shape[0]) - starts[group]] = p_pos
    return counts, table


def rescore_chunks(nq, chunk=None):
    """[(first query, end)] of the re-score launches: at most RESCORE_CHUNK queries each."""
    chunk = int(RESCORE_CHUNK if chunk is None else chunk)
    return [(a, min(nq, a + chunk)) for a in range(0, nq, chunk)]


class DevPool:
    def __init__(self, run_path, queries_path, collection_path, tokenizer, query_max_len, passage_max_len, top_k=0, token_cache_dir=None):
        self.run_path = str(run_path)
        self.query_max_len, self.passage_max_len, self.top_k = int(query_max_len), int(passage_max_len), int(top_k)
        self._set_pairs(*read_run(self.run_path, self.top_k))
        cache_dir = token_cache_dir or None
        self.q_tokens, self.q_lens = self._tokens(queries_path, self.query_ids, tokenizer, self.query_max_len, cache_dir)
        self.p_tokens, self.p_lens = self._tokens(collection_path, self.passage_ids, tokenizer, self.passage_max_len, cache_dir)

    @classmethod
    def from_pairs(cls, qids, pids, token_source, query_max_len, passage_max_len, name="<arrays>"):
        """A pool without files (timing tools): the pairs as ``read_run`` returns them from ``qid pid`` lines in this order, tokens from
        ``token_source(which, ids, max_len) -> (tokens int32 [n, max_len], lens int32 [n])`` for the distinct queries ("q") / passages ("p")."""
        self = cls.__new__(cls)
        self.run_path, self.top_k = name, 0
        self.query_max_len, self.passage_max_len = int(query_max_len), int(passage_max_len)
        self._set_pairs(*group_pairs(qids, pids)[:4])
        self.q_tokens, self.q_lens = token_source("q", self.query_ids, self.query_max_len)
        self.p_tokens, self.p_lens = token_source("p", self.passage_ids, self.passage_max_len)
        return self

    def _set_pairs(self, qids, pids, group, starts):
        self.qids, self.pids, self.group, self.starts = qids, pids, group, starts
        self._batches = {}
        # queries arrive grouped in order of first appearance: query g of the table is the query of the pairs starts[g] .. starts[g + 1]
        self.query_ids = self.qids[self.starts[:-1]]
        up, first, inv = np.unique(self.pids, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        pos_of = np.empty(up.shape[0], dtype=np.int64)
        pos_of[by_first] = np.arange(up.shape[0])
        self.passage_ids = up[by_first]                            # distinct passages in order of first appearance
        self.p_pos = pos_of[inv.reshape(-1)]                       # pair -> passage position
        self.counts, self.cand_rows = candidate_table(self.group, self.starts, self.p_pos)

    n_pairs = property(lambda self: int(self.qids.shape[0]))
    n_queries = property(lambda self: int(self.query_ids.shape[0]))
    n_passages = property(lambda self: int(self.passage_ids.shape[0]))

    # ---- tokens -------------------------------------------------------------------------------------------------------------
    def _missing(self, key):
        return KeyError(f"id {int(key)} of {self.run_path} is not in the query / passage table")

    def _tokens(self, path, keys, tokenizer, max_len, cache_dir):
        """(tokens int32 [n, max_len] zero padded, lens int32 [n]) of the ``id\\ttext`` rows ``keys``: from an existing sequence token cache
        of the file (built by index_text / rerank_top_passages at the same length with the same tokenizer), else tokenised here."""
        if cache_dir:
            stem = SequenceTokenCache.stem_for(cache_dir, str(path), max_len)
            if os.path.exists(stem + ".meta.json"):
                try:
                    cache = SequenceTokenCache.load(stem, SequenceTokenCache.source_meta(str(path), tokenizer, max_len))
                except ValueError:
                    cache = None                                   # another file / tokenizer / length: not ours to rebuild
                if cache is not None:
                    return self._tokens_from_cache(cache, keys, max_len)
        need = {int(k): i for i, k in enumerate(keys.tolist())}
        texts = [None] * len(need)
        with open(path) as fh:
            for ln, line in enumerate(fh):
                a = line.strip().split("\t")
                if len(a) < 2:
                    continue
                i = need.get(int(a[0]))
                if i is None:
                    continue
                if len(a) == 2:
                    texts[i] = a[1]                                # a repeated id keeps its last text, as the reference's dict does
                elif len(a) == 3:                                  # pid, title, para (reference dataset/utils.py:13-28)
                    texts[i] = a[1] + " " + tokenizer.sep_token + " " + a[2]
                else:
                    raise ValueError(f"{path}:{ln + 1}: expected 'id<TAB>text'")
        for k, i in need.items():
            if texts[i] is None:
                raise self._missing(k)
        tokens = np.zeros((len(texts), max_len), dtype=np.int32)
        lens = np.zeros(len(texts), dtype=np.int32)
        for a in range(0, len(texts), 8192):
            enc = tokenizer(texts[a:a + 8192], padding=False, truncation="longest_first", max_length=int(max_len))["input_ids"]
            for r, t in enumerate(enc, start=a):
                tokens[r, :len(t)] = t
                lens[r] = len(t)
        return tokens, lens

    def _tokens_from_cache(self, cache, keys, max_len):
        ck = np.asarray(cache.keys)
        order = np.argsort(ck, kind="stable")
        at = np.searchsorted(ck[order], keys)
        at = np.minimum(at, max(ck.shape[0] - 1, 0))
        bad = np.nonzero(ck[order][at] != keys)[0] if ck.shape[0] else np.arange(keys.shape[0])
        if bad.size:
            raise self._missing(keys[bad[0]])
        rows = order[at]
        by_row = np.argsort(rows, kind="stable")                   # ascending rows: sequential reads of the memory map
        tokens = np.zeros((keys.shape[0], max_len), dtype=np.int32)
        tokens[by_row] = np.asarray(cache.ids[rows[by_row]]).astype(np.int32)
        return tokens, np.asarray(cache.lens)[rows].astype(np.int32)

    # ---- scoring ------------------------------------------------------------------------------------------------------------
    def _host_batches(self, which, batch_size):
        """[(positions int64 tensor, batch dict on the host)] of one side in (length, pool position) order, made once per batch size"""
        key = (which, int(batch_size))
        if key not in self._batches:
            tokens, lens = (self.q_tokens, self.q_lens) if which == "q" else (self.p_tokens, self.p_lens)
            out = []
            for rows in length_batches(lens, int(batch_size)):           # (length, pool position) order
                ln = lens[rows].astype(np.int64)
                width = int(ln.max())
                ids = torch.from_numpy(tokens[rows, :width].astype(np.int64))
                mask = torch.from_numpy((np.arange(width)[None, :] < ln[:, None]).astype(np.int64))
                out.append((torch.from_numpy(rows.astype(np.int64)), {"input_ids": ids, "attention_mask": mask, "lengths": ln.tolist()}))
            self._batches[key] = out
        return self._batches[key]

    def _encode(self, model, which, batch_size, dev):
        out = None
        n = self.n_queries if which == "q" else self.n_passages
        for rows, batch in self._host_batches(which, batch_size):
            b = {k: (v.to(dev, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            reps = model.query_embs(b) if which == "q" else model.passage_embs(b)
            if out is None:
                out = torch.empty(n, reps.shape[1], dtype=torch.float32, device=dev)
            out.index_copy_(0, rows.to(dev, non_blocking=True), reps.float())
        return out

    def score(self, model, batch_size=512, timings=None):
        """np.float32 [n_pairs]: the score of every pair, in pool order.  The caller provides the evaluation state (eval mode, no_grad);
        ``timings`` (a dict): filled with ``query_encode_s`` / ``passage_encode_s`` / ``score_s``, each ended by a device synchronisation."""
        import time
        if int(batch_size) < 1:
            raise ValueError("batch_size is at least 1")
        if self.n_pairs == 0:
            return np.zeros(0, dtype=np.float32)
        dev = next(model.parameters()).device
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            if timings is not None:
                torch.cuda.synchronize(dev)
                now = time.perf_counter()
                timings[name] = now - t0
                t0 = now
        q_emb = self._encode(model, "q", batch_size, dev)
        lap("query_encode_s")
        p_emb = self._encode(model, "p", batch_size, dev)
        if getattr(model, "cosine", False):
            # a cosine model: the pool's rows become unit vectors where they lie (the kernel the index's rows went through), so the re-score
            # below is the cosine - still the number FlatIPIndex.search returns for these vectors
            ops.l2_normalize_rows(q_emb)
            ops.l2_normalize_rows(p_emb)
        lap("passage_encode_s")
        scores = self.score_embeddings(q_emb, p_emb)
        lap("score_s")
        return scores

    def score_embeddings(self, q_emb, p_emb):
        """The pairs' scores from device-resident fp32 embeddings (query g / passage position p in the rows of the two tensors)."""
        nq, cap = self.cand_rows.shape
        if q_emb.shape[0] != nq or p_emb.shape[0] != self.n_passages or q_emb.shape[1] != p_emb.shape[1]:
            raise ValueError("score_embeddings: one row per distinct query / passage of the pool, same width")
        dev = q_emb.device
        q_emb, p_emb = q_emb.contiguous(), p_emb.contiguous()
        counts = torch.from_numpy(self.counts).to(dev)
        cand = torch.from_numpy(self.cand_rows).to(dev)
        out = torch.zeros(nq, cap, dtype=torch.float32, device=dev)
        for a, b in rescore_chunks(nq):
            ops.topk_rescore(q_emb[a:b], p_emb, counts[a:b], cand[a:b], out[a:b])
        return out.cpu().numpy()[self.group, np.arange(self.n_pairs) - self.starts[self.group]]
