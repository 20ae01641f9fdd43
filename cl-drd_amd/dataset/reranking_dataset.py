"""Input contract of a re-ranking pass over a run file (reference ``dataset/reranking_dataset.py:14-87``): ``(qid, pid)`` pairs of a
``qid pid [rank] [score]`` run file, the query and passage tables, and a ``collate_fn`` that tokenises either the (query, passage) pair
for a cross-encoder (``is_cross_encoder=True``: ``max_len``) or both sides apart for a dual encoder (``query_max_len`` /
``passage_max_len``).  The cross-encoder teacher of this package reads pairs from token caches instead
(``models.cross_encoder.CrossEncoder.score_cached``, ``retriever.rerank_top_passages``); this class is the padded batch path."""
from __future__ import annotations

import torch


def load_queries(path):
    """``qid\\ttext`` lines -> {qid: text} (reference dataset/utils.py:4-11)."""
    qid_to_query = {}
    with open(path) as fh:
        for line in fh:
            qid, query = line.strip().split("\t")
            qid_to_query[int(qid)] = query
    return qid_to_query


def load_passages(path):
    """``pid\\ttext`` or ``pid\\ttitle\\tpara`` lines -> {pid: text or {"title", "para"}} (reference dataset/utils.py:13-28)."""
    pid_to_passage = {}
    with open(path) as fh:
        for line in fh:
            array = line.strip().split("\t")
            if len(array) == 2:
                pid_to_passage[int(array[0])] = array[1]
            elif len(array) == 3:
                pid_to_passage[int(array[0])] = {"title": array[1], "para": array[2]}
            else:
                raise ValueError(f"array {array}, with illegal length")
    return pid_to_passage


class RerankingDataset(torch.utils.data.Dataset):
    """ranking_path lines: ``qid\\tpid\\trank\\tscore``, ``qid\\tpid\\tscore`` or ``qid\\tpid`` (``query_first=False``: pid first)."""

    def __init__(self, ranking_path, queries_path, passages_path, tokenizer, is_cross_encoder, query_first=True, **kwargs):
        self.qid_pid_pairs = []
        with open(ranking_path) as fh:
            for line in fh:
                array = line.strip().split("\t")
                a, b = int(array[0]), int(array[1])
                self.qid_pid_pairs.append((a, b) if query_first else (b, a))
        self.qid_to_query = load_queries(queries_path)
        self.pid_to_passage = load_passages(passages_path)
        self.is_cross_encoder = is_cross_encoder
        if is_cross_encoder:
            self.seq_max_len = kwargs["max_len"]
        else:
            self.query_max_len = kwargs["query_max_len"]
            self.passage_max_len = kwargs["passage_max_len"]
        self.tokenizer = tokenizer

    def __getitem__(self, idx):
        qid, pid = self.qid_pid_pairs[idx]
        query = self.qid_to_query[qid]
        passage = self.pid_to_passage[pid]
        if isinstance(passage, dict):
            passage = passage["title"] + " " + self.tokenizer.sep_token + " " + passage["para"]
        elif not isinstance(passage, str):
            raise ValueError(f"passage {passage} donot have desired format.")
        return {"qid": qid, "pid": pid, "query": query, "passage": passage}

    def __len__(self):
        return len(self.qid_pid_pairs)

    def collate_fn(self, batch):
        qids = [e["qid"] for e in batch]
        pids = [e["pid"] for e in batch]
        queries = [e["query"] for e in batch]
        passages = [e["passage"] for e in batch]
        if self.is_cross_encoder:
            query_passages = self.tokenizer(queries, passages, padding=True, truncation="longest_first", return_tensors="pt",
                                            max_length=self.seq_max_len)
            return {"qid": qids, "pid": pids, "query_passage": query_passages}
        queries = self.tokenizer(queries, padding=True, truncation="longest_first", return_tensors="pt", max_length=self.query_max_len)
        passages = self.tokenizer(passages, padding=True, truncation="longest_first", return_tensors="pt", max_length=self.passage_max_len)
        return {"qid": qids, "pid": pids, "query": queries, "passage": passages}
