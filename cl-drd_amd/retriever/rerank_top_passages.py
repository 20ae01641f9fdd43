"""Teacher re-scoring of a candidate run file with a cross-encoder (the step of a CL-DRD iteration that makes the next iteration's
training data: every training query's top-k student candidates re-scored by the teacher).

    python -m cldrd_amd.retriever.rerank_top_passages --run_path RUN --queries_path Q.tsv --collection_path C.tsv \\
        --model_name_or_path DIR --tokenizer_name_or_path TOK --output_path OUT [--max_len 256] [--top_k K] [--batch_size B]
        [--token_cache_dir DIR] [--score_store DIR [--score_store_flush_pairs N]]

``--score_store DIR`` (teacher mode only): pairs that the teacher score store ``DIR`` (``retriever.score_store``) holds are not scored again,
the others are scored and added to it - after every N of them, so a killed job has lost at most N; the output file is the same, byte for byte.

``--dual_encoder [--resume CKPT] [--share_weights] [--query_max_len 30] [--passage_max_len 256]`` is the student mode: the same run, files,
``--top_k``, ``--token_cache_dir``, ``--fp32_encode`` and output rules, scored by the dual encoder through ``evaluation.DevPool``.

``RUN``: ``qid pid [rank] [score]`` lines; ``Q.tsv`` / ``C.tsv``: ``id\\ttext``; ``DIR``: an HF BertForSequenceClassification /
DistilBertForSequenceClassification directory.  Both tables are tokenised once into token caches built at ``--max_len`` (kept in
``--token_cache_dir`` when given), pairs are assembled on the GPU from the cache rows and scored in batches of similar length.
Output: ``qid\\tpid\\trank\\tscore`` - queries in order of first appearance in RUN, each query's candidates (its first ``--top_k`` distinct
pids in RUN order) by teacher score descending, ties in RUN order.  The file does not depend on ``--batch_size``
(``CrossEncoder.score_cached``: a pair's score depends on the pair alone).  One process, one GPU.

Host side at the scale of a training set (~100 M pairs): the run is parsed into int64 arrays (~16 bytes a pair), grouped and sorted with
numpy, and written by the native run-file writer when every query has the same number of candidates (the usual top-k run); a ragged run
goes through the writer's Python loop."""
from __future__ import annotations

import argparse
import os
import tempfile

import numpy as np
import torch

from ..dataset import SequenceTokenCache
from ..models.cross_encoder import CrossEncoder, pair_lengths
from .retrieve_top_passages import write_run_file


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="re-score a run file's (query, passage) pairs with a cross-encoder; write the re-ranked run")
    ap.add_argument("--run_path", required=True)
    ap.add_argument("--queries_path", required=True)
    ap.add_argument("--collection_path", required=True)
    ap.add_argument("--model_name_or_path", required=True)
    ap.add_argument("--tokenizer_name_or_path", default=None, help="default: --model_name_or_path")
    ap.add_argument("--max_len", type=int, default=256)
    ap.add_argument("--top_k", type=int, default=0, help="candidates per query, in run order (0: all)")
    ap.add_argument("--batch_size", type=int, default=None,
                    help="pairs per encoder batch (default 2048: profiles/rerank_teacher_timing.txt; fewer than 1024 are padded to 1024); "
                         "--dual_encoder: sequences per encoder batch (default 512)")
    ap.add_argument("--token_cache_dir", default="")
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--fp32_encode", action="store_true", default=False,
                    help="run the cross-encoder body in the exact fp32 evaluation pass (CrossEncoder.score_cached(fp32=True))")
    ap.add_argument("--dual_encoder", action="store_true", default=False,
                    help="student mode: re-score with the dual encoder --model_name_or_path [--resume CKPT] instead of a cross-encoder")
    ap.add_argument("--resume", default="", help="--dual_encoder: trainer checkpoint (checkpoint_<step>.pth.tar) loaded into the student")
    ap.add_argument("--share_weights", action="store_true", default=False)
    ap.add_argument("--apply_consine_similarity", "--apply_cosine_similarity", dest="apply_consine_similarity", action="store_true", default=False,
                    help="--dual_encoder: ""score by cosine similarity even if the checkpoint does not say so (a checkpoint written with the flag is read as one anyway)")
    ap.add_argument("--query_max_len", type=int, default=30)
    ap.add_argument("--passage_max_len", type=int, default=256)
    from .score_store import add_arguments
    add_arguments(ap)
    args = ap.parse_args(argv)
    if args.score_store and args.dual_encoder:
        ap.error("--score_store keeps teacher scores: it cannot be used with --dual_encoder (a student's scores change with every checkpoint)")
    if args.batch_size is None:
        args.batch_size = 512 if args.dual_encoder else 2048
    return args


def query_groups(qid):
    """(group, n_queries): ``group[i]`` int64 = position of line i's query among the distinct qids in order of first appearance."""
    uq, q_first, q_inv = np.unique(qid, return_index=True, return_inverse=True)
    rank_of = np.empty(uq.shape[0], dtype=np.int64)
    rank_of[np.argsort(q_first, kind="stable")] = np.arange(uq.shape[0])
    return rank_of[q_inv.reshape(-1)], uq.shape[0]


def read_run(path, top_k=0):
    """(qids, pids, group, starts) int64: the distinct (qid, pid) pairs of a ``qid pid [rank] [score]`` run file, queries in order of
    first appearance, each query's pids in run order (its first top_k); ``group[i]`` = position of pair i's query in that order, the
    pairs of query g are ``starts[g] .. starts[g + 1]``."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # (an empty file)
        a = np.loadtxt(path, dtype=np.int64, usecols=(0, 1), ndmin=2)
    return group_pairs(a[:, 0], a[:, 1], top_k)[:4]


def group_pairs(qid, pid, top_k=0):
    """:func:`read_run` on the two id columns (int64 arrays, one entry per line): (qids, pids, group, starts, src), ``src[i]`` = the line pair
    i came from."""
    qid, pid = np.asarray(qid, dtype=np.int64), np.asarray(pid, dtype=np.int64)
    # one entry per distinct pair, the first occurrence
    _, first = np.unique(np.stack([qid, pid], 1), axis=0, return_index=True)
    src = np.sort(first)
    qid, pid = qid[src], pid[src]
    # queries by first appearance; pairs grouped by query, run order inside
    group, n_q = query_groups(qid)
    order = np.argsort(group, kind="stable")
    qid, pid, group, src = qid[order], pid[order], group[order], src[order]
    counts = np.bincount(group, minlength=n_q)
    starts = np.zeros(n_q + 1, dtype=np.int64)
    np.cumsum(counts, out=starts[1:])
    if top_k > 0:
        sel = np.arange(qid.shape[0]) - starts[group] < top_k
        qid, pid, group, src = qid[sel], pid[sel], group[sel], src[sel]
        counts = np.minimum(counts, top_k)
        np.cumsum(counts, out=starts[1:])
    return qid, pid, group, starts, src


def length_batches(lengths, batch_size):
    """Pair positions in (length, position) order, cut into batches of at most batch_size pairs."""
    order = np.argsort(np.asarray(lengths), kind="stable")
    return [order[i:i + batch_size] for i in range(0, order.shape[0], batch_size)]


def score_pairs(model, q_cache, p_cache, q_rows, p_rows, max_len, batch_size, fp32=False, on_batch=None):
    """Teacher scores of the pairs (query cache row ``q_rows[i]``, passage cache row ``p_rows[i]``; host int64 arrays) as ONE fp32 device
    tensor [n]: scored in batches of similar pair length (:func:`length_batches`), each batch's scores scattered to the pairs' positions on
    the device - nothing comes to the host per batch.  The batching of this program and of ``retriever.build_stage_file``.
    ``on_batch`` (a test hook): called on the host with the batch's pair count after each batch; a test stops a run between two batches by
    raising from it."""
    q_rows, p_rows = np.asarray(q_rows, dtype=np.int64).reshape(-1), np.asarray(p_rows, dtype=np.int64).reshape(-1)
    _, _, lengths, _ = pair_lengths(np.asarray(q_cache.lens)[q_rows] - 2, np.asarray(p_cache.lens)[p_rows] - 2, max_len)
    scores = None
    for b in length_batches(lengths, batch_size):
        s = model.score_cached(q_cache, p_cache, q_rows[b], p_rows[b], max_len, **({"fp32": True} if fp32 else {}))
        if scores is None:
            scores = torch.empty(q_rows.shape[0], dtype=torch.float32, device=s.device)
        scores.index_copy_(0, torch.from_numpy(b).to(s.device), s)
        if on_batch is not None:
            on_batch(int(b.shape[0]))
    return scores if scores is not None else torch.empty(0, dtype=torch.float32, device=next(model.parameters()).device)


def main_dual_encoder(args):
    """``--dual_encoder``: the run re-scored by the student through an evaluation.DevPool (every distinct query and passage encoded once,
    score = the flat search's exact re-score of the two CLS embeddings); output format and ordering rules as the teacher mode's."""
    from ..evaluation.dev_pool import DevPool
    from ..evaluation.reranking_evaluator import evaluation_state
    from ..models.nway_dual_encoder import NwayDualEncoder
    from .index_text import load_checkpoint_into
    if max(args.query_max_len, args.passage_max_len) > 256 or args.batch_size < 1:
        raise ValueError("--query_max_len / --passage_max_len are at most 256, --batch_size at least 1")
    torch.cuda.set_device(0)
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path or args.model_name_or_path)
    model = NwayDualEncoder(args.model_name_or_path, share_weights=args.share_weights)
    from .retrieval_utils import set_score_mode
    set_score_mode(model, load_checkpoint_into(model, args.resume) if args.resume else None, getattr(args, "apply_consine_similarity", False))
    model.cuda()
    model.eval_fp32 = bool(args.fp32_encode)
    pool = DevPool(args.run_path, args.queries_path, args.collection_path, tokenizer, args.query_max_len, args.passage_max_len,
                   top_k=args.top_k, token_cache_dir=args.token_cache_dir)
    with evaluation_state(model):
        scores = pool.score(model, args.batch_size)
    total = write_ranked_run(args.output_path, pool.qids, pool.pids, pool.group, pool.starts, scores)
    print(f"re-scored {total} pairs of {pool.n_queries} queries")
    return total


def score_pairs_stored(store, model, q_cache, p_cache, row_qid, starts, pid, q_rows, p_rows, max_len, batch_size, flush_pairs, fp32=False,
                       on_batch=None):
    """:func:`score_pairs` through a ``score_store.TeacherScoreStore``: the pairs of the CSR batch (``row_qid`` int64 [nq], ``starts`` int64
    [nq + 1], ``pid`` int64 [n], on the device; ``q_rows`` / ``p_rows`` their cache rows, host arrays) that the store holds are not scored,
    the others are scored in global pair-length order and added to it.  Returns (scores fp32 [n] on the device, stats)."""
    from .score_store import score_through_store
    q_rows, p_rows = np.asarray(q_rows, dtype=np.int64).reshape(-1), np.asarray(p_rows, dtype=np.int64).reshape(-1)
    _, _, lengths, _ = pair_lengths(np.asarray(q_cache.lens)[q_rows] - 2, np.asarray(p_cache.lens)[p_rows] - 2, max_len)

    def score_chunk(at):
        return score_pairs(model, q_cache, p_cache, q_rows[at], p_rows[at], max_len, batch_size, fp32=fp32, on_batch=on_batch)
    return score_through_store(store, row_qid, starts, pid, lengths, score_chunk, flush_pairs)


def main(args, on_batch=None):
    """``on_batch`` (a test hook): handed to :func:`score_pairs`."""
    if getattr(args, "dual_encoder", False):
        if getattr(args, "score_store", ""):
            raise ValueError("--score_store cannot be used with --dual_encoder")
        return main_dual_encoder(args)
    if args.max_len > 256 or args.batch_size < 1:
        raise ValueError("--max_len is at most 256, --batch_size at least 1")
    torch.cuda.set_device(0)
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path or args.model_name_or_path)
    model = CrossEncoder.from_pretrained(args.model_name_or_path, max_len=args.max_len, eval_only=True).cuda()
    qids, pids, group, starts = read_run(args.run_path, args.top_k)
    with tempfile.TemporaryDirectory() as tmp:
        cache_dir = args.token_cache_dir or tmp
        os.makedirs(cache_dir, exist_ok=True)
        q_cache = SequenceTokenCache.open_or_build(cache_dir, args.queries_path, tokenizer, args.max_len)
        p_cache = SequenceTokenCache.open_or_build(cache_dir, args.collection_path, tokenizer, args.max_len)
        q_row = {int(k): i for i, k in enumerate(np.asarray(q_cache.keys))}
        p_row = {int(k): i for i, k in enumerate(np.asarray(p_cache.keys))}
        try:
            uq, q_inv = np.unique(qids, return_inverse=True)
            q_rows = np.array([q_row[int(q)] for q in uq], dtype=np.int64)[q_inv.reshape(-1)]
            up, p_inv = np.unique(pids, return_inverse=True)
            p_rows = np.array([p_row[int(p)] for p in up], dtype=np.int64)[p_inv.reshape(-1)]
        except KeyError as exc:
            raise KeyError(f"id {exc.args[0]} of {args.run_path} is not in the query / passage table") from exc
        fp32 = bool(getattr(args, "fp32_encode", False))
        if getattr(args, "score_store", ""):
            from .score_store import TeacherScoreStore, teacher_identity
            dev = torch.device("cuda", torch.cuda.current_device())
            with TeacherScoreStore(args.score_store, teacher_identity(model, args.max_len, fp32, q_cache, p_cache), dev) as store:
                scores, st = score_pairs_stored(store, model, q_cache, p_cache, torch.from_numpy(qids[starts[:-1]]).to(dev),
                                                torch.from_numpy(starts).to(dev), torch.from_numpy(pids).to(dev), q_rows, p_rows,
                                                args.max_len, args.batch_size, args.score_store_flush_pairs, fp32=fp32, on_batch=on_batch)
                scores = scores.cpu().numpy()
            print(f"score store {args.score_store}: {st['pairs']} pairs, {st['hits']} hits, {st['scored']} scored, {st['segments']} segments")
        else:
            scores = score_pairs(model, q_cache, p_cache, q_rows, p_rows, args.max_len, args.batch_size, fp32=fp32,
                                 on_batch=on_batch).cpu().numpy()
    total = write_ranked_run(args.output_path, qids, pids, group, starts, scores)
    print(f"re-scored {total} pairs of {starts.shape[0] - 1} queries")
    return total


def rank_order(group, scores):
    """Positions of the pairs in output order: queries as they are, inside a query score descending, ties in run order (the pairs arrive
    grouped by query in run order) - what the reference's stable sort does."""
    scores = np.asarray(scores)
    return np.lexsort((np.arange(scores.shape[0]), -scores.astype(np.float64), group))


def write_ranked_run(path, qids, pids, group, starts, scores, order=None):
    """``qid\\tpid\\trank\\tscore`` of the pairs of :func:`read_run` ranked by :func:`rank_order`: the native writer when every query has the
    same number of candidates (the usual top-k run), the writer's Python loop for a ragged run.  ``order``: the pairs' positions in output
    order when the caller already has them (``build_stage_file``: from the selection kernel) - what :func:`rank_order` would return."""
    if order is None:
        order = rank_order(group, scores)
    pids, scores = pids[order], np.ascontiguousarray(np.asarray(scores)[order], dtype=np.float32)
    q_out = qids[starts[:-1]]
    counts = np.diff(starts)
    if counts.shape[0] and (counts == counts[0]).all() and counts[0] > 0:
        return write_run_file(path, q_out.tolist(), pids.reshape(-1, counts[0]), scores.reshape(-1, counts[0]))
    return write_run_file(path, q_out.tolist(), [pids[a:b].tolist() for a, b in zip(starts[:-1], starts[1:])],
                          [scores[a:b].tolist() for a, b in zip(starts[:-1], starts[1:])])


if __name__ == "__main__":
    main(get_args())
