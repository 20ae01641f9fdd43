"""One job per curriculum stage: from a student checkpoint to the next stage's training file in one process on one GPU - what
``retriever.retrieve_top_passages``, ``retriever.rerank_top_passages`` and ``dataset.curriculum_file`` do as three programs that hand each
other run files (100.6 M lines each at 503 k queries x top-200).

    python -m cldrd_amd.retriever.build_stage_file --resume CKPT --model_name_or_path STUDENT --tokenizer_name_or_path TOK [--share_weights] \\
        --index_path IDX [--use_float16 | --use_int8] --queries_path Q.tsv --collection_path C.tsv [--query_max_len 30] [--top_k 200] \\
        --teacher_name_or_path DIR [--teacher_tokenizer_name_or_path TOK] [--teacher_max_len 256] [--teacher_batch_size 2048] \\
        [--token_cache_dir DIR] --label_mode M [--most_hard_ranks LO:HI] [--semi_hard_ranks LO:HI] [--n_most_hard N] [--seed S] \\
        [--with_scores] --output_path train.json [--student_run_path RUN] [--teacher_run_path RUN] \\
        [--score_store DIR [--score_store_flush_pairs N]]

``--score_store DIR``: teacher scores are taken from the store ``DIR`` (``retriever.score_store``, shared with ``rerank_top_passages``) where
it holds the pair; only the others are scored, and added to it.  Every file written is the same, byte for byte.

The search's ids and the teacher's scores stay dense ``[queries, top_k]`` arrays in HBM from the search to the selection
(``dataset.curriculum_file.select_examples_device``, one kernel launch); the host sees the ids once (to find the passages' token-cache rows,
with array operations) and the selected examples.  ``--output_path`` is byte for byte the file the three programs produce from the same
inputs (``--top_k`` of the retrieve, ``--max_len`` = ``--teacher_max_len``, the same windows and seed); ``--student_run_path`` /
``--teacher_run_path`` also write the two run files those programs write, through the same writers, for whoever keeps them.

The windows are validated before anything is loaded.  ``ValueError``: a queries file that holds a qid twice (the three programs merge such
lines in ways that differ from program to program), and an index with fewer rows than ``--top_k`` (there the retrieve pads with id -1,
which the teacher step then fails to find in the collection).  The index's ids must be distinct, as the collection's are.

One process, one GPU; ``retriever.index_text`` stays its own step."""
from __future__ import annotations

import argparse
import os
import tempfile
import time

import numpy as np
import torch

from ..dataset import curriculum_file as C


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="retrieve the training queries' top-k with the student, score them with the teacher, select "
                                             "one label mode's curriculum examples on the GPU and write the training file")
    ap.add_argument("--resume", default="", help="trainer checkpoint (checkpoint_<step>.pth.tar) loaded into the student")
    ap.add_argument("--model_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--tokenizer_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--share_weights", action="store_true", default=False)
    ap.add_argument("--index_path", required=True, help="the index retriever.index_text built with the same student")
    ap.add_argument("--use_float16", action="store_true", default=False, help="attach the index in fp16-row mode")
    ap.add_argument("--queries_path", required=True)
    ap.add_argument("--collection_path", required=True)
    ap.add_argument("--query_max_len", type=int, default=30, help="retrieve_top_passages --max_length")
    ap.add_argument("--top_k", type=int, default=200)
    ap.add_argument("--teacher_name_or_path", required=True, help="an HF (Distil)BertForSequenceClassification directory")
    ap.add_argument("--teacher_tokenizer_name_or_path", default=None, help="default: --teacher_name_or_path")
    ap.add_argument("--teacher_max_len", type=int, default=256, help="rerank_top_passages --max_len")
    ap.add_argument("--teacher_batch_size", type=int, default=2048, help="pairs per cross-encoder batch")
    ap.add_argument("--token_cache_dir", default="")
    ap.add_argument("--label_mode", required=True, help="2-10: relT / negative counts from dataset.nway_dataset")
    ap.add_argument("--most_hard_ranks", default=None, type=C.parse_window, help="LO:HI teacher ranks (default n_rel+1:100)")
    ap.add_argument("--semi_hard_ranks", default=None, type=C.parse_window, help="LO:HI teacher ranks (default 101:200)")
    ap.add_argument("--n_most_hard", default=None, type=int)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--with_scores", action="store_true", default=False, help="also write the teacher's score of every written pid")
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--student_run_path", default="", help="also write the student's run (what retrieve_top_passages writes)")
    ap.add_argument("--teacher_run_path", default="", help="also write the teacher-ranked run (what rerank_top_passages writes)")
    ap.add_argument("--use_int8", action="store_true", default=False, help="attach the index in int8-row mode (excludes --use_float16)")
    ap.add_argument("--apply_consine_similarity", "--apply_cosine_similarity", dest="apply_consine_similarity", action="store_true", default=False,
                    help="score by cosine similarity even if the checkpoint does not say so (a checkpoint written with the flag is read as one anyway)")
    from .score_store import add_arguments
    add_arguments(ap)
    args = ap.parse_args(argv)
    if args.use_int8 and args.use_float16:
        ap.error("--use_int8 and --use_float16 exclude one another")
    return args


def read_query_ids(path) -> np.ndarray:
    """The ids of an ``id\\ttext`` file in line order (the lines ``SequenceDataset.create_from_seqs_file`` keeps); ``ValueError`` naming the
    first id that occurs twice."""
    ids = []
    with open(path) as fh:
        for line in fh:
            a = line.strip().split("\t")
            if len(a) >= 2:
                ids.append(int(a[0]))
    ids = np.asarray(ids, dtype=np.int64)
    u, first, n = np.unique(ids, return_index=True, return_counts=True)
    if (n > 1).any():
        raise ValueError(f"{path}: qid {int(ids[first[n > 1].min()])} occurs more than once")
    return ids


def cache_rows(keys, ids, what: str) -> np.ndarray:
    """Row of every id of ``ids`` (any shape) in a token cache's ``keys``: one sort of the keys and one binary search, no dict.
    ``KeyError`` naming the first id the table does not hold."""
    keys = np.asarray(keys, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    by_key = np.argsort(keys, kind="stable")
    at = np.minimum(np.searchsorted(keys[by_key], ids), max(keys.shape[0] - 1, 0))
    rows = by_key[at] if keys.shape[0] else np.zeros(ids.shape, dtype=np.int64)
    miss = (keys[rows] != ids) if keys.shape[0] else np.ones(ids.shape, dtype=bool)
    if miss.any():
        raise KeyError(f"id {int(ids[miss][0])} is not in the {what} table")
    return rows


def main(args):
    # 0. validate: a bad window fails here, in milliseconds, before a model, a tokenizer or an index is touched
    spec = C.curriculum_spec(args.label_mode, args.most_hard_ranks, args.semi_hard_ranks, args.n_most_hard)
    k = int(args.top_k)
    if k < 1 or args.teacher_max_len > 256 or args.teacher_batch_size < 1:
        raise ValueError("--top_k and --teacher_batch_size are at least 1, --teacher_max_len at most 256")
    file_qids = read_query_ids(args.queries_path)

    from ..dataset import SequenceDataset, SequenceTokenCache
    from ..models.cross_encoder import CrossEncoder
    from ..models.nway_dual_encoder import NwayDualEncoder
    from .index_text import load_checkpoint_into
    from .rerank_top_passages import score_pairs, score_pairs_stored, write_ranked_run
    from .retrieval_utils import (cap_host_threads, check_index_normalized, convert_index_to_gpu, get_embeddings_from_scratch, read_index,
                                  set_score_mode)
    from .retrieve_top_passages import write_run_file
    from transformers import AutoTokenizer

    torch.cuda.set_device(0)
    cap_host_threads()
    dev = torch.device("cuda", 0)
    timings = {}
    t_last = [time.perf_counter()]

    def lap(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + now - t_last[0]
        t_last[0] = now

    index = read_index(args.index_path)                                # memory-mapped: nothing is read yet
    if index.ntotal < k:
        raise ValueError(f"{args.index_path} holds {index.ntotal} rows, fewer than --top_k {k}")
    lap("index_read_s")

    # 1. encode the queries and search, as retrieve_top_passages does; ids and scores stay in HBM
    model = NwayDualEncoder(args.model_name_or_path, share_weights=args.share_weights)
    ckpt = load_checkpoint_into(model, args.resume) if args.resume else None
    check_index_normalized(index, set_score_mode(model, ckpt, getattr(args, "apply_consine_similarity", False)), args.index_path)
    del ckpt
    model.cuda()
    lap("model_load_s")
    tokenizer = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path)
    dataset = SequenceDataset.create_from_seqs_file(args.queries_path, tokenizer, args.query_max_len, is_query=True)
    loader = torch.utils.data.DataLoader(dataset, batch_size=512, shuffle=False, num_workers=4, collate_fn=dataset.collate_fn)
    query_embs, query_ids = get_embeddings_from_scratch(model, loader, use_fp16=True, is_query=True, show_progress_bar=True)
    del model
    lap("encode_queries_s")
    index = index.to_gpu(0, int8_rows=True) if getattr(args, "use_int8", False) else convert_index_to_gpu(index, 0, bool(args.use_float16))
    lap("index_to_gpu_s")
    q_dev = torch.from_numpy(np.ascontiguousarray(query_embs, dtype=np.float32)).to(dev)
    student_scores, pid = index.search_ids_device(q_dev, k)            # fp32 [nq, k], int64 [nq, k] in HBM
    pid = pid.contiguous()
    nq = pid.shape[0]
    pid_h = pid.cpu().numpy()                                          # the one host copy of the ids: token-cache rows, run files
    del index, q_dev
    lap("search_s")
    if args.student_run_path:
        write_run_file(args.student_run_path, query_ids, pid_h, student_scores.cpu().numpy())
        lap("student_run_file_s")
    del student_scores

    # 2. the teacher's score of every (query, candidate) pair, one fp32 [nq, k] tensor in HBM
    t_tok = AutoTokenizer.from_pretrained(args.teacher_tokenizer_name_or_path or args.teacher_name_or_path)
    teacher = CrossEncoder.from_pretrained(args.teacher_name_or_path, max_len=args.teacher_max_len, eval_only=True).cuda()
    lap("teacher_load_s")
    with tempfile.TemporaryDirectory() as tmp:
        cache_dir = args.token_cache_dir or tmp
        os.makedirs(cache_dir, exist_ok=True)
        q_cache = SequenceTokenCache.open_or_build(cache_dir, args.queries_path, t_tok, args.teacher_max_len)
        p_cache = SequenceTokenCache.open_or_build(cache_dir, args.collection_path, t_tok, args.teacher_max_len)
        lap("token_cache_s")
        q_rows = np.repeat(cache_rows(q_cache.keys, file_qids, "query"), k)
        p_rows = cache_rows(p_cache.keys, pid_h, "passage").reshape(-1)
        lap("map_rows_s")
        if args.score_store:
            from .score_store import TeacherScoreStore, teacher_identity
            with TeacherScoreStore(args.score_store, teacher_identity(teacher, args.teacher_max_len, False, q_cache, p_cache), dev) as store:
                score, st = score_pairs_stored(store, teacher, q_cache, p_cache, torch.from_numpy(file_qids).to(dev),
                                               torch.arange(nq + 1, dtype=torch.int64, device=dev) * k, pid.view(-1), q_rows, p_rows,
                                               args.teacher_max_len, args.teacher_batch_size, args.score_store_flush_pairs)
            score = score.view(nq, k)
            timings["score_store_lookup_s"], timings["score_store_append_s"] = st["lookup_s"], st["append_s"]      # (parts of teacher_score_s)
            print(f"score store {args.score_store}: {st['pairs']} pairs, {st['hits']} hits, {st['scored']} scored, {st['segments']} segments")
        else:
            score = score_pairs(teacher, q_cache, p_cache, q_rows, p_rows, args.teacher_max_len, args.teacher_batch_size).view(nq, k)
        del q_rows, p_rows
    del teacher
    lap("teacher_score_s")

    # 3. select on the device, write
    qid = torch.from_numpy(file_qids).to(dev)
    count = torch.full((nq,), k, dtype=torch.int32, device=dev)
    ex, order = C.select_examples_device(qid, pid, score, count, spec, seed=args.seed, with_scores=bool(args.with_scores))
    lap("select_s")
    n = C.write_examples(args.output_path, ex, with_scores=bool(args.with_scores))
    lap("training_file_s")
    if args.teacher_run_path:
        starts = np.arange(nq + 1, dtype=np.int64) * k
        flat = (order.cpu().numpy().astype(np.int64) + starts[:-1, None]).reshape(-1)
        write_ranked_run(args.teacher_run_path, np.repeat(file_qids, k), pid_h.reshape(-1), np.repeat(np.arange(nq, dtype=np.int64), k), starts,
                         score.reshape(-1).cpu().numpy(), order=flat)
        lap("teacher_run_file_s")
    print(f"wrote {n} queries to {args.output_path}; skipped {ex.n_skipped} with fewer than {spec.min_candidates} candidates")
    print("timings: " + " ".join(f"{name}={v:.3f}" for name, v in timings.items()))
    main.last_timings = timings
    return n, ex.n_skipped


if __name__ == "__main__":
    main(get_args())
