"""``evaluation/continue_rerank_evaluator.py`` of the reference (named by its ``scripts/unity/continue_rerank_evaluator.sh``, which gives the
flags; the program itself is not published): validate every checkpoint of a finished (or running) training run after the fact - the
student of each ``checkpoint_<step>.pth.tar`` in ``--resume_folder`` re-ranks the dev run, in step order.

    python -m cldrd_amd.evaluation.continue_rerank_evaluator --resume_folder RUN/models --dev_path RUN.tsv --dev_queries_path Q.tsv \\
        --dev_qrels_path QRELS --collection_path C.tsv --model_name_or_path DIR --tokenizer_name_or_path TOK --output_path OUT.log
        [--share_weights] [--dev_batch_size 512] [--dev_top_k 0] [--dev_qrels_trec] [--query_max_len 30] [--passage_max_len 256]
        [--token_cache_dir DIR]

The dev pool (``evaluation.DevPool``) is built once.  ``OUT.log`` is the table the trainer writes to ``dev_logs.log`` with the same flags
(``epoch step`` + the metric keys + ``seconds``); the best step by ``MRR@10`` (a tie keeps the earlier step) is printed and returned.  One
process, one GPU."""
from __future__ import annotations

import argparse
import os
import re
import time

import torch


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="re-rank a dev run with every checkpoint of a folder; write the metric table, print the best step")
    ap.add_argument("--resume_folder", required=True)
    ap.add_argument("--dev_path", required=True)
    ap.add_argument("--dev_queries_path", required=True)
    ap.add_argument("--dev_qrels_path", required=True)
    ap.add_argument("--collection_path", required=True)
    ap.add_argument("--share_weights", action="store_true", default=False)
    ap.add_argument("--dev_batch_size", type=int, default=512)
    ap.add_argument("--dev_top_k", type=int, default=0)
    ap.add_argument("--dev_qrels_trec", action="store_true", default=False)
    ap.add_argument("--model_name_or_path", default="sebastian-hofstaetter/distilbert-dot-tas_b-b256-msmarco")
    ap.add_argument("--tokenizer_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--query_max_len", type=int, default=30)
    ap.add_argument("--passage_max_len", type=int, default=256)
    ap.add_argument("--token_cache_dir", default=None)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--apply_consine_similarity", "--apply_cosine_similarity", dest="apply_consine_similarity", action="store_true", default=False,
                    help="score by cosine similarity even if the checkpoint does not say so (a checkpoint written with the flag is read as one anyway)")
    return ap.parse_args(argv)


def checkpoints_in_step_order(folder):
    """[(step, path)] of the ``checkpoint_<step>.pth.tar`` files of ``folder``, ascending steps."""
    found = []
    for name in os.listdir(folder):
        m = re.fullmatch(r"checkpoint_(\d+)\.pth\.tar", name)
        if m:
            found.append((int(m.group(1)), os.path.join(folder, name)))
    return sorted(found)


def main(args):
    from transformers import AutoTokenizer
    from ..models.nway_dual_encoder import NwayDualEncoder
    from ..retriever.retrieval_utils import cap_host_threads, set_score_mode
    from .dev_pool import DevPool
    from .reranking_evaluator import RerankingEvaluator, update_dev_best, write_dev_logs
    ckpts = checkpoints_in_step_order(args.resume_folder)
    if not ckpts:
        raise FileNotFoundError(f"no checkpoint_<step>.pth.tar in {args.resume_folder}")
    torch.cuda.set_device(0)
    cap_host_threads()
    tok = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path)
    pool = DevPool(args.dev_path, args.dev_queries_path, args.collection_path, tok, args.query_max_len, args.passage_max_len,
                   top_k=args.dev_top_k, token_cache_dir=args.token_cache_dir)
    evaluator = RerankingEvaluator(args.dev_qrels_path, is_trec=args.dev_qrels_trec)
    model = NwayDualEncoder(args.model_name_or_path, share_weights=args.share_weights).cuda()
    if os.path.exists(args.output_path):
        os.remove(args.output_path)                       # one table per call, with its header
    best = None
    for step, path in ckpts:
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in ckpt["state_dict"].items()})
        set_score_mode(model, ckpt, getattr(args, "apply_consine_similarity", False))        # per checkpoint: each says how it scores
        t0 = time.perf_counter()
        metrics = evaluator.compute_metrics_pool(model, pool, batch_size=args.dev_batch_size)
        epoch = int(ckpt.get("epoch", 0))
        write_dev_logs(args.output_path, epoch, step, metrics, time.perf_counter() - t0)
        best = update_dev_best(args.output_path + ".best.json", best, metrics, step, epoch, path)
    print(f"best step {best['step']} ({best['metric']} = {best['value']:.6f}): {best['checkpoint']}")
    return best


if __name__ == "__main__":
    main(get_args())
