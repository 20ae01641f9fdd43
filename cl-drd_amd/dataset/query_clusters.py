"""Cluster the training queries for topic-aware batches (``trainer.nway_listwise --tas_clusters``): encode them with the query tower,
k-means the embeddings on the device (``cldrd_amd.cluster.kmeans``), write ``qid<TAB>cluster``.

    python -m cldrd_amd.dataset.query_clusters --resume CKPT --model_name_or_path M --tokenizer_name_or_path T --queries_path Q \\
        --n_clusters K --output_path OUT.tsv [--training_path FILE] [--iters 20] [--seed 0] [--max_length 32] [--fp32_encode]
        [--apply_consine_similarity]

``--training_path``: only the queries that training file names (its ``qid`` fields) are encoded and clustered.  A cosine checkpoint's rows
are unit rows (``retrieval_utils.cosine_of``, as in retrieve_top_passages).  Outputs: ``OUT.tsv`` in the order of the queries file,
``OUT.tsv.centroids.npy`` (fp32 [K, d]) and ``OUT.tsv.meta.json`` (k, iters, seed, n, d, n_empty, moved per round, smallest / median /
largest cluster size).  Nothing about retrieval quality is claimed: the file decides who shares a batch, nothing else."""
from __future__ import annotations

import argparse
import json
import os


def get_args(argv=None):
    ap = argparse.ArgumentParser(description="k-means of the query embeddings -> qid<TAB>cluster (for --tas_clusters)")
    ap.add_argument("--resume", default="")
    ap.add_argument("--model_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--tokenizer_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--queries_path", required=True)
    ap.add_argument("--training_path", default=None, help="cluster only the queries this training file names")
    ap.add_argument("--n_clusters", required=True, type=int)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--iters", default=20, type=int)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--max_length", default=32, type=int)
    ap.add_argument("--is_parallel", default=True)
    ap.add_argument("--share_weights", action="store_true", default=False)
    ap.add_argument("--fp32_encode", action="store_true", default=False, help="encode with the exact fp32 evaluation pass")
    ap.add_argument("--apply_consine_similarity", "--apply_cosine_similarity", dest="apply_consine_similarity", action="store_true", default=False)
    args = ap.parse_args(argv)
    if args.n_clusters < 1 or args.iters < 0:
        ap.error("--n_clusters must be >= 1 and --iters >= 0")
    return args


def training_qids(path):
    """the ``qid`` of every line of a training file (any label mode: every line is a JSON object with a qid)"""
    out = set()
    with open(path) as fh:
        for line in fh:
            if line.strip():
                out.add(int(json.loads(line)["qid"]))
    return out


def main(args):
    import numpy as np
    import torch
    from transformers import AutoTokenizer

    from ..cluster import kmeans
    from ..models.nway_dual_encoder import NwayDualEncoder
    from ..retriever.index_text import load_checkpoint_into
    from ..retriever.retrieval_utils import cap_host_threads, get_embeddings_from_scratch, set_score_mode
    from .sequence_dataset import SequenceDataset

    tokenizer = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path)
    dataset = SequenceDataset.create_from_seqs_file(args.queries_path, tokenizer, args.max_length, is_query=True)
    if args.training_path:
        keep = training_qids(args.training_path)
        rows = [i for i, q in enumerate(dataset.ids) if q in keep]
        dataset = SequenceDataset([dataset.ids[i] for i in rows], [dataset.seqs[i] for i in rows], tokenizer, args.max_length, is_query=True)
    n = len(dataset)
    if args.n_clusters > n:          # before the model is loaded
        raise ValueError(f"--n_clusters {args.n_clusters} is larger than the number of queries to cluster ({n})")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    cap_host_threads()
    model = NwayDualEncoder(args.model_name_or_path, share_weights=args.share_weights)
    ckpt = load_checkpoint_into(model, args.resume, args.is_parallel) if args.resume else None
    set_score_mode(model, ckpt, args.apply_consine_similarity)
    del ckpt
    model.cuda()
    loader = torch.utils.data.DataLoader(dataset, batch_size=512, shuffle=False, num_workers=0, collate_fn=dataset.collate_fn)
    embs, ids = get_embeddings_from_scratch(model, loader, use_fp16=not args.fp32_encode, is_query=True)
    assert list(ids) == list(dataset.ids)
    x = torch.from_numpy(np.ascontiguousarray(embs, dtype=np.float32)).cuda()
    res = kmeans(x, args.n_clusters, iters=args.iters, seed=args.seed)
    assign, sizes = res.assign.cpu().numpy(), res.sizes.cpu()          # the only read-backs: after the last round
    parent = os.path.dirname(os.path.abspath(args.output_path))
    os.makedirs(parent, exist_ok=True)
    with open(args.output_path, "w") as fh:
        fh.write("".join(f"{q}\t{c}\n" for q, c in zip(ids, assign.tolist())))
    np.save(args.output_path + ".centroids.npy", res.centroids.cpu().numpy())
    meta = {"k": args.n_clusters, "iters": args.iters, "seed": args.seed, "n": n, "d": int(x.shape[1]), "n_empty": int(res.n_empty.item()),
            "moved": res.moved.cpu().tolist(), "size_min": int(sizes.min()), "size_median": int(sizes.median()), "size_max": int(sizes.max())}
    with open(args.output_path + ".meta.json", "w") as fh:
        json.dump(meta, fh)
    print(f"query_clusters: {n} queries, {args.n_clusters} clusters, sizes {meta['size_min']} / {meta['size_median']} / {meta['size_max']} "
          f"(min / median / max), {meta['n_empty']} empty in the last update")
    return meta


if __name__ == "__main__":
    main(get_args())
