#!/usr/bin/env python3
"""Digest of what the flat index (retriever.retrieval_utils) computes, for comparing two commits bit for bit: for fixed seeds and a handful
of cases that between them take every path of attach and search in the three row modes, one line per case with the SHA-256 of ``D`` and of
``I``, the ``last_stats`` counts (without ``search_ms``) and the SHA-256 of every file ``write_index`` writes for the attached index in the compact
format of its own ``row_dtype`` (int8 rows: ``int8=True`` - ``R8``, the scales, ``mu`` and the bound's norms; fp16 rows, and the fp16 shadow of an
fp32-row index: ``fp16=True`` - ``mu``, the fp16 rows and both norms).  Only the public surface is used, so the same file runs on either commit; the outputs must be equal line for
line.

    timeout -k 10 600 python tools/index_digest.py [--out FILE]

One process, one GPU; not to be re-run after a fault before its cause is known."""
import argparse
import hashlib
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cldrd_amd.synthetic as syn
from cldrd_amd.retriever import retrieval_utils as RU

DEV = torch.device("cuda", 0)
LINES = []


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def file_sha(path) -> str:
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def clean(stats):
    if "shards" in stats:
        return [clean(s) for s in stats["shards"]]
    return {k: stats[k] for k in sorted(stats) if k != "search_ms"}


def files(index, tmp) -> str:
    path = os.path.join(tmp, "digest.index")
    written = lambda: sorted(f for f in os.listdir(tmp) if f.startswith("digest.index."))
    for f in written():                          # the previous case's files
        os.remove(os.path.join(tmp, f))
    RU.write_index(index, path, **({"int8": True} if index.row_dtype == "int8" else {"fp16": True}))
    return " ".join(f"{f[len('digest.index.'):]} {file_sha(os.path.join(tmp, f))}" for f in written())


def report(name, index, q, k, tmp):
    D, I = index.search(q, k)
    shards = getattr(index, "shards", None)
    written = files(index, tmp) if shards is None else " | ".join(files(sh, tmp) for sh in shards)
    line = f"{name}: D {sha(D)} I {sha(I)} stats {clean(index.last_stats)} files {written}"
    print(line, flush=True)
    LINES.append(line)
    return D, I


def host_index(emb, ids=None, id_offset=0, **hooks):
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    index.id_offset = id_offset
    for name, value in hooks.items():
        setattr(index, name, value)
    return index


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    RU.cap_host_threads()
    with tempfile.TemporaryDirectory() as tmp:
        # 1. exhaustive
        emb, q = syn.corpus_embeddings(1, 3000, 128), syn.corpus_embeddings(2, 40, 128)
        report("1 exhaustive 3000x128 k10", RU.convert_index_to_gpu(host_index(emb), 0, False), q, 10, tmp)
        report("13 exhaustive 3000x128 k10 int8-row", host_index(emb).to_gpu(0, int8_rows=True), q, 10, tmp)
        # 2. probe pass at QT = 128, with an id table, both modes; 8. the fp16-row file of the second one read back and attached
        emb, q = syn.corpus_embeddings(3, 20000, 128) + np.float32(0.2), syn.corpus_embeddings(4, 300, 128)
        ids = np.arange(20000, dtype=np.int64) * 3 + 5
        for fp16 in (False, True):
            index = RU.convert_index_to_gpu(host_index(emb, ids), 0, fp16)
            report(f"2 probe 20000x128 nq300 k100 ids {'fp16-row' if fp16 else 'fp32'}", index, q, 100, tmp)
        path = os.path.join(tmp, "case8.index")
        RU.write_index(index, path, fp16=True)
        report("8 fp16-row file read back and attached", RU.convert_index_to_gpu(RU.read_index(path), 0, False), q, 100, tmp)
        # 10. the same in int8-row mode; 11. its int8-row file read back and attached
        index = host_index(emb, ids).to_gpu(0, int8_rows=True)
        report("10 probe 20000x128 nq300 k100 ids int8-row", index, q, 100, tmp)
        path = os.path.join(tmp, "case11.index")
        RU.write_index(index, path, int8=True)
        report("11 int8-row file read back and attached", RU.convert_index_to_gpu(RU.read_index(path), 0, False), q, 100, tmp)
        # 3. several passes at QT = 256, with and without the probe pass
        emb, q = syn.corpus_embeddings(5, 60000, 768), syn.corpus_embeddings(6, 700, 768)
        for hooks in ({}, {"probe": False}):
            report(f"3 60000x768 nq700 k100 {hooks or 'default'}", RU.convert_index_to_gpu(host_index(emb, **hooks), 0, False), q, 100, tmp)
        # 4. a full 256-query tile at k = 1000 on a small index (the densest hit lists the scan sees): half the queries are searched again
        emb, q = syn.corpus_embeddings(41, 20000, 768), syn.corpus_embeddings(42, 256, 768)
        report("4 dense tile 20000x768 nq256 k1000", RU.convert_index_to_gpu(host_index(emb), 0, False), q, 1000, tmp)
        # 5. the exact fallback
        emb = syn.corpus_embeddings(45, 40000, 128)
        emb[1000:10000] = emb[1000]
        q = np.repeat(emb[1000:1001] * 3.0, 3, axis=0).astype(np.float32)
        q[1] += syn.corpus_embeddings(46, 1, 128)[0] * 0.01
        index = RU.convert_index_to_gpu(host_index(emb), 0, False)
        attempts, RU.MAX_ATTEMPTS = RU.MAX_ATTEMPTS, 3
        try:
            report("5 fallback 40000x128 9000 identical rows k1000 MAX_ATTEMPTS=3", index, q, 1000, tmp)
        finally:
            RU.MAX_ATTEMPTS = attempts
        # 6. device rows, fp16-row mode, three chunks; 12. the same rows in int8-row mode
        P, u = syn.cls_like_corpus(150000, 768, 91, DEV)
        q = syn.cls_like_queries(10, u, 92).cpu().numpy()
        report("6 from_device_rows 150000x768 fp16-row k100", RU.FlatIPIndex.from_device_rows(P, id_offset=11, fp16_rows=True), q, 100, tmp)
        report("12 from_device_rows 150000x768 int8-row k100", RU.FlatIPIndex.from_device_rows(P, id_offset=11, int8_rows=True), q, 100, tmp)
        del P
        # 7. two shards on one device, both modes
        emb = syn.corpus_embeddings(83, 30001, 128) + np.float32(0.3) * (np.arange(30001, dtype=np.float32)[:, None] / 30001)
        q = syn.corpus_embeddings(84, 12, 128)
        for fp16 in (False, True):
            report(f"7 [0, 0] 30001x128 id_offset 500 k50 {'fp16-row' if fp16 else 'fp32'}",
                   RU.convert_index_to_gpu(host_index(emb, id_offset=500), [0, 0], fp16), q, 50, tmp)
        # 9. a CLS-like shard of bench size at k = 1000: kept sets beyond the default buffer, the probe pass grows it
        P, u = syn.cls_like_corpus(1105228, 768, 93, DEV)
        q = syn.cls_like_queries(700, u, 94).cpu().numpy()
        for fp16 in (False, True):
            report(f"9 cls-like 1105228x768 nq700 k1000 {'fp16-row' if fp16 else 'fp32'}", RU.FlatIPIndex.from_device_rows(P, fp16_rows=fp16), q, 1000, tmp)
        del P
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
