"""``retriever.retrieval_utils`` of the reference (``retriever/retrieval_utils.py``) on MI355X.

Same call surface: ``get_embeddings_from_scratch`` (:30-58), ``construct_flatindex_from_embeddings`` (:116-129),
``index_retrieve`` (:131-153), ``convert_index_to_gpu`` (:155-184).  faiss is replaced by :class:`FlatIPIndex`
(``IndexIDMap(IndexFlatIP)`` semantics: exact fp32 inner product, results sorted by score descending, ids mapped,
missing results id -1) whose ``search`` runs on the GPU, device resident from the query upload to the result download:

    0. queries             : one H2D copy; fp16 / bf16 copies and norms in one kernel
    1. threshold estimate  : bf16 MFMA scores of the queries against a strided row sample -> per-query k_s-th largest = est_q;
                             thr_q = est_q - 2 eps_q  (a heuristic: it only decides how many candidates the scan emits)
    2. scan                : fp16 MFMA scores of 128 queries against the fp16 shadow of the whole shard, streamed once through
                             LDS (HBM-bound: 2 B per index element per 128-query batch); (row, score) pairs >= thr_q are kept
    3. select              : t^_q = k-th largest scan score; only rows with scan score >= t^_q - 2 eps_q can be in the exact
                             top-k, where eps_q >= |scan score - exact score| bounds the fp16 rounding of both operands
                             (2^-10 |q| max|p|), the fp32 accumulation and fp16 underflow (csrc/topk.hip: thresholds_kernel)
    4. exact re-score      : fp32 dot products of those rows from the fp32 rows (what faiss would have computed); in fp16-row mode
                             (``useFloat16=True``, :class:`FlatIPIndex`) from the stored fp16 rows - there are no fp32 rows then
    5. sort + cut          : (score desc, row position asc) -> top-k
    6. proof of exactness  : per query ON THE DEVICE: the list is complete down to t^_q - 2 eps_q (thr_q <= that, >= k candidates,
                             no overflow, no dropped hit).  The host reads the flags once per search; a query that fails is
                             searched again with a corrected threshold (rare: the estimate is 4.5 sigma conservative).

Steps 2-6 of every 128-query batch are enqueued back to back by one C-ABI call (``cldrd_flatip_search``): no host round trip,
no allocation inside the search.

Multi-GPU: one process per GPU, rank r holds the contiguous row shard r; queries are replicated;
each rank returns its shard's top-k with GLOBAL ids and rank 0 merges (score desc, tie -> global row position asc): on the device
when the lists arrive over RCCL, by a native multi-threaded host merge otherwise (:class:`ShardedFlatIPIndex`).
The faiss sharding code of the reference (:164-182) is dead (undefined ``gpu_resources``); this is the design it intended.
"""
from __future__ import annotations

import dataclasses
import math
import os
import pickle
import warnings
from timeit import default_timer as timer
from types import SimpleNamespace

import numpy as np
import torch

from .. import hip_ops as ops

SAMPLE_ROWS = 16384          # rows scored for the threshold estimate (a heuristic: 4x fewer rows cost ~20 % more candidates, which
                             # only the cheap select sees, and make the estimate 4x cheaper)
CAND_CAP = 8192              # candidate slots per query (LDS limit of cldrd_topk_select / cldrd_topk_sort)
QUERY_TILE = 128             # the reference searches in batches of 128 (retrieve_top_passages.py:88); at d = 768 two such batches
                             # share one pass over the index (FlatIPIndex.query_tile = 256: the index bytes are read once per 256 queries)
EST_CHUNK = 1024             # queries per threshold-estimate GEMM
MAX_ATTEMPTS = 12
ATTACH_CHUNK_ROWS = 65536    # fp16-row mode: fp32 rows reach the GPU in chunks of this many rows (two staging buffers), never as a whole
HOST_CHUNK_ROWS = 16384      # fp16-row file written from a host index: rows converted per numpy step
FORMAT_F32 = "cldrd-flatip-v1"
FORMAT_F16 = "cldrd-flatip-f16-v1"
FORMAT_I8 = "cldrd-flatip-i8-v1"
PROGRESS_HOOK = None         # tools: callable(timings dict) every 500 batches of get_embeddings_from_scratch
_MERGE_DEVICE, _MERGE_HOST = "device (cldrd_merge_topk_device)", "host (cldrd_merge_topk)"       # last_merge["path"] of a sharded search


def cap_host_threads(limit: int = 8):
    """The host side of every batch is a handful of tiny CPU tensor ops between kernel launches.  torch sizes its intra-op pool to the
    machine (128 threads on a 256-CPU MI355X host): waking that pool costs MILLISECONDS per op (an int64 sum over a 32 k-element mask:
    18 ms, measured, profiles/r06_microbench.txt section 8), and eight rank processes would each own such a pool.  The command lines
    (trainer, index_text, retrieve_top_passages) cap it; a library user's process is left alone."""
    if torch.get_num_threads() > limit:
        torch.set_num_threads(limit)


def batch_to_device(batch, target_device: torch.device):
    seq = batch.get("seq") if hasattr(batch, "get") else None
    if seq is not None and hasattr(seq, "keys") and "lengths" not in seq and isinstance(seq.get("attention_mask"), torch.Tensor) \
            and not seq["attention_mask"].is_cuda:
        # token counts while the mask is still on the host: the encoder packs the batch (HipEncoder.encode) - the tokenizer pads every
        # sequence to the longest of its batch of 512, about half of the rows of an MS MARCO batch
        # (numpy on the zero-copy view: one thread; torch's intra-op pool on a 256-CPU host takes milliseconds to wake for such a reduction)
        m = seq["attention_mask"].numpy()
        lens = np.count_nonzero(m, axis=-1).reshape(-1)
        if m.ndim == 2 and np.array_equal(m != 0, np.arange(m.shape[1])[None, :] < lens[:, None]):       # right-padded, as HF tokenizers pad
            seq = dict(seq.items())
            batch["seq"] = seq
            seq["lengths"] = lens.tolist()
    for key in batch:
        if isinstance(batch[key], torch.Tensor):
            batch[key] = batch[key].to(target_device, non_blocking=True)          # asynchronous when the loader pinned the batch
        if isinstance(batch[key], dict) or hasattr(batch[key], "keys"):
            for sub_key in batch[key]:
                if isinstance(batch[key][sub_key], torch.Tensor):
                    batch[key][sub_key] = batch[key][sub_key].to(target_device, non_blocking=True)
    return batch


def cosine_of(checkpoint, flag: bool = False) -> bool:
    """Whether a model built from ``checkpoint`` (the loaded dict of a trainer checkpoint, or None) scores by cosine similarity: it does if
    the checkpoint's ``score`` key says so (written by a trainer run with --apply_consine_similarity) or if the program's own
    --apply_consine_similarity (``flag``) is given - as an --index_fp16 file is searched in its mode with or without the flag."""
    score = checkpoint.get("score") if isinstance(checkpoint, dict) else None
    return bool(flag) or (isinstance(score, dict) and score.get("kind") == "cosine")


def set_score_mode(model, checkpoint, flag: bool = False) -> bool:
    """``model.cosine`` (and the checkpoint's ``cosine_scale``) from `cosine_of`: the one call of every program that builds a model from
    ``--resume``.  -> model.cosine"""
    model.cosine = cosine_of(checkpoint, flag)
    score = checkpoint.get("score") if isinstance(checkpoint, dict) else None
    if model.cosine and isinstance(score, dict) and "scale" in score:
        model.cosine_scale = float(score["scale"])
    return model.cosine


def check_index_normalized(index, cosine: bool, index_path: str = ""):
    """A cosine model searches unit rows: refuse an index without the ``normalized`` mark of index_text.  (An index of unit rows searched
    with a dot-product model is an ordinary inner-product search and is not refused.)"""
    if cosine and not getattr(index, "normalized", False):
        raise ValueError(f"the model scores by cosine similarity, but the index {index_path} holds raw rows (its .meta.pkl has no "
                         "'normalized' mark): rebuild it with index_text from the same checkpoint (or with --apply_consine_similarity)")


def get_embeddings_from_scratch(model, dataloader, use_fp16, is_query, show_progress_bar=False, normalize=None):
    """Encode every batch of ``dataloader`` ({"seq": {input_ids, attention_mask}, "id": list[int]}) with the query or
    passage tower in eval mode -> (np.float32 [n, D], list[int]).

    ``use_fp16`` is the reference's flag (:30-58: autocast only when it is set).  True: the towers' 16-bit evaluation pass (fp16 operands in
    the FFN / out-projection GEMMs, bf16 QKV / attention, fp32 accumulate, fp32 residual stream, fp32 CLS output).  False: the exact fp32
    evaluation pass (``HipEncoder.encode(fp32=True)``: fp32 operands on the f32-input MFMA, weights read from the fp32 master copy) - the
    model's ``eval_fp32`` is set for the duration of the call and restored afterwards, also when the loader raises; a model without that
    attribute is left alone.  The output is fp32 in both modes (the reference's too, :56).

    The host side of the loop is timed (``get_embeddings_from_scratch.last_timings``, seconds): ``load_s`` waiting for the loader (tokens
    from the cache / tokeniser), ``h2d_enqueue_s`` moving the batch and enqueuing the encode, ``d2h_wait_s`` waiting for the PREVIOUS
    batch's embeddings (the GPU's encode of it, as far as the host sees it: one batch of D2H stays in flight), ``gather_s`` collecting the
    rows.  When the loader knows its row count (``dataset.n_rows``: the token-cache and synthetic datasets) the [n, D] result is allocated
    once and filled in place; the reference appends per-batch arrays and concatenates 27 GB at the end (:51).

    ``normalize`` (ours; None: ``getattr(model, "cosine", False)``): every row leaves as ``x / max(||x||, 1e-8)``, taken on the device
    (``cldrd_l2_normalize_rows``) in front of the D2H copy: inner products of what is returned are cosines."""
    normalize = bool(getattr(model, "cosine", False)) if normalize is None else bool(normalize)
    if use_fp16 or not hasattr(model, "eval_fp32"):
        return _embeddings_from_scratch(model, dataloader, is_query, normalize)
    before = model.eval_fp32
    model.eval_fp32 = True
    try:
        return _embeddings_from_scratch(model, dataloader, is_query, normalize)
    finally:
        model.eval_fp32 = before


def _embeddings_from_scratch(model, dataloader, is_query, normalize=False):
    """The loop of :func:`get_embeddings_from_scratch` in whichever arithmetic mode the model is in."""
    import time
    tm = {"load_s": 0.0, "h2d_enqueue_s": 0.0, "d2h_wait_s": 0.0, "gather_s": 0.0, "batches": 0}
    embeddings, embeddings_ids = [], []
    model.eval()
    dev = next(model.parameters()).device
    n_rows = getattr(getattr(dataloader, "dataset", None), "n_rows", None)
    out, filled = None, 0
    pending = None

    out_ids = None

    def collect(p):
        nonlocal out, filled, out_ids
        t0 = time.perf_counter()
        p[1].synchronize()
        t1 = time.perf_counter()
        a = p[0].numpy()
        if n_rows is not None:
            if out is None:
                out = np.empty((int(n_rows), a.shape[1]), dtype=np.float32)
            if p[2] is not None:
                # a length-bucketed batch (CachedSequenceDataset(bucket_window=...)): its rows go back to their positions in the collection
                rows = np.asarray(p[2], dtype=np.int64)
                if out_ids is None:
                    out_ids = np.full(int(n_rows), -1, dtype=np.int64)
                out[rows] = a
                out_ids[rows] = np.asarray(p[3], dtype=np.int64)
            else:
                out[filled:filled + a.shape[0]] = a
            filled += a.shape[0]
        else:
            embeddings.append(a.copy())
        tm["d2h_wait_s"] += t1 - t0
        tm["gather_s"] += time.perf_counter() - t1
    t_prev = time.perf_counter()
    for _, batch in enumerate(dataloader):
        t0 = time.perf_counter()
        tm["load_s"] += t0 - t_prev
        with torch.no_grad():
            batch = batch_to_device(batch, dev)
            reps = model.query_embs(batch["seq"]) if is_query else model.passage_embs(batch["seq"])
            if normalize:
                reps = ops.l2_normalize_rows(reps, torch.empty(reps.shape, dtype=torch.float32, device=reps.device))
            text_ids = batch["id"]
        # keep one batch in flight: the D2H copy of batch i overlaps the encode of batch i+1 (the reference syncs per batch, :47)
        host = torch.empty(reps.shape, dtype=torch.float32, pin_memory=True)
        host.copy_(reps, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        tm["h2d_enqueue_s"] += time.perf_counter() - t0
        if pending is not None:
            collect(pending)
        rows = batch.get("row") if (n_rows is not None and hasattr(batch, "get")) else None
        pending = (host, ev, rows, text_ids if rows is not None else None)
        assert isinstance(text_ids, list)
        if rows is None:
            embeddings_ids.extend(text_ids)
        tm["batches"] += 1
        if PROGRESS_HOOK is not None and tm["batches"] % 500 == 0:
            PROGRESS_HOOK(tm)
        t_prev = time.perf_counter()
    if pending is not None:
        collect(pending)
    t0 = time.perf_counter()
    if n_rows is not None and out is not None:
        if filled != out.shape[0]:
            raise RuntimeError(f"the loader announced {out.shape[0]} rows and delivered {filled}")
        embeddings = out
        if out_ids is not None:
            if embeddings_ids:
                raise RuntimeError("a loader must deliver either every batch with row positions or none")
            embeddings_ids = out_ids.tolist()
    else:
        embeddings = np.concatenate(embeddings)
    tm["gather_s"] += time.perf_counter() - t0
    get_embeddings_from_scratch.last_timings = tm
    assert len(embeddings_ids) == embeddings.shape[0]
    assert isinstance(embeddings_ids[0], int)
    print(f"# nan in embeddings: {np.sum(np.isnan(embeddings))}")
    return embeddings, embeddings_ids


@dataclasses.dataclass
class _Resident:
    """What an attached shard keeps in HBM and what the search needs to know about it.  Built completely by ``FlatIPIndex._attach`` and
    never changed afterwards, except for the lazily filled members at the end."""
    device: torch.device
    mode: str                    # "float32" | "float16" | "int8": the key of ``_MODES``, which says which of the row tensors below exist
    n: int                       # rows of the shard
    mu: torch.Tensor             # fp32 [d]: mean row of the shard
    sample: torch.Tensor         # bf16 [s_rows rounded up to 8, d]: every s_stride-th centred row (threshold estimate)
    s_stride: int
    s_rows: int
    cnorm: float                 # max |p - mu| (int8-row mode: of the stored centred rows, max_r a_r |R8[r]|_2)
    raw_max: float               # max |p|
    max_norm: float              # the norm the eps bound multiplies (FlatIPIndex._attach)
    query_tile: int              # queries per pass over the index bytes
    p16: object = None           # float32 / float16: fp16 [n, d] = fp16(p - mu), what the scan reads; in fp16-row mode also the stored rows
    p32: object = None           # float32: fp32 [n, d], the rows the re-score reads
    r8: object = None            # int8: int8 [n, d], the quantised centred rows (scan operand AND stored rows) ...
    scale: object = None         # ... and fp32 [n], their scales a_r: the stored row is mu + a_r R8[r]
    b1: float = 0.0              # int8: max_r a_r |R8[r]|_1, what the query-digit term of eps multiplies
    ids_dev: object = None       # int64 [n]: the id table, uploaded by the first search that maps ids
    mu_host: object = None       # np.float32 [d]: the host copy of mu, made when first asked for
    ws: dict = dataclasses.field(default_factory=dict)       # cap2 -> per-batch scratch of the search


@dataclasses.dataclass
class _StoredRows:
    """The stored rows of fp16-row or int8-row mode on the host, as their file holds them: what ``FlatIPIndex.read`` keeps of such a file
    (``rows`` memory-mapped) and what ``FlatIPIndex.write`` writes, from a file, from an attached shard or freshly encoded."""
    mode: str                    # "float16" | "int8"
    rows: np.ndarray             # np.float16 [n, d] = fp16(p - mu) | np.int8 [n, d] = R8
    scale: object                # int8: np.float32 [n], the scales a_r; float16: None
    mu: np.ndarray               # np.float32 [d]
    cnorm: float                 # max |p - mu| | max_r a_r |R8[r]|_2
    raw_max: float               # max |p|
    b1: float = 0.0              # int8: max_r a_r |R8[r]|_1


@dataclasses.dataclass
class _ScanQueries:
    """The queries as the scan reads them: the fp16 copy ``qh`` [nq, d], or - int8-row mode - the digit planes ``qd`` int8 [2, nq, d] and their
    common scale ``sq`` [nq].  Empty for a search that does not scan (exhaustive)."""
    qh: object = None
    qd: object = None
    sq: object = None

    def select(self, sel) -> "_ScanQueries":         # the queries ``sel`` (a slice or an index tensor)
        qd = self.qd
        if qd is not None:
            qd = (qd[:, sel] if isinstance(sel, slice) else qd.index_select(1, sel)).contiguous()
        return _ScanQueries(_sel(self.qh, sel), qd, _sel(self.sq, sel))


def _host_tensor(a: np.ndarray) -> torch.Tensor:
    """torch view of a host array that is only the source of an upload and never written through (a memory-mapped index file is read-only)"""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        return torch.from_numpy(a)


def _sel(t, sel):
    """the entries ``sel`` (a slice or an index tensor) of a per-query tensor that may be None"""
    return None if t is None else (t[sel] if isinstance(sel, slice) else t.index_select(0, sel))


def _all_missing(nq: int, k: int):
    return np.full((nq, k), -np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64)


def _check_queries(queries, d: int, k):
    """-> (fp32 contiguous queries [nq, d], int k, the (empty) result of an empty query set or None)"""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != d:
        raise ValueError("queries must be [nq, d]")
    k = int(k)
    if k <= 0:
        raise ValueError("k must be positive")
    return q, k, (_all_missing(0, k) if q.shape[0] == 0 else None)


def _cap2_after_probe(cap2: int, status: np.ndarray, kept: np.ndarray) -> int:
    """Slots of the kept-set buffer for the passes after the probe pass, from the probe's status words and kept-set sizes: the smallest
    power-of-two multiple of ``cap2`` with 25 % + 64 slots of headroom over the largest kept set (``CAND_CAP`` at most, and ``CAND_CAP``
    when a probe query's kept set did not fit: status bit 16)."""
    need = int(kept.max()) if ((status & 16) == 0).all() else CAND_CAP
    cap2_rest = cap2
    while cap2_rest < min(CAND_CAP, int(1.25 * need) + 64):
        cap2_rest *= 2
    return min(cap2_rest, CAND_CAP)


def _retry_step(status: np.ndarray, thr: np.ndarray, eps: np.ndarray, khat: np.ndarray, attempt: int):
    """What a failed proof does to the thresholds of the unproven queries: their status words (bits of cldrd_flatip_search: 1 too few
    candidates, 2 candidate list overflowed, 4 the scan dropped hits, 8 threshold above t^ - 2 eps, 16 the kept set does not fit its
    buffer), thresholds, eps and k-th scan scores (float64) and the attempt number (1, 2, ...) -> (new thresholds float64, scan with the
    tiled kernels, use the full ``CAND_CAP`` kept-set buffer)."""
    t = thr.copy()
    has_k = np.isfinite(khat)
    over = (status & 2) != 0
    few = ((status & 1) != 0) & ~over
    high = ((status & 8) != 0) & ~over & ~few
    # proven bound: the list was complete and long enough, only the threshold sat above t^ - 2 eps
    t[high] = khat[high] - 2.0 * eps[high] * (1.0 + 1e-3) - 1e-6 * np.abs(khat[high]) - 1e-30
    # too few candidates: the estimate was too high; lower it, faster every attempt (but never by more than 8 eps + 20 % at once:
    # a threshold far below t^ only fills the lists)
    t[few] = t[few] - np.minimum(np.maximum(4.0 * eps[few], 0.05 * np.abs(t[few]) + 1e-3) * (2.0 ** (attempt - 1)),
                                 8.0 * eps[few] * attempt + 0.2 * np.abs(t[few]) + 1e-3)
    # overflow: the list holds an arbitrary `cap` of the c rows above thr; its k-th largest score is a (low) estimate of t^
    up = np.where(has_k, khat - 2.0 * eps, -np.inf)
    t[over] = np.maximum(t[over] + np.maximum(eps[over], 1e-3 * np.abs(t[over])) * (2.0 ** (attempt - 1)), up[over])
    # status bit 4: the streaming scan dropped hits (its per-wave on-chip lists overflowed inside one tile: hit density above
    # ~5 % of a tile, e.g. k = 1000 on an index of a few 10k rows).  Every query of such a pass carries the bit and the same
    # kernel would drop the same hits again: the retry scans with the tiled kernels, which have no on-chip list.  Queries with
    # ONLY that bit (or bit 16: a larger buffer, not another threshold) keep their threshold.
    return t, bool(((status & 4) != 0).any()), bool(((status & 16) != 0).any())


# ---- the three row modes: everything that differs between them, from the file to the chained search, is stated here and nowhere else ----
_EXCLUSION = {"FlatIPIndex.to_gpu": "FlatIPIndex.to_gpu: fp16_rows and int8_rows exclude one another",
              "FlatIPIndex.from_device_rows": "FlatIPIndex.from_device_rows: fp16_rows and int8_rows exclude one another",
              "FlatIPIndex.write": "FlatIPIndex.write: fp16 and int8 exclude one another",
              "write_index": "write_index: int8=True excludes faiss_format=True and fp16=True (the int8-row format is this package's own)"}
_NOT_FINITE16 = "FlatIPIndex: embeddings must be finite and inside the fp16 range (|x| <= 65504) for the scan shadow"
_NOT_FINITE8 = "FlatIPIndex: embeddings must be finite for the int8 rows"


def _requested_mode(fp16: bool, int8: bool, who: str) -> str:
    """The row mode a caller's two flags ask for; ``who`` (a key of ``_EXCLUSION``) names the caller in the refusal of both at once."""
    if fp16 and int8:
        raise ValueError(_EXCLUSION[who])
    return "int8" if int8 else ("float16" if fp16 else "float32")


def _attach_mode(holds, requested: str) -> str:
    """The mode ``to_gpu`` attaches in: the stored rows of a file (``holds`` "float16" / "int8") as they are, fp32 rows ("float32") as ``requested``."""
    if (holds, requested) == ("float16", "int8"):
        raise ValueError("FlatIPIndex.to_gpu: this index holds fp16 rows only (read from an fp16-row file): int8 rows are quantised from fp32 rows")
    if holds in ("float16", "int8"):
        return holds
    if holds is None and requested != "float32":
        raise ValueError("FlatIPIndex.to_gpu: the index holds no rows")
    return requested


def _check16(d, n, fresh):
    """the shard a 16-bit attach takes; ``fresh``: fp16-row mode made from fp32 rows (the mean-row kernel's limit applies, the fp32 form keeps its own)"""
    if d % 4:
        raise ValueError("FlatIPIndex: the embedding width must be a multiple of 4")
    if fresh and d > 2048:
        raise ValueError(f"FlatIPIndex: fp16-row mode supports an embedding width of at most 2048 (the mean-row kernel's limit), got {d}")
    if fresh and n <= 0:
        raise ValueError("FlatIPIndex: no rows to attach")


def _check8(d, n=1, fresh=True):
    if d % 64 or d > 2048 or d <= 0:
        raise ValueError(f"FlatIPIndex: int8-row mode supports an embedding width that is a multiple of 64 and at most 2048, got {d}")
    if n <= 0:
        raise ValueError("FlatIPIndex: no rows to attach")


def _upload_rest8(st, dest, sample, s_stride, s_rows):      # the scales as they are; the sample rows are dequantised on the host
    dest["scale"].copy_(_host_tensor(np.ascontiguousarray(st.scale, dtype=np.float32)))
    for lo in range(0, s_rows, HOST_CHUNK_ROWS):
        sel = np.arange(lo, min(s_rows, lo + HOST_CHUNK_ROWS)) * s_stride
        rows = st.scale[sel][:, None] * np.asarray(st.rows[sel], dtype=np.float32)       # fp32 products, as the device forms them
        sample[lo:lo + sel.size].copy_(torch.from_numpy(rows).to(torch.bfloat16))


def _encode16(chunk, mu):
    c = np.asarray(chunk, dtype=np.float32) - mu                  # fp32 subtraction, as the device does it
    if not (np.abs(c) <= 65504.0).all():
        raise ValueError(_NOT_FINITE16)
    return c.astype(np.float16), None, 0.0, float(np.einsum("ij,ij->i", c, c, dtype=np.float64).max())          # round to nearest even


def _prep16(q32, qb, qnorm, flag):
    qh = torch.empty(q32.shape, dtype=torch.float16, device=q32.device)
    ops.topk_prep_queries(q32, qh, qb, qnorm, flag)
    return _ScanQueries(qh=qh)


def _prep8(q32, qb, qnorm, flag):
    qs = _ScanQueries(qd=torch.empty(2, *q32.shape, dtype=torch.int8, device=q32.device), sq=torch.empty(q32.shape[0], dtype=torch.float32, device=q32.device))
    ops.topk_prep_queries_i8(q32, qs.qd, qb, qs.sq, qnorm, flag)
    return qs


# One record per mode.  Storage: `rows_field` names the _Resident member the scan reads (in the two compact modes also the stored rows), `new_rows`
# allocates the mode's resident row tensors as a dict of _Resident members; `file_format` / `rows_ext` / `np_dtype` / `bad_file`: the mode's file.
# Attach (FlatIPIndex._attach is the skeleton): `check(d, n, fresh)` refuses a shard (fresh: made from fp32 rows, not uploaded from a file),
# `alloc_first`: the resident tensors are allocated before the statistics walk, `convert`: the per-chunk op over `n_maxima` running maxima, which
# `norms(values) -> (cnorm, b1)` reads, `upload_rest` finishes an upload from a file (the sample), `max_norm`: the norm eps multiplies.  Host writer:
# `host_check(d)`, `encode(chunk, mu) -> (rows, scales or None, chunk max of the l1 bound, chunk max of the squared centred norm)`.  Search: `prep`
# makes the queries' scan operand, `bound` runs the threshold / eps op, `chain` the chained search over the rows `rows` of the shard; `qmu`: scores
# are <q, mu> + ... of the stored rows; `status_mask`: the status bits that count; `bad_queries`: the refusal of the range flag.
_MODES = {"float16": SimpleNamespace(
    rows_field="p16", new_rows=lambda n, d, dev: {"p16": torch.empty(n, d, dtype=torch.float16, device=dev)},
    file_format=FORMAT_F16, rows_ext=".emb16.npy", np_dtype=np.float16, bad_file="{path}.emb16.npy: expected float16 [n, {d}]",
    check=_check16, alloc_first=False, n_maxima=1, norms=lambda v: (math.sqrt(v[0]), 0.0),
    # centre + cast: fp16 rows + max centred norm + bf16 sample + range flag in ONE pass per chunk (cldrd_index_center_cast)
    convert=lambda c, mu, dest, lo, sample, s_stride, s_rows, flag, maxima: ops.index_center_cast(
        c, mu, dest["p16"][lo:lo + c.shape[0]], sample, s_stride, s_rows, flag, row0=lo, cmax=maxima[0]),
    upload_rest=lambda st, dest, sample, s_stride, s_rows: ops.gather_cast_rows(dest["p16"], sample, s_rows, s_stride),
    # max |p - mu| for the bound, plus 2^-12 max|p|: the fp32 subtraction p - mu itself rounds (2^-24 |p| per element), which moves a
    # centred score by up to |q| sqrt(d) 2^-24 max|p| < 2^-10 |q| (2^-12 max|p|) - folded into the norm the eps formula multiplies by 2^-10
    # (fp16-row mode: the scan's operand IS the stored row, so that term is slack there; the bound is kept as it is)
    max_norm=lambda cnorm, raw_max: cnorm * (1.0 + 1e-6) + raw_max * 2.0 ** -12,
    # queries per pass over the index bytes: 256 at d = 768 (the streaming scan's two-batch form), else the reference's 128
    # (`query_tile_request`: a test hook that asks for 128 at d = 768)
    query_tile=lambda d, request: 256 if (d == 768 and request != 128) else 128,
    not_finite=_NOT_FINITE16, no_host_rows="FlatIPIndex.write: the index holds no rows", host_check=lambda d: None, encode=_encode16,
    prep=_prep16, bound=lambda res, d, est, sq, qnorm, thr, eps: ops.topk_thresholds(est, qnorm, res.max_norm, d, thr, eps),
    chain=lambda res, rows, q32, qs, thr, eps, qmu, bufs, exhaustive, tiled: ops.flatip_search(
        q32, qs.qh, thr, eps, res.p16[rows], *bufs, exhaustive=exhaustive, qtile=res.query_tile, tiled=tiled, qmu=qmu),
    qmu=True, status_mask=~0, bad_queries="queries must be finite and inside the fp16 range (|x| <= 65504)")}
# the fp32 form: the fp16 rows are the scan's shadow of ONE resident fp32 tensor, which the re-score reads; it has no file of stored rows
_MODES["float32"] = SimpleNamespace(**{
    **vars(_MODES["float16"]), "check": lambda d, n, fresh: _check16(d, n, False), "qmu": False,
    "chain": lambda res, rows, q32, qs, thr, eps, qmu, bufs, exhaustive, tiled: ops.flatip_search(
        q32, qs.qh, thr, eps, res.p16[rows], *bufs, exhaustive=exhaustive, qtile=res.query_tile, tiled=tiled, P32=res.p32[rows])})
_MODES["int8"] = SimpleNamespace(
    rows_field="r8", new_rows=lambda n, d, dev: {"r8": torch.empty(n, d, dtype=torch.int8, device=dev), "scale": torch.empty(n, dtype=torch.float32, device=dev)},
    file_format=FORMAT_I8, rows_ext=".emb8.npy", np_dtype=np.int8, bad_file="{path}.emb8.npy / .scale.npy: expected int8 [n, {d}] and float32 [n]",
    check=_check8, alloc_first=True, n_maxima=2, norms=lambda v: (math.sqrt(v[1]), v[0]),
    # quantise: R8, a, the bf16 sample of the stored centred rows and the two maxima of the bound per chunk (cldrd_index_quantize_i8)
    convert=lambda c, mu, dest, lo, sample, s_stride, s_rows, flag, maxima: ops.index_quantize_i8(
        c, mu, dest["r8"][lo:lo + c.shape[0]], dest["scale"][lo:lo + c.shape[0]], sample, s_stride, s_rows, flag, *maxima, row0=lo),
    # the bound's two norms with the slack of their own fp32 rounding (csrc/topk_i8.hip: thresholds_i8_kernel)
    max_norm=lambda cnorm, raw_max: cnorm * (1.0 + 1e-6), query_tile=lambda d, request: 128, upload_rest=_upload_rest8,
    not_finite=_NOT_FINITE8, no_host_rows="FlatIPIndex.write: the index holds no fp32 rows to quantise", host_check=_check8,
    encode=lambda chunk, mu: (lambda r8, a, l1, l2sq: (r8, a, l1.max(), l2sq.max()))(*FlatIPIndex.quantize_rows_i8(chunk, mu)),
    prep=_prep8, bound=lambda res, d, est, sq, qnorm, thr, eps: ops.topk_thresholds_i8(est, sq, qnorm, res.b1, res.max_norm, d, thr, eps),
    # the int8 scan has no tiled form and no on-chip hit list: a hit is lost only to a full candidate list - bit 2 of THAT query; the
    # dropped-hit counter (bit 4) marks every query of its pass and carries nothing more
    chain=lambda res, rows, q32, qs, thr, eps, qmu, bufs, exhaustive, tiled: ops.flatip_search_i8(
        q32, qs.qd, qs.sq, thr, eps, res.r8[rows], res.scale[rows], qmu, *bufs, exhaustive=exhaustive, qtile=res.query_tile),
    qmu=True, status_mask=~4, bad_queries="queries must be finite")
_FILE_MODES = {m.file_format: name for name, m in _MODES.items() if name != "float32"}


def _host_stats(emb, not_finite: str):
    """The statistics pass of the host encoder over fp32 rows in chunks: -> (mu = fp32 of the fp64 column mean, max |p|^2 in fp64)."""
    colsum, raw_sq = np.zeros(emb.shape[1], dtype=np.float64), 0.0
    for lo in range(0, emb.shape[0], HOST_CHUNK_ROWS):
        c = np.asarray(emb[lo:lo + HOST_CHUNK_ROWS], dtype=np.float32)
        colsum += c.sum(axis=0, dtype=np.float64)
        raw_sq = max(raw_sq, float(np.einsum("ij,ij->i", c, c, dtype=np.float64).max()))
    if not (math.isfinite(raw_sq) and np.isfinite(colsum).all()):
        raise ValueError(not_finite)
    return (colsum / float(emb.shape[0])).astype(np.float32), raw_sq


class FlatIPIndex:
    """Exact inner-product index over one shard of rows (faiss ``IndexIDMap(IndexFlatIP(d))`` semantics).

    Three row modes.  Default (``row_dtype == "float32"``): the fp32 rows are resident next to the fp16 scan shadow and scores are exact fp32
    inner products (6 B per element in HBM).  **fp16-row mode** (``to_gpu(dev, fp16_rows=True)``, ``convert_index_to_gpu(..., useFloat16=True)``,
    or an index read from an fp16-row file; ``row_dtype == "float16"``): the shard keeps ``mu`` (fp32 [d], its mean row) and
    ``R16 = fp16(p - mu)`` (round to nearest even) and nothing else of the rows - 2 B per element.  The stored row is ``mu + R16[r]`` and

        s(q, r) = fp32( sum_j q_j mu_j + sum_j q_j R16[r, j] )          both sums in fp64, one rounding

    i.e. the exact inner product with the stored row; ``search`` returns the top-k of s by (s desc, row position asc), everything else of the
    contract is unchanged.  This differs from faiss' ``useFloat16``, which stores plain ``fp16(p)``: the centred array is the one the scan
    reads anyway (one array serves scan and re-score), and its rounding error is relative to ``|p - mu|`` instead of ``|p|`` - on CLS-like
    embeddings the stored rows are closer to the fp32 ones.  ``mu`` is the fp32 value of the fp64 column mean; a host-written file and a
    device-attached index of the same rows may differ in the last bit of ``mu`` and therefore of a few ``R16`` values.

    **int8-row mode** (``to_gpu(dev, int8_rows=True)`` or an index read from an int8-row file; ``row_dtype == "int8"``; ``d % 64 == 0``,
    ``d <= 2048``): the shard keeps ``mu``, ``R8`` (int8 [n, d]) and ``a`` (fp32 [n]) - ``d + 4`` bytes per row.  With ``c = p - mu`` (fp32):
    ``a_r = max_j |c_j| / 127``, ``R8[r, j] = clamp(rint(c_j / a_r), -127, 127)`` (correctly rounded fp32 divisions, half to even; an all-zero
    ``c`` gives ``a_r = 0``), the stored row is ``mu + a_r R8[r]`` and

        s(q, r) = fp32( sum_j q_j mu_j + a_r sum_j q_j R8[r, j] )       both sums and the product in fp64, one rounding

    The scan runs on the i8 MFMA with the query split into two int8 digits; its integer sums are exact, so the scan's only error is the
    rounding of the query, and the top-k of ``s`` is PROVEN as in the other modes (csrc/topk_i8.hip derives the bound).  What is approximate
    is the stored row, not the search: rankings differ from the fp32 rows' where quantisation moves a score across a neighbour's.

    State.  Host side: ``embeddings`` / ``ids`` / ``id_offset``, or - an index read from an fp16-row or int8-row file - ``_stored``, a
    :class:`_StoredRows` (the rows as the file holds them, ``mu``, the norms of the bound; its ``mode`` is the index's).  Device side: ONE
    :class:`_Resident` in ``_res``, None until an attach has succeeded: :meth:`_attach` assigns it as its last statement, :meth:`add_with_ids`
    drops it; its ``mode`` keys ``_MODES``, the one place that says what differs between the modes.  ``device``, ``query_tile``, ``_p16``,
    ``_p32``, ``_sample`` and ``_max_norm`` are read-only views of it (what bench.py, the tools and the tests read)."""

    def __init__(self, d: int):
        self.d = d
        self.ntotal = 0
        self.embeddings = None       # np.float32 [n, d] on the host until moved to a GPU
        self.ids = None              # np.int64 [n] or None (ids = row positions + id_offset)
        self.id_offset = 0
        self._stored = None          # _StoredRows: an index read from an fp16-row or int8-row file (no fp32 rows anywhere)
        self.normalized = False      # the rows are unit vectors (index_text with a cosine model): written to / read from the meta file
        self._res = None             # _Resident: the attached shard
        self.last_stats = {}
        self.profile = False          # bench.py: time the search with HIP events and count candidates
        self.probe = True             # first pass of a long search sizes the kept-set buffer of the rest (test hook: False)
        self.query_tile_request = None

    device = property(lambda self: None if self._res is None else self._res.device, doc="the GPU the shard is attached to, or None")
    query_tile = property(lambda self: self._res.query_tile, doc="queries per pass over the index bytes (attached index)")
    _p16 = property(lambda self: None if self._res is None else self._res.p16, doc="the resident fp16 rows [n, d], or None")
    _p32 = property(lambda self: None if self._res is None else self._res.p32, doc="the resident fp32 rows, or None (fp16-row mode)")
    _sample = property(lambda self: None if self._res is None else self._res.sample, doc="the resident bf16 threshold sample, or None")
    _max_norm = property(lambda self: self._res.max_norm, doc="the norm the eps bound multiplies (attached index)")

    @property
    def row_dtype(self) -> str:
        """``"float16"``: fp16-row mode (attached with ``fp16_rows=True`` or read from an fp16-row file); ``"int8"``: int8-row mode (attached with
        ``int8_rows=True`` or read from an int8-row file); ``"float32"`` otherwise."""
        return self._stored.mode if self._stored is not None else (self._res.mode if self._res is not None else "float32")

    @property
    def mu(self):
        """The shard's mean row the fp16 rows are centred on: np.float32 [d], read-only (None before the index has one)."""
        if self._res is not None:
            if self._res.mu_host is None:
                self._res.mu_host = self._res.mu.cpu().numpy()
            mu = self._res.mu_host
        elif self._stored is not None:
            mu = self._stored.mu
        else:
            return None
        out = mu.view()
        out.flags.writeable = False
        return out

    # -- construction -----------------------------------------------------------------------------------------
    def add_with_ids(self, embeddings, ids):
        if self._stored is not None:
            raise ValueError(f"an index read from an {self._stored.mode.replace('float', 'fp')}-row file holds no fp32 rows: rows cannot be added to it")
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        if emb.ndim != 2 or emb.shape[1] != self.d:
            raise ValueError("embeddings must be [n, d]")
        ids = None if ids is None else np.asarray(ids).astype(np.int64)
        if ids is not None and ids.shape[0] != emb.shape[0]:
            raise ValueError("ids and embeddings differ in length")
        if self.embeddings is None:
            self.embeddings, self.ids = emb, ids
        else:
            self.embeddings = np.concatenate([self.embeddings, emb])
            self.ids = None if self.ids is None or ids is None else np.concatenate([self.ids, ids])
        self.ntotal = self.embeddings.shape[0]
        self._res = None             # the attached shard is not these rows any more

    def add(self, embeddings):
        self.add_with_ids(embeddings, None)

    @classmethod
    def from_device_rows(cls, rows32: torch.Tensor, id_offset: int = 0, fp16_rows: bool = False, int8_rows: bool = False) -> "FlatIPIndex":
        """Index over fp32 rows that already live in HBM (e.g. an encode shard that never left the GPU).  ``fp16_rows``: centre + cast on the
        device and keep no reference to ``rows32`` (fp16-row mode, class docstring); ``int8_rows``: the same into int8-row mode."""
        mode = _requested_mode(fp16_rows, int8_rows, "FlatIPIndex.from_device_rows")
        idx = cls(rows32.shape[1])
        n = idx.ntotal = rows32.shape[0]
        idx.id_offset = id_offset
        rows32 = rows32.contiguous()
        if mode == "float32":
            idx._attach(rows32.device, n, mode, lambda: ((0, rows32),), keep32=rows32)
        else:
            idx._attach(rows32.device, n, mode, lambda: ((lo, rows32[lo:lo + ATTACH_CHUNK_ROWS]) for lo in range(0, n, ATTACH_CHUNK_ROWS)))
        return idx

    def to_gpu(self, device, fp16_rows: bool = False, int8_rows: bool = False):
        """Make the shard resident in HBM.  Default: fp32 rows (exact re-score), fp16 shadow (scan), bf16 row sample (threshold).
        ``fp16_rows=True`` (or an index read from an fp16-row file, whatever the argument says): fp16-row mode - only ``mu``, the centred fp16
        rows and the sample become resident; the fp32 rows pass through two staging buffers of ``ATTACH_CHUNK_ROWS`` rows.
        ``int8_rows=True`` (or an index read from an int8-row file, whatever the arguments say): int8-row mode - ``mu``, the int8 rows, their
        scales and the sample, staged the same way.  The two flags exclude one another."""
        requested = _requested_mode(fp16_rows, int8_rows, "FlatIPIndex.to_gpu")
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("FlatIPIndex.search runs on the GPU only (no CPU path)")
        stored = self._stored
        mode = _attach_mode(stored.mode if stored is not None else ("float32" if self.embeddings is not None else None), requested)
        if stored is not None:
            self._attach(device, stored.rows.shape[0], mode, None)
        elif mode == "float32":
            rows32 = _host_tensor(np.ascontiguousarray(self.embeddings)).to(device)        # the fp32 form uploads once
            self._attach(device, rows32.shape[0], mode, lambda: ((0, rows32),), keep32=rows32)
        else:
            self._attach(device, self.embeddings.shape[0], mode, lambda: self._staged_chunks(device))
        return self

    def _staged_chunks(self, device):
        """(first row, fp32 device tensor) for every ``ATTACH_CHUNK_ROWS`` rows of the host array (a numpy array or a memory-mapped file), through
        two staging buffers: the H2D copy of chunk i + 1 (a side stream) runs under the kernels the consumer enqueued for chunk i."""
        emb = self.embeddings
        n, d = emb.shape
        m_max = min(n, ATTACH_CHUNK_ROWS)
        cur, side = torch.cuda.current_stream(device), torch.cuda.Stream(device)
        bufs = [torch.empty(m_max, d, dtype=torch.float32, device=device) for _ in range(2 if n > m_max else 1)]
        consumed = [None] * len(bufs)
        side.wait_stream(cur)
        try:
            for i, lo in enumerate(range(0, n, ATTACH_CHUNK_ROWS)):
                hi = min(n, lo + ATTACH_CHUNK_ROWS)
                b = i % len(bufs)
                host = _host_tensor(np.ascontiguousarray(emb[lo:hi], dtype=np.float32))
                with torch.cuda.stream(side):
                    if consumed[b] is not None:
                        side.wait_event(consumed[b])
                    bufs[b][:hi - lo].copy_(host, non_blocking=True)
                    ready = torch.cuda.Event()
                    ready.record(side)
                cur.wait_event(ready)
                yield lo, bufs[b][:hi - lo]
                consumed[b] = torch.cuda.Event()
                consumed[b].record(cur)
        finally:
            cur.wait_stream(side)
            cur.synchronize()            # the staging buffers go back to the allocator only when nothing reads or writes them

    def _shard_stats(self, device, n: int, chunks, one_chunk: bool):
        """First walk of an attach over fp32 chunks: max |p|^2 and the mean row of every chunk (cldrd_row_sqnorm_max, cldrd_index_col_mean: fp64
        column sums) -> (mu on the device, its host copy or None, max |p|)."""
        raw = torch.zeros(1, dtype=torch.int32, device=device)
        means, sizes = [], []
        for lo, c in chunks():
            ops.row_sqnorm_max_into(c, raw)
            means.append(ops.index_col_mean(c))
            sizes.append(c.shape[0])
        del c                        # the last view of a staging buffer: the second walk allocates its own
        raw_max = math.sqrt(float(raw.view(torch.float32).item()))
        if not math.isfinite(raw_max):
            return torch.zeros(self.d, dtype=torch.float32, device=device), None, raw_max
        if one_chunk:
            return means[0], None, raw_max            # one chunk: the device's mean row as it is
        # the chunk means combined on the host in fp64 weighted by chunk size (mu depends neither on the device nor on timing;
        # it need not equal the fp32 mode's mu bit for bit)
        w = np.asarray(sizes, dtype=np.float64)[:, None]
        mu_h = ((torch.stack(means).cpu().numpy().astype(np.float64) * w).sum(axis=0) / float(n)).astype(np.float32)
        return torch.from_numpy(mu_h).to(device), mu_h, raw_max

    def _new_sample(self, device, n: int):
        """-> (s_stride, s_rows, the zeroed bf16 sample buffer).  The threshold sample: SAMPLE_ROWS rows, or 1 / 64 of the rows on a larger index
        (the whole 8.84 M-row collection on one GPU: with 16 384 rows the expected number of sample rows inside the top 1000 is 1.9, the estimate
        is the 9th largest sample score and the candidate lists come out at ~6 300 +- 2 000 of their 8 192 slots: overflowing queries, one or two
        extra passes; with 138 k rows ~2 300).  The GEMM wants a column count that is a multiple of 8: zero rows pad the sample (never read by
        the select)."""
        s_stride = max(1, n // min(max(SAMPLE_ROWS, n // 64), 1 << 18))
        s_rows = min(n, (n + s_stride - 1) // s_stride)
        return s_stride, s_rows, torch.zeros((s_rows + 7) // 8 * 8, self.d, dtype=torch.bfloat16, device=device)

    def _attach(self, device, n: int, mode: str, chunks, keep32=None):
        """Every attach, in row mode ``mode``.  ``chunks()`` yields (first row, fp32 device tensor) over the shard in order and is walked twice
        (statistics, then the mode's conversion: centre + cast, or quantise); the fp32 form is the one-chunk case over the whole tensor, which
        ``keep32`` keeps resident for the re-score.  In the other two modes no fp32 row stays in HBM.  ``chunks=None``: an index read from an
        fp16-row or int8-row file - the stored rows go to HBM as they are (chunked H2D straight into their tensor), the sample is made from
        them, ``mu`` and the norms come from the file: no statistics pass.

        The stored / shadow rows are CENTRED on the shard's mean row mu.  <q, p - mu> = <q, p> - <q, mu> moves every score of a query by the same
        constant, so the ranking - all the scan decides - is unchanged, while the rounding bound of the scan, eps ~ 2^-10 |q| max|p - mu|,
        shrinks with the rows' common component.  Dual-encoder CLS embeddings are dominated by one (reference model: q . p = 17 +- 2 over a
        corpus): on the CLS-like shard of the tests eps goes from 0.042 to 0.007 and the 2 eps band under the k-th score from ~1 250 rows to
        ~200, i.e. the re-score gathers about half the rows and the scan emits half the hits; on an isotropic corpus mu ~ 0 and nothing
        changes.  In fp32 mode the exact scores still come from the untouched fp32 rows (re-score)."""
        d, m = self.d, _MODES[mode]
        stored = self._stored if chunks is None else None
        m.check(d, n, stored is None)
        with torch.cuda.device(device):
            if m.alloc_first:
                (s_stride, s_rows, sample), dest = self._new_sample(device, n), m.new_rows(n, d, device)
            # statistics: max |p|^2 and the mean row of every chunk (cldrd_row_sqnorm_max, cldrd_index_col_mean: fp64 column sums)
            if stored is not None:
                mu_h, raw_max = stored.mu, stored.raw_max
                mu = torch.from_numpy(np.ascontiguousarray(mu_h, dtype=np.float32)).to(device)
            else:
                mu, mu_h, raw_max = self._shard_stats(device, n, chunks, one_chunk=keep32 is not None)
            if not m.alloc_first:
                (s_stride, s_rows, sample), dest = self._new_sample(device, n), m.new_rows(n, d, device)
            if stored is not None:
                cnorm, b1, flag, rows = stored.cnorm, stored.b1, 0, dest[m.rows_field]
                for lo in range(0, n, ATTACH_CHUNK_ROWS):
                    rows[lo:lo + ATTACH_CHUNK_ROWS].copy_(_host_tensor(np.ascontiguousarray(stored.rows[lo:lo + ATTACH_CHUNK_ROWS])))
                m.upload_rest(stored, dest, sample, s_stride, s_rows)
            else:
                flag_d, *maxima = (torch.zeros(1, dtype=torch.int32, device=device) for _ in range(1 + m.n_maxima))
                for lo, c in chunks():
                    m.convert(c, mu, dest, lo, sample, s_stride, s_rows, flag_d, maxima)
                del c
                cnorm, b1 = m.norms([float(t.view(torch.float32).item()) for t in maxima])
                flag = int(flag_d.item())
        if flag or not (math.isfinite(raw_max) and math.isfinite(b1) and math.isfinite(cnorm)):
            raise ValueError(m.not_finite)
        self._res = _Resident(device=device, mode=mode, n=n, mu=mu, sample=sample, s_stride=s_stride, s_rows=s_rows, cnorm=cnorm, raw_max=raw_max,
                              max_norm=m.max_norm(cnorm, raw_max), query_tile=m.query_tile(d, self.query_tile_request), mu_host=mu_h,
                              p32=keep32, b1=b1, **dest)

    # -- search -------------------------------------------------------------------------------------------------
    @staticmethod
    def _cap2(kk: int) -> int:
        """slots for the rows that survive the select (k + the 2 eps band + ties), a power of two for the bitonic sort"""
        need, c = kk + max(512, kk // 2), 1024
        while c < need:
            c *= 2
        return min(c, CAND_CAP)

    def search(self, queries, k: int):
        """(D np.float32 [nq, k] descending, I np.int64 [nq, k]); missing results: id -1, score -inf."""
        if self._res is None:
            raise RuntimeError("index is not on a GPU: call convert_index_to_gpu(index, device) first (no CPU search path)")
        q, k, empty = _check_queries(queries, self.d, k)
        if empty is not None:
            return empty
        with torch.cuda.device(self.device):
            Dd, ids64 = self.search_ids_device(torch.from_numpy(q).to(self.device), k)
            return Dd.cpu().numpy(), ids64.cpu().numpy()

    def search_ids_device(self, q32: torch.Tensor, k: int):
        """:meth:`search` without the two PCIe copies: fp32 queries [nq, d] in HBM -> (D fp32 [nq, k], ids int64 [nq, k]) in HBM
        (row position -> id on the device: IndexIDMap).  What a sharded search gathers over RCCL."""
        res = self._res
        with torch.cuda.device(res.device):
            Dd, Id, stats = self.search_device(q32, int(k))
            if self.ids is not None and res.ids_dev is None:
                res.ids_dev = torch.from_numpy(np.ascontiguousarray(self.ids, dtype=np.int64)).to(res.device)
            ids64 = ops.map_ids(Id, res.ids_dev if self.ids is not None else None, int(self.id_offset))     # one launch (cldrd_map_ids)
        self.last_stats = stats
        return Dd, ids64

    def search_device(self, q32: torch.Tensor, k: int):
        """Search with device-resident fp32 queries [nq, d]; returns device tensors (D fp32 [nq, k], I int32 row positions
        [nq, k], -1 = missing) and the statistics dict.  ONE host synchronisation (the proof flags) when nothing is redone."""
        res = self._res
        m = _MODES[res.mode]
        dev, QT = res.device, res.query_tile
        n, d = res.n, self.d
        nq = q32.shape[0]
        kk = min(k, n)
        exhaustive = n <= CAND_CAP
        if not exhaustive and kk > CAND_CAP // 2:
            raise ValueError(f"top_k = {k} is not supported on an index of {n} rows: the candidate lists hold {CAND_CAP} entries "
                             f"(top_k <= {CAND_CAP // 2}, or an index of at most {CAND_CAP} rows)")
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        # 0. queries: the bf16 copy and the mode's scan operand, norms, range flag; stored-row modes: <q, mu> in fp64, added by the re-score
        q32 = q32.contiguous()
        qb = torch.empty(nq, d, dtype=torch.bfloat16, device=dev)
        qnorm, flag = torch.empty(nq, **f32), torch.zeros(1, **i32)
        qh = m.prep(q32, qb, qnorm, flag)
        qmu = ops.query_dot64(q32, res.mu) if m.qmu else None
        # 1. thresholds
        thr, eps = self._estimate_thresholds(qb, qnorm, kk, exhaustive, sq=qh.sq)
        # 2. the first pass over every query
        stats = dict(scans=0, rescans=0, candidates=0, rescored=0, unproven_first_pass=0, exhaustive=bool(exhaustive))
        cap2 = CAND_CAP if exhaustive else self._cap2(kk)
        D, I = torch.empty(nq, k, **f32), torch.empty(nq, k, **i32)
        if self.profile:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        # How many rows survive the select (k + the 2 eps band) depends on the corpus: ~1.3 k on isotropic embeddings, where the k-th
        # score sits far out in a thin tail, 2-3 k on CLS-like ones, where every row scores close to every other (top-k
        # notes).  A search of more than two passes therefore runs its first pass as a PROBE with the default buffer, reads that pass's
        # kept-set sizes (one extra host sync per search) and sizes the buffer of the remaining passes from them - instead of
        # overflowing it query after query and scanning those a second time.
        probe = 0 if (exhaustive or nq <= 2 * QT or not self.probe) else QT
        if probe:
            head, tail = slice(0, probe), slice(probe, nq)
            first = self._run(q32[head], qh.select(head), thr[head], eps[head], _sel(qmu, head), k, cap2, D[head], I[head])
            pr = torch.stack([first[0], first[2]]).cpu().numpy()
            cap2_rest = _cap2_after_probe(cap2, pr[0], pr[1])
            stats["cap2"] = [cap2, cap2_rest]
            rest = self._run(q32[tail], qh.select(tail), thr[tail], eps[tail], _sel(qmu, tail), k, cap2_rest, D[tail], I[tail])
            st, counts, n2, khat = (torch.cat(pair) for pair in zip(first, rest))
            cap2 = cap2_rest
        else:
            st, counts, n2, khat = self._run(q32, qh, thr, eps, qmu, k, cap2, D, I, exhaustive=exhaustive)
        if self.profile:
            e1.record()
        # 3. the proof flags
        status = st.cpu().numpy()                       # the synchronisation of a search (plus the probe's)
        if int(flag.item()):
            raise ValueError(m.bad_queries)
        status = status & m.status_mask
        nb = (nq + QT - 1) // QT
        stats["scans"] = 0 if exhaustive else nb
        stats["query_tile"] = QT
        if self.profile:
            # pass b keeps its list lengths at counts[(QT + 1) b .. (QT + 1) b + m) and the dropped-hit counter right behind them
            c_all = counts.view(nb, QT + 1)[:, :QT].reshape(-1)[:nq]
            stats["search_ms"] = e0.elapsed_time(e1)
            stats["rescored"] = int(n2.sum().item())
            stats["rescored_max"] = int(n2.max().item())
            stats["candidates"] = int(c_all.clamp(max=CAND_CAP).sum().item())
        bad = np.nonzero(status)[0]
        stats["unproven_first_pass"] = int(bad.size)
        stats["status_bits_first_pass"] = {int(b): int(((status & b) != 0).sum()) for b in (1, 2, 4, 8, 16) if ((status & b) != 0).any()}
        stats["fallback_queries"] = 0
        # 4. the proof loop: unproven queries are searched again as :func:`_retry_step` says
        attempt = 0
        thr_h = eps_h = None
        while bad.size:
            attempt += 1
            if exhaustive:
                raise RuntimeError(f"exhaustive top-k left queries unproven (status bits {sorted(set(status[bad].tolist()))}): a bug")
            idx = torch.from_numpy(bad).to(dev)
            if attempt > MAX_ATTEMPTS:
                # More ties / near-ties around the k-th score than the candidate buffers hold (or a threshold that would not settle):
                # the remaining queries are searched EXACTLY, chunk by chunk, with every row re-scored in fp32 - slow, cannot fail.
                Db, Ib = self._search_exhaustive_chunks(q32.index_select(0, idx), k)
                D.index_copy_(0, idx, Db)
                I.index_copy_(0, idx, Ib)
                stats["fallback_queries"] = int(bad.size)
                break
            if thr_h is None:
                thr_h, eps_h = thr.cpu().numpy().astype(np.float64), eps.cpu().numpy().astype(np.float64)
            t_b, tiled, full = _retry_step(status[bad], thr_h[bad], eps_h[bad], khat.cpu().numpy().astype(np.float64)[bad], attempt)
            cap2_b = CAND_CAP if full else cap2
            Db, Ib = torch.empty(bad.size, k, **f32), torch.empty(bad.size, k, **i32)
            st2, _, _, khat2 = self._run(q32.index_select(0, idx), qh.select(idx), torch.from_numpy(t_b.astype(np.float32)).to(dev),
                                         eps.index_select(0, idx), _sel(qmu, idx), k, cap2_b, Db, Ib, tiled=tiled)
            status_b = st2.cpu().numpy() & m.status_mask
            good = status_b == 0
            if good.any():
                gi = torch.from_numpy(bad[good]).to(dev)
                sel = torch.from_numpy(np.nonzero(good)[0]).to(dev)
                D.index_copy_(0, gi, Db.index_select(0, sel))
                I.index_copy_(0, gi, Ib.index_select(0, sel))
            thr_h[bad] = t_b
            khat.index_copy_(0, idx, khat2)
            status[bad] = status_b
            nbad = (bad.size + QT - 1) // QT
            stats["scans"] += nbad
            stats["rescans"] += nbad
            # a kept set that does not fit the largest buffer (bit 16 at cap2 = CAND_CAP) cannot be helped by another threshold:
            # those queries go straight to the exact fallback on the next turn
            if cap2_b == CAND_CAP and ((status_b & 16) != 0).any():
                attempt = MAX_ATTEMPTS
            bad = bad[~good]
        return D, I, stats

    def _estimate_thresholds(self, qb, qnorm, kk: int, exhaustive: bool, sq=None):
        """-> (thr, eps) fp32 [nq] on the device: eps_q bounds |scan score - exact score|, thr_q = est_q - 2 eps_q with est_q the kth largest
        bf16 score of query q against the row sample (-inf, i.e. every row, on an exhaustive search).  ``sq``: the queries' digit scale
        (int8-row mode: the bound of csrc/topk_i8.hip)."""
        res, nq = self._res, qb.shape[0]
        f32 = dict(dtype=torch.float32, device=res.device)
        thr, eps = torch.full((nq,), -float("inf"), **f32), torch.empty(nq, **f32)

        bound = _MODES[res.mode].bound
        if exhaustive:
            bound(res, self.d, None, sq, qnorm, None, eps)
            return thr, eps
        # lam = expected number of sample rows inside the global top-kk; +4.5 sigma makes a too-high estimate (-> that query is searched
        # again) a ~1e-5 event per query
        S, n = res.s_rows, res.n
        lam = kk * S / n
        kth = int(min(S, math.ceil(lam + 4.5 * math.sqrt(lam) + 1.0))) if S < n else kk
        est = torch.empty(nq, **f32)
        samp = torch.empty(min(nq, EST_CHUNK), res.sample.shape[0], **f32)
        for lo in range(0, nq, EST_CHUNK):
            m = min(EST_CHUNK, nq - lo)
            ops.gemm_nt(qb[lo:lo + m], res.sample, samp[:m], m)
            ops.topk_kth_largest(samp[:m], S, kth, est[lo:lo + m])
        bound(res, self.d, est, sq, qnorm, thr, eps)
        return thr, eps

    def _search_exhaustive_chunks(self, q32: torch.Tensor, k: int):
        """Exact top-k of a few queries with EVERY row re-scored in fp32, CAND_CAP rows at a time (the exhaustive form of
        cldrd_flatip_search on row slices), the running top-k merged with each chunk's by the same sort kernel (score desc, row position
        asc).  The last resort of :meth:`search_device`: reads the fp32 rows once per 128/256 queries, needs no threshold, cannot fail.
        fp16-row / int8-row mode: the same over slices of the stored rows (scores as the class docstring defines them)."""
        res = self._res
        n, nq = res.n, q32.shape[0]
        qmu = ops.query_dot64(q32.contiguous(), res.mu) if _MODES[res.mode].qmu else None
        if 2 * k > CAND_CAP:
            raise ValueError(f"exact fallback: top_k = {k} > {CAND_CAP // 2}")
        i32, f32 = dict(dtype=torch.int32, device=res.device), dict(dtype=torch.float32, device=res.device)
        D = torch.full((nq, k), -float("inf"), **f32)
        I = torch.full((nq, k), -1, **i32)
        eps = torch.zeros(nq, **f32)
        thr = torch.full((nq,), -float("inf"), **f32)
        two = torch.full((nq,), 2 * k, **i32)
        for lo in range(0, n, CAND_CAP):
            Dc, Ic = torch.empty(nq, k, **f32), torch.empty(nq, k, **i32)
            self._run(q32, None, thr, eps, qmu, k, CAND_CAP, Dc, Ic, exhaustive=True, rows=slice(lo, lo + CAND_CAP))
            Ic = torch.where(Ic >= 0, Ic + lo, Ic)
            rows = torch.cat([I, Ic], dim=1).contiguous()
            scores = torch.cat([D, Dc], dim=1).contiguous()
            D, I = torch.empty(nq, k, **f32), torch.empty(nq, k, **i32)
            ops.topk_sort(two, rows, scores, k, D, I)          # missing entries (row -1, score -inf) sort last and come out as missing
        return D, I

    def _run(self, q32, qh, thr, eps, qmu, k, cap2, D, I, exhaustive=False, tiled=False, rows=slice(None)):
        """One chained search in the shard's row mode over the queries given and the rows ``rows`` of the shard, kept sets in buffers of ``cap2``
        slots -> (status, counts, n2, khat) on the device.  The per-batch scratch is reused by every batch of every search (same stream: no hazard)."""
        res = self._res
        dev, QT, nq = res.device, res.query_tile, q32.shape[0]
        if cap2 not in res.ws:
            res.ws[cap2] = dict(cand_rows=torch.empty(QT, CAND_CAP, dtype=torch.int32, device=dev),
                                cand_scores=torch.empty(QT, CAND_CAP, dtype=torch.float32, device=dev),
                                rows2=torch.empty(QT, cap2, dtype=torch.int32, device=dev),
                                scores2=torch.empty(QT, cap2, dtype=torch.float32, device=dev))
        ws = res.ws[cap2]
        counts = torch.zeros((nq + QT - 1) // QT * (QT + 1), dtype=torch.int32, device=dev)
        n2 = torch.empty(nq, dtype=torch.int32, device=dev)
        status = torch.empty(nq, dtype=torch.int32, device=dev)
        khat = torch.empty(nq, dtype=torch.float32, device=dev)
        bufs = (k, counts, ws["cand_rows"], ws["cand_scores"], ws["rows2"], ws["scores2"], n2, status, khat, D, I)
        _MODES[res.mode].chain(res, rows, q32, qh or _ScanQueries(), thr, eps, qmu, bufs, exhaustive, tiled)
        return status, counts, n2, khat

    # -- persistence (own format; faiss' binary layout is not reproduced) ----------------
    def write(self, path: str, fp16: bool = False, int8: bool = False):
        """``path.emb.npy`` (fp32 rows) + ``path.meta.pkl``; ``fp16=True``: the fp16-row format - ``path.emb16.npy`` (``R16 = fp16(p - mu)``,
        numpy float16, memory-mappable) and ``mu``, ``max_centred_norm``, ``raw_max_norm`` next to ``d / ids / id_offset`` in the meta file.  An
        index that is on a GPU writes the ``mu`` / ``R16`` it searches with; a host index computes them with numpy in chunks (same definition:
        ``mu`` = fp32 of the fp64 column mean - the last bit of ``mu``, and with it a few ``R16`` values, may differ between the two).
        ``int8=True``: the int8-row format - ``path.emb8.npy`` (``R8``, int8 [n, d], memory-mappable), ``path.scale.npy`` (``a``, fp32 [n]) and
        ``mu``, ``bound_l1`` (max a_r |R8[r]|_1), ``max_centred_norm`` (max a_r |R8[r]|_2), ``raw_max_norm`` in the meta file; an index attached in
        int8-row mode writes what it searches with, a host index quantises with numpy in chunks (the class docstring's definition; the same
        last-bit caveat for ``mu``).  The flags exclude one another; a refused call writes nothing."""
        mode = _requested_mode(fp16, int8, "FlatIPIndex.write")
        res, stored = self._res, self._stored
        if mode != "int8" and ((stored is not None and stored.mode == "int8") or (res is not None and res.mode == "int8" and self.embeddings is None)):
            raise ValueError("this index holds int8 rows only: write it with int8=True")
        if mode == "float32":
            if self.embeddings is None:
                raise ValueError("this index holds fp16 rows only (read from an fp16-row file): write it with fp16=True")
            np.save(path + ".emb.npy", self.embeddings)
            with open(path + ".meta.pkl", "wb") as fh:
                pickle.dump({"d": self.d, "ids": self.ids, "id_offset": self.id_offset, "format": FORMAT_F32, **self._normalized_mark()}, fh)
            return
        m = _MODES[mode]
        if mode == "float16" and res is not None and res.mode == "int8":
            raise ValueError("this index is attached in int8-row mode: write it with int8=True (or detach it: the fp16 rows come from fp32 rows)")
        # what an attached shard searches with (the fp32 form: its fp16 shadow), else the file's rows, else encoded straight into the rows file
        encoded = False
        if res is not None and (res.mode == mode or (mode, res.mode) == ("float16", "float32")):
            st = _StoredRows(mode, getattr(res, m.rows_field).cpu().numpy(), None if res.scale is None else res.scale.cpu().numpy(),
                             np.array(self.mu), res.cnorm, res.raw_max, res.b1)
        elif stored is not None and stored.mode == mode:
            st = stored
        else:
            st, encoded = self._encode_host(mode, path + m.rows_ext), True
        if not encoded:
            np.save(path + m.rows_ext, st.rows)
        meta = {"d": self.d, "ids": self.ids, "id_offset": self.id_offset, "format": m.file_format, "mu": st.mu}
        if st.scale is not None:
            np.save(path + ".scale.npy", st.scale)
            meta["bound_l1"] = float(st.b1)
        meta.update(max_centred_norm=float(st.cnorm), raw_max_norm=float(st.raw_max), **self._normalized_mark())
        with open(path + ".meta.pkl", "wb") as fh:
            pickle.dump(meta, fh)

    def _normalized_mark(self) -> dict:
        return {"normalized": True} if self.normalized else {}          # a raw-row index has exactly the keys it had

    def _encode_host(self, mode: str, rows_path: str) -> _StoredRows:
        """The host encoder of fp16-row / int8-row mode: the host's fp32 rows in chunks of ``HOST_CHUNK_ROWS`` -> the stored rows, written into
        ``rows_path`` (a memory-mapped .npy) as they are made, and their statistics (the device's definitions in numpy)."""
        m, emb = _MODES[mode], self.embeddings
        if emb is None or emb.shape[0] == 0:
            raise ValueError(m.no_host_rows)
        n, d = emb.shape
        m.host_check(d)
        mu, raw_sq = _host_stats(emb, m.not_finite)
        out = np.lib.format.open_memmap(rows_path, mode="w+", dtype=m.np_dtype, shape=(n, d))
        scale, b1, c_sq = None, 0.0, 0.0
        for lo in range(0, n, HOST_CHUNK_ROWS):
            rows, a, l1, c2 = m.encode(emb[lo:lo + HOST_CHUNK_ROWS], mu)
            out[lo:lo + rows.shape[0]] = rows
            if a is not None:
                scale = np.empty(n, dtype=np.float32) if scale is None else scale
                scale[lo:lo + rows.shape[0]] = a
            b1, c_sq = max(b1, l1), max(c_sq, c2)
        out.flush()
        return _StoredRows(mode, out, scale, mu, math.sqrt(float(np.float32(c_sq))), math.sqrt(float(np.float32(raw_sq))), float(b1))

    @staticmethod
    def quantize_rows_i8(rows32: np.ndarray, mu: np.ndarray):
        """The definition of int8-row mode on the host, for fp32 rows [m, d] and the shard's mean row: -> (R8 int8 [m, d], a fp32 [m],
        a_r |R8[r]|_1 and a_r^2 |R8[r]|_2^2 as the fp32 values of the fp64 products with the exact integer sums).  numpy's float32 division is
        correctly rounded and ``rint`` rounds half to even, as the device kernel does."""
        c = np.asarray(rows32, dtype=np.float32) - np.asarray(mu, dtype=np.float32)
        if not np.isfinite(c).all():
            raise ValueError(_NOT_FINITE8)
        a = (np.abs(c).max(axis=1) / np.float32(127.0)).astype(np.float32)
        live = a > 0
        t = np.zeros_like(c)
        np.divide(c, a[:, None], out=t, where=live[:, None])
        r8 = np.clip(np.rint(t), -127.0, 127.0).astype(np.int8)
        r64 = r8.astype(np.int64)
        a64 = a.astype(np.float64)
        l1 = (a64 * np.abs(r64).sum(axis=1)).astype(np.float32)
        l2sq = ((a64 * a64) * (r64 * r64).sum(axis=1)).astype(np.float32)
        return r8, a, l1, l2sq

    @classmethod
    def read(cls, path: str) -> "FlatIPIndex":
        with open(path + ".meta.pkl", "rb") as fh:
            meta = pickle.load(fh)
        idx = cls(meta["d"])
        mode = _FILE_MODES.get(meta.get("format"))
        if mode is None:
            rows = idx.embeddings = np.load(path + ".emb.npy", mmap_mode="r")
        else:
            m = _MODES[mode]
            rows = np.load(path + m.rows_ext, mmap_mode="r")
            scale = np.load(path + ".scale.npy") if mode == "int8" else None
            if rows.dtype != m.np_dtype or rows.ndim != 2 or rows.shape[1] != idx.d \
                    or (scale is not None and (scale.dtype != np.float32 or scale.shape != (rows.shape[0],))):
                raise ValueError(m.bad_file.format(path=path, d=idx.d))
            idx._stored = _StoredRows(mode, rows, scale, np.ascontiguousarray(meta["mu"], dtype=np.float32), float(meta["max_centred_norm"]),
                                      float(meta["raw_max_norm"]), float(meta.get("bound_l1", 0.0)))
        idx.ids, idx.id_offset = meta["ids"], meta.get("id_offset", 0)
        idx.normalized = bool(meta.get("normalized", False))
        idx.ntotal = rows.shape[0]
        return idx


def write_index(index: FlatIPIndex, path: str, faiss_format: bool = False, fp16: bool = False, int8: bool = False):
    """``faiss.write_index`` of the reference (index_text.py:103).  Default: this package's memory-mappable pair of files;
    ``faiss_format=True`` writes faiss' own ``IndexIDMap(IndexFlatIP)`` serialisation to ``path`` (see ``write_faiss_index``);
    ``fp16=True`` writes the fp16-row format, ``int8=True`` the int8-row format (:meth:`FlatIPIndex.write`; neither is available in faiss'
    layout).  The three flags exclude one another: a call with two of them raises and writes nothing."""
    if faiss_format and fp16:
        raise ValueError("write_index: the fp16-row format exists in this package's own layout only (faiss_format=True with fp16=True)")
    if int8 and faiss_format:
        raise ValueError(_EXCLUSION["write_index"])
    _requested_mode(fp16, int8, "write_index")
    if faiss_format:
        write_faiss_index(index, path)
    else:
        index.write(path, fp16=fp16, int8=int8)


def read_index(path: str) -> FlatIPIndex:
    """``faiss.read_index`` of the reference (retrieve_top_passages.py:77): reads either format (a faiss file starts with the
    fourcc ``IxMp`` / ``IxM2`` / ``IxFI``)."""
    if os.path.isfile(path):
        with open(path, "rb") as fh:
            magic = fh.read(4)
        if magic in (b"IxMp", b"IxM2", b"IxFI"):
            return read_faiss_index(path)
    return FlatIPIndex.read(path)


# ---- faiss binary interop -----------------------------------------------------------------
# Layout restated from faiss' published serialisation (faiss/impl/index_write.cpp, v1.7+), little endian:
#   index header : int32 d | int64 ntotal | int64 dummy (1 << 20) | int64 dummy | uint8 is_trained | int32 metric_type
#                  (0 = inner product, 1 = L2; a float32 metric_arg follows only for metric_type > 1)
#   "IxFI" flat  : header | uint64 n_floats (= ntotal * d) | n_floats float32, row major
#   "IxMp" idmap : header | <nested index> | uint64 n_ids | n_ids int64            ("IxM2" = IndexIDMap2, same payload)
# PARITY UNPINNED: faiss is not installed in the build image, so these two functions are checked against each other and
# against a hand-assembled byte string only (tests/test_oracle_optim_retrieval.py), not against a file written by faiss.
def _faiss_header(d: int, ntotal: int) -> bytes:
    import struct
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1, 0)


def write_faiss_index(index: "FlatIPIndex", path: str):
    import struct
    emb = np.ascontiguousarray(index.embeddings, dtype=np.float32)
    n, d = emb.shape
    ids = np.asarray(index.ids if index.ids is not None else np.arange(n) + index.id_offset, dtype=np.int64)
    with open(path, "wb") as fh:
        fh.write(b"IxMp" + _faiss_header(d, n))
        fh.write(b"IxFI" + _faiss_header(d, n) + struct.pack("<Q", n * d))
        fh.write(emb.tobytes())
        fh.write(struct.pack("<Q", n))
        fh.write(ids.tobytes())


def read_faiss_index(path: str) -> "FlatIPIndex":
    import struct

    def header(fh):
        d, ntotal, _, _, trained, metric = struct.unpack("<iqqqBi", fh.read(33))
        if metric > 1:
            fh.read(4)
        if metric != 0:
            raise ValueError("only inner-product flat indexes are supported (the reference builds IndexFlatIP)")
        return d, ntotal

    def flat(fh):
        d, ntotal = header(fh)
        (nfl,) = struct.unpack("<Q", fh.read(8))
        if nfl != ntotal * d:
            raise ValueError("faiss flat index: vector size does not match ntotal * d")
        return d, np.frombuffer(fh.read(4 * nfl), dtype=np.float32).reshape(ntotal, d)

    with open(path, "rb") as fh:
        magic = fh.read(4)
        if magic in (b"IxMp", b"IxM2"):
            header(fh)
            if fh.read(4) != b"IxFI":
                raise ValueError("faiss id map: nested index is not IndexFlatIP")
            d, emb = flat(fh)
            (nid,) = struct.unpack("<Q", fh.read(8))
            ids = np.frombuffer(fh.read(8 * nid), dtype=np.int64)
        elif magic == b"IxFI":
            d, emb = flat(fh)
            ids = None
        else:
            raise ValueError(f"not a faiss flat inner-product index (fourcc {magic!r})")
    idx = FlatIPIndex(d)
    if ids is None:
        idx.add(emb)
    else:
        idx.add_with_ids(emb, ids)
    return idx


def construct_flatindex_from_embeddings(embeddings, ids):
    """reference :116-129: flat inner-product index (+ id map when ``ids`` is given)."""
    hidden_size = embeddings.shape[1]
    print("embedding shape: " + str(embeddings.shape))
    index = FlatIPIndex(hidden_size)
    if ids is not None:
        if isinstance(ids, list):
            ids = np.array(ids)
        ids = ids.astype(np.int64)
        print(ids.shape, ids.dtype)
        index.add_with_ids(embeddings, ids)
    else:
        index.add(embeddings)
    return index


class ShardedFlatIPIndex:
    """Row-sharded index: this process holds rows [lo, hi) of the global matrix on its GPU; ``search`` returns the global
    top-k on rank 0 (other ranks get their local lists).  Works without torch.distributed as a single shard.

    The exchange + merge of one search (the reference's dead ``index_cpu_to_gpu_multiple(shard=True)`` branch,
    retriever/retrieval_utils.py:164-182):
      * over ProcessGroupNCCL (= RCCL over xGMI) with a device-resident local index the shard lists never leave HBM: every rank's
        (scores fp32 [nq, k], ids int64 [nq, k]) go to rank 0 with ONE ``dist.gather`` per tensor, rank 0 merges them with one sort launch
        (``cldrd_merge_topk_device``) and downloads the final [nq, k] pair - the same 84 MB a single-GPU search downloads at cfg5;
      * otherwise (gloo: the CPU tests; a stand-in local index): tensors are gathered through the host and merged by the native
        multi-threaded k-way merge (``cldrd_merge_topk``).
    Round 4 pickled the numpy lists (``gather_object``) and ran ``np.lexsort`` over [6980, 8000]: 15.6 s at cfg5 for 0.02 s of search."""

    def __init__(self, local: FlatIPIndex, rank: int = 0, world: int = 1, group=None):
        self.local, self.rank, self.world, self.group = local, rank, world, group
        self.row_dtype = getattr(local, "row_dtype", "float32")      # the local index searches in either row mode; the exchange does not care
        self.ntotal = local.ntotal
        self.last_merge = {}
        self.force_exchange = False        # tests / bench: run gather + merge with a process group of ONE rank too

    @staticmethod
    def shard_bounds(n: int, world: int, rank: int):
        per = -(-n // world)
        return min(n, rank * per), min(n, (rank + 1) * per)

    def _device_path(self):
        import torch.distributed as dist
        return (hasattr(self.local, "search_ids_device") and getattr(self.local, "device", None) is not None
                and dist.get_backend(self.group) == "nccl")

    def search(self, queries, k):
        if self.world == 1 and not self.force_exchange:
            return self.local.search(queries, k)
        import torch.distributed as dist
        k = int(k)
        if self._device_path():
            dev = self.local.device
            q = np.ascontiguousarray(queries, dtype=np.float32)
            with torch.cuda.device(dev):
                Dd, Id = self.local.search_ids_device(torch.from_numpy(q).to(dev), k)
                Dm, Im = self.gather_merge_device(Dd.contiguous(), Id.contiguous(), k)
                return Dm.cpu().numpy(), Im.cpu().numpy()
        D, I = self.local.search(queries, k)
        Dt, It = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(I, dtype=np.int64))
        gD = [torch.empty_like(Dt) for _ in range(self.world)] if self.rank == 0 else None
        gI = [torch.empty_like(It) for _ in range(self.world)] if self.rank == 0 else None
        dist.gather(Dt, gD, dst=0, group=self.group)
        dist.gather(It, gI, dst=0, group=self.group)
        if self.rank != 0:
            return D, I
        t0 = timer()
        out = merge_shard_results([g.numpy() for g in gD], [g.numpy() for g in gI], k)
        self.last_merge = {"path": _MERGE_HOST, "merge_s": timer() - t0}
        return out

    def gather_merge_device(self, Dd: torch.Tensor, Id: torch.Tensor, k: int):
        """Device tensors of this rank's lists -> the merged (D, I) device tensors on rank 0 (the local lists elsewhere)."""
        import torch.distributed as dist
        if self.world == 1 and not self.force_exchange:
            return Dd, Id
        nq = Dd.shape[0]
        if self.rank == 0:
            allD = torch.empty(self.world, nq, k, dtype=torch.float32, device=Dd.device)
            allI = torch.empty(self.world, nq, k, dtype=torch.int64, device=Dd.device)
            gD, gI = list(allD.unbind(0)), list(allI.unbind(0))
        else:
            allD = allI = gD = gI = None
        dist.gather(Dd, gD, dst=0, group=self.group)
        dist.gather(Id, gI, dst=0, group=self.group)
        if self.rank != 0:
            return Dd, Id
        D, I, path = _merge_lists(allD, allI, k, as_tensors=True)
        self.last_merge = {"path": path}
        return D, I


def merge_shard_results(shard_D, shard_I, k):
    """Host k-way merge of per-shard top-k lists (native, multi-threaded: ``cldrd_merge_topk``): score desc; ties -> shard asc, then list
    position asc (= global row position asc for row-range shards: the single-index tie rule); missing entries (id -1) last."""
    return ops.merge_topk_host(shard_D, shard_I, k)


def _merge_lists(allD: torch.Tensor, allI: torch.Tensor, k: int, as_tensors: bool):
    """The lists of W shards gathered on one device (scores fp32 [W, nq, k], ids int64 [W, nq, k]) -> (D, I, the path taken, for
    ``last_merge``): one sort launch when its LDS holds W * k candidates per query, else - more candidates than one launch holds - the
    native host merge.  ``as_tensors``: the result as tensors on that device, else as numpy arrays; only the path whose own output is of
    the other kind converts."""
    if allD.shape[0] * k <= CAND_CAP:
        D, I = ops.merge_topk_device(allD, allI, k)
        return (D, I, _MERGE_DEVICE) if as_tensors else (D.cpu().numpy(), I.cpu().numpy(), _MERGE_DEVICE)
    D, I = ops.merge_topk_host(list(allD.cpu().numpy()), list(allI.cpu().numpy()), k)
    return (torch.from_numpy(D).to(allD.device), torch.from_numpy(I).to(allD.device), _MERGE_HOST) if as_tensors else (D, I, _MERGE_HOST)


class MultiDeviceFlatIPIndex:
    """ONE process, several row shards on the devices of a list: what the reference's list branch of ``convert_index_to_gpu`` intends
    (retriever/retrieval_utils.py:164-182: ``index_cpu_to_gpu_multiple(..., shard=True)``; dead code there - ``gpu_resources`` is undefined).
    Shard s holds the contiguous row range ``ShardedFlatIPIndex.shard_bounds(n, S, s)`` of the index on ``devices[s]`` (a device may appear
    more than once: two shards on one GPU, which is how a one-GPU box tests this path).  ``search``: the queries are uploaded to every
    device and the shards are searched ONE AFTER ANOTHER (every search reads its proof flags back to the host before it returns, so shards
    on different GPUs do not overlap), the per-shard lists - scores fp32 [nq, k], ids int64 [nq, k], already mapped - are copied device to
    device onto the first live shard's device and merged by the same launch a multi-process search uses on rank 0
    (``cldrd_merge_topk_device``; more than 8192 candidates per query: the native host merge).  Order: score desc, ties -> shard asc, then
    list position asc = global row position asc, the single-index rule.  An index without rows answers with all-missing lists.
    The production path for 8 GPUs stays one process per GPU (:class:`ShardedFlatIPIndex`, retrieve_top_passages.py under RANK /
    WORLD_SIZE): one Python thread drives all devices here.  int8-row mode is not offered here (an index read from an int8-row file holds no
    host rows to shard and is refused like any index without them); a sharded int8 search is one process per GPU."""

    def __init__(self, index: FlatIPIndex, devices, fp16_rows: bool = False):
        if not devices:
            raise ValueError("convert_index_to_gpu: empty device list")
        if index.embeddings is None:
            raise ValueError("convert_index_to_gpu(index, [devices...]): the index must still hold its rows on the host")
        self.d, self.ntotal = index.d, index.ntotal
        self.row_dtype = "float16" if fp16_rows else "float32"       # fp16-row mode: every shard is centred on its OWN mean row
        self.devices = [torch.device("cuda", d) if isinstance(d, int) else torch.device(d) for d in devices]
        self.shards = []
        S = len(self.devices)
        for s_, dev in enumerate(self.devices):
            lo, hi = ShardedFlatIPIndex.shard_bounds(index.ntotal, S, s_)
            sh = FlatIPIndex(index.d)
            if hi > lo:
                if index.ids is not None:
                    sh.add_with_ids(index.embeddings[lo:hi], index.ids[lo:hi])
                else:
                    sh.add(index.embeddings[lo:hi])
                    sh.id_offset = index.id_offset + lo
                sh.to_gpu(dev, fp16_rows=fp16_rows)
            self.shards.append(sh)
        self.last_stats = {}
        self.last_merge = {}

    def search(self, queries, k):
        q, k, empty = _check_queries(queries, self.d, k)
        if empty is not None:
            return empty
        nq = q.shape[0]
        live = [sh for sh in self.shards if sh.ntotal > 0]
        if not live:
            return _all_missing(nq, k)
        dev0 = live[0].device
        qh = torch.from_numpy(q)
        lists = []
        for sh in live:
            with torch.cuda.device(sh.device):
                Dd, Id = sh.search_ids_device(qh.to(sh.device, non_blocking=True), k)
            lists.append((Dd, Id))
        self.last_stats = {"shards": [sh.last_stats for sh in live]}
        if len(lists) == 1:
            return lists[0][0].cpu().numpy(), lists[0][1].cpu().numpy()
        with torch.cuda.device(dev0):
            W = len(lists)
            allD = torch.empty(W, nq, k, dtype=torch.float32, device=dev0)
            allI = torch.empty(W, nq, k, dtype=torch.int64, device=dev0)
            for w, (Dd, Id) in enumerate(lists):
                if Dd.device != dev0:
                    torch.cuda.current_stream(dev0).wait_stream(torch.cuda.current_stream(Dd.device))      # the shard's search is done
                allD[w].copy_(Dd, non_blocking=True)        # device to device (xGMI between GPUs of one node)
                allI[w].copy_(Id, non_blocking=True)
            D, I, path = _merge_lists(allD, allI, k, as_tensors=False)
            self.last_merge = {"path": path, "shards": W}
            return D, I


def convert_index_to_gpu(index, faiss_gpu_index, useFloat16=False):
    """reference :155-184.  int (or 1-element list): whole index on that GPU.  list of several devices: the index is row-sharded over
    them inside THIS process (:class:`MultiDeviceFlatIPIndex`; the reference's branch, :164-182, is dead code - this is what it
    intends); the 8-GPU production path is still one process per GPU (:class:`ShardedFlatIPIndex`).  ``useFloat16=False``: fp32 rows and the
    fp16 scan shadow are resident, scores are exact fp32.  ``useFloat16=True``: fp16-row mode (:class:`FlatIPIndex`) - as in faiss the vectors
    live on the GPU in half precision only (a third of the default's bytes) and scores come from the half-precision vectors; unlike faiss the
    stored vectors are the CENTRED rows ``fp16(p - mu)`` plus ``mu``.  An index read from an fp16-row file is in that mode whatever the flag, and
    one read from an int8-row file attaches in int8-row mode whatever the flag; int8-row mode on an fp32-format index is
    ``index.to_gpu(device, int8_rows=True)``."""
    if type(faiss_gpu_index) == list and len(faiss_gpu_index) == 1:
        faiss_gpu_index = faiss_gpu_index[0]
    if isinstance(faiss_gpu_index, int):
        return index.to_gpu(faiss_gpu_index, fp16_rows=bool(useFloat16))
    if isinstance(faiss_gpu_index, (list, tuple)):
        return MultiDeviceFlatIPIndex(index, list(faiss_gpu_index), fp16_rows=bool(useFloat16))
    raise TypeError(f"convert_index_to_gpu: a device index or a list of them, got {type(faiss_gpu_index).__name__}")


def index_retrieve(index, query_embeddings, topk, batch=None, as_arrays=False):
    """reference :131-153: search everything at once or in query batches; returns (scores, ids) as nested lists when
    batched (as the reference does), arrays otherwise.  ``as_arrays`` (ours): arrays also when batched - 14 M Python scalars of a
    dev-set run (6980 x 1000 x 2) cost seconds to build and the run-file writer takes arrays."""
    print("Query Num", len(query_embeddings))
    start = timer()
    if batch is None:
        nn_scores, nearest_neighbors = index.search(query_embeddings, topk)
    else:
        # The reference searches slice by slice (:141-149).  Here the whole query set goes to the index in ONE call - the search
        # itself walks it in batches of 128 on the device, and a sharded index gathers / merges once instead of once per slice -
        # and only the conversion to the nested lists the reference returns is done per `batch` slice.
        all_scores, all_nn = index.search(query_embeddings, topk)
        if as_arrays:
            elapsed_time = timer() - start
            print(f"Elapsed Time: {elapsed_time:.1f}s, Elapsed Time per query: {1000 * elapsed_time / len(query_embeddings):.1f}ms")
            return all_scores, all_nn
        query_offset_base = 0
        nearest_neighbors = []
        nn_scores = []
        while query_offset_base < len(query_embeddings):
            nearest_neighbors.extend(all_nn[query_offset_base:query_offset_base + batch].tolist())
            nn_scores.extend(all_scores[query_offset_base:query_offset_base + batch].tolist())
            query_offset_base += batch
    elapsed_time = timer() - start
    elapsed_time_per_query = 1000 * elapsed_time / len(query_embeddings)
    print(f"Elapsed Time: {elapsed_time:.1f}s, Elapsed Time per query: {elapsed_time_per_query:.1f}ms")
    return nn_scores, nearest_neighbors
