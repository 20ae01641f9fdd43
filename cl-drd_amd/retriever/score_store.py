"""Teacher score store: every (query, passage) pair is scored by the teacher once across runs.

A pair's teacher score does not depend on the batch it is scored in (``CrossEncoder.score_cached``), so a stored score is, bit for bit, the
score a re-run would compute (for one build of the kernel library).  ``retriever.rerank_top_passages`` and ``retriever.build_stage_file``
look their pairs up here first (``--score_store DIR``), score only the misses and append them; the two programs share stores.

Layout: a directory of SEGMENTS and one ``meta.json``.  A segment is ``seg-NNNNNN.q.npy`` (int64), ``.p.npy`` (int64), ``.s.npy``
(float32): at most 2^31 - 1 entries, strictly ascending in the key (qid, pid) - lexicographic, qid major, signed compares.  Segments are
pairwise disjoint by construction (only pairs that missed are scored and appended).  ``meta.json`` is the commit point: it is written
to a temporary name and moved into place with ``os.replace`` after the segment files it names; segment files it does not name are
leftovers of an interrupted write and are removed on open.  One writer: ``.lock`` is created with ``O_EXCL``.

The store keeps the IDENTITY of what produced its scores (:func:`teacher_identity`) and refuses to open under another one.  The arrays
live in HBM; search and merge are ``hip_ops.pair_lookup`` / ``hip_ops.pair_merge``, sorting a chunk is two stable ``torch.sort`` calls."""
from __future__ import annotations

import hashlib
import json
import os
import re
import time

import numpy as np
import torch

from .. import _lib
from .. import hip_ops as ops

FORMAT = 1
COMPACT_ABOVE = 8                   # close() compacts a store of more segments than this
DEFAULT_FLUSH_PAIRS = 1 << 23       # misses scored between two appends: a convenience (what a killed job loses at most), not a tuned number
SEGMENT_MAX = ops.PAIR_SEGMENT_MAX
_SEG_FILE = re.compile(r"^(seg-\d{6,})\.[qps]\.npy$")
_CACHE_FIELDS = ("source_bytes", "max_length", "tokenizer", "vocab_size")     # the token cache's staleness rule without path and mtime


class ScoreStoreError(RuntimeError):
    pass


def file_sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 22), b""):
            h.update(block)
    return h.hexdigest()


def teacher_identity(model, max_len: int, fp32: bool, q_cache, p_cache) -> dict:
    """What a stored score depends on, as a flat dict: a SHA-256 over the teacher's parameters as loaded (the encoder's flat parameter
    buffer, the four head tensors) and its config, ``num_labels``, the pair ``max_len``, the arithmetic (``fp32`` for the exact pass, else
    the tower's ``CLDRD_AMP`` mode as it read it) and, of each token cache's own ``meta``, the fields of its staleness rule."""
    from dataclasses import asdict
    h = hashlib.sha256()
    h.update(json.dumps(asdict(model.cfg), sort_keys=True, default=str).encode())
    for t in (model.encoder.flat_p, model.head_w1, model.head_b1, model.head_w2, model.head_b2):
        a = t.detach().to("cpu", torch.float32).contiguous().numpy()
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    ident = {"teacher_sha256": h.hexdigest(), "num_labels": int(model.num_labels), "max_len": int(max_len),
             "arithmetic": "fp32" if fp32 else str(model.encoder.amp_mode)}
    for side, cache in (("query_cache", q_cache), ("passage_cache", p_cache)):
        for k in _CACHE_FIELDS:
            ident[f"{side}.{k}"] = cache.meta[k]
    return ident


def _save(path, a):
    with open(path, "wb") as fh:
        np.save(fh, a)
        fh.flush()
        os.fsync(fh.fileno())


class TeacherScoreStore:
    """``TeacherScoreStore(path, identity, device)`` opens (or creates) the store, as its one writer.  Use as a context manager or call
    :meth:`close`.  ``library_path``: the kernel library whose digest is compared with the recorded one (default: the loaded one)."""

    def __init__(self, path: str, identity: dict, device="cuda", library_path: str | None = None):
        self.path, self.device = str(path), torch.device(device)
        self.identity = dict(identity)
        self.segments = []              # [(name, q, p, s)]: the committed segments, arrays on the device
        self.next_segment = 0
        self._locked = False
        lib_digest = file_sha256(library_path or _lib.LIB_PATH)
        os.makedirs(self.path, exist_ok=True)
        self._lock()
        try:
            meta = self._read_meta()
            if meta is None:
                self.library_sha256 = lib_digest
            else:
                self._check_identity(meta)
                self.library_sha256 = meta.get("library_sha256", "")
                if self.library_sha256 != lib_digest:
                    print(f"score store {self.path}: filled by another build of the kernel library - its scores are the teacher's scores "
                          "to rounding, byte equality with a re-run holds for one build only")
                self.next_segment = int(meta["next_segment"])
            named = {} if meta is None else {s["name"]: int(s["entries"]) for s in meta["segments"]}
            self._remove_unnamed(named)
            for name, entries in named.items():
                self.segments.append((name, *self._load_segment(name, entries)))
            if meta is None:
                self._commit(self.segments)     # the identity is on disk before the first score
        except BaseException:
            self._unlock()
            raise

    # ------------------------------------------------------------------ files
    def _file(self, name, part=None):
        return os.path.join(self.path, name if part is None else f"{name}.{part}.npy")

    def _lock(self):
        lock = self._file(".lock")
        try:
            fd = os.open(lock, os.O_CREAT | os.O_EXCL | os.O_WRONLY)
        except FileExistsError:
            raise ScoreStoreError(f"score store {self.path} is locked: another job writes to it, or one was killed - if none is running, "
                                  f"delete {lock}") from None
        os.write(fd, f"{os.getpid()}\n".encode())
        os.close(fd)
        self._locked = True

    def _unlock(self):
        if self._locked:
            self._locked = False
            try:
                os.remove(self._file(".lock"))
            except FileNotFoundError:
                pass

    def _need_lock(self):
        if not self._locked:
            raise ScoreStoreError(f"score store {self.path} is closed: its lock is released, nothing may be written")

    def _read_meta(self):
        try:
            with open(self._file("meta.json")) as fh:
                meta = json.load(fh)
        except FileNotFoundError:
            return None
        if meta.get("format") != FORMAT:
            raise ScoreStoreError(f"score store {self.path}: format {meta.get('format')!r}, this program reads format {FORMAT}")
        return meta

    def _check_identity(self, meta):
        stored = meta["identity"]
        for k in sorted(set(stored) | set(self.identity)):
            if stored.get(k) != self.identity.get(k):
                raise ScoreStoreError(f"score store {self.path}: filled with {k}={stored.get(k)!r}, this run has {self.identity.get(k)!r}: "
                                      "its scores are not this run's - use another --score_store directory")

    def _remove_unnamed(self, named):
        for f in os.listdir(self.path):
            m = _SEG_FILE.match(f)
            if (m and m.group(1) not in named) or f == "meta.json.tmp":
                os.remove(os.path.join(self.path, f))

    def _load_segment(self, name, entries):
        try:
            q, p, s = (np.load(self._file(name, part)) for part in "qps")
        except (OSError, ValueError) as exc:
            raise ScoreStoreError(f"score store {self.path}: segment {name} is named by meta.json but cannot be read ({exc})") from exc
        if (q.dtype, p.dtype, s.dtype) != (np.int64, np.int64, np.float32) or not (q.shape == p.shape == s.shape == (entries,)):
            raise ScoreStoreError(f"score store {self.path}: segment {name} does not match meta.json ({entries} entries, int64 / int64 / float32)")
        q, p, s = (torch.from_numpy(a).to(self.device) for a in (q, p, s))
        if entries > 1 and not bool(((q[1:] > q[:-1]) | ((q[1:] == q[:-1]) & (p[1:] > p[:-1]))).all()):
            raise ScoreStoreError(f"score store {self.path}: segment {name} is not strictly ascending in (qid, pid): the store is damaged")
        return q, p, s

    def _write_segment(self, q, p, s):
        name = f"seg-{self.next_segment:06d}"
        self.next_segment += 1
        for part, a in zip("qps", (q, p, s)):
            _save(self._file(name, part), a.cpu().numpy())
        return name

    def _commit(self, segments):
        meta = {"format": FORMAT, "identity": self.identity, "library_sha256": self.library_sha256, "next_segment": self.next_segment,
                "segments": [{"name": name, "entries": int(q.shape[0])} for name, q, _, _ in segments]}
        tmp = self._file("meta.json.tmp")
        with open(tmp, "w") as fh:
            json.dump(meta, fh, indent=1)
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, self._file("meta.json"))
        self.segments = list(segments)

    # ------------------------------------------------------------------ operations
    def __len__(self):
        return sum(int(q.shape[0]) for _, q, _, _ in self.segments)

    def lookup(self, qid, starts, pid):
        """CSR batch (qid int64 [nq], starts int64 [nq + 1], pid int64 [total], on the device) -> (score fp32 [total], hit uint8 [total]):
        over all segments; a missed pair has hit 0 (and score 0)."""
        score = torch.zeros(pid.shape[0], dtype=torch.float32, device=pid.device)
        hit = torch.zeros(pid.shape[0], dtype=torch.uint8, device=pid.device)
        for _, q, p, s in self.segments:
            ops.pair_lookup(q, p, s, qid, starts, pid, score, hit)
        return score, hit

    def append(self, qid_per_pair, pid, score):
        """One new segment from a chunk of scored pairs (device arrays, one entry per pair, any order).  The same key twice in the chunk is
        kept once when the score bits agree, ``ScoreStoreError`` when they differ.  The pairs must not be in the store (they missed)."""
        self._need_lock()
        n = int(pid.shape[0])
        if qid_per_pair.shape[0] != n or score.shape[0] != n:
            raise ValueError("append: one qid, one pid and one score per pair")
        if n == 0:
            return
        if n > SEGMENT_MAX:
            raise ValueError("append: a segment holds at most 2^31 - 1 entries; flush smaller chunks")
        by_p = torch.sort(pid, stable=True).indices
        order = by_p[torch.sort(qid_per_pair[by_p], stable=True).indices]
        q, p, s = qid_per_pair[order], pid[order], score.to(torch.float32)[order]
        same = (q[1:] == q[:-1]) & (p[1:] == p[:-1])
        if bool(same.any()):
            bits = s.view(torch.int32)
            clash = same & (bits[1:] != bits[:-1])
            if bool(clash.any()):
                at = int(clash.nonzero()[0])
                raise ScoreStoreError(f"append: pair ({int(q[at])}, {int(p[at])}) occurs twice in one chunk with different scores")
            keep = torch.cat([torch.ones(1, dtype=torch.bool, device=same.device), ~same])
            q, p, s = q[keep], p[keep], s[keep]
        name = self._write_segment(q, p, s)
        self._commit(self.segments + [(name, q, p, s)])

    def compact(self):
        """All segments merged into one on the device (smallest first; two whose sum would pass 2^31 - 1 entries stay apart), written as a
        new segment, committed, the old files removed.  ``ValueError`` when two segments share a key: nothing on disk has changed then."""
        self._need_lock()
        work = sorted(self.segments, key=lambda seg: int(seg[1].shape[0]))
        old, merged = [], False
        while len(work) > 1 and int(work[0][1].shape[0]) + int(work[1][1].shape[0]) <= SEGMENT_MAX:
            (na, *a), (nb, *b) = work[0], work[1]
            old += [nm for nm in (na, nb) if nm is not None]
            work = sorted([(None, *ops.pair_merge(*a, *b))] + work[2:], key=lambda seg: int(seg[1].shape[0]))
            merged = True
        if not merged:
            return
        counter = self.next_segment
        try:
            final = [(self._write_segment(q, p, s) if nm is None else nm, q, p, s) for nm, q, p, s in work]
            self._commit(final)
        except BaseException:
            self.next_segment = counter
            raise
        for name in old:
            for part in "qps":
                os.remove(self._file(name, part))

    def close(self, compact: bool = True):
        """Release the lock; a store of more than COMPACT_ABOVE segments is compacted first (``compact=False``: not, as after an error)."""
        try:
            if self._locked and compact and len(self.segments) > COMPACT_ABOVE:
                self.compact()
        finally:
            self._unlock()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(compact=exc_type is None)
        return False


def score_through_store(store, row_qid, starts, pid, lengths, score_chunk, flush_pairs=DEFAULT_FLUSH_PAIRS):
    """Scores fp32 [total] (device) of a CSR batch of pairs - ``row_qid`` int64 [nq], ``starts`` int64 [nq + 1], ``pid`` int64 [total], on
    the device - taken from ``store`` where it has them; the misses are scored by ``score_chunk(positions)`` (host int64 positions into the
    batch -> device fp32 scores) in global pair-length order (``lengths``: host array, one per pair), at most ``flush_pairs`` at a time,
    each chunk appended to the store before the next is scored.  Returns (scores, stats): pairs, hits, scored, segments, lookup_s,
    append_s."""
    flush_pairs = int(flush_pairs)
    if flush_pairs < 1:
        raise ValueError("--score_store_flush_pairs is at least 1")
    total = int(pid.shape[0])
    stats = {"pairs": total, "hits": 0, "scored": 0, "segments": len(store.segments), "lookup_s": 0.0, "append_s": 0.0}
    if total == 0:
        return torch.zeros(0, dtype=torch.float32, device=pid.device), stats
    t0 = time.perf_counter()
    score, hit = store.lookup(row_qid, starts, pid)
    miss = (hit == 0).nonzero().reshape(-1).cpu().numpy()           # (the copy waits for the lookups)
    stats["lookup_s"] = time.perf_counter() - t0
    stats["hits"] = total - int(miss.shape[0])
    if miss.shape[0]:
        qid_per_pair = torch.repeat_interleave(row_qid, starts[1:] - starts[:-1], output_size=total)
        miss = miss[np.argsort(np.asarray(lengths)[miss], kind="stable")]
        for a in range(0, miss.shape[0], flush_pairs):
            chunk = miss[a:a + flush_pairs]
            s = score_chunk(chunk)
            at = torch.from_numpy(chunk).to(pid.device)
            score.index_copy_(0, at, s)
            torch.cuda.synchronize(pid.device)
            t0 = time.perf_counter()
            store.append(qid_per_pair[at], pid[at], s)
            stats["append_s"] += time.perf_counter() - t0
            stats["scored"] += int(chunk.shape[0])
    stats["segments"] = len(store.segments)
    return score, stats


def add_arguments(ap):
    ap.add_argument("--score_store", default="", help="directory of a teacher score store: pairs it holds are not scored again, the others "
                                                      "are scored and added (the store refuses another teacher, max_len, arithmetic or token cache)")
    ap.add_argument("--score_store_flush_pairs", type=int, default=DEFAULT_FLUSH_PAIRS,
                    help="misses scored between two writes to the store: what a killed job loses at most")
