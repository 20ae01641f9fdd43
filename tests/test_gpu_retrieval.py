"""Index / retrieve path on the MI355X against the oracle (oracle/retrieval_ref.py: exact fp64->fp32 inner product,
score desc then row position asc).  Integer outputs (ids, ranks) must be identical; scores within 1e-5 relative."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops
import selftest
from cldrd_amd.retriever import retrieval_utils as RU
from oracle import retrieval_ref as R

DEV = "cuda"


def test_kth_largest_matches_numpy():
    x = (syn.normal(5, 7 * 5000).reshape(7, 5000) * 3).astype(np.float32)
    x[2, :50] = 1.5          # ties
    xd = torch.from_numpy(x).to(DEV)
    thr = torch.empty(7, device=DEV)
    for kth in (1, 2, 37, 1000, 5000, 9999):
        ops.topk_kth_largest(xd, 5000, kth, thr)
        ref = -np.sort(-x, axis=1)[:, min(kth, 5000) - 1]
        assert np.array_equal(thr.cpu().numpy(), ref), kth


@pytest.mark.parametrize("S", [1024, 8192, 8193, 16496, 32768, 32769, 40000])
def test_kth_largest_register_and_streaming_forms(S):
    """S <= 32768 keeps the row in registers (8 or 32 per thread), larger rows are re-read per radix digit; both against numpy, with ties, negative
    values, infinities and a leading dimension larger than S."""
    nq = 5
    x = (syn.normal(11, nq * (S + 8)).reshape(nq, S + 8) * 5).astype(np.float32)
    x[1, : S // 2] = -2.25
    x[2, :3] = [np.inf, -np.inf, 0.0]
    x[3] = np.abs(x[3]) * 1e-30
    xd = torch.from_numpy(x).to(DEV)
    thr = torch.empty(nq, device=DEV)
    for kth in (1, 34, 257, S // 2, S - 1, S):
        ops.topk_kth_largest(xd, S, kth, thr)
        ref = -np.sort(-x[:, :S], axis=1)[:, kth - 1]
        assert np.array_equal(thr.cpu().numpy(), ref), (S, kth)


@pytest.mark.parametrize("cap,k", [(2, 1), (100, 10), (128, 128), (1000, 1000), (2048, 1000), (3000, 100), (8192, 1000)])
def test_topk_sort_orders_by_score_then_row(cap, k):
    """The bitonic sort runs its narrow steps without workgroup barriers: every list length around the 128-key chunk size and the
    power-of-two padding, ties broken by the lower row, short lists padded with (-inf, -1)."""
    rng = np.random.default_rng(cap)
    nq = 9
    counts = rng.integers(0, cap + 1, size=nq).astype(np.int32)
    counts[0], counts[1], counts[2] = cap, 0, min(cap, 129)
    rows = np.stack([rng.permutation(50000)[:cap] for _ in range(nq)]).astype(np.int32)
    scores = rng.standard_normal((nq, cap)).astype(np.float32)
    scores[:, ::3] = np.round(scores[:, ::3]) + 0.0      # plenty of ties (+ 0.0: no -0.0, which the key order puts below 0.0)
    D = torch.empty(nq, k, device=DEV)
    I = torch.empty(nq, k, dtype=torch.int32, device=DEV)
    ops.topk_sort(torch.from_numpy(counts).to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(scores).to(DEV), k, D, I)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    for q in range(nq):
        n = int(counts[q])
        order = np.lexsort((rows[q, :n], -scores[q, :n].astype(np.float64)))[:k]
        m = len(order)
        assert np.array_equal(I[q, :m], rows[q, order]) and np.array_equal(D[q, :m], scores[q, order]), (cap, q)
        assert np.all(I[q, m:] == -1) and np.all(np.isneginf(D[q, m:]))


def same_ranking(D, I, Dr, Ir, rel=1e-5):
    """Identical ids and ranks wherever adjacent reference scores differ by more than rel * |score|; scores within rel.
    Inside a run of near-equal reference scores (adjacent gaps <= rel * |score| + 1e-6) the order may differ but the id SET of
    the run must be the same; only the run that is cut by the list end may differ in membership (ties across the cut-off)."""
    assert D.shape == Dr.shape and I.shape == Ir.shape
    finite = np.isfinite(Dr)
    assert np.array_equal(np.isfinite(D), finite)
    assert np.allclose(D[finite], Dr[finite], rtol=rel, atol=1e-6)
    assert np.array_equal(I[~finite], Ir[~finite])          # padding: -1 in both
    swaps = 0
    for q in range(D.shape[0]):
        if np.array_equal(I[q], Ir[q]):
            continue
        kq = int(finite[q].sum())
        dr = Dr[q, :kq].astype(np.float64)
        gap_ok = np.abs(np.diff(dr)) <= rel * np.abs(dr[1:]) + 1e-6          # True: j and j+1 are near-ties
        start = 0
        for j in range(kq):
            if j == kq - 1 or not gap_ok[j]:
                run = slice(start, j + 1)
                if j + 1 < kq or kq < D.shape[1]:           # a complete run: same members, any order
                    assert sorted(I[q, run].tolist()) == sorted(Ir[q, run].tolist()), (q, start, j, I[q, run], Ir[q, run], dr[run])
                swaps += int((I[q, run] != Ir[q, run]).sum())
                start = j + 1
    return swaps


@pytest.mark.parametrize("n,d,nq,k", [(20000, 768, 7, 1000), (20000, 768, 150, 100), (3000, 128, 5, 10), (500, 128, 3, 1000),
                                       (70001, 256, 33, 1000)])
def test_flat_ip_search_matches_oracle(n, d, nq, k):
    emb = syn.corpus_embeddings(11, n, d)
    emb[n // 2] = emb[n // 3]                # exact duplicate -> tie broken by row position
    q = syn.corpus_embeddings(12, nq, d)
    q[0] = emb[17] * 1.0                      # a query that is a corpus row
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    RU.convert_index_to_gpu(index, 0, False)
    D, I = index.search(q, k)
    Dr, Ir = R.flat_ip_search(emb, ids, q, k)
    same_ranking(D, I, Dr, Ir)
    assert np.all(np.diff(D[:, :min(k, n)], axis=1) <= 0)
    if k > n:
        assert np.all(I[:, n:] == -1) and np.all(np.isneginf(D[:, n:]))
    st = index.last_stats
    assert st["exhaustive"] == (n <= RU.CAND_CAP)
    assert st["exhaustive"] or st["scans"] >= (nq + index.query_tile - 1) // index.query_tile


@pytest.mark.parametrize("hook", [{}, {"probe": False}, {"query_tile_request": 128}])
def test_multi_pass_search_switches_give_the_same_answer(hook):
    """A search of several passes (more than two query tiles) with the probe pass off / with 128-query tiles (test hooks of FlatIPIndex, set
    before the shard is attached): the exact result cannot depend on how the thresholds were found or how the queries were tiled - scores
    and ids against the oracle, and equal to the default's."""
    n, d, nq, k = 60000, 768, 700, 100
    emb = syn.corpus_embeddings(21, n, d)
    q = syn.corpus_embeddings(22, nq, d)
    ids = np.arange(n, dtype=np.int64)
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    for kk, vv in hook.items():
        setattr(index, kk, vv)
    RU.convert_index_to_gpu(index, 0, False)
    assert index.query_tile == (128 if hook.get("query_tile_request") == 128 else 256)
    D, I = index.search(q, k)
    st = dict(index.last_stats)
    assert not st["exhaustive"] and st["scans"] >= 3
    Dr, Ir = R.flat_ip_search(emb, ids, q[:64], k)
    same_ranking(D[:64], I[:64], Dr, Ir)
    index2 = RU.construct_flatindex_from_embeddings(emb, ids)
    RU.convert_index_to_gpu(index2, 0, False)
    D2, I2 = index2.search(q, k)
    assert np.array_equal(D, D2) and np.array_equal(I, I2)


@pytest.mark.parametrize("nq,k,rows", [(1, 1, 50), (3, 100, 50), (0, 10, 50), (2, 5, 1)])
def test_degenerate_searches(nq, k, rows):
    """One query, k = 1, k larger than the index, no queries at all (faiss returns empty [0, k] arrays), an index of one row."""
    emb = syn.corpus_embeddings(3, 50, 128)[:rows]
    ids = np.arange(rows, dtype=np.int64) + 7
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    RU.convert_index_to_gpu(index, 0, False)
    q = syn.corpus_embeddings(4, max(nq, 1), 128)[:nq]
    D, I = index.search(q, k)
    assert D.shape == (nq, k) and I.shape == (nq, k)
    if nq:
        Dr, Ir = R.flat_ip_search(emb, ids, q, k)
        same_ranking(D, I, Dr, Ir)
        assert np.all(I[:, min(k, rows):] == -1)


def test_duplicate_rows_tie_break_and_no_ids():
    emb = syn.corpus_embeddings(13, 4096, 128)
    emb[100] = emb[7]
    emb[3000] = emb[7]
    index = RU.construct_flatindex_from_embeddings(emb, None)
    RU.convert_index_to_gpu(index, [0], False)
    q = emb[7:8].copy()
    D, I = index.search(q, 5)
    assert I[0, :3].tolist() == [7, 100, 3000]          # equal scores: lower row position first
    assert D[0, 0] == D[0, 1] == D[0, 2]


def test_index_retrieve_batching_and_persistence(tmp_path):
    emb = syn.corpus_embeddings(14, 9000, 128)
    ids = np.arange(9000, dtype=np.int64) + 100
    q = syn.corpus_embeddings(15, 300, 128)
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    RU.write_index(index, str(tmp_path / "t.index"))
    index2 = RU.convert_index_to_gpu(RU.read_index(str(tmp_path / "t.index")), 0)
    s_all, i_all = RU.index_retrieve(index2, q, 20, batch=None)
    s_b, i_b = RU.index_retrieve(index2, q, 20, batch=128)
    assert isinstance(i_b, list) and len(i_b) == 300
    assert np.array_equal(np.array(i_b), i_all) and np.array_equal(np.array(s_b, dtype=np.float32), s_all)
    Dr, Ir = R.flat_ip_search(emb, ids, q, 20)
    same_ranking(s_all, i_all, Dr, Ir)
    with pytest.raises(RuntimeError):
        RU.read_index(str(tmp_path / "t.index")).search(q, 5)        # not on a GPU: refuses instead of searching on the CPU


def test_two_shards_merge_equals_global():
    emb = syn.corpus_embeddings(16, 10001, 128)
    q = syn.corpus_embeddings(17, 9, 128)
    Dr, Ir = R.flat_ip_search(emb, None, q, 50)
    parts = []
    for r in range(2):
        lo, hi = RU.ShardedFlatIPIndex.shard_bounds(10001, 2, r)
        idx = RU.construct_flatindex_from_embeddings(emb[lo:hi], np.arange(lo, hi, dtype=np.int64))
        RU.convert_index_to_gpu(idx, 0)
        parts.append(idx.search(q, 50))
    D, I = RU.merge_shard_results([p[0] for p in parts], [p[1] for p in parts], 50)
    same_ranking(D, I, Dr, Ir)


@pytest.mark.parametrize("rows,d,stride", [(10001, 768, 7), (3, 128, 1), (70000, 256, 64), (1, 64, 5), (777, 1280, 3)])
def test_attach_statistics_kernels_equal_the_numpy_restatement(rows, d, stride):
    """cldrd_index_col_mean / cldrd_index_center_cast / cldrd_map_ids (FlatIPIndex._attach and the id map of a search: torch arithmetic until
    round 5) against numpy: the mean row to one fp32 ulp of the fp64 mean, the fp16 scan shadow and the bf16 threshold sample of the centred
    rows BIT FOR BIT (fp32 subtraction, one RNE), the largest centred norm as the fp32 value of the fp64 row sums, the range flag."""
    rng = np.random.default_rng(rows + d)
    P = (rng.standard_normal((rows, d)) * 3.0 + 2.5).astype(np.float32)          # a common component, as CLS embeddings have
    Pd = torch.from_numpy(P).to(DEV)
    mu = ops.index_col_mean(Pd)
    mu_ref = P.astype(np.float64).mean(0)
    assert np.all(np.abs(mu.cpu().numpy().astype(np.float64) - mu_ref) <= np.spacing(np.abs(mu_ref).astype(np.float32)).astype(np.float64))
    s_rows = min(rows, (rows + stride - 1) // stride)
    s_rows = max(1, s_rows - 1) if s_rows > 2 else s_rows                          # fewer sample rows than the stride would give: the cut is honoured
    P16 = torch.empty(rows, d, dtype=torch.float16, device=DEV)
    sample = torch.zeros((s_rows + 7) // 8 * 8, d, dtype=torch.bfloat16, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    cmax = ops.index_center_cast(Pd, mu, P16, sample, stride, s_rows, flag)
    c = P - mu.cpu().numpy()[None, :]                                               # fp32 subtraction, as the kernel's
    assert np.array_equal(P16.cpu().numpy().view(np.uint16), c.astype(np.float16).view(np.uint16))
    want_s = torch.from_numpy(c[::stride][:s_rows]).to(torch.bfloat16)
    assert torch.equal(sample[:s_rows].cpu().view(torch.int16), want_s.view(torch.int16)) and not sample[s_rows:].any()
    want_max = np.float32((c.astype(np.float64) ** 2).sum(1).max())
    assert cmax.view(torch.float32).item() == want_max and int(flag.item()) == 0
    # a centred value outside the fp16 range raises the flag
    P2 = P.copy()
    P2[rows // 2, d // 2] = 1e6
    ops.index_center_cast(torch.from_numpy(P2).to(DEV), mu, P16, None, 1, 0, flag)
    assert int(flag.item()) == 1
    # id map: table or offset, -1 stays -1
    I = torch.from_numpy(rng.integers(-1, rows, size=(5, 9)).astype(np.int32)).to(DEV)
    table = torch.from_numpy((np.arange(rows, dtype=np.int64) * 7 + 3)).to(DEV)
    In = I.cpu().numpy().astype(np.int64)
    assert np.array_equal(ops.map_ids(I, table, 0).cpu().numpy(), np.where(In >= 0, In * 7 + 3, -1))
    assert np.array_equal(ops.map_ids(I, None, 1000).cpu().numpy(), np.where(In >= 0, In + 1000, -1))


def test_index_center_cast_in_chunks_equals_one_call():
    """cldrd_index_center_cast on rows [row0, row0 + rows): 104 rows as chunks of 64 + 40 leave the fp16 rows, the whole shard's sample (stride 3),
    the largest centred norm and the range flag (raised by a row of the second chunk) bit for bit as one call with row0 = 0 does."""
    rows, d, stride = 104, 128, 3
    P = (np.random.default_rng(104).standard_normal((rows, d)) * 3.0 + 2.5).astype(np.float32)
    P[70, 5] = 1e6                                          # outside the fp16 range
    Pd = torch.from_numpy(P).to(DEV)
    mu = ops.index_col_mean(Pd)
    s_rows = (rows + stride - 1) // stride

    def run(bounds):
        P16 = torch.zeros(rows, d, dtype=torch.float16, device=DEV)
        sample = torch.zeros((s_rows + 7) // 8 * 8, d, dtype=torch.bfloat16, device=DEV)
        flag, cmax = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for lo, hi in bounds:
            ops.index_center_cast(Pd[lo:hi], mu, P16[lo:hi], sample, stride, s_rows, flag, row0=lo, cmax=cmax)
        return P16.view(torch.int16), sample.view(torch.int16), cmax, flag
    whole, chunked = run([(0, rows)]), run([(0, 64), (64, rows)])
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
    assert int(whole[3].item()) == 1 and whole[1][:s_rows].any(dim=1).all() and int(whole[2].item()) != 0


@pytest.mark.parametrize("devices,with_ids", [([0, 0], True), ([0, 0, 0], False)])
def test_convert_index_to_gpu_device_list_shards_in_one_process(devices, with_ids):
    """The reference's LIST form, ``convert_index_to_gpu(index, [d0, d1, ...])`` (retriever/retrieval_utils.py:164-182: sharded clone, dead
    code there): one process, one row shard per list entry, per-shard search + cldrd_merge_topk_device.  One GPU per box, so the list names
    device 0 several times - the shard split, the id mapping, the device-to-device gather and the merge are what a [0..7] list runs.  Equal
    to the oracle's search of the whole index, incl. duplicated rows that land in DIFFERENT shards (tie -> global row position asc) and a
    k larger than one shard's contribution."""
    n = 10001
    emb = syn.corpus_embeddings(21, n, 128)
    emb[9000] = emb[7]                   # the same row in the first and the last shard
    emb[5000] = emb[7]
    ids = (np.arange(n, dtype=np.int64) * 3 + 11) if with_ids else None
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    multi = RU.convert_index_to_gpu(index, devices, False)
    assert isinstance(multi, RU.MultiDeviceFlatIPIndex) and len(multi.shards) == len(devices) and multi.ntotal == n
    assert sum(sh.ntotal for sh in multi.shards) == n
    q = np.concatenate([emb[7:8], syn.corpus_embeddings(22, 40, 128)])
    for k in (5, 300):
        D, I = RU.index_retrieve(multi, q, k, batch=None)
        Dr, Ir = R.flat_ip_search(emb, ids, q, k)
        same_ranking(D, I, Dr, Ir)
    D, I = multi.search(q[:1], 3)
    want = [7, 5000, 9000] if ids is None else [7 * 3 + 11, 5000 * 3 + 11, 9000 * 3 + 11]
    assert I[0].tolist() == want and D[0, 0] == D[0, 1] == D[0, 2]
    assert multi.last_merge["path"].startswith("device")
    # the single-device forms are unchanged
    one = RU.convert_index_to_gpu(RU.construct_flatindex_from_embeddings(emb, ids), [0], False)
    assert isinstance(one, RU.FlatIPIndex)
    D1, I1 = one.search(q, 300)
    Dm, Im = multi.search(q, 300)
    assert np.array_equal(I1, Im) and np.array_equal(D1, Dm)          # sharded in one process == the whole index on one device, bit for bit
    with pytest.raises(TypeError):
        RU.convert_index_to_gpu(index, "cuda:0")
    # a list longer than the index has rows: the empty shards are skipped
    tiny = RU.convert_index_to_gpu(RU.construct_flatindex_from_embeddings(emb[:2], None), [0, 0, 0], False)
    Dt, It = tiny.search(q[:2], 4)
    Drt, Irt = R.flat_ip_search(emb[:2], None, q[:2], 4)
    same_ranking(Dt, It, Drt, Irt)


@pytest.mark.parametrize("world,nq,k,tie_levels,short", [(8, 300, 1000, 16, ()), (8, 64, 1000, 1, (1, 5)), (2, 33, 50, 4, (1,)), (3, 17, 2000, 0, ()),
                                                        (8, 40, 1024, 2, (0, 1, 2, 3, 4, 5, 6, 7))])
def test_device_merge_of_shard_lists_equals_oracle_merge(world, nq, k, tie_levels, short):
    """cldrd_merge_topk_device (what rank 0 runs on lists gathered over RCCL): one sort launch over world * k candidates per query,
    ids and scores identical to the oracle's merge incl. cross-shard ties, -1 / -inf padding and k_out < k_in."""
    from test_distributed_cpu import _shard_lists
    Ds, Is = _shard_lists(world * 100 + k, world, nq, k, 1105228, tie_levels, short)
    allD = torch.from_numpy(np.stack(Ds)).to(DEV)
    allI = torch.from_numpy(np.stack(Is)).to(DEV)
    for k_out in (k, max(1, k // 3)):
        D, I = ops.merge_topk_device(allD, allI, k_out)
        Dr, Ir = R.merge_shard_results(Ds, Is, k_out)
        assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr)
    # and the native host merge on the same lists (the gloo path)
    Dh, Ih = ops.merge_topk_host(Ds, Is, k)
    Dr, Ir = R.merge_shard_results(Ds, Is, k)
    assert np.array_equal(Ih, Ir) and np.array_equal(Dh, Dr)


def test_device_merge_at_cfg5_size():
    """8 shards x 6 980 queries x top-1000 merged on the device: equal to the oracle on a query sample, sorted
    everywhere, and far below the 19-ms device search it follows (asked: <= 30 ms)."""
    from test_distributed_cpu import _shard_lists
    Ds, Is = _shard_lists(77, 8, 6980, 1000, 1105228, tie_levels=64, short=(3,))
    allD = torch.from_numpy(np.stack(Ds)).to(DEV)
    allI = torch.from_numpy(np.stack(Is)).to(DEV)
    ops.merge_topk_device(allD[:, :16].contiguous(), allI[:, :16].contiguous(), 1000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    D, I = ops.merge_topk_device(allD, allI, 1000)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    sel = np.arange(0, 6980, 53)
    Dr, Ir = R.merge_shard_results([d[sel] for d in Ds], [i[sel] for i in Is], 1000)
    Dn, In = D.cpu().numpy(), I.cpu().numpy()
    assert np.array_equal(In[sel], Ir) and np.array_equal(Dn[sel], Dr)
    assert (np.diff(Dn.astype(np.float64), axis=1) <= 0).all()
    print(f"device merge of 8 x 6980 x 1000: {ms:.2f} ms")
    assert ms < 30.0


def test_sharded_search_over_rccl_with_one_rank_takes_the_device_exchange(tmp_path):
    """ShardedFlatIPIndex over ProcessGroupNCCL (= RCCL): gather of device tensors + device merge.  One GPU per box, so the process group
    has ONE rank (force_exchange) - what runs is the real backend's gather and the merge kernel, not a scaling number."""
    import subprocess
    import sys
    code = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.getcwd())
import cldrd_amd.synthetic as syn
from cldrd_amd.retriever import retrieval_utils as RU
from oracle import retrieval_ref as R
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[1], RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
emb = syn.corpus_embeddings(31, 20011, 128)
q = syn.corpus_embeddings(32, 70, 128)
idx = RU.construct_flatindex_from_embeddings(emb, np.arange(20011, dtype=np.int64) * 3 + 5)
RU.convert_index_to_gpu(idx, 0)
sh = RU.ShardedFlatIPIndex(idx, 0, 1)
sh.force_exchange = True
D, I = sh.search(q, 100)
Dr, Ir = R.flat_ip_search(emb, np.arange(20011, dtype=np.int64) * 3 + 5, q, 100)
assert sh.last_merge.get("path", "").startswith("device"), sh.last_merge
assert np.array_equal(I, Ir), "ids differ"
assert np.allclose(D, Dr, rtol=1e-5, atol=0)
dist.destroy_process_group()
print("ok")
"""
    import socket
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    r = subprocess.run([sys.executable, "-c", code, str(port)], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_encode_and_cli_end_to_end(tmp_path):
    from oracle import encoder_ref as E
    from cldrd_amd.dataset import SyntheticSequenceDataset
    from cldrd_amd.retriever import index_text, retrieve_top_passages
    cfg = selftest.tiny_config()
    model = selftest.build_tiny_model(cfg).cuda().eval()
    ds = SyntheticSequenceDataset(300, 32, vocab=cfg.vocab_size, batch_size=128)
    embs, ids = RU.get_embeddings_from_scratch(model, ds.loader(), use_fp16=True, is_query=False, show_progress_bar=False)
    assert embs.shape == (300, cfg.dim) and embs.dtype == np.float32 and ids == list(range(300))
    qp, pp = selftest.oracle_params(model)
    b0 = ds[0]
    ref = E.cls_embs(pp, selftest.oracle_cfg(cfg), b0["seq"]).detach().numpy()
    assert np.abs(embs[:128] - ref).max() <= 3e-2 * np.abs(ref).max()
    # CLIs: save a checkpoint in the reference's DDP layout, index 500 synthetic passages, retrieve 20 synthetic queries
    mdir = tmp_path / "model"
    model.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp_path / "checkpoint_10.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in model.state_dict().items()}}, ckpt)
    a = index_text.get_args(["--resume", str(ckpt), "--model_name_or_path", str(mdir), "--index_dir", str(tmp_path / "index"),
                             "--max_length", "32", "--synthetic_rows", "500"])
    index_path = index_text.main(a)
    out = tmp_path / "runs" / "dev.run"
    b = retrieve_top_passages.get_args(["--resume", str(ckpt), "--model_name_or_path", str(mdir), "--index_path", index_path,
                                        "--max_length", "16", "--top_k", "7", "--synthetic_queries", "20", "--output_path", str(out)])
    retrieve_top_passages.main(b)
    lines = open(out).read().strip().split("\n")
    assert len(lines) == 20 * 7
    qid, docid, rank, score = lines[0].split("\t")
    assert rank == "1" and 0 <= int(docid) < 500 and float(score) == float(score)
    ranks = [int(l.split("\t")[2]) for l in lines[:7]]
    scores = [float(l.split("\t")[3]) for l in lines[:7]]
    assert ranks == list(range(1, 8)) and scores == sorted(scores, reverse=True)
    # the run file feeds the evaluator (reference evaluation/retrieval_evaluator.py): with the rank-3 document of every query marked
    # relevant, MRR@10 = 1/3, Recall@5 = 1, and every query is counted
    from cldrd_amd.evaluation import RankingEvaluator
    qrels = tmp_path / "qrels.tsv"
    with open(qrels, "w") as fh:
        for l in lines:
            q_, d_, r_, _ = l.split("\t")
            if r_ == "3":
                fh.write(f"{q_}\t0\t{d_}\t1\n")
    m = RankingEvaluator(str(qrels), mrr_at_k=[10], ndcg_at_k=[10], recall_at_k=[5], map_at_k=10).compute_metrics(str(out))
    assert m["QueriesRanked"] == 20 and m["MRR@10"] == pytest.approx(1 / 3) and m["Recall@5"] == 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nq,rows,d", [(128, 40000, 768), (37, 5003, 768), (16, 9000, 128), (128, 70001, 256), (256, 40000, 768), (200, 9000, 768)])
def test_scan_stream_and_tiled_report_the_same_candidates(nq, rows, d, dtype):
    if nq > 128 and dtype != torch.float16:
        pytest.skip("more than 128 queries per pass: fp16 shadow only")
    """The streaming scan (hit list on chip, flushed when it fills) and the tiled scan must report the same (query, row) sets
    with the same 16-bit-operand scores; only the order inside a query's list is unspecified."""
    Q = torch.from_numpy(syn.normal(21, nq * d).reshape(nq, d).astype(np.float32)).to(DEV).to(dtype)
    P = torch.from_numpy(syn.normal(22, rows * d).reshape(rows, d).astype(np.float32)).to(DEV).to(dtype)
    S = Q.float() @ P.float().T
    thr = torch.quantile(S[:, :4096], 1.0 - 40.0 / 4096, dim=1).contiguous()
    got = []
    for tiled in (False, True):
        counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
        cr = torch.full((nq, 2048), -1, dtype=torch.int32, device=DEV)
        cs = torch.zeros(nq, 2048, device=DEV)
        ops.topk_scan_filter(Q, P, thr, counts, cr, cs, tiled=tiled)
        c = counts.cpu().numpy()
        assert c[nq] == 0 and (c[:nq] <= 2048).all()
        crh, csh = cr.cpu().numpy(), cs.cpu().numpy()
        got.append([dict(zip(crh[q, :c[q]].tolist(), csh[q, :c[q]].tolist())) for q in range(nq)])
    Sh, th = S.cpu().numpy(), thr.cpu().numpy()
    for q in range(nq):
        assert got[0][q].keys() == got[1][q].keys()
        rows_q = np.fromiter(got[0][q].keys(), dtype=np.int64)
        assert len(rows_q) == len(set(rows_q.tolist())) and (rows_q >= 0).all() and (rows_q < rows).all()
        # every clear hit is present, nothing clearly below the threshold is (fp32 accumulation order differs from torch's)
        tol = 1e-3 * (1.0 + abs(th[q]))
        assert set(np.where(Sh[q] >= th[q] + tol)[0].tolist()) <= set(rows_q.tolist())
        assert (Sh[q, rows_q] >= th[q] - tol).all()
        a = np.array([got[0][q][r] for r in rows_q]); b = np.array([got[1][q][r] for r in rows_q])
        assert np.allclose(a, b, rtol=1e-5, atol=1e-5) and np.allclose(a, Sh[q, rows_q], rtol=1e-4, atol=1e-3)


def test_scan_stream_never_drops_a_hit_when_its_on_chip_lists_overflow():
    """A threshold far too low makes EVERY (query, row) pair a hit: far more than the streaming kernel's per-wave on-chip lists hold between
    two flush decisions.  Since round 4 the overflow goes straight to the global lists (a slow path, csrc/topk.hip: emit) instead of
    being counted as dropped and redone by the tiled kernels: every count must be exact, nothing reported as dropped, and with lists
    long enough the candidate sets must be complete."""
    nq, rows, d = 128, 30000, 768
    Q = torch.from_numpy(syn.normal(23, nq * d).reshape(nq, d).astype(np.float32)).to(DEV).half()
    P = torch.from_numpy(syn.normal(24, rows * d).reshape(rows, d).astype(np.float32)).to(DEV).half()
    thr = torch.full((nq,), -1e30, device=DEV)
    for tiled in (False, True):
        counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
        cr = torch.empty(nq, 64, dtype=torch.int32, device=DEV)
        cs = torch.empty(nq, 64, device=DEV)
        ops.topk_scan_filter(Q, P, thr, counts, cr, cs, tiled=tiled)
        c = counts.cpu().numpy()
        assert c[nq] == 0 and (c[:nq] == rows).all(), (tiled, c[nq], c[:4])
    # hits in bursts: one row in 50 scores high for EVERY query at once (the CLS-like regime: a common component in queries and rows),
    # nothing else comes near the threshold - 128 hits per hot row, far more per tile than a wave's list takes between two flush decisions
    rows2, cap = 20000, 1024
    u = torch.ones(d, device=DEV) / (d ** 0.5)
    Qc = (0.1 * Q.float() + 3.0 * u).half()
    P2 = 0.05 * torch.from_numpy(syn.normal(25, rows2 * d).reshape(rows2, d).astype(np.float32)).to(DEV)
    hot = torch.arange(7, rows2, 50, device=DEV)
    P2[hot] = 10.0 * u
    P2h = P2.half()
    S = Qc.float() @ P2h.float().T
    thr2 = torch.full((nq,), 15.0, device=DEV)
    assert bool((S[:, hot] > 20).all()) and int((S > 10).sum()) == nq * len(hot)
    counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    cr = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
    cs = torch.zeros(nq, cap, device=DEV)
    ops.topk_scan_filter(Qc, P2h, thr2, counts, cr, cs)
    c = counts.cpu().numpy()
    assert c[nq] == 0 and (c[:nq] == len(hot)).all(), (c[nq], c[:8])
    crh = cr.cpu().numpy()
    want = np.sort(hot.cpu().numpy())
    for q in range(nq):
        assert np.array_equal(np.sort(crh[q, :c[q]]), want)


@pytest.mark.parametrize("nq", [128, 256])
def test_scan_stream_flushes_its_hit_list(nq):
    """Every wave keeps its own on-chip hit list (~150 slots at d = 768).  ~8 hits per wave and tile over ~24 tiles per workgroup
    is more than a list holds, so every workgroup flushes mid-stream (without that the overflow would be REPORTED as dropped hits);
    the candidate sets must still equal the tiled kernel's (nothing lost, nothing duplicated, nothing reported as dropped)."""
    rows, d, cap = 200000, 768, 4096
    Q = torch.from_numpy(syn.normal(31, nq * d).reshape(nq, d).astype(np.float32)).to(DEV).half()
    P = torch.from_numpy(syn.normal(32, rows * d).reshape(rows, d).astype(np.float32)).to(DEV).half()
    S = Q.float() @ P.float().T
    # ~3100 hits per query at 128 queries, ~1550 at 256 (same hits per wave; the list level is checked with a lag of two tiles,
    # so a rate far beyond anything a search produces overflows a list between two checks - which is reported, not lost)
    frac = 0.0156 if nq == 128 else 0.0078
    thr = torch.quantile(S[:, :8000], 1.0 - frac, dim=1).contiguous()
    got = []
    for tiled in (False, True):
        counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
        cr = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
        cs = torch.zeros(nq, cap, device=DEV)
        ops.topk_scan_filter(Q, P, thr, counts, cr, cs, tiled=tiled)
        c = counts.cpu().numpy()
        assert c[nq] == 0 and (c[:nq] <= cap).all() and c[:nq].mean() > 0.6 * frac * rows
        crh = cr.cpu().numpy()
        got.append([np.sort(crh[q, :c[q]]) for q in range(nq)])
    for q in range(nq):
        assert len(np.unique(got[0][q])) == len(got[0][q])
        # the two kernels accumulate in different orders: rows within 1e-3 of the threshold may differ
        diff = np.setxor1d(got[0][q], got[1][q])
        assert len(diff) <= 4 and (np.abs(S[q, diff].cpu().numpy() - thr[q].item()) < 2e-3).all()


def _bench_corpus(rows, d, seed, chunk=1 << 20):
    """The bench.py corpus (unit-variance Gaussian direction x per-row norm ~ U(9, 12)), generated on the
    device in row chunks so the transient memory stays small at 8.8 M rows."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    P = torch.empty(rows, d, device=DEV)
    for lo in range(0, rows, chunk):
        blk = torch.randn(min(chunk, rows - lo), d, device=DEV, generator=gen)
        blk *= (9.0 + 3.0 * torch.rand(blk.shape[0], 1, device=DEV, generator=gen)) / blk.norm(dim=1, keepdim=True)
        P[lo:lo + blk.shape[0]] = blk
    return P


def _device_fp64_topk(P32, q32, k, chunk=1 << 19):
    """Independent exact reference on the device: fp64 scores rounded to fp32 once (the oracle's definition), running top-k over
    row chunks with torch, final order (score desc, row asc) fixed on the host."""
    nq = q32.shape[0]
    q64 = q32.double()
    best_s = torch.full((nq, 0), -float("inf"), device=DEV)
    best_i = torch.zeros((nq, 0), dtype=torch.int64, device=DEV)
    for lo in range(0, P32.shape[0], chunk):
        s = (q64 @ P32[lo:lo + chunk].double().T).float()
        idx = torch.arange(lo, lo + s.shape[1], device=DEV).expand(nq, -1)
        cs, ci = torch.cat([best_s, s], 1), torch.cat([best_i, idx], 1)
        top = torch.topk(cs, min(k + 8, cs.shape[1]), dim=1)
        best_s, best_i = top.values, torch.gather(ci, 1, top.indices)
    s, i = best_s.cpu().numpy().astype(np.float64), best_i.cpu().numpy()
    order = np.lexsort((i, -s), axis=1)[:, :k]
    return np.take_along_axis(s, order, 1).astype(np.float32), np.take_along_axis(i, order, 1)


@pytest.mark.parametrize("rows,d,nq,k", [(2873, 128, 128, 1000), (9000, 128, 64, 1000), (60000, 768, 40, 100)])
def test_scores_are_the_correctly_rounded_inner_products_on_heavy_tailed_rows(rows, d, nq, k):
    """Rows whose norms spread over two orders of magnitude: a low-ranked score of ~2 sits next to |q| |p| ~ 1e4, where an fp32-accumulated
    inner product is 1e-4 off (tools/search_fuzz.py found it).  The re-score accumulates in fp64 and rounds once, so D equals the fp64
    reference rounded to fp32 BIT FOR BIT and I follows (score desc, row asc) exactly - on the exhaustive and on the scanned path."""
    g = torch.Generator(device=DEV).manual_seed(3)
    P = torch.randn(rows, d, device=DEV, generator=g) * torch.exp(1.5 * torch.randn(rows, 1, device=DEV, generator=g))
    Q = torch.randn(nq, d, device=DEV, generator=g)
    index = RU.construct_flatindex_from_embeddings(P.cpu().numpy(), np.arange(rows, dtype=np.int64))
    RU.convert_index_to_gpu(index, 0, False)
    D, I = index.search(Q.cpu().numpy(), k)
    Dg, Ig = _device_fp64_topk(P, Q, k)
    assert np.array_equal(D, Dg), f"max relative score difference {np.max(np.abs(D - Dg) / (np.abs(Dg) + 1e-30)):.2e}"
    assert np.array_equal(I, Ig)


def test_cfg5_shard_search_matches_oracle_at_full_size():
    """BASELINE.json configs[4], one shard: 1 105 228 x 768 rows (8 841 823 / 8), 6 980 queries, k = 1000 (reference loop
    retriever/retrieval_utils.py:131-153).  The first 128-query batch is checked against the CPU oracle (oracle/retrieval_ref.py),
    64 queries spread over the rest against an independent fp64 reference on the device, and every query for the properties any
    exact top-k has.  The threshold / proof logic depends on the corpus size (lam = k S / n): this is the size the bench searches."""
    rows, d, nq, k = 1105228, 768, 6980, 1000
    P = _bench_corpus(rows, d, 1234)
    gen = torch.Generator(device=DEV).manual_seed(99)
    Q = torch.randn(nq, d, device=DEV, generator=gen)
    Q *= 10.0 / Q.norm(dim=1, keepdim=True)
    index = RU.FlatIPIndex.from_device_rows(P, id_offset=7 * rows)
    index.profile = True
    D, I = index.search(Q.cpu().numpy(), k)
    st = index.last_stats
    print(f"cfg5 shard: scans {st['scans']} rescans {st['rescans']} unproven after the first pass {st['unproven_first_pass']} "
          f"candidates/query {st['candidates'] / nq:.0f} rescored/query {st['rescored'] / nq:.0f} search {st['search_ms']:.1f} ms")
    assert st["scans"] >= (nq + index.query_tile - 1) // index.query_tile and st["rescans"] <= 2
    assert st["rescored"] / nq < 1.6 * k              # the 2 eps band stays a fraction of k: the re-score is not a second scan
    assert np.all(np.diff(D, axis=1) <= 0) and I.min() >= 7 * rows and I.max() < 8 * rows
    assert all(len(np.unique(I[q])) == k for q in range(0, nq, 97))
    Ph = P.cpu().numpy()
    Dr, Ir = R.flat_ip_search(Ph, None, Q[:128].cpu().numpy(), k)
    swaps = same_ranking(D[:128], I[:128] - 7 * rows, Dr, Ir)
    del Ph
    sel = np.arange(128 + 53, nq, (nq - 181) // 64)[:64]
    Dg, Ig = _device_fp64_topk(P, Q[torch.from_numpy(sel).to(DEV)], k)
    swaps += same_ranking(D[sel], I[sel] - 7 * rows, Dg, Ig)
    print(f"cfg5 shard: {swaps} positions differ inside near-tie runs (1e-5 relative) over {128 + 64} checked queries")


def test_cfg5_full_index_on_one_gpu_sampled_check():
    """The whole 8 841 823-row index on one MI355X (27 GB fp32 + 14 GB fp16 of the 288 GB): 128 queries, k = 1000; 16 of them are
    checked against the independent fp64 device reference, all of them for order / range / uniqueness."""
    rows, d, nq, k = 8841823, 768, 128, 1000
    P = _bench_corpus(rows, d, 4321)
    gen = torch.Generator(device=DEV).manual_seed(98)
    Q = torch.randn(nq, d, device=DEV, generator=gen)
    Q *= 10.0 / Q.norm(dim=1, keepdim=True)
    index = RU.FlatIPIndex.from_device_rows(P)
    index.profile = True
    D, I = index.search(Q.cpu().numpy(), k)
    st = index.last_stats
    print(f"cfg5 full: scans {st['scans']} rescans {st['rescans']} candidates/query {st['candidates'] / nq:.0f} "
          f"rescored/query {st['rescored'] / nq:.0f} search {st['search_ms']:.2f} ms")
    assert st["rescans"] <= 1
    assert np.all(np.diff(D, axis=1) <= 0) and I.min() >= 0 and I.max() < rows
    assert all(len(np.unique(I[q])) == k for q in range(nq))
    sel = np.arange(3, nq, 8)[:16]
    Dg, Ig = _device_fp64_topk(P, Q[torch.from_numpy(sel).to(DEV)], k)
    same_ranking(D[sel], I[sel], Dg, Ig)


def test_search_recovers_from_dropped_hits_on_a_small_dense_index():
    """k = 1000 on an index just above CAND_CAP rows with a FULL 256-query tile: ~5 % of every tile are hits, the streaming scan's
    per-wave lists overflow inside the two-tile snapshot lag and every query of the pass gets status bit 4.  The same kernel would
    drop the same hits again, so the retry must go through the tiled scan (or the exact fallback) - and still return the oracle's
    answer (this used to end in 'did not converge')."""
    n, d, nq, k = 20000, 768, 256, 1000
    emb = syn.corpus_embeddings(41, n, d)
    q = syn.corpus_embeddings(42, nq, d)
    index = RU.construct_flatindex_from_embeddings(emb, None)
    RU.convert_index_to_gpu(index, 0, False)
    D, I = index.search(q, k)
    st = index.last_stats
    print(f"dense tile: scans {st['scans']} rescans {st['rescans']} unproven first pass {st['unproven_first_pass']} fallback {st['fallback_queries']}")
    sel = np.arange(0, nq, 9)
    Dr, Ir = R.flat_ip_search(emb, None, q[sel], k)
    same_ranking(D[sel], I[sel], Dr, Ir)
    assert all(len(np.unique(I[j])) == k for j in range(nq))


def test_exact_chunked_fallback_matches_oracle():
    """The last resort of search_device (every row re-scored in fp32, CAND_CAP rows at a time, running merge by the sort kernel):
    called directly, against the oracle - including a chunk boundary that is not a multiple of anything and k above the last chunk."""
    n, d, nq, k = 2 * RU.CAND_CAP + 777, 128, 5, 1000
    emb = syn.corpus_embeddings(43, n, d)
    emb[n - 5] = emb[11]                         # a tie across chunks: lower row first
    q = syn.corpus_embeddings(44, nq, d)
    index = RU.FlatIPIndex(d)
    index.add(emb)
    index.to_gpu(0)
    Dd, Id = index._search_exhaustive_chunks(torch.from_numpy(q).to(DEV), k)
    Dr, Ir = R.flat_ip_search(emb, None, q, k)
    same_ranking(Dd.cpu().numpy(), Id.cpu().numpy().astype(np.int64), Dr, Ir)


def test_search_falls_back_to_the_exact_path_when_the_band_never_fits(monkeypatch):
    """More exact ties at the k-th score than any candidate buffer holds (9000 identical rows, k = 1000): no threshold can prove
    the list, and the search must end in the exact fallback with the tie rule (row position asc) instead of raising."""
    n, d, nq, k = 40000, 128, 3, 1000
    emb = syn.corpus_embeddings(45, n, d)
    emb[1000:10000] = emb[1000]                  # 9000 copies of one row
    q = np.repeat(emb[1000:1001] * 3.0, nq, axis=0).astype(np.float32)      # ... which is every query's best match
    q[1] += syn.corpus_embeddings(46, 1, d)[0] * 0.01
    index = RU.FlatIPIndex(d)
    index.add(emb)
    index.to_gpu(0)
    monkeypatch.setattr(RU, "MAX_ATTEMPTS", 3)
    D, I = index.search(q, k)
    st = index.last_stats
    assert st["fallback_queries"] > 0
    Dr, Ir = R.flat_ip_search(emb, None, q, k)
    assert np.array_equal(I, Ir) and np.allclose(D, Dr, rtol=1e-5)
    assert np.array_equal(I[0], np.arange(1000, 2000))


def _cls_like_corpus(rows, d, seed):
    return syn.cls_like_corpus(rows, d, seed, DEV)


def test_cls_like_anisotropic_corpus_at_shard_size():
    """exactness of the top-k on embeddings with a dominant common component (per-query score std / mean
    ~ 0.12), 1 105 228 rows x 768, k = 1000, 512 queries: checked against the independent fp64 device reference, and the candidate /
    re-score / rescan statistics are reported (they go into DESIGN.md)."""
    rows, d, nq, k = 1105228, 768, 512, 1000
    P, u = _cls_like_corpus(rows, d, 777)
    Q = syn.cls_like_queries(nq, u, 778)
    s0 = (P[:200000] @ Q[0])
    ratio = float(s0.std() / s0.mean())
    print(f"cls-like corpus: score mean {float(s0.mean()):.2f} std {float(s0.std()):.2f} (std/mean {ratio:.3f}), |q| {float(Q[0].norm()):.2f}, "
          f"max|p| {float(P[:200000].norm(dim=1).max()):.2f}")
    assert 0.08 < ratio < 0.16
    index = RU.FlatIPIndex.from_device_rows(P)
    index.profile = True
    D, I = index.search(Q.cpu().numpy(), k)
    st = index.last_stats
    print(f"cls-like shard: scans {st['scans']} rescans {st['rescans']} unproven first pass {st['unproven_first_pass']} fallback {st['fallback_queries']} "
          f"candidates/query {st['candidates'] / nq:.0f} rescored/query {st['rescored'] / nq:.0f} search {st['search_ms']:.1f} ms")
    assert np.all(np.diff(D, axis=1) <= 0) and I.min() >= 0 and I.max() < rows
    assert all(len(np.unique(I[j])) == k for j in range(0, nq, 7))
    sel = np.arange(1, nq, 8)[:64]
    Dg, Ig = _device_fp64_topk(P, Q[torch.from_numpy(sel).to(DEV)], k)
    swaps = same_ranking(D[sel], I[sel], Dg, Ig)
    print(f"cls-like shard: {swaps} positions differ inside near-tie runs (1e-5 relative) over {len(sel)} checked queries")
    assert st["fallback_queries"] == 0 and st["rescans"] <= 4


def _run_cli(mod, argv, env_extra, cwd):
    import subprocess
    import sys as _sys
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = cwd + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.Popen([_sys.executable, "-m", mod] + argv, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_sharded_index_and_retrieve_clis_equal_the_single_process_run(tmp_path):
    """SURVEY.md section 8e (e-index / e-retrieve), the reference flow retriever/index_text.py:84-109 -> retrieve_top_passages.py:85-107:
    index_text under RANK=0/1, WORLD_SIZE=2 writes two row-range shards; retrieve_top_passages as two ranks (gloo, both on this one GPU)
    searches its shard each and rank 0 merges: the run file must be the single-process run file BYTE FOR BYTE."""
    import socket
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = selftest.tiny_config()
    model = selftest.build_tiny_model(cfg).cuda().eval()
    mdir = tmp_path / "model"
    model.query_encoder.save_pretrained(str(mdir))
    ckpt = tmp_path / "checkpoint_10.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in model.state_dict().items()}, "scheduler": {"last_epoch": 3}}, ckpt)
    rows, nq, k = 1301, 45, 20
    common = ["--resume", str(ckpt), "--model_name_or_path", str(mdir)]
    # single process
    p = _run_cli("cldrd_amd.retriever.index_text", common + ["--index_dir", str(tmp_path / "one"), "--max_length", "32", "--synthetic_rows", str(rows)], {}, root)
    out, _ = p.communicate(timeout=600)
    assert p.returncode == 0, out[-2000:]
    one_index = str(tmp_path / "one" / "checkpoint_10.index")
    p = _run_cli("cldrd_amd.retriever.retrieve_top_passages", common + ["--index_path", one_index, "--max_length", "16", "--top_k", str(k), "--synthetic_queries", str(nq),
                                                                  "--output_path", str(tmp_path / "one" / "dev.run")], {}, root)
    out, _ = p.communicate(timeout=600)
    assert p.returncode == 0, out[-2000:]
    # two shards, written by two index_text processes (no collective on that path)
    for r in range(2):
        p = _run_cli("cldrd_amd.retriever.index_text", common + ["--index_dir", str(tmp_path / "two"), "--max_length", "32", "--synthetic_rows", str(rows)],
                     {"RANK": str(r), "WORLD_SIZE": "2", "LOCAL_RANK": "0"}, root)
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out[-2000:]
    shard_files = sorted(f for f in os.listdir(tmp_path / "two") if f.endswith(".meta.pkl") or f.endswith(".npy"))
    assert any("shard0of2" in f for f in shard_files) and any("shard1of2" in f for f in shard_files), shard_files
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [_run_cli("cldrd_amd.retriever.retrieve_top_passages",
                      common + ["--index_path", str(tmp_path / "two" / "checkpoint_10.index"), "--max_length", "16", "--top_k", str(k), "--synthetic_queries", str(nq),
                                "--output_path", str(tmp_path / "two" / "dev.run")],
                      {"RANK": str(r), "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)}, root) for r in range(2)]
    outs = [pr.communicate(timeout=600)[0] for pr in procs]
    assert all(pr.returncode == 0 for pr in procs), outs[0][-1500:] + outs[1][-1500:]
    a, b = (tmp_path / "one" / "dev.run").read_bytes(), (tmp_path / "two" / "dev.run").read_bytes()
    assert len(a.splitlines()) == nq * k
    assert a == b, "the merged run file of the two-shard run differs from the single-process run file"
