#!/usr/bin/env python3
"""Randomised exactness check of FlatIPIndex.search: random shapes (rows 1e3 .. 4e5, d in {128, 256, 768}, 1 .. 700 queries, k in {1, 10, 100,
1000}) x random corpora (isotropic, CLS-like with a common component, duplicated rows, heavy-tailed norms, queries that ARE corpus rows)
against an independent fp64 reference computed on the device.  usage: tools/search_fuzz.py [cases] [seed] [fp16]
``fp16``: the index is attached in fp16-row mode (useFloat16=True) and the reference scores the rows that mode stores, by its definition:
fp32(<q, mu> + <q, R16[r]>) with the index's own mu and R16, sums in fp64."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from cldrd_amd.retriever import retrieval_utils as RU
from test_gpu_retrieval import same_ranking, _device_fp64_topk
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
DEV = "cuda"
FP16_ROWS = len(sys.argv) > 3 and sys.argv[3] == "fp16"


def _device_fp64_topk16(index, q32, k, chunk=1 << 19):
    """_device_fp64_topk over the stored rows mu + R16 of an index in fp16-row mode"""
    R16, nq = index._p16, q32.shape[0]
    q64 = q32.double()
    qmu = q64 @ torch.from_numpy(np.asarray(index.mu)).to(DEV).double()
    best_s = torch.full((nq, 0), -float("inf"), device=DEV)
    best_i = torch.zeros((nq, 0), dtype=torch.int64, device=DEV)
    for lo in range(0, R16.shape[0], chunk):
        s = (qmu[:, None] + q64 @ R16[lo:lo + chunk].double().T).float()
        idx = torch.arange(lo, lo + s.shape[1], device=DEV).expand(nq, -1)
        cs, ci = torch.cat([best_s, s], 1), torch.cat([best_i, idx], 1)
        top = torch.topk(cs, min(k + 8, cs.shape[1]), dim=1)
        best_s, best_i = top.values, torch.gather(ci, 1, top.indices)
    s, i = best_s.cpu().numpy().astype(np.float64), best_i.cpu().numpy()
    order = np.lexsort((i, -s), axis=1)[:, :k]
    return np.take_along_axis(s, order, 1).astype(np.float32), np.take_along_axis(i, order, 1)


bad = 0
t0 = time.time()
for c in range(cases):
    rows = int(10 ** rng.uniform(3, 5.6)); d = int(rng.choice([128, 256, 768])); nq = int(rng.choice([1, 3, 17, 128, 129, 300, 700]))
    k = int(rng.choice([1, 10, 100, 1000])); kind = str(rng.choice(["iso", "cls", "dup", "heavy", "self"]))
    g = torch.Generator(device=DEV).manual_seed(int(rng.integers(1 << 30)))
    P = torch.randn(rows, d, device=DEV, generator=g)
    Q = torch.randn(nq, d, device=DEV, generator=g)
    if kind == "cls":
        common = torch.randn(d, device=DEV, generator=g) * 3.0
        P = common[None] * (0.8 + 0.4 * torch.rand(rows, 1, device=DEV, generator=g)) + 0.3 * P
        Q = common[None] * (0.8 + 0.4 * torch.rand(nq, 1, device=DEV, generator=g)) + 0.3 * Q
    elif kind == "dup":
        P[rows // 2:] = P[: rows - rows // 2].clone()
    elif kind == "heavy":
        P = P * torch.exp(1.5 * torch.randn(rows, 1, device=DEV, generator=g))
    elif kind == "self":
        Q = P[torch.randint(0, rows, (nq,), device=DEV, generator=g)].clone()
    ids = np.arange(rows, dtype=np.int64) * 2 + 1
    index = RU.construct_flatindex_from_embeddings(P.cpu().numpy(), ids)
    RU.convert_index_to_gpu(index, 0, FP16_ROWS)
    D, I = index.search(Q.cpu().numpy(), k)
    st = index.last_stats
    sel = np.unique(rng.integers(0, nq, size=min(nq, 24)))
    Dg, Ig = (_device_fp64_topk16(index, Q[torch.from_numpy(sel).to(DEV)], k) if FP16_ROWS
              else _device_fp64_topk(P, Q[torch.from_numpy(sel).to(DEV)], k))
    Ig = np.where(Ig >= 0, Ig * 2 + 1, -1)
    try:
        swaps = same_ranking(D[sel], I[sel], Dg, Ig)
        ok = "ok"
    except AssertionError as e:
        bad += 1; ok = "MISMATCH " + str(e)[:200]; swaps = -1
    print(f"case {c}: rows {rows} d {d} nq {nq} k {k} {kind}: {ok} (near-tie swaps {swaps}; scans {st.get('scans')}, rescans {st.get('rescans')}, "
          f"exhaustive {st.get('exhaustive')}, fallback {st.get('fallback_queries', 0)})", flush=True)
    del index, P, Q
print(f"{cases} cases, {bad} mismatches, {time.time() - t0:.0f} s")
sys.exit(1 if bad else 0)
