"""k-means (Lloyd) of embedding rows on the device: what topic-aware batches cluster the query embeddings with
(``dataset.query_clusters`` -> ``trainer.nway_listwise --tas_clusters``).

A round is ``hip_ops.kmeans_assign`` (one launch on the f32-input MFMA, no [n, k] matrix in memory) and ``hip_ops.kmeans_update`` (the
members' sums by sort + fixed-order segment sum, one division).  Nothing uses a float atomic and every kernel has one schedule, so two runs
on the same input give the same bits.  The definition of an assignment stands in include/cldrd_hip.h."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import hip_ops as ops


class KMeansResult(NamedTuple):
    centroids: torch.Tensor      # fp32 [k, d]
    assign: torch.Tensor         # int64 [n]: the nearest of ``centroids`` (ties: the lower index)
    sizes: torch.Tensor          # int64 [k]: members per cluster under ``assign``
    moved: torch.Tensor          # int64 [iters]: points whose cluster changed in round t (round 0: all n)
    n_empty: torch.Tensor        # int32 [1]: clusters that were empty in the last update (they kept their centroid)


def kmeans(x, k, iters=20, seed=0, init=None) -> KMeansResult:
    """``x`` fp32 [n, d] on the GPU, contiguous.  Start centroids: ``init`` ([k, d]) or rows ``torch.randperm(n, generator=<CPU generator
    seeded seed>)[:k]`` of x.  Exactly ``iters`` rounds of assign + update and one final assign, so ``assign`` belongs to the returned
    centroids; no early stop and no host synchronisation inside the loop."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()):
        raise ValueError("kmeans: x must be a contiguous fp32 [n, d] tensor on the GPU (there is no CPU path)")
    n, d = x.shape
    k, iters = int(k), int(iters)
    if not 1 <= k <= n:
        raise ValueError(f"kmeans: 1 <= k <= n, got k = {k}, n = {n}")
    if iters < 0:
        raise ValueError("kmeans: iters must be >= 0")
    if init is not None:
        if tuple(init.shape) != (k, d):
            raise ValueError(f"kmeans: init must be [k, d] = [{k}, {d}], got {tuple(init.shape)}")
        centroids = init.to(device=x.device, dtype=torch.float32).contiguous().clone()
    else:
        g = torch.Generator()
        g.manual_seed(int(seed))
        centroids = x[torch.randperm(n, generator=g)[:k].to(x.device)].contiguous()
    h = ops.kmeans_half_sqnorm(centroids)
    moved = torch.zeros(iters, dtype=torch.int64, device=x.device)
    n_empty = torch.zeros(1, dtype=torch.int32, device=x.device)
    prev = torch.full((n,), -1, dtype=torch.int64, device=x.device)
    for t in range(iters):
        assign = ops.kmeans_assign(x, centroids, h)
        moved[t] = (assign != prev).sum()
        h, _, n_empty = ops.kmeans_update(x, assign, centroids)
        prev = assign
    assign = ops.kmeans_assign(x, centroids, h)
    return KMeansResult(centroids, assign, torch.bincount(assign, minlength=k), moved, n_empty)
