"""k-means on the device (csrc/kmeans.hip, hip_ops.kmeans_*, cldrd_amd.cluster.kmeans) against float64 and against a CPU emulation of the
documented summation order.

The assignment bound.  With u = 2^-24, E_ij = u ((d + 2) |x_i| |c_j| + 2 h_j), norms in float64: the standard bound of a d-term fma chain
(d u |x| |c|, first order; the two extra terms pay for the second order) plus the rounding of h and of the subtraction (u h each, as
|s| <= |x| |c| + h).  A point is RESOLVABLE when its float64 best score exceeds the second best by more than 2 max_j E_ij: there the kernel
must return the float64 argmax.  Elsewhere the chosen centroid's float64 score must lie within 2 max_j E_ij of the best.  ``best`` is within
E of the float64 score of the chosen centroid.  At most 1 % of the points of a case may be unresolvable, asserted from float64 alone.

The update has no tolerance: centroids equal a CPU fp32 emulation bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cldrd_amd import hip_ops as ops
from cldrd_amd.cluster import kmeans

U = 2.0 ** -24
DEV = "cuda"


def _case(n, k, d, seed, noise=0.1):
    """Gaussian points; centroids are noisy copies of k of them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    pick = torch.randperm(n, generator=g)[:k]
    c = x[pick] + noise * torch.randn(k, d, generator=g)
    return x, c


def _check_assign(x, c, assign, best=None):
    """the gap rule of the module docstring; x, c fp32 CPU tensors -> the share of unresolvable points"""
    x64, c64 = x.double(), c.double()
    h64 = 0.5 * (c64 * c64).sum(1)
    s = x64 @ c64.T - h64[None, :]
    e = U * ((x.shape[1] + 2) * x64.norm(dim=1)[:, None] * c64.norm(dim=1)[None, :] + 2.0 * h64[None, :])
    emax = e.max(dim=1).values
    top = s.topk(min(2, c.shape[0]), dim=1)
    gap = top.values[:, 0] - top.values[:, 1] if c.shape[0] > 1 else torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    resolvable = gap > 2.0 * emax
    a = assign.cpu()
    assert a.dtype == torch.int64 and a.shape == (x.shape[0],) and int(a.min()) >= 0 and int(a.max()) < c.shape[0]
    assert torch.equal(a[resolvable], top.indices[:, 0][resolvable]), "a resolvable point is not at the float64 argmax"
    chosen = s.gather(1, a[:, None])[:, 0]
    assert bool((chosen >= top.values[:, 0] - 2.0 * emax).all()), "an unresolvable point sits further than 2 E from the best"
    if best is not None:
        err = (best.cpu().double() - chosen).abs()
        bound = e.gather(1, a[:, None])[:, 0]
        assert bool((err <= bound).all()), float((err / bound).max())
    return 1.0 - float(resolvable.double().mean())


@pytest.mark.parametrize("n,k,d,pitch", [(1, 1, 32, 0), (127, 2, 64, 0), (129, 65, 384, 0), (1000, 257, 64, 0), (2000, 2000, 768, 0), (300, 70, 96, 4)])
def test_assign_against_float64(n, k, d, pitch):
    x, c = _case(n, k, d, seed=n + k)
    if pitch:
        buf = torch.full((n, d + pitch), float("nan"), device=DEV)          # the padding must never be read as data
        xd = buf[:, :d]
        xd.copy_(x)
        assert xd.stride(0) == d + pitch
    else:
        xd = x.to(DEV)
    cd = c.to(DEV)
    assign, best = ops.kmeans_assign(xd, cd, best=True)
    torch.cuda.synchronize()
    unresolvable = _check_assign(x, c, assign, best)
    print(f"kmeans_assign ({n}, {k}, {d}): {unresolvable:.4%} of the points unresolvable")
    assert unresolvable <= 0.01
    # the half norms may be handed in, and best is optional
    h = ops.kmeans_half_sqnorm(cd)
    assert torch.equal(ops.kmeans_assign(xd, cd, h), assign)
    assert torch.equal(h.cpu(), (0.5 * (c.double() * c.double()).sum(1)).float())


def test_ties_go_to_the_lower_index_and_a_point_on_a_centroid_picks_it():
    n, k, d = 700, 200, 64
    x, c = _case(n, k, d, seed=5)
    dup = {150 + j: j for j in range(0, 40, 3)}          # centroid j' is a copy of centroid j < j'
    for hi, lo in dup.items():
        c[hi] = c[lo]
    x[:k] = c                                            # point i < k IS centroid i (or the copy's original)
    assign = ops.kmeans_assign(x.to(DEV), c.to(DEV)).cpu()
    assert not set(assign.tolist()) & set(dup)
    want = torch.tensor([dup.get(i, i) for i in range(k)])
    assert torch.equal(assign[:k], want)
    _check_assign(x, c, assign)


def test_a_row_does_not_depend_on_the_launch():
    n, k, d = 1000, 257, 64
    x, c = _case(n, k, d, seed=11)
    xd, cd = x.to(DEV), c.to(DEV)
    h = ops.kmeans_half_sqnorm(cd)
    assign, best = ops.kmeans_assign(xd, cd, h, best=True)
    for a, b in ((37, 901), (129, 129 + 257), (1, 999)):
        sa, sb = ops.kmeans_assign(xd[a:b], cd, h, best=True)
        assert torch.equal(sa, assign[a:b]) and torch.equal(sb.view(torch.int32), best[a:b].view(torch.int32)), (a, b)
    for _ in range(40):
        ra, rb = ops.kmeans_assign(xd, cd, h, best=True)
        assert torch.equal(ra, assign) and torch.equal(rb.view(torch.int32), best.view(torch.int32))


def _update_emulation(x, assign, c):
    """CPU fp32: ascending rows, chunks of 64 summed left to right, chunk sums added left to right, one division"""
    x, out = x.numpy(), c.numpy().copy()
    a = assign.numpy()
    for j in range(out.shape[0]):
        rows = np.nonzero(a == j)[0]
        if rows.size == 0:
            continue
        total = None
        for s in range(0, rows.size, ops.SEGMENT_CHUNK):
            part = x[rows[s]].copy()
            for r in rows[s + 1:s + ops.SEGMENT_CHUNK]:
                part = part + x[r]
            total = part if total is None else total + part
        out[j] = total / np.float32(rows.size)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


@pytest.mark.parametrize("n,k,d", [(3000, 7, 64), (900, 40, 96)])
def test_update_equals_the_documented_order_bit_for_bit(n, k, d):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=g) * 3.0 + 1.0
    c = torch.randn(k, d, generator=g)
    # skewed sizes: one cluster of more than 16 chunks (n = 3000), many of less than one chunk, two EMPTY ones
    w = torch.ones(k)
    w[0], w[2], w[k - 1] = 3.0 * k, 0.0, 0.0
    assign = torch.multinomial(w, n, replacement=True, generator=g)
    sizes = torch.bincount(assign, minlength=k)
    assert int(sizes[2]) == 0 and int(sizes[k - 1]) == 0 and (n < 3000 or int(sizes[0]) > 16 * ops.SEGMENT_CHUNK)
    want = _update_emulation(x, assign, c)
    cd = c.to(DEV)
    h, got_sizes, n_empty = ops.kmeans_update(x.to(DEV), assign.to(DEV), cd)
    torch.cuda.synchronize()
    got = cd.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[2], c[2]) and torch.equal(got[k - 1], c[k - 1])          # an empty cluster keeps its row
    assert torch.equal(got_sizes.cpu().long(), sizes) and n_empty.cpu().tolist() == [2]
    assert torch.equal(h.cpu(), (0.5 * (got.double() * got.double()).sum(1)).float())


def _blobs(seed=0, per=150, d=64):
    g = torch.Generator().manual_seed(seed)
    centres = 10.0 * torch.randn(8, d, generator=g)
    labels = torch.arange(8).repeat_interleave(per)
    x = centres[labels] + 0.1 * torch.randn(8 * per, d, generator=g)
    shuffle = torch.randperm(8 * per, generator=g)
    return x[shuffle].contiguous(), labels[shuffle]


def test_kmeans_recovers_separated_blobs_and_is_reproducible():
    x, labels = _blobs()
    xd = x.to(DEV)
    init = torch.stack([x[(labels == j).nonzero()[0, 0]] for j in range(8)])
    r = kmeans(xd, 8, iters=5, init=init)
    assert torch.equal(r.assign.cpu(), labels) and r.sizes.tolist() == [150] * 8 and r.n_empty.tolist() == [0]
    assert r.moved.tolist() == [1200, 0, 0, 0, 0]
    assert torch.equal(init, torch.stack([x[(labels == j).nonzero()[0, 0]] for j in range(8)]))          # init is not written to
    # one seed, two runs: the same bits
    a, b = kmeans(xd, 8, iters=6, seed=3), kmeans(xd, 8, iters=6, seed=3)
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q)
    # the same rounds composed by hand from the three ops
    g = torch.Generator().manual_seed(3)
    c = xd[torch.randperm(x.shape[0], generator=g)[:8].to(DEV)].contiguous()
    h = ops.kmeans_half_sqnorm(c)
    prev, moved = torch.full((x.shape[0],), -1, device=DEV), []
    for _ in range(6):
        assign = ops.kmeans_assign(xd, c, h)
        moved.append(int((assign != prev).sum()))
        h, _, n_empty = ops.kmeans_update(xd, assign, c)
        prev = assign
    assign = ops.kmeans_assign(xd, c, h)
    assert torch.equal(c.view(torch.int32), a.centroids.view(torch.int32)) and torch.equal(assign, a.assign) and moved == a.moved.tolist()
    assert torch.equal(a.sizes, torch.bincount(assign, minlength=8)) and torch.equal(n_empty, a.n_empty)
    # random start: every point of the final assign sits at its nearest returned centroid
    _check_assign(x, a.centroids.cpu(), a.assign)
