"""cldrd_wgrad_group under a per-problem chunk plan (csrc/gemm_tn.hip: wgrad_plan_group; run with -m gpu): groups whose problems are cut
differently in one launch - two long chunks, one long and a few short ones, short chunks only, a single chunk written directly - against a
float64 product of the same 16-bit operands, at the bar tests/test_gpu_kernels.py::test_wgrad_group sets for this kernel (rtol 1e-4, atol
1e-4 sqrt(M): fp32 accumulation-order noise only).  The layers of a group share their operand tensors (the launch cannot tell), so the
reference is one product per distinct shape."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cldrd_amd import hip_ops as ops

DEV = "cuda"


def layer(T, d=768, f=3072):
    return [(T, d, f, False), (T, f, d, True), (T, d, d, False), (T, 3 * d, d, True)]        # (M, N1, N2, bias), the backward's order


def cls_layer(Mc, T, d=768, f=3072):
    return [(Mc, d, f, False), (Mc, f, d, True), (Mc, d, d, False), (Mc, d, d, True), (T, 2 * d, d, True)]


GROUPS = {
    "cfg2": cls_layer(256, 32768) + layer(32768) * 5,              # the passage tower's group: 25 problems, long and short chunks, direct tiles
    "ragged": cls_layer(100, 20011) + layer(20011) * 2,            # packed batch: the last K tile is partial, the last chunks are short of their length
    "two_launches": [(5000, 256, 192, i % 3 == 0) for i in range(40)],      # more than 32 problems, 256 x 192 tiles
}


def operands(probs, dtype):
    """one (dY, X, float64 dY^T X, float64 column sums) per distinct (M, N1, N2); rows beyond M are never read: they hold NaN"""
    gen = torch.Generator(device=DEV).manual_seed(1234)
    out = {}
    for M, N1, N2, _ in probs:
        if (M, N1, N2) in out:
            continue
        dY = torch.full((M + 3, N1), float("nan"), dtype=dtype, device=DEV)
        X = torch.full((M + 3, N2), float("nan"), dtype=dtype, device=DEV)
        dY[:M] = torch.randn(M, N1, generator=gen, device=DEV).to(dtype)
        X[:M] = torch.randn(M, N2, generator=gen, device=DEV).to(dtype)
        a = dY[:M].double()
        out[(M, N1, N2)] = (dY, X, a.T @ X[:M].double(), a.sum(0))
        del a
    return out


def queue(probs, ops_by_shape, fill):
    q, outs = ops.WgradQueue(), []
    for M, N1, N2, bias in probs:
        dY, X, _, _ = ops_by_shape[(M, N1, N2)]
        dW = torch.full((N1, N2), fill, dtype=torch.float32, device=DEV)
        db = torch.full((N1,), -fill, dtype=torch.float32, device=DEV) if bias else None
        q.add(dY, X, dW, M, dbias=db)
        outs.append((dW, db))
    return q, outs


def check(probs, ops_by_shape, outs, base, scale):
    for (M, N1, N2, _), (dW, db) in zip(probs, outs):
        _, _, rW, rb = ops_by_shape[(M, N1, N2)]
        for got, ref, b, what in ((dW, rW, base, "dW"), (db, rb, -base, "dbias")):
            if got is None:
                continue
            ref = ref / scale + b
            err = (got.double() - ref).abs()
            tol = 1e-4 * math.sqrt(M) + 1e-4 * ref.abs()
            print(f"{what} {M}x{N1}x{N2}: max err {err.max().item():.3e}, smallest margin {(tol - err).min().item():.3e}")
            assert bool((err <= tol).all()), f"{what} {M}x{N1}x{N2}: {int((err > tol).sum())} off, max err {err.max().item():.3e}"


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_planned_group_matches_float64(name, dtype, accumulate):
    probs = GROUPS[name]
    data = operands(probs, dtype)
    fill = 2.0 if accumulate else float("nan")         # without `accumulate` every output element must be overwritten
    q, outs = queue(probs, data, fill)
    st = ops.new_loss_scale_state(DEV)
    scale = 64.0 if name != "ragged" else 1.0          # 1 / S applied where the gradients are written (slab reduction or direct epilogue)
    st[0], st[1] = scale, 1.0 / scale
    with ops.loss_scale(st.data_ptr() if scale != 1.0 else None):
        q.flush(accumulate=accumulate)
    torch.cuda.synchronize()
    check(probs, data, outs, 2.0 if accumulate else 0.0, scale)


@pytest.mark.parametrize("name", ["cfg2", "ragged"])
def test_planned_group_is_reproducible_eager_and_in_a_graph(name):
    """Two launches on the same operands give the same bits; so does a captured launch replayed three times (workspace reused by every replay)."""
    probs = GROUPS[name]
    data = operands(probs, torch.bfloat16)
    runs = []
    for _ in range(2):
        q, outs = queue(probs, data, float("nan"))
        q.flush()
        runs.append(outs)
    torch.cuda.synchronize()
    for (w0, b0), (w1, b1) in zip(*runs):
        assert torch.equal(w0, w1) and (b0 is None or torch.equal(b0, b1))
    q, outs = queue(probs, data, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            q.flush()
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(3):
        for dW, db in outs:
            dW.fill_(float("nan"))
            if db is not None:
                db.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for (w0, b0), (w1, b1) in zip(runs[0], outs):
            assert torch.equal(w0, w1) and (b0 is None or torch.equal(b0, b1)), f"replay {rep} differs from the eager launch"


@pytest.mark.parametrize("accumulate", [False, True])
def test_planned_group_leaves_the_clip_norm_of_what_it_wrote(accumulate):
    """The norm sink (hip_ops.norm_sink) under a plan that mixes reduced and directly written problems: the slots the launch fills must add up
    to the squared norm of everything it wrote, at the tolerance tests/test_gpu_amp16.py holds the trainer's norm to (2e-6 of the norm)."""
    probs = GROUPS["cfg2"]
    data = operands(probs, torch.bfloat16)
    q, outs = queue(probs, data, 0.5 if accumulate else float("nan"))
    slots = torch.full((256 * len(probs),), float("nan"), dtype=torch.float32, device=DEV)
    with ops.norm_sink(slots) as ns:
        q.flush(accumulate=accumulate)
    torch.cuda.synchronize()
    assert 0 < ns.used <= slots.numel(), ns.used
    sq = sum(dW.double().pow(2).sum().item() + (db.double().pow(2).sum().item() if db is not None else 0.0) for dW, db in outs)
    got, ref = math.sqrt(slots[:ns.used].double().sum().item()), math.sqrt(sq)
    print(f"norm from the sink {got:.9e}, of the buffers {ref:.9e}, relative difference {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= 2e-6 * ref
    assert bool(torch.isnan(slots[ns.used:]).all())
