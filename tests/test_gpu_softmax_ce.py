"""``cldrd_softmax_ce`` on the GPU: value, valid-row count and gradient against a float64 restatement of the header's definition (which is
itself checked against ``F.cross_entropy`` here), the duplicate rule, bit reproducibility, the wrappers, the trainer's step (eager and
replayed, fp16 and bf16, dot product and cosine, with and without in-batch columns) and the command lines end to end.

The bar of the kernel tests is the cosine tests' rule: the same formulas evaluated in fp32 with torch on the CPU are some distance from their
float64 evaluation; over the grid of `GRID` that distance is at most D_grad on a gradient (max |x - x64| / max |x64|) and D_loss on the
value (relative); the kernel may be at most 4 times as far, on every case of this file.  A different summation order passes, a wrong term
does not."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
import cldrd_amd.synthetic as syn
import selftest
from cldrd_amd import hip_ops as ops
from cldrd_amd import losses
from cldrd_amd.trainer import NwayTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 2), (2, 3), (4, 64), (3, 35), (5, 300), (2, 8192)]
TAUS = [1.0, 0.05]
POS_MINS = [None, 0.3]
REDUCTIONS = ["mean", "sum"]
GRID = [(B, Np, tau, pm, red) for (B, Np) in SHAPES for tau in TAUS for pm in POS_MINS for red in REDUCTIONS]


# ------------------------------------------------------------------------------------------------ the reference
def _cols(B, N, mode):
    return N if mode == 0 else (B * N if mode == 1 else 2 * N)


def column_pids(pids, mode):
    """int64 [B, Np]: the passage id behind every logit column (oracle/encoder_ref.py: in_batch_index)."""
    B, N = pids.shape
    flat = pids.reshape(-1)
    rows = []
    for b in range(B):
        own = list(range(b * N, (b + 1) * N))
        if mode == 1:
            own += [g if g < b * N else g + N for g in range((B - 1) * N)]
        elif mode == 2:
            own += list(range(((b + 1) % B) * N, ((b + 1) % B) * N + N))
        rows.append(flat[torch.tensor(own, dtype=torch.int64)])
    return torch.stack(rows)


def ce_reference(logits, labels, tau=1.0, pos_min=None, neg_max=0.0, reduction="mean", pids=None, mode=0, dtype=torch.float64):
    """The definition of include/cldrd_hip.h, term by term, in ``dtype`` on the CPU -> (loss, valid rows, d loss / d logits).  The classes are
    judged on the fp32 labels against fp32 bounds, as the kernel judges them."""
    B, Np = logits.shape
    lab = labels.float()
    z = logits.to(dtype) / torch.tensor(tau, dtype=dtype)
    colp = column_pids(pids, mode) if pids is not None else None
    grad = torch.zeros(B, Np, dtype=dtype)
    total, R = torch.zeros((), dtype=dtype), 0
    for b in range(B):
        pos = lab[b] >= torch.tensor(pos_min, dtype=torch.float32) if pos_min is not None else lab[b] == lab[b].max()
        neg = (lab[b] <= torch.tensor(neg_max, dtype=torch.float32)) & ~pos
        if colp is not None:
            kept = set(colp[b][~neg].tolist())
            neg = neg & torch.tensor([int(p) not in kept for p in colp[b].tolist()])
        if not pos.any() or not neg.any():
            continue
        R += 1
        m = z[b][pos | neg].max()
        e = torch.exp(z[b] - m)
        Z = e[neg].sum()
        D = e[pos] + Z
        n_pos = int(pos.sum())
        total = total + (torch.log(D) - (z[b][pos] - m)).sum() / n_pos
        w = 1.0 / (torch.tensor(tau, dtype=dtype) * n_pos)
        grad[b][pos] = w * (e[pos] / D - 1.0)
        grad[b][neg] = w * e[neg] * (1.0 / D).sum()
    if reduction == "mean" and R > 0:
        total, grad = total / R, grad / R
    return total, R, grad


def run_kernel(logits, labels, **kw):
    """The raw entry point on NaN-filled outputs -> (loss_out [2], grad) on the CPU."""
    loss_out = torch.full((2,), float("nan"), device=DEV)
    grad = torch.full(tuple(logits.shape), float("nan"), device=DEV)
    if kw.get("pids") is not None:
        kw = dict(kw, pids=kw["pids"].to(DEV))
    ops.softmax_ce(logits.to(DEV).contiguous(), labels.to(DEV).contiguous(), loss_out, grad, **kw)
    torch.cuda.synchronize()
    return loss_out.cpu(), grad.cpu()


def label_row(Np):
    """A label-mode-9-like row: the first third relT at 1/rank, then -0.25, -0.5 and 0 in turn."""
    k = max(1, Np // 3)
    rest = [(-0.25, -0.5, 0.0)[i % 3] for i in range(Np - k)]
    return torch.tensor([1.0 / (r + 1) for r in range(k)] + rest, dtype=torch.float32)


def grid_inputs(B, Np, seed=0):
    gen = torch.Generator().manual_seed(1000 + 31 * B + Np + seed)
    logits = (torch.randn(B, Np, generator=gen) * 3.0).contiguous()
    labels = label_row(Np).repeat(B, 1).contiguous()
    return logits, labels


def distances(got_loss, got_grad, ref):
    ref_loss, _, ref_grad = ref
    d_grad = float((got_grad.double() - ref_grad).abs().max()) / max(float(ref_grad.abs().max()), 1e-300)
    d_loss = abs(float(got_loss) - float(ref_loss)) / abs(float(ref_loss)) if float(ref_loss) != 0.0 else abs(float(got_loss))
    return d_grad, d_loss


@functools.lru_cache(maxsize=None)
def references():
    """The float64 reference of every grid case, computed once and left unchanged, and the bar taken from the fp32 evaluation of all of them."""
    refs, worst_g, worst_l = {}, 0.0, 0.0
    for B, Np, tau, pm, red in GRID:
        logits, labels = grid_inputs(B, Np)
        ref = ce_reference(logits, labels, tau, pm, 0.0, red)
        l32, _, g32 = ce_reference(logits, labels, tau, pm, 0.0, red, dtype=torch.float32)
        dg, dl = distances(l32, g32, ref)
        worst_g, worst_l = max(worst_g, dg), max(worst_l, dl)
        refs[(B, Np, tau, pm, red)] = ref
    return refs, 4.0 * worst_g, 4.0 * worst_l


def check(name, got, ref):
    _, bar_g, bar_l = references()
    loss_out, grad = got
    dg, dl = distances(loss_out[0], grad, ref)
    print(f"softmax_ce_parity {name}: gradient {dg:.3e} (bar {bar_g:.3e}) loss {dl:.3e} (bar {bar_l:.3e}) valid rows {int(loss_out[1])}")
    assert int(loss_out[1]) == ref[1] and float(loss_out[1]) == float(ref[1]), (name, loss_out, ref[1])
    assert torch.isfinite(grad).all() and torch.isfinite(loss_out).all(), name
    assert dg <= bar_g, (name, "gradient", dg, bar_g)
    assert dl <= bar_l, (name, "loss", dl, bar_l)


def test_the_reference_is_cross_entropy_for_one_positive():
    """CPU only: with one positive the closed form is F.cross_entropy(z[P u G], target) and its autograd gradient, neutral columns left out."""
    gen = torch.Generator().manual_seed(5)
    for B, Np, tau in ((3, 7, 1.0), (4, 33, 0.05)):
        logits = torch.randn(B, Np, generator=gen, dtype=torch.float64) * 2.0
        labels = torch.zeros(B, Np)
        labels[:, 2] = 1.0
        labels[:, 3] = 0.5                                                  # neutral
        labels[:, 5:] = -0.5
        x = logits.clone().requires_grad_(True)
        keep = [c for c in range(Np) if c != 3]
        want = F.cross_entropy(x[:, keep] / tau, torch.full((B,), 2, dtype=torch.int64))          # column 2 stays at position 2
        want.backward()
        loss, R, grad = ce_reference(logits, labels, tau)
        assert R == B and abs(float(loss) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
        assert float((grad - x.grad).abs().max()) <= 1e-13 * float(x.grad.abs().max()) and (grad[:, 3] == 0).all()
        s_loss, _, s_grad = ce_reference(logits, labels, tau, reduction="sum")
        assert abs(float(s_loss) - B * float(want.detach())) <= 1e-12 * abs(float(s_loss)) and torch.allclose(s_grad, grad * B, rtol=1e-13, atol=0)
    # several positives: the closed form against float64 autograd of the definition written with logsumexp
    logits = torch.randn(3, 20, generator=gen, dtype=torch.float64) * 2.0
    labels = label_row(20).repeat(3, 1)
    x = logits.clone().requires_grad_(True)
    pos, neg = labels[0] >= 0.3, labels[0] <= 0.0
    z = x / 0.05
    lse = torch.stack([torch.logsumexp(torch.cat([z[:, i:i + 1], z[:, neg]], dim=1), dim=1) - z[:, i] for i in torch.nonzero(pos).ravel()], dim=1)
    want = lse.mean(dim=1).mean()
    want.backward()
    loss, R, grad = ce_reference(logits, labels, 0.05, pos_min=0.3)
    assert R == 3 and int(pos.sum()) == 3 and abs(float(loss) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    assert float((grad - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


# ------------------------------------------------------------------------------------------------ 1. the kernel against the reference
@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("pos_min", POS_MINS)
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("B,Np", SHAPES)
def test_kernel_against_float64(B, Np, tau, pos_min, reduction):
    logits, labels = grid_inputs(B, Np)
    got = run_kernel(logits, labels, temperature=tau, pos_min=pos_min, reduction=reduction)
    check(f"B{B}_Np{Np}_tau{tau:g}_posmin{pos_min}_{reduction}", got, references()[0][(B, Np, tau, pos_min, reduction)])


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_a_tie_at_the_row_maximum_gives_several_positives(reduction):
    logits, labels = grid_inputs(3, 35, seed=1)
    labels[:, 4] = 1.0                                                       # columns 0 and 4 tie at the maximum, 1 .. 3 stay neutral
    labels[1, 0:12] = 0.5                                                    # row 1: twelve positives tie at 0.5, the rest is <= 0
    ref = ce_reference(logits, labels, 0.05, reduction=reduction)
    got = run_kernel(logits, labels, temperature=0.05, reduction=reduction)
    check(f"tie_{reduction}", got, ref)
    assert (got[1][0, [0, 4]] < 0).all() and (got[1][1, :12] < 0).all() and (got[1][0, 1:4] == 0).all()


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_rows_without_a_negative_or_without_a_positive(reduction):
    logits, labels = grid_inputs(4, 64, seed=2)
    labels[1] = labels[1].clamp_min(0.25)                                    # no negative
    labels[2] = float("nan")                                                 # no positive (nothing equals the maximum), no negative
    ref = ce_reference(logits, labels, 0.05, reduction=reduction)
    got = run_kernel(logits, labels, temperature=0.05, reduction=reduction)
    assert ref[1] == 2
    check(f"invalid_rows_{reduction}", got, ref)
    assert (got[1][1] == 0).all() and (got[1][2] == 0).all() and float(got[1][0].abs().max()) > 0
    # pos_min above every label: no positive anywhere; every row like row 1: no negative anywhere
    for lab, kw in ((labels, dict(pos_min=2.0)), (labels.nan_to_num(1.0).clamp_min(0.25), {})):
        loss_out, grad = run_kernel(logits, lab, temperature=0.05, reduction=reduction, **kw)
        assert loss_out.tolist() == [0.0, 0.0] and (grad == 0).all()


def test_neutral_columns_do_not_change_a_bit():
    logits, labels = grid_inputs(3, 35, seed=3)
    neutral = (labels > 0) & (labels < 1)
    assert neutral.any()
    base = run_kernel(logits, labels, temperature=0.05)
    for v in (1e30, -1e30, float("inf"), float("nan")):
        other = run_kernel(torch.where(neutral, torch.full_like(logits, v), logits), labels, temperature=0.05)
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]), v
    assert (base[1][neutral] == 0).all()


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_large_logits_do_not_overflow(reduction):
    gen = torch.Generator().manual_seed(9)
    B, Np = 3, 35
    logits = torch.randn(B, Np, generator=gen) + torch.where(torch.arange(Np) % 2 == 0, 3.0e3, -3.0e3)[None, :]
    labels = label_row(Np).repeat(B, 1)
    labels[2] = torch.roll(labels[2], 1)                                     # row 2: its positive (column 1) sits at -3e3 under negatives at +3e3
    for pm in POS_MINS:
        ref = ce_reference(logits, labels, 1.0, pm, reduction=reduction)
        got = run_kernel(logits, labels, temperature=1.0, pos_min=pm, reduction=reduction)
        check(f"logits_3e3_posmin{pm}_{reduction}", got, ref)
        assert float(ref[0]) > 1e3


# ------------------------------------------------------------------------------------------------ 2. the duplicate rule
BASE = 1 << 40


def planted(B, N):
    """ids beyond 2^40, distinct, then the planted repeats (labels of a row: [1, 1/2, 0]: positive, neutral, negative)."""
    pids = BASE * 3 + torch.arange(B * N, dtype=torch.int64).view(B, N) * 1000003
    if B >= 4:
        pids[1, 1] = pids[0, 0]            # another row's relT is this row's positive: that in-batch column of row 0 becomes neutral
        pids[2, 0] = pids[0, 1]            # ... is this row's neutral column: neutral too
        pids[3, 2] = pids[0, 2]            # ... is this row's negative: stays a negative
        pids[1, 2] = pids[1, 0]            # inside row 1's own columns: its negative repeats its positive
    else:
        pids[0, 2] = pids[0, 1]            # the row's own negative repeats its neutral column
    return pids


@pytest.mark.parametrize("B,N", [(4, 3), (1, 3)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_duplicate_rule(B, N, mode):
    Np = _cols(B, N, mode)
    gen = torch.Generator().manual_seed(40 + mode + B)
    logits = (torch.randn(B, Np, generator=gen) * 3.0).contiguous()
    labels = torch.cat([torch.tensor([1.0, 0.5, 0.0]).repeat(B, 1), torch.full((B, Np - N), -0.5)], dim=1).contiguous()
    distinct = BASE * 5 + torch.arange(B * N, dtype=torch.int64).view(B, N)
    for reduction in REDUCTIONS:
        kw = dict(temperature=0.5, reduction=reduction)                      # (no negative's exp underflows: their gradients are > 0)
        unmasked = run_kernel(logits, labels, **kw)
        if B == 1 and mode == 2:
            # the in-batch columns are the row's own passages: the repeats of its positive and neutral leave, the repeat of its negative stays
            got = run_kernel(logits, labels, pids=distinct, mode=mode, **kw)
            check(f"dup_B1_mode2_{reduction}", got, ce_reference(logits, labels, 0.5, reduction=reduction, pids=distinct, mode=mode))
            assert (got[1][0, [3, 4]] == 0).all() and float(got[1][0, 5]) > 0 and not torch.equal(got[1], unmasked[1])
            # a row of relT only (label mode 6): every in-batch column ends up neutral, no negative is left
            relT = torch.cat([torch.tensor([[1.0, 0.5, 1.0 / 3]]), torch.full((1, 3), -0.5)], dim=1)
            loss_out, grad = run_kernel(logits, relT, pids=distinct, mode=mode, **kw)
            assert loss_out.tolist() == [0.0, 0.0] and (grad == 0).all()
        else:
            same = run_kernel(logits, labels, pids=distinct, mode=mode, **kw)            # no repeat: the unmasked result, bit for bit
            assert torch.equal(same[0], unmasked[0]) and torch.equal(same[1], unmasked[1])
        pids = planted(B, N)
        ref = ce_reference(logits, labels, 0.5, reduction=reduction, pids=pids, mode=mode)
        got = run_kernel(logits, labels, pids=pids, mode=mode, **kw)
        check(f"dup_B{B}_N{N}_mode{mode}_{reduction}", got, ref)
        colp = column_pids(pids, mode)
        if B == 4:
            assert float(got[1][1, 2]) == 0.0 and ref[1] == (3 if mode == 0 else 4)          # row 1 keeps a negative only among in-batch columns
            if mode == 1:
                for pid, zero in ((pids[0, 0], True), (pids[0, 1], True), (pids[0, 2], False)):
                    cols = torch.nonzero(colp[0][N:] == pid).ravel() + N
                    assert len(cols) == 1 and (float(got[1][0, cols[0]]) == 0.0) == zero, (int(pid), zero)
        else:
            assert float(got[1][0, 2]) == 0.0


# ------------------------------------------------------------------------------------------------ 3. determinism and the wrappers
def test_equal_bits_call_after_call_and_every_element_written():
    logits, labels = grid_inputs(5, 300)
    pids = BASE + torch.randint(0, 40, (5, 60), generator=torch.Generator().manual_seed(3), dtype=torch.int64)
    for kw in (dict(temperature=0.05), dict(temperature=0.05, reduction="sum", pos_min=0.3), dict(temperature=0.05, pids=pids, mode=1)):
        first = run_kernel(logits, labels, **kw)                      # (run_kernel starts from NaN-filled buffers)
        assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all()
        for _ in range(3):
            again = run_kernel(logits, labels, **kw)
            assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("B,Np", [(1, 4), (3, 35), (300, 4)])
def test_forty_calls_in_a_row_give_the_bits_of_the_first(B, Np, streams):
    """More launches than the kernel has arrival slots, back to back on one stream or alternating over two: every launch finds its slot at
    zero and leaves it at zero, and the workgroup that arrives last (B = 1: the first ticket is the last; B = 300: more rows than threads in
    the final sum) adds the rows and rescales the gradient of its own launch.  The first call at the bars of test_kernel_against_float64.
    (tau = 1 on the inputs of seed 1: at tau = 0.05 the one row of B = 1 has a largest gradient entry of 1.6e-54 in float64, below the range of
    fp32, where a relative bar says nothing; here the fp32 restatement of all three cases is within 2e-7 of float64.)"""
    logits, labels = grid_inputs(B, Np, seed=1)
    ref = ce_reference(logits, labels, 1.0)
    ld, lb = logits.to(DEV), labels.to(DEV)
    outs = [(torch.full((2,), float("nan"), device=DEV), torch.full((B, Np), float("nan"), device=DEV)) for _ in range(40)]
    lanes = [torch.cuda.Stream() for _ in range(streams)]
    for s in lanes:
        s.wait_stream(torch.cuda.current_stream())
    for i, (loss_out, grad) in enumerate(outs):
        with torch.cuda.stream(lanes[i % streams]):
            ops.softmax_ce(ld, lb, loss_out, grad, temperature=1.0)
    for s in lanes:
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = outs[0][0].cpu(), outs[0][1].cpu()
    check(f"forty_calls_B{B}_Np{Np}_streams{streams}", first, ref)
    for i, (loss_out, grad) in enumerate(outs[1:], 1):
        assert torch.equal(loss_out.cpu().view(torch.int32), first[0].view(torch.int32)), i
        assert torch.equal(grad.cpu().view(torch.int32), first[1].view(torch.int32)), i


@pytest.mark.parametrize("mode", [0, 1])
def test_autograd_op_and_module_equal_the_raw_call(mode):
    B, N = 4, 6
    logits, labels = grid_inputs(B, _cols(B, N, mode), seed=4)
    pids = BASE + torch.randint(0, 12, (B, N), generator=torch.Generator().manual_seed(8), dtype=torch.int64)
    want = run_kernel(logits, labels, temperature=0.05, pos_min=0.3, neg_max=-0.1, reduction="mean", pids=pids, mode=mode)
    x = logits.to(DEV).requires_grad_(True)
    out, _ = torch.ops.cldrd.softmax_ce(x, labels.to(DEV), pids.to(DEV), mode, 0.05, 0.3, -0.1, True)
    (out[0] * 3.0).backward()
    assert torch.equal(out.detach().cpu(), want[0]) and torch.equal(x.grad.cpu(), want[1] * 3.0)
    x2 = logits.to(DEV).requires_grad_(True)
    mod = losses.SoftmaxCE(temperature=0.05, pos_min=0.3, neg_max=-0.1)
    value = mod(x2, labels.to(DEV), pids=pids.to(DEV), mode=mode, nway=N)
    value.backward()
    assert torch.equal(value.detach().cpu(), want[0][0]) and torch.equal(x2.grad.cpu(), want[1]) and float(mod.last_valid) == float(want[0][1])
    plain = losses.SoftmaxCE(temperature=0.05, reduction="sum")(logits.to(DEV), labels.to(DEV))
    assert torch.equal(plain.cpu(), run_kernel(logits, labels, temperature=0.05, reduction="sum")[0][0])
    torch.library.opcheck(torch.ops.cldrd.softmax_ce, (logits.to(DEV), labels.to(DEV), pids.to(DEV), mode, 0.05, None, 0.0, True),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(Exception):
        torch.ops.cldrd.softmax_ce(logits, labels, None, 0, 0.05, None, 0.0, True)               # CPU tensors: no kernel, no fall-back


# ------------------------------------------------------------------------------------------------ 4. the trainer's step
def _model(mode, cosine=None, cfg=None, seed=3, std=0.1):
    from cldrd_amd.models import NwayDualEncoder
    kw = dict(cosine=True, cosine_scale=cosine) if cosine else {}
    model = NwayDualEncoder(cfg or selftest.tiny_config(), share_weights=False, in_batch_loss=mode != 0, all_in_batch_neg=mode == 1, **kw)
    with torch.no_grad():
        for ti, tower in enumerate(model.towers()):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed + ti, name, tuple(p.shape), std=std, perturb=True))
    return model.cuda().train()


def _dev(batch):
    return {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}


def _batch(seed, B=3, N=4, Lq=8, Lp=16, vocab=512, pids=False):
    """a padded batch with the rank labels; ``pids``: plus passage ids that repeat within and across rows, other ids every seed"""
    batch = syn.nway_batch(seed, B, N, Lq, Lp, vocab=vocab, ragged=True, label_kind="mode9")
    if pids:
        batch["nway_pids"] = BASE + torch.randint(0, 2 * N, (B, N), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    return _dev(batch)


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("cosine", [None, 20.0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_step_hands_its_own_logits_and_labels_to_the_kernel(mode, cosine, amp, monkeypatch):
    """loss_out and dlogits of a step are the kernel's on that step's logits, the label row with -0.5 on the in-batch columns and the
    batch's passage ids; the value is the float64 reference's on those logits."""
    from cldrd_amd.trainer import nway_listwise as T
    monkeypatch.setenv("CLDRD_AMP", amp)
    monkeypatch.setenv("CLDRD_GRAPH", "0")
    B, N = 3, 4
    tr = NwayTrainer(_model(mode, cosine), loss="softmax_ce", ce_temperature=0.5, ce_mask_duplicate_pids=True, learning_rate=1e-3,
                     warmup_steps=0, total_steps=10)
    assert tr.amp16 == (amp == "fp16") and tr.cosine == bool(cosine)
    seen = []
    real = ops.softmax_ce

    def spy(logits, labels, loss_out, grad, **kw):
        real(logits, labels, loss_out, grad, **kw)
        seen.append((logits, labels, loss_out, grad, kw))
    monkeypatch.setattr(T.ops, "softmax_ce", spy)
    batch = _batch(70 + mode, B, N, pids=True)
    loss_out, logits = tr.forward_backward(batch)
    torch.cuda.synchronize()
    monkeypatch.setattr(T.ops, "softmax_ce", real)
    assert len(seen) == 1
    s_logits, s_labels, s_loss, s_grad, kw = seen[0]
    Np = _cols(B, N, mode)
    assert s_logits.data_ptr() == logits.data_ptr() and s_loss.data_ptr() == loss_out.data_ptr() and tuple(logits.shape) == (B, Np)
    assert kw["mode"] == mode and kw["nway"] == N and kw["temperature"] == 0.5 and kw["pos_min"] is None and kw["neg_max"] == 0.0
    assert torch.equal(kw["pids"], batch["nway_pids"])
    assert torch.equal(s_labels[:, :N], batch["labels"]) and (s_labels[:, N:] == -0.5).all()
    if cosine:
        assert float(logits.abs().max()) <= cosine * (1 + 1e-6)
    want = run_kernel(logits.cpu(), s_labels.cpu(), temperature=0.5, pids=batch["nway_pids"].cpu(), mode=mode)
    assert torch.equal(loss_out.cpu(), want[0]) and torch.equal(s_grad.cpu(), want[1])
    check(f"step_mode{mode}_cos{cosine}_{amp}", want, ce_reference(logits.cpu(), s_labels.cpu(), 0.5, pids=batch["nway_pids"].cpu(), mode=mode))
    assert float(loss_out[1]) >= 1 and float(tr.flat_g.abs().max()) > 0 and torch.isfinite(tr.flat_g).all()
    # without the flag the ids are not read; a batch without them is refused by a trainer that masks
    plain = NwayTrainer(_model(mode, cosine), loss="softmax_ce", ce_temperature=0.5, learning_rate=1e-3, warmup_steps=0, total_steps=10)
    lo, lg = plain.forward_backward({k: v for k, v in batch.items() if k != "nway_pids"})
    assert torch.equal(lo.cpu(), run_kernel(lg.cpu(), s_labels.cpu(), temperature=0.5)[0])
    with pytest.raises(ValueError, match="nway_pids"):
        tr.forward_backward({k: v for k, v in batch.items() if k != "nway_pids"})


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def test_one_training_step_against_the_oracle_towers():
    """tests/test_gpu_cosine.py: test_one_training_step_against_the_oracle_towers with the float64 reference of this file on top of the
    oracle's float64 logits (cosine scale 20, temperature 0.5: an effective temperature of 1/40), under that test's bars."""
    from oracle import encoder_ref as E
    from test_gpu_model import small_cfg
    cfg = small_cfg("distilbert")
    model = _model(0, 20.0, cfg=cfg)
    batch = syn.nway_batch(4680, 3, 5, 10, 40, vocab=cfg.vocab_size, ragged=True, label_kind="mode9")
    qp, pp = ({k: v.double().requires_grad_(True) for k, v in d_.items()} for d_ in selftest.oracle_params(model))
    ocfg = selftest.oracle_cfg(cfg)
    ref = 20.0 * F.cosine_similarity(E.cls_embs(qp, ocfg, batch["query"]).unsqueeze(1), E.nway_passage_embs(pp, ocfg, batch["nway_passages"]),
                                     dim=-1, eps=1e-8)
    ref_logits = ref.detach()
    ref_loss, R, dl = ce_reference(ref_logits, batch["labels"], 0.5)
    ref_loss = float(ref_loss)
    ref.backward(dl)
    tr = NwayTrainer(model, loss="softmax_ce", ce_temperature=0.5, learning_rate=1e-3, warmup_steps=0, total_steps=100)
    loss_out, logits = tr.forward_backward(batch)
    torch.cuda.synchronize()
    got, ref_np = logits.cpu().numpy(), ref_logits.numpy()
    scale = np.abs(ref_np).max()
    print(f"softmax_ce step: logits off {np.abs(got - ref_np).max() / scale:.3e} of max |logit| {scale:.3f}; loss {loss_out[0].item():.5f} oracle {ref_loss:.5f}")
    assert R == 3 and float(loss_out[1]) == 3.0
    assert np.abs(got - ref_np).max() <= 2e-2 * scale, f"logits off: {np.abs(got - ref_np).max() / scale:.3e}"
    assert loss_out[0].item() == pytest.approx(ref_loss, rel=5e-2, abs=1e-3)
    checked = 0
    for tname, tower, ref_params in (("query_encoder", model.query_encoder, qp), ("passage_encoder", model.passage_encoder, pp)):
        tower.ensure_grads()
        all_g, all_r = [], []
        for name, p in tower.named_flat():
            gg, rr = p.grad.detach().cpu().numpy(), ref_params[name].grad.numpy()
            all_g.append(gg.ravel()), all_r.append(rr.ravel())
            if np.linalg.norm(rr) > 1e-3 * max(1.0, ref_loss):          # skip analytically-zero grads (k bias)
                thr = 0.99 if "token_type" in name else 0.995
                checked += 1
                assert _cos(gg, rr) > thr, f"{tname}.{name}: cosine {_cos(gg, rr):.5f}"
                assert np.linalg.norm(gg) == pytest.approx(np.linalg.norm(rr), rel=5e-2), f"{tname}.{name}"
        assert _cos(np.concatenate(all_g), np.concatenate(all_r)) > 0.999
    assert checked >= 20, checked


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
@pytest.mark.parametrize("dup", [False, True])
def test_deterministic_replayed_steps_equal_eager_ones_and_runs_repeat(dup, amp, monkeypatch):
    """--deterministic, in-batch columns, cosine: three eager steps, the capture and replays against a run that never captures - the whole
    gradient buffer, the parameters and both moments bit for bit - and a second replayed run against the first.  With the duplicate flag the
    passage ids are one more input of the captured step and change every step."""
    from test_gpu_deterministic import small_cfg
    monkeypatch.setenv("CLDRD_AMP", amp)
    ends = []
    for graph in ("1", "0", "1"):
        monkeypatch.setenv("CLDRD_GRAPH", graph)
        cfg = small_cfg()
        torch.manual_seed(0)
        tr = NwayTrainer(_model(1, 20.0, cfg=cfg, seed=11, std=0.05), loss="softmax_ce", ce_temperature=0.5, ce_mask_duplicate_pids=dup,
                         learning_rate=3e-3, warmup_steps=5, total_steps=40, deterministic=True)
        counts = []
        for i in range(8):
            batch = _batch(300 + i, 3, 4, 8, 16, vocab=cfg.vocab_size, pids=dup)
            assert len(tr._step_inputs(batch)) == (6 if dup else 5)
            counts.append(tr.train_step(batch)[1].item())
        torch.cuda.synchronize()
        assert bool(tr._graphs) == (graph == "1") and min(counts) >= 1.0
        assert torch.isfinite(tr.flat_p).all().item() and float(tr.m.abs().max()) > 0
        ends.append((tr.flat_g.clone(), tr.flat_p.clone(), tr.m.clone(), tr.v.clone()))
    for other in ends[1:]:
        for a, b, name in zip(ends[0], other, ("flat_g", "flat_p", "m", "v")):
            assert torch.equal(a, b), name


def test_softmax_ce_learns():
    """dropout as configured, one fixed batch with in-batch columns, 30 steps: the loss falls and the train MRR rises."""
    batch = _batch(4680, 4, 6, 8, 24)
    tr = NwayTrainer(_model(1, std=0.05), loss="softmax_ce", ce_temperature=0.5, learning_rate=1e-3, warmup_steps=0, total_steps=1000)
    losses_, mrr = [], []
    for _ in range(30):
        losses_.append(tr.train_step(batch)[0].item())
        mrr.append(tr.train_metrics(tr.last_logits, tr.metric_labels(batch, tr.last_logits.shape[1]))[0])
    print(f"softmax_ce: loss {losses_[0]:.6g} at the first step, {losses_[-1]:.6g} after 30; train MRR {mrr[0]:.3f} -> {mrr[-1]:.3f}")
    assert np.isfinite(losses_).all() and losses_[-1] < losses_[0] and mrr[-1] > mrr[0]


# ------------------------------------------------------------------------------------------------ 5. the command lines end to end
def test_command_lines_end_to_end(tmp_path):
    """Train on the committed dataset fixture with the in-batch columns, cosine scoring and the duplicate mask, validating on a dev run; index
    and retrieve with the checkpoint; a second line with the distillation term behind the new loss."""
    from cldrd_amd.retriever import index_text as I, retrieve_top_passages as S
    from cldrd_amd.retriever.retrieval_utils import read_index
    from cldrd_amd.trainer import nway_listwise as T
    from toy_tokenizer import make_tokenizer
    fix = os.path.join(conftest.GOLDEN, "nway_dataset_fixture")
    queries, collection, train_path = (os.path.join(fix, n) for n in ("queries.tsv", "collection.tsv", "train_10relT_20neg.jsonl"))
    tok_dir = str(tmp_path / "tok")
    make_tokenizer().save_pretrained(tok_dir)
    student = selftest.build_tiny_model(selftest.tiny_config(), std=0.05)
    mdir = str(tmp_path / "student")
    student.query_encoder.save_pretrained(mdir)
    ckpt0 = tmp_path / "checkpoint_0.pth.tar"
    torch.save({"state_dict": {"module." + k: v.cpu() for k, v in student.state_dict().items()}}, ckpt0)
    rows = [json.loads(line) for line in open(train_path)]
    dev_run, qrels = str(tmp_path / "dev.run.tsv"), str(tmp_path / "qrels.dev.tsv")
    open(dev_run, "w").write("".join(f"{r['qid']}\t{p}\t{k + 1}\t{10.0 - k}\n" for r in rows[:6] for k, p in enumerate(r["most_hard_pids"][:3] + r["relT_pids"][:2])))
    open(qrels, "w").write("".join(f"{r['qid']}\t0\t{r['relT_pids'][0]}\t1\n" for r in rows[:6]))
    common = ["--experiment_folder", str(tmp_path), "--queries_path", queries, "--collection_path", collection, "--label_mode", "9",
              "--model_name_or_path", mdir, "--model_checkpoint", str(ckpt0), "--tokenizer_name_or_path", tok_dir, "--query_max_len", "8",
              "--passage_max_len", "24", "--train_batch_size", "4", "--logging_steps", "3", "--evaluate_steps", "3", "--warmup_steps", "1",
              "--num_train_epochs", "2", "--learning_rate", "1e-3", "--loader_workers", "0", "--loss", "softmax_ce", "--ce_temperature", "0.5"]
    tr = T.train(T.set_env(T.get_args(common + [
        "--run_folder", "ce", "--training_path", train_path, "--in_batch_loss", "--all_in_batch_neg", "--apply_consine_similarity",
        "--cosine_scale", "20", "--ce_mask_duplicate_pids", "--dev_path", dev_run, "--dev_queries_path", queries, "--dev_qrels_path", qrels])))
    assert tr.global_step == 6 and tr.loss_kind == "softmax_ce" and tr.ce_mask_duplicate_pids and tr.cosine
    assert tuple(tr.last_logits.shape) == (4, 120) and float(tr.last_logits.abs().max()) <= 20.0 * (1 + 1e-6)
    assert torch.isfinite(tr.flat_p).all().item() and tr.skipped_steps() == 0
    run_dir = tmp_path / "ce"
    log = (run_dir / "log" / "train_logs.log").read_text().splitlines()
    assert [ln.split("\t")[1] for ln in log[1:]] == ["6"] and float(log[1].split("\t")[2]) > 0.0
    dev_log = (run_dir / "log" / "dev_logs.log").read_text().splitlines()
    assert len(dev_log) == 3 and [ln.split("\t")[1] for ln in dev_log[1:]] == ["3", "6"]
    assert json.load(open(run_dir / "dev_best.json"))
    ckpt_path = str(run_dir / "models" / "checkpoint_6.pth.tar")
    assert torch.load(ckpt_path, map_location="cpu", weights_only=False)["score"] == {"kind": "cosine", "scale": 20.0, "eps": 1e-8}
    model_flags = ["--model_name_or_path", mdir, "--tokenizer_name_or_path", tok_dir, "--resume", ckpt_path]
    index_path = I.main(I.get_args(model_flags + ["--passages_path", collection, "--index_dir", str(tmp_path / "index"), "--max_length", "24"]))
    index = read_index(index_path)
    assert index.ntotal == 90 and index.normalized is True
    run_out = str(tmp_path / "dev.ce.run.tsv")
    S.main(S.get_args(model_flags + ["--queries_path", queries, "--index_path", index_path, "--max_length", "8", "--top_k", "10",
                                     "--output_path", run_out]))
    lines = open(run_out).read().splitlines()
    assert len(lines) == 12 * 10 and all(abs(float(ln.split("\t")[3])) <= 1.0 + 1e-3 for ln in lines)
    # the distillation term behind the new loss, on the same file with scores
    scored = tmp_path / "train.scored.jsonl"
    rng = np.random.default_rng(3)
    with open(scored, "w") as fh:
        for r in rows:
            s = np.sort(rng.normal(0.0, 3.0, 30))[::-1].round(4).tolist()
            fh.write(json.dumps(dict(r, relT_scores=s[:10], most_hard_scores=s[10:20], semi_hard_scores=s[20:])) + "\n")
    tr2 = T.train(T.set_env(T.get_args(common + ["--run_folder", "ce_kd", "--training_path", str(scored), "--distill_loss", "margin_mse",
                                                 "--distill_alpha", "0.5"])))
    assert tr2.global_step == 6 and tr2.distill == "margin_mse" and float(tr2.last_kd) > 0 and torch.isfinite(tr2.flat_p).all().item()
    log2 = (tmp_path / "ce_kd" / "log" / "train_logs.log").read_text().splitlines()
    assert "kd_loss" in log2[0] and len(log2) == 2
