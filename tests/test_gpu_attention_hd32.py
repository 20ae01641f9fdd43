"""The head-dim-32 attention kernels on the MI355X (csrc/attention_hd32.hip and the _hd32 pair of csrc/encoder_f32.hip; run with -m gpu): the 16-bit
forward and its CLS form against float64 at the bars test_gpu_kernels.py sets for head dim 64 (the rounding model is the same: P goes through 16 bits
before P.V, ctx is stored in 16 bits), the layout and item-independence contracts bit for bit, and the fp32 pair against float64 with the forward
error bound of test_gpu_fp32_pass.py written out for 32 head dims."""
import math

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 32
BF16, F16 = torch.bfloat16, torch.float16


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((syn.normal(seed, int(np.prod(shape))) * scale).astype(np.float32).reshape(shape))


def close(got, ref, rtol, atol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = int((err > tol).sum())
    print(f"{what}: max err {err.max().item():.4e}, max err / tol {float((err / tol).max()):.3f}")
    assert bad == 0, f"{what}: {bad}/{err.numel()} off, max err {err.max().item():.4e} (ref max {ref.abs().max().item():.3e})"


def attn_ref(qkv, mask, nseq, L, H):
    """float64 softmax(Q K^T / sqrt(32) + key mask) V of 16-bit-rounded inputs."""
    x = qkv.double().view(nseq, L, 3, H, HD)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(2, 3) / math.sqrt(HD)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, -1e30)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(nseq * L, H * HD)


def _mask(seed, nseq, L):
    lens = np.clip(syn.msmarco_lengths(seed, nseq, L), 2, L)
    lens[0] = L
    return torch.from_numpy((np.arange(L)[None, :] < lens[:, None]).astype(np.int64))


# unit normal q, k, v: scores q.k / sqrt(32) are again about N(0, 1)
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("nseq,L,H,masked", [(3, 32, 2, False), (2, 30, 2, True), (5, 8, 2, True), (4, 128, 2, True), (2, 100, 4, True),
                                              (2, 64, 12, False), (2, 256, 2, True), (1, 160, 2, True), (2, 129, 2, False), (1, 224, 2, True)])
def test_attention_fwd_hd32_against_float64(nseq, L, H, masked, dt):
    d, T = H * HD, nseq * L
    qkv = rnd(10, (T, 3 * d), 1.0).to(dt)
    mask = _mask(11, nseq, L) if masked else None
    ref = attn_ref(qkv, mask, nseq, L, H)
    ctx = torch.full((T, d), float("nan"), dtype=dt, device=DEV)
    ops.attention_fwd(qkv.to(DEV), None if mask is None else mask.to(DEV), ctx, None, nseq, L, H, head_dim=32)
    # bf16: test_attention_fwd_bwd's bar.  fp16: 8 times tighter (11 significant bits against 8: test_gpu_kernels.py's rule)
    k = 8.0 if dt == F16 else 1.0
    close(ctx, ref, 1 / 64 / k, 2e-2 / k, f"attention_fwd_hd32 {dt} nseq={nseq} L={L} H={H}")


def _every_length(W, lens, dt, H=2, seed=5):
    """One padded and one packed launch over sequences of the given lengths at width W -> (padded ctx, packed ctx with guard rows, row index, mask)."""
    nseq, d = len(lens), H * HD
    g = torch.Generator(device=DEV).manual_seed(seed * 1000 + W)
    lens_t = torch.tensor(lens, device=DEV, dtype=torch.int64)
    cu = torch.zeros(nseq + 1, dtype=torch.int32, device=DEV)
    cu[1:] = torch.cumsum(lens_t, 0).to(torch.int32)
    Tp = int(cu[-1])
    mask = (torch.arange(W, device=DEV)[None, :] < lens_t[:, None]).to(torch.int64).contiguous()
    tok = torch.nonzero(mask.reshape(-1)).reshape(-1)
    qkv = torch.randn(nseq * W, 3 * d, device=DEV, generator=g).to(dt)             # REAL values in the padding rows (masked, not zero)
    pad = torch.full((nseq * W, d), float("nan"), dtype=dt, device=DEV)
    ops.attention_fwd(qkv, mask, pad, None, nseq, W, H, head_dim=32)
    G = 3                                                                           # NaN guard rows in front of and behind the packed output
    out = torch.full((Tp + 2 * G, d), float("nan"), dtype=dt, device=DEV)
    ops.attention_fwd(qkv[tok].contiguous(), None, out[G:G + Tp], None, nseq, W, H, cu=cu, head_dim=32)
    torch.cuda.synchronize()
    return pad, out, G, Tp, tok, mask, lens_t


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("W,lens", [(256, None), (48, [1, 7, 31, 32, 33, 48])])
def test_attention_fwd_hd32_packed_rows_every_length(W, lens, dt):
    """A sequence of every length 1 .. 256 at width 256 (every count of live / skipped 32-key blocks, every position of the last key in a block), and
    the lengths around a block edge at width 48: packed rows give the padded launch's bits on every real row and write nothing else.  The padding
    rows of the PADDED launch: the head-dim-64 forward's contract is that they are written like any other row (a masked position still has a query:
    finite values, never NaN; zeros are what the BACKWARD leaves in dqkv there) - the same is asserted here, against the head-dim-64 kernel itself."""
    if lens is None:
        lens = (torch.randperm(W, generator=torch.Generator().manual_seed(W)) + 1).tolist()
    pad, out, G, Tp, tok, mask, lens_t = _every_length(W, lens, dt)
    assert torch.isnan(out[:G].float()).all() and torch.isnan(out[G + Tp:].float()).all(), "the packed launch wrote outside its rows"
    same = (out[G:G + Tp] == pad[tok]).all(1)
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=DEV), lens_t)
    bad = sorted(set(lens_t[seq_of[~same]].tolist()))
    assert not bad, f"packed rows differ from the padded layout for sequences of {bad[:20]} tokens"
    padding = ~mask.reshape(-1).bool()
    assert bool(torch.isfinite(pad.float()).all())
    # the head-dim-64 family on a batch of the same shape: its padding rows are finite values too
    nseq = len(lens)
    q64 = torch.randn(nseq * W, 3 * 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(dt)
    c64 = torch.full((nseq * W, 128), float("nan"), dtype=dt, device=DEV)
    ops.attention_fwd(q64, mask, c64, None, nseq, W, 2, full_family=dt == F16)
    assert bool(torch.isfinite(c64.float()[padding]).all()) == bool(torch.isfinite(pad.float()[padding]).all())


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_attention_fwd_hd32_items_do_not_depend_on_their_launch(dt):
    """The rows of six sequences (1, 32, 33, 128, 129, 256 tokens), bit for bit, from a launch of the six, from a launch of 400 MS MARCO-shaped
    sequences that holds them in another order, and from a seq_list launch that names only them - all at tile 256, H = 12.  At a SMALLER tile
    (a list of the four short ones at tile 128) the result agrees within test_attention_sequence_lists_..._short_kernels' tolerance."""
    H, L = 12, 256
    d = H * HD
    chosen = [1, 32, 33, 128, 129, 256]
    g = torch.Generator(device=DEV).manual_seed(99)
    x6 = [torch.randn(n, 3 * d, device=DEV, generator=g).to(dt) for n in chosen]

    def launch(seqs, seq_list=None, tile=0):
        lens = torch.tensor([s.shape[0] for s in seqs], dtype=torch.int64, device=DEV)
        cu = torch.zeros(len(seqs) + 1, dtype=torch.int32, device=DEV)
        cu[1:] = torch.cumsum(lens, 0).to(torch.int32)
        ctx = torch.full((int(cu[-1]), d), float("nan"), dtype=dt, device=DEV)
        ops.attention_fwd(torch.cat(seqs).contiguous(), None, ctx, None, len(seqs), L, H, cu=cu, seq_list=seq_list, tile=tile, head_dim=32)
        torch.cuda.synchronize()
        return ctx, cu

    own, _ = launch(x6)
    assert not torch.isnan(own.float()).any()
    big_lens = np.clip(syn.msmarco_lengths(7, 400, L), 1, L)
    others = [torch.randn(int(n), 3 * d, device=DEV, generator=g).to(dt) for n in big_lens]
    where = [390, 17, 201, 3, 350, 120]                     # positions of the six inside the big batch: another order
    for pos, s in zip(where, x6):
        others[pos] = s
    big, cu_big = launch(others)
    picked = torch.cat([big[int(cu_big[p]):int(cu_big[p + 1])] for p in where])
    assert torch.equal(picked, own), "a sequence's context depends on the other sequences of its launch"
    sl = torch.tensor(where, dtype=torch.int32, device=DEV)
    listed, _ = launch(others, seq_list=sl, tile=L)
    rows = torch.cat([torch.arange(int(cu_big[p]), int(cu_big[p + 1]), device=DEV) for p in where])
    assert torch.equal(listed[rows], own), "a seq_list launch differs from the launch of the whole batch"
    keep = torch.ones(listed.shape[0], dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert torch.isnan(listed[keep].float()).all(), "a seq_list launch wrote rows of sequences it does not name"
    short = [p for p, n in zip(where, chosen) if n <= 128]
    lo, _ = launch(others, seq_list=torch.tensor(short, dtype=torch.int32, device=DEV), tile=128)
    rows_s = torch.cat([torch.arange(int(cu_big[p]), int(cu_big[p + 1]), device=DEV) for p in short])
    a, b = lo[rows_s].float(), big[rows_s].float()
    tol = 2.0 ** (-9 if dt == F16 else -6)
    assert bool(((a - b).abs() <= tol * b.abs() + tol * b.abs().max() * 0.25).all()), float((a - b).abs().max())


@pytest.mark.parametrize("nseq,L,H", [(3, 40, 2), (2, 200, 2), (1, 256, 4), (4, 128, 12)])
def test_attention_hd32_fp16_copy_and_cls_form(nseq, L, H):
    d, T = H * HD, nseq * L
    qkv = rnd(150, (T, 3 * d), 1.0).to(BF16).to(DEV)
    mask = _mask(151, nseq, L).to(DEV)
    ref = attn_ref(qkv.cpu(), mask.cpu(), nseq, L, H)
    nan = lambda rows, dt: torch.full((rows, d), float("nan"), dtype=dt, device=DEV)
    plain, ctx, c16, only = nan(T, BF16), nan(T, BF16), nan(T, F16), nan(T, F16)
    ops.attention_fwd(qkv, mask, plain, None, nseq, L, H, head_dim=32)
    ops.attention_fwd(qkv, mask, ctx, None, nseq, L, H, ctx16=c16, head_dim=32)
    ops.attention_fwd(qkv, mask, None, None, nseq, L, H, ctx16=only, head_dim=32)
    assert torch.equal(ctx, plain) and torch.equal(only, c16)
    close(c16, ref, 1 / 64, 2e-2, "fp16 context copy")                       # P still goes through bf16
    assert (c16.float() - ctx.float()).abs().max().item() <= 2.0 ** -7 * ctx.float().abs().max().item()
    with pytest.raises(ValueError):
        ops.attention_fwd(qkv.to(F16), mask, nan(T, F16), None, nseq, L, H, ctx16=c16, head_dim=32)
    # CLS form against row 0 of the float64 reference: bf16 context, its fp16 copy, the copy alone, the fp16 pass; packed K | V rows
    kv = qkv[:, d:].contiguous()
    qc = qkv.view(nseq, L, 3 * d)[:, 0, :d].contiguous()
    ref0 = ref.view(nseq, L, d)[:, 0]
    cb, ch, ch2 = nan(nseq, BF16), nan(nseq, F16), nan(nseq, F16)
    ops.attention_cls_fwd(qc, kv, mask, cb, None, nseq, L, H, ctx16=ch, head_dim=32)
    ops.attention_cls_fwd(qc, kv, mask, None, None, nseq, L, H, ctx16=ch2, head_dim=32)
    close(cb, ref0, 1 / 64, 2e-2, "bf16 CLS context")
    close(ch, ref0, 1 / 256, 5e-3, "fp16 CLS context copy")
    assert torch.equal(ch, ch2)
    lens = mask.sum(1)
    cu = torch.zeros(nseq + 1, dtype=torch.int32, device=DEV)
    cu[1:] = torch.cumsum(lens, 0).to(torch.int32)
    tok = torch.nonzero(mask.reshape(-1)).reshape(-1)
    cp = nan(nseq, BF16)
    ops.attention_cls_fwd(qc, kv[tok].contiguous(), None, cp, None, nseq, L, H, cu=cu, head_dim=32)
    assert torch.equal(cp, cb), "CLS form: packed K | V rows differ from the padded layout"
    q16 = qkv.to(F16)
    ref16 = attn_ref(q16.cpu(), mask.cpu(), nseq, L, H).view(nseq, L, d)[:, 0]
    cf = nan(nseq, F16)
    ops.attention_cls_fwd(q16.view(nseq, L, 3 * d)[:, 0, :d].contiguous(), q16[:, d:].contiguous(), mask, cf, None, nseq, L, H, head_dim=32)
    close(cf, ref16, 1 / 256, 5e-3, "fp16 CLS context")


# ------------------------------------------------------------------------------------------------------------------------ fp32
U = 2.0 ** -24          # unit roundoff of fp32
H_ = 2
D_ = HD * H_
ATT_CASES = {256: [1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256], 48: [1, 7, 48]}          # test_gpu_fp32_pass.py's cases
_ATT = {}


def gamma(n):
    return n * U / (1.0 - n * U)


def _attention_case(L):
    """Inputs, float64 reference and error bound of one case, computed once and shared (never modified)."""
    if L in _ATT:
        return _ATT[L]
    lens = ATT_CASES[L]
    nseq = len(lens)
    g = torch.Generator().manual_seed(77 + L)
    qkv = torch.randn(nseq * L, 3 * D_, generator=g)
    qkv[:, :2 * D_] *= math.sqrt(8.0 / 3.0)          # q, k ~ N(0, 8/3): scores q.k / sqrt(32) ~ N(0, (8/3)^2), about +-8 at 3 sigma
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    ref = torch.zeros(nseq * L, D_, dtype=torch.float64)
    bound = torch.zeros(nseq * L, D_, dtype=torch.float64)
    x = qkv.double().view(nseq, L, 3, H_, HD)
    for m, n in enumerate(lens):
        for h in range(H_):
            q, k, v = x[m, :n, 0, h], x[m, :n, 1, h], x[m, :n, 2, h]
            s = q @ k.t() / math.sqrt(HD)
            P = torch.softmax(s, dim=-1)
            out = P @ v
            # test_gpu_fp32_pass.py's bound with 32 head dims, and one term more.  Scores: the chain of 32 products gives
            # |ds_ij| <= gamma_32 sum_k |q_ik k_jk| / sqrt(32).  At head dim 64 the factor 1 / 8 is exact; here the kernel multiplies the finished
            # chain by c = fl(1 / sqrt(32)), |c - 1 / sqrt(32)| <= u / sqrt(32), and rounds the product: two relative errors of u on the score,
            # 2 u |s_ij|.  So e_i = max_j gamma_32 sum_k |q_ik k_jk| / sqrt(32) + 2 u max_j |s_ij|.
            # Weights: the kernel forms exp(s_ij - m) for a running maximum m; any m cancels between numerator and normaliser, what stays is
            # the rounding of the subtraction (u R_i, R_i = the score range of the row), expf (4 u) and, per 32-key block, one rescale by
            # exp(m_old - m_new) (again u R_i + 4 u, + u for the product): relative error of a weight eps_i = e_i + (nb + 1) (R_i + 5) u.
            # Sums over the keys (numerator per head dim, normaliser): gamma_{n + nb} each, on top of the perturbed weights.
            # out = N / D: |d out_id| <= 2 (eps_i + gamma_{n + nb}) sum_j P_ij |v_jd| + u |out_id|  (first order; 1 % slack for the rest).
            e = gamma(HD) * ((q.abs() @ k.abs().t()) / math.sqrt(HD)).max(dim=1).values + 2.0 * U * s.abs().max(dim=1).values
            R = s.max(dim=1).values - s.min(dim=1).values
            nb = (n + 31) // 32
            eps = e + (nb + 1) * (R + 5.0) * U
            b = 1.01 * (2.0 * (eps + gamma(n + nb))[:, None] * (P @ v.abs()) + U * out.abs())
            ref[m * L:m * L + n, HD * h:HD * h + HD] = out
            bound[m * L:m * L + n, HD * h:HD * h + HD] = b
    real = mask.view(-1).bool()
    _ATT[L] = dict(lens=lens, nseq=nseq, qkv=qkv, mask=mask, ref=ref, bound=bound, real=real)
    return _ATT[L]


def _packed(case, L, seqs=None):
    lens = case["lens"]
    seqs = range(case["nseq"]) if seqs is None else seqs
    rows = torch.cat([torch.arange(m * L, m * L + lens[m]) for m in seqs])
    cu = torch.tensor(np.concatenate([[0], np.cumsum([lens[m] for m in seqs])]), dtype=torch.int32)
    return rows, cu


@pytest.mark.parametrize("L", [256, 48])
def test_attention_f32_hd32_against_float64_and_layouts(L):
    c = _attention_case(L)
    nseq, lens, real = c["nseq"], c["lens"], c["real"]
    qkv, mask = c["qkv"].cuda(), c["mask"].cuda()
    f32 = lambda *a, **k: ops.attention_fwd_f32(*a, head_dim=32, **k)
    ctx = torch.full((nseq * L, D_), float("nan"), device="cuda")
    f32(qkv, mask, ctx, nseq, L, H_)
    got = ctx.cpu()
    err = (got[real].double() - c["ref"][real]).abs()
    ratio = float((err / c["bound"][real]).max())
    print(f"attention_fwd_f32_hd32 L={L}: max err / bound = {ratio:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= c["bound"][real]).all()), ratio
    # packed rows through cu: the same bits on every real row, nothing stored elsewhere
    rows, cu = _packed(c, L)
    T = rows.numel()
    ctx_p = torch.full((T + 2, D_), float("nan"), device="cuda")
    f32(qkv[rows.cuda()].contiguous(), None, ctx_p, nseq, L, H_, cu=cu.cuda())
    assert torch.isnan(ctx_p[T:]).all()
    assert torch.equal(ctx_p[:T].cpu(), got[real])
    # the CLS form: one query row per sequence (a strided view of the padded rows: pitch L * 3 d) against K | V of every token: row 0 of the
    # full form bit for bit, and the pitch of qc changes nothing
    qc = qkv.view(nseq, L * 3 * D_)[:, :D_]
    assert qc.stride(0) == L * 3 * D_
    kv = qkv[:, D_:].contiguous()
    cls_pad = torch.full((nseq, D_), float("nan"), device="cuda")
    f32(kv, mask, cls_pad, nseq, L, H_, qc=qc)
    assert torch.equal(cls_pad.cpu(), got.view(nseq, L, D_)[:, 0])
    cls_pk = torch.full((nseq, D_), float("nan"), device="cuda")
    f32(kv[rows.cuda()].contiguous(), None, cls_pk, nseq, L, H_, cu=cu.cuda(), qc=qc.contiguous())
    assert torch.equal(cls_pk.cpu(), got.view(nseq, L, D_)[:, 0])
    # a sequence's rows do not depend on the other sequences of the launch: two sub-batches, both layouts
    for seqs in ([nseq - 1], [1, nseq - 2]):
        r2, cu2 = _packed(c, L, seqs)
        out2 = torch.empty(r2.numel(), D_, device="cuda")
        f32(qkv[r2.cuda()].contiguous(), None, out2, len(seqs), L, H_, cu=cu2.cuda())
        assert torch.equal(out2.cpu(), got[r2])
        pad_rows = torch.cat([torch.arange(m * L, (m + 1) * L) for m in seqs]).cuda()
        out3 = torch.empty(len(seqs) * L, D_, device="cuda")
        f32(qkv[pad_rows].contiguous(), mask[torch.tensor(seqs).cuda()].contiguous(), out3, len(seqs), L, H_)
        keep = torch.cat([torch.arange(i * L, i * L + lens[m]) for i, m in enumerate(seqs)])
        assert torch.equal(out3.cpu()[keep], got[r2])
