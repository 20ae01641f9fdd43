"""The exact fp32 evaluation pass on the GPU (csrc/encoder_f32.hip, HipEncoder.encode(fp32=True)): the two kernels against float64 with
forward-error bounds derived from the arithmetic (never from what the kernels give), their row-independence properties bit for bit, and the pass
against the float64 oracle, HF transformers, the full-size golden and the retrieval surface.

Set CLDRD_FP32_PARITY_OUT to a file name to get the measured ratios e_gpu / e32 appended to it (profiles/fp32_pass_parity.txt is such a record)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops
from cldrd_amd.encoder import EncoderConfig, HipEncoder
from oracle import encoder_ref as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(n):
    """|fl(sum of n products) - exact| <= gamma(n) * sum |products|, any summation order (Higham, Accuracy and Stability, section 3.1)."""
    return n * U / (1.0 - n * U)


def _record(line):
    print(line)
    path = os.environ.get("CLDRD_FP32_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------------------ GEMM
GEMM_M = (1, 37, 130)


@pytest.mark.parametrize("mode", ["plain", "bias", "bias_gelu", "bias_residual"])
@pytest.mark.parametrize("N,K", [(128, 128), (384, 128), (256, 256), (128, 256)])
def test_gemm_nt_f32_against_float64_and_row_independence(N, K, mode):
    g = torch.Generator().manual_seed(1000 * N + K)
    Mx = max(GEMM_M)
    A = torch.randn(Mx, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)          # pre-activations ~ N(0, 1): GELU's whole range
    bias = torch.randn(N, generator=g) if mode != "plain" else None
    res = torch.randn(Mx, N, generator=g) if mode == "bias_residual" else None
    A64, W64 = A.double(), W.double()
    pre = A64 @ W64.t()
    mag = A64.abs() @ W64.abs().t()                            # sum |a w| per element
    if bias is not None:
        pre = pre + bias.double()
        mag = mag + bias.double().abs()
    # bound of the pre-activation / the linear result: gamma_{K+2} (sum|a w| + |bias| + |residual|)
    if mode == "bias_gelu":
        ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        bound = 1.13 * gamma(K + 2) * mag + 8 * U * ref.abs()      # |gelu'| <= 1.13; erff and the products around it: 8 u |y|
    else:
        ref = pre if res is None else pre + res.double()
        bound = gamma(K + 2) * (mag if res is None else mag + res.double().abs())
    Ad, Wd = A.cuda(), W.cuda()
    wide = torch.zeros(Mx, 5 * K, device="cuda")
    wide[:, :K] = Ad
    wide[:, K:] = float("nan")                                # a kernel that read beyond a row of the strided view would show it
    bd, rd = (None if bias is None else bias.cuda()), (None if res is None else res.cuda())
    outs = {}
    for M in GEMM_M:
        for strided in (False, True):
            a = wide[:M, :K] if strided else Ad[:M].contiguous()
            assert a.stride(0) == (5 * K if strided else K)
            out = torch.full((M + 3, N), float("nan"), device="cuda")
            ops.gemm_nt_f32(a, Wd, out, M, bias=bd, residual=None if rd is None else rd[:M], act=1 if mode == "bias_gelu" else 0)
            assert torch.isnan(out[M:]).all()                 # rows >= M are never stored
            got = out[:M].cpu()
            err = (got.double() - ref[:M]).abs()
            ratio = float((err / bound[:M].clamp_min(1e-300)).max())
            print(f"gemm_nt_f32 M={M} N={N} K={K} {mode} strided={strided}: max err / bound = {ratio:.3f}")
            assert bool((err <= bound[:M]).all()), (M, strided, ratio)
            outs[(M, strided)] = got
    for M in GEMM_M:
        assert torch.equal(outs[(M, False)], outs[(M, True)])                      # the pitch changes nothing
        assert torch.equal(outs[(Mx, False)][:M], outs[(M, False)])                # a row does not depend on the rows it shares a launch with


# ------------------------------------------------------------------------------------------------------------------------ attention
H_ = 2
D_ = 64 * H_
ATT_CASES = {256: [1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256], 48: [1, 7, 48]}
_ATT = {}


def _attention_case(L):
    """Inputs, float64 reference and error bound of one case, computed once and shared (never modified)."""
    if L in _ATT:
        return _ATT[L]
    lens = ATT_CASES[L]
    nseq = len(lens)
    g = torch.Generator().manual_seed(77 + L)
    qkv = torch.randn(nseq * L, 3 * D_, generator=g)
    qkv[:, :2 * D_] *= math.sqrt(8.0 / 3.0)          # q, k ~ N(0, 8/3): scores q.k / 8 ~ N(0, (8/3)^2), about +-8 at 3 sigma
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    ref = torch.zeros(nseq * L, D_, dtype=torch.float64)
    bound = torch.zeros(nseq * L, D_, dtype=torch.float64)
    x = qkv.double().view(nseq, L, 3, H_, 64)
    for m, n in enumerate(lens):
        for h in range(H_):
            q, k, v = x[m, :n, 0, h], x[m, :n, 1, h], x[m, :n, 2, h]
            s = q @ k.t() / 8.0
            P = torch.softmax(s, dim=-1)
            out = P @ v
            # The bound, written out.  Scores: |ds_ij| <= gamma_64 sum_k |q_ik k_jk| / 8 (the 1 / 8 is exact); e_i = max_j |ds_ij|.
            # Weights: the kernel forms exp(s_ij - m) for a running maximum m; any m cancels between numerator and normaliser, what stays is
            # the rounding of the subtraction (u R_i, R_i = the score range of the row), expf (4 u) and, per 32-key block, one rescale by
            # exp(m_old - m_new) (again u R_i + 4 u, + u for the product): relative error of a weight eps_i = e_i + (nb + 1) (R_i + 5) u.
            # Sums over the keys (numerator per head dim, normaliser): gamma_{n + nb} each, on top of the perturbed weights.
            # out = N / D: |d out_id| <= 2 (eps_i + gamma_{n + nb}) sum_j P_ij |v_jd| + u |out_id|  (first order; 1 % slack for the rest).
            e = gamma(64) * ((q.abs() @ k.abs().t()) / 8.0).max(dim=1).values
            R = s.max(dim=1).values - s.min(dim=1).values
            nb = (n + 31) // 32
            eps = e + (nb + 1) * (R + 5.0) * U
            b = 1.01 * (2.0 * (eps + gamma(n + nb))[:, None] * (P @ v.abs()) + U * out.abs())
            ref[m * L:m * L + n, 64 * h:64 * h + 64] = out
            bound[m * L:m * L + n, 64 * h:64 * h + 64] = b
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
def test_attention_f32_against_float64_and_layouts(L):
    c = _attention_case(L)
    nseq, lens, real = c["nseq"], c["lens"], c["real"]
    qkv, mask = c["qkv"].cuda(), c["mask"].cuda()
    s = c["qkv"].double().view(nseq, L, 3, H_, 64)
    assert float((s[0, :1, 0] * s[0, :1, 1]).abs().max()) > 0          # (the inputs are not degenerate)
    # padded rows + mask
    ctx = torch.full((nseq * L, D_), float("nan"), device="cuda")
    ops.attention_fwd_f32(qkv, mask, ctx, nseq, L, H_)
    got = ctx.cpu()
    err = (got[real].double() - c["ref"][real]).abs()
    ratio = float((err / c["bound"][real]).max())
    print(f"attention_fwd_f32 L={L}: max err / bound = {ratio:.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= c["bound"][real]).all()), ratio
    # packed rows through cu: the same bits on every real row, nothing stored elsewhere
    rows, cu = _packed(c, L)
    T = rows.numel()
    ctx_p = torch.full((T + 2, D_), float("nan"), device="cuda")
    ops.attention_fwd_f32(qkv[rows.cuda()].contiguous(), None, ctx_p, nseq, L, H_, cu=cu.cuda())
    assert torch.isnan(ctx_p[T:]).all()
    assert torch.equal(ctx_p[:T].cpu(), got[real])
    # the CLS form: one query row per sequence (a strided view of the padded rows: pitch L * 3 d) against K | V of every token
    qc = qkv.view(nseq, L * 3 * D_)[:, :D_]
    kv = qkv[:, D_:].contiguous()
    cls_pad = torch.full((nseq, D_), float("nan"), device="cuda")
    ops.attention_fwd_f32(kv, mask, cls_pad, nseq, L, H_, qc=qc)
    assert torch.equal(cls_pad.cpu(), got.view(nseq, L, D_)[:, 0])
    cls_pk = torch.full((nseq, D_), float("nan"), device="cuda")
    ops.attention_fwd_f32(kv[rows.cuda()].contiguous(), None, cls_pk, nseq, L, H_, cu=cu.cuda(), qc=qc.contiguous())
    assert torch.equal(cls_pk.cpu(), got.view(nseq, L, D_)[:, 0])
    # a sequence's rows do not depend on the other sequences of the launch: two sub-batches, both layouts
    for seqs in ([nseq - 1], [1, nseq - 2]):
        r2, cu2 = _packed(c, L, seqs)
        out2 = torch.empty(r2.numel(), D_, device="cuda")
        ops.attention_fwd_f32(qkv[r2.cuda()].contiguous(), None, out2, len(seqs), L, H_, cu=cu2.cuda())
        assert torch.equal(out2.cpu(), got[r2])
        pad_rows = torch.cat([torch.arange(m * L, (m + 1) * L) for m in seqs]).cuda()
        out3 = torch.empty(len(seqs) * L, D_, device="cuda")
        ops.attention_fwd_f32(qkv[pad_rows].contiguous(), mask[torch.tensor(seqs).cuda()].contiguous(), out3, len(seqs), L, H_)
        keep = torch.cat([torch.arange(i * L, i * L + lens[m]) for i, m in enumerate(seqs)])
        assert torch.equal(out3.cpu()[keep], got[r2])


# ------------------------------------------------------------------------------------------------------------------------ the pass, tiny towers
def tiny_cfg(arch):
    return EncoderConfig(arch=arch, vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=64,
                         dropout=0.0, attention_dropout=0.0)


def ref_cfg(cfg):
    return E.RefConfig(arch=cfg.arch, vocab_size=cfg.vocab_size, dim=cfg.dim, n_heads=cfg.n_heads, hidden_dim=cfg.hidden_dim,
                       n_layers=cfg.n_layers, max_position_embeddings=cfg.max_position_embeddings)


def tower(cfg, seed, std=0.02):
    enc = HipEncoder(cfg, seed=1)
    params = {}
    with torch.no_grad():
        for name, p in enc.named_flat():
            params[name] = syn.init_param(seed, name, tuple(p.shape), std=std)
            p.copy_(params[name])
    return enc.cuda().eval(), params


def oracle_cls(params, cfg, ids, mask, dtype):
    with torch.no_grad():
        return E.encoder_forward({k: v.to(dtype) for k, v in params.items()}, ref_cfg(cfg), ids, mask)[:, 0]


def rel(a, b64):
    return float((a.double() - b64).abs().max() / b64.abs().max())


@pytest.mark.parametrize("arch", ["distilbert", "bert"])
def test_fp32_pass_tiny_towers_against_the_float64_oracle(arch):
    cfg = tiny_cfg(arch)
    enc, params = tower(cfg, 12)
    batch = syn.nway_batch(4680, 4, 8, 16, 48, vocab=512, ragged=True)
    for what, ids, mask in (("passages", batch["nway_passages"]["input_ids"].reshape(32, 48), batch["nway_passages"]["attention_mask"].reshape(32, 48)),
                            ("queries", batch["query"]["input_ids"], batch["query"]["attention_mask"])):
        o64 = oracle_cls(params, cfg, ids, mask, torch.float64)
        e32 = rel(oracle_cls(params, cfg, ids, mask, torch.float32), o64)
        idc, mc = ids.cuda(), mask.cuda()
        with torch.no_grad():
            got = enc.encode(idc, mc, fp32=True)
            got16 = enc.encode(idc, mc, fp16=False)
        e_gpu, e16 = rel(got.cpu(), o64), rel(got16.cpu(), o64)
        _record(f"tiny {arch} {what}: e32 = {e32:.3e}, e_gpu = {e_gpu:.3e}, e_gpu / e32 = {e_gpu / e32:.2f}, 16-bit pass e16 = {e16:.3e} "
                f"(e16 / e_gpu = {e16 / e_gpu:.0f})")
        assert e_gpu <= 32 * e32
        assert 100 * e_gpu <= e16
        # packed (lengths) == padded (mask), and a sequence's vector does not depend on the batch it is encoded in: bit for bit
        lens = mask.sum(1).tolist()
        with torch.no_grad():
            assert torch.equal(enc.encode(idc, mc, lengths=lens, fp32=True), got)
            assert torch.equal(enc.encode(idc[:5] if what == "passages" else idc[:3], mc[:5] if what == "passages" else mc[:3], fp32=True),
                               got[:5] if what == "passages" else got[:3])
            assert torch.equal(enc.encode(idc[:5], mc[:5], lengths=lens[:5], fp32=True)[:3], got[:3])


def test_fp32_pass_towers_without_the_cls_only_last_layer_and_without_layers():
    cfg = tiny_cfg("distilbert")
    enc, params = tower(cfg, 12)
    batch = syn.nway_batch(4680, 4, 8, 16, 48, vocab=512, ragged=True)
    ids, mask = batch["nway_passages"]["input_ids"].reshape(32, 48)[:6].cuda(), batch["nway_passages"]["attention_mask"].reshape(32, 48)[:6].cuda()
    with torch.no_grad():
        a = enc.encode(ids, mask, fp32=True)
        enc.cls_only_last = False
        b = enc.encode(ids, mask, fp32=True)
    assert torch.equal(a, b)                          # the CLS row of the full last layer: the same operations on the same numbers
    cfg0 = copy.copy(cfg)
    cfg0.n_layers = 0
    enc0, p0 = tower(cfg0, 12)
    with torch.no_grad():
        c = enc0.encode(ids, mask, fp32=True)
    o64 = oracle_cls(p0, cfg0, ids.cpu(), mask.cpu(), torch.float64)
    assert rel(c.cpu(), o64) <= 32 * rel(oracle_cls(p0, cfg0, ids.cpu(), mask.cpu(), torch.float32), o64)


# ------------------------------------------------------------------------------------------------------------------------ BERT with token types
def test_cross_encoder_fp32_against_transformers(tmp_path):
    from cldrd_amd.models.cross_encoder import CrossEncoder
    from test_gpu_rerank import _hf_logits, _hf_model, _pairs, _save
    hf = _hf_model("bert", 128, 2, 1, seed=8)
    model = CrossEncoder.from_pretrained(_save(hf, tmp_path, "m")).cuda()
    qc, pc, qr, pr = _pairs(3, 12, 40, 40, 1000, 256, 120)
    ref32, batch = _hf_logits(hf, "bert", qc, pc, qr, pr, 256)
    hf64 = copy.deepcopy(hf).double()
    with torch.no_grad():
        ref64 = torch.cat([hf64(**{k: v[a:a + 16] for k, v in batch.items()}).logits for a in range(0, len(qr), 16)])
    assert ref64.dtype == torch.float64
    scale = float(ref64.abs().max())
    e32 = float((torch.from_numpy(ref32).double() - ref64).abs().max()) / scale
    got = model(batch, fp32=True).cpu()
    sc = model.score_cached(qc, pc, qr, pr, 256, fp32=True).cpu()
    e_fwd, e_sc = float((got.double() - ref64).abs().max()) / scale, float((sc.double() - ref64[:, 0]).abs().max()) / scale
    _record(f"tiny BERT cross-encoder, token types: e32 = {e32:.3e}, forward e_gpu / e32 = {e_fwd / e32:.2f}, score_cached e_gpu / e32 = {e_sc / e32:.2f}")
    assert e_fwd <= 32 * e32 and e_sc <= 32 * e32
    # a pair's score does not depend on how many pairs share the call
    assert torch.equal(model.score_cached(qc, pc, qr[:3], pr[:3], 256, fp32=True).cpu(), sc[:3])
    assert not torch.equal(model.score_cached(qc, pc, qr, pr, 256).cpu(), sc)          # (the 16-bit pass is another function)


# ------------------------------------------------------------------------------------------------------------------------ full size, once
def test_fp32_pass_full_size_distilbert_against_oracle_and_golden():
    from test_oracle_encoder import load_case
    path = os.path.join(conftest.GOLDEN, "full_distilbert_cfg1.npz")
    if not os.path.exists(path):
        pytest.skip("full-size golden not generated")
    g, rcfg, qp, pp, batch = load_case("full_distilbert_cfg1.npz")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    cfg = EncoderConfig(arch="distilbert", n_layers=rcfg.n_layers, dropout=0.0, attention_dropout=0.0)
    Lp = int(g["Lp"])
    p_ids = batch["nway_passages"]["input_ids"].reshape(-1, Lp)[:8]
    p_mask = batch["nway_passages"]["attention_mask"].reshape(-1, Lp)[:8]
    gold = {"queries": torch.from_numpy(np.asarray(g["q_cls"])).reshape(-1, cfg.dim)[:4],
            "passages": torch.from_numpy(np.asarray(g["p_cls"])).reshape(-1, cfg.dim)[:8]}
    for what, params, ids, mask in (("queries", qp, batch["query"]["input_ids"][:4], batch["query"]["attention_mask"][:4]),
                                    ("passages", pp, p_ids, p_mask)):
        enc = HipEncoder(cfg, seed=1)
        with torch.no_grad():
            for name, p in enc.named_flat():
                p.copy_(params[name])
        enc = enc.cuda().eval()
        with torch.no_grad():
            o64 = E.encoder_forward({k: v.double() for k, v in params.items()}, rcfg, ids, mask)[:, 0]
            o32 = E.encoder_forward(params, rcfg, ids, mask)[:, 0]
            got = enc.encode(ids.cuda(), mask.cuda(), fp32=True).cpu()
        e32, e_gpu = rel(o32, o64), rel(got, o64)
        e_gold = float((got.double() - gold[what].double()).abs().max() / o64.abs().max())
        _record(f"full-size DistilBERT cfg1 {what}: e32 = {e32:.3e}, e_gpu / e32 = {e_gpu / e32:.2f}, against the golden's rows: "
                f"e / e32 = {e_gold / e32:.2f}")
        assert e_gpu <= 32 * e32
        assert e_gold <= (32 + 1) * e32
        del enc


# ------------------------------------------------------------------------------------------------------------------------ retrieval surface
def _tiny_pair():
    from cldrd_amd.models import NwayDualEncoder
    model = NwayDualEncoder(tiny_cfg("distilbert"), share_weights=False)
    params = {}
    with torch.no_grad():
        for seed, key, t in ((11, "q", model.query_encoder), (12, "p", model.passage_encoder)):
            params[key] = {}
            for name, p in t.named_flat():
                params[key][name] = syn.init_param(seed, name, tuple(p.shape), std=0.02)
                p.copy_(params[key][name])
    return model.cuda().eval(), params


def test_get_embeddings_from_scratch_honours_use_fp16():
    from cldrd_amd.dataset.sequence_dataset import SyntheticSequenceDataset
    from cldrd_amd.retriever.retrieval_utils import get_embeddings_from_scratch
    model, _ = _tiny_pair()
    ds = SyntheticSequenceDataset(64, 48, vocab=512, batch_size=24)
    h0, ids0 = get_embeddings_from_scratch(model, ds.loader(), use_fp16=True, is_query=False)
    assert model.eval_fp32 is False
    f, ids1 = get_embeddings_from_scratch(model, ds.loader(), use_fp16=False, is_query=False)
    assert model.eval_fp32 is False and ids0 == ids1 == list(range(64))
    h1, _ = get_embeddings_from_scratch(model, ds.loader(), use_fp16=True, is_query=False)
    assert np.array_equal(h0, h1)                      # the 16-bit path is untouched
    assert f.shape == h0.shape == (64, 128) and not np.array_equal(f, h0)
    with torch.no_grad():
        direct = torch.cat([model.passage_encoder.encode(b["seq"]["input_ids"].cuda(), b["seq"]["attention_mask"].cuda(), fp32=True) for b in ds.loader()])
    assert torch.equal(torch.from_numpy(f), direct.cpu())
    model.eval_fp32 = True                             # ... and it is left as it was found
    f2, _ = get_embeddings_from_scratch(model, ds.loader(), use_fp16=False, is_query=False)
    assert model.eval_fp32 is True and np.array_equal(f2, f)
    with pytest.raises(RuntimeError, match="eval_fp32"):
        model.passage_embs({k: v.cuda() for k, v in ds[0]["seq"].items()})              # gradients enabled: there is no fp32 tape


def test_fp32_encode_to_exact_search_gives_the_float64_ids():
    from cldrd_amd.retriever.retrieval_utils import FlatIPIndex
    model, params = _tiny_pair()
    cfg = tiny_cfg("distilbert")
    batch = syn.nway_batch(4680, 16, 32, 16, 48, vocab=512, ragged=True)
    q_ids, q_mask = batch["query"]["input_ids"], batch["query"]["attention_mask"]
    p_ids, p_mask = batch["nway_passages"]["input_ids"].reshape(512, 48), batch["nway_passages"]["attention_mask"].reshape(512, 48)
    model.eval_fp32 = True
    with torch.no_grad():
        q = model.query_embs({"input_ids": q_ids.cuda(), "attention_mask": q_mask.cuda()}).cpu().numpy()
        p = model.passage_embs({"input_ids": p_ids.cuda(), "attention_mask": p_mask.cuda(), "lengths": p_mask.sum(1).tolist()}).cpu().numpy()
    index = FlatIPIndex(128)
    index.add_with_ids(p, np.arange(512))
    index.to_gpu(0)
    _, I = index.search(q, 10)
    S = (oracle_cls(params["q"], cfg, q_ids, q_mask, torch.float64) @ oracle_cls(params["p"], cfg, p_ids, p_mask, torch.float64).t()).numpy()
    order = np.lexsort((np.broadcast_to(np.arange(512), S.shape), -S), axis=1)       # score descending, ties: row ascending (the project's rule)
    srt = np.take_along_axis(S, order, 1)
    comparable = (srt[:, :10] - srt[:, 1:11]) >= 1e-4 * np.abs(S).max()
    left_out = 1.0 - comparable.mean()
    print(f"fp32 encode -> FlatIPIndex: {int(comparable.sum())} of 160 rank positions comparable ({100 * left_out:.1f} % left out), "
          f"{int((I == order[:, :10])[comparable].sum())} identical; all positions identical: {int((I == order[:, :10]).sum())}")
    assert left_out <= 0.10
    assert np.array_equal(I[comparable], order[:, :10][comparable])
