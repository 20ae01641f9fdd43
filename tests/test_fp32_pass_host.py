"""Host side of the fp32 evaluation pass (encode(fp32=True), csrc/encoder_f32.hip) without a GPU: the argument checks of the new entry points
(small integers stand in for device pointers: every call must be rejected in front of any HIP call), the launch sequence of the pass with
stubbed launches, its refusals, the command-line flags and the restore of ``eval_fp32`` by get_embeddings_from_scratch."""
import numpy as np
import pytest
import torch

from cldrd_amd import _lib, hip_ops as ops
from cldrd_amd.encoder import EncoderConfig, HipEncoder

NEW = ("cldrd_gemm_nt_f32", "cldrd_attention_fwd_f32", "cldrd_attention_cls_fwd_f32")
SIXTEEN_BIT = ("cldrd_gemm_nt16", "cldrd_attention_fwd", "cldrd_attention_cls_fwd")


def test_new_entry_points_reject_inconsistent_arguments():
    try:
        lib = _lib.load()
    except Exception as e:
        pytest.skip(f"libcldrd_hip.so not built: {e}")
    P, nseq, L, H = 64, 4, 32, 2            # P: any non-null, 16-byte aligned "pointer"

    def gemm(A=P, W=P, C=P, M=5, N=128, K=128, lda=None, ldw=None, ldc=None, bias=None, res=None, ldr=0, act=0):
        return "gemm_nt_f32", lib.cldrd_gemm_nt_f32(A, W, C, M, N, K, K if lda is None else lda, K if ldw is None else ldw, N if ldc is None else ldc,
                                                    bias, res, ldr, act, None)

    def attn(qkv=P, mask=None, cu=None, ctx=P, L=L, nseq=nseq):
        return "attention_fwd_f32", lib.cldrd_attention_fwd_f32(qkv, mask, cu, ctx, nseq, L, H, None)

    def cls(qc=P, ldq=H * 64, kv=P, mask=None, cu=None, ctx=P, L=L):
        return "attention_cls_fwd_f32", lib.cldrd_attention_cls_fwd_f32(qc, ldq, kv, mask, cu, ctx, nseq, L, H, None)

    cases = [
        lambda: attn(mask=P, cu=P), lambda: cls(mask=P, cu=P),                       # mask together with cu_rows
        lambda: attn(L=257), lambda: cls(L=257), lambda: attn(L=0),                  # L outside 1 .. 256
        lambda: gemm(K=100), lambda: gemm(K=16), lambda: gemm(N=100),                # K % 32, N % 8
        lambda: gemm(C=None), lambda: attn(ctx=None), lambda: cls(ctx=None),         # null outputs
        lambda: gemm(A=None), lambda: attn(qkv=None), lambda: cls(kv=None), lambda: cls(qc=None),
        lambda: gemm(res=P, ldr=0), lambda: gemm(res=P, ldr=64),                     # a residual without a (sufficient) pitch
        lambda: gemm(M=0), lambda: gemm(lda=64), lambda: gemm(lda=130), lambda: gemm(act=2), lambda: gemm(A=68),
        lambda: attn(nseq=0), lambda: cls(ldq=64), lambda: cls(ldq=130), lambda: cls(qc=72),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"


def test_wrappers_refuse_cpu_tensors():
    a, w, o = torch.zeros(4, 32), torch.zeros(8, 32), torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gemm_nt_f32(a, w, o)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attention_fwd_f32(torch.zeros(8, 384), None, torch.zeros(8, 128), 1, 8, 2)


class _Calls(list):
    def __init__(self):
        super().__init__()
        self.args = []


@pytest.fixture
def stubbed(monkeypatch):
    """Every launch is recorded instead of made, the device check of the argument validators is lifted; reaching refresh_shadows fails the test."""
    try:
        _lib.load()
    except Exception as e:
        pytest.skip(f"libcldrd_hip.so not built: {e}")
    calls = _Calls()

    def chk(t, dtype, name, dim=None):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        if dim is not None and t.dim() != dim:
            raise ValueError(f"{name}: expected {dim} dims, got {t.dim()}")
        if t.stride(-1) != 1:
            raise ValueError(f"{name}: last dim must be contiguous")
        return t

    def no_shadows(self, *a, **k):
        raise AssertionError("the fp32 pass reads flat_p in place: refresh_shadows must not be reached")
    monkeypatch.setattr(ops, "_chk", chk)
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), calls.args.append((name, a))))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(HipEncoder, "refresh_shadows", no_shadows)
    return calls


def cfg_of(arch, layers):
    return EncoderConfig(arch=arch, vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=layers, max_position_embeddings=64,
                         dropout=0.1, attention_dropout=0.1)


M_, L_ = 6, 24
LENS = np.array([24, 3, 10, 17, 5, 8])


def _batch():
    ids = torch.randint(3, 500, (M_, L_))
    mask = (torch.arange(L_)[None, :] < torch.from_numpy(LENS)[:, None]).long()
    return ids, mask


@pytest.mark.parametrize("arch,layers", [("distilbert", 3), ("bert", 2), ("distilbert", 1)])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("typed", [False, True])
def test_fp32_pass_call_sequence(stubbed, arch, layers, packed, typed):
    enc = HipEncoder(cfg_of(arch, layers), seed=1)
    ids, mask = _batch()
    tt = (torch.arange(L_)[None, :] >= 5).long().expand(M_, L_) if typed else None
    cls = enc.encode(ids, mask, lengths=LENS.tolist() if packed else None, token_type_ids=tt, fp32=True)
    assert cls.shape == (M_, 128) and cls.dtype == torch.float32
    seq = list(stubbed)
    assert not set(seq) & set(SIXTEEN_BIT), seq
    assert seq.count("cldrd_gemm_nt_f32") == 4 * (layers - 1) + 5          # QKV, out, FFN1, FFN2 per full layer; K|V, Q, out, FFN1, FFN2 in the last
    assert seq.count("cldrd_attention_fwd_f32") == layers - 1 and seq.count("cldrd_attention_cls_fwd_f32") == 1
    assert seq.count("cldrd_embed_ln_fwd") == 1 and seq.count("cldrd_layernorm_fwd") == 2 * layers
    assert seq[0] == ("cldrd_gather_i64" if packed else "cldrd_embed_ln_fwd") and seq[-1] == "cldrd_layernorm_fwd"
    # the layout is said by cu_rows (argument 2 of the full form, 4 of the CLS form); a padded pass hands the mask instead
    for name, cu_pos, mask_pos in (("cldrd_attention_fwd_f32", 2, 1), ("cldrd_attention_cls_fwd_f32", 4, 3)):
        for n, a in stubbed.args:
            if n == name:
                assert (a[cu_pos] is not None) == packed and (a[mask_pos] is not None) == (not packed), name
    assert ("cldrd_gather_rows" in seq) == packed                        # CLS rows: gathered when packed, a strided view when padded
    # token types reach the embedding kernel on BERT only (argument 4 = type_ids)
    assert [a[4] is not None for n, a in stubbed.args if n == "cldrd_embed_ln_fwd"] == [typed and arch == "bert"]
    # every LayerNorm and the embedding write their fp32 output (or the CLS rows); the GEMM of the padded CLS rows takes the pitch L * d
    pitches = {a[6] for n, a in stubbed.args if n == "cldrd_gemm_nt_f32"}
    assert (L_ * 128 in pitches) == (not packed)


def test_fp32_pass_packed_rows_and_full_last_layer(stubbed):
    enc = HipEncoder(cfg_of("bert", 2), seed=1)
    T = int(LENS.sum())
    pos = torch.cat([torch.arange(n) for n in LENS]).to(torch.int32)
    rows = (torch.randint(3, 500, (T,)), torch.zeros(T, dtype=torch.int32), pos, 32)
    cls = enc.encode(None, None, lengths=LENS.tolist(), packed=rows, fp32=True)
    assert cls.shape == (M_, 128) and "cldrd_gather_i64" not in stubbed and "cldrd_attention_cls_fwd_f32" in stubbed
    assert all(a[7] == 32 for n, a in stubbed.args if n == "cldrd_attention_cls_fwd_f32")          # L = the width the caller gave
    # a tower built without the CLS-only last layer: full layers only, never packed, packed rows refused; a tower without layers pools the embedding
    del stubbed[:]
    enc.cls_only_last = False
    ids, mask = _batch()
    enc.encode(ids, mask, lengths=LENS.tolist(), fp32=True)
    assert stubbed.count("cldrd_attention_fwd_f32") == 2 and "cldrd_attention_cls_fwd_f32" not in stubbed and "cldrd_gather_i64" not in stubbed
    with pytest.raises(ValueError, match="CLS-only"):
        enc.encode(None, None, lengths=LENS.tolist(), packed=rows, fp32=True)
    enc0 = HipEncoder(cfg_of("distilbert", 0), seed=1)
    del stubbed[:]
    assert enc0.encode(ids, mask, lengths=LENS.tolist(), fp32=True).shape == (M_, 128) and list(stubbed) == ["cldrd_embed_ln_fwd"]


@pytest.mark.parametrize("kw", [dict(save=True), dict(train=True), dict(device_seed=True), dict(fp16=True)])
def test_fp32_pass_is_an_evaluation_pass_and_nothing_else(stubbed, kw):
    enc = HipEncoder(cfg_of("distilbert", 2), seed=1)
    ids, mask = _batch()
    with pytest.raises(ValueError, match="evaluation pass"):
        enc.encode(ids, mask, fp32=True, **kw)
    assert not stubbed


def test_dual_encoder_eval_fp32_routes_and_refuses_gradients(stubbed):
    from cldrd_amd.models import NwayDualEncoder
    model = NwayDualEncoder(cfg_of("distilbert", 2), share_weights=False)
    assert model.eval_fp32 is False
    ids, mask = _batch()
    model.eval_fp32 = True
    with pytest.raises(RuntimeError, match="eval_fp32"):
        model.passage_embs({"input_ids": ids, "attention_mask": mask})
    with torch.no_grad():
        model.query_embs({"input_ids": ids, "attention_mask": mask})
        model.passage_embs({"input_ids": ids, "attention_mask": mask, "lengths": LENS.tolist()})
        model.nway_passage_embs({"input_ids": ids.view(2, 3, L_), "attention_mask": mask.view(2, 3, L_)})
    assert not set(stubbed) & set(SIXTEEN_BIT) and stubbed.count("cldrd_attention_cls_fwd_f32") == 3


def test_wrappers_check_dtype_shape_and_layout(stubbed):
    a, w, o = torch.zeros(4, 32), torch.zeros(8, 32), torch.zeros(4, 8)
    ops.gemm_nt_f32(a, w, o, bias=torch.zeros(8), residual=torch.zeros(4, 8), act=1)
    for bad in (lambda: ops.gemm_nt_f32(a.half(), w, o), lambda: ops.gemm_nt_f32(a, w.bfloat16(), o)):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: ops.gemm_nt_f32(a, torch.zeros(8, 16), torch.zeros(4, 8)), lambda: ops.gemm_nt_f32(a, w, o, residual=torch.zeros(4, 16)),
                lambda: ops.gemm_nt_f32(a, w, o, bias=torch.zeros(4)), lambda: ops.gemm_nt_f32(a, w, o, act=3),
                lambda: ops.gemm_nt_f32(a.t().contiguous().t(), w, o)):
        with pytest.raises(ValueError):
            bad()
    qkv, ctx, mask, cu = torch.zeros(16, 384), torch.zeros(16, 128), torch.ones(2, 8, dtype=torch.int64), torch.tensor([0, 8, 16], dtype=torch.int32)
    ops.attention_fwd_f32(qkv, mask, ctx, 2, 8, 2)
    ops.attention_fwd_f32(qkv, None, ctx, 2, 8, 2, cu=cu)
    ops.attention_fwd_f32(qkv[:, :256].contiguous(), None, torch.zeros(2, 128), 2, 8, 2, cu=cu, qc=torch.zeros(2, 8 * 128)[:, :128])
    assert list(stubbed) == ["cldrd_gemm_nt_f32", "cldrd_attention_fwd_f32", "cldrd_attention_fwd_f32", "cldrd_attention_cls_fwd_f32"]
    assert stubbed.args[-1][1][1] == 8 * 128                              # the pitch of the CLS query rows
    for bad in (lambda: ops.attention_fwd_f32(qkv, mask, ctx, 2, 8, 2, cu=cu), lambda: ops.attention_fwd_f32(qkv, None, ctx, 2, 257, 2),
                lambda: ops.attention_fwd_f32(qkv, None, torch.zeros(16, 64), 2, 8, 2), lambda: ops.attention_fwd_f32(qkv, None, ctx, 2, 8, 2, qc=ctx)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.attention_fwd_f32(qkv.half(), None, ctx, 2, 8, 2)


def test_command_lines_parse_fp32_encode(tmp_path):
    from cldrd_amd.retriever import index_text, rerank_top_passages, retrieve_top_passages
    assert index_text.get_args(["--index_dir", str(tmp_path)]).fp32_encode is False
    assert index_text.get_args(["--index_dir", str(tmp_path), "--fp32_encode"]).fp32_encode is True
    assert retrieve_top_passages.get_args([]).fp32_encode is False
    assert retrieve_top_passages.get_args(["--fp32_encode"]).fp32_encode is True
    need = ["--run_path", "r", "--queries_path", "q", "--collection_path", "c", "--model_name_or_path", "m", "--output_path", "o"]
    assert rerank_top_passages.get_args(need).fp32_encode is False
    assert rerank_top_passages.get_args(need + ["--fp32_encode"]).fp32_encode is True


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.eval_fp32 = False
        self.seen = []

    def passage_embs(self, seq):
        self.seen.append(self.eval_fp32)
        raise KeyboardInterrupt          # (never reached by the failing loader below)


def _failing_loader(model, seen):
    seen.append(model.eval_fp32)
    raise OSError("the loader broke")
    yield


def test_get_embeddings_restores_eval_fp32_after_a_loader_exception():
    from cldrd_amd.retriever.retrieval_utils import get_embeddings_from_scratch
    for before in (False, True):
        model, seen = _Model(), []
        model.eval_fp32 = before
        with pytest.raises(OSError):
            get_embeddings_from_scratch(model, _failing_loader(model, seen), use_fp16=False, is_query=False)
        assert seen == [True] and model.eval_fp32 is before
    model, seen = _Model(), []
    with pytest.raises(OSError):
        get_embeddings_from_scratch(model, _failing_loader(model, seen), use_fp16=True, is_query=False)
    assert seen == [False] and model.eval_fp32 is False          # use_fp16=True does what it did
    plain = torch.nn.Linear(1, 1)                                # a model without the attribute is left alone
    with pytest.raises(OSError):
        get_embeddings_from_scratch(plain, _failing_loader(_Model(), []), use_fp16=False, is_query=False)
    assert not hasattr(plain, "eval_fp32")
