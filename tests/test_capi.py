"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/cldrd_hip.h declares; the Python binding table covers the same set; the product has no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cldrd_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cldrd_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from cldrd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cldrd_hip.h but not exported"


def test_binding_table_matches_header():
    from cldrd_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_format_constants_match_the_header_enum():
    """hip_ops names the 16-bit format codes it passes as `fmt`: the names and values are enum cldrd_fmt16's, every member of it."""
    from cldrd_amd import hip_ops as ops
    body = re.search(r"enum\s+cldrd_fmt16\s*\{(.*?)\}", open(HEADER).read(), flags=re.S).group(1)
    enum = {name: int(value) for name, value in re.findall(r"\bCLDRD_(FMT_[A-Z0-9_]+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))}
    assert enum == {"FMT_BF16": 0, "FMT_F16": 1, "FMT_F16_C_BF16": 3, "FMT_F16_TAPE": 5}
    assert {name: getattr(ops, name) for name in enum} == enum
    assert sorted(n for n in vars(ops) if n.startswith("FMT_")) == sorted(enum)


def test_product_library_reads_no_environment_variable():
    """An inherited environment variable must not be able to change what a run computes (round-3 review): the shipped library imports no
    getenv, contains no CLDRD_* switch name - in particular none of the timing-only ablation modes (CLDRD_GEMM_ABLATE, CLDRD_SCAN_ABLATE:
    wrong results by design) - and its sources call getenv nowhere and carry no CLDRD_DEV_* build switch."""
    import subprocess
    from cldrd_amd import _lib
    path = os.path.join(ROOT, "cl-drd_amd", "libcldrd_hip.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    blob = open(path, "rb").read()
    for needle in (b"CLDRD_GEMM_ABLATE", b"CLDRD_SCAN_ABLATE", b"CLDRD_"):
        assert needle not in blob, f"{needle.decode()} found in the product library"
    und = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True).stdout
    assert "getenv" not in und, "the product library imports getenv"
    csrc = os.path.join(ROOT, "cl-drd_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, f)).read()
            assert "getenv(" not in text, f"{f}: getenv in the kernel library's sources"
            assert "CLDRD_DEV_" not in text, f"{f}: development-build switch in the kernel library's sources"


def test_set_tuning_rejects_unknown_keys():
    from cldrd_amd import hip_ops as ops
    from cldrd_amd._lib import CldrdError
    ops.set_tuning("gemm_splitk", 0)
    with pytest.raises(CldrdError):
        ops.set_tuning("no_such_knob", 1)


def test_version_and_error_string_without_gpu():
    from cldrd_amd import _lib
    lib = _lib.load()
    assert lib.cldrd_version() >= 100
    assert isinstance(lib.cldrd_last_error(), bytes)


def test_attention_entry_points_reject_inconsistent_layouts():
    """The layout rule of include/cldrd_hip.h (mask / cu_rows / seq_list, n_list, Ltile) and the other argument checks of the four attention entry
    points, without a GPU: every call below is rejected by a check in front of any HIP call, so small integers stand in for the device pointers.
    No call here may pass the checks - a fake pointer must never reach a launch."""
    from cldrd_amd import _lib
    lib = _lib.load()
    P, nseq, L, H = 64, 4, 32, 2            # P: any non-null "pointer"

    def fwd(mask=None, cu=None, sl=None, n_list=0, Ltile=0, ctx=P, lse=P, L=L, fmt=0, bits=None, ctx16=None):
        return "attention_fwd", lib.cldrd_attention_fwd(P, mask, cu, sl, n_list, Ltile, ctx, lse, nseq, L, H, 0.1, 7, fmt, bits, ctx16, None)

    def bwd(mask=None, cu=None, sl=None, n_list=0, Ltile=0, lse=P, L=L, fmt=0):
        return "attention_bwd", lib.cldrd_attention_bwd(P, mask, cu, sl, n_list, Ltile, P, P, lse, P, nseq, L, H, 0.1, 7, fmt, None, None)

    def cls_fwd(mask=None, cu=None, ctx=P, probs=P, L=L, fmt=0, ctx16=None):
        return "attention_cls_fwd", lib.cldrd_attention_cls_fwd(P, P, mask, cu, ctx, probs, nseq, L, H, 0.1, 7, fmt, ctx16, None)

    def cls_bwd(cu=None, L=L):
        return "attention_cls_bwd", lib.cldrd_attention_cls_bwd(P, P, cu, P, P, P, P, nseq, L, H, 0.1, 7, 0, None)

    cases = [
        lambda: fwd(mask=P, cu=P), lambda: bwd(mask=P, cu=P), lambda: cls_fwd(mask=P, cu=P),              # mask together with cu_rows
        lambda: fwd(sl=P, n_list=2, Ltile=L), lambda: bwd(sl=P, n_list=2, Ltile=L),                        # seq_list without cu_rows
        lambda: fwd(cu=P, sl=P, n_list=0, Ltile=L), lambda: bwd(cu=P, sl=P, n_list=0, Ltile=L),            # n_list = 0
        lambda: fwd(cu=P, sl=P, n_list=nseq + 1, Ltile=L), lambda: bwd(cu=P, sl=P, n_list=nseq + 1, Ltile=L),
        lambda: fwd(cu=P, sl=P, n_list=2, Ltile=L + 1), lambda: bwd(cu=P, sl=P, n_list=2, Ltile=L + 1),
        lambda: fwd(L=257), lambda: bwd(L=257), lambda: cls_fwd(L=257), lambda: cls_bwd(L=257), lambda: cls_bwd(cu=P, L=257),
        lambda: fwd(ctx=None, ctx16=None),                                                                 # no output
        lambda: fwd(fmt=1, ctx16=P), lambda: cls_fwd(fmt=1, ctx16=P),                                      # the fp16 pass writes ctx only
        lambda: fwd(fmt=2),
        lambda: bwd(lse=None),
        lambda: cls_fwd(probs=None),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"


def test_merged_entry_points_reject_inconsistent_arguments():
    """The row-mode rule of the search (P32 / P16 / qmu) and the int8 chain's own rules, the token-type rule of the embedding forward, the gradient-stream rule of the two
    LayerNorm backwards (enum cldrd_stream_fmt), the fp16 shadow range of the optimizer step and the row rule of the CLS scatter
    (include/cldrd_hip.h), without a GPU: as above, every call is rejected in front of any HIP call and none may pass the checks."""
    from cldrd_amd import _lib
    lib = _lib.load()
    P = 64                                  # any non-null "pointer"
    BF16, F32, F16 = 0, 1, 2                # enum cldrd_stream_fmt

    def search(P16=P, P32=None, qmu=None):
        return "flatip_search", lib.cldrd_flatip_search(P, P, P, P, P16, P32, qmu, 1000, 128, 4, 10, 128, P, P, P, 1024, P, P, 1024, P, P, P, P, P, 0, None)

    def search8(qd=P, sq=P, scale=P, d=128, qtile=128, exhaustive=0):
        return "flatip_search_i8", lib.cldrd_flatip_search_i8(P, qd, sq, P, P, P, scale, P, 1000, d, 4, 10, qtile, P, P, P, 1024, P, P, 1024, P, P, P, P, P,
                                                              exhaustive, None)

    def rescore(P16=P, P32=None, qmu=None):
        return "topk_rescore", lib.cldrd_topk_rescore(P, P32, P16, qmu, 128, P, P, P, 4, 1024, None)

    def embed_fwd(table=P, type_ids=P, type_vocab=2):
        return "embed_ln_fwd", lib.cldrd_embed_ln_fwd(P, P, P, table, type_ids, type_vocab, P, P, P, P, P, 16, 8, 128, 300, 1e-12, 0.0, 7, None, 0, None, None)

    def ln_bwd(x_f32=1, fmt=BF16, dx_dropped=P, branch=None):
        return "layernorm_bwd", lib.cldrd_layernorm_bwd(P, P, P, P, P, P, dx_dropped, None, None, None, P, 16, 128, 0.0, 7, 0, x_f32, fmt, 0, branch, None)

    def embed_bwd(fmt=BF16, branch=None):
        return "embed_ln_bwd", lib.cldrd_embed_ln_bwd(P, P, P, P, None, P, P, P, P, P, None, None, None, P, 16, 8, 128, 300, 0.0, 7, 0, None, fmt, 0, branch, None)

    def adamw(lo, hi, n=1024):
        return "adamw_step", lib.cldrd_adamw_step(P, P, P, P, P, None, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, None, P, lo, hi, None)

    def scatter(stride, idx=None):
        return "scatter_cls_grad", lib.cldrd_scatter_cls_grad(P, P, 4, 128, stride, idx, 32, BF16, None)

    cases = [
        lambda: search(P32=P, qmu=P), lambda: rescore(P32=P, qmu=P),                    # fp32 rows take no qmu
        lambda: search(), lambda: rescore(),                                            # neither P32 nor qmu
        lambda: search(P16=None, qmu=P), lambda: rescore(P16=None, qmu=P),              # fp16-row mode without the fp16 rows
        lambda: search(P16=None), lambda: rescore(P16=None),                            # no rows at all
        lambda: search8(qtile=256), lambda: search8(exhaustive=2), lambda: search8(d=132),             # the int8 chain: its tile, no tiled form, its widths,
        lambda: search8(qd=None), lambda: search8(scale=None),                                         # a scan without the query digits, no scales
        lambda: embed_fwd(table=None), lambda: embed_fwd(type_vocab=0), lambda: embed_fwd(type_vocab=-1),
        lambda: ln_bwd(x_f32=0, fmt=F32), lambda: ln_bwd(fmt=F32, dx_dropped=None), lambda: ln_bwd(x_f32=0, fmt=F16),
        lambda: ln_bwd(fmt=BF16, branch=P), lambda: ln_bwd(fmt=3), lambda: ln_bwd(fmt=-1),
        lambda: embed_bwd(fmt=BF16, branch=P), lambda: embed_bwd(fmt=3),
        lambda: adamw(2, 64), lambda: adamw(0, 62), lambda: adamw(0, 1028), lambda: adamw(1024, 2048),
        lambda: scatter(0), lambda: scatter(-8),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"


def test_no_cpu_fallback():
    """Ops refuse CPU tensors instead of silently computing on the host."""
    from cldrd_amd import hip_ops as ops
    from cldrd_amd.losses import KLDiv
    a = torch.zeros(64, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.gemm_nt(a, a, torch.zeros(64, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        KLDiv()(torch.zeros(2, 3), torch.zeros(2, 3))


def test_state_dict_keys_match_reference_layout():
    from cldrd_amd.encoder import EncoderConfig
    from cldrd_amd.models import NwayDualEncoder
    from oracle.encoder_ref import RefConfig, param_shapes
    for arch in ("distilbert", "bert"):
        cfg = EncoderConfig(arch=arch, vocab_size=256, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=32)
        m = NwayDualEncoder(cfg, share_weights=False)
        ref = param_shapes(RefConfig(arch=arch, vocab_size=256, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=32))
        sd = m.state_dict()
        assert sorted(sd) == sorted([f"{t}.{k}" for t in ("query_encoder", "passage_encoder") for k in ref])
        for k, shp in ref.items():
            assert tuple(sd["query_encoder." + k].shape) == tuple(shp)
        shared = NwayDualEncoder(cfg, share_weights=True)
        assert shared.passage_encoder is shared.query_encoder
        assert len(shared.state_dict()) == 2 * len(ref)       # both prefixes present, as in the reference


def test_flat_views_alias_and_load_state_dict():
    from cldrd_amd.encoder import EncoderConfig, HipEncoder
    cfg = EncoderConfig(vocab_size=256, dim=128, n_heads=2, hidden_dim=256, n_layers=1, max_position_embeddings=32)
    a, b = HipEncoder(cfg, seed=1), HipEncoder(cfg, seed=2)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.flat_p, b.flat_p)
    # DDP-style 'module.' prefix stripping as in reference retriever/index_text.py:63-73
    sd = {"module." + k: v for k, v in a.state_dict().items()}
    c = HipEncoder(cfg, seed=3)
    c.load_state_dict({k[7:]: v for k, v in sd.items()})
    assert torch.equal(a.flat_p, c.flat_p)
    # q/k/v weights are adjacent: the fused [3d, d] view is a plain slice
    off = c.layout.entries["transformer.layer.0.attention.q_lin.weight"][0]
    fused = c.flat_p[off:off + 3 * 128 * 128].view(384, 128)
    assert torch.equal(fused[128:256], dict(c.named_parameters())["transformer.layer.0.attention.k_lin.weight"])


def test_weight_decay_groups_follow_reference_rule():
    from cldrd_amd.trainer import no_decay
    assert no_decay("module.query_encoder.embeddings.LayerNorm.weight")
    assert no_decay("module.query_encoder.transformer.layer.0.ffn.lin1.bias")
    assert not no_decay("module.query_encoder.transformer.layer.0.sa_layer_norm.weight")


def test_lr_schedule_matches_golden():
    import numpy as np
    from cldrd_amd.trainer import linear_schedule_factor
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "lr_schedule.npz"))
    for name in ("a", "b", "c"):
        warm, total = int(g[name + "/warmup"]), int(g[name + "/total"])
        for s, f in zip(g[name + "/steps"], g[name + "/factor"]):
            assert linear_schedule_factor(int(s), warm, total) == pytest.approx(float(f), abs=1e-12)


def test_torch_library_ops_are_registered_with_fake_kernels():
    """torch.ops.cldrd.* (cl-drd_amd/torch_ops.py): every op is known to the dispatcher, has a schema and a fake (meta) kernel so
    shapes can be inferred without a GPU; a CPU tensor finds no kernel (no CPU fallback)."""
    import cldrd_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in T.OPS:
        assert hasattr(torch.ops.cldrd, name), name
        assert "cldrd::" + name in str(getattr(torch.ops.cldrd, name).default._schema)
    with FakeTensorMode():
        q, p = torch.empty(4, 768), torch.empty(32, 768)
        assert torch.ops.cldrd.nway_score(q, p, 4, 8, 0).shape == (4, 8)
        assert torch.ops.cldrd.nway_score(q, p, 4, 8, 1).shape == (4, 32)
        assert torch.ops.cldrd.nway_score(q, p, 4, 8, 2).shape == (4, 16)
        out, grad = torch.ops.cldrd.listwise_loss(torch.empty(4, 8), torch.empty(4, 8), 0, None, 1.0, -1.0, True)
        assert out.shape == (2,) and grad.shape == (4, 8)
        y = torch.ops.cldrd.linear(torch.empty(64, 128, dtype=torch.bfloat16), torch.empty(256, 128, dtype=torch.bfloat16), None, None, True, False)
        assert y.shape == (64, 256) and y.dtype == torch.bfloat16
        assert torch.ops.cldrd.self_attention(torch.empty(60, 384, dtype=torch.bfloat16), None, 2, 30, 2).shape == (60, 128)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.cldrd.nway_score(torch.zeros(2, 8), torch.zeros(4, 8), 2, 2, 0)
