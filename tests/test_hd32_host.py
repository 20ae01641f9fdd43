"""Head dim 32 (MiniLM-shaped BERT) without a GPU: the configurations that are accepted and refused, the argument checks of the four C entry
points (every call below is rejected in front of any HIP call, so small integers stand in for device pointers) and the refusals of
hip_ops.*(head_dim=32) that are raised before the device is touched."""
import os
import re

import pytest
import torch

from conftest import ROOT
from cldrd_amd import _lib
from cldrd_amd import hip_ops as ops
from cldrd_amd.encoder import EncoderConfig, HipEncoder, encode_autograd
from cldrd_amd.models.cross_encoder import CrossEncoder

NEW = ("cldrd_attention_fwd_hd32", "cldrd_attention_cls_fwd_hd32", "cldrd_attention_fwd_f32_hd32", "cldrd_attention_cls_fwd_f32_hd32")


def test_encoder_config_accepts_head_dim_64_and_even_headed_32():
    for dim, heads, hd in ((384, 12, 32), (128, 4, 32), (768, 12, 64), (128, 2, 64)):
        cfg = EncoderConfig(dim=dim, n_heads=heads, hidden_dim=4 * dim)
        cfg.validate()
        assert cfg.head_dim == hd
    for dim, heads in ((96, 2), (96, 3), (384, 3)):           # head dim 48; odd H at head dim 32; head dim 128
        with pytest.raises(ValueError, match="head dim 64.*head dim 32"):
            EncoderConfig(dim=dim, n_heads=heads, hidden_dim=256).validate()
        with pytest.raises(ValueError):
            HipEncoder(EncoderConfig(dim=dim, n_heads=heads, hidden_dim=256))


def test_cross_encoder_reads_a_minilm_config(tmp_path):
    from transformers import BertConfig, BertForSequenceClassification
    BertConfig(vocab_size=30522, hidden_size=384, num_hidden_layers=6, num_attention_heads=12, intermediate_size=1536, num_labels=1,
               architectures=["BertForSequenceClassification"]).save_pretrained(str(tmp_path))
    cfg, num_labels = CrossEncoder.read_config(str(tmp_path))
    assert (cfg.dim, cfg.n_heads, cfg.head_dim, cfg.n_layers, cfg.hidden_dim, num_labels) == (384, 12, 32, 6, 1536, 1)
    torch.manual_seed(0)
    tiny = tmp_path / "tiny"
    hf = BertForSequenceClassification(BertConfig(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
                                                  max_position_embeddings=300, num_labels=1))
    hf.save_pretrained(str(tiny))
    model = CrossEncoder.from_pretrained(str(tiny), eval_only=True)
    assert model.cfg.head_dim == 32 and torch.equal(model.head_w2, hf.state_dict()["classifier.weight"])
    with pytest.raises(ValueError, match="head dim 32.*eval_only"):          # a caller that does not say so gets what it got before: head dim 64
        CrossEncoder.from_pretrained(str(tiny))
    odd = tmp_path / "odd"
    BertConfig(vocab_size=100, hidden_size=96, num_hidden_layers=2, num_attention_heads=3, intermediate_size=256, num_labels=1,
               architectures=["BertForSequenceClassification"]).save_pretrained(str(odd))
    with pytest.raises(ValueError, match="head dim 32 with 3 heads"):
        CrossEncoder.read_config(str(odd))


def test_a_head_dim_32_tower_refuses_training_up_front():
    enc = HipEncoder(EncoderConfig(arch="distilbert", vocab_size=64, dim=128, n_heads=4, hidden_dim=256, n_layers=2, max_position_embeddings=32))
    ids, mask = torch.ones(2, 8, dtype=torch.int64), torch.ones(2, 8, dtype=torch.int64)
    for call in (lambda: enc.encode(ids, mask, save=True), lambda: enc.encode(ids, mask, train=True), lambda: enc.train().encode(ids, mask),
                 lambda: encode_autograd(enc, ids, mask)):
        with pytest.raises(ValueError, match="head dim 32 runs the evaluation passes only"):
            call()
    from cldrd_amd.trainer.nway_listwise import NwayTrainer

    class Model:          # the trainer looks at the towers' configurations before anything else
        def towers(self):
            return [enc]
    with pytest.raises(ValueError, match="head dim 32 runs the evaluation passes only"):
        NwayTrainer(Model())


def test_the_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cldrd_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name)


def test_hd32_entry_points_reject_bad_layouts_without_a_gpu():
    lib = _lib.load()
    P, nseq, L, H = 64, 4, 32, 2            # P: any non-null "pointer"

    def fwd(mask=None, cu=None, sl=None, n_list=0, Ltile=0, ctx=P, L=L, H=H, fmt=0, ctx16=None):
        return "attention_fwd_hd32", lib.cldrd_attention_fwd_hd32(P, mask, cu, sl, n_list, Ltile, ctx, nseq, L, H, fmt, ctx16, None)

    def cls_fwd(mask=None, cu=None, ctx=P, L=L, H=H, fmt=0, ctx16=None):
        return "attention_cls_fwd_hd32", lib.cldrd_attention_cls_fwd_hd32(P, P, mask, cu, ctx, nseq, L, H, fmt, ctx16, None)

    def f32(mask=None, cu=None, ctx=P, L=L, qkv=P):
        return "attention_fwd_f32_hd32", lib.cldrd_attention_fwd_f32_hd32(qkv, mask, cu, ctx, nseq, L, H, None)

    def f32_cls(mask=None, cu=None, ctx=P, L=L, ldq=H * 32):
        return "attention_cls_fwd_f32_hd32", lib.cldrd_attention_cls_fwd_f32_hd32(P, ldq, P, mask, cu, ctx, nseq, L, H, None)

    cases = [
        lambda: fwd(mask=P, cu=P), lambda: cls_fwd(mask=P, cu=P), lambda: f32(mask=P, cu=P), lambda: f32_cls(mask=P, cu=P),      # mask with cu_rows
        lambda: fwd(L=257), lambda: cls_fwd(L=257), lambda: f32(L=257), lambda: f32_cls(L=257),
        lambda: fwd(H=3), lambda: cls_fwd(H=3), lambda: fwd(H=1),                                                               # odd H
        lambda: fwd(fmt=5), lambda: cls_fwd(fmt=5), lambda: fwd(fmt=2), lambda: fwd(fmt=3),
        lambda: fwd(ctx=None, ctx16=None), lambda: cls_fwd(ctx=None, ctx16=None), lambda: f32(ctx=None), lambda: f32_cls(ctx=None),   # no output
        lambda: fwd(sl=P, n_list=2, Ltile=L),                                                                                   # seq_list without cu_rows
        lambda: fwd(cu=P, sl=P, n_list=0, Ltile=L), lambda: fwd(cu=P, sl=P, n_list=nseq + 1, Ltile=L), lambda: fwd(cu=P, sl=P, n_list=2, Ltile=L + 1),
        lambda: fwd(fmt=1, ctx16=P), lambda: cls_fwd(fmt=1, ctx16=P), lambda: fwd(fmt=1, ctx=None, ctx16=P),                   # the fp16 pass writes ctx only
        lambda: f32(qkv=None), lambda: f32(qkv=P + 4), lambda: f32_cls(ldq=H * 32 - 4), lambda: f32_cls(ldq=H * 32 + 2),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"
    lib.cldrd_set_tuning(None, 0)
    assert fwd(H=3)[1] != 0 and "even" in lib.cldrd_last_error().decode()


def test_hip_ops_head_dim_keyword_refusals():
    bf, f32 = torch.bfloat16, torch.float32
    nseq, L, H = 2, 8, 2
    qkv, ctx = torch.zeros(nseq * L, 3 * H * 32, dtype=bf), torch.zeros(nseq * L, H * 32, dtype=bf)
    lse, bits = torch.zeros(nseq, H, L, dtype=f32), torch.zeros(4, dtype=torch.int32)
    for kw in (dict(dropout_p=0.1), dict(lse=lse), dict(drop_bits=bits), dict(full_family=True)):
        args = dict(lse=None)
        args.update(kw)
        with pytest.raises(ValueError, match="head dim 32 runs the evaluation forward only"):
            ops.attention_fwd(qkv, None, ctx, args.pop("lse"), nseq, L, H, head_dim=32, **args)
    qc, kv = torch.zeros(nseq, H * 32, dtype=bf), torch.zeros(nseq * L, 2 * H * 32, dtype=bf)
    for kw in (dict(probs=torch.zeros(nseq, H, L, dtype=f32)), dict(probs=None, dropout_p=0.1)):
        with pytest.raises(ValueError, match="head dim 32 runs the evaluation forward only"):
            ops.attention_cls_fwd(qc, kv, None, ctx[:nseq], kw.pop("probs"), nseq, L, H, head_dim=32, **kw)
    for hd in (16, 48, 128, 0):
        with pytest.raises(ValueError, match="head dim"):
            ops.attention_fwd(qkv, None, ctx, None, nseq, L, H, head_dim=hd)
        with pytest.raises(ValueError, match="head dim"):
            ops.attention_cls_fwd(qc, kv, None, ctx[:nseq], None, nseq, L, H, head_dim=hd)
        with pytest.raises(ValueError, match="head dim"):
            ops.attention_fwd_f32(qkv.float(), None, ctx.float(), nseq, L, H, head_dim=hd)
    with pytest.raises(ValueError, match="even number of heads"):
        ops.attention_fwd(torch.zeros(nseq * L, 3 * 3 * 32, dtype=bf), None, torch.zeros(nseq * L, 3 * 32, dtype=bf), None, nseq, L, 3, head_dim=32)
