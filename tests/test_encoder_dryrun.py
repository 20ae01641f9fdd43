"""Host logic of the encoder / trainer without a GPU: every kernel launch is stubbed (`_lib.call` does nothing, the device check of the argument
validators is lifted), so a forward + backward walks the whole Python control flow - buffer formats, tape contents, the argument validation of
every hip_ops wrapper - in every mode: padded / packed, training / eval, fp16-operand FFN + QKV on / off, DistilBERT / BERT, CLS-only last layer.
Nothing is computed (the oracle and the GPU tests check values); this catches a wrong dtype, shape or missing buffer before a GPU box sees it."""
import numpy as np
import pytest
import torch

import cldrd_amd.synthetic as syn
from cldrd_amd import _lib, hip_ops as ops
from cldrd_amd.encoder import EncoderConfig, HipEncoder
from cldrd_amd.models import NwayDualEncoder


@pytest.fixture
def stubbed(monkeypatch):
    try:
        _lib.load()
    except Exception as e:
        pytest.skip(f"libcldrd_hip.so not built: {e}")
    return _install_stubs(monkeypatch)


def _install_stubs(monkeypatch):
    """Stub every launch; returns the recorder (the launch-trace generator next to the goldens installs the same stubs)."""
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
        calls.keep.append(t)
        return t
    monkeypatch.setattr(ops, "_chk", chk)
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), calls.args.append((name, a))))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(HipEncoder, "refresh_shadows", lambda self, need_transposed=True, cast=True, cast16=None, h_stale=False: _cpu_shadows(self))
    monkeypatch.setattr(HipEncoder, "_shadows_ok", lambda self, need_t, need_h=True: self.flat_h is not None)
    return calls


class _Calls(list):
    """The entry-point names in call order (what most tests look at); ``args``: (name, argument tuple) of the same calls."""

    def __init__(self):
        super().__init__()
        self.args = []
        self.keep = []          # every tensor a wrapper validated (the launch trace needs them alive: no address is reused)


# position of cu_rows (and, for the full-attention calls, of seq_list) in the C signatures of include/cldrd_hip.h
_CU_ARG = {"cldrd_attention_fwd": 2, "cldrd_attention_bwd": 2, "cldrd_attention_cls_fwd": 3, "cldrd_attention_cls_bwd": 2}
_LIST_ARG = 3
# position of the arguments that select a branch of a merged entry point: type_ids of the embedding forward, idx of the CLS-row calls
_TYPE_IDS_ARG = 4
_IDX_ARG = {"cldrd_add_rows": 5, "cldrd_scatter_cls_grad": 5}


def _cu_set(recorded, name):
    """For every recorded call of ``name``: is its cu_rows argument non-null (the packed layout)?"""
    return [a[_CU_ARG[name]] is not None for n, a in recorded if n == name]


def _cpu_shadows(enc):
    enc.flat_h = torch.zeros(enc.layout.total, dtype=torch.bfloat16)
    enc.flat_h16 = torch.zeros(enc.layout.total, dtype=torch.float16)
    enc.flat_t = torch.zeros(enc.layout.t_total, dtype=torch.float16 if enc.amp16 else torch.bfloat16)
    enc._t_fresh = True
    enc._shadow_version = enc.flat_p._version


def cfg_of(arch, layers):
    return EncoderConfig(arch=arch, vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=layers, max_position_embeddings=64,
                         dropout=0.1, attention_dropout=0.1)


@pytest.mark.parametrize("arch,layers", [("distilbert", 3), ("bert", 2), ("distilbert", 1), ("bert", 7)])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("amp,stream16", [("fp16", True), ("fp16", False), ("bf16", True)])
def test_forward_backward_walks_every_mode(stubbed, monkeypatch, arch, layers, packed, amp, stream16):
    """CLDRD_AMP = fp16 (all-fp16 training pass; evaluation with fp16 FFN / out-projection operands, fp16 QKV operands on towers deeper than 6
    layers: the 7-layer case) and bf16 (every operand bf16), the fp16 mode also with its fp32 gradient stream (test hook)."""
    monkeypatch.setenv("CLDRD_AMP", amp)
    enc = HipEncoder(cfg_of(arch, layers), seed=1)
    enc._grad_stream16 = stream16
    assert enc.amp16 == (amp == "fp16") and enc.grad_stream16 == (amp == "fp16" and stream16) and enc.needs_h16 == (amp == "fp16")
    t16 = torch.float16 if enc.amp16 else torch.bfloat16
    M, L = 6, 24
    lens = np.array([24, 3, 10, 17, 5, 8])
    ids = torch.randint(3, 500, (M, L))
    mask = (torch.arange(L)[None, :] < torch.from_numpy(lens)[:, None]).long()
    lengths = lens.tolist() if packed else None
    for hp in (False, True):
        enc.hp_forward = hp
        cls = enc.encode(ids, mask, train=False, save=False, lengths=lengths)
        assert cls.shape == (M, 128) and cls.dtype == torch.float32
        cls, tape = enc.encode(ids, mask, train=True, save=True, lengths=lengths)
        pk = packed                                 # one pass per mode for both towers: a training pass packs whenever it is given lengths
        assert (tape.pack is not None) == pk and tape.T == (int(lens.sum()) if pk else M * L)
        for a in tape.layers:                       # what the backward's MFMAs read: one 16-bit format per mode
            for k in ("x_in", "ctx", "x1", "h", "pre"):
                assert a[k] is not None and a[k].dtype == t16, (k, a[k].dtype)
            assert (a.get("qkv") if "qkv" in a else a["kv"]).dtype == t16
        hooks = []
        enc.backward_from_cls(tape, torch.zeros(M, 128), after_layer=hooks.append, accumulate=False)
        assert sorted(hooks) == list(range(-1, layers))        # every bucket reported once (the embedding block before the last weight-gradient group)
    kinds = set(stubbed)
    assert "cldrd_gemm_nt16" in kinds and "cldrd_wgrad_group" in kinds and "cldrd_embed_ln_bwd" in kinds
    for name in ("cldrd_attention_cls_fwd", "cldrd_attention_cls_bwd"):       # the packed layout is said by the cu_rows argument
        assert any(_cu_set(stubbed.args, name)) == packed, name
    for name in ("cldrd_attention_fwd", "cldrd_attention_bwd"):              # (a one-layer tower has only the CLS-only last layer)
        assert any(_cu_set(stubbed.args, name)) == (packed and layers > 1), name
    assert "cldrd_unpack_rows16" not in kinds                      # round 6: attention reads the packed rows through cu, no row moves
    # the CLS rows are said by idx in a packed pass, by the stride L in a padded one; the full last layer (test hook; never packed) scatters dcls
    if not packed:
        enc.hp_forward, enc.cls_only_last = False, False
        cls, tape = enc.encode(ids, mask, train=True, save=True)
        enc.backward_from_cls(tape, torch.zeros(M, 128), accumulate=False)
        enc.cls_only_last = True
        assert "cldrd_scatter_cls_grad" in stubbed
    assert "cldrd_add_rows" in stubbed
    for name, pos in _IDX_ARG.items():
        assert all((a[pos] is not None) == packed for n, a in stubbed.args if n == name), name
    # token types: none of the passes above has any; a pass that is given some hands them to the same entry point - BERT only, DistilBERT has no table
    assert not any(a[_TYPE_IDS_ARG] is not None for n, a in stubbed.args if n == "cldrd_embed_ln_fwd")
    n0, enc.hp_forward = len(stubbed.args), False
    enc.encode(ids, mask, train=False, save=False, lengths=lengths, token_type_ids=(torch.arange(L)[None, :] >= 5).long().expand(M, L))
    assert [a[_TYPE_IDS_ARG] is not None for n, a in stubbed.args[n0:] if n == "cldrd_embed_ln_fwd"] == [arch == "bert"]


@pytest.mark.parametrize("lens,want", [([200, 3, 10, 130, 5, 128], 2), ([100, 3, 10, 128, 5, 64], 1), ([200, 150, 129, 130, 131, 199], 0)])
def test_packed_batches_above_128_tokens_split_their_attention_launches_by_length(stubbed, monkeypatch, lens, want):
    """encoder._Pack at L > 128: the sequences of at most 128 tokens go through the L <= 128 kernels (cldrd_attention_fwd / _bwd with a seq_list and tile 128),
    the others through a second launch at tile L; all short: one listed launch; all long: the plain packed launch."""
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=256,
                        dropout=0.1, attention_dropout=0.1)
    enc = HipEncoder(cfg, seed=1)
    lens = lens * 4                                   # 24 sequences: enough tokens for the encoder to pack (would_pack: >= 1024)
    M, L = len(lens), 200
    ids = torch.randint(3, 500, (M, L))
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    n0 = len(stubbed)
    cls, tape = enc.encode(ids, mask, train=True, save=True, lengths=lens)
    assert tape.pack is not None and [t for _, t in tape.pack.groups] == ([128, L] if want == 2 else [128] if want == 1 else [0])
    if want:
        assert sorted(int(i) for sl, _ in tape.pack.groups for i in sl.tolist()) == list(range(M))
    enc.backward_from_cls(tape, torch.randn(M, cfg.dim))
    for name in ("cldrd_attention_fwd", "cldrd_attention_bwd"):
        calls = [a for n, a in stubbed.args[n0:] if n == name]
        listed = sum(a[_LIST_ARG] is not None for a in calls)
        plain_packed = sum(a[_CU_ARG[name]] is not None and a[_LIST_ARG] is None for a in calls)
        assert listed == want * 1 and plain_packed == (0 if want else 1), name


def test_trainer_step_walks_with_stubbed_kernels(stubbed, monkeypatch):
    """forward_backward + optimizer launches of NwayTrainer (padded and packed batch) with stubbed kernels; `lengths` travel from the
    host-side mask (trainer.batch_to_device) to the passage tower."""
    from cldrd_amd.trainer import nway_listwise as TL
    monkeypatch.setattr(TL.NwayTrainer, "_require_gpu", staticmethod(lambda dev: None))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: _Null())
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: _FakeStream())
    monkeypatch.setenv("CLDRD_GRAPH", "0")
    model = NwayDualEncoder(cfg_of("distilbert", 2), share_weights=False)
    tr = TL.NwayTrainer(model, loss="kl_div")
    tr.q_stream = None
    batch = syn.nway_batch(5, 2, 3, 6, 20, vocab=512, ragged=True, label_kind="teacher")
    moved = TL.batch_to_device(batch, torch.device("cpu"))
    assert moved["nway_passages"]["lengths"].tolist() == batch["nway_passages"]["attention_mask"].sum(-1).reshape(-1).tolist()
    n0 = len(stubbed)
    tr.train_step(moved)
    assert tr.global_step == 1 and "cldrd_adamw_step" in stubbed[n0:] and "cldrd_loss_fwd_bwd" in stubbed[n0:]


@pytest.mark.parametrize("ln_defer", [True, False])
def test_two_backwards_on_one_tower_keep_their_own_queues(stubbed, monkeypatch, ln_defer):
    """A shared-weights tower has two tapes: their backwards, run one after the other with ``accumulate=True``, each launch their own
    weight-gradient / LayerNorm-reduction groups - one weight-gradient launch per tape, and no launch mixes the token-row counts of the two
    tapes (6 x 24 rows on one, 4 x 12 on the other): the queues are locals of one backward_from_cls call."""
    monkeypatch.setenv("CLDRD_AMP", "fp16")
    enc = HipEncoder(cfg_of("distilbert", 3), seed=1)
    enc.ln_defer = ln_defer
    shapes = ((6, 24), (4, 12))
    tapes = [enc.encode(torch.randint(3, 500, s), torch.ones(s, dtype=torch.long), train=True, save=True, seed=11)[1] for s in shapes]
    n0 = len(stubbed.args)
    for t in tapes:
        enc.backward_from_cls(t, torch.zeros(t.M, 128), accumulate=True)
    rows = {"cldrd_wgrad_group": 4, "cldrd_ln_reduce_group": 1}       # position of the per-job row counts (int array) in the C signature
    count = {"cldrd_wgrad_group": 9, "cldrd_ln_reduce_group": 5}      # ... and of the job count
    want = sorted((n, a[count[n]], list(a[rows[n]])) for n, a in stubbed.args[n0:] if n in rows)
    assert [g[0] for g in want].count("cldrd_wgrad_group") == 2 and all(len(set(g[2])) <= 2 for g in want)       # (T and M rows of ONE tape each)


@pytest.mark.parametrize("kind", ["device_seed", "own_scale"])
def test_a_failing_launch_in_the_backward_restores_the_launch_contexts(stubbed, monkeypatch, kind):
    """backward_from_cls runs under up to two thread-local launch contexts - the device seed word of a ``device_seed`` tape, and the tower's own
    loss scale for an fp16 tape outside a trainer.  A launch that raises in the middle of the pass must leave ``ops._TLS.seed_base`` /
    ``ops._TLS.loss_scale`` at what they were before the call."""
    monkeypatch.setenv("CLDRD_AMP", "fp16" if kind == "own_scale" else "bf16")
    enc = HipEncoder(cfg_of("distilbert", 3), seed=1)
    word = torch.zeros(2, dtype=torch.int64)                # stands in for the trainer's device seed word
    enc.seed_base_ptr = word.data_ptr()
    ids, mask = _trace_batch()
    cls, tape = enc.encode(ids, mask, train=True, save=True, device_seed=kind == "device_seed")
    assert tape.device_seed == (kind == "device_seed") and (tape.layers[-1]["h"].dtype == torch.float16) == (kind == "own_scale")
    inside = []

    def failing(name, *a):
        if name == "cldrd_attention_bwd":                   # layer 1's attention backward: the last layer is behind it, two layers ahead
            inside.append((getattr(ops._TLS, "seed_base", None), getattr(ops._TLS, "loss_scale", None)))
            raise RuntimeError("launch failed")
    monkeypatch.setattr(ops, "call", failing)
    before = (getattr(ops._TLS, "seed_base", None), getattr(ops._TLS, "loss_scale", None))
    with pytest.raises(RuntimeError, match="launch failed"):
        enc.backward_from_cls(tape, torch.zeros(len(_LENS), 128))
    seed_in, scale_in = inside[0]                           # the context under test really was entered when the launch failed
    assert (seed_in == word.data_ptr()) if kind == "device_seed" else (scale_in is not None and scale_in[0] == enc._own_scale.data_ptr())
    assert (getattr(ops._TLS, "seed_base", None), getattr(ops._TLS, "loss_scale", None)) == before


class _FakeEvent:
    def record(self, stream=None):
        pass


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _FakeStream:
    cuda_stream = 0

    def wait_stream(self, s):
        pass

    def wait_event(self, e):
        pass


def test_would_pack_rules():
    """Packing is chosen from the host-side token counts: needs a mask and lengths, at least 8 % padding, and never moves the Linear layers across the
    M = 1024 boundary between the large-M and the small-M GEMM kernels (their summation orders differ: packed == padded would stop being bit-exact)."""
    enc = HipEncoder(cfg_of("distilbert", 2), seed=1)
    M, L = 64, 32                                     # 2048 padded rows
    full = [L] * M
    assert not enc.would_pack(full, M, L)             # no padding at all
    assert not enc.would_pack(None, M, L)
    assert enc.would_pack([20] * M, M, L)             # 1280 tokens: both sides of the run on the large-M kernel
    assert not enc.would_pack([20] * M, M, L, has_mask=False)
    assert not enc.would_pack([10] * M, M, L)         # 640 tokens < 1024 <= 2048 padded rows: stays padded
    assert enc.would_pack([10] * 16, 16, L)           # 160 of 512: both small-M
    assert not enc.would_pack([31] * M, M, L)         # 3 % padding: not worth the row moves
    assert not enc.would_pack([20] * (M - 1) + [0], M, L)         # an empty row: the packed kernels take 1 .. L rows per sequence
    assert not enc.would_pack([20] * (M - 1) + [L + 1], M, L) and not enc.would_pack([20] * (M - 1), M, L)      # counts of another batch shape


_MAIN = _FakeStream()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Launch trace: what the tower hands to the C ABI, launch by launch, in a canonical form that two walks of one case reproduce exactly.
# tests/golden/encoder_launch_trace.json holds the trace of every case below as taken at the commit it names (make_encoder_launch_trace.py,
# next to it, imports the cases from here); a host-side change of the tower that is meant to change no behaviour must reproduce it.
# Canonical form of a launch: the entry-point name and every argument in order - floats as repr, every address (an int >= 2^32, also inside
# the ctypes pointer arrays of the grouped launches) as p<k>, k = order of first appearance within the case.  Addresses are comparable
# because nothing is freed during a case (`_KeepAlive` + the stubbed _chk hold every tensor) and the seeds are explicit and small (a drawn
# seed is a 47-bit number and would read as an address; where the trainer draws them they are still the same number in every walk).

class _KeepAlive(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self, keep):
        super().__init__()
        self.keep = keep

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.keep.extend(t for t in torch.utils._pytree.tree_leaves(out) if isinstance(t, torch.Tensor))
        return out


def _canonical(recorded):
    """[(name, argument tuple)] -> [(name, canonical argument string)]"""
    import ctypes
    seen = {}

    def one(v):
        if isinstance(v, ctypes.Array):
            return "[" + ",".join(one(e) for e in v) + "]"
        if isinstance(v, int) and not isinstance(v, bool):
            return f"p{seen.setdefault(v, len(seen))}" if v >= 1 << 32 else str(v)
        if isinstance(v, (float, bool, bytes, str)) or v is None:
            return repr(v)
        raise TypeError(f"launch trace: unexpected argument type {type(v)}")
    return [(name, ",".join(one(v) for v in a)) for name, a in recorded]


_LENS = [24, 3, 10, 17, 5, 8]


def _trace_batch(lens=_LENS, L=24):
    return torch.randint(3, 500, (len(lens), L)), (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()


def _mark(calls, what):
    """a hook whose calls appear in the trace between the launches"""
    return lambda *a: calls.args.append((what, a))


def _tower_case(amp, arch, layers, lengths, tweak=None, cls_only=True):
    """evaluation pass with hp_forward off and on, then a training pass + backward, writing and accumulating"""
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", amp)
        enc = HipEncoder(cfg_of(arch, layers), seed=1)
        enc.cls_only_last = cls_only
        if tweak is not None:
            setattr(enc, *tweak)
        ids, mask = _trace_batch()
        lens = _LENS if lengths else None
        for hp in (False, True):
            enc.hp_forward = hp
            enc.encode(ids, mask, train=False, seed=11, lengths=lens)
        enc.hp_forward = False
        for acc in (False, True):
            cls, tape = enc.encode(ids, mask, train=True, save=True, seed=11, lengths=lens)
            enc.backward_from_cls(tape, torch.zeros(len(_LENS), 128), after_layer=_mark(calls, "after_layer"), accumulate=acc,
                                  before_last_wgrad=_mark(calls, "before_last_wgrad"))
    return run


def _empty_tower_case(amp):
    """no transformer layer at all: the CLS rows of the embedding LayerNorm (forward only: there is nothing to send a gradient through)"""
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", amp)
        enc = HipEncoder(cfg_of("distilbert", 0), seed=1)
        ids, mask = _trace_batch()
        enc.encode(ids, mask, train=False, seed=11)
        enc.encode(ids, mask, train=False, seed=11, lengths=_LENS)
        enc.encode(ids, mask, train=True, save=True, seed=11)
        enc.encode(ids, mask, fp32=True)
    return run


def _typed_case(amp, arch, layers, lengths):
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", amp)
        enc = HipEncoder(cfg_of(arch, layers), seed=1)
        ids, mask = _trace_batch()
        enc.encode(ids, mask, train=False, seed=11, lengths=_LENS if lengths else None,
                   token_type_ids=(torch.arange(24)[None, :] >= 5).long().expand(len(_LENS), 24))
    return run


def _packed_rows(typed=True):
    T = sum(_LENS)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in _LENS])
    return torch.randint(3, 500, (T,)), ((pos >= 2).to(torch.int32) if typed else None), pos


def _packed_case(amp, arch, layers, width):
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", amp)
        enc = HipEncoder(cfg_of(arch, layers), seed=1)
        rows = _packed_rows()
        enc.encode(None, None, train=False, seed=11, lengths=_LENS, packed=rows + ((width,) if width else ()))
    return run


def _fp32_case(arch, layers, form):
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", "fp16")
        enc = HipEncoder(cfg_of(arch, layers), seed=1)
        ids, mask = _trace_batch()
        types = (torch.arange(24)[None, :] >= 5).long().expand(len(_LENS), 24)
        if form == "padded":
            enc.encode(ids, mask, fp32=True, token_type_ids=types)
        elif form == "lengths":
            enc.encode(ids, mask, fp32=True, lengths=_LENS, token_type_ids=types)
        elif form == "packed":
            enc.encode(None, None, fp32=True, lengths=_LENS, packed=_packed_rows())
            enc.encode(None, None, fp32=True, lengths=_LENS, packed=_packed_rows(typed=False) + (32,))
        else:
            enc.cls_only_last = False
            enc.encode(ids, mask, fp32=True)
            enc.encode(ids, mask, fp32=True, lengths=_LENS)          # (stays padded)
    return run


def _long_case(lens):
    """the batches of test_packed_batches_above_128_tokens_...: 2, 1 and 0 listed attention launches"""
    def run(calls, monkeypatch):
        monkeypatch.setenv("CLDRD_AMP", "fp16")
        cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=256,
                            dropout=0.1, attention_dropout=0.1)
        enc = HipEncoder(cfg, seed=1)
        ids, mask = _trace_batch(lens * 4, 200)
        cls, tape = enc.encode(ids, mask, train=True, save=True, seed=11, lengths=lens * 4)
        enc.backward_from_cls(tape, torch.zeros(len(lens) * 4, cfg.dim))
    return run


def _trainer_case():
    """one NwayTrainer.train_step on fake streams (the optimizer launches included)"""
    def run(calls, monkeypatch):
        from cldrd_amd.trainer import nway_listwise as TL
        monkeypatch.setattr(TL.NwayTrainer, "_require_gpu", staticmethod(lambda dev: None))
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _MAIN)
        monkeypatch.setattr(torch.cuda, "stream", lambda s_: _Null())
        monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: _FakeStream())
        monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: _FakeEvent())
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s_: None)
        monkeypatch.setenv("CLDRD_GRAPH", "0")
        monkeypatch.setenv("CLDRD_AMP", "fp16")
        torch.manual_seed(0)
        model = NwayDualEncoder(cfg_of("distilbert", 3), share_weights=False)
        tr = TL.NwayTrainer(model, loss="kl_div")
        tr.q_stream, tr.l_stream = _FakeStream(), _FakeStream()
        batch = syn.nway_batch(5, 2, 3, 6, 20, vocab=512, ragged=True, label_kind="teacher")
        tr.train_step(TL.batch_to_device(batch, torch.device("cpu")))      # (the ragged batch with host lengths)
        return model, tr
    return run


def _trace_cases():
    cases = {}
    for amp in ("fp16", "bf16"):
        for lengths in (False, True):
            lay = "lengths" if lengths else "padded"
            for arch, layers in (("distilbert", 3), ("bert", 2), ("bert", 7), ("distilbert", 1)):
                cases[f"tower-{amp}-{lay}-{arch}{layers}"] = _tower_case(amp, arch, layers, lengths)
            for tag, tweak in (("stream32", ("_grad_stream16", False)), ("ln_now", ("ln_defer", False)), ("flush2", ("wgrad_flush_layers", 2))):
                if tag != "stream32" or amp == "fp16":
                    cases[f"tower-{amp}-{lay}-distilbert3-{tag}"] = _tower_case(amp, "distilbert", 3, lengths, tweak)
            cases[f"typed-{amp}-{lay}-bert2"] = _typed_case(amp, "bert", 2, lengths)
            cases[f"typed-{amp}-{lay}-distilbert3"] = _typed_case(amp, "distilbert", 3, lengths)
        cases[f"tower-{amp}-lengths-bert7-flush2"] = _tower_case(amp, "bert", 7, True, ("wgrad_flush_layers", 2))
        cases[f"tower-{amp}-padded-distilbert0"] = _empty_tower_case(amp)
        cases[f"full_last-{amp}-padded-distilbert3"] = _tower_case(amp, "distilbert", 3, False, cls_only=False)
        for width in (0, 32):
            cases[f"packed_rows-{amp}-bert2-width{width}"] = _packed_case(amp, "bert", 2, width)
            cases[f"packed_rows-{amp}-bert7-width{width}"] = _packed_case(amp, "bert", 7, width)
    for form in ("padded", "lengths", "packed", "full_last"):
        cases[f"fp32-{form}-bert2"] = _fp32_case("bert", 2, form)
        cases[f"fp32-{form}-distilbert3"] = _fp32_case("distilbert", 3, form)
    for lens, want in (([200, 3, 10, 130, 5, 128], 2), ([100, 3, 10, 128, 5, 64], 1), ([200, 150, 129, 130, 131, 199], 0)):
        cases[f"long-listed{want}"] = _long_case(lens)
    cases["trainer-free_running"] = _trainer_case()
    return cases


TRACE_CASES = _trace_cases()


def walk_trace(case, calls, monkeypatch, cases=None):
    """Run one case (of ``cases``, default TRACE_CASES) under the stubs of ``_install_stubs``; -> [(entry point, 8-hex-digit hash of its
    canonical arguments)]"""
    import hashlib
    monkeypatch.delenv("CLDRD_PACK", raising=False)
    n0 = len(calls.args)
    with _KeepAlive(calls.keep):
        calls.keep.append((TRACE_CASES if cases is None else cases)[case](calls, monkeypatch))
    return [(name, hashlib.sha1(a.encode()).hexdigest()[:8]) for name, a in _canonical(calls.args[n0:])]


_TRACE_GOLDEN = None


def _load_golden(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as fh:
        return json.load(fh)["cases"]


def _trace_golden():
    global _TRACE_GOLDEN
    if _TRACE_GOLDEN is None:
        _TRACE_GOLDEN = _load_golden("encoder_launch_trace.json")
    return _TRACE_GOLDEN


def test_launch_trace_golden_lists_every_case():
    assert sorted(_trace_golden()) == sorted(TRACE_CASES)


@pytest.mark.parametrize("case", sorted(TRACE_CASES))
def test_launch_trace_matches_golden(stubbed, monkeypatch, case):
    """Every launch of the case - entry point, argument values, which buffer goes where - is the one the golden's commit made."""
    want = _trace_golden()[case]
    got = walk_trace(case, stubbed, monkeypatch)
    for k, ((name, digest), wname, wdigest) in enumerate(zip(got, want["names"], want["hashes"])):
        assert (name, digest) == (wname, wdigest), f"{case}: launch {k} differs: {name} (golden: {wname})"
    assert len(got) == len(want["names"]), f"{case}: {len(got)} launches, golden {len(want['names'])}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# Launch trace of the training step (tests/golden/trainer_launch_trace.json, written by make_encoder_launch_trace.py --trainer at the commit
# it names): the same canonical form, with the stream in it.  `torch.cuda.stream(s)` is a real context over a stack of fake streams, every
# launch's stream argument is the small index of the stack's top, and the cross-stream edges (wait_stream, wait_event, Event.record) and
# the graph calls (capture begin / end, replay) are marks between the launches - so a change of NwayTrainer's host code that is meant to
# leave every launch on its stream, in its order, behind its waits must reproduce the golden.

class _TraceStream:
    def __init__(self, rig, idx):
        self.rig, self.idx, self.cuda_stream = rig, idx, idx

    def wait_stream(self, s):
        self.rig.mark("wait_stream", self.idx, s.idx)

    def wait_event(self, e):
        self.rig.mark("wait_event", self.idx, e.idx)


class _TraceEvent:
    def __init__(self, rig, idx):
        self.rig, self.idx = rig, idx

    def record(self, stream=None):
        self.rig.mark("event_record", self.idx, (stream or self.rig.stack[-1]).idx)


class _TraceGraph:
    def __init__(self, rig, idx):
        self.rig, self.idx = rig, idx

    def replay(self):
        self.rig.mark("graph_replay", self.idx)


class _StreamRig:
    """torch.cuda's stream / event / graph surface as the trainer uses it, on the host: stream 0 is the main one."""

    def __init__(self, calls, monkeypatch):
        import contextlib
        self.calls, self.n_streams, self.n_events, self.n_graphs, self.capturing = calls, 0, 0, 0, False
        self.stack = [self.new_stream()]

        @contextlib.contextmanager
        def on(s):
            self.stack.append(s)
            try:
                yield
            finally:
                self.stack.pop()

        @contextlib.contextmanager
        def capture(g, **kw):
            self.mark("capture_begin", g.idx)
            self.capturing = True
            try:
                yield
            finally:
                self.capturing = False
                self.mark("capture_end", g.idx)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: self.stack[-1])
        monkeypatch.setattr(torch.cuda, "stream", on)
        monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: self.new_stream())
        monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: self.new_event())
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: self.capturing)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
        monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: self.new_graph())
        monkeypatch.setattr(torch.cuda, "graph", capture)
        monkeypatch.setattr(torch.Tensor, "record_stream", lambda t, s_: None)
        monkeypatch.setattr(ops, "_stream", lambda: self.stack[-1].idx)

    def mark(self, what, *a):
        self.calls.args.append((what, a))

    def new_stream(self):
        self.n_streams += 1
        return _TraceStream(self, self.n_streams - 1)

    def new_event(self):
        self.n_events += 1
        return _TraceEvent(self, self.n_events - 1)

    def new_graph(self):
        self.n_graphs += 1
        return _TraceGraph(self, self.n_graphs - 1)


def _step_batch(TL, ragged, batch=2, teacher=False):
    """``ragged``: the packed batch.  (At 20 tokens the generator's MS MARCO-shaped lengths are all 20 - its floor is 16 - so the padding that
    makes the encoder pack the batch is cut here: 63 of 120 token rows.)"""
    b = syn.nway_batch(5, batch, 3, 6, 20, vocab=512, ragged=ragged, label_kind="teacher", with_teacher_scores=teacher)
    if ragged:
        nw = b["nway_passages"]
        mask = (torch.arange(20)[None, :] < torch.tensor([20, 3, 10, 17, 5, 8] * batch)[:3 * batch, None]).long().view(batch, 3, 20)
        nw["attention_mask"], nw["input_ids"] = mask, nw["input_ids"] * mask
    return TL.batch_to_device(b, torch.device("cpu"))


def _step_trainer(calls, monkeypatch, amp, model_kw, trainer_kw, hooks=()):
    from cldrd_amd.trainer import nway_listwise as TL
    rig = _StreamRig(calls, monkeypatch)
    monkeypatch.setattr(TL.NwayTrainer, "_require_gpu", staticmethod(lambda dev: None))
    monkeypatch.setenv("CLDRD_AMP", amp)
    torch.manual_seed(0)
    model = NwayDualEncoder(cfg_of("distilbert", 3), **{"share_weights": False, **model_kw})
    tr = TL.NwayTrainer(model, **{"loss": "kl_div", **trainer_kw})
    tr.q_stream, tr.l_stream = rig.new_stream(), rig.new_stream()       # (the constructor makes none for a host model)
    for name, value in hooks:
        setattr(tr, name, value)
    return TL, rig, model, tr


def _step_case(amp="fp16", ragged=(True, False), model_kw=None, trainer_kw=None, hooks=(), standalone=False, sink_used=None):
    """one eager step per entry of ``ragged`` (True: the packed batch, False: the padded one) on one trainer.  ``sink_used``: what the
    library reports for a norm sink after the passage tower's gradient launches (stubbed launches write nothing: 0, the separate late
    pass); a positive count walks the sink's own branch, -2 (the sink overflowed) the separate pass behind ONE warning."""
    def run(calls, monkeypatch):
        import warnings
        monkeypatch.setenv("CLDRD_GRAPH", "0")
        TL, rig, model, tr = _step_trainer(calls, monkeypatch, amp, model_kw or {}, trainer_kw or {}, hooks)
        if sink_used is not None:
            class reported(ops.norm_sink):
                def __exit__(self, *exc):
                    super().__exit__(*exc)
                    if self.slots is not None:
                        self.used = sink_used
            monkeypatch.setattr(ops, "norm_sink", reported)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for r in ragged:
                batch = _step_batch(TL, r, teacher=tr.distill is not None)
                nw = batch["nway_passages"]
                assert model.passage_encoder.would_pack(nw["lengths"], 6, 20) == r
                if standalone:
                    tr.forward_backward(batch)
                    tr.optimizer_step()
                else:
                    tr.train_step(batch)
        assert tr.global_step == len(ragged) and len([w for w in caught if "norm sink" in str(w.message)]) == (1 if sink_used == -2 else 0)
        return model, tr
    return run


def _graph_case():
    """the graph path: six steps of one padded shape (three eager, the capture + first replay, two replays), one eager step of a second
    shape while the step state lives in device memory, then a stand-alone forward_backward + optimizer_step in that state.  A host tensor
    is never ``is_cuda``, so `_graph_wanted` is its one-GPU rule without the device test."""
    def run(calls, monkeypatch):
        import warnings
        from cldrd_amd.encoder import _env_flag
        monkeypatch.delenv("CLDRD_GRAPH", raising=False)
        TL, rig, model, tr = _step_trainer(calls, monkeypatch, "fp16", {}, {})
        monkeypatch.setattr(TL.NwayTrainer, "_graph_wanted", lambda self: (not self.model.share_weights and not self._graph_broken
                                                                            and _env_flag("CLDRD_GRAPH", "1") != "0"))
        with warnings.catch_warnings():
            warnings.simplefilter("error")          # a failed capture is a warning and an eager step: not what this case walks
            for _ in range(6):
                tr.train_step(_step_batch(TL, False))
            assert rig.n_graphs == 1 and [e["graph"] is not None for e in tr._graphs.values()] == [True]
            other = _step_batch(TL, False, batch=3)
            tr.train_step(other)
            tr.forward_backward(other)
            tr.optimizer_step()
        assert rig.n_graphs == 1 and tr.global_step == 8 and tr._state is not None
        return model, tr
    return run


def _trainer_trace_cases():
    cases = {}
    for amp in ("fp16", "bf16"):
        cases[f"step-{amp}-packed"] = _step_case(amp, ragged=(True,))
        cases[f"step-{amp}-padded"] = _step_case(amp, ragged=(False,))
    cases["step-distill_kl_div"] = _step_case(trainer_kw=dict(distill="kl_div", distill_alpha=0.5, distill_T=2.0))
    cases["step-distill_only"] = _step_case(trainer_kw=dict(loss="lambda_mrr", distill="kl_div", distill_only=True))
    cases["step-reg_lambda"] = _step_case(trainer_kw=dict(reg_lambda=0.25))
    cases["step-share_weights"] = _step_case(model_kw=dict(share_weights=True))
    cases["step-zero_all_grads"] = _step_case(hooks=(("zero_all_grads", True),))
    cases["step-no_norm_sink"] = _step_case(hooks=(("use_norm_sink", False),))
    cases["step-sink_used"] = _step_case(sink_used=7)
    cases["step-sink_overflow"] = _step_case(sink_used=-2)
    cases["step-in_batch"] =_step_case(model_kw=dict(in_batch_loss=True, all_in_batch_neg=False))
    cases["step-all_in_batch"] = _step_case(model_kw=dict(in_batch_loss=True, all_in_batch_neg=True))
    cases["step-standalone"] = _step_case(standalone=True)
    cases["graph-six_steps_then_second_shape"] = _graph_case()
    return cases


TRAINER_TRACE_CASES = _trainer_trace_cases()
_TRAINER_GOLDEN = None


def _trainer_golden():
    global _TRAINER_GOLDEN
    if _TRAINER_GOLDEN is None:
        _TRAINER_GOLDEN = _load_golden("trainer_launch_trace.json")
    return _TRAINER_GOLDEN


def test_trainer_launch_trace_golden_lists_every_case():
    assert sorted(_trainer_golden()) == sorted(TRAINER_TRACE_CASES)


@pytest.mark.parametrize("case", sorted(TRAINER_TRACE_CASES))
def test_trainer_launch_trace_matches_golden(stubbed, monkeypatch, case):
    """Every launch of the training step - entry point, arguments, stream - and every cross-stream wait between them is the one the golden's
    commit made."""
    want = _trainer_golden()[case]
    got = walk_trace(case, stubbed, monkeypatch, TRAINER_TRACE_CASES)
    for k, ((name, digest), wname, wdigest) in enumerate(zip(got, want["names"], want["hashes"])):
        assert (name, digest) == (wname, wdigest), f"{case}: entry {k} differs: {name} (golden: {wname})"
    assert len(got) == len(want["names"]), f"{case}: {len(got)} entries, golden {len(want['names'])}"
