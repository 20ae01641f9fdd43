"""The deterministic mode of the embedding backward (--deterministic), host side, without a GPU: the argument checks of the new entry
points, the chunk constant, the command-line flag down to the towers, and a stubbed step that walks the new launches."""
import os
import re

import pytest
import torch

from conftest import ROOT


def test_new_entry_points_reject_inconsistent_arguments():
    """Every call below is rejected by a check in front of any HIP call, so small integers stand in for device pointers (tests/test_capi.py);
    the message names the op and never carries a switch-like CLDRD_ word (the product library is searched for those)."""
    from cldrd_amd import _lib
    lib = _lib.load()
    P = 64                                  # any non-null "pointer"
    BIG = 1 << 30

    def rows(T=16, d=128, L=8, fmt=0, branch=None, dx=P, dy=P, ids=P, vocab=300):
        return "embed_ln_bwd_rows", lib.cldrd_embed_ln_bwd_rows(dy, ids, P, P, None, P, P, P, dx, None, None, None, P, T, L, d, vocab, 0.0, 7, 0, None,
                                                                fmt, 0, branch, None)

    def order(keys=P, T=16, n_keys=300, out=P, offsets=P, ws=P, nbytes=BIG):
        return "key_order", lib.cldrd_key_order(keys, T, n_keys, out, offsets, ws, nbytes, None)

    def seg(rows_=P, order_=P, offsets=P, T=16, d=128, n_keys=300, out=P):
        return "segment_sum_rows", lib.cldrd_segment_sum_rows(rows_, order_, offsets, T, d, n_keys, out, 0, None)

    cases = [
        lambda: rows(T=0), lambda: rows(T=-4), lambda: rows(d=0), lambda: rows(d=130), lambda: rows(d=1028), lambda: rows(L=0),
        lambda: rows(fmt=3), lambda: rows(fmt=-1), lambda: rows(fmt=0, branch=P), lambda: rows(dx=None), lambda: rows(dy=None),
        lambda: rows(ids=None), lambda: rows(vocab=0),
        lambda: order(keys=None), lambda: order(out=None), lambda: order(offsets=None), lambda: order(T=0), lambda: order(T=-1),
        lambda: order(T=(1 << 22) + 1), lambda: order(n_keys=0), lambda: order(n_keys=-3), lambda: order(n_keys=(1 << 20) + 1),
        lambda: order(ws=None), lambda: order(nbytes=16),
        lambda: seg(rows_=None), lambda: seg(out=None), lambda: seg(T=0), lambda: seg(T=-1), lambda: seg(n_keys=0), lambda: seg(n_keys=-1),
        lambda: seg(d=0), lambda: seg(d=6), lambda: seg(d=1028),
        lambda: seg(order_=None, offsets=P),                      # offsets without order
        lambda: seg(order_=P, offsets=None),
    ]
    for i, case in enumerate(cases):
        lib.cldrd_set_tuning(None, 0)       # leaves "set_tuning: null key" behind: the message read below is this case's own
        op, rc = case()
        msg = lib.cldrd_last_error().decode()
        assert rc != 0, f"case {i} ({op}) was not rejected"
        assert msg.startswith(op + ":") and len(msg) > len(op) + 2, f"case {i}: {msg!r}"
        assert "CLDRD_" not in msg
    assert lib.cldrd_key_order_workspace(0, 10) == 0 and lib.cldrd_key_order_workspace(10, 0) == 0
    assert lib.cldrd_key_order_workspace((1 << 22) + 1, 10) == 0
    # three int32 arrays of T entries + one 256-bin histogram per tile of 1024 entries
    assert lib.cldrd_key_order_workspace(4099, 30522) == 4 * (3 * 4099 + 256 * 5)


def test_existing_embedding_backward_keeps_its_messages():
    from cldrd_amd import _lib
    lib = _lib.load()
    P = 64
    lib.cldrd_set_tuning(None, 0)
    rc = lib.cldrd_embed_ln_bwd(P, P, P, P, None, P, P, P, P, P, None, None, None, P, 16, 8, 128, 300, 0.0, 7, 0, None, 3, 0, None, None)
    assert rc != 0 and lib.cldrd_last_error().decode().startswith("embed_ln_bwd: grad_fmt")


def test_segment_chunk_mirrors_the_header():
    from cldrd_amd import hip_ops as ops
    text = open(os.path.join(ROOT, "include", "cldrd_hip.h")).read()
    m = re.search(r"^#define\s+CLDRD_SEGMENT_CHUNK\s+(\d+)\s*$", text, flags=re.M)
    assert m is not None
    assert ops.SEGMENT_CHUNK == int(m.group(1)) and ops.SEGMENT_CHUNK > 1


def test_python_wrappers_check_before_they_launch():
    from cldrd_amd import hip_ops as ops
    with pytest.raises(RuntimeError):
        ops.key_order(torch.zeros(8, dtype=torch.int64), 4)                       # CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        ops.segment_sum_rows(torch.zeros(8, 4), None, None, torch.zeros(2, 4))


def test_deterministic_flag_reaches_the_trainer_and_its_towers(monkeypatch):
    from cldrd_amd.trainer import nway_listwise as TL
    from cldrd_amd.encoder import tiny_config
    from cldrd_amd.models import NwayDualEncoder
    base = ["--experiment_folder", "x", "--synthetic_steps", "2"]
    assert TL.get_args(base).deterministic is False
    assert TL.get_args(base + ["--deterministic"]).deterministic is True
    import test_encoder_dryrun as D
    D._install_stubs(monkeypatch)           # a trainer on CPU tensors: no launch, no shadow casts
    monkeypatch.setattr(TL.NwayTrainer, "_require_gpu", staticmethod(lambda dev: None))
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: None)
    for share in (False, True):
        model = NwayDualEncoder(tiny_config(), share_weights=share)
        assert all(t.deterministic_embed is False for t in model.towers())
        assert TL.NwayTrainer(model, loss="kl_div").deterministic is False
        assert all(t.deterministic_embed is False for t in model.towers())
        tr = TL.NwayTrainer(model, loss="kl_div", deterministic=True)
        assert tr.deterministic is True and all(t.deterministic_embed is True for t in model.towers())
    # the command line hands the flag to the constructor
    seen = {}

    class Stop(Exception):
        pass

    def ctor(self, model, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(TL.NwayTrainer, "__init__", ctor)
    for flag in ([], ["--deterministic"]):
        args = TL.get_args(base + ["--synthetic_model", "tiny", "--loader_workers", "0"] + flag)
        args.device, args.distributed, args.rank = torch.device("cpu"), False, 0
        seen.clear()
        with pytest.raises(Stop):
            TL.train(args)
        assert seen["deterministic"] is bool(flag)
    tool = open(os.path.join(ROOT, "tools", "time_train_cli.py")).read()
    assert '["--deterministic"] if det else []' in tool          # the timing tool passes its own --deterministic through


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_stubbed_backward_walks_the_deterministic_launches(monkeypatch, packed, amp):
    """With every launch stubbed (tests/test_encoder_dryrun.py), the tower's backward issues the rows kernel and the two table sums where the
    default path issues cldrd_embed_ln_bwd - and the default path, mode off, issues none of the new launches."""
    import test_encoder_dryrun as D
    from cldrd_amd.encoder import HipEncoder
    calls = D._install_stubs(monkeypatch)
    monkeypatch.setenv("CLDRD_AMP", amp)
    seen = {}
    for det in (False, True):
        del calls[:]
        enc = HipEncoder(D.cfg_of("distilbert", 2), seed=3).train()
        enc.deterministic_embed = det
        M, L = 6, 16
        ids = torch.randint(0, 100, (M, L))
        mask = torch.ones(M, L, dtype=torch.int64)
        lens = None
        if packed:
            lens = [3, 16, 5, 2, 9, 4]
            for m, n in enumerate(lens):
                mask[m, n:] = 0
        cls, tape = enc.encode(ids, mask, train=True, save=True, seed=5, lengths=lens)
        assert (tape.pack is not None) == packed
        enc.backward_from_cls(tape, torch.zeros_like(cls))
        seen[det] = list(calls)
    new = {"cldrd_key_order", "cldrd_embed_ln_bwd_rows", "cldrd_segment_sum_rows"}
    assert not new & set(seen[False]) and "cldrd_embed_ln_bwd" in seen[False]
    on = seen[True]
    assert "cldrd_embed_ln_bwd" not in on
    assert on.count("cldrd_key_order") == (2 if packed else 1)
    i = on.index("cldrd_embed_ln_bwd_rows")
    assert on[i + 1:i + 3] == ["cldrd_segment_sum_rows", "cldrd_segment_sum_rows"] and on.count("cldrd_segment_sum_rows") == 2
    strip = lambda seq: [c for c in seq if c not in new and c != "cldrd_embed_ln_bwd"]
    assert strip(on) == strip(seen[False])          # nothing else moves
