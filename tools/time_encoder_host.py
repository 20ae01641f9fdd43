#!/usr/bin/env python3
"""Host cost of the encoder tower's Python: every launch stubbed (as tests/test_encoder_dryrun.py does), a 6-layer tower of width 128 on the
CPU, no GPU needed.  Prints the median microseconds of one training forward + backward, one 16-bit evaluation pass and one fp32 evaluation
pass, 200 repetitions each.  ROOT (default: this checkout) is the tree whose package is timed - to compare two commits, check the other one
out somewhere, build it, and alternate the two:

    python tools/time_encoder_host.py [ROOT]
"""
import os
import statistics
import sys
import time

sys.dont_write_bytecode = True
sys.path[:0] = [sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import torch  # noqa: E402

from cldrd_amd import _lib, hip_ops as ops  # noqa: E402
from cldrd_amd.encoder import EncoderConfig, HipEncoder  # noqa: E402

_lib.load()


def chk(t, dtype, name, dim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(name)
    if t.dtype != dtype:
        raise TypeError(name)
    if dim is not None and t.dim() != dim:
        raise ValueError(name)
    if t.stride(-1) != 1:
        raise ValueError(name)
    return t


def shadows(enc, *a, **k):
    enc.flat_h = torch.zeros(enc.layout.total, dtype=torch.bfloat16)
    enc.flat_h16 = torch.zeros(enc.layout.total, dtype=torch.float16)
    enc.flat_t = torch.zeros(enc.layout.t_total, dtype=torch.float16 if enc.amp16 else torch.bfloat16)
    enc._t_fresh = True
    enc._shadow_version = enc.flat_p._version


ops._chk = chk
ops.call = lambda name, *a: None
ops._stream = lambda: 0
HipEncoder.refresh_shadows = shadows
HipEncoder._shadows_ok = lambda self, need_t, need_h=True: self.flat_h is not None
torch.set_num_threads(1)

cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=6, max_position_embeddings=64,
                    dropout=0.1, attention_dropout=0.1)
enc = HipEncoder(cfg, seed=1)
ids = torch.randint(3, 500, (8, 32))
mask = torch.ones(8, 32, dtype=torch.long)
dcls = torch.zeros(8, 128)


def train():
    cls, tape = enc.encode(ids, mask, train=True, save=True, seed=11)
    enc.backward_from_cls(tape, dcls, accumulate=False)


def evalp():
    enc.encode(ids, mask, train=False, seed=11)


def fp32p():
    enc.encode(ids, mask, fp32=True)


out = []
for fn in (train, evalp, fp32p):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    out.append(statistics.median(ts) * 1e6)
print("%.1f %.1f %.1f" % tuple(out))
