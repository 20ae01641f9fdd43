#!/usr/bin/env python3
"""Host cost of NwayTrainer.train_step's Python: every launch stubbed and torch.cuda's streams faked (as tests/test_encoder_dryrun.py does), a
3-layer model of width 128 on the CPU, no GPU needed.  Prints median, 10th percentile and minimum microseconds of one eager step on a padded
and on a packed batch (B = 2, N = 3, Lq = 6, L = 20), 1500 repetitions each.  With FILE - another copy of trainer/nway_listwise.py, a parent
commit's, say - both trainers are built in this process and their steps alternated, so the load of a shared machine falls on both alike:

    python tools/time_trainer_host.py [FILE]
"""
import contextlib
import importlib.util
import os
import statistics
import sys
import time

sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import torch  # noqa: E402

import cldrd_amd.synthetic as syn  # noqa: E402
from cldrd_amd import _lib, hip_ops as ops  # noqa: E402
from cldrd_amd.encoder import EncoderConfig, HipEncoder  # noqa: E402
from cldrd_amd.models import NwayDualEncoder  # noqa: E402
from cldrd_amd.trainer import nway_listwise as TL  # noqa: E402

MODULES = {"package": TL}
if len(sys.argv) > 1:
    spec = importlib.util.spec_from_file_location("cldrd_amd.trainer._timed_other", sys.argv[1])
    MODULES["file"] = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = MODULES["file"]
    spec.loader.exec_module(MODULES["file"])
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


class Stream:
    cuda_stream = 0

    def wait_stream(self, s):
        pass

    def wait_event(self, e):
        pass


class Event:
    def record(self, stream=None):
        pass


MAIN = Stream()
ops._chk = chk
ops.call = lambda name, *a: None
ops._stream = lambda: 0
HipEncoder.refresh_shadows = shadows
HipEncoder._shadows_ok = lambda self, need_t, need_h=True: self.flat_h is not None
for mod in MODULES.values():
    mod.NwayTrainer._require_gpu = staticmethod(lambda dev: None)
torch.cuda.current_stream = lambda *a, **k: MAIN
torch.cuda.stream = lambda s: contextlib.nullcontext()
torch.cuda.Stream = lambda *a, **k: Stream()
torch.cuda.Event = lambda *a, **k: Event()
torch.cuda.is_current_stream_capturing = lambda: False
torch.Tensor.record_stream = lambda self, s: None
os.environ["CLDRD_GRAPH"] = "0"
os.environ["CLDRD_AMP"] = "fp16"
torch.set_num_threads(1)

cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=3, max_position_embeddings=64,
                    dropout=0.1, attention_dropout=0.1)


def trainer(mod):
    tr = mod.NwayTrainer(NwayDualEncoder(cfg, share_weights=False), loss="kl_div")
    tr.q_stream, tr.l_stream = Stream(), Stream()
    return tr


def batch(packed):
    b = syn.nway_batch(5, 2, 3, 6, 20, vocab=512, ragged=False, label_kind="teacher")
    if packed:
        nw = b["nway_passages"]
        mask = (torch.arange(20)[None, :] < torch.tensor([20, 3, 10, 17, 5, 8])[:, None]).long().view(2, 3, 20)
        nw["attention_mask"], nw["input_ids"] = mask, nw["input_ids"] * mask
    return TL.batch_to_device(b, torch.device("cpu"))


trainers = {name: trainer(mod) for name, mod in MODULES.items()}
for packed in (False, True):
    b = batch(packed)
    times = {name: [] for name in trainers}
    for tr in trainers.values():
        for _ in range(30):
            tr.train_step(b)
    for i in range(1500):
        for name, tr in (list(trainers.items())[::-1] if i % 2 else trainers.items()):
            t0 = time.perf_counter()
            tr.train_step(b)
            times[name].append(time.perf_counter() - t0)
    for name, ts in times.items():
        ts.sort()
        print("%-7s %-7s median %.1f  p10 %.1f  min %.1f us" % ("packed" if packed else "padded", name, statistics.median(ts) * 1e6,
                                                               ts[len(ts) // 10] * 1e6, ts[0] * 1e6))
