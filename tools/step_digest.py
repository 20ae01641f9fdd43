#!/usr/bin/env python3
"""Digest of what the training step (trainer.NwayTrainer) computes, for comparing two versions of its host code bit for bit: twelve
deterministic steps (``deterministic=True``, fixed seeds, dropout on) of a 2-layer width-128 model at B = 3, N = 4, Lq = 8, L = 16 per case -

    fp16 mode, padded batches (captured at step 4, replayed from then on)     fp16 mode, packed batches (every step eager)
    bf16 mode, padded batches                                                 fp16 mode, padded batches, distill="kl_div"

- and one line per case with the SHA-256 of ``flat_p``, ``m``, ``v``, the twelve {loss, pair count} words and ``_scale_state``.  The kernels
are the library's either way; ``--trainer-file`` runs another copy of ``trainer/nway_listwise.py`` (a parent commit's, say) inside this
package, so the two outputs must be equal line for line.  ``--resume_at K`` interrupts every case after step K: the trainer's ``state_dict()``
goes through ``torch.save``, a model built from another init seed under a fresh trainer loads it with ``load_state_dict(exact=True)`` and runs the
remaining steps (eager warm-up and a capture of its own); the lines must equal those of the run without the flag (profiles/resume_digest.txt).

    timeout -k 10 300 python tools/step_digest.py [--trainer-file FILE] [--resume_at K] [--out FILE]

One process, one GPU; not to be re-run after a fault before its cause is known."""
import argparse
import hashlib
import importlib.util
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cldrd_amd.synthetic as syn
import selftest
from cldrd_amd.encoder import EncoderConfig
from cldrd_amd.trainer import nway_listwise as TL

STEPS = 12
CASES = (("fp16 padded", "fp16", False, None), ("fp16 packed", "fp16", True, None), ("bf16 padded", "bf16", False, None),
         ("fp16 padded kl_div", "fp16", False, "kl_div"))


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def run(TL, name, amp, packed, distill, dev, resume_at=None):
    os.environ["CLDRD_AMP"] = amp                   # read when the towers are built
    cfg = EncoderConfig(arch="distilbert", vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=2, max_position_embeddings=64,
                        dropout=0.1, attention_dropout=0.1)

    def build(seed):
        model = selftest.build_tiny_model(cfg, seed=seed).to(dev).train()
        return model, TL.NwayTrainer(model, loss="kl_div", learning_rate=1e-3, warmup_steps=2, total_steps=40, distill=distill, distill_alpha=0.5,
                                     distill_T=2.0, deterministic=True)
    model, tr = build(3)
    assert tr.amp16 == (amp == "fp16")
    losses = []
    for i in range(STEPS):
        if i == resume_at:          # the job is killed here: its checkpoint, a file, is all that is left of it
            buf = io.BytesIO()
            torch.save(tr.state_dict(), buf)
            buf.seek(0)
            model, tr = build(4)
            tr.load_state_dict(torch.load(buf, map_location="cpu", weights_only=False), exact=True)
        batch = syn.nway_batch(4680 + i, 3, 4, 8, 16, vocab=cfg.vocab_size, ragged=False, label_kind="teacher",
                               with_teacher_scores=distill is not None)
        if packed:      # 4 .. 16 tokens per passage, another assignment every step: ~60 % token fill, the encoder packs it
            lens = 4 + (torch.arange(12) * 5 + i) % 13
            mask = (torch.arange(16)[None, :] < lens[:, None]).to(torch.int64).view(3, 4, 16)
            batch["nway_passages"]["attention_mask"] = mask
            batch["nway_passages"]["input_ids"] = batch["nway_passages"]["input_ids"] * mask
        batch = TL.batch_to_device(batch, dev)
        nw = batch["nway_passages"]
        assert model.passage_encoder.would_pack(nw["lengths"], 12, 16) == packed, "the batch is not of the layout this case is about"
        losses.append(tr.train_step(batch).clone())
    torch.cuda.synchronize()
    captured = sum(e["graph"] is not None for e in getattr(tr, "_graphs", {}).values())      # (older trainers: no attribute before a capture)
    warm = STEPS - (resume_at or 0) > tr._DDP_WARM       # (a trainer resumed within three steps of the end never gets to its capture)
    assert captured == (1 if warm and not packed else 0) and tr.global_step == STEPS, (captured, tr.global_step)
    scale = sha(tr._scale_state) if tr._scale_state is not None else "-"
    return (f"{name}: flat_p {sha(tr.flat_p)} m {sha(tr.m)} v {sha(tr.v)} loss {sha(torch.stack(losses))} scale_state {scale} "
            f"graphs {captured} loss[-1] {float(losses[-1][0]):.6f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--trainer-file", default=None, help="another copy of trainer/nway_listwise.py to run in place of the package's")
    ap.add_argument("--resume_at", default=None, type=int, help="save after this many steps and go on from the checkpoint with a fresh model and trainer")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mod = TL
    if args.trainer_file:
        spec = importlib.util.spec_from_file_location("cldrd_amd.trainer._digest_other", args.trainer_file)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for case in CASES:
        lines.append(run(mod, *case, dev, resume_at=args.resume_at))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
