#!/usr/bin/env python3
"""Golden values + gradients of ``rank(y_pred, y_true) + alpha * kd(y_pred[:, :Nt], teacher)`` from the reference's own losses
(build container only; IMPORTS THE REFERENCE: ``losses.KLDiv``, ``losses.MarginMSE``, ``losses.lambda_mrr_loss``,
``losses.ranknet_loss``, fp32 on the CPU, gradients by autograd) -> ``distill_losses.npz``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_distill_golden.py

Cases: shapes (B, Np, Nt) x kd {kl_div, margin_mse} x T {1, 2, 0.5} x rank {lambda_mrr, ranknet, none}; ``Np > Nt`` are the in-batch
shapes of models/nway_dual_encoder.py:30-44 (a row's own Nt passages first, then the other samples' with the label -0.5 and no teacher
score).  Student scores at dot-product scale (mean 100, sd 5), teacher scores at cross-encoder scale (normal, sd 4).  The file holds
y_pred, y_true and teacher once per shape (``<B>x<Np>x<Nt>/...``: every case of a shape shares them) and per case alpha, T, value (the
total), kd (the unweighted term) and grad (d value / d y_pred), plus value64 / kd64 from a float64 run of the reference; that run also
gives the reference's own fp32 rounding, printed per case (gradient too) and in total.  Only arrays are written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import cldrd_amd.synthetic as syn  # noqa: E402

SHAPES = [(8, 30, 30), (2, 200, 200), (4, 120, 30), (8, 60, 30), (1, 7, 3)]
KDS = ("kl_div", "margin_mse")
TS = (1.0, 2.0, 0.5)
RANKS = ("lambda_mrr", "ranknet", "none")
ALPHAS = (0.5, 1.0, 2.0)


def import_reference():
    import transformers  # noqa: F401
    sys.modules["transformers"].AdamW = torch.optim.AdamW        # imported (unused) by the reference's models package
    sys.path.insert(0, REF)
    import losses as ref_losses
    return ref_losses


def total(ref, rank, kd, y_pred, y_true, teacher, alpha, T, dtype):
    yp = torch.tensor(y_pred, dtype=dtype).requires_grad_(True)
    yt, te = torch.tensor(y_true, dtype=dtype), torch.tensor(teacher, dtype=dtype)
    Nt = te.shape[1]
    crit = ref.KLDiv(T) if kd == "kl_div" else ref.MarginMSE()
    term = crit(yp[:, :Nt], te)
    out = alpha * term
    if rank == "lambda_mrr":
        out = ref.lambda_mrr_loss(yp, yt) + out
    elif rank == "ranknet":
        out = ref.ranknet_loss(yp, yt) + out
    out.backward()
    return float(out.item()), float(term.item()), yp.grad.numpy()


def main():
    ref = import_reference()
    blob, names = {}, []
    worst_v = worst_g = 0.0
    n = 0
    for (B, Np, Nt) in SHAPES:
        seed = 100000 + 1000 * B + Np + Nt
        y_pred = (syn.normal(seed, B * Np).reshape(B, Np) * 5.0 + 100.0).astype(np.float32)
        teacher = (syn.normal(seed + 1, B * Nt).reshape(B, Nt) * 4.0).astype(np.float32)
        y_true = np.concatenate([syn.labels_mode9(B, Nt), np.full((B, Np - Nt), -0.5, np.float32)], axis=1)
        shape = f"{B}x{Np}x{Nt}"
        blob[shape + "/y_pred"], blob[shape + "/y_true"], blob[shape + "/teacher"] = y_pred, y_true, teacher
        for kd in KDS:
            for T in TS:
                for rank in RANKS:
                    alpha = ALPHAS[n % 3]
                    n += 1
                    name = f"{shape}.{kd}.T{T}.{rank}"
                    v, k, g = total(ref, rank, kd, y_pred, y_true, teacher, alpha, T, torch.float32)
                    v64, k64, g64 = total(ref, rank, kd, y_pred, y_true, teacher, alpha, T, torch.float64)
                    names.append(name)
                    for key, val in (("alpha", np.float64(alpha)), ("T", np.float64(T)), ("value", np.float64(v)), ("kd", np.float64(k)),
                                     ("grad", g.astype(np.float32)), ("value64", np.float64(v64)), ("kd64", np.float64(k64))):
                        blob[f"{name}/{key}"] = np.asarray(val)
                    ev = abs(v - v64) / abs(v64)
                    eg = float(np.abs(g - g64).max() / np.abs(g64).max())
                    worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
                    print(f"  {name:40s} alpha={alpha} value={v:.6f} kd={k:.6f}  fp32 vs fp64: value {ev:.1e}, grad {eg:.1e} of max|grad|")
    blob["names"] = np.array(names)
    out = os.path.join(HERE, "distill_losses.npz")
    np.savez_compressed(out, **blob)
    print(f"{len(names)} cases -> {out} ({os.path.getsize(out)} bytes); the reference's fp32 against its fp64: value {worst_v:.1e} relative, "
          f"gradient {worst_g:.1e} of max|grad|")


if __name__ == "__main__":
    main()
