#!/usr/bin/env python3
"""Golden values + gradients for ``cldrd_lambda_term`` from the reference's ``lambda_loss`` (``losses/standard_lambda_rank.py``)
-> ``lambda_term.npz``.  Build container only: IMPORTS THE REFERENCE, whose checkout is the one argument.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lambda_term_golden.py /path/to/reference

The label transform of the entry point is applied HERE, in fp32 as include/cldrd_hip.h states it (mean of the columns n_rel.. as a
left-to-right sum and one division, then the row minimum, then the offset; padding is judged on the labels as given), and the
reference then runs in float64 on logits[:, :Ns] and the transformed labels: value and autograd gradient.

Cases (every one: fp32-representable inputs, a finite value, at least one pair):
  schemes   all 8 weighing schemes x {power, linear} gain x {natural, binary} log x {mean, sum}, k in {none, 1, 10}, sigma in {1, 2},
            B = 3, Ns = 30 (+5 columns behind the slate in half of them), -1 padding: a padded tail, a row with two live items, tied labels
  sizes     Ns in {2, 3, 30, 31, 255, 256, 257} (around the 256-thread workgroup) x B in {1, 3} x Np - Ns in {0, 5}
  teacher   labels that are teacher scores, no padding (pad indicator -inf): all four (mean, row_min) combinations on cross-encoder-like
            scores and on log-softmax-like scores that are all negative, with and without an offset
Ns = 1 is left out: the reference's mean over zero pairs is NaN.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:                 # (tests/test_gpu_lambda_term.py imports `transform` from here: leave its interpreter as it is)
    sys.path.insert(0, ROOT)
import cldrd_amd.synthetic as syn  # noqa: E402

SCHEMES = [None, "ndcgLoss1_scheme", "ndcgLoss2_scheme", "lambdaRank_scheme", "ndcgLoss2PP_scheme", "rankNet_scheme",
           "rankNetWeightedByGTDiff_scheme", "rankNetWeightedByGTDiffPowed_scheme"]
F32 = np.float32


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def transform(labels, pad, mean, row_min, n_rel, offset):
    """The label transform of cldrd_lambda_term in fp32."""
    out = labels.astype(F32).copy()
    B, Ns = out.shape
    for b in range(B):
        live = labels[b] != F32(pad)
        if mean:
            s, n = F32(0.0), 0
            for i in range(n_rel, Ns):
                if live[i]:
                    s = F32(s + out[b, i])
                    n += 1
            if n:
                tail = live & (np.arange(Ns) >= n_rel)
                out[b, tail] = F32(s / F32(n))
        if row_min and live.any():
            out[b, live] = (out[b, live] - out[b, live].min()).astype(F32)
        if offset != 0.0:
            out[b, live] = (out[b, live] + F32(offset)).astype(F32)
        assert not (out[b, live] == F32(pad)).any(), "a transformed label equals the padding indicator"
    return out


def rank_labels(seed, B, Ns, linear):
    """Graded labels with -1 padding: row 0 a padded tail, the last row two live items (B > 1), tied labels in between."""
    t = np.round(np.abs(syn.normal(seed, B * Ns).reshape(B, Ns)) * 1.5, 1)
    if linear:
        t = 1.0 + np.minimum(t, 3.0)              # gain = label - 1 >= 0
    t = t.astype(F32)
    if Ns >= 6:
        t[0, Ns - Ns // 4:] = -1.0
        t[B // 2, :3] = 2.0
        t[B // 2, Ns // 2] = -1.0
    if B > 1 and Ns >= 3 and not linear:           # (linear gain: a padded item counts -1 / discount in the reference's maxDCG, which
        t[B - 1, :] = -1.0                         # 28 of them would turn negative: clamped to eps, gains of 1e4 - not a case to pin)
        t[B - 1, 1], t[B - 1, Ns - 1] = 2.0, 0.5
    if Ns < 6:                                     # tiny slates: distinct live labels, so that every row has a pair
        t[0, :] = (1.0 + np.arange(Ns)[::-1]).astype(F32)
    return t


def teacher_labels(seed, B, Ns, negative):
    t = syn.normal(seed, B * Ns).reshape(B, Ns)
    t = -np.abs(t) * 3.0 - 0.05 if negative else t * 4.0 + 8.0
    return (-np.sort(-t, axis=1)).astype(F32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ll = load(os.path.join(sys.argv[1], "losses", "standard_lambda_rank.py"), "ref_ll")
    blob, meta = {}, {}

    def add(B, Ns, extra, labels, *, pad, scheme, k=None, sigma=1.0, mu=10.0, reduction="mean", log="natural", gain="power", mean=False,
            row_min=False, n_rel=None, offset=0.0):
        name = f"case{len(meta)}"
        Np = Ns + extra
        n_rel = Ns if n_rel is None else n_rel
        logits = (syn.normal(1000 + len(meta), B * Np).reshape(B, Np) * 2.0).astype(F32)
        lab = transform(labels, pad, mean, row_min, n_rel, offset)
        yp = torch.tensor(logits[:, :Ns].astype(np.float64)).requires_grad_(True)
        out = ll.lambda_loss(yp, torch.tensor(lab.astype(np.float64)), padded_value_indicator=float(pad), weighing_scheme=scheme, k=k,
                             sigma=sigma, mu=mu, reduction=reduction, reduction_log=log, gain=gain)
        out.backward()
        assert np.isfinite(out.item()) and np.isfinite(yp.grad.numpy()).all(), (name, out.item())
        blob[name + ".logits"], blob[name + ".labels"] = logits, labels.astype(F32)
        blob[name + ".value"], blob[name + ".grad"] = np.float64(out.item()), yp.grad.numpy()
        meta[name] = dict(pad=("-inf" if pad == -np.inf else float(pad)), weighing_scheme=scheme, k=k, sigma=sigma, mu=mu, reduction=reduction,
                          reduction_log=log, gain=gain, neg_mean=mean, row_min=row_min, n_rel=n_rel, label_offset=offset)

    n = 0
    for sch in SCHEMES:
        for gain, log, red in (("power", "natural", "mean"), ("power", "binary", "sum"), ("linear", "natural", "sum"),
                               ("linear", "binary", "mean")):
            k = (None, 1, 10)[n % 3]
            if k == 1 and red == "mean" and sch != "ndcgLoss1_scheme":
                k = 10                              # one position, no pair: the reference's mean is NaN
            add(3, 30, 5 * (n % 2), rank_labels(200 + n, 3, 30, gain == "linear"), pad=-1.0, scheme=sch, k=k, sigma=(1.0, 2.0)[(n // 2) % 2],
                mu=7.0, reduction=red, log=log, gain=gain)
            n += 1
    for Ns in (2, 3, 30, 31, 255, 256, 257):
        for B in (1, 3):
            for extra in (0, 5):
                sch = SCHEMES[n % 8]
                mean, row_min = bool(n & 1), bool(n & 2)
                add(B, Ns, extra, rank_labels(300 + n, B, Ns, False), pad=-1.0, scheme=sch, k=(None, 10)[(n // 2) % 2] if Ns > 3 and not (B == 1 and mean) else None,      # (one row, its ten all negatives: no pair)
                    sigma=(1.0, 2.0)[(n // 4) % 2], mean=mean, row_min=row_min, n_rel=min(10, Ns - 1))
                n += 1
    for negative in (False, True):
        for mean in (False, True):
            for row_min in (False, True):
                for sch in ("ndcgLoss1_scheme", "ndcgLoss2PP_scheme"):
                    add(3, 30, 5 * (n % 2), teacher_labels(400 + n, 3, 30, negative), pad=-np.inf, scheme=sch, k=(None, 10)[n % 2],
                        mean=mean, row_min=row_min, n_rel=10, offset=(0.0, 0.5)[(n // 2) % 2], log=("natural", "binary")[n % 2])
                    n += 1
    blob["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "lambda_term.npz"), **blob)
    vals = [float(blob[f"case{i}.value"]) for i in range(len(meta))]
    print("cases:", len(meta), "values min / max:", min(vals), max(vals), "zero values:", sum(v == 0.0 for v in vals))


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
