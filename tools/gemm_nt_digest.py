#!/usr/bin/env python3
"""Digest of what the 16-bit NT GEMM (hip_ops.gemm_nt) and the top-k scan (hip_ops.topk_scan_filter) compute, for comparing two commits bit for
bit: fixed seeds, the smallest shapes that reach each route of the host dispatch (64 x 64 one launch, 64 x 64 split + finish, 128 x 128 one
pass, 128 x 128 split, the ring at 192- and 256-column tiles with a ragged last row tile, the ring's fp16 fall-back to the 128 x 128 kernel),
at each route every compiled epilogue flavour plus one that only the run-time-switched kernel serves, in each format the flavour exists in.
One line per case with the SHA-256 of every output (C, and the GELU tape where one is written).  The scan's three routes (streaming, ring
with the index rows as M, tiled 128 x 128) in both formats; candidate lists are sorted per query first, their order depends on atomics.
Only the public surface is used, so the same file runs on either commit (copy it there); the outputs must be equal line for line.

    timeout -k 10 300 python tools/gemm_nt_digest.py [--out FILE]

One process, one GPU; not to be re-run after a fault before its cause is known."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cldrd_amd import hip_ops as ops

DEV = torch.device("cuda", 0)
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
BIAS, PREACT, GELU, GELUGRAD, DROPOUT, RESIDUAL, OUT32, RES32, DGELU, RESLN = 1, 2, 4, 8, 16, 32, 64, 256, 1024, 2048
R32 = RESIDUAL | RES32 | OUT32
# the compiled flavour sets (csrc/gemm_epilogue.h), written out: this file must run on a commit that does not name them
BF16_SMALL = [0, BIAS, BIAS | PREACT | GELU, BIAS | PREACT | GELU | DGELU, GELUGRAD | DGELU, BIAS | RESIDUAL, BIAS | DROPOUT | RESIDUAL, GELUGRAD,
              RESIDUAL, OUT32, R32, BIAS | R32, BIAS | DROPOUT | R32, BIAS | R32 | RESLN, BIAS | DROPOUT | R32 | RESLN]
BF16_RING = BF16_SMALL + [BIAS | GELU]
F16_RING = [BIAS, BIAS | PREACT | GELU | DGELU, BIAS | GELU, BIAS | R32, BIAS | DROPOUT | R32, BIAS | R32 | RESLN, BIAS | DROPOUT | R32 | RESLN,
            0, GELUGRAD | DGELU, OUT32]
F16_SMALL = F16_RING + [R32]
GENERIC = [BIAS | OUT32, BIAS | GELU | RESIDUAL]           # in no bf16 list: the run-time-switched instantiation
LINES = []


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def emit(line):
    print(line, flush=True)
    LINES.append(line)


def operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    return {"A": r(M, K), "B": r(N, K, scale=0.05), "bias": r(N), "res": r(M, N), "tape": r(M, N), "mean": r(M, scale=0.1),
            "rstd": r(M).abs() + 0.5, "gamma": r(N), "beta": r(N)}


def run_gemm(tag, x, M, N, K, epi, operand_dt, out16_dt):
    """One gemm_nt call of flavour ``epi``: operands ``operand_dt``, a 16-bit C ``out16_dt``, the GELU tape in the operands' format."""
    kw = {}
    act = (1 if epi & GELU else 0) | (2 if epi & DGELU else 0)
    if epi & BIAS:
        kw["bias"] = x["bias"]
    if epi & RESIDUAL:
        kw["residual"] = x["res"] if epi & RES32 else x["res"].to(BF16)
    if epi & RESLN:
        kw["residual_ln"] = (x["mean"], x["rstd"], x["gamma"], x["beta"])
    if epi & DROPOUT:
        kw.update(dropout_p=0.1, seed=20231)
    pre = None
    if epi & PREACT:
        pre = kw["preact"] = torch.full((M, N), 7.0, device=DEV, dtype=operand_dt)
    if epi & GELUGRAD:
        kw["gelu_pre"] = x["tape"].to(operand_dt)
    out = torch.full((M, N), 7.0, device=DEV, dtype=F32 if epi & OUT32 else out16_dt)
    ops.gemm_nt(x["A"].to(operand_dt), x["B"].to(operand_dt), out, act=act, **kw)
    torch.cuda.synchronize()
    fmt = "bf16" if operand_dt == BF16 else ("fp16" if out16_dt == F16 else "fp16->bf16")
    emit(f"{tag} {M}x{N}x{K} {fmt}{'+tape' if pre is not None or epi & GELUGRAD else ''} epi {epi}: C {sha(out)}" + (f" preact {sha(pre)}" if pre is not None else ""))


def run_route(tag, shape, seed, bf16_list, f16_list):
    M, N, K = shape
    x = operands(M, N, K, seed)
    for epi in bf16_list + GENERIC:
        run_gemm(tag, x, M, N, K, epi, BF16, BF16)
    for epi in f16_list:
        run_gemm(tag, x, M, N, K, epi, F16, F16)
        if not epi & (OUT32 | PREACT | GELUGRAD):          # a 16-bit C without a tape also exists as fp16 operands, bf16 C
            run_gemm(tag, x, M, N, K, epi, F16, BF16)


def run_scan(tag, nq, rows, d, tiled, seed):
    g = torch.Generator().manual_seed(seed)
    Q32, P32 = torch.randn(nq, d, generator=g).to(DEV), torch.randn(rows, d, generator=g).to(DEV)
    cap = 512
    for dt in (BF16, F16):
        thr = torch.full((nq,), 2.2 * d ** 0.5, device=DEV)        # ~1.4 % of the rows of a query pass
        counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
        cand_rows = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
        cand_scores = torch.zeros(nq, cap, device=DEV)
        ops.topk_scan_filter(Q32.to(dt).contiguous(), P32.to(dt).contiguous(), thr, counts, cand_rows, cand_scores, tiled=tiled)
        torch.cuda.synchronize()
        c, r, s = counts.cpu().numpy(), cand_rows.cpu().numpy(), cand_scores.cpu().numpy()
        h = hashlib.sha256(c.tobytes())
        assert int(c[:nq].max()) <= cap and int(c[:nq].sum()) > 0, "digest shapes keep every hit and have some"
        for q in range(nq):
            order = np.argsort(r[q, :c[q]], kind="stable")
            h.update(r[q, :c[q]][order].tobytes())
            h.update(s[q, :c[q]][order].tobytes())
        emit(f"{tag} nq{nq} rows{rows} d{d} {'bf16' if dt == BF16 else 'fp16'}: hits {int(c[:nq].sum())} lists {h.hexdigest()[:16]}")


def tuned(key, value, fn, *a):
    ops.set_tuning(key, value)
    try:
        fn(*a)
    finally:
        ops.set_tuning(key, {"gemm_nt64": 1, "gemm_splitk": 0}[key])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    run_route("1 64x64 one launch", (70, 72, 128), 1, BF16_RING, F16_SMALL)
    run_route("2 64x64 split + finish", (256, 768, 2304), 2, BF16_RING, F16_SMALL)
    tuned("gemm_nt64", 0, run_route, "3 128x128 one pass", (130, 136, 64), 3, BF16_SMALL, F16_SMALL)
    tuned("gemm_splitk", 3, run_route, "4 128x128 split", (130, 136, 512), 4, BF16_SMALL, F16_SMALL)
    for i, N in enumerate((192, 256, 768)):
        run_route(f"5 ring N={N}", (1025, N, 64), 5 + i, BF16_RING, F16_RING)
    x = operands(1025, 192, 64, 8)
    run_gemm("6 ring16 declines -> 128x128", x, 1025, 192, 64, R32, F16, F16)
    run_scan("7 scan streaming", 40, 3000, 128, False, 9)
    run_scan("8 scan ring", 100, 5000, 128, True, 10)
    run_scan("9 scan tiled 128x128", 40, 3000, 128, True, 11)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
