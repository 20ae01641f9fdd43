"""Throughput of the exact fp32 evaluation pass (HipEncoder.encode(fp32=True)) next to the 16-bit evaluation pass: 4096 synthetic passages of
up to 128 tokens with MS MARCO-shaped lengths on the full-size DistilBERT, packed, in index-encode batches of 512.

    python tools/time_fp32_pass.py [--out profiles/fp32_pass_timing.txt] [--rows 4096] [--timeout 240]

A record, not a bar.  Each mode is measured by a child process of its own under a time limit (a step that hangs ends there and nothing
else is started); the parent never opens the GPU.  Host threads are capped at 16.  Reported: passages/s, tokens/s and, for the fp32 pass, the
achieved fraction of the 157.3 TFLOP/s f32 matrix peak of an MI355X, counting the FLOPs the pass really runs (real tokens only, CLS-only
last layer; the 32 x 32 score tiles of the attention kernel are counted as run, masked part included)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MATRIX_PEAK = 157.3e12


def pass_flops(lens, d, f, n_layers):
    """FLOPs of one evaluation pass over packed sequences of these lengths (GEMMs and attention contractions; 2 per multiply-add)."""
    T, M = int(sum(lens)), len(lens)
    full = 2 * T * (4 * d * d + 2 * d * f)                                    # QKV, out, FFN1, FFN2 per full layer
    att = sum(4 * d * 32 * ((n + 31) // 32) * 32 * ((n + 31) // 32) for n in lens)      # Q K^T and P V on 32 x 32 tiles, all heads
    last = 2 * T * 2 * d * d + 2 * M * (2 * d * d + 2 * d * f) + sum(4 * d * 32 * 32 * ((n + 31) // 32) for n in lens)
    return (n_layers - 1) * (full + att) + last


def child(mode, rows):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    from cldrd_amd.dataset.sequence_dataset import SyntheticSequenceDataset
    from cldrd_amd.encoder import EncoderConfig, HipEncoder
    cfg = EncoderConfig(dropout=0.0, attention_dropout=0.0)                   # distilbert-base-uncased's shape
    enc = HipEncoder(cfg, seed=3).cuda().eval()
    batches = []
    for b in SyntheticSequenceDataset(rows, 128).loader():
        ids, mask = b["seq"]["input_ids"], b["seq"]["attention_mask"]
        batches.append((ids.cuda(), mask.cuda(), mask.sum(1).tolist()))
    kw = dict(fp32=True) if mode == "fp32" else dict(fp16=False)

    def run():
        with torch.no_grad():
            for ids, mask, lens in batches:
                enc.encode(ids, mask, lengths=lens, **kw)
    run()                                                                    # warm-up: code objects, allocator, weight shadows
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    lens = [n for _, _, ln in batches for n in ln]
    print(json.dumps(dict(mode=mode, rows=rows, tokens=int(sum(lens)), seconds=best,
                          flops=pass_flops(lens, cfg.dim, cfg.hidden_dim, cfg.n_layers))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_pass_timing.txt"))
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measured mode")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.rows)
    lines = [f"fp32 evaluation pass vs 16-bit evaluation pass: {args.rows} synthetic passages, L <= 128, MS MARCO-shaped lengths, full-size DistilBERT, "
             "packed batches of 512, best of 3 sweeps (tools/time_fp32_pass.py)"]
    for mode in ("fp32", "16bit"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--rows", str(args.rows)], capture_output=True, text=True,
                           timeout=args.timeout)
        if r.returncode != 0:
            # a failed step ends the run: nothing else is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{mode}: the measurement failed (exit status {r.returncode})")
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        line = (f"{mode:>5}: {res['seconds'] * 1e3:9.1f} ms  {res['rows'] / res['seconds']:10.0f} passages/s  {res['tokens'] / res['seconds']:12.0f} tokens/s  "
                f"({res['tokens']} tokens, {res['flops'] / 1e12:.2f} TFLOP)")
        if mode == "fp32":
            line += f"  {res['flops'] / res['seconds'] / 1e12:.1f} TFLOP/s = {100 * res['flops'] / res['seconds'] / F32_MATRIX_PEAK:.1f} % of the f32 matrix peak"
        print(line)
        lines.append(line)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
