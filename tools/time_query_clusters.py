"""Time of the k-means behind topic-aware batches at MS MARCO size: a synthetic mixture of 503 000 x 768 points, k = 2000, one MI355X.

    python tools/time_query_clusters.py [--out profiles/query_clusters_timing.txt] [--n 503000] [--k 2000] [--d 768] [--rounds 5] [--timeout 420]

A record, not a bar.  Reported: ms per assign launch (cldrd_kmeans_assign) and per update (key order + segment sum + finish), the achieved
TFLOP/s of the assign launch (2 n k d FLOP) next to the f32 matrix peak, and seconds for cluster.kmeans with 20 rounds.  Baseline, in
ALTERNATED rounds of the same process: the assignment as chunked ``torch.addmm`` (-h + X C^T, fp32 matmul, no reduced-precision mode) +
``argmax``, the update as ``index_add_`` + a division.  Also the share of points both assignments agree on.  The measuring child runs
under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MATRIX_PEAK = 157.3e12
CHUNK = 32768          # rows per addmm of the baseline: a [32768, 2000] fp32 score block is 262 MB


def child(n, k, d, rounds):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    from cldrd_amd import hip_ops as ops
    from cldrd_amd.cluster import kmeans
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centres = torch.randn(k, d, device=dev, generator=g)
    x = torch.empty(n, d, device=dev)
    for lo in range(0, n, CHUNK):          # the mixture: a centre drawn per point, unit Gaussian noise of the centres' own scale
        hi = min(n, lo + CHUNK)
        lab = torch.randint(0, k, (hi - lo,), device=dev, generator=g)
        x[lo:hi] = centres[lab] + torch.randn(hi - lo, d, device=dev, generator=g)
    c = x[torch.randperm(n, device=dev, generator=g)[:k]].contiguous()
    h = ops.kmeans_half_sqnorm(c)

    def ours_assign():
        return ops.kmeans_assign(x, c, h)

    def torch_assign():
        out = torch.empty(n, dtype=torch.int64, device=dev)
        ct = c.t().contiguous()
        for lo in range(0, n, CHUNK):
            hi = min(n, lo + CHUNK)
            out[lo:hi] = torch.addmm(-h, x[lo:hi], ct).argmax(1)
        return out

    def ours_update(a, cc):
        return ops.kmeans_update(x, a, cc)

    def torch_update(a, cc):
        sums = torch.zeros(k, d, device=dev).index_add_(0, a, x)
        m = torch.bincount(a, minlength=k)
        cc.copy_(torch.where(m[:, None] > 0, sums / m.clamp(min=1)[:, None].float(), cc))

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    a_ours, a_torch = ours_assign(), torch_assign()          # warm-up: code objects, allocator, BLAS plans
    ours_update(a_ours, c.clone()), torch_update(a_ours, c.clone())
    res = {"assign_ours_ms": [], "assign_torch_ms": [], "update_ours_ms": [], "update_torch_ms": []}
    for _ in range(rounds):
        res["assign_ours_ms"].append(timed(ours_assign)[0])
        res["assign_torch_ms"].append(timed(torch_assign)[0])
        res["update_ours_ms"].append(timed(ours_update, a_ours, c.clone())[0])
        res["update_torch_ms"].append(timed(torch_update, a_ours, c.clone())[0])
    res["equal_share"] = float((a_ours == a_torch).double().mean())
    t20, r = timed(lambda: kmeans(x, k, iters=20, seed=0))
    res["kmeans20_s"] = t20 / 1e3
    res["moved"] = r.moved.cpu().tolist()
    res["n_empty"] = int(r.n_empty.item())
    res.update(n=n, k=k, d=d)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_clusters_timing.txt"))
    ap.add_argument("--n", type=int, default=503000)
    ap.add_argument("--k", type=int, default=2000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.n, args.k, args.d, args.rounds)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--k", str(args.k), "--d", str(args.d),
                        "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:          # a failed step ends the run: nothing else is started on the GPU
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed (exit status {r.returncode})")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    flop = 2.0 * res["n"] * res["k"] * res["d"]

    def row(name, v):
        return f"{name:<24}" + " ".join(f"{t:9.2f}" for t in v) + f"   min {min(v):9.2f}  max {max(v):9.2f}"
    lo = min(res["assign_ours_ms"])
    lines = [f"k-means of {res['n']} x {res['d']} synthetic mixture points, k = {res['k']}, one MI355X; {args.rounds} alternated rounds, ms per call "
             "(tools/time_query_clusters.py)",
             row("assign, this library", res["assign_ours_ms"]), row("assign, addmm + argmax", res["assign_torch_ms"]),
             row("update, this library", res["update_ours_ms"]), row("update, index_add_", res["update_torch_ms"]),
             f"assign launch: {flop / 1e12:.2f} TFLOP, best {lo:.2f} ms = {flop / lo / 1e9:.1f} TFLOP/s = {100 * flop / lo / 1e9 / (F32_MATRIX_PEAK / 1e12):.1f} % "
             "of the f32 matrix peak",
             f"assign, this library / torch (best of each): {lo / min(res['assign_torch_ms']):.3f}",
             f"equal assignments (this library vs addmm + argmax): {100 * res['equal_share']:.4f} %",
             f"cluster.kmeans, 20 rounds + final assign: {res['kmeans20_s']:.2f} s; moved per round {res['moved']}; empty clusters in the last update {res['n_empty']}"]
    print("\n".join(lines))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
