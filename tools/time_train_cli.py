#!/usr/bin/env python3
"""The TRAINING command line as a job (the analogue of tools/time_cfg5_full.py for `python -m cldrd_amd.trainer.nway_listwise`): cfg2-shaped synthetic
batches (DistilBERT x2, N = 32, per-GPU batch 8, passages of up to 128 tokens, queries 30) through `train(args)` - the loader's worker processes,
batch_to_device, train_step, logging every 50 steps - and the wall clock per step after the warm-up, next to bench.py's resident-batch number.
The host's share of a step is split three ways: waiting for the loader, batch_to_device, train_step (enqueue only: nothing here waits for the GPU
except through the queue depth).

    python tools/time_train_cli.py [steps=400] [--fixed] [--workers N] [--profile] [--ddp1] [--loss KIND] [--distill_loss KIND] [--deterministic]
                                   [--weighing_scheme S] [--lambda_k K] [--lambda_sigma X] [--lambda_mu X] [--lambda_gain G] [--lambda_log L]
                                   [--label_source rank|teacher] [--neg_score_mode M] [--teacher_label_shift S]
                                   [--apply_consine_similarity [--cosine_scale X]]
                                   [--ce_temperature X] [--ce_pos_min X] [--ce_neg_max X] [--in_batch_loss [--all_in_batch_neg]]
        --fixed: every passage 128 tokens (the bench's headline batch: one shape, replayed as a HIP graph); default: MS MARCO-shaped lengths
        --loss: the trainer's --loss (default here: kl_div, the bench's); with lambda_loss the lambda / label flags above are passed through too
        --distill_loss kl_div | margin_mse: passed through to the trainer (the synthetic loader then adds teacher_scores to every batch)
        --ce_temperature, --ce_pos_min, --ce_neg_max: passed through to the trainer with --loss softmax_ce (cldrd_softmax_ce on the loss stream);
                 --in_batch_loss, --all_in_batch_neg: passed through (the [B, B*N] / [B, 2N] logit matrices)
        --apply_consine_similarity, --cosine_scale: passed through to the trainer (the cosine scorer on the loss stream)
        --deterministic: passed through to the trainer (embedding-table gradients as fixed-order sums instead of float atomics)
        --ddp1:  the data-parallel code path (bucket hooks, RCCL all-reduces, agreement step) with a process group of ONE rank (CLDRD_FORCE_DDP=1)
"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ddp1 = "--ddp1" in sys.argv
if ddp1:
    os.environ.update({"CLDRD_FORCE_DDP": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": os.environ.get("MASTER_PORT", "29533"), "RANK": "0",
                       "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
import torch
from cldrd_amd.trainer import nway_listwise as T

steps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 400)
fixed = "--fixed" in sys.argv
workers = int(sys.argv[sys.argv.index("--workers") + 1]) if "--workers" in sys.argv else 4
distill = sys.argv[sys.argv.index("--distill_loss") + 1] if "--distill_loss" in sys.argv else None
loss = sys.argv[sys.argv.index("--loss") + 1] if "--loss" in sys.argv else "kl_div"
passed = [a for f in ("--weighing_scheme", "--lambda_k", "--lambda_sigma", "--lambda_mu", "--lambda_gain", "--lambda_log", "--label_source",
                      "--neg_score_mode", "--teacher_label_shift", "--cosine_scale", "--ce_temperature", "--ce_pos_min", "--ce_neg_max") if f in sys.argv for a in (f, sys.argv[sys.argv.index(f) + 1])] \
    + [f for f in ("--apply_consine_similarity", "--in_batch_loss", "--all_in_batch_neg") if f in sys.argv]
det = "--deterministic" in sys.argv
with tempfile.TemporaryDirectory(dir="/tmp") as td:
    argv = ["--experiment_folder", td, "--run_folder", "run", "--synthetic_steps", str(steps), "--synthetic_model", "distilbert", "--synthetic_nway", "32",
            "--passage_max_len", "128", "--query_max_len", "30", "--train_batch_size", "8", "--logging_steps", "50", "--evaluate_steps", "1000000",
            "--num_train_epochs", "1", "--loss", loss, "--label_mode", "9", "--loader_workers", str(workers)] + (["--synthetic_fixed"] if fixed else []) \
        + (["--local_rank", "0"] if ddp1 else []) + (["--distill_loss", distill] if distill else []) \
        + (["--deterministic"] if det else []) + passed
    args = T.set_env(T.get_args(argv))
    stamps, spent = [], {"batch_to_device": 0.0, "train_step": 0.0}
    real_step, real_move = T.NwayTrainer.train_step, T.batch_to_device
    warm = 20

    def timed_step(self, batch):
        t = time.perf_counter()
        out = real_step(self, batch)
        now = time.perf_counter()
        if len(stamps) >= warm:
            spent["train_step"] += now - t
        stamps.append(now)
        return out

    def timed_move(batch, dev):
        t = time.perf_counter()
        out = real_move(batch, dev)
        if len(stamps) >= warm:
            spent["batch_to_device"] += time.perf_counter() - t
        return out
    T.NwayTrainer.train_step, T.batch_to_device = timed_step, timed_move
    t0 = time.perf_counter()
    if "--profile" in sys.argv:
        import cProfile, pstats
        pr = cProfile.Profile()
        tr = pr.runcall(T.train, args)
        pstats.Stats(pr).sort_stats("tottime").print_stats(22)
    else:
        tr = T.train(args)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n = len(stamps) - 1 - warm
    per = (stamps[-1] - stamps[warm]) / n
    mv, st = spent["batch_to_device"] / (n + 1), spent["train_step"] / (n + 1)
    print(f"trainer CLI loop{f' (--loss {loss})' if loss != 'kl_div' else ''}{' (' + ' '.join(passed) + ')' if passed else ''}{f' (--distill_loss {distill})' if distill else ''}{' (--deterministic)' if det else ''}{' (data-parallel path, one rank over RCCL)' if ddp1 else ''}, {'fixed-length' if fixed else 'MSMARCO-shaped'} cfg2 batches, {workers} loader workers, {torch.get_num_threads()} torch host threads: "
          f"{steps} steps in {t1 - t0:.1f} s; steady state {1e3 * per:.3f} ms per step = {8 / per:.1f} samples/s (clock between train_step returns, steps "
          f"{warm}..{len(stamps) - 1}); host per step: batch_to_device {1e3 * mv:.2f} ms, train_step enqueue {1e3 * st:.2f} ms, loader wait + logging "
          f"{1e3 * (per - mv - st):.2f} ms; graph replay: {any(e['graph'] is not None for e in getattr(tr, '_graphs', {}).values())}; final global_step {tr.global_step}")
