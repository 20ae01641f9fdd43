"""Curriculum training files from a teacher-scored run (dataset.curriculum_file): teacher order and its tie rules, the sampling contract
restated with Python integers, the file read back by NwayDataset, subset invariance, refusals, skipped queries, the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import cldrd_amd  # noqa: F401
from cldrd_amd.dataset import NwayDataset, labels_for_mode
from cldrd_amd.dataset import curriculum_file as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def sm64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, qid, pid):
    return sm64(sm64(sm64(seed & M64) ^ (qid & M64)) ^ (pid & M64))


def expected_sample(teacher, window, n, qid, seed):
    """n pids of teacher ranks window[0]..window[1] (1-based) with the smallest keys (ties by pid), in teacher order."""
    cand = teacher[window[0] - 1:window[1]]
    chosen = set(sorted(cand, key=lambda p: (key(seed, qid, p), p))[:n])
    return [p for p in cand if p in chosen]


# windows that fit 40 candidates: mode -> (most-hard window, semi-hard window)
WINDOWS = {"8": ((6, 22), (23, 40)), "9": ((11, 25), (26, 40)), "10": ((21, 30), (31, 40))}
QIDS = (503, 17, 90021)
RANK_TIES = ((3, 4, 5), (19, 20))        # teacher positions (0-based) with one score that only the rank column orders
LINE_TIES = ((9, 10),)                   # one score and one rank: only the line order decides


def hand_made_run(path, seed=0):
    """3 queries x 40 candidates, lines shuffled across queries.  Returns {qid: pids in the intended teacher order}.  The rank column is
    a random permutation except inside the tie groups; rank-tie lines are placed in reverse teacher order, line-tie lines in teacher
    order, so a wrong tie rule gives a wrong order.  The ties straddle the relT cut of modes 8 (5), 9 (10) and 10 (20)."""
    rng = np.random.default_rng(seed)
    teacher, rows = {}, []
    for qi, q in enumerate(QIDS):
        pids = (rng.permutation(1000)[:40] + 7000 * qi).tolist()
        teacher[q] = pids
        score = [10.0 - 0.25 * t for t in range(40)]
        rank = (rng.permutation(40) + 1).tolist()
        for g in RANK_TIES:
            for t in g:
                score[t] = score[g[0]]
            for t, r in zip(g, sorted(rank[t] for t in g)):
                rank[t] = r
        for g in LINE_TIES:
            for t in g:
                score[t], rank[t] = score[g[0]], rank[g[0]]
        rows += [(q, t, pids[t], rank[t], score[t]) for t in range(40)]
    order = rng.permutation(len(rows))
    pos = {(r[0], r[1]): int(i) for i, r in zip(order, rows)}
    for q in QIDS:
        for groups, reverse in ((RANK_TIES, True), (LINE_TIES, False)):
            for g in groups:
                slots = sorted(pos[(q, t)] for t in g)
                for t, s in zip(sorted(g, reverse=reverse), slots):
                    pos[(q, t)] = s
    lines = [None] * len(rows)
    for q, t, p, r, s in rows:
        lines[pos[(q, t)]] = f"{q}\t{p}\t{r}\t{s}\n"
    # queries in order of first appearance
    first = sorted(QIDS, key=lambda q: min(pos[(q, t)] for t in range(40)))
    with open(path, "w") as fh:
        fh.write("".join(lines))
    return {q: teacher[q] for q in first}


def read_lines(path):
    with open(path) as fh:
        return [json.loads(line) for line in fh]


@pytest.mark.parametrize("mode", ["8", "9", "10"])
def test_hand_made_run(mode, tmp_path):
    run = tmp_path / "teacher.run"
    teacher = hand_made_run(run)
    most_w, semi_w = WINDOWS[mode]
    spec = C.curriculum_spec(mode, most_w, semi_w)
    n_rel = {"8": 5, "9": 10, "10": 20}[mode]
    assert (spec.n_rel, spec.n_most_hard, spec.n_semi_hard) == {"8": (5, 12, 13), "9": (10, 10, 10), "10": (20, 5, 5)}[mode]
    picks = {}
    for seed in (0, 12345):
        out = tmp_path / f"train{seed}.json"
        assert C.build_curriculum_file(str(run), str(out), mode, most_w, semi_w, seed=seed) == (3, 0)
        got = read_lines(out)
        assert [ex["qid"] for ex in got] == list(teacher)
        for ex in got:
            assert list(ex) == ["qid", "relT_pids", "most_hard_pids", "semi_hard_pids"]
            t = teacher[ex["qid"]]
            pos = {p: i + 1 for i, p in enumerate(t)}
            assert ex["relT_pids"] == t[:n_rel]
            assert len(ex["most_hard_pids"]) == spec.n_most_hard and len(ex["semi_hard_pids"]) == spec.n_semi_hard
            assert all(most_w[0] <= pos[p] <= most_w[1] for p in ex["most_hard_pids"])
            assert all(semi_w[0] <= pos[p] <= semi_w[1] for p in ex["semi_hard_pids"])
            every = ex["relT_pids"] + ex["most_hard_pids"] + ex["semi_hard_pids"]
            assert len(set(every)) == len(every)
            assert ex["most_hard_pids"] == expected_sample(t, most_w, spec.n_most_hard, ex["qid"], seed)
            assert ex["semi_hard_pids"] == expected_sample(t, semi_w, spec.n_semi_hard, ex["qid"], seed)
        picks[seed] = [(ex["most_hard_pids"], ex["semi_hard_pids"]) for ex in got]
    assert picks[0] != picks[12345]


def test_default_counts_and_windows_follow_the_label_mode_tables():
    want = {"2": (10, 10, 10), "3": (10, 20, 0), "4": (10, 10, 10), "5": (20, 10, 0), "6": (30, 0, 0), "7": (5, 25, 0),
            "8": (5, 12, 13), "9": (10, 10, 10), "10": (20, 5, 5)}
    for mode, counts in want.items():
        s = C.curriculum_spec(mode)
        assert (s.n_rel, s.n_most_hard, s.n_semi_hard) == counts
        assert s.most_hard_ranks == (counts[0] + 1, 100) and s.semi_hard_ranks == (101, 200)
    assert C.curriculum_spec("6").min_candidates == 30 and C.curriculum_spec("3").min_candidates == 100
    assert C.curriculum_spec(9).min_candidates == 200


def _tables(tmp_path, pids, qids):
    from toy_tokenizer import WORDS
    q_path, c_path = tmp_path / "queries.tsv", tmp_path / "collection.tsv"
    q_path.write_text("".join(f"{q}\t{' '.join(WORDS[(q + i) % len(WORDS)] for i in range(3))}\n" for q in qids))
    c_path.write_text("".join(f"{p}\t{' '.join(WORDS[(p * 7 + i) % len(WORDS)] for i in range(1 + p % 9))}\n" for p in pids))
    return q_path, c_path


@pytest.mark.parametrize("mode,ctor", [("8", "create_from_5relT_25neg_file"), ("9", "create_from_10relT_20neg_file"),
                                       ("10", "create_from_20relT_10neg_file")])
def test_round_trip_through_the_loader(mode, ctor, tmp_path):
    from toy_tokenizer import make_tokenizer
    run = tmp_path / "teacher.run"
    teacher = hand_made_run(run, seed=4)
    out = tmp_path / "train.json"
    C.build_curriculum_file(str(run), str(out), mode, *WINDOWS[mode], seed=7)
    q_path, c_path = _tables(tmp_path, sorted(p for t in teacher.values() for p in t), list(teacher))
    ds = getattr(NwayDataset, ctor)(str(q_path), str(c_path), str(out), make_tokenizer(), 8, 12, mode)
    got = read_lines(out)
    assert len(ds) == 3
    batch = ds.collate_fn([ds[i] for i in range(3)])
    want = [ex["relT_pids"] + ex["most_hard_pids"] + ex["semi_hard_pids"] for ex in got]
    assert batch["nway_pids"].tolist() == want
    assert torch.equal(batch["labels"], torch.FloatTensor([labels_for_mode(mode)] * 3))
    assert tuple(batch["nway_passages"]["input_ids"].shape[:2]) == (3, len(labels_for_mode(mode)))


def random_run(path, n_q=25, k=60, seed=9, short=()):
    """n_q queries x k candidates (fewer for the queries listed in `short`: {index: count}), random scores with ties, lines shuffled.
    Returns (lines, qids in generation order)."""
    rng = np.random.default_rng(seed)
    qids = rng.choice(10 ** 6, n_q, replace=False)
    rows = []
    for i, q in enumerate(qids):
        n = dict(short).get(i, k)
        for r, p in enumerate(rng.choice(10 ** 7, n, replace=False)):
            rows.append(f"{q}\t{p}\t{r + 1}\t{float(rng.integers(0, 30)) * 0.5}\n")
    lines = [rows[i] for i in rng.permutation(len(rows))]
    with open(path, "w") as fh:
        fh.write("".join(lines))
    return lines, qids.tolist()


def test_a_subset_of_the_queries_gives_the_same_lines(tmp_path):
    lines, _ = random_run(tmp_path / "all.run")
    full = tmp_path / "all.json"
    C.build_curriculum_file(str(tmp_path / "all.run"), str(full), "9", "11:30", "31:60", seed=3)
    by_q = {ex["qid"]: ex for ex in read_lines(full)}
    order = list(dict.fromkeys(int(line.split("\t")[0]) for line in lines))
    assert list(by_q) == order
    keep = set(order[::2])
    (tmp_path / "half.run").write_text("".join(line for line in lines if int(line.split("\t")[0]) in keep))
    C.build_curriculum_file(str(tmp_path / "half.run"), str(tmp_path / "half.json"), "9", "11:30", "31:60", seed=3)
    half = read_lines(tmp_path / "half.json")
    assert [ex["qid"] for ex in half] == order[::2]
    assert all(ex == by_q[ex["qid"]] for ex in half)


@pytest.mark.parametrize("kw,match", [
    (dict(label_mode="1"), "label mode 1"),
    (dict(label_mode="11"), "not one of"),
    (dict(label_mode="9", most_hard_ranks="10:30"), "relT"),
    (dict(label_mode="8", semi_hard_ranks="3:40", most_hard_ranks="41:60"), "relT"),
    (dict(label_mode="9", most_hard_ranks="11:40", semi_hard_ranks="40:60"), "overlap"),
    (dict(label_mode="9", most_hard_ranks="11:15"), "fewer than the 10"),
    (dict(label_mode="9", semi_hard_ranks="101:105"), "fewer than the 10"),
    (dict(label_mode="9", n_most_hard=21), "n_most_hard"),
])
def test_refusals_before_the_run_is_read(kw, match, tmp_path):
    with pytest.raises(ValueError, match=match):
        C.build_curriculum_file(str(tmp_path / "does-not-exist.run"), str(tmp_path / "out.json"), **kw)
    assert not (tmp_path / "out.json").exists()


def test_refusals_of_the_run(tmp_path):
    lines, _ = random_run(tmp_path / "a.run", n_q=4, k=40)
    (tmp_path / "dup.run").write_text("".join(lines[:30] + [lines[7]] + lines[30:]))
    q, p = lines[7].split("\t")[:2]
    with pytest.raises(ValueError, match=f"qid {q}, pid {p}"):
        C.build_curriculum_file(str(tmp_path / "dup.run"), str(tmp_path / "o.json"), "9", "11:20", "21:40")
    (tmp_path / "two.run").write_text("".join("\t".join(line.split("\t")[:2]) + "\n" for line in lines))
    with pytest.raises(ValueError, match="4 columns"):
        C.build_curriculum_file(str(tmp_path / "two.run"), str(tmp_path / "o.json"), "9", "11:20", "21:40")
    (tmp_path / "three.run").write_text("".join(lines[:50]) + "5\t6\t7\n" + "".join(lines[50:]))
    with pytest.raises(ValueError, match="4 columns"):
        C.build_curriculum_file(str(tmp_path / "three.run"), str(tmp_path / "o.json"), "9", "11:20", "21:40")
    assert not (tmp_path / "o.json").exists()


def test_short_queries_are_skipped_and_counted(tmp_path):
    # windows 11:30 / 31:60: a query needs 60 candidates; 59 is too short, 61 is enough
    lines, qids = random_run(tmp_path / "r.run", n_q=8, k=60, short={1: 59, 4: 12, 6: 61})
    n, skipped = C.build_curriculum_file(str(tmp_path / "r.run"), str(tmp_path / "o.json"), "9", "11:30", "31:60")
    order = list(dict.fromkeys(int(line.split("\t")[0]) for line in lines))
    got = read_lines(tmp_path / "o.json")
    assert (n, skipped) == (6, 2)
    assert [ex["qid"] for ex in got] == [q for q in order if q not in (qids[1], qids[4])]
    assert all(len(ex["relT_pids"]) == 10 and len(ex["most_hard_pids"]) == 10 and len(ex["semi_hard_pids"]) == 10 for ex in got)
    # mode 6 draws no negatives: 30 candidates are enough whatever the windows
    n6, skipped6 = C.build_curriculum_file(str(tmp_path / "r.run"), str(tmp_path / "o6.json"), "6")
    assert (n6, skipped6) == (7, 1)
    assert all(len(ex["relT_pids"]) == 30 and ex["most_hard_pids"] == [] == ex["semi_hard_pids"] for ex in read_lines(tmp_path / "o6.json"))


def test_n_most_hard_changes_the_split(tmp_path):
    random_run(tmp_path / "r.run", n_q=5)
    C.build_curriculum_file(str(tmp_path / "r.run"), str(tmp_path / "a.json"), "9", "11:40", "41:60")
    C.build_curriculum_file(str(tmp_path / "r.run"), str(tmp_path / "b.json"), "9", "11:40", "41:60", n_most_hard=16)
    for a, b in zip(read_lines(tmp_path / "a.json"), read_lines(tmp_path / "b.json")):
        assert (len(a["most_hard_pids"]), len(a["semi_hard_pids"])) == (10, 10)
        assert (len(b["most_hard_pids"]), len(b["semi_hard_pids"])) == (16, 4)
        assert a["relT_pids"] == b["relT_pids"]


def test_command_line_writes_the_library_output(tmp_path):
    random_run(tmp_path / "r.run", n_q=9, short={2: 20})
    lib = tmp_path / "lib.json"
    C.build_curriculum_file(str(tmp_path / "r.run"), str(lib), "8", "6:30", "31:60", n_most_hard=14, seed=99)
    cli = tmp_path / "out" / "cli.json"
    r = subprocess.run([sys.executable, "-m", "cldrd_amd.dataset.curriculum_file", "--run_path", str(tmp_path / "r.run"), "--label_mode", "8",
                        "--output_path", str(cli), "--most_hard_ranks", "6:30", "--semi_hard_ranks", "31:60", "--n_most_hard", "14",
                        "--seed", "99"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "wrote 8 queries" in r.stdout and "skipped 1" in r.stdout
    assert cli.read_bytes() == lib.read_bytes()
    assert os.listdir(tmp_path / "out") == ["cli.json"]          # the temporary file was renamed into place


def test_native_writer_run_gives_the_hand_written_examples(tmp_path):
    """The teacher's run as rerank_top_passages writes it (write_run_file from float32 arrays: tabs, repr of the fp32 score) and the same
    values hand-written with spaces and a shorter score text: the same examples."""
    from cldrd_amd.retriever.retrieve_top_passages import write_run_file
    rng = np.random.default_rng(21)
    nq, k = 12, 50
    qids = rng.choice(10 ** 6, nq, replace=False).astype(np.int64)
    pids = np.stack([rng.choice(10 ** 7, k, replace=False) for _ in range(nq)]).astype(np.int64)
    scores = -np.sort((rng.integers(0, 40, (nq, k)) * 0.1).astype(np.float32), axis=1)             # descending, with ties
    assert write_run_file(str(tmp_path / "native.run"), qids.tolist(), pids, scores) == nq * k
    native = (tmp_path / "native.run").read_text().splitlines()
    assert native[0].split("\t")[:3] == [str(qids[0]), str(pids[0, 0]), "1"]
    (tmp_path / "hand.run").write_text("".join(f"{qids[i]}  {pids[i, j]} {j + 1} {np.float32(scores[i, j])}\n"
                                               for i in range(nq) for j in range(k)))
    for mode in ("9", "10"):
        a = C.build_curriculum_file(str(tmp_path / "native.run"), str(tmp_path / "a.json"), mode, "21:35", "36:50", seed=5)
        b = C.build_curriculum_file(str(tmp_path / "hand.run"), str(tmp_path / "b.json"), mode, "21:35", "36:50", seed=5)
        assert a == b == (nq, 0)
        assert (tmp_path / "a.json").read_bytes() == (tmp_path / "b.json").read_bytes()
        ex = read_lines(tmp_path / "a.json")
        assert [e["relT_pids"] for e in ex] == pids[:, :C.curriculum_spec(mode).n_rel].tolist()


def test_splitmix64_matches_the_python_restatement():
    xs = [0, 1, 2 ** 63, M64, 0x9E3779B97F4A7C15, 123456789]
    assert C.splitmix64(np.array(xs, dtype=np.uint64)).tolist() == [sm64(x) for x in xs]
    assert C.splitmix64(np.array([-1, -5], dtype=np.int64)).tolist() == [sm64(M64), sm64(M64 - 4)]
    assert C.splitmix64(-3).tolist() == [sm64(M64 - 2)]
    assert sm64(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0
