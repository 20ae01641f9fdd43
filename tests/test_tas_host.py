"""Topic-aware batches without a GPU: the k-means entry points' library surface (header, exports, SIGNATURES, every limit refused before a
device is touched), the TopicBatchSampler on a stub dataset, and the --tas_clusters flag of the trainer (refusals by flag name, the
checkpoint's position fields, an unchanged default loader)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
from cldrd_amd import _lib
from cldrd_amd.trainer import nway_listwise as T

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = {"cldrd_kmeans_assign": 10, "cldrd_kmeans_half_sqnorm": 5, "cldrd_kmeans_finish": 8}


# ------------------------------------------------------------------------------------------------------------------ the library surface
def test_header_exports_and_signatures_agree():
    text = open(os.path.join(conftest.ROOT, "include", "cldrd_hip.h")).read()
    assert "assign[i] = the lowest j that attains max_j s(i, j)" in text            # the definition stands in the header
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, n_args in ENTRY.items():
        m = re.search(rf"int\s+{name}\s*\(([^)]*)\)", text)
        assert m, f"include/cldrd_hip.h does not declare {name}"
        params = [p.strip() for p in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.ci and len(params) == len(argtypes) == n_args
        for p, a in zip(params, argtypes):
            assert a is (_lib.vp if "*" in p else _lib.ci), (name, p, a)
        assert hasattr(lib, name)
    assert lib.cldrd_version() == _lib.ABI_VERSION


P = C.c_void_p(64)          # a fake, aligned, non-null pointer: every call below must be refused before the library touches a device


def _assign(**over):
    a = dict(X=P, ldx=64, n=1000, d=64, C=P, h=P, k=10, assign=P, best=None, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return "kmeans_assign", _lib.load().cldrd_kmeans_assign(*a.values())


def _half(**over):
    a = dict(C=P, k=10, d=64, h=P, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return "kmeans_half_sqnorm", _lib.load().cldrd_kmeans_half_sqnorm(*a.values())


def _finish(**over):
    a = dict(sums=P, offsets=P, C=P, h=P, n_empty=P, k=10, d=64, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return "kmeans_finish", _lib.load().cldrd_kmeans_finish(*a.values())


ODD = C.c_void_p(68)
WIDTHS = [dict(d=0), dict(d=16), dict(d=48), dict(d=1056), dict(d=2048)]


@pytest.mark.parametrize("call,over,word", [
    *[(_assign, o, "d must") for o in WIDTHS], *[(_half, o, "d must") for o in WIDTHS], *[(_finish, o, "d must") for o in WIDTHS],
    (_assign, dict(k=0), "k must"), (_assign, dict(k=65537, n=70000), "k must"), (_assign, dict(k=1001), "k must not exceed n"),
    (_assign, dict(n=0, k=1), "n must"), (_assign, dict(n=(1 << 22) + 1), "n must"),
    (_assign, dict(ldx=60), "ldx"), (_assign, dict(ldx=66), "ldx"),
    (_assign, dict(X=None), "null X"), (_assign, dict(C=None), "null C"), (_assign, dict(h=None), "null h"), (_assign, dict(assign=None), "null assign"),
    (_assign, dict(X=ODD), "X must be 16-byte"), (_assign, dict(C=ODD), "C must be 16-byte"), (_assign, dict(h=ODD), "h must be 16-byte"),
    (_assign, dict(assign=ODD), "assign must be 16-byte"), (_assign, dict(best=ODD), "best must be 16-byte"),
    (_half, dict(k=0), "k must"), (_half, dict(k=65537), "k must"), (_half, dict(C=None), "null C"), (_half, dict(h=None), "null h"),
    (_half, dict(C=ODD), "C must be 16-byte"), (_half, dict(h=ODD), "h must be 16-byte"),
    (_finish, dict(k=0), "k must"), (_finish, dict(k=65537), "k must"),
    (_finish, dict(sums=None), "null sums"), (_finish, dict(offsets=None), "null offsets"), (_finish, dict(C=None), "null C"),
    (_finish, dict(h=None), "null h"), (_finish, dict(n_empty=None), "null n_empty"),
    (_finish, dict(sums=ODD), "sums must be 16-byte"), (_finish, dict(offsets=ODD), "offsets must be 16-byte"), (_finish, dict(n_empty=ODD), "n_empty must be 16-byte"),
])
def test_limits_are_refused_without_a_device(call, over, word):
    op, rc = call(**over)
    msg = _lib.load().cldrd_last_error().decode()
    assert rc != 0 and msg.startswith(op + ":") and word in msg, (over, rc, msg)


def test_the_wrappers_have_no_cpu_path():
    from cldrd_amd import cluster, hip_ops
    x, c = torch.zeros(10, 64), torch.zeros(2, 64)
    for fn in (lambda: hip_ops.kmeans_assign(x, c), lambda: hip_ops.kmeans_half_sqnorm(c),
               lambda: hip_ops.kmeans_update(x, torch.zeros(10, dtype=torch.int64), c)):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fn()
    with pytest.raises(ValueError, match="on the GPU"):
        cluster.kmeans(x, 2)


# ------------------------------------------------------------------------------------------------------------------------- the sampler
class _Stub:
    """what TopicBatchSampler reads of a dataset: train_examples[i]["qid"]"""

    def __init__(self, qids):
        self.train_examples = [{"qid": q} for q in qids]

    def __len__(self):
        return len(self.train_examples)


def _gen(seed=7):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _stub(sizes):
    """examples 100, 101, ...: cluster c holds sizes[c] of them, interleaved so that grouping has something to do"""
    cl = [c for c, m in enumerate(sizes) for _ in range(m)]
    order = torch.randperm(len(cl), generator=_gen(1)).tolist()
    cl = [cl[i] for i in order]
    qids = [100 + i for i in range(len(cl))]
    return _Stub(qids), dict(zip(qids, cl)), cl


def test_sampler_cuts_pure_and_mixed_batches():
    ds, cof, cl = _stub([5, 4, 3])
    s = T.TopicBatchSampler(ds, cof, 4, generator=_gen())
    assert len(s) == 12 // 4 == 3 and s.n_pure == 2
    for _ in range(3):          # every epoch
        batches = list(s)
        assert len(batches) == 3 and sorted(i for b in batches for i in b) == list(range(12))          # every example once
        kinds = sorted(len({cl[i] for i in b}) for b in batches)
        assert kinds == [1, 1, 2]          # two pure batches (clusters 0 and 1), one mixed of the remainders 1 + 0 + 3
    assert "2 pure + 1 mixed" in s.describe() and "66.7 %" in s.describe()


def test_pure_batches_hold_one_cluster_and_the_tail_is_dropped():
    ds, cof, cl = _stub([9, 1, 1, 1])
    s = T.TopicBatchSampler(ds, cof, 4, generator=_gen())
    assert len(s) == 3 and s.n_pure == 2
    seen = set()
    for _ in range(4):
        batches = list(s)
        flat = [i for b in batches for i in b]
        assert len(batches) == 3 and len(set(flat)) == 12 and all(len(b) == 4 for b in batches)
        pure = [b for b in batches if len({cl[i] for i in b}) == 1]
        assert len(pure) == 2 and all(cl[b[0]] == 0 for b in pure)
        mixed = [b for b in batches if len({cl[i] for i in b}) > 1]
        assert len(mixed) == 1 and sorted(cl[i] for i in mixed[0]) == [0, 1, 2, 3]          # remainders in ascending cluster order: 1 + 1 + 1 + 1
        assert [cl[i] for i in mixed[0]] == [0, 1, 2, 3]
        seen.add(tuple(map(tuple, batches)))
    assert len(seen) > 1          # epochs differ
    ds, cof, cl = _stub([6, 5, 3])          # 14 examples at B = 4: 2 pure, remainders 2 + 1 + 3 -> one mixed, two examples dropped
    s = T.TopicBatchSampler(ds, cof, 4, generator=_gen())
    batches = list(s)
    assert len(s) == len(batches) == 14 // 4 and s.n_pure == 2 and len({i for b in batches for i in b}) == 12
    assert len(list(T.TopicBatchSampler(_Stub([1, 2]), {1: 0, 2: 0}, 4, generator=_gen()))) == 0


def test_equally_seeded_samplers_give_the_same_stream_and_a_resume_gives_its_tail():
    ds, cof, _ = _stub([5, 4, 3, 7, 2])
    a, b = (T.TopicBatchSampler(ds, cof, 4, generator=_gen(3)) for _ in range(2))
    sa, sb = [list(a) for _ in range(3)], [list(b) for _ in range(3)]
    assert sa == sb and sa[0] != sa[1]
    assert [list(a.with_generator(g)) for g in [_gen(3)] for _ in range(3)] == sa
    # under the position wrapper: the stream after resume(skip, state) is the tail of the uninterrupted one, then the next epoch
    g = _gen(3)
    pos = T._EpochPosition(T.TopicBatchSampler(ds, cof, 4, generator=g), g)
    full, states = [], []
    for _ in range(3):
        full.append(list(pos))
        states.append(pos.epoch_state.clone())
    assert full == sa and len(full[0]) == len(pos) == 21 // 4
    for epoch in (0, 1):
        for skip in (0, 2, 5):
            g2 = _gen(99)
            pos2 = T._EpochPosition(T.TopicBatchSampler(ds, cof, 4, generator=g2), g2)
            pos2.resume(skip, states[epoch])
            assert list(pos2) == full[epoch][skip:] and list(pos2) == full[epoch + 1], (epoch, skip)


# ---------------------------------------------------------------------------------------------------------------------------- the flag
def _args(tmp_path, extra=()):
    sys.path.insert(0, HERE)
    from toy_tokenizer import make_tokenizer
    fix = os.path.join(HERE, "golden", "nway_dataset_fixture")
    tokdir = os.path.join(str(tmp_path), "tok")
    if not os.path.isdir(tokdir):
        make_tokenizer().save_pretrained(tokdir)
    a = T.get_args(["--experiment_folder", str(tmp_path), "--run_folder", "run", "--queries_path", os.path.join(fix, "queries.tsv"),
                    "--collection_path", os.path.join(fix, "collection.tsv"), "--training_path", os.path.join(fix, "train_10relT_20neg.jsonl"),
                    "--label_mode", "9", "--tokenizer_name_or_path", tokdir, "--query_max_len", "6", "--passage_max_len", "16",
                    "--train_batch_size", "4", "--loader_workers", "0", *extra])
    a.rank, a.nranks, a.distributed = 0, 1, False
    return a


def _fixture_qids():
    import json
    fix = os.path.join(HERE, "golden", "nway_dataset_fixture", "train_10relT_20neg.jsonl")
    return [int(json.loads(line)["qid"]) for line in open(fix)]


def _cluster_file(tmp_path, name, qids, sizes=(5, 4, 3)):
    cl = [c for c, m in enumerate(sizes) for _ in range(m)]
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write("".join(f"{q}\t{c}\n" for q, c in zip(qids, cl)))
    return path, dict(zip(qids, cl))


def test_refusals_name_the_flag(tmp_path):
    with pytest.raises(ValueError, match="--tas_clusters.*--synthetic_steps"):
        T.get_args(["--synthetic_steps", "4", "--tas_clusters", "clusters.tsv", "--loss", "kl_div"])
    qids = _fixture_qids()
    assert len(qids) == 12
    short, _ = _cluster_file(tmp_path, "short.tsv", qids[2:], sizes=(5, 3, 2))
    with pytest.raises(ValueError, match=rf"--tas_clusters: 2 of the 12 training examples.*the first: {qids[0]}\)"):
        T.build_dataloader(_args(tmp_path, ["--tas_clusters", short]))
    for i, bad in enumerate(("12\t1\tx\n", "12\n", "abc\t1\n", "12\t1.5\n", "12\t-1\n", "\n")):
        path = os.path.join(str(tmp_path), f"bad{i}.tsv")
        open(path, "w").write(f"{qids[0]}\t0\n" + bad)
        with pytest.raises(ValueError, match="--tas_clusters: line 2 of"):
            T.build_dataloader(_args(tmp_path, ["--tas_clusters", path]))
    empty = os.path.join(str(tmp_path), "empty.tsv")
    open(empty, "w").close()
    with pytest.raises(ValueError, match="--tas_clusters"):
        T.read_query_clusters(empty)


def test_the_loader_under_the_flag_and_without_it(tmp_path):
    import numpy as np
    qids = _fixture_qids()
    path, cof = _cluster_file(tmp_path, "clusters.tsv", qids)
    # without the flag: exactly the samplers of today
    _, plain = T.build_dataloader(_args(tmp_path))
    inner = T._position_of(plain).inner
    assert type(inner) is torch.utils.data.BatchSampler and type(inner.sampler) is torch.utils.data.RandomSampler
    assert inner.batch_size == 4 and inner.drop_last and inner.sampler.generator is T._position_of(plain).generator
    assert T.get_args([]).tas_clusters is None
    # with it
    a = _args(tmp_path, ["--tas_clusters", path])
    ds, loader = T.build_dataloader(a)
    pos = T._position_of(loader)
    assert isinstance(pos, T._EpochPosition) and type(pos.inner) is T.TopicBatchSampler and pos.inner.generator is pos.generator
    assert len(loader) == 3 and pos.inner.n_pure == 2 and re.fullmatch(r"[0-9a-f]{16}", pos.inner.file_digest)
    assert pos.inner.file_digest == T.read_query_clusters(path)[1]
    states = []
    for _ in range(2):
        batches = [np.asarray(b["qid"]).tolist() for b in loader]
        states.append(pos.epoch_state.clone())
        assert sorted(q for b in batches for q in b) == sorted(qids)
        assert sorted(len({cof[q] for q in b}) for b in batches) == [1, 1, 2]
    # a rank that replays its generator replays THIS sampler's draws
    for e in range(2):
        assert torch.equal(T.replayed_epoch_state(loader, a.seed + a.rank, e), states[e])


def test_position_fields_with_and_without_the_flag():
    saved = {"train_batch_size": 8, "nranks": 1, "seed": 4680, "dataset_len": 503000, "steps_per_epoch": 62875, "num_train_epochs": 4}
    assert T.TAS_POSITION_FIELDS == ("tas_clusters", "tas_clusters_digest") and not set(T.TAS_POSITION_FIELDS) & set(T.POSITION_FIELDS)
    tas = dict(saved, tas_clusters="a.tsv", tas_clusters_digest="0123456789abcdef")
    T.check_resume_position(saved, dict(saved))
    T.check_resume_position(tas, dict(tas))
    for s, c, field in ((tas, dict(tas, tas_clusters_digest="f" * 16), "tas_clusters_digest"), (tas, dict(tas, tas_clusters="b.tsv"), "tas_clusters"),
                        (saved, tas, "tas_clusters"), (tas, saved, "tas_clusters")):
        with pytest.raises(ValueError, match=rf"--resume_exact: {field} was "):
            T.check_resume_position(s, c)
