"""The chunk plan of a weight-gradient group launch (csrc/gemm_tn.hip: wgrad_plan_group) through the host-only export cldrd_wgrad_plan:
no device call, so this runs without a GPU.  A plan cuts every problem's token range into n_long chunks of c_long K tiles (64 tokens) followed
by n_short chunks of c_short; the launch runs all long items first, the short ones last.

Reference figures (replay of the dispatch on 256 CUs, item cost = K tiles + 6, items in launch order) for the cfg2 passage group, 25
problems at T = 32 768: one split count for the launch gives 1 310 (2), 1 245 (3, what the launch used), 1 220 (4), 1 219 (5), 1 280 (6) units for
1 163 units of work per CU at 3 splits; the candidate set holds the long-first schedule that reaches 1 172 (256-K-tile chunks, the remainder
beyond four whole rounds re-cut into 32-K-tile chunks, 16 slabs for those tiles).  The planner also weighs the slab bytes (as the split rule
always did) and takes 128-K-tile short chunks instead: makespan 1 192, modelled time 1 280.9 against 1 302.5 for the 1 172 schedule and 1 384.9
for 3 splits, 319 MB of slabs instead of 510 MB."""
import ctypes as C
import os

import pytest

from conftest import ROOT  # noqa: F401

BK = 64
MAXK = 256          # the drift cap: no item sweeps more K tiles (csrc/gemm_tn.hip: WGRAD_MAXK)


@pytest.fixture(scope="module")
def lib():
    from cldrd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def layer(T, d=768, f=3072):
    """the four problems (M, N1, N2) of a full encoder layer, in the order the backward queues them"""
    return [(T, d, f), (T, f, d), (T, d, d), (T, 3 * d, d)]


def cls_layer(Mc, T, d=768, f=3072):
    """the CLS-only last layer: four problems over the Mc CLS rows and the K/V projection over all tokens"""
    return [(Mc, d, f), (Mc, f, d), (Mc, d, d), (Mc, d, d), (T, 2 * d, d)]


GROUPS = {
    "cfg2_passage": cls_layer(256, 32768) + layer(32768) * 5,
    "cfg2_two_layers": layer(32768) * 2,
    "cfg2_three_layers": layer(32768) * 3,
    "cfg2_cls_and_one_layer": cls_layer(256, 32768) + layer(32768),
    "query": cls_layer(30, 240) + layer(240) * 5,
    "cfg4_bert_base": cls_layer(256, 4 * 64 * 256) + layer(4 * 64 * 256) * 11,       # 49 problems: two launches
    "packed_ragged": cls_layer(256, 30001) + layer(30001) * 5,                       # token count not a multiple of 64
    "tiny": [(4096, 128, 128)] * 3,
    "n2_192": [(3000, 768, 576), (3000, 1536, 768), (777, 512, 192)],
}


def plan(lib, probs, uniform=0):
    n = len(probs)
    IN = C.c_int * n
    M, N1, N2 = IN(*[p[0] for p in probs]), IN(*[p[1] for p in probs]), IN(*[p[2] for p in probs])
    chunks, info, model = (C.c_int * (4 * n))(), (C.c_int * 8)(), (C.c_double * 2)()
    rc = lib.cldrd_wgrad_plan(M, N1, N2, n, uniform, chunks, info, model)
    assert rc == 0, lib.cldrd_last_error()
    return {"chunks": [tuple(chunks[4 * i:4 * i + 4]) for i in range(n)], "tile": (info[0], info[1]), "items": info[2], "launches": info[3],
            "arg_bytes": info[4], "arg_limit": info[5], "per_launch": info[6], "makespan": model[0], "cost": model[1],
            "workspace": lib.cldrd_wgrad_group_workspace(M, N1, N2, n)}


def chunk_ranges(kt, c):
    """[kbeg, kend) of every chunk as the kernel derives them: long chunks from K tile 0, short ones from n_long * c_long, clipped to kt"""
    n_long, c_long, n_short, c_short = c
    out = [(i * c_long, min(kt, (i + 1) * c_long)) for i in range(n_long)]
    base = n_long * c_long
    out += [(base + i * c_short, min(kt, base + (i + 1) * c_short)) for i in range(n_short)]
    return out


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_plan_covers_every_k_range_once(lib, name):
    probs = GROUPS[name]
    p = plan(lib, probs)
    t1, t2 = p["tile"]
    items = workspace = 0
    for (M, N1, N2), c in zip(probs, p["chunks"]):
        kt = (M + BK - 1) // BK
        ranges = chunk_ranges(kt, c)
        assert ranges, (name, c)
        pos = 0
        for lo, hi in ranges:           # every tile of the problem sweeps the same chunks: no gap, no overlap, no empty chunk, none over the cap
            assert lo == pos and hi > lo and hi - lo <= MAXK, (name, (M, N1, N2), c, ranges)
            pos = hi
        assert pos == kt, (name, (M, N1, N2), c)
        assert N1 % t1 == 0 and N2 % t2 == 0
        items += (N1 // t1) * (N2 // t2) * len(ranges)
        if len(ranges) > 1:
            workspace += len(ranges) * (N1 * N2 + N1)       # one fp32 slab (dW and dbias) per chunk; a single chunk writes dW directly
    assert items == p["items"]
    assert workspace == p["workspace"]
    assert p["launches"] == (len(probs) + p["per_launch"] - 1) // p["per_launch"]
    assert p["arg_bytes"] <= p["arg_limit"] == 4096


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_plan_is_never_modelled_slower_than_a_uniform_split(lib, name):
    probs = GROUPS[name]
    p = plan(lib, probs)
    kt = max((M + BK - 1) // BK for M, _, _ in probs)
    uniform = {sp: plan(lib, probs, uniform=sp) for sp in range(1, 9)}
    fastest = min(u["makespan"] for u in uniform.values())
    for sp, u in uniform.items():
        assert p["makespan"] <= u["makespan"] + 1e-9, (name, sp, p["makespan"], u["makespan"])
        # the planner takes the smallest modelled time (replay + slab bytes + reduction launch) among the candidates that replay no longer than
        # every uniform count: a uniform count that is such a candidate itself (and that the drift cap allows) is therefore no cheaper
        if u["makespan"] <= fastest + 1e-9 and (kt + sp - 1) // sp <= MAXK:
            assert p["cost"] <= u["cost"] + 1e-9, (name, sp, p["cost"], u["cost"])


def test_cfg2_replay_matches_the_reference(lib):
    probs = GROUPS["cfg2_passage"]
    u3 = plan(lib, probs, uniform=3)
    assert u3["items"] == 1944 and u3["makespan"] == 1245.0
    assert [plan(lib, probs, uniform=sp)["makespan"] for sp in (4, 6)] == [1220.0, 1280.0]
    p = plan(lib, probs)
    assert p["makespan"] <= 1192.0 and p["cost"] < u3["cost"]
    assert p["workspace"] < 0.7 * 3 * sum(N1 * N2 + N1 for _, N1, N2 in probs)      # and fewer slab bytes: two slabs for most tiles instead of three
    assert all(c == (0, 256, 1, 4) for c in p["chunks"][:4])   # the CLS-only layer's four-K-tile problems: one short item each, written directly


def test_query_group_plan_is_what_it_was(lib):
    probs = GROUPS["query"]
    p, u1 = plan(lib, probs), plan(lib, probs, uniform=1)
    assert p["chunks"] == u1["chunks"] == [(1, (M + BK - 1) // BK, 0, 0) for M, _, _ in probs]
    assert p["items"] == u1["items"] and p["workspace"] == 0


def test_single_problem_keeps_the_split_rule(lib):
    for M, N1, N2 in [(32768, 768, 768), (32768, 3072, 768), (240, 768, 768), (4096, 128, 128), (30001, 2304, 768)]:
        sp = lib.cldrd_wgrad_splits(M, N1, N2)
        kt = (M + BK - 1) // BK
        p = plan(lib, [(M, N1, N2)])
        assert p["chunks"] == [(sp, (kt + sp - 1) // sp, 0, 0)]
        assert p["workspace"] == (sp * (N1 * N2 + N1) if sp > 1 else 0)


def test_plan_is_deterministic(lib):
    for name, probs in sorted(GROUPS.items()):
        a = plan(lib, probs)
        plan(lib, GROUPS["tiny"])
        b = plan(lib, probs)
        assert a == b, name
