"""The NT GEMM's launch plan, from the host: cldrd_gemm_nt_splitk_workspace() answers for the shape alone and needs no GPU, so which shapes
are split along K, and into how many slabs, is compared against a table recorded with the library of the commit in front of the dispatch
refactor (tests/golden/gemm_nt_plan.json, written by tests/golden/make_gemm_nt_plan.py) under every tuning state the tests use."""
import json
import os

import pytest

from conftest import ROOT

MS = (1, 64, 240, 256, 257, 1000, 1023, 1024)
NS = (8, 72, 768, 1600, 2304, 3072)
KS = (64, 96, 512, 768, 1024, 1088, 2304, 3072)        # 96: not a multiple of the 64-deep K tile
STATES = {"default": {}, "gemm_nt64=0": {"gemm_nt64": 0}, "gemm_splitk=1": {"gemm_splitk": 1}, "gemm_splitk=3": {"gemm_splitk": 3}}
DEFAULTS = {"gemm_nt64": 1, "gemm_splitk": 0}
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_nt_plan.json")


def plan_table(lib):
    """{state: [workspace bytes for every (M, N, K) of the grid, M slowest]}; leaves the tuning keys at their defaults."""
    table = {}
    try:
        for state, keys in STATES.items():
            for key, value in {**DEFAULTS, **keys}.items():
                assert lib.cldrd_set_tuning(key.encode(), value) == 0
            table[state] = [int(lib.cldrd_gemm_nt_splitk_workspace(M, N, K)) for M in MS for N in NS for K in KS]
    finally:
        for key, value in DEFAULTS.items():
            lib.cldrd_set_tuning(key.encode(), value)
    return table


def test_workspace_plan_matches_the_recorded_table(request):
    from cldrd_amd import _lib
    lib = _lib.load()
    request.addfinalizer(lambda: [lib.cldrd_set_tuning(k.encode(), v) for k, v in DEFAULTS.items()])
    golden = json.load(open(GOLDEN))
    assert golden["grid"] == {"M": list(MS), "N": list(NS), "K": list(KS)}
    table = plan_table(lib)
    assert sorted(table) == sorted(golden["workspace_bytes"])
    shapes = [(M, N, K) for M in MS for N in NS for K in KS]
    for state in STATES:
        want = golden["workspace_bytes"][state]
        assert len(want) == len(shapes)
        wrong = [(s, g, w) for s, g, w in zip(shapes, table[state], want) if g != w]
        assert not wrong, f"{state}: (shape, got, recorded) {wrong[:5]}"
    # the table is not trivially zero: each state but "never split" splits some shape, and the states differ from one another
    assert not any(golden["workspace_bytes"]["gemm_splitk=1"][i] for i, (M, N, K) in enumerate(shapes) if K <= 1024)
    assert all(any(golden["workspace_bytes"][s]) for s in ("default", "gemm_nt64=0", "gemm_splitk=3"))
    assert len({tuple(v) for v in golden["workspace_bytes"].values()}) == len(STATES)


def test_fp16_operands_with_a_16_bit_residual_are_refused_before_any_launch():
    """fp16 operands know no 16-bit residual: neither the ring (M = 1024 rows, N = 192) nor the 128 x 128 kernel builds that flavour.  The
    dispatch walks both compiled lists and returns the error in front of any HIP call, so a fake pointer stands in for device memory."""
    from cldrd_amd import _lib, hip_ops as ops
    lib = _lib.load()
    P = 64                                  # any non-null, 16-byte aligned "pointer"
    lib.cldrd_set_tuning(None, 0)           # leaves "set_tuning: null key" behind: the message read below is this call's own
    rc = lib.cldrd_gemm_nt16(P, P, P, 1024, 192, 64, 64, 64, 192, P, P, 192, None, None, 0, 1.0, 0.0, 7, 0, 0, ops.FMT_F16,
                             None, None, None, None, None, 0, None)
    assert rc != 0
    assert lib.cldrd_last_error().decode() == "gemm_nt: this epilogue combination is not built for the fp16 format"
