#!/usr/bin/env python3
"""Golden launch plan of the NT GEMM (``gemm_nt_plan.json``): cldrd_gemm_nt_splitk_workspace(M, N, K) over the grid and the tuning states of
``tests/test_gemm_plan_host.py`` (both imported from it, so golden and test cannot drift).  Needs a built library and no GPU.

The file records the behaviour of ONE commit, named inside it: it is taken with that commit's library in front of a change of the GEMM's host
dispatch that is meant to leave every choice as it is, and never regenerated to make that change pass.  CLDRD_LIB selects the library:

    CLDRD_LIB=/path/to/that/commit/libcldrd_hip.so python tests/golden/make_gemm_nt_plan.py COMMIT
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import test_gemm_plan_host as T
    from cldrd_amd import _lib
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    table = T.plan_table(_lib.load())
    with open(T.GOLDEN, "w") as fh:
        json.dump({"commit": sys.argv[1], "grid": {"M": list(T.MS), "N": list(T.NS), "K": list(T.KS)}, "order": "M slowest, K fastest",
                   "workspace_bytes": table}, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{T.GOLDEN}: {sum(len(v) for v in table.values())} entries, {sum(1 for v in table.values() for b in v if b)} of them split")


if __name__ == "__main__":
    main()
