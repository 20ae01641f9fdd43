#!/usr/bin/env python3
"""Golden launch trace of the encoder tower (``encoder_launch_trace.json``): for every case of ``tests/test_encoder_dryrun.py::TRACE_CASES`` the
entry points the tower calls, in order, and one short hash per launch of its canonical arguments (the form is described in that module; the
cases and the walk are imported from it, so golden and test cannot drift).  Needs the built library and no GPU.

The file records the behaviour of ONE commit, named inside it: it is taken before a change of the tower's host code that is meant to leave
every launch as it is, and never regenerated to make that change pass.  It refuses to run on a tree whose package differs from HEAD.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encoder_launch_trace.py

``--trainer`` writes ``trainer_launch_trace.json`` instead: ``TRAINER_TRACE_CASES`` of the same module, the training step with its streams
and cross-stream waits (same walk, same rule: taken at the commit in front of a change of ``NwayTrainer``'s host code).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import pytest
    import test_encoder_dryrun as T
    if subprocess.run(["git", "diff", "--quiet", "HEAD", "--", "cl-drd_amd"], cwd=ROOT).returncode:
        raise SystemExit("the package differs from HEAD: the golden is the trace of a commit")
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    T._lib.load()
    trainer = "--trainer" in sys.argv[1:]
    source, out = (T.TRAINER_TRACE_CASES, "trainer_launch_trace.json") if trainer else (T.TRACE_CASES, "encoder_launch_trace.json")
    cases = {}
    for case in sorted(source):
        walks = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as mp:
                walks.append(T.walk_trace(case, T._install_stubs(mp), mp, source))
        if walks[0] != walks[1]:
            raise SystemExit(f"{case}: two walks differ - the canonical form is not deterministic here")
        cases[case] = dict(names=[n for n, _ in walks[0]], hashes=[h for _, h in walks[0]])
    with open(os.path.join(HERE, out), "w") as fh:
        fh.write('{"commit": "%s",\n "cases": {\n' % commit)
        fh.write(",\n".join('  %s: %s' % (json.dumps(c), json.dumps(v, separators=(",", ":"))) for c, v in cases.items()))
        fh.write("\n }}\n")
    print("wrote", out + ":", len(cases), "cases,", sum(len(v["names"]) for v in cases.values()), "launches, at", commit)


if __name__ == "__main__":
    main()
