#!/usr/bin/env python3
"""Mutation audit of the call kernel's text (call_cell, graphtyper_amd/csrc/score_core.hpp): do the case sets of
tests/calls_cases.py notice a one-line misreading of the reference's call?  All of it on the host.

Every entry of mutants.json is one such change: a piece of the header's text that occurs once, and what replaces it.  For each,
the header is copied into a temporary directory and changed, tests/emu_calls is built against that directory as a plain
stand-alone program (make CSRC=<tmp> SAN= OPT=-O2; a mutant whose only fault may be a load out of bounds names the sanitizer it is
built with instead, "build"), and the sets are run through it in ORDER until one differs from the restatement
(tests/calls_ref.py) or the program dies.  A mutant no set notices SURVIVES: either mutants.json says why it computes the same
function on every input within the contract ("expect": "survives"), or the sets have a gap.  Results go to audit.json
(committed; tests/test_calls_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/calls_mutants/run_audit.py [-j 8] [--only ID ...]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import calls_cases as cc  # noqa: E402

HEADER = os.path.join(ROOT, "graphtyper_amd", "csrc", "score_core.hpp")
# the cheap sets first, so that a mutant's recorded killer is quick to run again (many_cells is the device's: not here)
ORDER = ["ties", "gq", "layout", "random", "depth_clamps", "pl_deltas", "wide"]
assert sorted(ORDER) == sorted(cc.SANITIZED)


def build(csrc, out, san=""):
    """tests/emu_calls against the header in `csrc` -> None, or the compiler's last words"""
    cc_ = subprocess.run(["make", "-C", os.path.join(TESTS, "emu_calls"), "-s", "-B", "CSRC=" + csrc, "SAN=" + san, "OPT=-O2", "OUT=" + out],
                         capture_output=True, text=True)
    return None if cc_.returncode == 0 else cc_.stderr[-300:]


def first_difference(exe, tmp, names):
    """the first set of `names` the program at `exe` gets wrong, and how -> (name, how) or None"""
    for name in names:
        for k, (case, want) in enumerate(zip(cc.cases(name), cc.expected(name))):
            path, out = os.path.join(tmp, "%s.%d.case" % (name, k)), os.path.join(tmp, "%s.%d.out" % (name, k))
            cc.write_case(path, case)
            try:
                run = subprocess.run([exe, path, out], capture_output=True, timeout=300)
            except subprocess.TimeoutExpired:
                return name, "does not end"
            if run.returncode != 0:
                return name, "the program dies (exit status %d)" % run.returncode
            if cc.differences(case, want, cc.read_result(out, case)):
                return name, "differs from the restatement"
    return None


def run_one(mutant, names=None):
    tmp = tempfile.mkdtemp(prefix="gtx_calls_mutant_")
    try:
        text = open(HEADER).read()
        if text.count(mutant["find"]) != 1:
            raise SystemExit("mutant %s: its text occurs %d times in the header (must be 1)" % (mutant["id"], text.count(mutant["find"])))
        open(os.path.join(tmp, "score_core.hpp"), "w").write(text.replace(mutant["find"], mutant["replace"], 1))
        exe = os.path.join(tmp, "emu_calls")
        error = build(tmp, exe, mutant.get("build", ""))
        if error is not None:
            return dict(id=mutant["id"], status="does not compile", detail=error)
        found = first_difference(exe, tmp, names or ORDER)
        if found is None:
            return dict(id=mutant["id"], status="SURVIVED")
        return dict(id=mutant["id"], status="killed", by=found[0], how=found[1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def unmodified_passes(names):
    """the header as it is, built the same way, over `names` -> None, or what went wrong"""
    tmp = tempfile.mkdtemp(prefix="gtx_calls_plain_")
    try:
        exe = os.path.join(tmp, "emu_calls")
        error = build(os.path.dirname(HEADER), exe)
        return error if error is not None else first_difference(exe, tmp, names)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    mutants = json.load(open(os.path.join(HERE, "mutants.json")))
    if a.only:
        mutants = [m for m in mutants if m["id"] in a.only]
    for name in ORDER:  # (the restatement's results once, before the threads ask for them)
        cc.expected(name)
    wrong = unmodified_passes(ORDER)
    if wrong is not None:
        raise SystemExit("the unmodified header fails: %s" % (wrong,))
    with ThreadPoolExecutor(a.j) as pool:
        results = list(pool.map(run_one, mutants))
    for r in results:
        print("%-36s %-16s %s" % (r["id"], r["status"], r.get("by", r.get("detail", "")) + (" -- " + r["how"] if "how" in r else "")))
    killed = sum(r["status"] in ("killed", "does not compile") for r in results)
    print("%d of %d mutants killed" % (killed, len(results)))
    if not a.only:
        with open(os.path.join(HERE, "audit.json"), "w") as f:
            json.dump(dict(cases=ORDER, killed=killed, total=len(results), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
