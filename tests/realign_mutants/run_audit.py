#!/usr/bin/env python3
"""Mutation audit of the realignment kernel's text (graphtyper_amd/csrc/gtx_realign_dev.hpp): do the pair sets and the entry
point's cases of tests/realign_cases.py notice a one-line misreading of the definition?  All of it on the host.

Every entry of mutants.json is one such change: a piece of the header's text that occurs once, and what replaces it.  For each,
the header is copied into a temporary directory and changed, tests/emu_realign is built against that directory as a plain
stand-alone program (make CSRC=<tmp> SAN= OPT=-O2; a mutant whose only fault is a load out of bounds names the sanitizer it is
built with instead, "build"), and the cases are run through it in ORDER until one differs from the restatement
(tests/realign_ref.py) or the program dies.  A mutant no case notices SURVIVES: either mutants.json says why it must
("expect": "survives"), or the pair sets have a gap.  Results go to audit.json (committed; tests/test_realign_mutants.py checks
it against mutants.json and re-runs a sample).

    python tests/realign_mutants/run_audit.py [-j 8] [--only ID ...]"""
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

import numpy as np  # noqa: E402

import realign_cases as rc  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402

HEADER = os.path.join(ROOT, "graphtyper_amd", "csrc", "gtx_realign_dev.hpp")
# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["exhaustive_ac", "exhaustive_acn", "ties", "codes_n_iupac", "no_padding", "bad_and_long", "bad_indices", "n_behind_the_read"] + sorted(rc.ENTRY) + \
        ["mismatch_runs_and_clips", "cross_n1", "cross_n2", "cross_n63", "cross_n64", "cross_n65", "reversed_pairs", "limits", "cross_n300", "indels_at_rows",
         "simulated", "cross_n2048"]
assert sorted(ORDER) == sorted(list(rc.SETS) + list(rc.ENTRY))


def build(csrc, out, san=""):
    """tests/emu_realign against the header in `csrc` -> None, or the compiler's last words"""
    cc = subprocess.run(["make", "-C", os.path.join(TESTS, "emu_realign"), "-s", "-B", "CSRC=" + csrc, "SAN=" + san, "OPT=-O2", "OUT=" + out],
                        capture_output=True, text=True)
    return None if cc.returncode == 0 else cc.stderr[-300:]


def first_difference(exe, tmp, names):
    """the first case of `names` the program at `exe` gets wrong, and how -> (name, how) or None"""
    for name in names:
        arrays, want = rc.case(name)
        case, out = os.path.join(tmp, name + ".case"), os.path.join(tmp, name + ".out")
        rc.write_case(case, *arrays)
        try:
            run = subprocess.run([exe, case, out], capture_output=True, timeout=300)
        except subprocess.TimeoutExpired:
            return name, "does not end"
        if run.returncode != 0:
            return name, "the program dies (exit status %d)" % run.returncode
        if rc.as_tuples(np.fromfile(out, gtx.REALIGN_RESULT)) != want:
            return name, "differs from the restatement"
    return None


def run_one(mutant, names=None):
    tmp = tempfile.mkdtemp(prefix="gtx_realign_mutant_")
    try:
        text = open(HEADER).read()
        if text.count(mutant["find"]) != 1:
            raise SystemExit("mutant %s: its text occurs %d times in the header (must be 1)" % (mutant["id"], text.count(mutant["find"])))
        open(os.path.join(tmp, "gtx_realign_dev.hpp"), "w").write(text.replace(mutant["find"], mutant["replace"], 1))
        exe = os.path.join(tmp, "emu_realign")
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
    tmp = tempfile.mkdtemp(prefix="gtx_realign_plain_")
    try:
        exe = os.path.join(tmp, "emu_realign")
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
        rc.case(name)
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
