#!/usr/bin/env python3
"""Mutation audit of the discovery events kernel's text (graphtyper_amd/csrc/gtx_disc_events_dev.hpp): do the case sets and the
launch-level cases of tests/disc_event_cases.py notice a one-line misreading of the reference's walk?  All of it on the host.

Every entry of mutants.json is one such change: a piece of the header's text that occurs once, and what replaces it.  For each,
the header is copied into a temporary directory and changed, tests/emu_disc_events is built against that directory as a plain
stand-alone program (make CSRC=<tmp> SAN= OPT=-O2; a mutant whose only fault is a load or a store out of bounds names the
sanitizer it is built with instead, "build"), and the cases are run through it in ORDER until one differs from the restatement
(tests/disc_events_ref.py), breaks a launch-level condition, or the program dies.  A mutant no case notices SURVIVES: either
mutants.json says why it must ("expect": "survives"), or the sets have a gap.  Results go to audit.json (committed;
tests/test_disc_events_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/disc_events_mutants/run_audit.py [-j 8] [--only ID ...]"""
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

import disc_event_cases as dc  # noqa: E402

HEADER = os.path.join(ROOT, "graphtyper_amd", "csrc", "gtx_disc_events_dev.hpp")
# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["ops", "group_edges", "insertions", "deletions", "short_rows", "quality_distance", "region_end", "codes", "event_counts", "long_deletion"] + \
        sorted(dc.LAUNCHES) + ["simulated"]
assert sorted(ORDER) == sorted(list(dc.SETS) + list(dc.LAUNCHES))


def build(csrc, out, san=""):
    """tests/emu_disc_events against the header in `csrc` -> None, or the compiler's last words"""
    cc = subprocess.run(["make", "-C", os.path.join(TESTS, "emu_disc_events"), "-s", "-B", "CSRC=" + csrc, "SAN=" + san, "OPT=-O2", "OUT=" + out],
                        capture_output=True, text=True)
    return None if cc.returncode == 0 else cc.stderr[-300:]


class Died(Exception):
    pass


def first_difference(exe, tmp, names):
    """the first case of `names` the program at `exe` gets wrong, and how -> (name, how) or None"""
    serial = [0]

    def runner(part, event_cap, counts, launches):
        serial[0] += 1
        case, out = os.path.join(tmp, "%d.case" % serial[0]), os.path.join(tmp, "%d.out" % serial[0])
        dc.write_case(case, part, dc.arrays(part), event_cap, counts, launches)
        try:
            run = subprocess.run([exe, case, out], capture_output=True, timeout=300)
        except subprocess.TimeoutExpired:
            raise Died("does not end")
        if run.returncode != 0:
            raise Died("the program dies (exit status %d)" % run.returncode)
        try:
            return dc.read_result(out, len(part.reads), event_cap)
        finally:
            os.remove(case)
            os.remove(out)

    for name in names:
        try:
            how = dc.judge(name, runner)
        except Died as e:
            how = str(e)
        if how is not None:
            return name, how
    return None


def run_one(mutant, names=None):
    tmp = tempfile.mkdtemp(prefix="gtx_disc_events_mutant_")
    try:
        text = open(HEADER).read()
        if text.count(mutant["find"]) != 1:
            raise SystemExit("mutant %s: its text occurs %d times in the header (must be 1)" % (mutant["id"], text.count(mutant["find"])))
        open(os.path.join(tmp, "gtx_disc_events_dev.hpp"), "w").write(text.replace(mutant["find"], mutant["replace"], 1))
        exe = os.path.join(tmp, "emu_disc_events")
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
    tmp = tempfile.mkdtemp(prefix="gtx_disc_events_plain_")
    try:
        exe = os.path.join(tmp, "emu_disc_events")
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
    for name in dc.SETS:  # (the restatement's results once, before the threads ask for them)
        dc.expected(name)
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
