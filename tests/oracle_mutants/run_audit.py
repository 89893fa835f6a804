#!/usr/bin/env python3
"""Mutation audit of the oracle's UNPINNED half (seed chaining with variants, walks, filters, orientation / pair selection,
explain_to_score, coverage, connections, the SV coverage model): does the ground-truth suite -- the tests that hold the oracle
to hand-worked or simulated truth, NOT to the product -- notice a one-token misreading of the reference?

Every entry of mutants.json is one such misreading: a unique piece of oracle text and what it is replaced by.  For each, the
oracle is copied, changed, compiled (g++ -O1) and the kill suite is run against it (GTO_LIB); a mutant that no test fails on
SURVIVES.  Results go to audit.json (committed; tests/test_oracle_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/oracle_mutants/run_audit.py [-j 6] [--only ID ...]"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import mutation_audit  # noqa: E402

KILL_SUITE = ["tests/test_oracle_truth.py", "tests/test_oracle_handworked.py", "tests/test_oracle_pinned.py", "tests/test_sv_vcf.py::test_coverage_model_hand_worked", "tests/test_sv_vcf.py::test_coverage_model_hand_worked_duplications_sizes_and_points",
              "tests/test_oracle_vcf_truth.py", "tests/test_oracle_handworked_pairs.py", "tests/test_oracle_merge.py", "tests/test_oracle_truth_walks.py", "tests/test_oracle_truth_pairs.py"]


def suite_passes(suite=None, lib=None):
    """the tests of `suite` (KILL_SUITE) against the oracle built at `lib` (the tree's own) -> None, or the first test that fails
    ("crash" when none is named), or "timeout ..." after 300 s"""
    try:
        t = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + list(suite or KILL_SUITE), cwd=ROOT,
                           env=dict(os.environ, GTO_LIB=lib) if lib else None, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        return "timeout (a loop that no longer ends)"
    if t.returncode == 0:
        return None
    failed = [l.split(" ")[1] for l in t.stdout.splitlines() if l.startswith("FAILED ") or l.startswith("ERROR ")]
    return failed[0] if failed else "crash"


def changed_oracle(change, suite=None):
    """a copy of oracle/ changed by change(directory), compiled (g++ -O1) and held to `suite` (KILL_SUITE) -> ("does not compile",
    the compiler's last words), ("SURVIVED", None) or ("killed", what suite_passes names)"""
    with tempfile.TemporaryDirectory(prefix="gto_mutant_") as tmp:
        work = os.path.join(tmp, "oracle")
        shutil.copytree(os.path.join(ROOT, "oracle"), work, ignore=shutil.ignore_patterns("*.so", "_ref"))
        change(work)
        so = os.path.join(tmp, "libgto_mutant.so")
        cc = subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-w", "-shared", "-o", so, os.path.join(work, "gto_capi.cpp")], capture_output=True, text=True)
        if cc.returncode != 0:
            return "does not compile", cc.stderr[-300:]
        by = suite_passes(suite, so)
        return ("SURVIVED", None) if by is None else ("killed", by)


def apply(mutant, oracle_dir):
    path = os.path.join(oracle_dir, mutant["file"])
    text = mutation_audit.changed(open(path).read(), mutant, mutant["file"])
    open(path, "w").write(text)


def run_one(mutant, suite=None):
    status, what = changed_oracle(lambda work: apply(mutant, work), suite)
    if status == "does not compile":
        return dict(id=mutant["id"], status=status, detail=what)
    return dict(id=mutant["id"], status=status, by=[what]) if what else dict(id=mutant["id"], status=status)


def main():
    a = mutation_audit.options(6).parse_args()
    wrong = suite_passes()
    if wrong is not None:
        raise SystemExit("the kill suite fails on the unmodified oracle: %s" % wrong)
    mutation_audit.audit(HERE, run_one, a.j, a.only, kill_suite=KILL_SUITE)


if __name__ == "__main__":
    main()
