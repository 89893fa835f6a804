#!/usr/bin/env python3
"""Mutation audit of the second pass's kernel text (graphtyper_amd/csrc/gtx_disc_second_dev.hpp): do the case sets and the launch
shapes of tests/disc_second_cases.py notice a one-line misreading of the reference's intake, buckets and rounds?  All of it on the
host, through tests/emu_disc_second; a case notices when it differs from the restatement (tests/disc_second_ref.py), breaks a
launch-level condition, or the program dies.  How an audit runs: tests/mutation_audit.py.  Results go to audit.json (committed;
tests/test_disc_second_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/disc_second_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import disc_second_cases as sc  # noqa: E402
import mutation_audit  # noqa: E402

# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["ops", "clips", "overruns", "lookups", "letters", "stream_order", "plan_rules", "candidates", "group_edges", "long_deletion"] + sorted(sc.LAUNCHES) + \
        ["simulated"]
AUDIT = mutation_audit.KernelAudit(HERE, "gtx_disc_second_dev.hpp", "emu_disc_second", sc, ORDER,
                                   covers=list(sc.SETS) + list(sc.LAUNCHES))  # (sorted(ORDER) == sorted(covers), or no audit)

if __name__ == "__main__":
    AUDIT.main()
