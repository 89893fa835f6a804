#!/usr/bin/env python3
"""Mutation audit of the discovery events kernel's text (graphtyper_amd/csrc/gtx_disc_events_dev.hpp): do the case sets and the
launch-level cases of tests/disc_event_cases.py notice a one-line misreading of the reference's walk?  All of it on the host,
through tests/emu_disc_events; a case notices when it differs from the restatement (tests/disc_events_ref.py), breaks a
launch-level condition, or the program dies.  How an audit runs: tests/mutation_audit.py.  Results go to audit.json (committed;
tests/test_disc_events_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/disc_events_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import disc_event_cases as dc  # noqa: E402
import mutation_audit  # noqa: E402

# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["ops", "group_edges", "insertions", "deletions", "short_rows", "quality_distance", "region_end", "codes", "event_counts", "long_deletion"] + \
        sorted(dc.LAUNCHES) + ["simulated"]
AUDIT = mutation_audit.KernelAudit(HERE, "gtx_disc_events_dev.hpp", "emu_disc_events", dc, ORDER,
                                   covers=list(dc.SETS) + list(dc.LAUNCHES))  # (sorted(ORDER) == sorted(covers), or no audit)

if __name__ == "__main__":
    AUDIT.main()
