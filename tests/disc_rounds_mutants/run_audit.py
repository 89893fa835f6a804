#!/usr/bin/env python3
"""Mutation audit of the rounds' kernel text (graphtyper_amd/csrc/gtx_disc_rounds_dev.hpp): do the case sets, the launch shapes and
the decision rows of tests/disc_rounds_cases.py notice a one-place misreading of the reference's windows, decisions, lists, counters
and good-support rule?  All of it on the host, through tests/emu_disc_rounds; a case notices when disc_rounds_cases.judge says how
it differs from the restatement (tests/disc_rounds_ref.py) or from gtx_disc_realign_target, or the program dies.  How an audit
runs: tests/mutation_audit.py.  Results go to audit.json (committed; tests/test_disc_rounds_mutants.py checks it against
mutants.json and re-runs a sample).

    python tests/disc_rounds_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import disc_rounds_cases as rc  # noqa: E402
import mutation_audit  # noqa: E402

# the cheap cases first, so that a mutant's recorded killer is quick to run again; the aligner's limits (reads of 925 bases) last
ORDER = ["decide", "fields", "shape0", "shape1", "own_ends", "search", "purity", "copies"] + list(rc.LAUNCHES) + ["edges", "chain", "again", "shape4", "shape5",
                                                                                                          "shape63", "shape64", "shape65", "limits"]
AUDIT = mutation_audit.KernelAudit(HERE, "gtx_disc_rounds_dev.hpp", "emu_disc_rounds", rc, ORDER, covers=rc.NAMES,  # (sorted(ORDER) == sorted(covers), or no audit)
                                   also=("gtx_disc_second_dev.hpp", "gtx_realign_dev.hpp", "gtx_disc_events_dev.hpp"))  # (the emulation's other headers, unchanged)

if __name__ == "__main__":
    AUDIT.main()
