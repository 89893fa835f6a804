#!/usr/bin/env python3
"""Mutation audit of the realignment kernel's text (graphtyper_amd/csrc/gtx_realign_dev.hpp): do the pair sets and the entry
point's cases of tests/realign_cases.py notice a one-line misreading of the definition?  All of it on the host, through
tests/emu_realign; a case notices when it differs from the restatement (tests/realign_ref.py) or the program dies.  How an audit
runs: tests/mutation_audit.py.  Results go to audit.json (committed; tests/test_realign_mutants.py checks it against mutants.json
and re-runs a sample).

    python tests/realign_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import mutation_audit  # noqa: E402
import realign_cases as rc  # noqa: E402

# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["exhaustive_ac", "exhaustive_acn", "ties", "codes_n_iupac", "no_padding", "bad_and_long", "bad_indices", "n_behind_the_read"] + sorted(rc.ENTRY) + \
        ["mismatch_runs_and_clips", "cross_n1", "cross_n2", "cross_n63", "cross_n64", "cross_n65", "reversed_pairs", "limits", "cross_n300", "indels_at_rows",
         "simulated", "cross_n2048"]
AUDIT = mutation_audit.KernelAudit(HERE, "gtx_realign_dev.hpp", "emu_realign", rc, ORDER,
                                   covers=list(rc.SETS) + list(rc.ENTRY))  # (sorted(ORDER) == sorted(covers), or no audit)

if __name__ == "__main__":
    AUDIT.main()
