#!/usr/bin/env python3
"""Mutation audit of the call kernel's text (call_cell, graphtyper_amd/csrc/score_core.hpp): do the case sets of
tests/calls_cases.py notice a one-line misreading of the reference's call?  All of it on the host, through tests/emu_calls; a set
notices when it differs from the restatement (tests/calls_ref.py) or the program dies.  How an audit runs: tests/mutation_audit.py.
mutants.json's survivors say why they compute the same function on every input within the contract.  Results go to audit.json
(committed; tests/test_calls_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/calls_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import calls_cases as cc  # noqa: E402
import mutation_audit  # noqa: E402

# the cheap sets first, so that a mutant's recorded killer is quick to run again (many_cells is the device's: not here)
ORDER = ["ties", "gq", "layout", "random", "depth_clamps", "pl_deltas", "wide"]
AUDIT = mutation_audit.KernelAudit(HERE, "score_core.hpp", "emu_calls", cc, ORDER, covers=cc.SANITIZED)  # (sorted(ORDER) == sorted(covers), or no audit)

if __name__ == "__main__":
    AUDIT.main()
