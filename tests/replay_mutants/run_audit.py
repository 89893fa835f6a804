#!/usr/bin/env python3
"""Mutation audit of the saturation replay's text -- mark_cells_at_guard and replay_cells (graphtyper_amd/csrc/score_replay.hpp) and the
replay branch of apply_recent with the calls that reach it (graphtyper_amd/csrc/score_core.hpp): do the item orders of
tests/replay_cases.py notice a one-line misreading?  All of it on the host, through tests/emu_replay; a set notices when the log, the
counts or an array differs from the restatement (score_ref.replay) or the program dies.  How an audit runs: tests/mutation_audit.py.
mutants.json's survivors say why they compute the same function on every input.  Results go to audit.json (committed;
tests/test_replay_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/replay_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import mutation_audit  # noqa: E402
import replay_cases as rc  # noqa: E402

# the cheap sets first, so that a mutant's recorded killer is quick to run again
ORDER = ["order_within_item", "halves", "masks", "many_cells", "tables_and_forms", "log_growth", "aligned_records", "boundary"]
AUDIT = mutation_audit.KernelAudit(HERE, "score_replay.hpp", "emu_replay", rc, ORDER, covers=rc.AUDITED, also=["score_core.hpp"])

if __name__ == "__main__":
    AUDIT.main()
