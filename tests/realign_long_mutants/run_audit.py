#!/usr/bin/env python3
"""Mutation audit of the long realignment kernel's text (graphtyper_amd/csrc/gtx_realign_long_dev.hpp): do the pair sets, the
entry-point cases and the planted pairs of tests/realign_long_cases.py notice a one-line misreading of the wider value, of the two
limits, of the rows per lane and their dispatch, of the early return or of the final maximum?  All of it on the host, through
tests/emu_realign_long; a case notices when it differs from what is expected or the program dies.  How an audit runs:
tests/mutation_audit.py.  Results go to audit.json (committed; tests/test_realign_long_mutants.py checks it against mutants.json
and re-runs a sample).

    python tests/realign_long_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import mutation_audit  # noqa: E402
import realign_long_cases as lc  # noqa: E402

# the cheap cases first, so that a mutant's recorded killer is quick to run again
ORDER = ["mixed_batch_257", "mixed_batch", "short_row", "offsets_by_hand", "rows_exact", "row_boundaries_wide_dirty", "rows_behind_the_read", "clips", "ties",
         "row_boundaries", "planted", "column_boundaries", "short_simulated", "both_limits"]
AUDIT = mutation_audit.KernelAudit(HERE, "gtx_realign_long_dev.hpp", "emu_realign_long", lc, ORDER, covers=lc.AUDIT_CASES, also=("gtx_realign_dev.hpp",))

if __name__ == "__main__":
    AUDIT.main()
