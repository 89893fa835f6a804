#!/usr/bin/env python3
"""Mutation audit of the text behind the tables of the position-hinted pass (graphtyper_amd/csrc/index_build.hpp, and what gtx_host.cpp
adds to it on the host: the graph's part of the tables, the filters, the windows' list): do the hand-made graphs of
tests/hint_tables_cases.py notice a one-place misreading of a flag's definition, a constant, a bound, a shift or a field?  All of it on
the host, through tests/emu_hint_tables; a set notices when hint_tables_cases.judge says which word of which table differs from the
restatement over the oracle's index (tests/hint_tables_ref.py), or the program dies.  How an audit runs: tests/mutation_audit.py.
Results go to audit.json (committed; tests/test_hint_tables_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/hint_tables_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import hint_tables_cases as tc  # noqa: E402
import mutation_audit  # noqa: E402

# the small sets first, so that a mutant's recorded killer is quick to run again
ORDER = [n for n in tc.NAMES if n.startswith("size")] + ["letters", "sv", "repeats", "nodes", "plain", "far", "multi", "two", "pruned", "crowded_nb", "windows", "crowded"]
AUDIT = mutation_audit.KernelAudit(HERE, "index_build.hpp", "emu_hint_tables", tc, ORDER, covers=tc.NAMES, also=("gtx_host.cpp",))

if __name__ == "__main__":
    AUDIT.main()
