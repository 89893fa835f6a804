#!/usr/bin/env python3
"""Mutation audit of the scoring kernels' text (compare_single, compare_pairs, geno_is_good, add_coverage, collect_recent,
explain_epsilon, apply_recent, emit_conn, score_item: graphtyper_amd/csrc/score_core.hpp): do the case sets of tests/score_cases.py
notice a one-line misreading of the reference?  All of it on the host, through tests/emu_score; a set notices when it differs from the
restatement (tests/score_ref.py) or the program dies.  How an audit runs: tests/mutation_audit.py.  mutants.json's survivors say why
they compute the same function on every input within the contract.  Results go to audit.json (committed; tests/test_score_mutants.py
checks it against mutants.json and re-runs a sample).

    python tests/score_mutants/run_audit.py [-j 8] [--only ID ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import mutation_audit  # noqa: E402
import score_cases as sc  # noqa: E402

# the cheap sets first, so that a mutant's recorded killer is quick to run again (many_items is the device's: not here)
ORDER = ["single", "pairs", "goodness", "epsilon_stats", "record_forms", "site_tables", "lanes", "coverage", "connections", "aligned_records"]
AUDIT = mutation_audit.KernelAudit(HERE, "score_core.hpp", "emu_score", sc, ORDER, covers=sc.AUDITED)  # (sorted(ORDER) == sorted(covers), or no audit)

if __name__ == "__main__":
    AUDIT.main()
