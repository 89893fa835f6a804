#!/usr/bin/env python3
"""Mutation audit of the record walk's kernel text (graphtyper_amd/csrc/gtx_disc_bam_walk_dev.hpp): do the streams of
tests/disc_bam_walk_cases.py notice a one-place misreading of walk, guess, resolve or emit -- where a record begins, which of the
chain's two tests and the two verdicts speaks first, what a turn of 64 leaves behind its first bad record, which guess is adopted and
which segment walked again, what the tables and the totals hold?  All of it on the host, through tests/emu_disc_bam_walk; a case
notices when disc_bam_walk_cases.judge says how a walk differs from the definition, or the program dies or does not end.  A case's
name is "<set>/<wavefronts>": every set at 1, 2, 3 and 300 wavefronts, as tests/test_disc_bam_walk_emu.py runs them.  How an audit
runs: tests/mutation_audit.py.  Results go to audit.json (committed; tests/test_disc_bam_walk_mutants.py checks it against
mutants.json and re-runs a sample).

    python tests/disc_bam_walk_mutants/run_audit.py [-j 8] [--only ID ...]"""
import functools
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import disc_bam_walk_cases as wc  # noqa: E402
import mutation_audit  # noqa: E402

WAVES = (1, 2, 3, 300)
# the cheap sets first, so that a mutant's recorded killer is quick to run again; the streams of 100 KB last
SETS = ["smallest", "align", "straddle", "resync", "span", "damage", "decoy", "precedence", "order", "odd", "counts", "turns"]
ORDER = ["%s/%d" % (name, waves) for name in SETS for waves in WAVES]
NAMES = ["%s/%d" % (name, waves) for name in sorted(wc.SETS) for waves in WAVES]  # what tests/test_disc_bam_walk_emu.py runs
ENDS_IN = 20  # seconds: a walk that is given no exit (a mutant of the loops' conditions) goes round for ever; every case takes well under one


def judge(name, run):
    """the set of `name` through the program behind `run` over the wavefronts of `name`"""
    which, waves = name.split("/")
    return wc.judge(which, functools.partial(wc.through, functools.partial(run, timeout=ENDS_IN), int(waves)))


AUDIT = mutation_audit.KernelAudit(HERE, "gtx_disc_bam_walk_dev.hpp", "emu_disc_bam_walk", types.SimpleNamespace(judge=judge), ORDER, covers=NAMES,  # (sorted(ORDER) == sorted(covers), or no audit)
                                   also=("graph_dev.hpp",))  # (the wave policy, unchanged)

if __name__ == "__main__":
    AUDIT.main()
