#!/usr/bin/env python3
"""Mutation audit of the device record stream's kernel text (graphtyper_amd/csrc/gtx_dstream_dev.hpp): do the record sets of
tests/dstream_cases.py notice a one-place misreading of gtx_stream_push -- which records are kept, which are duplicates and of whom,
the tasks' meta and plane rows, who pairs with whom, what waits, and why a push fails?  All of it on the host, through
tests/emu_dstream; a case notices when dstream_cases.judge says how a push differs from the definition, or the program dies.  A
case's name is "<set>/<wavefronts>": every set at 1, 2, 3 and 300 wavefronts, as tests/test_dstream_emu.py runs them.  How an audit
runs: tests/mutation_audit.py.  Results go to audit.json (committed; tests/test_dstream_mutants.py checks it against mutants.json and
re-runs a sample).

    python tests/dstream_mutants/run_audit.py [-j 8] [--only ID ...]"""
import functools
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import dstream_cases as dc  # noqa: E402
import mutation_audit  # noqa: E402

WAVES = (1, 2, 3, 300)
# the cheap sets first, so that a mutant's recorded killer is quick to run again; the 5 000 records last
SETS = ["zero_first", "front_ops", "hint", "fail_order", "groups", "dropped_names", "filters", "dups_flags", "orient", "limits", "pieces", "dups_runs", "rows",
        "pairs_apart", "pairs_many", "model"]
ORDER = ["%s/%d" % (name, waves) for name in SETS for waves in WAVES]
NAMES = ["%s/%d" % (name, waves) for name in sorted(dc.SETS) for waves in WAVES]  # what tests/test_dstream_emu.py runs


def judge(name, run):
    """the set of `name` through the program behind `run` over the wavefronts of `name`"""
    which, waves = name.split("/")
    return dc.judge(which, functools.partial(dc.through, run, int(waves)))


AUDIT = mutation_audit.KernelAudit(HERE, "gtx_dstream_dev.hpp", "emu_dstream", types.SimpleNamespace(judge=judge), ORDER, covers=NAMES,  # (sorted(ORDER) == sorted(covers), or no audit)
                                   also=("graph_dev.hpp",))  # (the wave policy and the plane layout, unchanged)

if __name__ == "__main__":
    AUDIT.main()
