#!/usr/bin/env python3
"""Mutation audit of the unpack kernel's text (graphtyper_amd/csrc/gtx_disc_bam_dev.hpp): do the record sets of
tests/disc_bam_cases.py notice a one-place misreading of unpack_record, of the launch's addressing (BamBatch) or of the loop over a
wavefront's records -- where the name ends, which nibble is a base, which ballot is which word, where a row and a record's CIGAR
words begin?  All of it on the host, through tests/emu_disc_bam, which runs the text record by record over heap blocks and once more
over the launch's own arrays and insists on the same bytes; a case notices when disc_bam_cases.judge says how an output differs from
the definition, or the program dies.  The cases are those of tests/test_disc_bam_emu.py: every set, and the 257 records of `counts`
over 1, 2, 64 and 300 wavefronts ("waves/<n>").  How an audit runs: tests/mutation_audit.py.  Results go to audit.json (committed;
tests/test_disc_bam_mutants.py checks it against mutants.json and re-runs a sample).

    python tests/disc_bam_mutants/run_audit.py [-j 8] [--only ID ...]"""
import functools
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import disc_bam_cases as bc  # noqa: E402
import mutation_audit  # noqa: E402

WAVES = (1, 2, 64, 300)
# the cheap sets first, so that a mutant's recorded killer is quick to run again; the half megabyte of CIGAR words last
SETS = ["lengths", "codes", "shift", "cigars", "quals", "wide", "names", "counts", "far_cigar"]
ORDER = SETS + ["waves/%d" % waves for waves in WAVES]
NAMES = sorted(bc.SETS) + ["waves/%d" % waves for waves in WAVES]  # what tests/test_disc_bam_emu.py runs


def judge(name, run):
    """the set `name`, or the last file of `counts` over the wavefronts of "waves/<n>", through the program behind `run`"""
    if name.startswith("waves/"):
        f = bc.File(bc.files("counts")[-1].records, waves=int(name.split("/")[1]))
        return bc.file_differs(f, bc.through(run, f))
    return bc.judge(name, functools.partial(bc.through, run))


AUDIT = mutation_audit.KernelAudit(HERE, "gtx_disc_bam_dev.hpp", "emu_disc_bam", types.SimpleNamespace(judge=judge), ORDER, covers=NAMES,  # (sorted(ORDER) == sorted(covers), or no audit)
                                   also=("graph_dev.hpp", "gtx_disc_bam.hpp"))  # (the wave policy and DISC_BAM_SLACK, unchanged: the emulation takes both from the changed directory)

if __name__ == "__main__":
    AUDIT.main()
