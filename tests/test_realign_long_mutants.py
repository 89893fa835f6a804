"""The committed mutation audit of the long realignment kernel's text (tests/realign_long_mutants/): audit.json has to cover every
mutant of mutants.json, each noticed by a case of tests/realign_long_cases.py unless the list itself says why it computes the same
function; and a sample is re-run here (build tests/emu_realign_long against the changed header -- a plain host build of a
stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/realign_long_mutants/run_audit.py."""
import mutation_audit
import realign_long_cases as lc
from realign_long_mutants.run_audit import AUDIT

SAMPLE = ("cb_bits_9", "limit_in_force_ignored", "rows_behind_the_read_pay_nothing")


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=lc.AUDIT_CASES, floor=30, survivors_ok=lambda n: n <= 4)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
