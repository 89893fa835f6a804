"""The committed mutation audit of the realignment kernel's text (tests/realign_mutants/): audit.json has to cover every mutant
of mutants.json, each noticed by a pair set or an entry-point case of tests/realign_cases.py unless the list itself says why it
must survive; and a sample is re-run here (build tests/emu_realign against the changed header -- a plain host build of a
stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/realign_mutants/run_audit.py."""
import mutation_audit
import realign_cases as rc
from realign_mutants.run_audit import AUDIT

SAMPLE = ("lane_best_ge", "rows_behind_the_read_pay_nothing", "offsets_out_of_order_pass")


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=list(rc.SETS) + list(rc.ENTRY), floor=25, survivors_ok=lambda n: n <= 4)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
