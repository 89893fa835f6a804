"""The committed mutation audit of the discovery events kernel's text (tests/disc_events_mutants/): audit.json has to cover every
mutant of mutants.json, each noticed by a case set or a launch-level case of tests/disc_event_cases.py unless the list itself says
why it must survive; and a sample is re-run here (build tests/emu_disc_events against the changed header -- a plain host build of
a stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/disc_events_mutants/run_audit.py."""
import disc_event_cases as dc
import mutation_audit
from disc_events_mutants.run_audit import AUDIT

SAMPLE = ("block_mask_gt_32", "deletion_limit_one_more", "overflow_to_the_event_counter")


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=list(dc.SETS) + list(dc.LAUNCHES), floor=30, survivors_ok=lambda n: n <= 4)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
