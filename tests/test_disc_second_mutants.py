"""The committed mutation audit of the second pass's kernel text (tests/disc_second_mutants/): audit.json has to cover every
mutant of mutants.json, each noticed by a case set or a launch shape of tests/disc_second_cases.py unless the list itself says why
it must survive; and a sample is re-run here (build tests/emu_disc_second against the changed header -- a plain host build of a
stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/disc_second_mutants/run_audit.py."""
import disc_second_cases as sc
import mutation_audit
from disc_second_mutants.run_audit import AUDIT

SAMPLE = ("region_n_is_a_mismatch", "global_max_begins_at_1", "lookup_ignores_the_type")
REQUIRED = {"score_match_2", "score_mismatch_3", "score_gap_open_6", "score_gap_extend_2", "score_clip_4", "read_n_is_a_mismatch", "region_n_is_a_mismatch",
            "clip_begin_is_op_0_or_1", "insertion_not_cut_at_the_read", "empty_insertion_pays", "deletion_bound_gt", "bucket_max_begins_at_0",
            "global_max_begins_at_1", "empty_bucket_global_0", "wants_1_le", "wants_2_le", "wants_3_ge", "wants_4_ge", "descent_ge", "descent_stops_at_bucket_1",
            "pad_49", "pad_51", "begin_padded_one_pad", "end_padded_one_pad", "anti_support_keeps_out", "lookup_takes_later_positions", "lookup_ignores_the_type",
            "lookup_takes_longer_entries", "lookup_ignores_the_last_letter"}


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=list(sc.SETS) + list(sc.LAUNCHES), floor=90, survivors_ok=lambda n: n <= 1, required=REQUIRED)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
