"""The committed mutation audit of the record walk's kernel text (tests/disc_bam_walk_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a set of tests/disc_bam_walk_cases.py at some number of wavefronts unless the list itself says why it
must survive; and a sample is re-run here (build tests/emu_disc_bam_walk against the changed header -- a plain host build of a
stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  No mutant ever runs on a
device.  The full audit: python tests/disc_bam_walk_mutants/run_audit.py.

The survivors: at most 16 may, each with an argument of equivalence from the text.  The committed record has 206 mutants, 190 noticed
and 16 that survive: the two bounds of one walk, each of which the other makes idle (the count a walk wants: dropped from the loop,
room without the reads taken, take without room, the break behind take < sound, emit's count unbounded; the limit: emit's walk up to
n_bytes), a turn of 63 records, the bound of 5 for the 4 bytes of a block word, the block's test unsigned (differs behind 2 GB only),
the sign test of l_seq in front of a 64-bit sum, that sum in 32 bits behind the sign test, the entry, base and cigar_base a guess leaves, the entry and
exit of a segment behind the bad record, and emit's skip of a segment without records."""
import disc_bam_walk_cases as wc
import mutation_audit
from disc_bam_walk_mutants.run_audit import AUDIT, NAMES, WAVES

SAMPLE = ("ch_block_lt_33", "ex_chain_before_counts", "ct_long_judged_first")  # killed by smallest, order and precedence
SURVIVORS = 16
FLOOR = 90
REQUIRED = {
    # what the sets `order`, `precedence`, `smallest`, `odd` and `turns` were made for
    "ex_chain_before_counts", "ct_long_judged_first", "ch_block_lt_33", "ct_codes_floor", "tk_words_behind_take_kept", "tk_len_behind_take_kept", "tk_zero_from_take_plus_1",
    # the chain's tests and their constants, the turn, the limits
    "ch_left_lt_3", "ch_left_lt_5", "ch_block_lt_31", "ch_block_unsigned", "ch_fit_ge", "ch_fit_minus_3", "ch_fit_minus_5", "ch_step_plus_3", "ch_step_plus_5", "wk_turn_of_65",
    "wk_turn_of_63", "wk_outer_limit_le", "wk_turn_limit_le",
    # the counts, the two verdicts, the fixed bytes
    "ct_fixed_31", "ct_fixed_33", "ct_name_dropped", "ct_cigar_dropped", "ct_cigar_times_2", "ct_cigar_times_8", "ct_codes_dropped", "ct_quals_dropped", "ct_sum_ge_block",
    "ct_sum_in_32_bits", "ct_signed_test_dropped", "ct_signed_test_le", "ct_long_gt_fffe", "ct_long_gt_10000", "ct_name_at_9", "ct_cigar_at_14", "ct_l_seq_at_20", "em_pos_at_0",
    "em_flag_at_12", "em_mapq_at_8",
    # a turn's take, the table entries, the accumulations, the exits
    "tk_first_bad_default_63", "tk_sound_is_k", "tk_sound_is_first_bad", "tk_room_ignored", "tk_take_is_the_larger", "em_offset_is_the_word", "em_index_without_base",
    "em_index_without_the_turns", "em_reserved_1", "em_l_qseq_is_n_cigar", "em_n_cigar_is_l_qseq", "em_cigar_off_without_base", "em_cigar_off_without_the_turns",
    "em_cigar_off_without_the_lanes", "ac_reads_assigned", "ac_cigar_assigned", "ac_longest_assigned", "ex_take_break_dropped", "ex_counts_test_dropped", "ex_chain_test_dropped",
    "ex_counts_goes_on", "ex_exit_is_the_limit", "sg_begin_of_segment_0", "sg_end_is_n_bytes",
    # guess, resolve, emit
    "gs_entry_0", "gs_base_1", "gs_cigar_base_1", "gs_exit_is_the_end", "gs_n_reads_0", "gs_max_l_seq_0", "gs_status_ok", "gs_bad_at_0", "gs_n_cigar_0", "rs_entry_le_end", "rs_every_guess_adopted",
    "rs_no_guess_adopted", "rs_adopted_exit_is_the_end", "rs_adopted_n_reads_0", "rs_adopted_max_l_seq_0", "rs_adopted_status_ok", "rs_adopted_bad_at_0", "rs_adopted_n_cigar_0",
    "rs_rewalked_exit_is_the_end", "rs_rewalked_n_reads_0", "rs_rewalked_max_l_seq_0", "rs_rewalked_status_ok", "rs_rewalked_bad_at_0", "rs_rewalked_n_cigar_0",
    "rs_rewalk_wants_64", "rs_reads_assigned", "rs_cigar_assigned", "rs_longest_assigned", "rs_status_not_kept", "rs_next_entry_is_the_end", "rs_base_0", "rs_cigar_base_0",
    "rs_behind_bad_branch_dropped", "rs_out_status_ok", "rs_out_longest_0", "rs_out_bad_at_0", "rs_out_n_cigar_0", "rs_out_n_reads_of_the_hits",
    "rs_out_hit_and_rewalked_swapped", "rs_out_rewalked_0", "et_empty_segment_walked", "et_empty_test_sense", "et_walk_from_the_start", "et_walk_to_n_bytes", "et_walk_wants_all",
    "et_base_0", "et_cigar_base_0"}


def test_the_audit_ran_what_the_tests_run():
    """tests/test_disc_bam_walk_emu.py: every set of SETS over 1, 2, 3 and 300 wavefronts"""
    import test_disc_bam_walk_emu
    marks = {m.args[0]: m.args[1] for m in test_disc_bam_walk_emu.test_every_walk_equals_the_definition.pytestmark}
    assert sorted(marks["name"]) == sorted(wc.SETS) and tuple(marks["waves"]) == WAVES
    assert sorted(NAMES) == sorted("%s/%d" % (name, waves) for name in marks["name"] for waves in marks["waves"]) and sorted(AUDIT.order) == sorted(NAMES)


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=NAMES, floor=FLOOR, survivors_ok=lambda n: n <= SURVIVORS, required=REQUIRED)


def test_the_survivors_are_few_and_each_says_why():
    """the bound on the record, counted off the list itself"""
    mutants, record = mutation_audit.load(AUDIT.here)
    survivors = [m["id"] for m in mutants if m.get("expect") == "survives"]
    assert len(survivors) == record["total"] - record["killed"] and all(len(m["why"]) > 80 for m in mutants if m["id"] in survivors)
    assert len(survivors) <= SURVIVORS and 10 * len(survivors) <= len(mutants), survivors


def test_a_mutant_built_with_a_sanitizer_is_a_stand_alone_program_and_says_why():
    mutants, _ = mutation_audit.load(AUDIT.here)
    assert all(m["build"] == "address" and m["why_build"] for m in mutants if "build" in m)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
