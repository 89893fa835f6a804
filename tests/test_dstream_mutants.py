"""The committed mutation audit of the device record stream's kernel text (tests/dstream_mutants/): audit.json has to cover every mutant
of mutants.json, each noticed by a record set of tests/dstream_cases.py at some number of wavefronts unless the list itself says why it
must survive; and a sample is re-run here (build tests/emu_dstream against the changed header -- a plain host build of a stand-alone
program -- and run the case recorded as its killer) so that the record cannot go stale silently.  No mutant ever runs on a device.  The
full audit: python tests/dstream_mutants/run_audit.py.

The survivors: at most 13 may, each with an argument of equivalence or unreachability from the text.  The committed record has 285
mutants, 272 noticed and 13 that survive: the early returns of walk and emit_items on a failing push (finish looks at `fail` first and
the slot beside the state is not adopted), four guards nothing reaches (perm[s - 1] < total, two parked mates of one key, the failing
record below n, the carried row's clamp to row_cap), the kept test in compare's last lanes() (the first one leaves a dropped record's
terms false) and in front of emit_tasks (a dropped record's rec meta is read by nobody), going on behind a key's end in walk (the sort left the key's elements side
by side), the sample of a parked entry, new or parked again (no kernel reads it), next_align_index of a failing push, and the tail of
the carried row."""
import dstream_cases as dc
import mutation_audit
from dstream_mutants.run_audit import AUDIT, NAMES, WAVES

SAMPLE = ("cmp_carry_have_dropped", "cl_order_row_before_long", "et_clip_code_mask_7")
SURVIVORS = 13
REQUIRED = {
    # forward_only, nib_bytes, differ16, same_key, dstream_failed
    "fo_unpaired_term_dropped", "fo_unpaired_sense", "fo_or_is_and", "fo_tid_term_dropped", "fo_tid_ne", "fo_lower_dropped", "fo_lower_ge", "fo_lower_1199",
    "fo_lower_1201", "fo_upper_dropped", "fo_upper_le", "fo_upper_1199", "fo_upper_1201", "fo_strands_dropped", "fo_strands_equal", "fo_own_strand_mask",
    "fo_mate_strand_mask", "fo_force_ignored", "fo_force_sense", "fo_bit_sense", "nib_bytes_floor", "nib_bytes_plus_2", "d16_x_dropped", "d16_y_dropped",
    "d16_z_dropped", "d16_w_dropped", "d16_equal_is_differ", "same_key_name_only", "same_key_rg_only", "failed_never",
    # classify: the arrays' defaults, every check, their order, the fail word, the kept bit and the count per wavefront
    "cl_tile_guard_dropped", "cl_tile_of_32", "cl_tile_stride", "cl_tile_stride_1", "cl_elem_is_0", "cl_wait_init_1", "cl_parked_split_le", "cl_parked_name",
    "cl_parked_rg", "cl_record_without_parked", "cl_name_32_bits", "cl_rg_8_bits", "cl_emit_init_1", "cl_partner_init_0", "cl_check_init_rg", "cl_rg_gt",
    "cl_rg_check_dropped", "cl_long_ge", "cl_long_check_dropped", "cl_row_nibbles_ge", "cl_row_nibbles_dropped", "cl_row_planes_dropped", "cl_row_planes_ge",
    "cl_row_planes_one_base_a_byte", "cl_order_long_before_rg", "cl_order_row_before_long", "cl_order_row_before_rg", "cl_fail_word_record_times_2",
    "cl_fail_word_without_record", "cl_fail_word_not_complemented", "cl_fail_word_check_first", "cl_kept_sense", "cl_kept_all", "cl_kept_in_is_i",
    "cl_kept_count_all", "cl_k_init_1", "cl_kept_seen_assigned", "cl_kept_seen_init_1", "cl_partial_of_wave_0",
    # compare: carried against previous kept record, each field, the steps and pieces of the rows, the ballot's byte, lane 0 of 8
    "cmp_failed_return_dropped", "cmp_tile_stride", "cmp_record_guard_dropped", "cmp_tile_of_4", "cmp_before_of_i", "cmp_before_always_carried",
    "cmp_before_is_i", "cmp_carried_test_sense", "cmp_carry_have_dropped", "cmp_carry_tid_dropped", "cmp_carry_pos_dropped", "cmp_carry_len_dropped",
    "cmp_carry_row_is_the_push", "cmp_prev_tid_dropped", "cmp_prev_pos_dropped", "cmp_prev_len_dropped", "cmp_prev_record_one_on", "cmp_prev_row_one_on",
    "cmp_fields_differ_is_no_head", "cmp_bytes_floor", "cmp_mine_is_row_0", "cmp_other_is_mine", "cmp_step_256", "cmp_piece_lane_mask_3",
    "cmp_piece_of_8_bytes", "cmp_cut_piece_skipped", "cmp_differ_may_be_reset", "cmp_piece_end_not_cut", "cmp_piece_end_le", "cmp_vector_on_a_cut_piece",
    "cmp_byte_loop_from_1", "cmp_byte_loop_one_short", "cmp_byte_eq", "cmp_ballot_7_lanes", "cmp_ballot_lane_0", "cmp_ballot_16_lanes",
    "cmp_ballot_not_shifted", "cmp_lane_0_of_4", "cmp_lane_1_of_8", "cmp_store_guard_dropped", "cmp_head_or_is_and", "cmp_final_kept_dropped", "cmp_head_sense",
    "cmp_head_in_is_i",
    # emit_tasks: whose align index and forward-only bit, the clip rule, both metas, the groups of the plane row and its tail
    "et_failed_return_dropped", "et_tile_stride", "et_record_guard_dropped", "et_not_kept_goes_on", "et_sub_of_4", "et_head_is_itself", "et_align_without_next",
    "et_align_task_of_the_record", "et_align_carried_is_next", "et_fo_of_the_record", "et_fo_carried_dropped", "et_fo_carried_is_0", "et_me_flag_without_fo",
    "et_me_mapq_is_score_diff", "et_me_pos_is_isize", "et_head_guard_dropped", "et_task_is_record", "et_clip_n_cigar_dropped", "et_clip_code_mask_7",
    "et_clip_code_5", "et_clip_code_0", "et_clip_shift_3", "et_clip_added", "et_clip_unused", "et_meta_flag_without_fo", "et_meta_tid_is_mtid",
    "et_meta_isize_0", "et_meta_l_qseq_0", "et_row_of_the_task", "et_bytes_floor", "et_groups_of_the_nibble_row", "et_group_stride_16", "et_last_group_left",
    "et_vector_on_a_cut_group", "et_vector_group_of_sub", "et_vector_words_swapped", "et_vector_z_is_w", "et_tail_not_zero", "et_tail_le", "et_byte_order",
    "et_word_index", "et_plane_row_of_the_record", "et_plane_pitch_of_the_nibble_row", "et_plane_group_of_sub", "et_plane_words_swapped",
    # gather_rg
    "gr_tile_stride", "gr_position_guard_dropped", "gr_element_is_position", "gr_key_of_position", "gr_key_0", "gr_key_8_bits",
    # walk: the key's first position, every branch of the two-state machine, the FIRST-bit clash
    "wk_failed_return_dropped", "wk_tile_stride", "wk_position_guard_dropped", "wk_position_0_guard_dropped", "wk_perm_guard_dropped",
    "wk_every_position_is_first", "wk_first_is_not_first", "wk_waiting_init_0", "wk_occurrences_from_the_second", "wk_occurrences_one_short",
    "wk_key_end_goes_on", "wk_key_end_sense", "wk_dropped_not_skipped", "wk_dropped_skipped_while_nothing_waits", "wk_dropped_skipped_while_something_waits",
    "wk_dropped_first_record_not_skipped", "wk_flag_of_a_parked_one", "wk_flag_of_record_x", "wk_paired_sense", "wk_paired_mask_2", "wk_waiting_flag_not_kept",
    "wk_unpaired_does_not_emit", "wk_first_branch_falls_through", "wk_two_parked_guard_dropped", "wk_clash_on_second_bit", "wk_clash_sense",
    "wk_clash_not_recorded", "wk_mate_does_not_emit", "wk_partner_is_itself", "wk_waiting_not_cleared", "wk_nothing_waits_at_the_end",
    # emit_items: both item shapes, both sources of a parked entry
    "ei_failed_return_dropped", "ei_tile_stride", "ei_element_guard_dropped", "ei_parked_room_guard_dropped", "ei_parked_room_le", "ei_wait_sense",
    "ei_parked_slot_0", "ei_parked_again_from_slot_0", "ei_parked_source_le", "ei_parked_name_0", "ei_parked_meta_of_record_0", "ei_parked_sample_0",
    "ei_parked_again_sample_0", "ei_parked_rg_0", "ei_emit_guard_dropped", "ei_parked_guard_dropped", "ei_record_without_parked", "ei_item_of_the_record",
    "ei_single_sense", "ei_single_first_of_record_0", "ei_single_second_index_0", "ei_single_second_flag_1", "ei_single_second_mapq_left",
    "ei_single_second_score_diff_left", "ei_single_second_pos_left", "ei_single_second_isize_left", "ei_pair_first_source_le", "ei_pair_first_parked_slot_0",
    "ei_pair_second_is_first", "ei_pair_swapped", "ei_sample_of_the_waiting_one", "ei_kind_1",
    # finish: the counts, both failure branches and their order, the carried record and its row
    "fn_n_parked_init_0", "fn_n_records_init_0", "fn_n_duplicated_init_0", "fn_why_mask_1", "fn_record_0", "fn_record_shift_1", "fn_l_qseq_0",
    "fn_l_qseq_of_record_0", "fn_record_guard_dropped", "fn_status_of_row_is_unsupported", "fn_status_sense", "fn_fail_ignored", "fn_n_align_without_the_last",
    "fn_n_items_without_the_last", "fn_n_wait_without_the_last", "fn_n_wait_of_the_parked", "fn_partial_step_128", "fn_partial_guard_dropped",
    "fn_partial_of_the_first_64", "fn_kept_assigned", "fn_clash_ignored", "fn_clash_status_capacity", "fn_clash_why_parked", "fn_order_parked_before_clash",
    "fn_parked_ge", "fn_parked_ignored", "fn_parked_status_arg", "fn_parked_why_clash", "fn_parked_n_not_set", "fn_ok_n_align_0", "fn_ok_n_items_0",
    "fn_ok_n_parked_not_set", "fn_ok_records_assigned", "fn_ok_duplicated_assigned", "fn_ok_duplicated_of_items", "fn_last_is_the_last_record",
    "fn_last_not_set", "fn_carry_starts_empty", "fn_carry_row_length_init_0", "fn_carry_have_0", "fn_carry_tid_0", "fn_carry_pos_0", "fn_carry_l_qseq_0",
    "fn_carry_align_index_0", "fn_carry_fo_0", "fn_carry_fo_whole_flag", "fn_carry_row_of_record_0", "fn_carry_bytes_floor", "fn_carry_bytes_not_clamped",
    "fn_next_align_not_advanced", "fn_next_align_of_a_failing_push", "fn_next_records_not_carried", "fn_next_duplicated_not_carried", "fn_row_copy_step_128",
    "fn_row_copy_of_byte_0", "fn_row_copy_one_short", "fn_row_tail_not_zero", "fn_carry_not_written"}


def test_the_audit_ran_what_the_tests_run():
    """tests/test_dstream_emu.py: every set of SETS over 1, 2, 3 and 300 wavefronts"""
    import test_dstream_emu
    marks = {m.args[0]: m.args[1] for m in test_dstream_emu.test_every_push_equals_the_definition.pytestmark}
    assert sorted(marks["name"]) == sorted(dc.SETS) and tuple(marks["waves"]) == WAVES
    assert sorted(NAMES) == sorted("%s/%d" % (name, waves) for name in marks["name"] for waves in marks["waves"]) and sorted(AUDIT.order) == sorted(NAMES)


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=NAMES, floor=150, survivors_ok=lambda n: n <= SURVIVORS, required=REQUIRED)


def test_at_most_one_in_ten_survives_and_each_says_why():
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
