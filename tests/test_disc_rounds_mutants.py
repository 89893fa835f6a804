"""The committed mutation audit of the rounds' kernel text (tests/disc_rounds_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a case set, a launch shape or the decision rows of tests/disc_rounds_cases.py unless the list itself
says why it must survive; and a sample is re-run here (build tests/emu_disc_rounds against the changed header -- a plain host build
of a stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/disc_rounds_mutants/run_audit.py.

The survivors: at most 8 may, each with an argument of equivalence from the text.  The committed record has 200 mutants, 192
noticed and 8 that survive: three guards the header itself calls never taken (the slot's room, the 2^31 clamp of a slot's size,
rounds_apply's look at the array's end), `end_padded >= REF_SIZE` against `>` (either arm of the ?: gives REF_SIZE), the walk
back's `pos > 0` (rp[0] is 0), `enters &&` in front of a max that only grows, leave-then-enter against enter-then-leave under sums
that commute, and the test of 50 that qual / depth >= 3.5 decides alone."""
import disc_rounds_cases as rc
import mutation_audit
from disc_rounds_mutants.run_audit import AUDIT
from test_disc_rounds_cases import ALL

SAMPLE = ("g_anti_count_32_bits", "ae_purity_end_4", "rd_num_ins_bound_plus_2")
REQUIRED = {
    # plain_window
    "pw_begin_one_pad", "pw_end_one_pad", "pw_end_padded_gt_ref_size", "pw_end_test_dropped",
    # apply_event: the first tests, the search, the purity test, a deletion's end test and loop, an insertion's copies, every mem_sync
    "ae_ref_pos_lt_0", "ae_pos_gt_seq_size", "ae_forward_bound_plus_2", "ae_forward_stops_one_early", "ae_back_bound_dropped", "ae_back_ge",
    "ae_purity_begin_2", "ae_purity_begin_4", "ae_purity_end_2", "ae_purity_end_4", "ae_purity_prev_plus_2", "ae_end_past_gt", "ae_end_past_dropped",
    "ae_end_differs_dropped", "ae_del_bound_le", "ae_del_step_32", "ae_del_step_128", "ae_ins_load_from_gt_pos", "ae_ins_store_from_gt_pos",
    "ae_ins_store_rp_from_pos_2", "ae_ins_rp_is_pos", "ae_ins_rp_is_ref_pos", "ae_ins_top_step_32", "ae_ins_top_step_128", "ae_ins_letters_step_128",
    "ae_ins_room_guard_dropped", "ae_ins_letters_guard_dropped", "ae_sync_del_loads", "ae_sync_del_stores", "ae_sync_ins_loads", "ae_sync_ins_stores",
    "ae_sync_ins_letters", "ww_sync_fill",
    # rounds_prepare, rounds_window_wave
    "rp_slots_lt_n_pairs", "rp_plain_insertion_is_d", "rp_own_insertion_is_d", "rp_need_upper_no_plus_1", "rp_own_table_guard_dropped", "rp_min_dropped",
    "ww_slot_ge_n_pairs", "ww_build_always", "ww_build_plain_only", "ww_own_without_k", "ww_target_even", "ww_target_odd", "ww_target_of_pair",
    "ww_windows_of_a_skipped_round",
    # rounds_decide
    "rd_db_is_1", "rd_de_gt_n", "rd_score_lt_is_not_better", "rd_equal_is_worse", "rd_overlap_left_gt", "rd_overlap_left_no_begin", "rd_overlap_right_lt",
    "rd_overlap_right_no_begin", "rd_pos_without_region_begin", "rd_pos_end_without_region_begin", "rd_clip_end_is_clip_end", "rd_num_ins_bound_plus_2",
    "rd_num_ins_bound_plus_0", "rd_num_ins_ne", "rd_better_makes_no_list", "rd_worse_makes_no_list", "rd_overlapping_makes_no_list",
    # count_entry, rounds_apply, the compaction
    "ce_anti_branch_dropped", "ce_multi_branch_dropped", "ce_support_counts_anti", "ce_reversed_mask_32", "ce_proper_pair_mask_1", "ce_mapq_le_255",
    "ce_max_when_leaving", "ce_max_is_a_store", "ra_enter_then_leave", "ra_to0_is_anti", "ra_applied_flag_sense", "ra_enter_lt", "ra_worse_is_multi",
    "ra_first_event_not_written", "ra_n_events_not_written", "ra_cap_guard_dropped", "cc_every_entry_to_coff", "cc_cap_guard_dropped",
    "cp_place_of_an_empty_list",
    # the final decision: every constant, every comparison, every width, depth's terms
    "gc_ins_2_is_4", "gc_ins_8_is_7", "gc_ins_over_9", "gc_del_3_is_4", "gc_del_10_is_9", "gc_del_over_11", "gc_arm1_hq_strict", "gc_arm1_count_strict",
    "gc_arm2_span_strict", "gc_arm2_hq_strict", "gc_arm2_count_strict", "gc_arm3_span_strict", "gc_arm3_hq_strict", "gc_arm3_count_strict", "gc_hq_count_32_bits",
    "g_hq_count_32_bits", "g_anti_count_32_bits", "g_multi_count_32_bits", "g_sequence_reversed_32_bits", "g_proper_pairs_32_bits", "g_max_mapq_32_bits",
    "g_depth_without_hq", "g_depth_without_anti", "g_depth_without_multi", "g_hq_le_6_strict", "g_reversed_le_0_strict",
    "g_reversed_ge_depth_strict", "g_pairs_le_4_strict", "g_hq_lt_10_le", "g_mapq_le_10_strict", "g_qual_times_2", "g_eps_6", "g_qual_lt_52", "g_qd_strict",
    "lq_gt01_gt_gt11"}


def test_the_audit_ran_what_the_tests_run():
    assert sorted(set(rc.NAMES) - set(rc.LAUNCHES) - {"decide"}) == sorted({name for name, _ in ALL})  # (the launches and the decision: test_disc_rounds_emu.py)


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=rc.NAMES, floor=200, survivors_ok=lambda n: n <= 8, required=REQUIRED)


def test_at_most_8_survive():
    """the bound on the record, counted off the list itself"""
    mutants, record = mutation_audit.load(AUDIT.here)
    survivors = [m["id"] for m in mutants if m.get("expect") == "survives"]
    assert len(survivors) == record["total"] - record["killed"] and all(m.get("why") for m in mutants if m["id"] in survivors)
    assert len(survivors) <= 8, survivors


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
