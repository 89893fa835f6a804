"""The committed mutation audit of the unpack kernel's text (tests/disc_bam_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a record set of tests/disc_bam_cases.py unless the list itself says why it must survive; and a sample is
re-run here (build tests/emu_disc_bam against the changed header -- a plain host build of a stand-alone program -- and run the case
recorded as its killer) so that the record cannot go stale silently.  No mutant ever runs on a device.  The full audit:
python tests/disc_bam_mutants/run_audit.py.

The survivors: at most 3 may.  The committed record has 109 mutants, 106 noticed and 3 that survive: the low nibble taken without its
mask (the four bit tests read bits 0 to 3 alone), and the two row products made in 32 bits, which differ only for rows behind byte
2^32 of their arrays -- more than a host case can hold; tests/test_gpu_disc_bam.py::test_rows_behind_2_32_bytes is their check, on the
device."""
import disc_bam_cases as bc
import mutation_audit
from disc_bam_mutants.run_audit import AUDIT, NAMES, WAVES

SAMPLE = ("nm_length_7_bits", "ad_cigar_off_16_bits", "sq_bytes_floor")  # killed by names, far_cigar and lengths
SURVIVORS = 3
FLOOR = 40
REQUIRED = {
    "nm_length_at_9", "nm_length_at_7", "nm_name_at_31", "nm_name_at_33", "nm_length_signed", "nm_length_7_bits", "cg_bytes_times_2", "cg_bytes_times_8", "sq_bytes_floor",
    "sq_bytes_plus_2", "gr_groups_of_32_bytes", "gr_groups_plus_1", "gr_loop_le", "gr_loop_last_pair_left", "bs_32_a_turn", "bs_without_the_lane", "bs_le_len", "bs_one_short",
    "bs_byte_is_the_next", "bs_byte_a_base", "nb_swapped", "nb_always_high", "nb_low_mask_7", "nb_high_shift_5", "bt_0_is_2", "bt_1_is_4", "bt_2_is_8", "bt_3_is_1",
    "st_row_4_words_a_turn", "st_word_0_is_plane_1", "st_word_1_is_plane_0", "st_word_2_is_plane_3", "st_word_3_is_plane_2", "st_word_4_low_half", "st_word_5_shift_31",
    "st_word_6_shift_33", "st_word_7_shift_16", "st_second_group_le", "st_second_group_never", "ql_stride_128", "ql_up_to_len", "ql_le_len", "ql_one_short", "ql_fill_255",
    "cw_stride_128", "cw_le", "cw_byte_0_is_1", "cw_byte_1_is_0", "cw_byte_1_shift_16", "cw_byte_2_is_3", "cw_byte_2_shift_8", "cw_byte_3_is_2", "cw_byte_3_shift_23",
    "ad_record_at_the_word", "ad_row_a_group_each", "ad_row_product_32_bits", "ad_qual_4_bytes_each", "ad_qual_product_32_bits", "ad_cigar_off_16_bits", "ad_cigar_off_ignored",
    "lp_le", "lp_one_short", "lp_stride_plus_1", "lp_from_first_plus_1"}


def test_the_audit_ran_what_the_tests_run():
    """tests/test_disc_bam_emu.py: every set of SETS, and the 257 records of `counts` over 1, 2, 64 and 300 wavefronts"""
    import test_disc_bam_emu
    names = {m.args[0]: m.args[1] for m in test_disc_bam_emu.test_every_byte_equals_the_definition.pytestmark}["name"]
    waves = {m.args[0]: m.args[1] for m in test_disc_bam_emu.test_the_records_over_any_number_of_wavefronts.pytestmark}["waves"]
    assert sorted(names) == sorted(bc.SETS) and tuple(waves) == WAVES
    assert sorted(NAMES) == sorted(list(names) + ["waves/%d" % w for w in waves]) and sorted(AUDIT.order) == sorted(NAMES)


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=NAMES, floor=FLOOR, survivors_ok=lambda n: n <= SURVIVORS, required=REQUIRED)


def test_the_survivors_are_few_and_each_says_why():
    """the bound on the record, counted off the list itself"""
    mutants, record = mutation_audit.load(AUDIT.here)
    survivors = [m["id"] for m in mutants if m.get("expect") == "survives"]
    assert len(survivors) == record["total"] - record["killed"] and all(len(m["why"]) > 80 for m in mutants if m["id"] in survivors)
    assert len(survivors) <= SURVIVORS, survivors


def test_a_mutant_built_with_a_sanitizer_is_a_stand_alone_program_and_says_why():
    mutants, _ = mutation_audit.load(AUDIT.here)
    assert all(m["build"] == "address" and m["why_build"] for m in mutants if "build" in m)


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
