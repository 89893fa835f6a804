"""The committed mutation audit of the scoring kernels' text (tests/score_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a case set of tests/score_cases.py unless the list itself says why it computes the same function on
every input within the contract; and a sample is re-run here (build tests/emu_score against the changed header -- a plain host
build of a stand-alone program -- and run the set recorded as its killer) so that the record cannot go stale silently.  The full
audit: python tests/score_mutants/run_audit.py."""
import itertools

import mutation_audit
import score_cases as sc
import score_ref as ref
from score_mutants.run_audit import AUDIT

SAMPLE = ("pairs_min_93", "sv_ratio_ge", "conn_seven_over_weight")
# the one-line changes the audit has to hold at the least
REQUIRED = {"single_min_93", "single_min_95", "single_tie_le", "single_return_1", "pairs_min_93", "pairs_min_95", "alt_calls_gt", "mm_cap_11", "mm_cap_9",
            "tie_returns_1", "rule63_second_64", "rule63_second_62", "good_size_62", "good_size_64", "ratio_ge_005", "ratio_ge_0025", "sv_size_91", "sv_size_89",
            "sv_ratio_ge", "hq_ratio_ge", "cov_alt_keeps_alt", "cov_ref_not_sticky", "cov_other_swapped", "cov_same_is_other", "members_le_2",
            "lowest_of_word", "sort_descending", "overlap_start_2", "overlap_end_4", "eps_base_11", "eps_unique_2", "eps_mapq_1", "eps_fully_2",
            "eps_overlap_2", "eps_floor_7", "eps_minus_3", "conn_weight_4", "conn_seven_over_weight", "conn_cross_63", "conn_near_lt",
            "conn_near_b1_stride", "stat_strand_swapped", "stat_mismatches_16_bits", "stat_stride_5", "score_one_gets_eps", "gts_multi_ref_counts_alt",
            "gts_multi_alt_pp_always", "gts_ref_counts_pp", "table_one_more", "conn_cap_gt", "cross_direction", "cross_shared_site_kept", "conn_first_128", "conn_second_128", "cross_first_128",
            "cross_second_128"}


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=sc.AUDITED, floor=100, survivors_ok=lambda n: n == 6, required=REQUIRED)


def test_the_survivors_compute_the_same_function():
    """the reasons mutants.json gives for the two redundant lines of the pair comparison, over every combination of lengths around its
    constants: where the first 63-rule or `M1 >= 94 && M1 > M2` decides, no line behind it could have returned anything but 1"""
    geno = lambda t: ref.Geno([ref.Path(0, 0, 0, t - 1, 0, [])] if t else [], t, 150, False)  # noqa: E731
    lengths = (0, 1, 62, 63, 64, 93, 94, 95, 149)
    for t in itertools.product(lengths, repeat=4):
        which, rule = ref.compare_pairs(*(geno(x) for x in t))
        m1, m2 = max(t[:2]), max(t[2:])
        if rule == "rule63" and which == 1 or rule == "longer" and which == 1 and m1 == 94:  # (where the two mutants change the line's verdict)
            second_rule = m1 == 0 and t[2] >= 63 and t[3] >= 63
            equal_maxima = m1 >= 94 and m2 >= 94
            assert not second_rule and not equal_maxima and not (m2 >= 94 and m2 > m1)  # nothing but `return 1` is left
    # conn_first_63, conn_first_128, conn_second_128: a set of 64 alleles or more has weight >= 64 with any other set, and 6 / weight is 0
    assert all(6 // (k * n) == 0 for k in (64, 65, 100, 2559) for n in range(1, 65))


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
