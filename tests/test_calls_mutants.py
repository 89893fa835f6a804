"""The committed mutation audit of the call kernel's text (tests/calls_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a case set of tests/calls_cases.py unless the list itself says why it computes the same function on
every input within the contract; and a sample is re-run here (build tests/emu_calls against the changed header -- a plain host
build of a stand-alone program -- and run the set recorded as its killer) so that the record cannot go stale silently.  The full
audit: python tests/calls_mutants/run_audit.py."""
import decimal

import calls_cases as cc
import calls_ref as ref
import mutation_audit
from calls_mutants.run_audit import AUDIT

SAMPLE = ("last_zero_is_gt", "next_lowest_from_254", "cell_stride_3")
# the one-line changes the audit has to hold at the least
REQUIRED = {"cap_le_255", "all_equal_test_dropped", "last_zero_is_gt", "one_zero_gives_gq_0", "next_lowest_from_254", "next_lowest_le", "ambiguous_sat16",
            "alt_words_sat8", "ref_inner_clamp_dropped", "ref_outer_clamp_dropped", "alt_without_ambiguous", "ref_keeps_ambiguous_alt",
            "alt_sum_from_allele_0", "cell_stride_3", "scores_at_allele_off", "cov_at_tri_off", "cov_stride_total_tri", "counters_2_1_3", "x_lt_y",
            "sample_and_hap_swapped", "constant_3_0103"}


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=cc.SANITIZED, floor=40, survivors_ok=lambda n: n == 5, required=REQUIRED)


def test_the_survivors_compute_the_same_function():
    """the reasons mutants.json gives, as far as they are arithmetic: over every delta two uint16 scores can have"""
    c = float("3.01029995663981195213738894724493026768189881462108541")

    def llround(x):
        return int(decimal.Decimal(x).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP))

    for delta in range(0x10000):
        score, short = llround(float(delta) * c), llround(float(delta) * 3.0103)
        want = ref.pl_of(delta)
        assert (score if score < 255 else 255) == want == (score if score <= 255 else 255)  # cap_le_255
        assert (score if score < 254 else 255) == want                                       # cap_lt_254
        assert (short if short < 255 else 255) == want                                       # constant_3_0103
    assert llround(0.0 * c) == 0                                                             # all_equal_test_dropped


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
