"""The committed mutation audit of the text behind the tables of the position-hinted pass (tests/hint_tables_mutants/: index_build.hpp
and the tables' part of gtx_host.cpp): audit.json has to cover every mutant of mutants.json, each noticed by a set of
tests/hint_tables_cases.py -- the judge names the table, the position and the field that differ from the restatement over the oracle's
index -- unless the list itself says why it must survive; and a sample is re-run here (build tests/emu_hint_tables against the changed
text -- a plain host build of a stand-alone program -- and run the set recorded as its killer) so that the record cannot go stale
silently.  The full audit: python tests/hint_tables_mutants/run_audit.py.

The survivors: at most one mutant in twenty may, each with an argument of equivalence.  The committed record has 223 mutants, 212
noticed and 11 that survive: three that rest on a fact about the index which tests/hint_tables_ref.py asserts on every graph (an
interval lies under one set of sites: the site tests of `same`, of `known` and of the verdict), the 64-key rule on either side
(HINT_HE_CAP refuses sooner), the interval of an alternative allele's key (the sweep keeps that walk), an allele of no bases, the two
ends of "reaches into the allele" (on either side of each the window's path is the linear reference), the last node's site, and the
search's midpoint.  What the first runs found redundant in the text itself is no longer in the text."""
import hint_tables_cases as tc
import mutation_audit
from hint_tables_mutants.run_audit import AUDIT

SAMPLE = ("bh_filter_forgets_the_last_key", "hg_tail_five_alleles", "nok_nb_max_strict")
REQUIRED = {
    # plain: the flags of a lone SNP, its allele bytes and offset, HINT_SNP_GROUP, a SNP whose other k-mer occurs elsewhere, five alleles
    "fa_l1_of_two", "fa_r1_of_two", "fa_l1_reads_right", "fa_single_exact_without_par", "fa_alt_without_flag", "fa_alt_idx_shift", "fa_alt_verdict_not_asked",
    "fa_alt_verdict_of_allele_0", "fa_snp_offset_shift", "fa_refb_shift", "fa_nv_field", "fa_snp_left_from_15", "fa_snp_left_to_16", "fa_group_own_side_not_asked",
    "fa_group_other_side_not_asked", "fa_group_other_side_at_least", "fa_group_alleles_not_asked", "fa_snp_three_at_least", "fa_snp_len_any", "ev_any_allele", "ev_two_labels",
    "hg_tail_five_alleles", "hg_tail_three_alleles", "hg_tail_codes_shift", "hg_tail_node_is_next",
    # repeats: two labels, a neighbour on another interval
    "d1_first_base_unseen", "d1_and_for_or", "d1_several", "jk_same_any_start", "jk_same_any_end", "jk_left_group_one_short", "jk_right_group_first_only",
    "fa_single_any_allele",
    # far: every boundary of the codes, on both sides
    "fa_far_3_from_7", "fa_far_3_from_9", "fa_far_2_from_3", "fa_far_2_from_5", "fa_far_1_from_2", "fa_far_1_from_4", "fa_far_sides_swapped",
    "fa_far_right_group_is_left", "fa_far_bits_not_bases", "fa_far_max_not_min", "fa_far_counts_itself",
    # crowded: HINT_HE_CAP, the 64 keys, HINT_NB_MAX
    "nok_left_cap_strict", "nok_right_cap_strict", "nok_left_cap_dropped", "nok_right_cap_dropped", "fa_far_group_65", "fa_far_group_63",
    "nok_nb_max_strict", "nok_nb_max_dropped", "jk_nb_counts_keys",
    # multi, two
    "ol_five_labels", "ol_three_labels", "ol_one_label_refused", "ol_one_label_never", "ol_allele_8", "ol_allele_7_refused", "ol_mask_shifted", "ol_several_sites",
    "ol_reference_alone_counts", "fa_multi_needs_two", "fa_multi_site_not_set", "t2_allele_4", "t2_allele_3_refused", "t2_sets_swapped", "t2_high_set_at_bit_3",
    "t2_sites_two_apart", "t2_three_labels_at_least", "fa_two_neighbours_same", "fa_two_site_is_second", "nkn_reads_same_bit", "nkn_known_not_asked",
    "jk_among_first_own_only", "jk_known_any_start", "jk_known_any_end", "t2_any_other_site", "nok_reads_known_bit",
    # pruned: a k-mer that is in no key, keys whose labels lie elsewhere
    "fk_any_key_is_found", "fa_single_interval_not_asked", "t2_interval_not_asked", "ol_interval_not_asked", "lo_any_start", "lo_any_end",
    # letters, nodes
    "ia_t_is_not", "ia_r_is", "pc_15_is_nothing", "pc_other_is_n", "tb_g_is_3", "tb_c_is_0", "fa_kmer_past_the_end", "fa_kmer_end_strict", "hg_back_cap_254",
    "hg_tail_next_cap_256", "hg_tail_any_length", "hg_tail_any_letter",
    # windows
    "ww_nine_alleles", "ww_seven_alleles", "ww_ref_allele_63", "ww_plain_to_5", "ww_plain_to_3", "ww_plain_any_length", "ww_near_prev_31", "ww_near_prev_29",
    "ww_near_next_31", "ww_near_next_29", "ww_near_prev_only", "ww_near_next_only", "aw_allele_65", "aw_allele_63", "wc_start_one_off", "wc_allele_one_short",
    "wc_behind_161", "wc_behind_skips_len_a", "wc_past_the_end", "wc_own_site_keeps_ok", "wc_every_site_loses_ok", "wf_last_kmer_out", "wf_kmer_leaves_window",
    "wf_reaches_one_late", "wf_reaches_one_early", "wf_reaches_one_long", "wf_reaches_one_short", "wf_front_start_one_off", "wf_copy_past_the_end",
    "wf_end_label_one_short", "hw_site_win_count_shift", "hw_window_len_0_is_len_a",
    # sv, the filters, the planes
    "ww_sv_graph_gets_windows", "fa_multi_in_sv_graph", "fa_single_on_sv_variants", "fa_single_never_in_sv_graph", "hg_tail_in_sv_graph",
    "bh_filter_forgets_the_last_key", "bh_filter_right_is_left", "fa_near_free_one_side", "fa_near_free_two_others", "fa_near_free_any_bit", "hp_shift_28",
    "hp_15_bases", "hg_planes_bit", "bh_window_planes_between"}


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=tc.NAMES, floor=223, survivors_ok=lambda n: 20 * n <= 223, required=REQUIRED)


def test_at_most_one_in_twenty_survives():
    """the bound on the record, counted off the list itself"""
    mutants, record = mutation_audit.load(AUDIT.here)
    survivors = [m["id"] for m in mutants if m.get("expect") == "survives"]
    assert len(survivors) == record["total"] - record["killed"] and all(m.get("why") for m in mutants if m["id"] in survivors)
    assert 20 * len(survivors) <= len(mutants), survivors


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
