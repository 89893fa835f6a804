"""The case sets of tests/disc_variants_cases.py hold what they are for, the restatement (tests/disc_variants_ref.py) gives a few
records worked out by hand from the reference's text, and the end-to-end file set of the region run meets the conditions it was
made for -- on the host, through what exists: the oracle's first pass and merge, the restatement of each file's second pass, and
the restatement of the records and the text.  The library against these: test_disc_variants.py (the C ABI), test_disc_variants_emu.py
(the same file under the sanitizers), test_gpu_discover.py (the region run on the device)."""
import pytest

import disc_variants_cases as vc
import disc_variants_ref as ref


@pytest.mark.parametrize("name", sorted(vc.SETS))
def test_the_set_holds_what_it_is_for(name):
    vc.FACTS[name](vc.cases(name))


def test_the_restatement_by_hand():
    """a region ACGTRACGTA at 100: an SNP under C, an insertion behind the R (N in front), a deletion of the last two letters; then the
    base in front at the region's edges"""
    reference, rb = "ACGTRACGTA", 100
    haps = [((101, "X", "T"), frozenset(), frozenset()), ((105, "I", "GG"), frozenset(), frozenset()), ((108, "D", "TA"), frozenset(), frozenset())]
    table = {(105, "I", "GG"): True, (108, "D", "TA"): True}
    recs = ref.records(reference, rb, table, haps)
    assert [(r["pos"], r["ref"], r["alt"], r["gt_id"], r["hap"], r["anti"]) for r in recs] == [
        (101, "C", "T", 1, [], [2, 3]), (104, "N", "NGG", 2, [], [3]), (107, "GTA", "G", 3, [], [])]
    assert ref.sites_text("c", recs) == ref.COLUMNS + ("c\t102\tc:102:SG\tC\tT\t0\t.\tGT_ANTI_HAPLOTYPE=2,3;GT_ID=1\n"
                                                       "c\t105\tc:105:IG\tN\tNGG\t0\t.\tGT_ANTI_HAPLOTYPE=3;GT_ID=2\n"
                                                       "c\t108\tc:108:IG\tGTA\tG\t0\t.\tGT_ID=3\n")
    # get_generated_reference_genome clamps to the region: [100, 101) in 1-based positions is in front of it and comes back empty
    assert ref.generated_reference(reference, rb, 100, 101) == ("", 101, 101)
    assert ref.generated_reference(reference, rb, 101, 102) == ("A", 101, 102) and ref.generated_reference(reference, rb, 110, 111) == ("A", 110, 111)
    assert ref.generated_reference(reference, rb, 111, 112) == ("", 111, 111)
    assert ref.add_base_in_front(reference, rb, 100, ["", "C"]) == (False, 100, ["", "C"])
    assert ref.add_base_in_front(reference, rb, 101, ["", "C"]) == (True, 100, ["A", "AC"])
    assert ref.add_base_in_front(reference, rb, 105, ["", "C"], add_n=False) == (False, 105, ["", "C"])
    assert ref.add_base_in_front(reference, rb, 101, ["*", "C"]) == (True, 100, ["*", "AC"])
    assert [ref.variant_type(s) for s in (["A", "C"], ["", "C"], ["A", "ACG"], ["", "CAG"], ["AC", "AG"], ["ACG", "A", "*"])] == ["SG", "SG", "IG", "IG", "XG", "IG"]


def test_the_words_written_here_are_the_librarys_format():
    """the word writer of the cases against the two parsers that exist: gtx_disc_indel_table and test_discovery.parse_result"""
    import numpy as np
    import test_discovery as td
    from graphtyper_amd import lib as gtx
    for name in ("dropped", "sets", "many"):
        for case in vc.cases(name):
            words = vc.arrays(case)["words"]
            entries, letters = gtx.disc_indel_table(words)
            assert [(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), bool(e["good"])) for e in entries] == \
                [vc.key(e) + (bool(e["good"]),) for e in case.table]
            indels, haps = td.parse_result(words)
            assert indels == [vc.key(e) for e in case.table] and list(haps) == [h[0] for h in case.haps]
            assert all(haps[e] == (set(ever), set(always)) for e, ever, always in case.haps)
            assert np.array_equal(words, np.asarray(words, np.uint32))


def test_the_end_to_end_file_set_holds_what_it_is_for():
    """three files over one region through the host chain: an indel good at the merge, one bad at the merge and good after its file's
    rounds, one bad to the end and dropped with a kept event behind it inside another record's window, records with GT_HAPLOTYPE and
    with GT_ANTI_HAPLOTYPE, every file with a list, no pair refused"""
    vc.facts_simulated(vc.host_chain())
