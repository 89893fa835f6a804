"""The case sets of tests/disc_rounds_cases.py hold what they are meant to hold (fact tests over the restatement's trace,
tests/disc_rounds_ref.py), the restatement and the second witness -- the library's host pieces strung by a loop, the counters
counted off the lists -- agree on every case, and gtx_disc_second_decide (host code) equals the restatement's final decision on
hand-made counters with every threshold at its edge.  No test here needs a GPU."""
import numpy as np
import pytest

import disc_rounds_cases as rc
import disc_rounds_ref as ref
import realign_ref as realign
from graphtyper_amd import lib as gtx

ALL = [(name, k) for name in sorted(rc.SETS) for k in range(len(rc.cases(name)))] + [("shape%d" % n, 0) for n in rc.SHAPE_PAIRS]


def case_of(name, k):
    return rc.shape_case(int(name[5:])) if name.startswith("shape") else rc.cases(name)[k]


def visits(case):
    return [(r["k"], i, outcome, bits, n) for r in rc.expected(case)["trace"]["rounds"] for i, outcome, bits, n in r["visits"]]


def counters(support):
    return [{f: info[f] for f in rc.SUPPORT_FIELDS} for info in support]


@pytest.mark.parametrize("name,k", ALL)
def test_the_two_witnesses_agree(name, k):
    case = case_of(name, k)
    want, other = rc.expected(case), rc.witness(case)
    assert other["states"] == want["states"] and other["entries"] == want["entries"]
    assert counters(other["support"]) == counters(want["support"])
    trace = want["trace"]
    assert (other["aligned"], other["refused"], other["skipped"]) == (trace["aligned"], trace["refused"], trace["skipped"])


@pytest.mark.parametrize("name,k", ALL)
def test_the_counters_are_the_holders_after_every_round_and_no_floor_acts(name, k):
    """the argument beside the kernels (gtx_disc_rounds_dev.hpp): from zeros, hq_count, sequence_reversed and proper_pairs are the
    current holders with the flag, so the floors of read.cpp:76,83 never act and no counter goes below zero"""
    case = case_of(name, k)
    want = rc.expected(case)
    assert want["trace"]["floors"] == 0
    for states, entries, support in want["before"]:
        held = rc.holders(case, states, entries)
        for t, info in enumerate(support):
            assert all(info[f] == held[t][f] and info[f] >= 0 for f in rc.SUPPORT_FIELDS if f != "max_mapq"), (t, info, held[t])


def test_chain_across_rounds():
    for case in rc.cases("chain"):
        v = visits(case)
        better = {(k, i) for k, i, o, _, _ in v if o == realign.BETTER}
        # made BETTER in one round, a candidate of a later one, whose window applies the entry it brought (bit 1 and above)
        assert any((k0, i) in better and k1 > k0 and bits & ~1 for k0, i in better for k1, j, _, bits, _ in v if j == i)
        # insertion then deletion in one window (entry k the insertion, the read's own entry the deletion), and the purity test
        # refusing an insertion two positions in front of entry k while the entry behind it in the list is applied (0b101)
        want = rc.expected(case)
        assert any(case.table[want["lst"][k]]["type"] == 'I' and bits == 0b11 and case.table[want["before"][k][1][i][0][0]]["type"] == 'D' for k, i, _, bits, _ in v)
        assert any(bits == 0b101 for _, _, _, bits, _ in v)
        assert any(s and s["num_ins_begin"] > 0 for s in want["states"])  # an alignment that begins inside inserted letters
        assert want["trace"]["lowered"] > 0                               # a replace that lowers what an earlier round raised
        assert {o for _, _, o, _, _ in v} >= {realign.BETTER, realign.WORSE, realign.SAME}
    # a read whose new place takes it out of a later round: before its BETTER round it passed that round's test, after it it does not
    case = rc.cases("chain")[0]
    want = rc.expected(case)
    taken_out = 0
    for k0, i, o, _, _ in visits(case):
        if o != realign.BETTER:
            continue
        old = want["before"][k0][0][i]
        for k1 in range(k0 + 1, len(want["lst"])):
            indel = case.table[want["lst"][k1]]
            if realign.wants(old["pos"], old["pos_end"], old["num_clipped_begin"], old["num_clipped_end"], indel["pos"], indel["span"]) and \
                    not any(k == k1 and j == i for k, j, _, _, _ in visits(case)):
                taken_out += 1
    assert taken_out > 0


def test_same_overlapping_at_both_ends_of_the_text():
    """:2086-2087 compares a contig position with region positions: with region_begin 0 a read that ends at the indel overlaps it, with
    a small region_begin another read does, with a large one none does"""
    per = [{(i, o) for _, i, o, _, _ in visits(case) if o in (realign.SAME, realign.SAME_OVERLAPPING)} for case in rc.cases("chain")]
    over = [{i for i, o in p if o == realign.SAME_OVERLAPPING} for p in per]
    assert over[0] and over[1] and over[0] != over[1] and not over[2]
    assert [case.region_begin for case in rc.cases("chain")] == [0, 7, 5000]


def test_the_first_entry_rule():
    """a list that names an entry again: a read that holds {t, -1} is aligned to t again, one that holds {t, 0} or {t, -2} is not"""
    case = rc.cases("again")[0]
    want = rc.expected(case)
    assert len(set(want["lst"])) < len(want["lst"])
    assert any(len([1 for t, p in per if (t, p) == (0, -1)]) > 1 for per in want["entries"])
    # an anti-support entry that the text still applies: WORSE in one round, that entry applied in a later round's window
    v = visits(case)
    worse = {(k, i) for k, i, o, _, _ in v if o == realign.WORSE}
    assert any(k1 > k0 and j == i and want["before"][k1][1][i][0][1] == -1 and bits & 2 for k0, i in worse for k1, j, _, bits, _ in v)
    seen_anti = seen_held = 0
    for r in want["trace"]["rounds"]:
        t, visited = want["lst"][r["k"]], {i for i, _, _, _ in r["visits"]}
        for i, per in enumerate(want["before"][r["k"]][1]):
            named = [p for te, p in per if te == t]
            if named and named[0] == -1 and i in visited:
                seen_anti += 1
            if named and named[0] != -1:
                assert i not in visited
                seen_held += 1
    assert seen_anti and seen_held


def test_edges_skip_rounds_and_lack_padding():
    for case in rc.cases("edges"):
        want = rc.expected(case)
        skipped = [case.table[want["lst"][r["k"]]] for r in want["trace"]["rounds"] if r["skipped"]]
        assert any(e["pos"] == case.region_begin for e in skipped)                                        # an indel at the region's first base
        assert any(e["type"] == 'D' and e["pos"] + len(e["seq"]) == case.region_begin + len(case.reference) for e in skipped)  # the end test
        by_round = {}
        for k, i, o, _, n in visits(case):
            by_round.setdefault(k, set()).add(o)
        assert sum(realign.NO_PADDING in o for o in by_round.values()) == 2  # at the window's first letter and at its last
        assert all(n < 400 for _, _, _, _, n in visits(case))                # both windows are cut off by the region


def test_counters_see_every_flag_and_mapq():
    case = rc.cases("chain")[0]
    want = rc.expected(case)
    holders = [(s["flags"] & 16, s["flags"] & 2, s["mapq"]) for s, per in zip(want["states"], want["entries"]) if any(p >= 0 for _, p in per)]
    assert {h[0] for h in holders} == {0, 16} and {h[1] for h in holders} == {0, 2} and {254, 255} <= {h[2] for h in holders}
    assert any(info["max_mapq"] == 254 for info in want["support"])


def test_the_aligners_limits():
    case = rc.cases("limits")[0]
    v = visits(case)
    lens = {len(case.reads[i]["seq"]): o for _, i, o, _, _ in v if len(case.reads[i]["seq"]) in (256, 257)}
    assert lens[256] != "refused" and lens[257] == "refused"
    assert {n for _, _, o, _, n in v if o == "refused"} >= {2049} and any(n == 2048 and o != "refused" for _, _, o, _, n in v)
    want = rc.expected(case)
    refused_only = {i for _, i, o, _, _ in v if o == "refused"} - {i for _, i, o, _, _ in v if o != "refused"}
    assert refused_only and all(want["states"][i] == want["before"][0][0][i] and not want["entries"][i] for i in refused_only)


def test_launch_shapes():
    for n in rc.SHAPE_PAIRS:
        case = rc.shape_case(n)
        rounds = rc.expected(case)["trace"]["rounds"]
        assert all(len(r["visits"]) == n for r in rounds)
        if n:
            assert sorted({v[3] for r in rounds for v in r["visits"]}) == [383, 385, 447, 449]


def test_rooms_differ_from_round_to_round():
    """the event array's model: a run that needs more than its live entries at the end (so an array of exactly max(live + new) has to
    compact), and rounds that leave lists behind"""
    case = rc.cases("again")[0]
    room = rc.room(case)
    live_end = sum(len(e) for e in rc.expected(case)["entries"])
    assert sum(new for _, new in room) > max(live + new for live, new in room) >= live_end


ROWS = rc.decide_rows()


def test_final_decision_on_hand_made_counters():
    table = [e for e, _, _ in ROWS]
    support = [s for _, s, _ in ROWS]
    assert table == sorted(table, key=rc.sc.ref.table_order)
    want = ref.good_after(table, list(range(len(table))), support)
    entries, _ = rc.sc.table_arrays(table)
    got = gtx.disc_second_decide(entries, np.arange(len(table), dtype=np.uint32), rc.support_array(support))
    for t, (_, _, what) in enumerate(ROWS):
        assert bool(got[t]) == want[t], what
    by = {what: want[t] for t, (_, _, what) in enumerate(ROWS)}
    # the facts: each threshold has a row on either side
    assert (by["span 4 hq 7"], by["span 5 hq 7"]) == (True, True) and not by["span 15 hq 5"]  # (hq <= 6 fails is_good_indel whatever the count)
    assert not by["hq 6 max_mapq 11"] and by["hq 7 max_mapq 11"] and not by["hq 7 max_mapq 10"] and not by["hq 9 max_mapq 10"] and by["hq 10 max_mapq 10"]
    assert not by["sequence_reversed 0 depth 10"] and by["sequence_reversed 1 depth 10"] and by["sequence_reversed 9 depth 10"]
    assert not by["sequence_reversed 10 depth 10"] and by["sequence_reversed 10 depth 11"] and not by["sequence_reversed 11 depth 11"]
    assert not by["proper_pairs 4"] and by["proper_pairs 5"]
    assert ref.get_log_qual(7, 25, 7) * 3 == 51 and ref.get_log_qual(7, 26, 7) * 3 == 48
    assert not by["3 * log_qual at anti 25"] and not by["3 * log_qual at anti 26"]
    assert by["qual / depth at multi 34"] and by["qual / depth at multi 35"] and not by["qual / depth at multi 36"]
    assert not by["good already"]
    # an entry outside the list is left alone too
    none = gtx.disc_second_decide(entries, np.zeros(0, np.uint32), rc.support_array(support))
    assert not none.any()


def test_the_count_lies_on_its_edges():
    """correction * hq_count is exactly 4.5, 5.0 and 5.5 for the rows that say so (the doubles are exact there)"""
    def count(kind, size, hq):
        return (float(size / 2.0 + 8.0) / 8.0 if kind == 'I' else float(size / 3.0 + 10.0) / 10.0) * hq
    assert count('I', 2, 4) == 4.5 and count('I', 4, 4) == 5.0 and count('I', 6, 4) == 5.5 and count('D', 15, 3) == 4.5 and count('D', 3, 5) == 5.5
    # the three arms alone, through is_good_count's text: hq 3 / 4 / 5 at spans 14 / 15 and 4 / 5 (is_good_indel is passed by none of
    # them -- hq_count <= 6 --, so the arms show in the count only)
    for kind, size, hq, span, arm in (('D', 15, 3, 15, True), ('D', 15, 3, 14, False), ('I', 4, 4, 5, True), ('I', 4, 4, 4, False), ('D', 3, 5, 1, True), ('D', 2, 5, 1, False)):
        c = count(kind, size, hq)
        assert ((hq >= 5 and c >= 5.5) or (span >= 5 and hq >= 4 and c >= 5.0) or (span >= 15 and hq >= 3 and c >= 4.5)) == arm
