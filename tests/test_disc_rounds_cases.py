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
    assert not by["good already"] and not by["log_qual floor at anti 100"] and ref.get_log_qual(10, 100, 7) == 0
    # the widths: every such row turns round when its counter is read at 32 bits, and has the value the narrow reading gives
    wide = {what: ref.is_good_count(e, s) and ref.is_good_indel(s) for e, s, what in ROWS}
    narrow = [what for what in by if "65536" in what or "256 +" in what]
    assert len(narrow) == 9 and all(by[what] != wide[what] for what in narrow if what not in ("hq_count 65536 + 10 multi 50", "hq 7 max_mapq 256 + 11", "hq_count 65536 + 4 count 4.5"))
    e, s4, _ = next(r for r in ROWS if r[2] == "hq_count 65536 + 4 count 4.5")
    assert ref.is_good_count(e, s4) and not ref.is_good_count(e, ref.as_the_reference_holds(s4))
    assert not by["hq_count 65536 + 10 multi 51"] and by["hq_count 65536 + 10 multi 50"] and by["anti_count 65536"] and by["multi_count 65536"]
    assert by["sequence_reversed 65536 + 5"] and not by["proper_pairs 65536 + 4"] and not by["hq 7 max_mapq 256 + 10"] and by["hq 7 max_mapq 256 + 11"]
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
    # the rows that show the arms through is_good_count: every bound of every arm has a row on it and one to the side that fails
    arm = {what: ref.is_good_count(e, s) for e, s, what in ROWS if what.startswith("arm ")}
    assert [what for what, good in arm.items() if good] == ["arm 2 span 5 hq 4 count 5.0", "arm 3 span 15 hq 3 count 4.5", "arm 1 span 4 hq 5 count 5.5"]
    assert len(arm) == 15 and count('I', 12, 3) == 5.25 and count('D', 39, 2) >= 4.5 > count('D', 14, 3) and count('D', 2, 5) < 5.5


# ---- the sets made for the windows' text ------------------------------------------------------------------------------------------------
def own_entries(case):
    """[(k, read, outcome, the table's entry, what the restatement saw in front of its apply_indel_event)] of every entry of a read's own"""
    want = rc.expected(case)
    return [(r["k"], i, outcome, case.table[x["t"]], x) for r in want["trace"]["rounds"] for (i, outcome, _, _), own in zip(r["visits"], r["own"]) for x in own]


def moving_steps(kind, index, size, n):
    """the steps of apply_event's moving loop over a window of n letters: 64 entries a step (gtx_disc_rounds_dev.hpp)"""
    return -(-(n - size - index) // 64) if kind == 'D' else -(-(n - index) // 64)


def test_copies_apply_every_size_as_entry_k_and_as_an_own_entry():
    applied_k, applied_own, after, steps = set(), set(), set(), {'D': 0, 'I': 0}
    for case in rc.cases("copies"):
        want = rc.expected(case)
        for r in want["trace"]["rounds"]:
            e = case.table[want["lst"][r["k"]]]
            if not r["skipped"]:
                applied_k.add((e["type"], len(e["seq"])))
                plain = min(len(case.reference), e["pos"] + 200) - max(0, e["pos"] - 200)
                after.add(((plain - len(e["seq"]) if e["type"] == 'D' else plain + len(e["seq"])) % 64, e["type"], len(e["seq"])))
        for k, i, _, e, x in own_entries(case):
            if x["applied"]:
                applied_own.add((e["type"], len(e["seq"])))
                n = next(v[3] for v in want["trace"]["rounds"][k]["visits"] if v[0] == i)  # the window behind every event
                before = n + len(e["seq"]) if e["type"] == 'D' else n - len(e["seq"])      # (the large event is the last applied)
                steps[e["type"]] = max(steps[e["type"]], moving_steps(e["type"], x["index"], len(e["seq"]), before))
    every = {(kind, size) for kind in "DI" for size in rc.COPY_SIZES}
    assert applied_k >= every and applied_own >= every
    assert after >= {(over % 64, kind, size) for over in (-1, 0, 1) for kind in "DI" for size in (63, 64, 65)}
    assert min(steps.values()) >= 3
    # an insertion of a read's own at the window's last index; the same entry behind a deletion: its position is no index any more
    def window(case, k, i):  # the letters of read i's window in round k, every event applied
        return next(v[3] for v in rc.expected(case)["trace"]["rounds"][k]["visits"] if v[0] == i)
    at_length, last, outside, one_left = rc.cases("copies")[-4:]
    assert any(x["search"] == "outside" and e["pos"] - 252 == window(at_length, k, i) for k, i, _, e, x in own_entries(at_length))  # pos == seq_size
    one_step = rc.cases("copies")[-5]
    assert len(one_step.reference) - 300 == 64 and rc.expected(one_step)["trace"]["rounds"][0]["visits"][0][1] == ref.realign.WORSE
    assert any(x["applied"] and e["type"] == 'I' and x["index"] == window(last, k, i) - len(e["seq"]) - 1 for k, i, _, e, x in own_entries(last))
    assert {x["search"] for *_, x in own_entries(outside)} == {"outside"}
    assert any(x["applied"] and e["type"] == 'D' and x["index"] + 1 == window(one_left, k, i) for k, i, _, e, x in own_entries(one_left))


def test_search_takes_every_exit():
    seen, sides = set(), set()
    for case in rc.cases("search"):
        want = rc.expected(case)
        for k, i, _, e, x in own_entries(case):
            seen.add((x["search"], e["type"]))
            if x["applied"]:
                sides.add((e["type"], "in front" if e["pos"] < case.table[want["lst"][k]]["pos"] else "behind"))
    assert seen >= {(how, kind) for how in ("at once", "walked forward", "walked back", "not found") for kind in "DI"}
    assert sides == {(kind, side) for kind in "DI" for side in ("in front", "behind")}
    # two entries of the read's own in front of a third: found 3 + 2 (theirs) + 2 (entry k's) indices in front of its position
    case = rc.cases("search")[3]
    k, i, _, e, x = own_entries(case)[-1]
    assert e["type"] == 'I' and x["search"] == "walked back" and (e["pos"] - 132) - x["index"] == 7
    # the walk forward crosses the letters entry k put in: it begins among them
    case = rc.cases("search")[2]
    k_entry = case.table[rc.expected(case)["lst"][2]]
    assert any(x["search"] == "walked forward" and k_entry["pos"] < e["pos"] < k_entry["pos"] + len(k_entry["seq"]) for *_, e, x in own_entries(case))
    # not found: by a deletion of entry k, and by a deletion of the read's own
    assert [x["search"] for *_, x in own_entries(rc.cases("search")[4]) if not x["applied"]][-2:] == ["not found"] * 2
    assert [(x["search"], x["applied"]) for *_, x in own_entries(rc.cases("search")[5])][-2:] == [("at once", True), ("not found", False)]


def test_own_ends_fail_and_hold_by_either_arm():
    seen = set()
    for n, case in enumerate(rc.cases("own_ends")):
        want = rc.expected(case)
        for k, i, outcome, e, x in own_entries(case):
            assert e["type"] == 'D' and x["pure"]
            arm = "past" if x["past"] else "differs" if x["differs"] else "holds"
            seen.add((n, arm, x["read_pos"], rc.OUTCOME[outcome]))
            assert x["applied"] == (arm == "holds")
            if not x["applied"] and outcome == ref.realign.BETTER:  # the refused entry goes into the new list as anti-support
                assert want["before"][k + 1][1][i] == [(want["lst"][k], 0), (x["t"], -1)]
                held, now = want["before"][k][2][x["t"]], want["before"][k + 1][2][x["t"]]
                if x["read_pos"] == 0:
                    assert now["hq_count"] < held["hq_count"] and now["anti_count"] > held["anti_count"] and now["max_mapq"] == held["max_mapq"]
    # one letter in front of the window's last: the end test holds; on it and one past it: the first arm; over an insertion and over a
    # deletion that entry k applied: the second.  Each with the entry held as support (0), as anti-support (-1) and as multi-support
    assert {(n, arm) for n, arm, _, _ in seen} == {(0, "holds"), (1, "past"), (2, "past"), (3, "differs"), (4, "differs")}
    for n in (1, 2, 3, 4):
        assert {(p, o) for m, _, p, o in seen if m == n} >= {(0, "BETTER"), (-1, "BETTER"), (-1, "WORSE")}
    case = rc.cases("own_ends")[1]
    t, k = (case.table[e] for e in rc.expected(case)["lst"])
    assert t["pos"] + len(t["seq"]) == k["pos"] + 200 < len(case.reference)  # the deletion ends with k's window, inside the region
    assert any(info["max_mapq"] == 254 and info["hq_count"] == 0 for c in rc.cases("own_ends") for info in rc.expected(c)["support"])


def test_purity_at_the_windows_ends_and_behind_an_applied_entry():
    cs = rc.cases("purity")
    first = {(x["index"], x["applied"]) for c in cs[:6] for *_, x in own_entries(c)}
    assert first == {(1, True), (2, True), (3, True)} and {c.region_begin for c in cs[:6]} == {0, 3000}
    last = set()
    for c in cs[6:11]:
        want = rc.expected(c)
        for k, i, _, e, x in own_entries(c):
            n = next(v[3] for v in want["trace"]["rounds"][k]["visits"] if v[0] == i)
            before = n + len(e["seq"]) if e["type"] == 'D' else n - len(e["seq"])
            last.add((before - x["index"], e["type"], x["applied"]))
    assert last == {(3, 'I', True), (3, 'D', True), (2, 'I', True), (2, 'D', True), (1, 'I', True)}
    behind = [[(x["pure"], x["applied"]) for *_, x in own_entries(c)] for c in cs[11:19]]
    assert behind[0::2] == [[(False, False)]] * 3 + [[(True, True)]] and behind[1::2] == [[(False, False)]] * 3 + [[(True, True)]]
    assert [rc.expected(c)["lst"] for c in cs[11:19]] == [[1, 0]] * 8  # the entry behind is the read's own, the one in front entry k
    # three and two positions in front of a deletion that entry k applied: pos + 3 is the first index the test does not look at
    assert [[(x["search"], x["pure"], x["applied"]) for *_, x in own_entries(c)] for c in cs[19:]] == [[("at once", True, True)], [("at once", False, False)]]


def test_fields_of_a_read_made_better_and_max_mapq():
    first, lets_go, sole, far, alone, left = rc.cases("fields")
    want = rc.expected(alone)
    assert want["trace"]["rounds"] == [dict(k=0, skipped=True, visits=[], own=[])] and alone.table[0]["pos"] + 4 == len(alone.reference)
    assert [rc.OUTCOME[v[1]] for v in rc.expected(left)["trace"]["rounds"][0]["visits"]] == ["SAME_OVERLAPPING", "SAME_OVERLAPPING", "SAME"]
    assert left.region_begin == 7 and [r["pos"] - left.table[0]["pos"] for r in left.reads] == [6, 7, 8]
    rounds = rc.expected(far)["trace"]["rounds"]
    assert rc.expected(far)["lst"] == [0, 1] and far.table[0]["pos"] + 200 < far.region_begin and [r["skipped"] for r in rounds] == [True, False]
    want = rc.expected(first)
    ins = first.table[0]
    assert ins["pos"] == len(first.reference) - 1 and [s["num_clipped_end"] for s in want["states"]] == [40, 0]
    s = want["states"][1]
    n = want["trace"]["rounds"][0]["visits"][1][3]
    # the alignment begins on the second inserted letter: the run of equal ref_pos values goes on to the window's last index, where
    # the loop's bound stops it (51 steps: 50 inserted letters and the region's last base)
    assert s["num_ins_begin"] == len(ins["seq"]) - 1 == 51 and s["num_clipped_begin"] == 10 and n == 201 + 52
    assert max(x["num_ins_begin"] for c in (lets_go, sole) for x in rc.expected(c)["states"]) == 0
    want = rc.expected(lets_go)
    assert lets_go.reads[2]["mapq"] == 254 and [want["before"][k][2][0]["hq_count"] for k in (1, 2)] == [1, 0]
    assert [want["before"][k][2][0]["max_mapq"] for k in (1, 2)] == [254, 254] and want["entries"][2] == [(1, 0), (0, -1)]
    want = rc.expected(sole)
    assert sole.reads[4]["mapq"] == 255 and want["support"][0]["hq_count"] == 1 and want["support"][0]["max_mapq"] == 0


def test_the_long_limits_change_nothing_of_the_new_sets():
    """no new read has more than 256 bases and no new window more than 2 048 letters: an object with max_read_len 1 000 gives the same"""
    import disc_rounds_long_cases as lr
    for name in NEW_SETS:
        for case in rc.cases(name):
            by_default, by_long = rc.expected(case), lr.expected_long(case)
            assert by_default["trace"]["refused"] == 0 and all(by_default[f] == by_long[f] for f in ("states", "entries", "support", "trace", "good"))


NEW_SETS = ("copies", "search", "own_ends", "purity", "fields")
