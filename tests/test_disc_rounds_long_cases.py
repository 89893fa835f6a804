"""What the cases of tests/disc_rounds_long_cases.py are for, asserted from the restatement's traces (tests/disc_rounds_ref.py) under
the default limits and under the long ones: nobody is refused in long mode, the default mode refuses what it always did, and the
good-bits depend on the evidence the default aligner leaves out.  No device; test_gpu_disc_rounds_long.py holds the library to the
same expectations."""
import disc_rounds_cases as rc
import disc_rounds_long_cases as lr
import disc_rounds_ref as ref


def visits(trace):
    return [(r["k"],) + tuple(v) for r in trace["rounds"] for v in r["visits"]]


def test_the_restatements_constants_are_put_back():
    lr.expected_long(lr.limits_turned_round())
    assert (ref.MAX_READ, ref.MAX_TARGET) == (256, 2048)


def test_limits_turned_round():
    case = lr.limits_turned_round()
    assert [len(r["seq"]) for r in case.reads] == [len(r["seq"]) for r in rc.cases("limits")[0].reads]
    by_default, by_long = rc.expected(case)["trace"], lr.expected_long(case)["trace"]
    assert by_default == rc.expected(rc.cases("limits")[0])["trace"] and by_default["refused"] == 4
    assert by_long["refused"] == 0 and by_long["aligned"] == by_default["aligned"] + by_default["refused"]
    seen = visits(by_long)
    assert (0, 2, ref.realign.BETTER) == seen[1][:3] and len(case.reads[2]["seq"]) == 257  # the 257-base read takes its new place
    assert sorted({v[4] for v in seen}) == [2047, 2048, 2049] and all(v[2] != "refused" for v in seen)
    assert lr.expected_long(case)["states"][2] != rc.expected(case)["states"][2]


def test_one_read_of_1000():
    case = lr.one_read_of_1000()
    by_default, by_long = rc.expected(case), lr.expected_long(case)
    assert sorted(len(r["seq"]) for r in case.reads)[-2:] == [60, 1000]
    assert by_long["trace"]["refused"] == 0 and by_long["trace"]["aligned"] == 17
    assert by_default["trace"]["aligned"] == 0 and by_default["trace"]["refused"] == 17  # pairs_refused == pairs
    lengths = {v[4] for v in visits(by_long["trace"])}
    assert min(lengths) == 2198 and max(lengths) == 2260
    long_pairs = [v for v in visits(by_long["trace"]) if len(case.reads[v[1]]["seq"]) == 1000]
    assert len(long_pairs) == 1 and long_pairs[0][2] == ref.realign.BETTER and long_pairs[0][4] == 2198  # one pair of 2.2 M cells
    assert by_long["good"] != by_default["good"] and any(by_long["good"]) and not any(by_default["good"])


def test_longest_600():
    seen = set()
    for case in lr.longest_600():
        by_default, by_long = rc.expected(case)["trace"], lr.expected_long(case)["trace"]
        assert max(len(r["seq"]) for r in case.reads) == 600 and by_long["refused"] == 0 and by_default["refused"] == 10
        per_length = {}
        for v in visits(by_long):
            per_length.setdefault(len(case.reads[v[1]]["seq"]), set()).add(rc.OUTCOME[v[2]])
            assert v[4] <= 1400
        equal = "SAME_OVERLAPPING" if case.region_begin == 0 else "SAME"
        assert all(per_length[m] >= {"BETTER", "WORSE", equal} for m in (257, 600)) and per_length[300] >= {"BETTER", "WORSE", equal, "NO_PADDING"}
        seen |= lr.outcomes(by_long)
    assert seen == {"NO_PADDING", "BETTER", "SAME_OVERLAPPING", "SAME", "WORSE"}
