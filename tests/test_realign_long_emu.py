"""The long realignment kernel's source (graphtyper_amd/csrc/gtx_realign_long_dev.hpp) behind the short one's, run pair by pair
through a sequential wave under AddressSanitizer / UBSan (tests/emu_realign_long), against the plain restatement of the
alignment's definition (tests/realign_ref.py, with the long limits applied by tests/realign_long_cases.py): every field of every
result is equal -- all values are integers, there is no tolerance -- and there is no sanitizer report.  Every pair within the
limits in force runs over heap blocks of exactly its sizes.  The device: test_gpu_realign_long.py."""
import functools

import pytest

import emu_programs
import realign_cases as rc
import realign_long_cases as lc
import realign_ref as rr


@pytest.fixture(scope="session")
def emu_realign_long(tmp_path_factory):
    return emu_programs.build("emu_realign_long", tmp_path_factory.mktemp("emu_realign_long"))


def run_emu(emu, tmp_path, arrays, max_read=lc.MAX_READ_LONG):
    return lc.through(functools.partial(emu_programs.run, emu, tmp_path), arrays, max_read)


def differences(pairs, got, want):
    assert len(got) == len(want)
    return [(i, tuple(pairs[i]), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]][:5]


@pytest.mark.parametrize("name", sorted(lc.SETS) + sorted(lc.ENTRY))
def test_every_field_equals_the_restatement(emu_realign_long, tmp_path, name):
    arrays, want = lc.case(name)
    assert differences(arrays[5], run_emu(emu_realign_long, tmp_path, arrays), want) == []


def test_rows_exactly_as_wide_as_the_read(emu_realign_long, tmp_path):
    for m in lc.ROW_M:
        arrays, want = lc.row_case(m)
        assert arrays[1] == (m + 31) // 32 * 16
        assert differences(arrays[5], run_emu(emu_realign_long, tmp_path, arrays), want) == [], m


def test_planted_alignments(emu_realign_long, tmp_path):
    """a fact that does not go through the restatement: score m - 5k, cb 0, clip_end m, target_begin the copy's place"""
    (reads, targets, pairs), want = lc.planted()
    assert len(pairs) == 60 and all(257 <= len(r) <= 1000 for r in reads) and all(2049 <= len(t) <= 4095 for t in targets)
    assert {w[0] - w[2] for w in want} == {0, -5, -10, -15, -20, -25}
    assert differences(pairs, run_emu(emu_realign_long, tmp_path, lc.arrays(reads, targets, pairs)), want) == []


def test_the_limit_in_force(emu_realign_long, tmp_path):
    """mixed_batch on a default object, at a limit of 257 and at one of 300: beyond the limit in force a pair stays too long, and
    the short pairs are the same everywhere"""
    reads, targets, pairs = lc.get("mixed_batch")
    arrays = lc.arrays(reads, targets, pairs)
    kinds = [lc.kind_of(reads, targets, p) for p in pairs]
    for max_read in (0, 256, 257, 300):
        want = [lc.result(reads, targets, p, max_read) for p in pairs]
        assert differences(pairs, run_emu(emu_realign_long, tmp_path, arrays, max_read), want) == [], max_read
        assert all(w == lc.expected("mixed_batch")[i] for i, w in enumerate(want) if kinds[i] != "long")
    at_257 = [lc.result(reads, targets, p, 257) for p in pairs]
    assert lc.TOO_LONG in [w for w, k in zip(at_257, kinds) if k == "long"] and any(w[5] == rr.OK for w, k in zip(at_257, kinds) if k == "long")


def test_the_short_sets_on_a_long_mode_object(emu_realign_long, tmp_path):
    """pairs within the short limits are the first kernel's: the long one returns without a store"""
    for name in ("simulated", "ties", "n_behind_the_read"):
        arrays, want = rc.case(name)
        assert differences(arrays[5], run_emu(emu_realign_long, tmp_path, arrays), want) == [], name


def test_the_sets_hold_what_they_are_for():
    want = lc.expected("both_limits")
    assert want[0] == (1000, 0, 1000, 3095, 4095, rr.OK)
    assert want[1][:3] == (1000 - 5 - (7 + 1) - (7 + 4), 0, 1000) and want[1][3:5] == (600, 1597)  # five inserted bases, two deleted
    assert want[2][:5] == (961 - 15, 0, 961, 500, 1461)
    want = lc.expected("clips")
    assert (want[0][1], want[0][2], want[1][1], want[1][2]) == (970, 1000, 0, 30)
    assert want[2] == (-4, 998, 999, 50, 51, rr.OK) and want[3] == (-9, 0, 1, 0, 1, rr.OK)
    reads, targets, pairs = lc.get("mixed_batch")
    kinds = [lc.kind_of(reads, targets, p) for p in pairs]
    assert len(pairs) % 4 != 0 and {frozenset(kinds[k:k + 4]) for k in range(0, len(pairs), 4)} >= {frozenset(("short", "long", "bad", "beyond"))}
    met = {(a, b) for a, b in zip(kinds, kinds[1:])}
    assert all((a, b) in met or (b, a) in met for a in ("short", "long", "bad", "beyond") for b in ("short", "long", "bad", "beyond"))
    want = lc.expected("column_boundaries")
    reads, targets, pairs = lc.get("column_boundaries")
    assert want[-1] == lc.TOO_LONG and all(w[5] == rr.OK for w in want[:-1])
    assert {len(t) for t in targets} == set(lc.COLUMN_N) | {4096}
    assert any(w[3] == 0 for w in want) and any(w[4] == len(targets[p[1]]) for w, p in zip(want, pairs)) and any(w[3] < 2047 < 2048 < w[4] for w in want)
    assert {len(r) for r in lc.get("row_boundaries")[0]} == set(lc.ROW_M)
    # the ties: every repeat leaves more than one cell, or more than one origin, at the best score; the rule names one
    assert [w[5] for w in lc.expected("ties")] == [rr.OK] * 4
