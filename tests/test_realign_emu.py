"""The realignment kernel's source (graphtyper_amd/csrc/gtx_realign_dev.hpp) run pair by pair through a sequential wave under
AddressSanitizer / UBSan (tests/emu_realign), against the plain restatement of the alignment's definition (tests/realign_ref.py):
every field of every result is equal -- all values are integers, there is no tolerance -- and there is no sanitizer report.
Every pair within the limits runs over heap blocks of exactly its sizes.  The device: test_gpu_realign.py."""
import functools

import pytest

import emu_programs
import realign_cases as rc
import realign_ref as rr


@pytest.fixture(scope="session")
def emu_realign(tmp_path_factory):
    return emu_programs.build("emu_realign", tmp_path_factory.mktemp("emu_realign"))


def run_emu(emu, tmp_path, arrays):
    """arrays: what rc.arrays returns"""
    return rc.through(functools.partial(emu_programs.run, emu, tmp_path), arrays)


@pytest.mark.parametrize("name", sorted(rc.SETS) + sorted(rc.ENTRY))
def test_every_field_equals_the_restatement(emu_realign, tmp_path, name):
    """the pair sets, and the cases of the entry point's other paths: rows wider than the reads, set bits behind a read's last
    base, offsets made by hand, letters in lower case and bytes that are no letters"""
    arrays, want = rc.case(name)
    got = run_emu(emu_realign, tmp_path, arrays)
    assert len(got) == len(want)
    wrong = [(i, tuple(arrays[5][i]), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert wrong == [], wrong[:5]


def test_a_pair_and_its_reversal_score_alike(emu_realign, tmp_path):
    """the model is symmetric under reversal: a check of reads over 64 bases that does not go through the restatement"""
    reads, _, pairs = rc.get("reversed_pairs")
    got = run_emu(emu_realign, tmp_path, rc.case("reversed_pairs")[0])
    assert len(got) == 2 * 2 * len(rc.M_SIZES) * len(rc.REVERSED_N) and all(g[5] == 0 for g in got)
    assert [(pairs[k], got[k], got[k + 1]) for k in range(0, len(got), 2) if got[k][0] != got[k + 1][0]] == []
    assert sum(len(reads[p[0]]) > 64 for p in pairs) >= len(pairs) // 2


def test_the_sets_hold_what_they_are_for():
    """the hand-made sets do reach the paths they are named after"""
    want = rc.expected("mismatch_runs_and_clips")
    reads, _, pairs = rc.get("mismatch_runs_and_clips")
    # a run of 12 mismatches: an insertion plus a deletion (2 * (7 + 11) = 36 lost; chance matches may give a little back) beats
    # pairing them (12 * 4 = 48 lost) and beats the clip
    assert want[2][0] >= 100 - 12 - 2 * (7 + 11) > 100 - 12 - 48 and (want[2][1], want[2][2]) == (0, 100)
    clipped = [w for w, p in zip(want, pairs) if w[1] > 0 or w[2] < len(reads[p[0]])]
    assert 5 <= len(clipped) < len(want) - 5  # some clips win, some lose
    assert {w[5] for w in rc.expected("bad_and_long")} == {0, 1, 2}
    n = len(rc.get("no_padding")[1][0])
    assert all(w[3] == 0 or w[4] == n for w in rc.expected("no_padding")[:5])
    assert len(rc.get("simulated")[2]) == 300
    assert (len(rc.get("exhaustive_ac")[2]), len(rc.get("exhaustive_acn")[2])) == (7812, 14400)
    n = 2048
    assert [w[:5] for w in rc.expected("limits")] == [(256, 0, 256, n - 256, n), (256, 0, 256, 0, 256), (1, 0, 1, n - 1, n)]
    # the hand-made offsets: bad windows between good ones, and two windows that share letters
    want = rc.case("offsets_by_hand")[1]
    assert [w[5] for w in want[::3]] == [0, 1, 0, 1, 1, 1, 0, 0]


def test_the_outcomes_the_pairs_with_window_records_reach():
    """which outcomes of the decision simulated() and no_padding reach with old_score one below, at and one above the new score (by the
    restatement): test_gpu_realign.py carries the device's results through gtx_disc_realign_decide over the same pairs"""
    assert rc.outcomes("simulated") == {rr.BETTER, rr.SAME_OVERLAPPING, rr.SAME, rr.WORSE}  # (its windows are padded well)
    assert rc.outcomes("no_padding") == {rr.NO_PADDING, rr.BETTER, rr.SAME, rr.WORSE}
