"""The host functions around the realignment (include/gtx.h: gtx_disc_realign_target, gtx_disc_realign_wants,
gtx_disc_realign_decide) against the restatement of the reference's text in tests/realign_ref.py and against hand-worked cases.
They need no device: the object is made with device -1."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import realign_ref as rr
from graphtyper_amd import lib as gtx

REGION_BEGIN = 5000
REFERENCE = "".join(random.Random(3).choice("ACGT") for _ in range(1200))


@pytest.fixture(scope="module")
def disc():
    h = C.c_void_p()
    gtx.check(gtx.lib().gtx_disc_create(REFERENCE.encode(), len(REFERENCE), REGION_BEGIN, -1, C.byref(h)))
    yield h
    gtx.lib().gtx_disc_destroy(h)


def both(disc, max_read_size, events):
    letters, ref_pos, begin_padded, applied = gtx.disc_realign_target(disc, max_read_size, events)
    got = (letters.decode(), [int(x) for x in ref_pos], begin_padded, applied)
    assert got == rr.target(REFERENCE, REGION_BEGIN, max_read_size, events)
    return got


def test_an_insertion_and_a_deletion_with_their_ref_pos(disc):
    # max_read_size 20: the window is [pos - 120, pos + 120) of the region, the indel at index 120
    pos = REGION_BEGIN + 600
    letters, ref_pos, begin_padded, applied = both(disc, 20, [(pos, "I", "TTG")])
    assert (begin_padded, applied, len(letters)) == (480, 1, 243)
    assert letters == REFERENCE[480:600] + "TTG" + REFERENCE[600:720]
    assert ref_pos == list(range(121)) + [121] * 3 + list(range(121, 240))  # (the inserted entries hold the index 120 + 1)
    letters, ref_pos, begin_padded, applied = both(disc, 20, [(pos, "D", "NNNNN")])
    assert (begin_padded, applied) == (480, 1)
    assert letters == REFERENCE[480:600] + REFERENCE[605:720] and ref_pos == list(range(120)) + list(range(125, 240))


def test_an_event_at_the_windows_edge_is_refused(disc):
    # the window begins at the region's begin; an indel on its first base has ref_pos 0, one in front of it a negative one
    for pos in (REGION_BEGIN, REGION_BEGIN - 1):
        letters, ref_pos, begin_padded, applied = both(disc, 20, [(pos, "D", "A")])
        assert (begin_padded, applied) == (0, 0) and letters == REFERENCE[:max(0, pos - REGION_BEGIN + 120)] and ref_pos == list(range(len(letters)))
    assert both(disc, 20, [(REGION_BEGIN + 1, "D", "A")])[3] == 1
    # a later event in front of the window's second base is refused, the indel itself is applied
    assert both(disc, 20, [(REGION_BEGIN + 600, "D", "A"), (REGION_BEGIN + 480, "I", "C"), (REGION_BEGIN + 481, "I", "C")])[3] == 0b101


def test_a_second_event_within_three_positions_is_not_pure(disc):
    pos = REGION_BEGIN + 600
    for delta, kind, want in ((1, "I", 0b01), (2, "I", 0b01), (3, "I", 0b01), (4, "I", 0b11), (-3, "D", 0b11), (-2, "D", 0b01), (-1, "D", 0b01),
                              (3, "D", 0b01), (6, "D", 0b01), (8, "D", 0b01), (9, "D", 0b11)):
        # (the test looks at the six entries from three in front to two behind: a deletion of 130 .. 135 leaves a step between the
        # indices 129 and 130, which an event at 127 does not see and one at 138 does; 133 is deleted and cannot be found)
        first = (pos, "I", "GG") if kind == "I" else (pos, "D", "NNNNNN")
        assert both(disc, 30, [first, (pos + delta, kind, "T")])[3] == want, (delta, kind)
    # three events: the third is tried on what the second left
    assert both(disc, 30, [(pos, "I", "GG"), (pos + 20, "D", "NN"), (pos + 22, "I", "A"), (pos - 30, "I", "ACGT")])[3] == 0b1011


def test_a_deletion_that_reaches_the_windows_end(disc):
    pos = REGION_BEGIN + len(REFERENCE) - 40  # the window ends with the region, 40 bases behind the indel
    assert both(disc, 20, [(pos, "D", "N" * 39)])[3] == 1
    assert both(disc, 20, [(pos, "D", "N" * 40)])[3] == 0  # its end is the window's end: refused (event.cpp:360)
    assert both(disc, 20, [(pos, "D", "N" * 41)])[3] == 0
    assert both(disc, 20, [(pos - 100, "D", "N"), (pos, "D", "N" * 40)])[3] == 1


def test_the_clamp_at_the_regions_begin_and_end(disc):
    L = gtx.lib()
    for pos, want_begin, want_len in ((REGION_BEGIN + 119, 0, 239), (REGION_BEGIN + 120, 0, 240), (REGION_BEGIN + 121, 1, 240),
                                      (REGION_BEGIN + len(REFERENCE) - 120, len(REFERENCE) - 240, 240),
                                      (REGION_BEGIN + len(REFERENCE) - 119, len(REFERENCE) - 239, 239),
                                      (REGION_BEGIN + len(REFERENCE) + 119, len(REFERENCE) - 1, 1)):
        letters, ref_pos, begin_padded, applied = both(disc, 20, [(pos, "D", "")])
        assert (begin_padded, len(letters)) == (want_begin, want_len), pos
    # a window that begins behind the region, and a buffer that is too small
    ev = np.array([(REGION_BEGIN + len(REFERENCE) + 120, 1, ord("D"), 0, 0)], gtx.REALIGN_EVENT)
    n, b, a = C.c_uint32(), C.c_int64(), C.c_uint64()
    seq, rp = np.zeros(300, np.uint8), np.zeros(300, np.int32)
    args = lambda cap: (disc, 20, ev.ctypes.data_as(C.c_void_p), 1, None, seq.ctypes.data_as(C.c_void_p), rp.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(b), C.byref(a))  # noqa: E731
    assert L.gtx_disc_realign_target(*args(300)) == 1  # GTX_ERR_ARG
    ev["pos"] = REGION_BEGIN + 600
    assert L.gtx_disc_realign_target(*args(100)) == 5 and n.value == 239  # GTX_ERR_CAPACITY with the size wanted
    assert L.gtx_disc_realign_target(*args(239)) == 0 and a.value == 1


def test_windows_of_seeded_events_equal_the_restatement(disc):
    rng = random.Random(29)
    for _ in range(300):
        pos = REGION_BEGIN + rng.randrange(-5, len(REFERENCE) + 5)
        events = []
        for k in range(rng.randrange(1, 6)):
            p = pos if k == 0 else pos + rng.randrange(-160, 160)
            events.append((p, rng.choice("ID"), "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 12)))))
        if max(0, pos - 150 - REGION_BEGIN) < len(REFERENCE):
            both(disc, rng.choice((0, 50, 151)), events)


def test_each_branch_of_the_overlap_test_at_its_boundary():
    L = gtx.lib()
    indel, span = 1000, 4
    cases = [  # (pos, pos_end, clipped begin, clipped end) -> wanted
        ((900, 999, 0, 0), 0), ((900, 1000, 0, 0), 1),              # no clip at the end: pos_end < indel.pos
        ((900, 979, 0, 10), 0), ((900, 980, 0, 10), 1),             # pos_end + clip + min(clip, 50) < indel.pos
        ((800, 839, 0, 80), 0), ((800, 870, 0, 80), 1), ((800, 869, 0, 80), 0),
        ((1005, 1100, 0, 0), 0), ((1004, 1100, 0, 0), 1),           # no clip at the begin: pos > indel.pos + span
        ((1025, 1100, 10, 0), 0), ((1024, 1100, 10, 0), 1),         # pos - clip - min(clip, 50) > indel.pos + span
        ((1135, 1200, 80, 0), 0), ((1134, 1200, 80, 0), 1),
        ((-1, 1200, 0, 0), 0), ((0, 1200, 0, 0), 1),
    ]
    for a, want in cases:
        assert L.gtx_disc_realign_wants(*a, indel, span) == want == rr.wants(*a, indel, span), a
    rng = random.Random(31)
    for _ in range(3000):
        a = (rng.randrange(800, 1200), rng.randrange(800, 1300), rng.choice((0, 0, 3, 49, 50, 51, 90)), rng.choice((0, 0, 3, 49, 50, 51, 90)))
        sp = rng.randrange(0, 30)
        assert L.gtx_disc_realign_wants(*a, indel, sp) == rr.wants(*a, indel, sp), (a, sp)


def decide_both(res, read_len, ref_pos, begin_padded, region_begin, old_score, indel_pos):
    d = gtx.disc_realign_decide(res + (0,), read_len, ref_pos, begin_padded, region_begin, old_score, indel_pos)
    got = (int(d["outcome"]), int(d["pos"]), int(d["pos_end"]), int(d["num_clipped_begin"]), int(d["num_clipped_end"]), int(d["num_ins_begin"]))
    assert got == rr.decide(res, read_len, ref_pos, begin_padded, region_begin, old_score, indel_pos)
    return got


def test_each_outcome_of_decide(disc):
    pos = REGION_BEGIN + 600
    _, ref_pos, begin_padded, _ = both(disc, 20, [(pos, "I", "TTG")])  # indices 121..123 are the insertion
    n = len(ref_pos)
    assert decide_both((50, 0, 50, 0, 50), 50, ref_pos, begin_padded, REGION_BEGIN, 10, pos)[0] == rr.NO_PADDING
    assert decide_both((50, 0, 50, n - 50, n), 50, ref_pos, begin_padded, REGION_BEGIN, 10, pos)[0] == rr.NO_PADDING
    assert decide_both((50, 0, 50, 1, n - 1), 50, ref_pos, begin_padded, REGION_BEGIN, 51, pos)[0] == rr.WORSE
    # the same score: overlapping when ref_pos[begin] + begin_padded <= indel.pos <= ref_pos[end] + begin_padded, as the text has it
    # (the indel's position is a contig position there, the other two are region positions: region_begin 0 makes them one)
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, REGION_BEGIN, 50, pos)[0] == rr.SAME
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, 0, 50, 600)[0] == rr.SAME_OVERLAPPING
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, 0, 50, 580)[0] == rr.SAME_OVERLAPPING   # = ref_pos[100] + 480
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, 0, 50, 579)[0] == rr.SAME
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, 0, 50, 627)[0] == rr.SAME_OVERLAPPING   # = ref_pos[150] + 480
    assert decide_both((50, 0, 50, 100, 150), 50, ref_pos, begin_padded, 0, 50, 628)[0] == rr.SAME
    # better: the new state
    assert decide_both((44, 3, 48, 100, 150), 50, ref_pos, begin_padded, REGION_BEGIN, 43, pos) == \
        (rr.BETTER, REGION_BEGIN + 480 + 100, REGION_BEGIN + 480 + 147, 3, 2, 0)
    # an alignment that begins on the insertion: num_ins_begin counts the equal entries behind target_begin
    assert ref_pos[120:125] == [120, 121, 121, 121, 121]
    assert decide_both((44, 0, 50, 121, 160), 50, ref_pos, begin_padded, REGION_BEGIN, 43, pos)[5] == 3
    assert decide_both((44, 0, 50, 122, 160), 50, ref_pos, begin_padded, REGION_BEGIN, 43, pos)[5] == 2
    assert decide_both((44, 0, 50, 124, 160), 50, ref_pos, begin_padded, REGION_BEGIN, 43, pos)[5] == 0
    assert decide_both((44, 0, 50, 120, 160), 50, ref_pos, begin_padded, REGION_BEGIN, 43, pos)[5] == 0
    # results that are not of this read and window, or carry a status
    L = gtx.lib()
    rp, out = np.array(ref_pos, np.int32), np.zeros(1, gtx.REALIGN_DECISION)
    for bad in ((44, 0, 50, 100, n + 1, 0), (44, 0, 51, 100, 150, 0), (0, 0, 0, 0, 0, 1), (44, 0, 50, 150, 150, 0)):
        res = np.array([bad], gtx.REALIGN_RESULT)
        assert L.gtx_disc_realign_decide(res.ctypes.data_as(C.c_void_p), 50, rp.ctypes.data_as(C.c_void_p), n, begin_padded, REGION_BEGIN, 43, pos,
                                         out.ctypes.data_as(C.c_void_p)) == 1


def test_decide_over_seeded_results_equals_the_restatement(disc):
    rng = random.Random(37)
    pos = REGION_BEGIN + 500
    _, ref_pos, begin_padded, _ = both(disc, 40, [(pos, "I", "ACGTAC"), (pos + 30, "D", "NNNN")])
    n = len(ref_pos)
    seen = set()
    for _ in range(2000):
        tb = rng.choice((0, 1, rng.randrange(0, n - 1)))
        te = rng.choice((n, n - 1, rng.randrange(tb + 1, n + 1)))
        cb = rng.randrange(0, 10)
        ce = rng.randrange(cb + 1, 61)
        score = rng.randrange(-9, 60)
        seen.add(decide_both((score, cb, ce, tb, te), 60, ref_pos, begin_padded, rng.choice((0, REGION_BEGIN)), score + rng.randrange(-1, 2),
                             rng.choice((pos, 500, 640)))[0])
    assert seen == {rr.NO_PADDING, rr.BETTER, rr.SAME_OVERLAPPING, rr.SAME, rr.WORSE}
