"""The second pass's kernel source (graphtyper_amd/csrc/gtx_disc_second_dev.hpp) run through a sequential wave under
AddressSanitizer / UBSan (tests/emu_disc_second -- a stand-alone program), against the plain restatement of the reference's text
(tests/disc_second_ref.py): per read its state, the two bucket arrays, max_read_size, the grouping by bucket, the found-bits, and
the pairs of the rounds in the reference's order of visit.  All values are integers; there is no tolerance.  Every array is a heap
block of exactly its size and there is no sanitizer report.  The restatement itself is held to a second statement of the score and
the ends (alignment columns, counted), the list of the host entry point gtx_disc_second_plan to the restatement's, and the table
of gtx_disc_indel_table to the words it is read from.  The device: test_gpu_disc_second.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import disc_second_cases as sc
import disc_second_ref as ref
import emu_programs
from graphtyper_amd import lib as gtx
from oracle_lib import _p


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_second", tmp_path_factory.mktemp("emu_disc_second"))


@pytest.mark.parametrize("name", sorted(sc.SETS))
def test_the_set_holds_what_it_is_for(name):
    sc.FACTS[name](sc.cases(name))


def test_the_launch_shapes_hold_what_they_are_for():
    sc.facts_launches()


def test_the_two_statements_of_the_score_and_the_ends_agree():
    """every read of every set whose CIGAR stays inside the read and the region: the walk of the reference's text and the count
    of alignment columns give the same score, pos_end, clips and IS_CLIPPED"""
    seen = 0
    for name in sorted(sc.SETS):
        for case in sc.cases(name):
            for i, (read, state) in enumerate(zip(case.reads, sc.expected(case)["taken"]["reads"])):
                if not ref.inside(case.reference, case.region_begin, read):
                    continue
                score, pos_end, begin, end, clipped = ref.column_statement(case.reference, case.region_begin, read)
                got = (state["score"], state["pos_end"], state["num_clipped_begin"], state["num_clipped_end"], bool(state["flags"] & ref.IS_CLIPPED))
                assert got == (score, pos_end, begin, end, clipped or bool(read["flag"] & ref.IS_CLIPPED)), (name, i)
                seen += 1
    assert seen > 3000


@pytest.mark.parametrize("name", sorted(sc.SETS))
def test_every_set_equals_the_restatement(emu, tmp_path, name):
    assert sc.judge(name, functools.partial(emu_programs.run, emu, tmp_path)) is None


@pytest.mark.parametrize("name", sorted(sc.LAUNCHES))
def test_every_launch_shape_equals_the_restatement(emu, tmp_path, name):
    assert sc.judge(name, functools.partial(emu_programs.run, emu, tmp_path)) is None


@pytest.mark.parametrize("name", sorted(sc.SETS))
def test_the_plan_of_the_library_is_the_restatements(name):
    """gtx_disc_second_plan (host) over the restatement's found-bits, for every file index the table names and one it does not"""
    for case in sc.cases(name):
        table, _ = sc.table_arrays(case.table)
        found = sc.expected(case)["found"]
        for file_index in sorted({e["file_index"] for e in case.table} | {7}):
            assert list(gtx.disc_second_plan(table, sc.found_words(found), file_index)) == ref.plan(case.table, found, file_index)


def test_a_list_that_does_not_fit_is_refused():
    case = sc.cases("plan_rules")[0]
    table, _ = sc.table_arrays(case.table)
    found, n = sc.found_words(sc.expected(case)["found"]), C.c_uint32()
    out = np.full(8, 0xA5A5A5A5, np.uint32)
    L = gtx.lib()
    assert L.gtx_disc_second_plan(_p(table), len(table), _p(found), 0, _p(out), 5, C.byref(n)) == 5 and n.value == 6 and (out == 0xA5A5A5A5).all()
    assert L.gtx_disc_second_plan(_p(table), len(table), _p(found), 0, _p(out), 6, C.byref(n)) == 0 and (out[6:] == 0xA5A5A5A5).all()
    assert L.gtx_disc_second_plan(None, 0, None, 0, None, 0, C.byref(n)) == 0 and n.value == 0  # an empty table: an empty list
    assert L.gtx_disc_second_plan(_p(table), len(table), None, 0, _p(out), 8, C.byref(n)) == 1 and L.gtx_disc_second_plan(_p(table), 1, _p(found), 0, _p(out), 8, None) == 1


def words_of(table):
    """a file's result words (include/gtx.h: gtx_disc_first_pass_haplotypes) that hold `table` and nothing else of interest: every
    entry with a phase entry of its own, so that the reader has to step over one"""
    w = [len(table)]
    for k, e in enumerate(table):
        w += [e["pos"], ord(e["type"]), len(e["seq"])] + [ord(c) for c in e["seq"]]
        w += [3, 0, 2, 1, 1, 0, 60, 9, 5, -1 & 0xFFFFFFFF, -1 & 0xFFFFFFFF, e["span"], 1, int(e["good"]), 77, e["file_index"] & 0xFFFFFFFF]
        w += [k % 2] + ([e["pos"] + 3, ord("X"), 1, ord("A"), 4] if k % 2 else [])
    return np.array(w + [0], np.uint32)  # (no haplotype entries)


def test_the_table_is_read_off_the_words():
    case = sc.cases("plan_rules")[0]
    want, letters = sc.table_arrays(case.table)
    words = words_of(case.table)
    got, seq = gtx.disc_indel_table(words)
    assert np.array_equal(got, want) and np.array_equal(seq, letters) and len(got) == 12
    # ... and off the words the library's own merge writes of them
    L = gtx.lib()
    merged, n = np.zeros(4 * len(words), np.uint32), C.c_uint64()
    gtx.check(L.gtx_disc_merge(None, 0, _p(words), len(words), _p(merged), len(merged), C.byref(n)))
    got, seq = gtx.disc_indel_table(merged[:n.value])
    assert np.array_equal(got, want) and np.array_equal(seq, letters)
    empty, none = gtx.disc_indel_table(np.zeros(0, np.uint32))
    assert len(empty) == 0 and len(none) == 0
    n32, n64 = C.c_uint32(), C.c_uint64()
    for cut in (1, 3, len(words) // 2, len(words) - 2):  # words that end early: refused, not read behind their end
        part = np.ascontiguousarray(words[:cut])
        assert L.gtx_disc_indel_table(_p(part), len(part), None, 0, C.byref(n32), None, 0, C.byref(n64)) == 1
    small = np.zeros(3, gtx.DISC_INDEL)
    assert L.gtx_disc_indel_table(_p(words), len(words), _p(small), 3, C.byref(n32), _p(np.zeros(64, np.uint8)), 64, C.byref(n64)) == 5 and n32.value == 12


def test_the_device_entry_points_refuse_an_object_without_a_device():
    """a gtx_disc made with device -1: GTX_ERR_NO_DEVICE behind the argument checks, GTX_ERR_ARG in front of them (nothing is
    dereferenced either way: the addresses are made up)"""
    L, h, p = gtx.lib(), C.c_void_p(), 0x1000
    gtx.check(L.gtx_disc_create(b"ACGTACGTAC", 10, 100, -1, C.byref(h)))
    try:
        intake = [h, p, 16, p, p, 4, 50, p, p, 1, 3] + [p] * 7 + [None]
        rounds = [h, p, 0, 1, p, 1, p, 4, None, 0, 50, p, p, p, p, p, p, 8, p, None]
        assert L.gtx_disc_second_intake(*intake) == 2 and L.gtx_disc_second_candidates(*rounds) == 2
        assert L.gtx_disc_indel_table_upload(h, p, 1, p, 3, p, p, None) == 2
        for at, bad in ((1, None), (1, p + 2), (2, 24), (6, 0), (11, None), (17, p + 1)):
            args = list(intake)
            args[at] = bad
            assert L.gtx_disc_second_intake(*args) == 1, at
        for at, bad in ((1, None), (3, 0), (10, 0), (16, None), (18, None), (18, p + 2)):
            args = list(rounds)
            args[at] = bad
            assert L.gtx_disc_second_candidates(*args) == (2 if (at, bad) == (3, 0) else 1), at  # (k1 == k0: an empty slice is legal)
        args = list(rounds)
        args[2], args[3] = 2, 1
        assert L.gtx_disc_second_candidates(*args) == 1 and L.gtx_disc_indel_table_upload(h, None, 1, p, 3, p, p, None) == 1
    finally:
        L.gtx_disc_destroy(h)
