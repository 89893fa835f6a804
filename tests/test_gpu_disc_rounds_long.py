"""The second pass from the aligner on, on the device, for a gtx_disc with gtx_disc_set_max_read_len(d, 1000): the cases of
tests/disc_rounds_long_cases.py through the intake and the rounds in both modes.  In long mode the reads' state, each read's list,
the counters, the statistics and the good-bits equal the restatement under the long limits (nobody is refused); on a default object
they equal the restatement as it stands (the pairs beyond 256 bases / 2 048 letters are refused and counted).  Every run is made
twice and leaves byte-equal arrays.  Then the whole chain behind a real first pass through lib.disc_second_file(...,
max_read_len=1000).  All values are integers or bits; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import disc_rounds_cases as rc
import disc_rounds_long_cases as lr
import disc_second_cases as sc
from disc_event_cases import cig, rd
from graphtyper_amd import lib as gtx
from oracle_lib import _p
from test_gpu_disc_rounds import Run
from test_gpu_disc_second import first_pass_words

pytestmark = pytest.mark.gpu


def whole(case, long_mode, keep=None):
    """the intake and all rounds, twice over fresh arrays, on an object in the mode -> the statistics and the good-bits (keep: a list
    that takes the bytes the run left)"""
    want = lr.expected_long(case) if long_mode else rc.expected(case)
    trace, n_list = want["trace"], len(want["lst"])
    cap = sum(new for _, new in (lr.room_long(case) if long_mode else rc.room(case)))
    seen = []
    run = Run(case)
    try:
        if long_mode:
            gtx.disc_set_max_read_len(run.h, gtx.MAX_READ_LONG)
        for _ in range(2):
            run.begin(cap)
            status, stats = run.rounds(0, n_list)
            assert status == 0
            second, events, support = run.state()
            differs = rc.state_differs(case, want["states"], want["entries"], want["support"], second, events, support)
            assert differs is None, differs
            assert stats == dict(pairs=trace["aligned"] + trace["refused"], pairs_aligned=trace["aligned"], pairs_refused=trace["refused"],
                                 windows_built=trace["windows"], rounds_done=n_list, rounds_skipped=trace["skipped"], compactions=stats["compactions"], events_wanted=0)
            good = list(gtx.disc_second_decide(run.a["table"], np.array(want["lst"], np.uint32), support))
            assert good == want["good"]
            seen.append((second.tobytes(), events[:run.used].tobytes(), support.tobytes(), run.used))
        assert seen[0] == seen[1]
        if keep is not None:
            keep.append(seen[0])
    finally:
        run.close()
    return stats, good


CASES = dict(lr.all_cases())


@pytest.mark.parametrize("name", sorted(CASES))
def test_nobody_is_refused_on_a_long_mode_object(name):
    stats, _ = whole(CASES[name], True)
    assert stats["pairs_refused"] == 0 and stats["pairs"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_default_object_refuses_what_it_did(name):
    stats, _ = whole(CASES[name], False)
    assert stats["pairs_refused"] > 0


@pytest.mark.parametrize("name", ("copies", "search", "own_ends", "purity", "fields"))
def test_the_sets_of_short_reads_leave_the_same_bytes_in_both_modes(name):
    """no read of these sets has more than 256 bases and no window more than 2 048 letters: a long-mode object refuses nobody either and
    leaves byte for byte what a default object leaves (test_disc_rounds_cases.py: the two restatements agree)"""
    for case in rc.cases(name):
        kept = []
        (by_long, good_long), (by_default, good_default) = whole(case, True, kept), whole(case, False, kept)
        assert by_long == by_default and good_long == good_default and kept[0] == kept[1] and by_long["pairs_refused"] == 0


def test_the_good_bits_depend_on_the_long_pairs():
    case = lr.one_read_of_1000()
    (by_long, good_long), (by_default, good_default) = whole(case, True), whole(case, False)
    assert by_long["pairs_refused"] == 0 and by_default["pairs_refused"] == by_default["pairs"] == by_long["pairs"]
    assert good_long != good_default


def test_the_chain_behind_a_real_first_pass():
    """two files of one region, each with one read of 1 000 bases beside its 150-base reads: gtx_disc_events_batch ->
    gtx_disc_first_pass_haplotypes_device -> gtx_disc_merge, then per file lib.disc_second_file(..., max_read_len=1000) over every
    twelfth read and the long one; the list, the reads, their lists, the counters, the statistics and the good-bits equal the
    restatement under the long limits, and two runs leave the same bytes in the event array"""
    import torch
    L = gtx.lib()
    files = []
    for seed in (7, 8):
        reference, rb, reads, _ = sc.simulated_file(seed)
        long_read = dict(rd(rb + 700, cig(("M", 1000)), reference[700:1700]), flag=3, mapq=60)
        files.append((reference, rb, sorted(reads + [long_read], key=lambda r: r["pos"]), sorted(reads[::12] + [long_read], key=lambda r: r["pos"])))
    reference, rb = files[0][0], files[0][1]
    merged = np.zeros(0, np.uint32)
    for f, (_, _, reads, _) in enumerate(files):
        words = first_pass_words(torch, L, sc.dc.Part(reference, rb, reads), f)
        out, n = np.zeros(len(merged) + len(words) + 16, np.uint32), C.c_uint64()
        gtx.check(L.gtx_disc_merge(_p(merged) if len(merged) else None, len(merged), _p(words), len(words), _p(out), len(out), C.byref(n)))
        merged = out[:n.value].copy()
    entries, letters = gtx.disc_indel_table(merged)
    table = [sc.ent(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), int(e["span"]), bool(e["good"]), int(e["file_index"]))
             for e in entries]
    aligned = beyond_default = 0
    for f, (_, _, _, mine) in enumerate(files):
        case = sc.Case(reference, rb, mine, table, file_index=f)
        want, a = lr.expected_long(case), sc.arrays(case)
        runs = []
        for _ in range(2):
            h = C.c_void_p()
            refb = reference.encode("latin-1")
            gtx.check(L.gtx_disc_create(refb, len(refb), rb, 0, C.byref(h)))
            try:
                runs.append(gtx.disc_second_file(h, len(reference), a["planes"], case.part.stride, a["reads"], a["cigar"], merged, f, bucket_size=case.bucket_size,
                                                 max_read_len=1000))
            finally:
                torch.cuda.synchronize()
                L.gtx_disc_destroy(h)
        got = runs[0]
        trace = want["trace"]
        assert list(got["lst"]) == want["lst"] and len(want["lst"]) > 0
        events = np.array([e for per in got["lists"] for e in per], gtx.DISC_SECOND_EVENT).reshape(-1)
        second = got["second"].copy()
        second["first_event"] = np.concatenate([[0], np.cumsum(second["n_events"])[:-1]])
        differs = rc.state_differs(case, want["states"], want["entries"], want["support"], second, events, got["support"])
        assert differs is None, differs
        assert list(got["good"]) == want["good"]
        assert (got["stats"]["pairs_aligned"], got["stats"]["pairs_refused"], got["stats"]["rounds_done"]) == (trace["aligned"], 0, len(want["lst"]))
        assert trace["refused"] == 0
        assert runs[0]["second"].tobytes() == runs[1]["second"].tobytes() and runs[0]["lists"] == runs[1]["lists"]
        assert runs[0]["support"].tobytes() == runs[1]["support"].tobytes()
        aligned += trace["aligned"]
        beyond_default += rc.expected(case)["trace"]["refused"]
    assert aligned > 8 and beyond_default > 0
