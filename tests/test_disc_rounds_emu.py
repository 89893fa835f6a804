"""The rounds' kernel source (graphtyper_amd/csrc/gtx_disc_rounds_dev.hpp, with gtx_disc_second_dev.hpp for a round's pairs and
gtx_realign_dev.hpp for the alignments) run through a sequential wave under AddressSanitizer / UBSan (tests/emu_disc_rounds -- a
stand-alone program), against the plain restatement (tests/disc_rounds_ref.py): the reads' state, each read's list, the counters and
the statistics; every window, ref_pos value and applied flag against gtx_disc_realign_target.  Every array is a heap block of
exactly its size -- a round's arena exactly the sum of its slots -- and there is no sanitizer report.  All values are integers;
there is no tolerance.  The device: test_gpu_disc_rounds.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import disc_rounds_cases as rc
import emu_programs
from graphtyper_amd import lib as gtx
from test_disc_rounds_cases import ALL, case_of


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_rounds", tmp_path_factory.mktemp("emu_disc_rounds"))


def differs(case, got, at=None):
    want = rc.expected(case)
    states, entries, support = (want["states"], want["entries"], want["support"]) if at is None else want["before"][at]
    return rc.state_differs(case, states, entries, support, got["second"], got["events"], got["support"])


@pytest.mark.parametrize("name,k", ALL)
def test_every_case_equals_the_restatement(emu, tmp_path, name, k):
    case = case_of(name, k)
    want = rc.expected(case)
    trace = want["trace"]
    got = rc.through(functools.partial(emu_programs.run, emu, tmp_path), case)
    assert got["status"] == 0 and differs(case, got) is None
    assert got["stats"] == dict(rounds_done=len(want["lst"]), rounds_skipped=trace["skipped"], pairs_aligned=trace["aligned"], pairs_refused=trace["refused"],
                                windows_built=trace["windows"], compactions=got["stats"]["compactions"], events_wanted=0)
    # the windows: letters, ref_pos values and applied flags of gtx_disc_realign_target over the same events
    L = gtx.lib()
    h = C.c_void_p()
    refb = case.reference.encode("latin-1")
    gtx.check(L.gtx_disc_create(refb, len(refb), case.region_begin, -1, C.byref(h)))
    try:
        seen = 0
        for k_, read, letters, ref_pos, flags in got["windows"]:
            indel = case.table[want["lst"][k_]]
            own = [] if read is None else [case.table[t] for t, _ in want["before"][k_][1][read]]
            assert len(own) == len(flags)
            begin = max(0, indel["pos"] - want["taken"]["max_read_size"] - 100 - case.region_begin)
            if begin >= len(case.reference):
                assert len(letters) == 0
                continue
            t_letters, t_pos, _, bits = gtx.disc_realign_target(h, want["taken"]["max_read_size"], [(e["pos"], e["type"], e["seq"]) for e in [indel] + own])
            assert letters == t_letters and np.array_equal(ref_pos, t_pos) and flags == [(bits >> (e + 1)) & 1 for e in range(len(own))], (k_, read)
            seen += 1
        assert seen == trace["windows"]
    finally:
        L.gtx_disc_destroy(h)


def test_slices_and_the_event_array(emu, tmp_path):
    """[0, k) then -- from the restatement's state in front of round k -- [k, n); the array exactly large enough (with compactions)
    and one entry short"""
    case = rc.cases("again")[0]
    run = functools.partial(emu_programs.run, emu, tmp_path)
    room = rc.room(case)
    n_list, need = len(room), max(live + new for live, new in room)
    for k in range(n_list + 1):
        first = rc.through(run, case, 0, k)
        assert first["status"] == 0 and differs(case, first, at=k) is None
        second = rc.through(run, case, k, n_list, before=k)
        assert second["status"] == 0 and differs(case, second) is None
    exact = rc.through(run, case, event_cap=need)
    assert exact["status"] == 0 and exact["stats"]["compactions"] >= 1 and differs(case, exact) is None
    short = rc.through(run, case, event_cap=need - 1)
    stop = next(k for k, (live, new) in enumerate(room) if live + new > need - 1)
    assert short["status"] == 5 and short["stats"]["rounds_done"] == stop and short["stats"]["events_wanted"] == sum(room[stop])
    assert differs(case, short, at=stop) is None
