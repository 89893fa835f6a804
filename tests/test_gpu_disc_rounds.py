"""The second pass from the aligner on, on the device (include/gtx.h: gtx_disc_second_rounds, gtx_disc_second_decide): every case set
and launch shape of tests/disc_rounds_cases.py through the intake and the rounds, with guard bytes behind every output array; the
reads' state, each read's list, the counters, the statistics and the good-bits equal the plain restatement
(tests/disc_rounds_ref.py); every run is made twice and leaves byte-equal arrays (the lists are placed by a scan, not by an atomic
bump).  Then slices, the event array exactly large enough and one entry short, a stream of the caller's, the argument errors, and
the whole chain behind a real first pass over two files through lib.disc_second_file.  All values are integers or bits; there is no
tolerance.  tests/test_disc_rounds_cases.py holds the sets to what they are meant to contain and the restatement to a second witness."""
import ctypes as C

import numpy as np
import pytest

import disc_rounds_cases as rc
import disc_second_cases as sc
from graphtyper_amd import lib as gtx
from oracle_lib import _p
from test_gpu_disc_second import Run as SecondRun, first_pass_words

pytestmark = pytest.mark.gpu


class Run(SecondRun):
    """a case's arrays on the device, its intake, and rounds over an event array and counters of the run's own"""

    def zeroed(self, nbytes):
        t = self.out(nbytes)
        t[:nbytes] = 0
        return t

    def begin(self, cap, stream=None):
        self.intake(stream)
        self.cap, self.used = cap, 0
        self.d_ev, self.d_support = self.out(cap * gtx.DISC_SECOND_EVENT.itemsize), self.zeroed(self.nt * gtx.DISC_SECOND_SUPPORT.itemsize)

    def args(self, k0, k1, stream=None):
        o = self.o
        self.n_used, self.stats = C.c_uint32(self.used), gtx.DiscRoundsStats()
        return [self.h, self.d_planes.data_ptr(), self.case.part.stride, self.d_lst.data_ptr(), k0, k1, self.d_table.data_ptr(), self.d_letters.data_ptr(), self.nt,
                len(self.a["letters"]), o["second"].data_ptr(), self.n, self.d_ev.data_ptr(), self.cap, C.byref(self.n_used), self.case.bucket_size,
                o["bucket_max"].data_ptr(), o["global_max"].data_ptr(), o["max_read_size"].data_ptr(), o["bucket_reads"].data_ptr(), o["bucket_off"].data_ptr(),
                self.d_support.data_ptr(), C.byref(self.stats), stream]

    def rounds(self, k0, k1, stream=None):
        self.torch.cuda.synchronize()
        rc_ = self.L.gtx_disc_second_rounds(*self.args(k0, k1, stream))
        self.torch.cuda.synchronize()
        assert rc_ in (0, 5), gtx.GtxError(rc_)
        self.used = self.n_used.value
        return rc_, self.stats.as_dict()

    def grow(self, cap):
        bigger = self.out(cap * gtx.DISC_SECOND_EVENT.itemsize)
        nbytes = self.used * gtx.DISC_SECOND_EVENT.itemsize
        bigger[:nbytes] = self.d_ev[:nbytes]
        self.d_ev, self.cap = bigger, cap

    def state(self):
        """-> (second, the whole event array, support), the guards checked, and with them the intake's other arrays, which the rounds
        leave alone"""
        second = self.down(self.o["second"], gtx.DISC_SECOND_READ, self.n)
        for key, dtype, count in (("bucket_max", np.int32, self.nb), ("global_max", np.int32, self.nb), ("max_read_size", np.uint32, 1),
                                  ("bucket_reads", np.uint32, self.n), ("bucket_off", np.uint32, self.nb + 1)):
            assert np.array_equal(self.down(self.o[key], dtype, count), self.got[key]), key
        return second, self.down(self.d_ev, gtx.DISC_SECOND_EVENT, self.cap), self.down(self.d_support, gtx.DISC_SECOND_SUPPORT, self.nt)

    def differs(self, at=None):
        """None, or how the device's state differs from the restatement's at the end (at None) or in front of round `at`"""
        want = rc.expected(self.case)
        states, entries, support = (want["states"], want["entries"], want["support"]) if at is None else want["before"][at]
        second, events, got = self.state()
        assert all(int(r["first_event"]) + int(r["n_events"]) <= self.used for r in second)
        return rc.state_differs(self.case, states, entries, support, second, events, got)


def whole(case, stream=None, cap=None):
    """the intake and all rounds, twice over fresh arrays -> the run; asserts the restatement, the statistics, the good-bits and that
    the two runs left the same bytes"""
    want = rc.expected(case)
    trace, n_list = want["trace"], len(want["lst"])
    cap = sum(new for _, new in rc.room(case)) if cap is None else cap  # room for every list ever made
    seen = []
    run = Run(case)
    try:
        for _ in range(2):
            run.begin(cap, stream)
            status, stats = run.rounds(0, n_list, stream)
            assert status == 0 and run.differs() is None, run.differs()
            assert stats == dict(pairs=trace["aligned"] + trace["refused"], pairs_aligned=trace["aligned"], pairs_refused=trace["refused"],
                                 windows_built=trace["windows"], rounds_done=n_list, rounds_skipped=trace["skipped"], compactions=stats["compactions"], events_wanted=0)
            second, events, support = run.state()
            seen.append((second.tobytes(), events[:run.used].tobytes(), support.tobytes(), run.used, stats["compactions"]))
            good = gtx.disc_second_decide(run.a["table"], np.array(want["lst"], np.uint32), support)
            assert list(good) == want["good"]
        assert seen[0] == seen[1]
    finally:
        run.close()
    return seen[0]


@pytest.mark.parametrize("name", sorted(rc.SETS))
def test_every_set_equals_the_restatement(name):
    for case in rc.cases(name):
        whole(case)


@pytest.mark.parametrize("n_pairs", rc.SHAPE_PAIRS)
def test_every_launch_shape_equals_the_restatement(n_pairs):
    """rounds of 0, 1, 4, 5, 63, 64 and 65 pairs; windows of 383, 385, 447 and 449 letters; lists of 0 and 1 entries"""
    whole(rc.shape_case(n_pairs))


def test_slices_equal_the_whole_run():
    """[0, k) then [k, n) for every k: the same bytes as one call"""
    case = rc.cases("again")[0]
    n_list = len(rc.expected(case)["lst"])
    cap = sum(new for _, new in rc.room(case))
    one = whole(case)
    run = Run(case)
    try:
        for k in range(n_list + 1):
            run.begin(cap)
            for k0, k1 in ((0, k), (k, n_list)):
                status, stats = run.rounds(k0, k1)
                assert status == 0 and stats["rounds_done"] == k1 - k0
                if k1 == k:
                    assert run.differs(at=k) is None
            second, events, support = run.state()
            assert (second.tobytes(), events[:run.used].tobytes(), support.tobytes(), run.used) == one[:4], k
    finally:
        run.close()


def test_the_event_array_exactly_large_enough_and_one_entry_short():
    case = rc.cases("again")[0]
    want, room = rc.expected(case), rc.room(case)
    n_list, need = len(want["lst"]), max(live + new for live, new in room)
    assert need < sum(new for _, new in room)  # an array of `need` entries has to be compacted on the way
    exact = whole(case, cap=need)
    assert exact[4] >= 1                       # it was
    run = Run(case)
    try:
        run.begin(need - 1)
        stop = next(k for k, (live, new) in enumerate(room) if live + new > need - 1)
        status, stats = run.rounds(0, n_list)
        assert status == 5 and stats["rounds_done"] == stop and stats["events_wanted"] == sum(room[stop])
        assert run.differs(at=stop) is None    # exactly the beginning of the round it stopped in front of
        run.grow(sum(new for _, new in room))
        status, stats = run.rounds(stop, n_list)
        assert status == 0 and stats["rounds_done"] == n_list - stop and run.differs() is None
        good = gtx.disc_second_decide(run.a["table"], np.array(want["lst"], np.uint32), run.state()[2])
        assert list(good) == want["good"]
    finally:
        run.close()


@pytest.mark.parametrize("k", range(len(rc.cases("copies"))))
def test_copies_in_an_array_exactly_large_enough_and_one_entry_short(k):
    """the host driver's part -- capacity, where the scan places the lists, when it compacts -- for lists that a window of up to 130
    copied letters made: max(live + new) entries are enough, one fewer stops in front of the round that does not fit, with
    events_wanted and the state in front of it, and the call goes on in a larger array"""
    case = rc.cases("copies")[k]
    want, room = rc.expected(case), rc.room(case)
    n_list, need = len(want["lst"]), max(live + new for live, new in room)
    whole(case, cap=need)
    run = Run(case)
    try:
        run.begin(need - 1)
        stop = next(k_ for k_, (live, new) in enumerate(room) if live + new > need - 1)
        status, stats = run.rounds(0, n_list)
        assert status == 5 and stats["rounds_done"] == stop and stats["events_wanted"] == sum(room[stop]) and run.differs(at=stop) is None
        run.grow(need)
        status, stats = run.rounds(stop, n_list)
        assert status == 0 and stats["rounds_done"] == n_list - stop and run.differs() is None
    finally:
        run.close()


def test_own_ends_slices_equal_the_whole_run():
    """the own_ends lists cannot come out of lib.disc_second_file (its list is the plan's, not the set's), so they go through
    gtx_disc_second_rounds directly: one call, and a call per round, leave the same bytes"""
    for case in rc.cases("own_ends"):
        n_list = len(rc.expected(case)["lst"])
        one = whole(case)
        run = Run(case)
        try:
            run.begin(sum(new for _, new in rc.room(case)))
            for k in range(n_list):
                status, _ = run.rounds(k, k + 1)
                assert status == 0 and run.differs(at=k + 1) is None
            second, events, support = run.state()
            assert (second.tobytes(), events[:run.used].tobytes(), support.tobytes(), run.used) == one[:4]
        finally:
            run.close()


def test_a_stream_of_the_callers():
    import torch
    whole(rc.cases("chain")[1], stream=torch.cuda.Stream().cuda_stream)


def test_the_argument_errors():
    case = rc.cases("edges")[0]
    run, host = Run(case), Run(case, device=-1)
    try:
        L = run.L
        n_list = len(rc.expected(case)["lst"])
        run.begin(64)
        host.o, host.d_ev, host.d_support, host.cap, host.used = run.o, run.d_ev, run.d_support, run.cap, 0
        assert L.gtx_disc_second_rounds(*host.args(0, n_list)) == 2  # an object made without a device
        for at in (1, 3, 6, 10, 12, 16, 17, 18, 19, 20, 21):
            for bad in (None, run.d_planes.data_ptr() + 2):
                args = run.args(0, n_list)
                args[at] = bad
                assert L.gtx_disc_second_rounds(*args) == 1, at
        for at, bad in ((0, None), (14, None), (22, None), (15, 0), (2, 24), (2, 0)):
            args = run.args(0, n_list)
            args[at] = bad
            assert L.gtx_disc_second_rounds(*args) == 1, at
        assert L.gtx_disc_second_rounds(*run.args(2, 1)) == 1        # a slice the wrong way round
        run.used = 65
        assert L.gtx_disc_second_rounds(*run.args(0, n_list)) == 1   # more entries in use than the array holds
        run.used = 0
        # a read whose list does not lie inside the entries in use
        second = run.state()[0]
        second[0]["first_event"], second[0]["n_events"] = 3, 2
        run.o["second"][:len(second.tobytes())] = run.torch.from_numpy(second.view(np.uint8).copy()).to("cuda:0")
        run.used = 4
        assert L.gtx_disc_second_rounds(*run.args(0, n_list)) == 1
        run.torch.cuda.synchronize()
        # an empty slice and no reads: legal, nothing is written but the statistics
        run.begin(64)
        run.d_ev, run.d_support = run.out(64 * 8), run.out(run.nt * gtx.DISC_SECOND_SUPPORT.itemsize)
        before = run.o["second"].cpu().numpy().copy()
        assert L.gtx_disc_second_rounds(*run.args(2, 2)) == 0 and run.stats.rounds_done == 0
        args = run.args(0, n_list)
        args[11] = 0
        assert L.gtx_disc_second_rounds(*args) == 0 and run.stats.rounds_done == 0
        args[1] = args[10] = None
        assert L.gtx_disc_second_rounds(*args) == 0
        run.torch.cuda.synchronize()
        assert np.array_equal(run.o["second"].cpu().numpy(), before) and (run.d_ev.cpu().numpy() == 0xA5).all() and (run.d_support.cpu().numpy() == 0xA5).all()
        # the final decision's arguments
        table = run.a["table"]
        bits = np.zeros(1, np.uint32)
        assert L.gtx_disc_second_decide(_p(table), len(table), _p(np.array([len(table)], np.uint32)), 1, _p(np.zeros(len(table), gtx.DISC_SECOND_SUPPORT)), _p(bits)) == 1
        assert L.gtx_disc_second_decide(None, len(table), None, 0, None, _p(bits)) == 1
    finally:
        run.close()
        host.close()


def test_the_chain_behind_a_real_first_pass():
    """two files of one region: gtx_disc_events_batch -> gtx_disc_first_pass_haplotypes_device -> gtx_disc_merge, then per file
    lib.disc_second_file -- the table, the intake, the plan, the rounds (from an event array that is too small at first, so the call
    is continued) and the final decision -- equal the restatement: the list, the reads, their lists, the counters, the good-bits.  The
    second pass runs over every fourth read of a file, which keeps the restatement's alignments (plain Python) to a few seconds"""
    import torch
    L = gtx.lib()
    files = [sc.simulated_file(seed) for seed in (7, 8)]
    reference, rb = files[0][0], files[0][1]
    merged = np.zeros(0, np.uint32)
    for f, (_, _, reads, _) in enumerate(files):
        words = first_pass_words(torch, L, rc.sc.dc.Part(reference, rb, reads), f)
        out, n = np.zeros(len(merged) + len(words) + 16, np.uint32), C.c_uint64()
        gtx.check(L.gtx_disc_merge(_p(merged) if len(merged) else None, len(merged), _p(words), len(words), _p(out), len(out), C.byref(n)))
        merged = out[:n.value].copy()
    entries, letters = gtx.disc_indel_table(merged)
    table = [sc.ent(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), int(e["span"]), bool(e["good"]), int(e["file_index"]))
             for e in entries]
    aligned = 0
    for f, (_, _, reads, _) in enumerate(files):
        case = sc.Case(reference, rb, reads[::4], table, file_index=f)
        want, a = rc.expected(case), sc.arrays(case)
        h = C.c_void_p()
        refb = reference.encode("latin-1")
        gtx.check(L.gtx_disc_create(refb, len(refb), rb, 0, C.byref(h)))
        try:
            got = gtx.disc_second_file(h, len(reference), a["planes"], case.part.stride, a["reads"], a["cigar"], merged, f, bucket_size=case.bucket_size, event_cap=4)
        finally:
            torch.cuda.synchronize()
            L.gtx_disc_destroy(h)
        trace = want["trace"]
        assert list(got["lst"]) == want["lst"] and len(want["lst"]) > 0
        events = np.array([e for per in got["lists"] for e in per], gtx.DISC_SECOND_EVENT).reshape(-1)
        second = got["second"].copy()
        second["first_event"] = np.concatenate([[0], np.cumsum(second["n_events"])[:-1]])
        assert rc.state_differs(case, want["states"], want["entries"], want["support"], second, events, got["support"]) is None
        assert list(got["good"]) == want["good"]
        assert (got["stats"]["pairs_aligned"], got["stats"]["pairs_refused"], got["stats"]["rounds_done"]) == (trace["aligned"], trace["refused"], len(want["lst"]))
        aligned += trace["aligned"]
    assert aligned > 20
