"""Discovery's two host loops on the device (include/gtx.h: gtx_disc_second_file, gtx_discover_region).

gtx_disc_second_file over every case set of tests/disc_rounds_cases.py -- the table's words written by tests/disc_variants_cases.py --
equals the plain restatement (disc_rounds_cases.expected): the list, the reads, their lists, the counters, the good-bits, the
statistics; it equals lib.disc_second_file, the same steps strung from the binding; and from an event array of four entries, so that
the call is continued, it leaves the same bytes.  gtx_discover_region over the end-to-end file set of tests/disc_variants_cases.py
equals the host chain (the oracle's first pass and merge, the restatement of each file's rounds, the restatement of the records and
the text: tests/test_disc_variants_cases.py holds that chain to what the set is for): the merged words, the final good flags, the
records, the text -- with the default capacities, with both at their smallest, with one and with three threads, and with
max_read_len 1000.  Then a file with a read of 1 000 bases in both modes, the argument errors and the empty inputs.  All values are
integers, letters or bits; there is no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import disc_event_cases as dc
import disc_rounds_cases as rc
import disc_rounds_long_cases as lr
import disc_second_cases as sc
import disc_variants_cases as vc
import disc_variants_ref as ref
from graphtyper_amd import lib as gtx
from oracle_lib import _p

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_DEVICE = 1, 2


# ---- a file's second pass ---------------------------------------------------------------------------------------------------------
def plain(case):
    """the case with the plan's own list and the intake's own state, which is what a whole second pass runs from"""
    if case.lst is None and not case.state and not case.entries:
        return case
    return sc.Case(case.reference, case.region_begin, case.reads, case.table, case.bucket_size, case.file_index, stride=case.part.stride, fill=case.part.fill)


class File:
    """a case's reads on the device and a gtx_disc of its region"""

    def __init__(self, case, max_read_len=None):
        import torch
        self.torch, self.L, self.case, self.a = torch, gtx.lib(), case, sc.arrays(case)
        self.h = C.c_void_p()
        refb = case.reference.encode("latin-1")
        gtx.check(self.L.gtx_disc_create(refb, len(refb), case.region_begin, 0, C.byref(self.h)))
        if max_read_len is not None:
            gtx.disc_set_max_read_len(self.h, max_read_len)
        dev = lambda x: torch.from_numpy(np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
        self.d_planes, self.d_reads, self.d_cigar = dev(self.a["planes"]), dev(self.a["reads"]), dev(self.a["cigar"])
        self.words = vc.words_of(case.table, ())
        torch.cuda.synchronize()

    def in_c(self, event_cap=0, state=True):
        return gtx.disc_second_file_c(self.h, self.d_planes.data_ptr(), self.case.part.stride, self.d_reads.data_ptr(), self.d_cigar.data_ptr(), len(self.a["reads"]),
                                      self.words, self.case.file_index, bucket_size=self.case.bucket_size, event_cap=event_cap, state=state)

    def from_the_binding(self, event_cap=None):
        return gtx.disc_second_file(self.h, len(self.case.reference), self.a["planes"], self.case.part.stride, self.a["reads"], self.a["cigar"], self.words,
                                    self.case.file_index, bucket_size=self.case.bucket_size, event_cap=event_cap)

    def close(self):
        self.torch.cuda.synchronize()
        self.L.gtx_disc_destroy(self.h)


def differs_from_the_restatement(case, want, got):
    trace = want["trace"]
    if list(got["lst"]) != want["lst"]:
        return "the list"
    events = np.array([e for per in got["lists"] for e in per], gtx.DISC_SECOND_EVENT).reshape(-1)
    second = got["second"].copy()
    second["first_event"] = np.concatenate([[0], np.cumsum(second["n_events"])[:-1]]) if len(second) else second["first_event"]
    how = rc.state_differs(case, want["states"], want["entries"], want["support"], second, events, got["support"])
    if how is not None:
        return how
    if list(got["good"]) != want["good"]:
        return "the good-bits"
    stats = dict(got["stats"])
    stats.pop("compactions")
    if stats != dict(pairs=trace["aligned"] + trace["refused"], pairs_aligned=trace["aligned"], pairs_refused=trace["refused"], windows_built=trace["windows"],
                     rounds_done=len(want["lst"]), rounds_skipped=trace["skipped"]):
        return "the statistics: %s" % stats
    return None


def same(a, b):
    """two runs of a file's second pass: the list, the good-bits, per read its state and its list, the counters"""
    keys = [k for k in gtx.DISC_SECOND_READ.names if k != "first_event"]
    return (list(a["lst"]) == list(b["lst"]) and list(a["good"]) == list(b["good"]) and a["lists"] == b["lists"] and a["support"].tobytes() == b["support"].tobytes() and
            all(np.array_equal(a["second"][k], b["second"][k]) for k in keys))


@pytest.mark.parametrize("name", sorted(rc.SETS))
def test_second_file_equals_the_restatement_and_the_binding(name):
    for k, case in enumerate(map(plain, rc.cases(name))):
        f = File(case)
        try:
            got, by_binding = f.in_c(), f.from_the_binding()
        finally:
            f.close()
        assert differs_from_the_restatement(case, rc.expected(case), got) is None, k
        assert same(got, by_binding) and got["stats"] == by_binding["stats"], k


@pytest.mark.parametrize("name", sorted(rc.SETS))
def test_second_file_continued_from_an_event_array_of_four(name):
    seen = 0
    for k, case in enumerate(map(plain, rc.cases(name))):
        f = File(case)
        try:
            got, small, small_by_binding, bare = f.in_c(), f.in_c(event_cap=4), f.from_the_binding(event_cap=4), f.in_c(event_cap=4, state=False)
        finally:
            f.close()
        assert differs_from_the_restatement(case, rc.expected(case), small) is None, k
        assert same(got, small) and same(small, small_by_binding) and small["stats"] == small_by_binding["stats"], k
        assert list(bare["lst"]) == list(small["lst"]) and list(bare["good"]) == list(small["good"]) and bare["stats"] == small["stats"] and "second" not in bare
        seen += max([live + new for live, new in rc.room(case)] or [0]) > 4  # (a round that needs more than four entries: the array is grown)
    assert (seen > 0) == (name not in ("fields", "limits"))


def test_second_file_with_a_read_of_1000_bases_in_both_modes():
    """disc_rounds_long_cases.one_read_of_1000: the good-bits that module pins for a default object (every pair refused) and for one in
    long mode (nobody refused), which differ"""
    case = lr.one_read_of_1000()
    got = {}
    for mode, max_read_len in (("default", None), ("long", 1000)):
        f = File(case, max_read_len)
        try:
            got[mode] = f.in_c()
        finally:
            f.close()
    assert differs_from_the_restatement(case, rc.expected(case), got["default"]) is None
    assert differs_from_the_restatement(case, lr.expected_long(case), got["long"]) is None
    assert list(got["default"]["good"]) == rc.expected(case)["good"] != lr.expected_long(case)["good"] == list(got["long"]["good"])
    assert got["long"]["stats"]["pairs_refused"] == 0 and got["default"]["stats"]["pairs_refused"] == got["default"]["stats"]["pairs"] > 0


def test_second_file_argument_errors():
    L = gtx.lib()
    case = rc.cases("chain")[0]
    f = File(case)
    host = vc.host_handle(case)
    try:
        nt = len(case.table)
        bits, lst, n_list, stats = np.zeros(1, np.uint32), np.zeros(nt, np.uint32), C.c_uint32(), gtx.DiscRoundsStats()
        args = [f.h, f.d_planes.data_ptr(), case.part.stride, f.d_reads.data_ptr(), f.d_cigar.data_ptr(), len(case.reads), _p(f.words), len(f.words), 0, 50, 0, _p(bits),
                _p(lst), nt, C.byref(n_list), C.byref(stats), None, None, 0, None, None, None]
        assert L.gtx_disc_second_file(*args) == 0 and n_list.value == len(rc.expected(case)["lst"])
        for k in (0, 11, 14, 15):  # the object, the good-bits, n_list, the statistics
            assert L.gtx_disc_second_file(*[None if j == k else a for j, a in enumerate(args)]) == ERR_ARG, k
        assert L.gtx_disc_second_file(*[0 if j == 9 else a for j, a in enumerate(args)]) == ERR_ARG  # bucket_size 0
        assert L.gtx_disc_second_file(*[host if j == 0 else a for j, a in enumerate(args)]) == ERR_NO_DEVICE
        assert L.gtx_disc_second_file(*[len(f.words) // 2 if j == 7 else a for j, a in enumerate(args)]) == ERR_ARG  # words cut inside the table
        short = list(args)
        short[13] = len(rc.expected(case)["lst"]) - 1  # the list does not fit: its size, nothing else
        bits[:], lst[:] = 0xA5A5A5A5, 0xA5A5A5A5
        assert L.gtx_disc_second_file(*short) == 5 and n_list.value == len(rc.expected(case)["lst"]) and (lst == 0xA5A5A5A5).all() and (bits == 0xA5A5A5A5).all()
    finally:
        f.close()
        L.gtx_disc_destroy(host)


# ---- a region -----------------------------------------------------------------------------------------------------------------------
def file_arrays(reference, rb, reads):
    part = dc.Part(reference, rb, reads)
    a = dc.arrays(part)
    return dict(planes=a["planes"], plane_stride=part.stride, qual=a["qual"], qual_stride=a["qual"].shape[1], reads=a["reads"], cigar=a["cigar"])


@functools.lru_cache(maxsize=None)
def region_files():
    reference, rb, files = vc.simulated_files()
    return [file_arrays(reference, rb, reads) for reads in files]


@functools.lru_cache(maxsize=None)
def region_run(**params):
    reference, rb, _ = vc.simulated_files()
    return gtx.discover_region(reference, rb, vc.CONTIG, region_files(), **params)


def outputs(run):
    """the four outputs of a region run as bytes"""
    return run["words"].tobytes(), run["good"].tobytes(), (run["variants"].tobytes(), run["letters"], run["ids"].tobytes()), run["text"]


def region_differs(run):
    """None, or how a run over the end-to-end set differs from the host chain"""
    hc = vc.host_chain()
    if not np.array_equal(run["words"], hc["merged"]):
        return "the merged words"
    if run["good"].tolist() != hc["good"]:
        return "the final good flags"
    recs, letters, ids = vc.record_arrays(hc["recs"])
    if run["variants"].tobytes() != recs.tobytes() or run["letters"] != letters or run["ids"].tolist() != ids.tolist():
        return "the records"
    if run["text"] != hc["text"]:
        return "the text"
    for f, (st, want) in enumerate(zip(run["stats"], hc["wants"])):
        trace = want["trace"]
        if (st["n_list"], st["rounds"]["rounds_done"], st["rounds"]["pairs_aligned"], st["rounds"]["pairs_refused"]) != (len(want["lst"]), len(want["lst"]), trace["aligned"], 0):
            return "the statistics of file %d: %s" % (f, st)
    return None


def test_the_region_equals_the_host_chain():
    run = region_run()
    assert region_differs(run) is None
    assert len(run["stats"]) == 3 and all(st["events_passes"] == 1 and st["events"] > 0 for st in run["stats"])


def test_the_region_from_the_smallest_capacities():
    """an events buffer and an event array of one entry: the events pass is repeated once per file, the rounds are continued, and the
    bytes are those of the default capacities"""
    run = region_run(first_event_cap=1, second_event_cap=1)
    assert region_differs(run) is None and outputs(run) == outputs(region_run())
    assert all(st["events_passes"] == 2 for st in run["stats"]) and [st["events"] for st in run["stats"]] == [st["events"] for st in region_run()["stats"]]


def test_the_region_does_not_depend_on_the_threads():
    one, three = region_run(n_threads=1), region_run(n_threads=3)
    assert outputs(one) == outputs(three) == outputs(region_run()) and one["stats"] == three["stats"]
    assert outputs(region_run(n_threads=3, first_event_cap=1, second_event_cap=1)) == outputs(one)
    assert outputs(region_run(n_threads=8)) == outputs(one)  # (more threads than files)


def test_the_region_in_long_mode():
    """no read of the set has more than 256 bases: max_read_len 1000 gives the bytes of the default mode"""
    assert outputs(region_run(max_read_len=1000)) == outputs(region_run())


def test_the_region_argument_errors_and_empty_inputs():
    L = gtx.lib()
    reference, rb, files = vc.simulated_files()
    whole = region_run()
    # no files; bad parameters; no device
    with pytest.raises(gtx.GtxError) as e:
        gtx.discover_region(reference, rb, vc.CONTIG, [])
    assert e.value.status == ERR_ARG
    for bad in (dict(n_threads=0), dict(n_threads=9), dict(bucket_size=0), dict(max_read_len=1001)):
        with pytest.raises(gtx.GtxError) as e:
            gtx.discover_region(reference, rb, vc.CONTIG, region_files(), **bad)
        assert e.value.status == ERR_ARG, bad
    with pytest.raises(gtx.GtxError) as e:
        gtx.discover_region(reference, rb, vc.CONTIG, region_files(), device=-1)
    assert e.value.status == ERR_NO_DEVICE
    h = C.c_void_p(77)
    params = gtx.DiscoverParams()
    L.gtx_discover_params_default(C.byref(params))
    assert (params.device, params.bucket_size, params.max_read_len, params.n_threads, params.first_event_cap, params.second_event_cap) == (0, 50, 0, 1, 0, 0)
    one = gtx.DiscFile(None, None, None, None, 16, 1, 0, 0)
    assert L.gtx_discover_region(None, 10, 0, b"c", C.byref(one), 1, C.byref(params), C.byref(h)) == ERR_ARG and h.value is None
    assert L.gtx_discover_region(b"ACGTACGTAC", 10, 0, b"c", C.byref(one), 1, None, C.byref(h)) == ERR_ARG
    assert L.gtx_discover_region(b"ACGTACGTAC", 10, 0, b"c", C.byref(one), 1, C.byref(params), None) == ERR_ARG
    bad_read = np.zeros(1, gtx.DISC_READ)
    bad_read[0] = (0, 3, 60, 0, 4, 2, 0)  # two cigar words where the file has one
    rows, qual, cigar = np.zeros(16, np.uint8), np.zeros(4, np.uint8), np.array([4 << 4], np.uint32)
    wrong = gtx.DiscFile(rows.ctypes.data, qual.ctypes.data, bad_read.ctypes.data, cigar.ctypes.data, 16, 4, 1, 1)
    assert L.gtx_discover_region(b"ACGTACGTAC", 10, 0, b"c", C.byref(wrong), 1, C.byref(params), C.byref(h)) == ERR_ARG and b"cigar" in L.gtx_last_error()
    # a file without reads behind the others: the others' result
    empty = dict(planes=np.zeros((0, 16), np.uint8), plane_stride=16, qual=np.zeros((0, 1), np.uint8), qual_stride=1, reads=np.zeros(0, gtx.DISC_READ),
                 cigar=np.zeros(0, np.uint32))
    with_empty = gtx.discover_region(reference, rb, vc.CONTIG, region_files() + [empty], n_threads=2)
    assert outputs(with_empty) == outputs(whole) and with_empty["stats"][:3] == whole["stats"] and with_empty["stats"][3]["events"] == 0
    only_empty = gtx.discover_region(reference, rb, vc.CONTIG, [empty])
    assert only_empty["text"] == ref.COLUMNS.encode() and len(only_empty["variants"]) == 0 and len(only_empty["good"]) == 0
    # a region where nothing survives: reads of the reference itself
    reads = [dc.rd(rb + s, dc.cig(("M", 100)), reference[s:s + 100]) for s in range(0, 400, 7)]
    nothing = gtx.discover_region(reference, rb, vc.CONTIG, [file_arrays(reference, rb, reads)] * 2, n_threads=2)
    assert nothing["text"] == ref.COLUMNS.encode() and len(nothing["variants"]) == 0 and [st["events"] for st in nothing["stats"]] == [0, 0]
