"""gtx_disc_events_kernel on the device (include/gtx.h: gtx_disc_events_batch), event by event: every case set of
tests/disc_event_cases.py equals the plain restatement of the reference's walk (tests/disc_events_ref.py) per read -- state,
n_events, pos_end, the events [first_event, first_event + n_events) in order, every field -- and the same device arrays, taken on
through gtx_disc_first_pass_device and gtx_disc_first_pass, give the oracle's words.  Then what a launch has to leave whatever
its size: the tiling of the event buffer, its capacity, counters that are not zero at entry, a stream of the caller's.  All values
are integers; there is no tolerance.  The same checks run over the kernel's text on the host in test_disc_events_emu.py."""
import ctypes as C

import numpy as np
import pytest

import disc_event_cases as dc
from graphtyper_amd import lib as gtx
from oracle_lib import _p

pytestmark = pytest.mark.gpu

CANARY = 64  # entries behind event_cap that nobody may touch


class Launch:
    """a part's arrays on the device; run() is one gtx_disc_events_batch over buffers of its own (or over the previous call's)"""

    def __init__(self, part, a=None):
        import torch
        self.torch, self.L, self.part = torch, gtx.lib(), part
        self.a = a = a or dc.arrays(part)
        self.n = len(a["reads"])
        self.h = C.c_void_p()
        refb = part.reference.encode("latin-1")
        gtx.check(self.L.gtx_disc_create(refb, len(refb), part.region_begin, 0, C.byref(self.h)))
        self.dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda:0")
        self.d_planes, self.d_qual, self.d_reads, self.d_cigar = (self.dev(a[k]) for k in ("planes", "qual", "reads", "cigar"))

    def run(self, event_cap, counts=(0, 0), stream=None, again=False, null_events=False):
        """-> (counts, read_out, the event buffer with CANARY entries behind event_cap)"""
        torch = self.torch
        if not again:
            self.d_events = torch.full(((event_cap + CANARY) * gtx.DISC_EVENT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
            self.d_counts = self.dev(np.array(counts, np.uint32))
            self.d_out = torch.full((max(self.n, 1) * gtx.DISC_READ_OUT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gtx.check(self.L.gtx_disc_events_batch(self.h, self.d_planes.data_ptr(), self.part.stride, self.d_qual.data_ptr(), self.a["qual"].shape[1],
                                               self.d_reads.data_ptr(), self.d_cigar.data_ptr(), self.n, None if null_events else self.d_events.data_ptr(), event_cap,
                                               self.d_counts.data_ptr(), self.d_out.data_ptr(), stream))
        torch.cuda.synchronize()
        self.cap = event_cap
        events = self.d_events.cpu().numpy().view(gtx.DISC_EVENT)
        assert (events[event_cap:].view(np.uint8) == 0xA5).all(), "an entry behind event_cap was written"
        return self.d_counts.cpu().numpy().view(np.uint32), self.d_out.cpu().numpy().view(gtx.DISC_READ_OUT)[:self.n], events

    def device_words(self):
        return gtx.disc_first_pass_device(self.h, self.d_planes.data_ptr(), self.part.stride, self.d_reads.data_ptr(), self.d_cigar.data_ptr(), self.d_out.data_ptr(),
                                          self.n, self.d_events.data_ptr(), self.d_counts.data_ptr())

    def host_words(self, counts, read_out, events):
        nib = gtx.pack_nibbles(self.a["codes"], stride=self.part.stride)
        events = np.ascontiguousarray(events[:int(counts[0])])
        n, cap = C.c_uint64(), 1 << 16
        while True:
            words = np.zeros(cap, np.uint32)
            rc = self.L.gtx_disc_first_pass(self.h, _p(self.a["reads"]), _p(self.a["cigar"]), _p(np.ascontiguousarray(read_out)), self.n, _p(events), len(events),
                                            _p(nib), self.part.stride, 50, _p(words), cap, C.byref(n))
            if rc == 5 and n.value > cap:
                cap = int(n.value)
                continue
            assert rc == 0, self.L.gtx_last_error()
            return words[:n.value]

    def close(self):
        self.torch.cuda.synchronize()
        self.L.gtx_disc_destroy(self.h)


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_every_event_equals_the_restatement_and_the_words_the_oracle(name):
    for k, (part, want) in enumerate(zip(dc.parts(name), dc.expected(name))):
        total = dc.total_events(want)
        run = Launch(part)
        try:
            counts, read_out, events = run.run(total)
            got = dc.per_read(read_out, events, limit=total)
            wrong = [(k, i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
            assert wrong == [], wrong[:3]
            assert dc.check_launch(want, counts, read_out, events, total) == 0 and tuple(counts) == (total, 0)
            words = dc.oracle_words(part)
            assert np.array_equal(run.device_words(), words), (name, k)
            assert np.array_equal(run.host_words(counts, read_out, events), words), (name, k)
        finally:
            run.close()


@pytest.fixture(scope="module")
def tiled():
    """event_counts repeated to 257 reads, on the device once for the tests that share it"""
    run = Launch(dc.tiling_part(257))
    yield run, dc.tiling_expected(257)
    run.close()


@pytest.mark.parametrize("n_reads", dc.TILING_READS + (40003,))
def test_the_pieces_tile_the_event_buffer(n_reads):
    part, want = dc.tiling_part(n_reads), dc.tiling_expected(n_reads)
    total = dc.total_events(want)
    run = Launch(part)
    try:
        counts, read_out, events = run.run(total)
        assert dc.check_launch(want, counts, read_out, events, total) == 0 and (n_reads < 2 or total > 0)
    finally:
        run.close()


@pytest.mark.parametrize("cap", ["total", "total - 1", "1", "0"])
def test_a_read_fits_or_is_counted_as_overflow(tiled, cap):
    """event_cap of all events, one fewer, 1, and 0 with a null event buffer: counts[1] is the sum of n_events over the reads that did not
    fit, every read that fits holds its right events, nothing behind entry event_cap is touched, read_out is written for all reads"""
    run, want = tiled
    total = dc.total_events(want)
    event_cap = eval(cap, dict(total=total))
    counts, read_out, events = run.run(event_cap, null_events=cap == "0")
    lost = dc.check_launch(want, counts, read_out, events, event_cap)
    assert (lost == 0) == (cap == "total") and (cap != "0" or int(counts[1]) == total)
    if cap == "0":
        assert (events.view(np.uint8) == 0xA5).all()


def test_counters_that_are_not_zero_at_entry(tiled):
    run, want = tiled
    total = dc.total_events(want)
    counts, read_out, events = run.run(7 + total, counts=(7, 3))
    assert dc.check_launch(want, counts, read_out, events, 7 + total, (7, 3)) == 0 and tuple(counts) == (7 + total, 3)
    assert (events[:7].view(np.uint8) == 0xA5).all()  # nobody's
    # two calls in a row on one event buffer accumulate: the second one's pieces lie behind the first one's
    counts, read_out, first = run.run(2 * total)
    first = first[:total].copy()
    assert dc.check_launch(want, counts, read_out, first, 2 * total) == 0
    counts, read_out, events = run.run(2 * total, again=True)
    assert dc.check_launch(want, counts, read_out, events, 2 * total, (total, 0)) == 0 and tuple(counts) == (2 * total, 0)
    assert np.array_equal(events[:total], first)  # (the first call's events are where they were)


def test_a_stream_of_the_callers(tiled):
    """the same call twice on fresh buffers, on a stream that is not the null stream: the same content per read (the order of the
    wavefronts' pieces may differ)"""
    run, want = tiled
    total = dc.total_events(want)
    stream = run.torch.cuda.Stream()
    seen = []
    for _ in range(2):
        counts, read_out, events = run.run(total, stream=stream.cuda_stream)
        assert dc.check_launch(want, counts, read_out, events, total) == 0
        seen.append(dc.per_read(read_out, events))
    assert [(r[0], r[1], r[2], r[3]) for r in seen[0]] == [(r[0], r[1], r[2], r[3]) for r in seen[1]]
