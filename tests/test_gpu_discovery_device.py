"""Discovery's first pass on the device (include/gtx.h: gtx_disc_first_pass_device, gtx_disc_first_pass_haplotypes_device): the
events of gtx_disc_events_batch stay where they are, the device sorts them by event, walks every event's run in read order,
counts the phase pairs, filters, and hands the survivors' words over.  Every expected value is the oracle's
(oracle/gto_discovery.hpp through tests/test_discovery.py); the host entry points over the same device events have to agree."""
import ctypes as C
import functools

import numpy as np
import pytest

from graphtyper_amd import lib as gtx
from oracle_lib import _p
from test_discovery import CODE, _read, cig, oracle_first_pass, oracle_full, parse, parse_result, simulate

pytestmark = pytest.mark.gpu


class Pass:
    """the reads of one region on the device with the events gtx_disc_events_batch made of them"""

    def __init__(self, reference, region_begin, reads, event_cap=None):
        import torch
        self.torch, self.L = torch, gtx.lib()
        self.reads, n = reads, len(reads)
        self.stride = stride = max(16, (max(len(r["seq"]) for r in reads) + 31) // 32 * 16)
        codes = np.zeros((n, stride * 2), np.uint8)
        qual = np.zeros((n, stride * 2), np.uint8)
        dr = np.zeros(n, gtx.DISC_READ)
        cg = []
        lut = np.zeros(256, np.uint8)
        for c, v in CODE.items():
            lut[ord(c)] = v
        for i, r in enumerate(reads):
            codes[i, :len(r["seq"])] = lut[np.frombuffer(r["seq"].encode(), np.uint8)]
            qual[i, :len(r["seq"])] = r["qual"]
            dr[i] = (r["pos"], r["flag"], r["mapq"], 0, len(r["seq"]), len(r["cigar"]), len(cg))
            cg.extend(r["cigar"])
        self.dr, self.cg = dr, np.array(cg + [0], np.uint32)
        self.nib = gtx.pack_nibbles(codes, stride=stride)
        planes = gtx.pack_planes(self.nib, stride)
        self.h = C.c_void_p()
        gtx.check(self.L.gtx_disc_create(reference.encode(), len(reference), region_begin, 0, C.byref(self.h)))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
        self.d_planes, self.d_qual, self.d_reads, self.d_cigar = dev(planes), dev(qual), dev(dr), dev(self.cg)
        self.cap = event_cap or 64 * n
        self.d_events = torch.zeros(self.cap * gtx.DISC_EVENT.itemsize, dtype=torch.uint8, device="cuda:0")
        self.d_counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        self.d_out = torch.zeros(n * gtx.DISC_READ_OUT.itemsize, dtype=torch.uint8, device="cuda:0")
        gtx.check(self.L.gtx_disc_events_batch(self.h, self.d_planes.data_ptr(), stride, self.d_qual.data_ptr(), stride * 2, self.d_reads.data_ptr(),
                                               self.d_cigar.data_ptr(), n, self.d_events.data_ptr(), self.cap, self.d_counts.data_ptr(), self.d_out.data_ptr(), None))
        torch.cuda.synchronize()

    def call(self, file_index=None, bucket_size=50, stream=None, cap=1 << 20):
        """one call of the entry point -> (status, words, n_words)"""
        words, n = np.zeros(max(cap, 1), np.uint32), C.c_uint64()
        a = [self.h, self.d_planes.data_ptr(), self.stride, self.d_reads.data_ptr(), self.d_cigar.data_ptr(), self.d_out.data_ptr(), len(self.reads),
             self.d_events.data_ptr(), self.d_counts.data_ptr(), bucket_size]
        tail = [_p(words), cap, C.byref(n), stream]
        if file_index is None:
            rc = self.L.gtx_disc_first_pass_device(*a, *tail)
        else:
            rc = self.L.gtx_disc_first_pass_haplotypes_device(*a, file_index, *tail)
        return rc, words[:min(n.value, cap)], int(n.value)

    def device(self, file_index=None, bucket_size=50, stream=None):
        rc, words, n = self.call(file_index, bucket_size, stream)
        if rc == 5 and n > len(words):
            rc, words, n = self.call(file_index, bucket_size, stream, cap=n)
        assert rc == 0, self.L.gtx_last_error()
        return words

    def host(self, file_index=None, bucket_size=50):
        """the host entry points over the same device events, downloaded"""
        counts = self.d_counts.cpu().numpy()
        events = self.d_events.cpu().numpy().view(gtx.DISC_EVENT)[:min(int(counts[0]), self.cap)]
        read_out = self.d_out.cpu().numpy().view(gtx.DISC_READ_OUT)
        n, cap = C.c_uint64(), 1 << 16
        while True:
            words = np.zeros(cap, np.uint32)
            a = [self.h, _p(self.dr), _p(self.cg), _p(read_out), len(self.reads), _p(events), len(events), _p(self.nib), self.stride, bucket_size]
            if file_index is None:
                rc = self.L.gtx_disc_first_pass(*a, _p(words), cap, C.byref(n))
            else:
                rc = self.L.gtx_disc_first_pass_haplotypes(*a, file_index, _p(words), cap, C.byref(n))
            if rc == 5 and n.value > cap:
                cap = int(n.value)
                continue
            assert rc == 0, self.L.gtx_last_error()
            return words[:n.value]

    def close(self):
        self.L.gtx_disc_destroy(self.h)


def both(reference, region_begin, reads, bucket_size=50):
    """device words of the first entry point; they and the second's are held to the oracle and to the host entry points here"""
    p = Pass(reference, region_begin, reads)
    try:
        got, want = p.device(None, bucket_size), oracle_first_pass(reference, region_begin, reads, bucket_size)
        assert len(got) == len(want) and np.array_equal(got, want), "first differing word %s" % np.nonzero(got[:min(len(got), len(want))] != want[:min(len(got), len(want))])[0][:5]
        assert np.array_equal(p.host(None, bucket_size), want)
        full = p.device(3, bucket_size)
        assert np.array_equal(full, oracle_full(reference, region_begin, reads, bucket_size, file_i=3)[0])
        assert np.array_equal(p.host(3, bucket_size), full)
    finally:
        p.close()
    return got


@functools.lru_cache(maxsize=None)
def simulated(seed):
    ref, rb, reads = simulate(seed, n_reads=6000 if seed % 2 else 2500, read_len=150 if seed != 4 else 250)
    want_full, _, read_out = oracle_full(ref, rb, reads, file_i=3)
    return ref, rb, reads, oracle_first_pass(ref, rb, reads), want_full, read_out


SEEDS = [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("seed", SEEDS)
def test_simulated_alignments_equal_the_oracle_and_the_host_stage(seed):
    ref, rb, reads, want, want_full, _ = simulated(seed)
    p = Pass(ref, rb, reads)
    try:
        got = p.device()
        assert len(got) == len(want) and np.array_equal(got, want), "first differing word %s" % np.nonzero(got[:min(len(got), len(want))] != want[:min(len(got), len(want))])[0][:5]
        full = p.device(3)
        assert np.array_equal(full, want_full)
        assert np.array_equal(p.host(), got) and np.array_equal(p.host(3), full)
        assert len(parse(got)) > 20 and len(parse_result(full)[1]) > 20
    finally:
        p.close()


def test_the_simulated_reads_lie_on_both_sides_of_the_two_event_limits():
    """the corrections for reads with 12..17 and with 18 and more events are exercised by the seeds above: counted reads (those in front
    of the first GTX_DISC_END read) of each class exist, by the oracle's own walk"""
    classes = set()
    for seed in SEEDS:
        ro = simulated(seed)[5]
        end = np.nonzero(ro["state"] == 2)[0]
        counted = ro[:end[0] if len(end) else len(ro)]
        n = counted["n_events"][counted["state"] == 1]
        classes |= {"few"} if (n < 12).any() else set()
        classes |= {"many"} if ((n >= 12) & (n < 18)).any() else set()
        classes |= {"very many"} if (n >= 18).any() else set()
    assert classes == {"few", "many", "very many"}


# ---- cases made by hand ---------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(11)
REF = "".join("ACGT"[i] for i in RNG.integers(0, 4, 600))
RB = 3000


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def carrier(start, sites, length=100, low=(), flag=1 | 2 | 64, ref=REF, rb=RB):
    """a read of `length` matched bases from `start` that differs from the reference at `sites` (region offsets); base quality 10 at `low`"""
    seq = list(ref[start:start + length])
    for s in sites:
        seq[s - start] = other(ref[s])
    r = _read(rb + start, "".join(seq), cig(("M", length)), flag=flag)
    for s in low:
        r["qual"][s - start] = 10
    return r


def supporters(sites, first_start, n=12, step=3):
    """n clean reads over `sites` from different starts, both strands, both mates: enough for a SNP to pass the filter"""
    return [carrier(first_start + step * k, sites, flag=1 | 2 | (16 if k % 2 else 0) | (64 if k % 3 else 128)) for k in range(n)]


def find(events, pos, kind="X"):
    hit = [e for e in events if e[0] == pos and e[1] == kind]
    assert len(hit) == 1, (pos, kind, [e[:3] for e in events])
    return hit[0]


@pytest.mark.parametrize("n_events", [12, 18])
def test_the_correction_comes_at_its_reads_place_in_the_order(n_events):
    """one SNP on a low-quality base of a read with many events and on a high-quality base of a clean read: with the noisy read first
    its correction finds nothing to take from hq (12..17 events) / takes its own lq back (18); behind the clean read it takes that
    read's hq.  (Twelve clean reads more let the SNP through the filter, so that its counters show.)"""
    snp = 250
    extra = [205 + 4 * k for k in range(n_events - 1)]
    extra = [s if s != snp else s + 1 for s in extra]
    noisy = carrier(200, [snp] + extra, low=[snp])
    clean = carrier(210, [snp])
    rest = supporters([snp], 170)
    seen = []
    for order in ([noisy, clean], [clean, noisy]):
        got = parse(both(REF, RB, order + rest))
        sup = find(got, RB + snp)[3]
        seen.append((sup["hq"], sup["lq"]))
    assert seen == ([(13, 1), (12, 2)] if n_events == 12 else [(13, 0), (12, 1)])


@pytest.mark.parametrize("n_events", [11, 12, 17, 18])
def test_reads_at_the_event_count_boundaries(n_events):
    """a read with exactly 11 / 12 / 17 / 18 events among twelve clean carriers of its first two: 11 leaves the counters alone, 12 and 17
    move its hq to lq, 18 takes it away; up to 17 events it adds a phase entry from its first event to every later one, with 18 none"""
    a, b = 240, 246
    sites = [a, b] + [252 + 3 * k for k in range(n_events - 2)]
    noisy = carrier(230, sites)
    got = parse(both(REF, RB, [noisy] + supporters([a, b], 180)))
    ev = find(got, RB + a)
    assert (ev[3]["hq"], ev[3]["lq"]) == {11: (13, 0), 12: (12, 1), 17: (12, 1), 18: (12, 0)}[n_events]
    phase = {q[0] - RB: q[3] for q in ev[4]}
    if n_events < 18:
        assert phase == {s: (13 if s == b else 1) for s in sites[1:]}
    else:
        assert phase == {b: 12}


def test_the_three_start_positions_follow_the_stream():
    snp = 300
    p, q, r = 240, 250, 260
    mk = lambda start, k: carrier(start, [snp], flag=1 | 2 | (16 if k % 2 else 0) | (64 if k % 3 else 128))  # noqa: E731
    for starts, want in (([p, p, q, q, r], (p, q, r)), ([q, p, p, r], (q, p, r))):
        sup = find(parse(both(REF, RB, [mk(s, k) for k, s in enumerate(starts)])), RB + snp)[3]
        assert (sup["u1"], sup["u2"], sup["u3"]) == tuple(RB + x for x in want)


def indel_read(start, at, ins="", dele=0, length=100, k=0, ref=REF, rb=RB):
    """a read from `start` with `ins` inserted in front of region offset `at`, or `dele` bases deleted there"""
    tail = length - (at - start) - len(ins)
    seq = ref[start:at] + ins + ref[at + dele:at + dele + tail]
    ops = [("M", at - start)] + ([("I", len(ins))] if ins else [("D", dele)]) + [("M", tail)]
    return _read(rb + start, seq, cig(*ops), flag=1 | 2 | (16 if k % 2 else 0) | (64 if k % 3 else 128))


def test_insertions_are_told_apart_at_every_length():
    """at one position: two 40-base insertions that differ in their last base (the key holds 13), "AC" beside "ACG" (a string sorts in
    front of its extensions), a deletion, a SNP -- all in one result, in the reference's order (insertions, deletions, SNPs)"""
    at = 300
    long_a, long_t = "ACGT" * 9 + "ACGA", "ACGT" * 10
    reads = []
    for j, ins in enumerate(["ACG", long_t, "AC", long_a]):
        reads += [indel_read(250 + 2 * k + j, at, ins=ins, length=120, k=k) for k in range(6)]
    reads += [indel_read(240 + 3 * k, at, dele=3, k=k) for k in range(6)]
    reads += supporters([at], 230, n=14)
    RNG2 = np.random.default_rng(5)
    reads = [reads[i] for i in RNG2.permutation(len(reads))]  # an unsorted stream: the events of one insertion are not neighbours
    got = parse(both(REF, RB, reads))
    here = [(t, s) for pos, t, s, _, _ in got if pos == RB + at]
    assert here == [("I", "AC"), ("I", "ACG"), ("I", long_a), ("I", long_t), ("D", REF[at:at + 3]), ("X", other(REF[at]))]
    assert all(e[3]["hq"] == 6 for e in got if e[0] == RB + at and e[1] != "X")


def test_the_span_of_indels_in_repeats():
    """bucket.cpp:100-160: an A in front of AAAAAA, an A deleted from it, a unit put into and taken out of a tandem repeat"""
    ref = "CGTACGTTGCA" + "AAAAAA" + "CGTGCATGCATTGCAGTCA" * 3 + "CACACACACACA" + "GTTGCAGTCATGCATCGTGCA" * 6
    homo, tandem = 11, 11 + 6 + 57
    for make in (lambda s, k: indel_read(s, homo, ins="A", length=80, k=k, ref=ref, rb=0), lambda s, k: indel_read(s, homo, dele=1, length=80, k=k, ref=ref, rb=0),
                 lambda s, k: indel_read(40 + s, tandem, ins="CA", length=80, k=k, ref=ref, rb=0),
                 lambda s, k: indel_read(40 + s, tandem, dele=2, length=80, k=k, ref=ref, rb=0)):
        got = [e for e in parse(both(ref, 0, [make(k, k) for k in range(10)])) if e[1] != "X"]
        assert len(got) == 1 and got[0][3]["span"] > 5 and got[0][3]["hq"] == 10 and got[0][3]["realign"] == 1


def test_the_pass_ends_at_the_first_read_behind_the_region():
    """a GTX_DISC_END read in the middle of an unsorted stream: the reads behind it add nothing (the same words as without them); an event
    in the region's last bucket stays, nothing lies behind it; BUCKET_SIZE decides nothing"""
    front = supporters([250], 180) + supporters([590], 500)
    end = _read(RB + len(REF), "ACGT" * 20, cig(("M", 80)))
    behind = supporters([400], 330) + supporters([250], 181)
    reads = front + [end] + behind
    got = both(REF, RB, reads)
    assert np.array_equal(got, oracle_first_pass(REF, RB, front)) and {e[0] - RB for e in parse(got)} == {250, 590}
    assert np.array_equal(both(REF, RB, reads, bucket_size=777), got)
    ref, rb, sim_reads, want = simulated(2)[:4]
    p = Pass(ref, rb, sim_reads)
    try:
        assert np.array_equal(p.device(bucket_size=777), want) and np.array_equal(p.device(bucket_size=50), want)
    finally:
        p.close()


def test_an_event_behind_the_last_bucket_is_dropped():
    """gtx_disc_events_batch ends a read's walk at the region's end, so an event behind the region's last bucket is made by hand: the
    event of one of twelve carriers of a SNP is moved 60 positions behind the region.  The reference cuts such a bucket off before
    its filters: the words are the oracle's over the same reads with that carrier clean (11 carriers, the coverage of 12).  Then
    with a read of two events whose second is moved: the first keeps its phase entry to the event that left, as the phase maps of
    the reference do -- the oracle's words over the read without its second event, and that one entry more."""
    import torch
    beyond = RB + len(REF) + 60

    def moved(reads, read, k):
        p = Pass(REF, RB, reads)
        try:
            ro = p.d_out.cpu().numpy().view(gtx.DISC_READ_OUT)
            ev = p.d_events.cpu().numpy().view(gtx.DISC_EVENT).copy()
            at = int(ro["first_event"][read]) + k
            assert ev["read"][at] == read and ev["type"][at] == ord("X")
            base = chr(int(ev["seq"][at]))
            ev["pos"][at] = beyond
            p.d_events.copy_(torch.from_numpy(ev.view(np.uint8).reshape(-1)))
            torch.cuda.synchronize()
            return [p.device(bucket_size=b) for b in (50, 777)] + [p.device(3)], base
        finally:
            p.close()

    reads = supporters([250], 180)
    clean = list(reads)
    clean[5] = carrier(180 + 3 * 5, [], flag=reads[5]["flag"])
    (got, got777, full), _ = moved(reads, 5, 0)
    want = oracle_first_pass(REF, RB, clean)
    assert np.array_equal(got, want) and np.array_equal(got777, want) and find(parse(got), RB + 250)[3]["hq"] == 11
    assert np.array_equal(full, oracle_full(REF, RB, clean, file_i=3)[0])
    # a phase target that left
    two = [carrier(200, [250, 270])] + supporters([250], 180)
    one = [carrier(200, [250])] + two[1:]
    (got, _, _), base = moved(two, 0, 1)
    want = parse(oracle_first_pass(REF, RB, one))
    snp = find(want, RB + 250)
    assert snp[4] == [] and base == other(REF[270])
    snp[4].append((beyond, "X", base, 1))
    assert parse(got) == want


def test_a_read_whose_events_lie_behind_the_event_count_is_refused():
    """d_counts[1] == 0, yet a counted read's first_event + n_events > d_counts[0] (read states that do not belong to these counts,
    made by hand here: gtx_disc_events_batch cannot leave them): GTX_ERR_CAPACITY, as the host stage answers, and nothing is read
    behind the events."""
    import torch
    reads = supporters([250], 180)
    p = Pass(REF, RB, reads)
    try:
        assert p.call()[0] == 0
        n_events = int(p.d_counts.cpu()[0])
        ro = p.d_out.cpu().numpy().view(gtx.DISC_READ_OUT).copy()
        assert ro["n_events"][5] == 1
        ro["first_event"][5] = n_events  # one behind the last
        p.d_out.copy_(torch.from_numpy(ro.view(np.uint8).reshape(-1)))
        torch.cuda.synchronize()
        assert p.call()[0] == 5 and p.call(3)[0] == 5  # GTX_ERR_CAPACITY
        assert b"behind the event buffer" in p.L.gtx_last_error()
    finally:
        p.close()


def test_a_counter_of_sixteen_bits_wraps():
    """65 540 copies of one 40-base read with one SNP, and eight reads more from other places: hq_count, proper_pairs, first_in_pairs wrap
    to 12.  The SNP is at the region's last base, where every read over it ends: the coverage there counts as zero (cov_down takes
    the reads away where they end), so the wrapped counts still pass the filter and show in the words."""
    ref = REF[:400]
    snp = 399
    copies = [carrier(360, [snp], length=40, ref=ref)] * 65540
    more = [carrier(352 + k, [snp], length=48 - k, flag=1 | 2 | 64 | (16 if k % 2 else 0), ref=ref) for k in range(8)]
    got = parse(both(ref, RB, copies + more))
    sup = find(got, RB + snp)[3]
    assert (sup["hq"], sup["proper"], sup["first"], sup["reversed"]) == (12, 12, 12, 4)


def test_an_overflowed_event_buffer_is_reported():
    ref, rb, reads = simulated(1)[:3]
    p = Pass(ref, rb, reads, event_cap=100)
    try:
        assert int(p.d_counts.cpu()[1]) > 0
        assert p.call()[0] == 5 and p.call(3)[0] == 5  # GTX_ERR_CAPACITY
    finally:
        p.close()


def test_the_same_call_gives_the_same_words():
    import torch
    ref, rb, reads, want, want_full, _ = simulated(3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    seen = []
    for stream in (s1, s2):
        p = Pass(ref, rb, reads)  # fresh buffers
        try:
            seen.append((p.device(stream=stream.cuda_stream), p.device(3, stream=stream.cuda_stream), p.device(3, stream=stream.cuda_stream)))
            rc, words, n = p.call(cap=0)
            assert rc == 5 and n == len(want) and len(words) == 0
            rc, words, n = p.call(3, cap=0)
            assert rc == 5 and n == len(want_full)
            assert np.array_equal(gtx.disc_first_pass_device(p.h, p.d_planes.data_ptr(), p.stride, p.d_reads.data_ptr(), p.d_cigar.data_ptr(), p.d_out.data_ptr(),
                                                             len(reads), p.d_events.data_ptr(), p.d_counts.data_ptr(), cap=16), want)
        finally:
            p.close()
    for a, b, c in seen:
        assert np.array_equal(a, want) and np.array_equal(b, want_full) and np.array_equal(c, want_full)
