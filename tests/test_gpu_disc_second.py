"""The second pass up to the aligner on the device (include/gtx.h: gtx_disc_indel_table_upload, gtx_disc_second_intake,
gtx_disc_second_candidates): every case set and launch shape of tests/disc_second_cases.py equals the plain restatement of the
reference's text (tests/disc_second_ref.py) -- per read its state, the two bucket arrays, max_read_size, the grouping by bucket,
the found-bits, the pairs in the reference's order of visit and the two counters -- with guard bytes behind every output array;
then a stream of the caller's, the argument errors, and the whole chain behind a real first pass over two files, whose pairs go
into gtx_disc_realign_batch.  All values are integers; there is no tolerance.  The same checks run over the kernels' text on the
host in test_disc_second_emu.py."""
import ctypes as C

import numpy as np
import pytest

import disc_event_cases as dc
import disc_second_cases as sc
from graphtyper_amd import lib as gtx
from oracle_lib import _p

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes behind every output array that nobody may touch


class Run:
    """a case's arrays on the device; intake() and candidates() are one call each over buffers of their own (or over the previous
    call's), and return what the emulation's program writes"""

    def __init__(self, case, device=0):
        import torch
        self.torch, self.L, self.case = torch, gtx.lib(), case
        self.a = a = sc.arrays(case)
        self.n, self.nb, self.nt = len(a["reads"]), case.n_buckets, len(a["table"])
        self.h = C.c_void_p()
        refb = case.reference.encode("latin-1")
        gtx.check(self.L.gtx_disc_create(refb, len(refb), case.region_begin, device, C.byref(self.h)))
        self.d_planes, self.d_reads, self.d_cigar, self.d_lst, self.d_events, self.d_state = (self.dev(a[k]) for k in ("planes", "reads", "cigar", "lst", "events", "state"))
        self.d_table, self.d_letters = self.out(self.nt * gtx.DISC_INDEL.itemsize), self.out(len(a["letters"]))
        if device >= 0:
            gtx.check(self.L.gtx_disc_indel_table_upload(self.h, _p(a["table"]) if self.nt else None, self.nt, _p(a["letters"]) if len(a["letters"]) else None,
                                                         len(a["letters"]), self.d_table.data_ptr(), self.d_letters.data_ptr(), None))
            assert np.array_equal(self.down(self.d_table, gtx.DISC_INDEL, self.nt), a["table"]) and np.array_equal(self.down(self.d_letters, np.uint8, len(a["letters"])), a["letters"])
        self.got = {}

    def dev(self, x):
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        return self.torch.from_numpy(np.concatenate([x, np.zeros(16, np.uint8)])).to("cuda:0")

    def out(self, nbytes):
        return self.torch.full((nbytes + GUARD,), 0xA5, dtype=self.torch.uint8, device="cuda:0")

    def down(self, t, dtype, count):
        raw = t.cpu().numpy()
        size = count * np.dtype(dtype).itemsize
        assert len(raw) == size + GUARD and (raw[size:] == 0xA5).all(), "bytes behind an output array were written"
        return raw[:size].view(dtype).copy()

    def intake_args(self, stream=None):
        o = self.o
        return [self.h, self.d_planes.data_ptr(), self.case.part.stride, self.d_reads.data_ptr(), self.d_cigar.data_ptr(), self.n, self.case.bucket_size,
                self.d_table.data_ptr(), self.d_letters.data_ptr(), self.nt, len(self.a["letters"]), o["second"].data_ptr(), o["bucket_max"].data_ptr(),
                o["global_max"].data_ptr(), o["max_read_size"].data_ptr(), o["bucket_reads"].data_ptr(), o["bucket_off"].data_ptr(), o["found"].data_ptr(), stream]

    def intake(self, stream=None, again=False):
        if not again:
            self.o = dict(second=self.out(self.n * gtx.DISC_SECOND_READ.itemsize), bucket_max=self.out(4 * self.nb), global_max=self.out(4 * self.nb),
                          max_read_size=self.out(4), bucket_reads=self.out(4 * self.n), bucket_off=self.out(4 * (self.nb + 1)), found=self.out(4 * ((self.nt + 31) // 32)))
        self.torch.cuda.synchronize()
        gtx.check(self.L.gtx_disc_second_intake(*self.intake_args(stream)))
        self.torch.cuda.synchronize()
        for key, dtype, count in (("second", gtx.DISC_SECOND_READ, self.n), ("bucket_max", np.int32, self.nb), ("global_max", np.int32, self.nb),
                                  ("max_read_size", np.uint32, 1), ("bucket_reads", np.uint32, self.n), ("bucket_off", np.uint32, self.nb + 1),
                                  ("found", np.uint32, (self.nt + 31) // 32)):
            self.got[key] = self.down(self.o[key], dtype, count)
        return self.got

    def candidates_args(self, k0, k1, pair_cap, stream=None, null_pairs=False):
        o = self.o
        state = self.d_state if self.a["given"] else o["second"]
        return [self.h, self.d_lst.data_ptr(), k0, k1, self.d_table.data_ptr(), self.nt, state.data_ptr(), self.n, self.d_events.data_ptr(), len(self.a["events"]),
                self.case.bucket_size, o["bucket_max"].data_ptr(), o["global_max"].data_ptr(), o["max_read_size"].data_ptr(), o["bucket_reads"].data_ptr(),
                o["bucket_off"].data_ptr(), None if null_pairs else self.d_pairs.data_ptr(), pair_cap, self.d_counts.data_ptr(), stream]

    def candidates(self, k0, k1, pair_cap, counts=(0, 0), stream=None, again=False, null_pairs=False):
        if not again:
            self.d_pairs, self.d_counts = self.out(pair_cap * gtx.DISC_SECOND_PAIR.itemsize), self.out(8)
            self.d_counts[:8] = self.torch.from_numpy(np.array(counts, np.uint32).view(np.uint8)).to("cuda:0")
        self.torch.cuda.synchronize()
        gtx.check(self.L.gtx_disc_second_candidates(*self.candidates_args(k0, k1, pair_cap, stream, null_pairs)))
        self.torch.cuda.synchronize()
        self.got["pairs"], self.got["counts"] = self.down(self.d_pairs, gtx.DISC_SECOND_PAIR, pair_cap), self.down(self.d_counts, np.uint32, 2)
        return self.got

    def whole(self, stream=None):
        """the intake and the rounds of the whole list, with room for all pairs -> None, or how the case differs from the restatement"""
        want = sc.expected(self.case)
        self.intake(stream)
        got = self.candidates(0, len(want["lst"]), len(want["pairs"]), stream=stream)
        return sc.differs(self.case, got)

    def close(self):
        self.torch.cuda.synchronize()
        self.L.gtx_disc_destroy(self.h)


@pytest.mark.parametrize("name", sorted(sc.SETS))
def test_every_set_equals_the_restatement(name):
    for k, case in enumerate(sc.cases(name)):
        run = Run(case)
        try:
            assert run.whole() is None, (name, k)
        finally:
            run.close()


@pytest.mark.parametrize("name", sorted(sc.LAUNCHES))
def test_every_launch_shape_equals_the_restatement(name):
    """1 .. 257 reads, 1 and 2 buckets (70: the set long_deletion), slices of 0, 1, 64 and 65 list entries, pair_cap of all pairs, one
    fewer, 1 and 0 with a null buffer, counters that are not zero at entry, two calls over the same buffers"""
    case, k0, k1, cap, before, launches = sc.launch(name)
    run = Run(case)
    try:
        for launch in range(launches):
            run.intake(again=launch > 0)
            got = run.candidates(k0, k1, cap, before, again=launch > 0, null_pairs=cap == 0)
        assert sc.differs(case, got, k0, k1, cap, before, launches) is None
    finally:
        run.close()


def test_a_stream_of_the_callers():
    """the same calls twice on fresh buffers, on a stream that is not the null stream: the same arrays both times, pair for pair"""
    case = sc.shape_case(257)
    run = Run(case)
    try:
        stream = run.torch.cuda.Stream()
        seen = []
        for _ in range(2):
            assert run.whole(stream.cuda_stream) is None
            seen.append({k: v.copy() for k, v in run.got.items()})
        assert all(np.array_equal(seen[0][k], seen[1][k]) for k in seen[0])
    finally:
        run.close()


def test_the_argument_errors():
    case = sc.cases("plan_rules")[0]
    run, host = Run(case), Run(case, device=-1)
    try:
        L, want = run.L, sc.expected(case)
        run.intake()
        run.candidates(0, len(want["lst"]), len(want["pairs"]))
        host.o, host.d_pairs, host.d_counts = run.o, run.d_pairs, run.d_counts
        a = run.a
        # an object made without a device
        assert L.gtx_disc_second_intake(*host.intake_args()) == 2 and L.gtx_disc_second_candidates(*host.candidates_args(0, 1, 4)) == 2
        assert L.gtx_disc_indel_table_upload(host.h, _p(a["table"]), run.nt, _p(a["letters"]), len(a["letters"]), run.d_table.data_ptr(), run.d_letters.data_ptr(), None) == 2
        # null and misaligned arrays, no bucket size, a slice the wrong way round
        for at in (1, 3, 4, 7, 11, 12, 13, 14, 15, 16, 17):
            for bad in (None, run.d_planes.data_ptr() + 2):
                args = run.intake_args()
                args[at] = bad
                assert L.gtx_disc_second_intake(*args) == 1, at
        for at in (1, 4, 6, 11, 12, 13, 14, 15, 16, 18):
            for bad in (None, run.d_planes.data_ptr() + 2):
                args = run.candidates_args(0, len(want["lst"]), len(want["pairs"]))
                args[at] = bad
                assert L.gtx_disc_second_candidates(*args) == 1, at
        args = run.intake_args()
        args[6] = 0
        assert L.gtx_disc_second_intake(*args) == 1
        args[6], args[2] = case.bucket_size, 24
        assert L.gtx_disc_second_intake(*args) == 1
        assert L.gtx_disc_second_candidates(*run.candidates_args(2, 1, 4)) == 1
        assert L.gtx_disc_second_intake(None, *run.intake_args()[1:]) == 1 and L.gtx_disc_second_candidates(None, *run.candidates_args(0, 1, 4)[1:]) == 1
        run.torch.cuda.synchronize()
        # no reads, an empty slice: legal, and nothing is written
        run.o = {k: run.out(16) for k in run.o}
        run.d_pairs, run.d_counts = run.out(16), run.out(8)
        args = run.intake_args()
        args[5] = 0
        assert L.gtx_disc_second_intake(*args) == 0 and L.gtx_disc_second_candidates(*run.candidates_args(3, 3, 2)) == 0
        args[1] = args[3] = args[4] = None
        assert L.gtx_disc_second_intake(*args) == 0
        run.torch.cuda.synchronize()
        assert all((t.cpu().numpy() == 0xA5).all() for t in list(run.o.values()) + [run.d_pairs, run.d_counts])
    finally:
        run.close()
        host.close()
    # an empty table: the intake and the plan are legal, the list is empty
    bare = sc.Case(case.reference, case.region_begin, case.reads)
    run = Run(bare)
    try:
        assert run.whole() is None and len(gtx.disc_second_plan(run.a["table"], run.got["found"], 0)) == 0
    finally:
        run.close()


def first_pass_words(torch, L, part, file_index):
    """a file's reads through gtx_disc_events_batch and gtx_disc_first_pass_haplotypes_device -> its result words"""
    a = dc.arrays(part)
    n = len(a["reads"])
    h = C.c_void_p()
    refb = part.reference.encode("latin-1")
    gtx.check(L.gtx_disc_create(refb, len(refb), part.region_begin, 0, C.byref(h)))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    d_planes, d_qual, d_reads, d_cigar = (dev(a[k]) for k in ("planes", "qual", "reads", "cigar"))
    cap = 32 * n
    d_events = torch.zeros(cap * gtx.DISC_EVENT.itemsize, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(n * gtx.DISC_READ_OUT.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    try:
        gtx.check(L.gtx_disc_events_batch(h, d_planes.data_ptr(), part.stride, d_qual.data_ptr(), a["qual"].shape[1], d_reads.data_ptr(), d_cigar.data_ptr(), n,
                                          d_events.data_ptr(), cap, d_counts.data_ptr(), d_out.data_ptr(), None))
        return gtx.disc_first_pass_device(h, d_planes.data_ptr(), part.stride, d_reads.data_ptr(), d_cigar.data_ptr(), d_out.data_ptr(), n, d_events.data_ptr(),
                                          d_counts.data_ptr(), 50, file_index=file_index)
    finally:
        torch.cuda.synchronize()
        L.gtx_disc_destroy(h)


def test_the_chain_behind_a_real_first_pass_ends_in_the_aligner():
    """two files of one region: gtx_disc_events_batch -> gtx_disc_first_pass_haplotypes_device -> gtx_disc_merge -> the table -> per file
    the intake, the plan and the rounds' pairs, all as the restatement has them; the pairs then go into gtx_disc_realign_batch with
    the plain windows of gtx_disc_realign_target, and every pair comes back GTX_REALIGN_OK"""
    import torch
    L = gtx.lib()
    files = [sc.simulated_file(seed) for seed in (7, 8)]
    reference, rb = files[0][0], files[0][1]
    merged = np.zeros(0, np.uint32)
    for f, (_, _, reads, _) in enumerate(files):
        words = first_pass_words(torch, L, dc.Part(reference, rb, reads), f)
        out, n = np.zeros(len(merged) + len(words) + 16, np.uint32), C.c_uint64()
        gtx.check(L.gtx_disc_merge(_p(merged) if len(merged) else None, len(merged), _p(words), len(words), _p(out), len(out), C.byref(n)))
        merged = out[:n.value].copy()
    entries, letters = gtx.disc_indel_table(merged)
    table = [sc.ent(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), int(e["span"]), bool(e["good"]), int(e["file_index"]))
             for e in entries]
    assert len(table) >= 8 and {e["file_index"] for e in table if not e["good"]} == {0, 1} and table == sorted(table, key=sc.ref.table_order)
    aligned = 0
    for f, (_, _, reads, _) in enumerate(files):
        case = sc.Case(reference, rb, reads, table, file_index=f)
        run = Run(case)
        try:
            run.intake()
            lst = gtx.disc_second_plan(entries, run.got["found"], f)
            want = sc.expected(case)
            assert list(lst) == want["lst"] and len(lst) > 0
            got = run.candidates(0, len(lst), len(want["pairs"]))
            assert sc.differs(case, got) is None
            pairs = got["pairs"]
            assert len(pairs) > 0
            windows = [gtx.disc_realign_target(run.h, int(got["max_read_size"][0]), [(table[t]["pos"], table[t]["type"], table[t]["seq"])])[0] for t in lst]
            target_seq = np.frombuffer(b"".join(windows), np.uint8)
            target_off = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.uint32)
            res = gtx.disc_realign_batch(run.h, run.a["planes"], case.part.stride, run.a["reads"]["l_qseq"].astype(np.uint16), run.n, target_seq, target_off,
                                         len(windows), pairs.view(gtx.REALIGN_PAIR), len(pairs))
            assert (res["status"] == gtx.REALIGN_OK).all()
            aligned += len(pairs)
        finally:
            run.close()
    assert aligned > 100
