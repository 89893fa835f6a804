"""Packed 2-bit rows with an exception list on the device: gtx_packed_to_planes against the host's plane rows, and
gtx_align_batch_packed[_staged] against gtx_align_batch_planes over the same reads -- records and side bytes byte for byte, in
default and long-read contexts, in chunks, and through a paired stream to scores and calls.  The host side: test_packed_reads.py."""
import ctypes as C

import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from test_packed_reads import masked_codes
from test_reads_over_256 import long_case

pytestmark = pytest.mark.gpu
RW = harness.REC_WORDS


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


def with_ambiguity(codes, seed, rate=0.003):
    """a few IUPAC sets and '=' besides the scenario's N"""
    rng = np.random.default_rng(seed)
    codes = codes.copy()
    amb = rng.random(codes.shape) < rate
    codes[amb] = rng.integers(0, 16, size=int(amb.sum())).astype(np.uint8)
    return codes


class Packed:
    """one batch on the device as plane rows (the yardstick) and as packed rows + list"""

    def __init__(self, b, meta, planes, rows, start, exc):
        import torch
        self.torch, self.b, self.n = torch, b, len(meta)
        self.packed_stride, self.plane_stride = rows.shape[1], planes.shape[1]
        self.rows, self.start, self.exc = rows, start, exc
        self.d_planes, self.d_rows, self.d_start, self.d_meta = b._dev(planes), b._dev(rows), b._dev(start), b._dev(meta)
        self.d_exc = b._dev(exc if len(exc) else np.zeros(1, np.uint16))

    @classmethod
    def of_nibbles(cls, b, seq, meta, packed_stride):
        return cls(b, meta, gtx.pack_planes(seq, 2 * packed_stride), *gtx.pack_2bit(seq, meta["l_qseq"], packed_stride))

    def buffers(self, n=None):
        n = self.n if n is None else n
        t = self.torch
        return t.zeros(max(n, 1) * 2 * RW, dtype=t.int32, device="cuda:0"), t.full((max(2 * n, 1),), 0x55, dtype=t.uint8, device="cuda:0")

    def planes(self):
        d_rec, d_fl = self.buffers()
        gtx.check(gtx.lib().gtx_align_batch_planes(self.b.ctx.h, self.d_planes.data_ptr(), self.plane_stride, self.d_meta.data_ptr(), self.n,
                                                   d_rec.data_ptr(), RW, d_fl.data_ptr(), None))
        return self.result(d_rec, d_fl)

    def packed(self):
        d_rec, d_fl = self.buffers()
        gtx.check(gtx.lib().gtx_align_batch_packed(self.b.ctx.h, self.d_rows.data_ptr(), self.packed_stride, self.d_start.data_ptr(),
                                                   self.d_exc.data_ptr(), len(self.exc), self.d_meta.data_ptr(), self.n, d_rec.data_ptr(), RW,
                                                   d_fl.data_ptr(), None))
        return self.result(d_rec, d_fl)

    def result(self, d_rec, d_fl):
        self.torch.cuda.synchronize()
        return d_rec.cpu().numpy().view(np.uint32)[:self.n * 2 * RW], d_fl.cpu().numpy()[:2 * self.n]


def same_records(b, seq, meta, packed_stride):
    """records and side bytes of the packed call = the plane call's.  Both start from an empty big-record arena; a record that
    lives there (GTX_ST_EXTERNAL: long reads with many paths) holds an arena offset, which the calls' workgroups claim in the
    order they finish -- those compare by content (parse_records), every other slot word for word."""
    p = Packed.of_nibbles(b, seq, meta, packed_stride)
    b.rewind_big_records()
    rec_p, fl_p = p.planes()
    big_p = b.big_records()[0].copy()
    b.rewind_big_records()
    rec_k, fl_k = p.packed()
    big_k = b.big_records()[0].copy()
    assert np.array_equal(fl_k, fl_p)
    ext = ((rec_p.reshape(-1, RW)[:, 0] >> 16) & gtx.ST_EXTERNAL) != 0
    assert np.array_equal(ext, ((rec_k.reshape(-1, RW)[:, 0] >> 16) & gtx.ST_EXTERNAL) != 0)
    diff = np.nonzero((rec_k.reshape(-1, RW) != rec_p.reshape(-1, RW)).any(axis=1) & ~ext)[0]
    assert len(diff) == 0, "task slots differ: %s (read lengths %s)" % (diff[:8], meta["l_qseq"][diff[:8] // 2])
    if ext.any():
        assert len(big_k) == len(big_p)
        order = b.ctx.hap_order
        assert gtx.parse_records(rec_k, p.n, RW, order, big_k) == gtx.parse_records(rec_p, p.n, RW, order, big_p)
    return p, rec_p, fl_p


def test_gpu_unpack_equals_host_planes():
    """about 200 k reads of every code (N, IUPAC, '='), lengths 1 .. 150: the device's plane rows are the host's inside each read"""
    import torch
    rng = np.random.default_rng(1)
    n = 200_000
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=(n, 150))]
    wild = rng.random(codes.shape) < 0.01
    codes[wild] = rng.integers(0, 16, size=int(wild.sum())).astype(np.uint8)
    codes[:50, :] = 15
    lengths = np.where(rng.random(n) < 0.9, 150, rng.integers(1, 151, size=n)).astype(np.uint32)
    seq = gtx.pack_nibbles(codes)
    rows, start, exc = gtx.pack_2bit(seq, lengths, 40)
    assert len(exc) > n
    b = harness.GpuBackend(gtx.graph_from_records(*scenarios.synthetic_case("snp100", n_ref=3000, n_reads=1, region_begin=1000)[:2],
                                                  region_begin=1000))
    L = gtx.lib()
    d_rows, d_start, d_exc = b._dev(rows), b._dev(start), b._dev(exc)
    for plane_stride in (80, 96):
        d_planes = torch.full((n * plane_stride,), 0xAB, dtype=torch.uint8, device="cuda:0")
        gtx.check(L.gtx_packed_to_planes(b.ctx.h, d_rows.data_ptr(), 40, d_start.data_ptr(), d_exc.data_ptr(), len(exc), n, d_planes.data_ptr(),
                                         plane_stride, None))
        torch.cuda.synchronize()
        got = d_planes.cpu().numpy().reshape(n, plane_stride)
        assert np.array_equal(masked_codes(got, lengths), masked_codes(gtx.pack_planes(seq, plane_stride), lengths))
        assert not got[:, 80:].any()  # (groups behind the packed row: zero)


def test_gpu_packed_align_snp100_with_n_and_iupac():
    ref, recs, codes, pos = scenarios.synthetic_case("snp100", n_ref=60000, n_reads=20000, region_begin=1000000, err=0.01, n_rate=0.003)
    codes = with_ambiguity(codes, 4)
    b = harness.GpuBackend(gtx.graph_from_records(ref, recs, region_begin=1000000))
    seq = gtx.pack_nibbles(codes)
    meta = harness.read_meta(np.full(len(codes), 150), pos=pos)
    p, rec, fl = same_records(b, seq, meta, 40)
    assert len(p.exc) > 10000 and not ((rec.reshape(-1, RW)[:, 0] >> 16) & gtx.ST_ERROR_MASK).any()
    assert np.array_equal(rec, b.align(seq, meta))  # (and the nibble entry point's)
    # wider rows (the hinted pass' row-by-row staging) and an empty batch with NULL buffers
    same_records(b, seq, meta, 48)
    L = gtx.lib()
    assert L.gtx_align_batch_packed(b.ctx.h, None, 40, None, None, 0, None, 0, None, RW, None, None) == 0


def test_gpu_packed_align_indel_graph():
    """the shape of cfg3: SNPs every 100 bp, a tenth of the sites short indels with a SNP close by, all variants added"""
    ref, recs, codes, pos = scenarios.synthetic_case("cfg3", n_ref=60000, n_reads=20000, region_begin=1000000, err=0.01, n_rate=0.003)
    codes = with_ambiguity(codes, 5)
    b = harness.GpuBackend(gtx.graph_from_records(ref, recs, region_begin=1000000, add_all_variants=True))
    seq = gtx.pack_nibbles(codes)
    same_records(b, seq, harness.read_meta(np.full(len(codes), 150), pos=pos), 40)


def test_gpu_packed_align_long_reads():
    """a max_read_len = 1 000 context, reads of 300 and 1 000 bases (rows of 256 bytes: 1 024 bases)"""
    g, o, codes, pos = long_case("snp100", 2000, seed=9, err=0.01, n_rate=0.003)
    codes = with_ambiguity(codes, 6)
    lengths = np.array([300, 1000] * 1000)
    b = harness.GpuBackend(g, max_read_len=1000)
    seq = gtx.pack_nibbles(codes)
    meta = harness.read_meta(lengths, pos=pos)
    p, rec, fl = same_records(b, seq, meta, 256)
    assert b.ctx.long_pass_tasks()[0] > 0 and fl[0::2].sum() > 100


def test_gpu_packed_staged_and_chunked():
    """_staged with a front event, a tail stream and a done event = the plain call; chunks with offset exc_start pointers and the
    matching part of the list = the whole batch"""
    import torch
    ref, recs, codes, pos = scenarios.synthetic_case("snp100", n_ref=60000, n_reads=30000, region_begin=1000000, err=0.01, n_rate=0.003)
    codes = with_ambiguity(codes, 7)
    b = harness.GpuBackend(gtx.graph_from_records(ref, recs, region_begin=1000000))
    seq = gtx.pack_nibbles(codes)
    meta = harness.read_meta(np.full(len(codes), 150), pos=pos)
    p, want_rec, want_fl = same_records(b, seq, meta, 40)
    L = gtx.lib()
    d_rec, d_fl = p.buffers()
    front, done = torch.cuda.Event(), torch.cuda.Event()
    tail = torch.cuda.Stream()
    front.record()  # (a torch event has a HIP event only once recorded)
    done.record()
    torch.cuda.synchronize()
    gtx.check(L.gtx_align_batch_packed_staged(b.ctx.h, p.d_rows.data_ptr(), 40, p.d_start.data_ptr(), p.d_exc.data_ptr(), len(p.exc),
                                              p.d_meta.data_ptr(), p.n, d_rec.data_ptr(), RW, d_fl.data_ptr(), None, C.c_void_p(front.cuda_event),
                                              C.c_void_p(tail.cuda_stream), C.c_void_p(done.cuda_event)))
    torch.cuda.current_stream().wait_event(done)
    rec, fl = p.result(d_rec, d_fl)
    assert np.array_equal(rec, want_rec) and np.array_equal(fl, want_fl)
    # three chunks of one batch: pointers into the rows, exc_start and the list, no rebasing
    d_rec, d_fl = p.buffers()
    for k, e in ((0, 9000), (9000, 21001), (21001, p.n)):
        m = e - k
        gtx.check(L.gtx_align_batch_packed(b.ctx.h, p.d_rows.data_ptr() + k * 40, 40, p.d_start.data_ptr() + 4 * k,
                                           p.d_exc.data_ptr() + 2 * int(p.start[k]), len(p.exc) - int(p.start[k]), p.d_meta.data_ptr() + k * gtx.READ_META.itemsize,
                                           m, d_rec.data_ptr() + k * 2 * RW * 4, RW, d_fl.data_ptr() + 2 * k, None))
    rec, fl = p.result(d_rec, d_fl)
    assert np.array_equal(fl, want_fl)
    heads = want_rec.reshape(-1, RW)[:, 0] >> 16
    assert not (heads & gtx.ST_EXTERNAL).any()  # (no record lies in the big-record arena: every word compares)
    assert np.array_equal(rec, want_rec)


def test_gpu_packed_paired_stream_scores_and_calls():
    """push_packed -> gtx_align_batch_packed -> score -> calls = the plane path's (set_planes -> gtx_align_batch_planes)"""
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=60000, n_pairs=6000, region_begin=310000, n_samples=3)
    codes = with_ambiguity(codes, 8, rate=0.002)
    b = harness.GpuBackend(gtx.graph_from_records(ref, recs, region_begin=310000))
    seq = gtx.pack_nibbles(codes)
    sp, sk = gtx.Stream(b.ctx.params, 1), gtx.Stream(b.ctx.params, 1)
    sp.set_planes(80)
    h = len(rec) // 2
    plane_parts = [sp.push(rec[:h], seq[:h]), sp.push(rec[h:], seq[h:])]
    packed_parts = [sk.push_packed(rec[:h], seq[:h], 40), sk.push_packed(rec[h:], seq[h:], 40)]
    assert sp.counts() == sk.counts()
    meta = np.concatenate([x[1] for x in plane_parts])
    items = np.concatenate([x[2] for x in plane_parts])
    assert np.array_equal(meta, np.concatenate([x[3] for x in packed_parts]))
    assert np.array_equal(items, np.concatenate([x[4] for x in packed_parts]))
    # the two pushes' lists side by side: the second part's offsets continue behind the first's entries
    rows = np.concatenate([x[0] for x in packed_parts])
    exc = np.concatenate([x[2] for x in packed_parts])
    start = np.concatenate([packed_parts[0][1][:-1], packed_parts[1][1] + packed_parts[0][1][-1]])
    p = Packed(b, meta, np.concatenate([x[0] for x in plane_parts]), rows, start, exc)
    rec_p, fl_p = p.planes()
    rec_k, fl_k = p.packed()
    assert np.array_equal(rec_k, rec_p) and np.array_equal(fl_k, fl_p)
    acc_p, acc_k = b.score(items, rec_p, 3), b.score(items, rec_k, 3)
    got_p, got_k = harness.canonical_scores(b.ctx, acc_p), harness.canonical_scores(b.ctx, acc_k)
    assert got_p.sum() > 0 and np.array_equal(got_k, got_p)
    (ph_p, calls_p), (ph_k, calls_k) = b.calls(acc_p, 3), b.calls(acc_k, 3)
    assert np.array_equal(ph_k, ph_p) and np.array_equal(calls_k, calls_p) and (calls_p["gt_second"] > 0).any()
