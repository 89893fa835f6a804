"""Reads as packed 2-bit rows with an exception list (include/gtx.h): the host packer (gtx_pack_2bit, gtx_stream_push_packed)
against a numpy restatement of the layout, and the unpacking of gtx_packed_kernel -- its graph_dev.hpp helpers, run through a
host emulation under AddressSanitizer (tests/emu_packed) -- against gtx_pack_planes, on well-formed and malformed lists.  The
device: test_gpu_packed_reads.py."""
import ctypes as C

import numpy as np
import pytest

import emu_programs
import scenarios
from graphtyper_amd import lib as gtx

ERR_ARG, ERR_NO_DEVICE, ERR_CAPACITY = 1, 2, 5
LENGTHS = [1, 31, 32, 33, 63, 150, 151, 250, 256, 300, 1000]


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


@pytest.fixture(scope="session")
def emu_packed(tmp_path_factory):
    return emu_programs.build("emu_packed", tmp_path_factory.mktemp("emu_packed"))


def tight(length):
    return max(8, (length + 31) // 32 * 8)


def random_codes(rng, n, length, p_exc=0.5):
    """codes of all 16 kinds: ACGT everywhere, and at a share p_exc of the bases any of the 16"""
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=(n, length))]
    wild = rng.random((n, length)) < p_exc
    codes[wild] = rng.integers(0, 16, size=int(wild.sum())).astype(np.uint8)
    return codes


def emulate(exe, tmp_path, rows, exc_start, exc, n_exc, plane_stride):
    """gtx_packed_kernel over (rows, exc_start, exc[:n_exc]) on the host, under ASan: [n, plane_stride] plane rows"""
    rows = np.ascontiguousarray(rows, np.uint8)
    n, packed_stride = rows.shape

    def write(path):
        with open(path, "wb") as f:
            f.write(np.array([n, packed_stride, plane_stride, n_exc], np.uint32).tobytes())
            f.write(rows.tobytes())
            f.write(np.ascontiguousarray(exc_start, np.uint32).tobytes())
            f.write(np.ascontiguousarray(exc[:n_exc], np.uint16).tobytes())
    return emu_programs.run(exe, tmp_path, write, lambda path: np.fromfile(path, np.uint8).reshape(n, plane_stride))


def masked_codes(planes, lengths):
    """the BAM code of every base inside each read's length (-1 behind it): plane rows compared where they mean something"""
    n, stride = planes.shape
    w = planes.view(np.uint32).reshape(n, stride // 16, 4)
    j = np.arange(32, dtype=np.uint32)
    bits = [((w[:, :, b, None] >> j) & 1).reshape(n, -1).astype(np.int16) for b in range(4)]
    codes = bits[0] | (bits[1] << 1) | (bits[2] << 2) | (bits[3] << 3)
    codes[np.arange(codes.shape[1])[None, :] >= np.asarray(lengths)[:, None]] = -1
    return codes


@pytest.mark.parametrize("length", LENGTHS)
def test_host_pack_is_the_packed_layout(length):
    rng = np.random.default_rng(length)
    codes = random_codes(rng, 65, length)
    seq = gtx.pack_nibbles(codes)
    for packed_stride in sorted({tight(length), tight(length) + 8, tight(length) + 40}):
        rows, start, exc = gtx.pack_2bit(seq, np.full(len(codes), length), packed_stride)
        w_rows, w_start, w_exc = gtx.packed_reference(codes, packed_stride)
        assert np.array_equal(rows, w_rows) and np.array_equal(start, w_start) and np.array_equal(exc, w_exc)


def test_host_pack_mixed_lengths_and_unambiguous_reads_equal_planes():
    """reads of different lengths in one batch; for a read of A, C, G and T only the packed words are plane words 1|3 and 2|3"""
    rng = np.random.default_rng(9)
    lengths = rng.integers(1, 1001, size=200)
    codes = random_codes(rng, 200, 1000, p_exc=0.002)
    seq = gtx.pack_nibbles(codes, stride=512)
    rows, start, exc = gtx.pack_2bit(seq, lengths, 256)
    w_rows, w_start, w_exc = gtx.packed_reference(codes, 256, lengths)
    assert np.array_equal(rows, w_rows) and np.array_equal(start, w_start) and np.array_equal(exc, w_exc)
    clean = np.diff(start.astype(np.int64)) == 0
    assert clean.sum() > 50
    planes = gtx.pack_planes(seq, 512).view(np.uint32).reshape(200, 32, 4)
    pw = rows.view(np.uint32).reshape(200, 32, 2)
    for i in np.nonzero(clean)[0]:
        g = (lengths[i] + 31) // 32
        last = np.uint32(0xFFFFFFFF) if lengths[i] % 32 == 0 else np.uint32((1 << (lengths[i] % 32)) - 1)
        mask = np.full(g, 0xFFFFFFFF, np.uint32)
        mask[-1] = last
        assert np.array_equal(pw[i, :g, 0], (planes[i, :g, 1] | planes[i, :g, 3]) & mask)
        assert np.array_equal(pw[i, :g, 1], (planes[i, :g, 2] | planes[i, :g, 3]) & mask)


@pytest.mark.parametrize("length", LENGTHS)
def test_emulated_unpack_equals_planes(emu_packed, tmp_path, length):
    rng = np.random.default_rng(100 + length)
    codes = random_codes(rng, 40, length, p_exc=0.05)
    codes[0, :] = 15  # all N
    codes[1, 0] = 15  # first base
    codes[2, -1] = 4 if length > 1 else 0  # last base ('=' for a single base)
    codes[3, 31::32] = 2 | 8  # the last base of every group ...
    codes[4, 32::32] = 0  # ... and the first of the next
    codes[5, :] = 1  # no exception
    seq = gtx.pack_nibbles(codes)
    lengths = np.full(len(codes), length)
    for packed_stride in sorted({tight(length), tight(length) + 16}):
        rows, start, exc = gtx.pack_2bit(seq, lengths, packed_stride)
        got = emulate(emu_packed, tmp_path, rows, start, exc, len(exc), 2 * packed_stride)
        want = gtx.pack_planes(seq, 2 * packed_stride)
        assert np.array_equal(masked_codes(got, lengths), masked_codes(want, lengths))


def test_emulated_unpack_of_a_slice(emu_packed, tmp_path):
    """exc_start + k with the matching part of the list (offsets from exc_start[0]): the slice unpacks as in the whole batch"""
    rng = np.random.default_rng(5)
    codes = random_codes(rng, 300, 150, p_exc=0.01)
    seq = gtx.pack_nibbles(codes)
    rows, start, exc = gtx.pack_2bit(seq, np.full(300, 150), 40)
    whole = emulate(emu_packed, tmp_path, rows, start, exc, len(exc), 80)
    for k, e in ((0, 100), (100, 217), (217, 300)):
        part = emulate(emu_packed, tmp_path, rows[k:e], start[k:e + 1], exc[start[k]:], len(exc) - int(start[k]), 80)
        assert np.array_equal(part, whole[k:e])
    # absolute values do not matter: the offsets count from the slice's first entry
    shifted = emulate(emu_packed, tmp_path, rows, start + np.uint32(0xFFFFFF00), exc, len(exc), 80)
    assert np.array_equal(shifted, whole)


def unpack_reference(rows, exc_start, exc, n_exc, plane_stride):
    """what the kernel promises for any list: the run of read i clamped to n_exc (decreasing: empty), entries of other
    groups skipped"""
    n, packed_stride = rows.shape
    w = rows.view(np.uint32).reshape(n, packed_stride // 8, 2)
    groups = plane_stride // 16
    out = np.zeros((n, groups, 4), np.uint32)
    pg = min(groups, packed_stride // 8)
    lo, hi = w[:, :pg, 0], w[:, :pg, 1]
    out[:, :pg] = np.stack([~lo & ~hi, lo & ~hi, ~lo & hi, lo & hi], axis=2)
    s = [int(x) for x in exc_start]
    for i in range(n):
        b = min((s[i] - s[0]) % (1 << 32), n_exc)
        e = max(min((s[i + 1] - s[0]) % (1 << 32), n_exc), b)
        for x in exc[b:e]:
            at, code = int(x) & 0xFFF, int(x) >> 12
            g = at >> 5
            if g < pg:
                bit = np.uint32(1 << (at & 31))
                for p in range(4):
                    out[i, g, p] = (out[i, g, p] & ~bit) | (bit if (code >> p) & 1 else 0)
    return out.reshape(n, groups * 4).view(np.uint8).reshape(n, plane_stride)


def test_emulated_unpack_of_malformed_lists(emu_packed, tmp_path):
    """decreasing starts, entries past the row, offsets that claim more entries than n_exc, unsorted runs: every access stays in
    the buffers (the driver runs under ASan with exact-size blocks) and the result is the clamped reading"""
    rng = np.random.default_rng(77)
    codes = random_codes(rng, 64, 150, p_exc=0.03)
    seq = gtx.pack_nibbles(codes)
    rows, start, exc = gtx.pack_2bit(seq, np.full(64, 150), 40)
    assert len(exc) > 50
    cases = []
    dec = start.copy()
    dec[10], dec[30] = dec[40], dec[2]  # two decreasing runs (and a long one in front of each)
    cases.append(("decreasing starts", dec, exc, len(exc)))
    past = exc.copy()
    past[::3] = (past[::3] & 0xF000) | rng.integers(160, 4096, size=len(past[::3])).astype(np.uint16)
    cases.append(("indices past the row", start, past, len(exc)))
    cases.append(("n_exc below the prefix", start, exc, len(exc) // 2))
    cases.append(("n_exc 0", start, exc, 0))
    huge = start.copy()
    huge[20:] += np.uint32(1 << 31)
    cases.append(("offsets far past the list", huge, exc, len(exc)))
    wrap = start.copy()
    wrap[0] = 1000
    cases.append(("starts below exc_start[0]", wrap, exc, len(exc)))
    cases.append(("unsorted runs", start, exc[rng.permutation(len(exc))], len(exc)))
    for name, s, e, ne in cases:
        for plane_stride in (80, 96, 48):
            got = emulate(emu_packed, tmp_path, rows, s, e, ne, plane_stride)
            assert np.array_equal(got, unpack_reference(rows, s, e, ne, plane_stride)), (name, plane_stride)
    # the well-formed list through the same restatement: the restatement is the plane layout
    assert np.array_equal(masked_codes(unpack_reference(rows, start, exc, len(exc), 80), np.full(64, 150)),
                          masked_codes(gtx.pack_planes(seq, 80), np.full(64, 150)))


def test_pack_argument_and_capacity_errors():
    L = gtx.lib()
    codes = np.full((4, 150), 15, np.uint8)
    seq = gtx.pack_nibbles(codes)
    lens = np.full(4, 150, np.uint32)
    rows = np.zeros((4, 40), np.uint8)
    start = np.zeros(5, np.uint32)
    exc = np.zeros(599, np.uint16)
    n = C.c_uint32()
    p = gtx._p
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 40, p(start), p(exc), 599, C.byref(n)) == ERR_CAPACITY
    assert n.value == 600 and start[4] == 600
    exc = np.zeros(600, np.uint16)
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 40, p(start), p(exc), 600, C.byref(n)) == 0 and n.value == 600
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 36, p(start), p(exc), 600, C.byref(n)) == ERR_ARG  # not a multiple of 8
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 32, p(start), p(exc), 600, C.byref(n)) == ERR_ARG  # 150 > 4 x 32
    assert L.gtx_pack_2bit(p(seq), 74, p(lens), 4, p(rows), 40, p(start), p(exc), 600, C.byref(n)) == ERR_ARG  # 150 > 2 x 74
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 40, None, p(exc), 600, C.byref(n)) == ERR_ARG
    assert L.gtx_pack_2bit(p(seq), 80, p(lens), 4, p(rows), 40, p(start), None, 600, C.byref(n)) == ERR_ARG
    big = gtx.pack_nibbles(np.ones((1, 4096), np.uint8))
    big_rows = np.zeros((1, 1024), np.uint8)
    s2 = np.zeros(2, np.uint32)
    assert L.gtx_pack_2bit(p(big), big.shape[1], p(np.array([4096], np.uint32)), 1, p(big_rows), 1024, p(s2), p(exc), 600, C.byref(n)) == ERR_ARG
    assert L.gtx_pack_2bit(p(big), big.shape[1], p(np.array([4095], np.uint32)), 1, p(big_rows), 1024, p(s2), p(exc), 600, C.byref(n)) == 0
    assert L.gtx_pack_2bit(None, 80, None, 0, None, 40, p(s2), None, 0, C.byref(n)) == 0 and n.value == 0 and s2[0] == 0


def test_device_entry_points_without_a_device():
    """argument checks first, then GTX_ERR_NO_DEVICE on a context made with device -1"""
    import harness
    ref, recs, codes, pos = scenarios.synthetic_case("snp100", n_ref=3000, n_reads=8, region_begin=1000)
    b = harness.EmuBackend(gtx.graph_from_records(ref, recs, region_begin=1000))
    L = gtx.lib()
    h = b.ctx.h if hasattr(b, "ctx") else b.h
    rows = np.zeros((8, 40), np.uint8)
    start = np.zeros(9, np.uint32)
    meta = harness.read_meta(np.full(8, 150), pos=pos)
    rec = np.zeros(8 * 2 * harness.REC_WORDS, np.uint32)
    planes = np.zeros((8, 80), np.uint8)
    p = gtx._p
    assert L.gtx_packed_to_planes(h, p(rows), 40, p(start), None, 0, 8, p(planes), 80, None) == ERR_NO_DEVICE
    assert L.gtx_align_batch_packed(h, p(rows), 40, p(start), None, 0, p(meta), 8, p(rec), harness.REC_WORDS, None, None) == ERR_NO_DEVICE
    assert L.gtx_align_batch_packed_staged(h, p(rows), 40, p(start), None, 0, p(meta), 8, p(rec), harness.REC_WORDS, None, None, None, None,
                                           None) == ERR_NO_DEVICE
    assert L.gtx_packed_to_planes(h, p(rows), 36, p(start), None, 0, 8, p(planes), 80, None) == ERR_ARG
    assert L.gtx_packed_to_planes(h, p(rows), 40, p(start), None, 3, 8, p(planes), 80, None) == ERR_ARG  # entries but no list
    assert L.gtx_packed_to_planes(h, p(rows), 40, None, None, 0, 8, p(planes), 80, None) == ERR_ARG
    assert L.gtx_packed_to_planes(h, p(rows), 40, p(start), None, 0, 8, p(planes), 72, None) == ERR_ARG
    assert L.gtx_packed_to_planes(None, p(rows), 40, p(start), None, 0, 8, p(planes), 80, None) == ERR_ARG
    assert L.gtx_align_batch_packed(h, p(rows), 40, p(start), None, 0, p(meta), 8, p(rec), 4, None, None) == ERR_ARG
    assert L.gtx_align_batch_packed(h, p(rows), 12, p(start), None, 0, p(meta), 8, p(rec), harness.REC_WORDS, None, None) == ERR_ARG
    assert L.gtx_align_batch_packed(h, p(rows), 40, None, None, 0, p(meta), 8, p(rec), harness.REC_WORDS, None, None) == ERR_ARG
    assert L.gtx_align_batch_packed(None, p(rows), 40, p(start), None, 0, p(meta), 8, p(rec), harness.REC_WORDS, None, None) == ERR_ARG


def push_both(rec, codes, packed_stride, params=None, n_rg=1, chunks=1):
    params = params or gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0)
    a, b = gtx.Stream(params, n_rg), gtx.Stream(params, n_rg)
    seq = gtx.pack_nibbles(codes)
    out_a, out_b = [], []
    for part in np.array_split(np.arange(len(rec)), chunks):
        out_a.append(a.push(rec[part], seq[part]))
        out_b.append(b.push_packed(rec[part], seq[part], packed_stride))
    assert a.counts() == b.counts()
    return out_a, out_b, a.counts()


@pytest.mark.parametrize("chunks", [1, 7])
def test_push_packed_equals_push(chunks):
    """paired reads with duplicates, filtered and low-MAPQ records: the same meta and items; rows and list = pack_2bit of what
    push returns"""
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=20000, n_pairs=400, region_begin=5000, dup_frac=0.2)
    codes = codes.copy()
    rng = np.random.default_rng(3)
    amb = rng.random(codes.shape) < 0.01
    codes[amb] = rng.integers(0, 16, size=int(amb.sum())).astype(np.uint8)
    out_a, out_b, counts = push_both(rec, codes, 40, chunks=chunks)
    for (a_seq, a_meta, a_items), (rows, start, exc, b_meta, b_items) in zip(out_a, out_b):
        assert np.array_equal(a_meta, b_meta) and np.array_equal(a_items, b_items)
        w_rows, w_start, w_exc = gtx.pack_2bit(a_seq, a_meta["l_qseq"], 40)
        assert np.array_equal(rows, w_rows) and np.array_equal(start, w_start) and np.array_equal(exc, w_exc)
    paired = np.concatenate([x[2] for x in out_a])["second"]["align_index"] != gtx.INVALID_ID
    assert sum(len(x[1]) for x in out_a) > 300 and sum(len(x[2]) for x in out_b) > 0
    assert counts["duplicated"] > 0 and paired.sum() > 100


def test_push_packed_errors_leave_the_stream_untouched():
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=20000, n_pairs=50, region_begin=5000)
    codes = codes.copy()
    codes[:, 7] = 15  # one N per read
    seq = gtx.pack_nibbles(codes)
    params = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0)
    s = gtx.Stream(params, 1)
    L = gtx.lib()
    n = len(rec)
    rows = np.zeros((n, 40), np.uint8)
    start = np.zeros(n + 1, np.uint32)
    exc = np.zeros(n, np.uint16)
    meta = np.zeros(n, gtx.READ_META)
    items = np.zeros(n, gtx.SCORE_ITEM)
    ne, na, ni = C.c_uint32(), C.c_uint32(), C.c_uint32()
    p = gtx._p
    recs_c = np.ascontiguousarray(rec, gtx.STREAM_RECORD)
    assert L.gtx_stream_push_packed(s.h, p(recs_c), p(seq), seq.shape[1], n, p(rows), 40, p(start), p(exc), n - 1, C.byref(ne), p(meta), n,
                                    C.byref(na), p(items), n, C.byref(ni)) == ERR_CAPACITY
    assert ne.value == n and s.counts()["records"] == 0 and s.counts()["parked"] == 0
    assert L.gtx_stream_push_packed(s.h, p(recs_c), p(seq), seq.shape[1], n, p(rows), 32, p(start), p(exc), n, C.byref(ne), p(meta), n,
                                    C.byref(na), p(items), n, C.byref(ni)) == ERR_ARG  # 150 bases > 4 x 32
    assert L.gtx_stream_push_packed(s.h, p(recs_c), p(seq), seq.shape[1], n, p(rows), 44, p(start), p(exc), n, C.byref(ne), p(meta), n,
                                    C.byref(na), p(items), n, C.byref(ni)) == ERR_ARG  # not a multiple of 8
    assert s.counts()["records"] == 0
    assert L.gtx_stream_push_packed(s.h, p(recs_c), p(seq), seq.shape[1], n, p(rows), 40, p(start), p(exc), n, C.byref(ne), p(meta), n,
                                    C.byref(na), p(items), n, C.byref(ni)) == 0
    assert s.counts()["records"] > 0 and ne.value == start[na.value] and ne.value > 0
