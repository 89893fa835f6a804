"""The record walk on the device (include/gtx.h: gtx_disc_bam_walk).

Every stream of tests/disc_bam_walk_cases.py with every one of its cut lists, judged by its judge: the status and its offset, the
counts, every byte of the two tables and the segments whose guess held or that were walked again equal the plain definition, the tables
preset to 0xA5 between guards that stay untouched.  Each list runs twice, for the counts alone and with tables of exactly the count,
and the two calls say the same.  Then a stream cut into more segments than the launch has wavefronts, the argument errors and a table that is too small, each leaving the tables as they were, and
the tables of gtx_disc_bam_read for the same records written as a file.  All values are bytes and words; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import disc_bam_cases as bc
import disc_bam_walk_cases as wc
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_NO_DEVICE, ERR_CAPACITY = 0, 1, 2, 5


@pytest.fixture(scope="module")
def disc():
    L, h = gtx.lib(), C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, 0, C.byref(h)))
    yield h
    L.gtx_disc_destroy(h)


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def walk(disc, data, lists):
    """wc.judge's `run` over the library"""
    import torch
    stream = on_device(np.frombuffer(data, np.uint8)) if data else None
    ptr = stream.data_ptr() if data else None
    out = []
    for cuts in lists:
        rc, counts = gtx.disc_bam_walk(disc, ptr, len(data), cuts)
        assert rc == OK
        tables = [on_device(wc.guarded(counts["n_reads"] * size)) for size in (4, 16)]
        torch.cuda.synchronize()
        rc, got = gtx.disc_bam_walk(disc, ptr, len(data), cuts, tables[0].data_ptr() + wc.GUARD, tables[1].data_ptr() + wc.GUARD, counts["n_reads"])
        assert rc == OK and got == counts
        torch.cuda.synchronize()
        out.append(dict(got, offsets=tables[0].cpu().numpy(), reads=tables[1].cpu().numpy()))
    return out


@pytest.mark.parametrize("name", sorted(wc.SETS))
def test_every_walk_equals_the_definition(disc, name):
    assert wc.judge(name, lambda data, lists: walk(disc, data, lists)) is None


def test_more_segments_than_wavefronts(disc):
    """the launch gives guess and emit a wavefront per segment up to 65 536 segments (16 384 blocks of four), and the sets' longest cut
    list is below 1 000 cuts: only here do the device's wavefronts stride over the segments (`s += step`), which the emulation alone ran
    before.  900 records cut at every byte: more than 65 536 segments, of which the 900 that begin with a record do any work"""
    s = wc.Stream(b"".join(wc.plain(k) for k in range(900)), label="900 records")
    n = len(s.data)
    assert n >= 65538 and s.want["status"] == wc.OK and s.want["n_reads"] == 900
    cuts = list(range(1, n))
    assert len(cuts) + 1 > 65536 and wc.segments(s.data, cuts)[:2] == (900, 0)
    cut, whole = walk(disc, s.data, [cuts, []])
    assert wc.differs(s, cuts, cut) is None and wc.differs(s, [], whole) is None
    assert all(cut[key] == whole[key] for key in ("status", "n_reads", "n_cigar", "max_l_seq")) and (cut["segments_hit"], whole["segments_hit"]) == (900, 1)
    assert cut["offsets"].tobytes() == whole["offsets"].tobytes() and cut["reads"].tobytes() == whole["reads"].tobytes()


def test_the_argument_errors_and_a_table_too_small(disc):
    import torch
    L = gtx.lib()
    s = wc.streams("align")[0]
    n, want = len(s.data), s.want
    stream = on_device(np.frombuffer(s.data, np.uint8))
    tables = [on_device(wc.guarded(want["n_reads"] * size)) for size in (4, 16)]
    torch.cuda.synchronize()
    out = gtx.BamWalkOut()
    cuts = np.array(s.cut_lists[1][1], np.uint32)
    args = dict(d=disc, d_stream=stream.data_ptr(), n_bytes=n, cuts=cuts.ctypes.data, n_cuts=len(cuts), d_offsets=tables[0].data_ptr() + wc.GUARD,
                d_reads=tables[1].data_ptr() + wc.GUARD, cap=want["n_reads"], out=C.byref(out), stream=None)

    def status(**changed):
        return L.gtx_disc_bam_walk(*[changed.get(k, v) for k, v in args.items()])

    def list_of(values):
        a = np.array(values, np.uint32)
        return dict(cuts=a.ctypes.data, n_cuts=len(a), keep=a)

    for bad in (list_of([0]), list_of([n]), list_of([n + 5]), list_of([100, 100]), list_of([200, 100]), list_of([100, 200, 150]), dict(n_bytes=1 << 32), dict(d=None),
                dict(out=None), dict(d_stream=None), dict(cuts=None), dict(d_offsets=None), dict(d_reads=None), dict(d_offsets=None, d_reads=None),
                dict(d_offsets=args["d_offsets"] + 2), dict(d_reads=args["d_reads"] + 1)):
        assert status(**bad) == ERR_ARG and L.gtx_last_error().startswith(b"gtx_disc_bam_walk"), bad
    host = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, -1, C.byref(host)))
    try:
        assert status(d=host) == ERR_NO_DEVICE
    finally:
        L.gtx_disc_destroy(host)
    # an empty stream: no records, nothing launched
    out.n_reads = 7
    assert status(n_bytes=0, n_cuts=0, cuts=None) == OK and status(n_bytes=0, n_cuts=0, cuts=None, d_stream=None, d_offsets=None, d_reads=None, cap=0) == OK
    assert (out.status, out.n_reads, out.n_cigar, out.max_l_seq, out.segments_hit, out.segments_rewalked) == (0, 0, 0, 0, 0, 0)
    # tables one entry too small: the counts are there and nothing is written
    for cap in (want["n_reads"] - 1, 0):
        assert status(cap=cap) == ERR_CAPACITY and b"records" in L.gtx_last_error()
        assert (out.status, out.n_reads, out.n_cigar, out.max_l_seq) == (0, want["n_reads"], want["n_cigar"], want["max_l_seq"])
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == wc.FILL).all() for t in tables)  # none of them wrote a table entry
    # the counts alone, and the call as it is meant
    assert status(d_offsets=None, d_reads=None, cap=0) == OK and out.n_reads == want["n_reads"] and out.segments_hit == len(cuts) + 1
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == wc.FILL).all() for t in tables)
    assert status() == OK
    torch.cuda.synchronize()
    got = dict({k: getattr(out, k) for k in ("status", "bad_at", "n_reads", "n_cigar", "max_l_seq", "segments_hit", "segments_rewalked")},
               offsets=tables[0].cpu().numpy(), reads=tables[1].cpu().numpy())
    assert wc.differs(s, cuts.tolist(), got) is None


def test_the_tables_are_those_of_the_host_walk(disc, tmp_path):
    """the same records written as a file and read by gtx_disc_bam_read: its stream walked on the device gives its two tables"""
    import torch
    records = [wc.plain(k) for k in range(300)] + [wc.plain(400, l_seq=700, n_cigar=40)]
    for block in (None, 777):
        path = tmp_path / ("walk%s.bam" % block)
        bc.write_bam(path, records, block=block)
        host = gtx.disc_bam_read(path)
        data = host["stream"].tobytes()
        assert data == b"".join(records)
        for cuts in ([], list(range(777, len(data), 777)), list(range(5000, len(data), 5000))):
            got, = walk(disc, data, [cuts])
            assert (got["status"], got["n_reads"], got["n_cigar"], got["max_l_seq"]) == (0, len(host["reads"]), host["n_cigar"], host["max_l_seq"])
            assert got["offsets"][wc.GUARD:-wc.GUARD].tobytes() == host["offsets"].tobytes() and got["reads"][wc.GUARD:-wc.GUARD].tobytes() == host["reads"].tobytes()
    torch.cuda.synchronize()
