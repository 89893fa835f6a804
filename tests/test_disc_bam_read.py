"""gtx_disc_bam_read (include/gtx.h): a BAM file of discovery read whole on the host -- the record stream, the offsets, the gtx_disc_read
table, the longest read, the CIGAR words' number, the sample -- against the records that were written (tests/disc_bam_cases.py), from
files with whole records per BGZF member and from files cut into members of 777 bytes, so that records, their fixed bytes and their
block_size words straddle members.  Then every stream of the record walk's sets (tests/disc_bam_walk_cases.py), whose definition claims
to be this walk: the same tables, or the error of the first bad record's class.  Then the empty file, an unmapped tail, every damage with its status -- the one gtx_reads_open /
gtx_reads_next give for the same file --, the two refusals, and gtx_discover_files' answer without a device.  No device."""
import struct

import numpy as np
import pytest

import bam_writer as bw
import disc_bam_cases as bc
import disc_bam_walk_cases as wc
from graphtyper_amd import lib as gtx

ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_IO = 1, 2, 4, 5, 7


@pytest.fixture(scope="module", autouse=True)
def built():
    gtx.build()


def differs(f, got):
    stream, offsets, reads, n_cigar = f.tables
    for what, a, b in (("the stream", got["stream"], stream), ("the offsets", got["offsets"], offsets), ("the reads", got["reads"], reads)):
        if a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return what
    longest = max([len(r["codes"]) for r in f.records] + [0])
    if (got["max_l_seq"], got["n_cigar"], got["sample"]) != (longest, n_cigar, "sample"):
        return "the sizes or the sample: %s" % ((got["max_l_seq"], got["n_cigar"], got["sample"]),)
    return None


@pytest.mark.parametrize("block", [None, 777])
@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_the_file_as_it_was_written(tmp_path, name, block):
    for k, f in enumerate(bc.files(name)):
        path = tmp_path / ("%s%d.bam" % (name, k))
        bc.write_bam(path, f.records, block=block)
        assert differs(f, gtx.disc_bam_read(str(path))) is None


def test_the_sample_is_the_file_name_without_read_groups(tmp_path):
    path = tmp_path / "NA12878.chr1.bam"
    bc.write_bam(path, bc.files("quals")[0].records, header_text="@HD\tVN:1.6\n")
    assert gtx.disc_bam_read(str(path))["sample"] == "NA12878"
    bc.write_bam(path, [], header_text="@RG\tID:a\tSM:one\n@RG\tID:b\tSM:one\tPL:x\n")  # two read groups of one sample
    assert gtx.disc_bam_read(str(path))["sample"] == "one"


def test_the_empty_file_and_an_unmapped_tail(tmp_path):
    path = tmp_path / "empty.bam"
    bc.write_bam(path, [])
    got = gtx.disc_bam_read(str(path))
    assert len(got["stream"]) == len(got["reads"]) == len(got["offsets"]) == 0 and (got["max_l_seq"], got["n_cigar"]) == (0, 0)
    # mapped reads, then reads of no contig: every record is there, file order, tid not looked at
    tail = [bc.rec(30, seed=1), bc.rec(31, seed=2, pos=500)] + [bc.rec(20 + k, n_cigar=0, pos=-1, flag=4 + 1 + 8, mapq=0, tid=-1, seed=10 + k) for k in range(3)]
    f = bc.File(tail)
    for block in (None, 777):
        bc.write_bam(path, tail, block=block)
        got = gtx.disc_bam_read(str(path))
        assert differs(f, got) is None and got["reads"]["pos"].tolist() == [100, 500, -1, -1, -1] and got["reads"]["n_cigar"].tolist()[2:] == [0, 0, 0]


def status_of(call, *args):
    with pytest.raises(gtx.GtxError) as e:
        call(*args)
    return e.value.status, str(e.value)


def reader_status(path):
    """what gtx_reads_open, or the gtx_reads_next behind it, says to the file"""
    def run():
        r = gtx.Reads([str(path)])
        try:
            while len(r.next(64, seq_stride=600)[0]):
                pass
        finally:
            r.close()
    return status_of(run)[0]


def damaged_files(tmp_path):
    """-> [(what, path, status)]"""
    good = [bc.record_bytes(bc.rec(40, seed=k, n_cigar=2)) for k in range(5)]
    head = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrT\0" + struct.pack("<i", 1000)
    body = bytearray(good[2])
    out = []

    def add(what, data, status):
        path = tmp_path / (what.replace(" ", "_") + ".bam")
        path.write_bytes(data if what == "no gzip" else bw.bgzf(data))
        out.append((what, path, status))
    add("no gzip", b"this is no BAM file at all, nor gzip" * 4, ERR_UNSUPPORTED)
    add("no magic", b"CRAM" + head[4:] + b"".join(good), ERR_UNSUPPORTED)
    add("header cut in the references", head[:18], ERR_IO)
    add("cut inside a record", head + b"".join(good)[:-17], ERR_IO)
    add("cut inside a block size", head + b"".join(good) + b"\x40\0", ERR_IO)
    add("a block below 32 bytes", head + good[0] + struct.pack("<i", 31) + bytes(31) + good[1], ERR_IO)
    add("a negative block size", head + good[0] + struct.pack("<i", -5), ERR_IO)
    for what, at, fmt, value in (("l_seq beyond the block", 4 + 16, "<i", 4000), ("a negative l_seq", 4 + 16, "<i", -1), ("n_cigar beyond the block", 4 + 12, "<H", 60000),
                                 ("a name beyond the block", 4 + 8, "<B", 255)):
        bad = bytearray(body)
        bad[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        add(what, head + good[0] + good[1] + bytes(bad) + good[3], ERR_IO)
    return out


def test_every_damage_has_the_status_the_merging_reader_gives(tmp_path):
    for what, path, status in damaged_files(tmp_path):
        got, message = status_of(gtx.disc_bam_read, str(path))
        assert got == status and str(path) in message, (what, got, message)
        assert reader_status(path) == status, what
    got, message = status_of(gtx.disc_bam_read, str(tmp_path / "none.bam"))
    assert got == ERR_IO == reader_status(tmp_path / "none.bam") and "none.bam" in message
    path = tmp_path / "rg.bam"
    bc.write_bam(path, [], header_text="@RG\tID:a\n")
    assert status_of(gtx.disc_bam_read, str(path))[0] == ERR_ARG == reader_status(path)


def test_a_read_of_65536_bases_and_two_samples_are_refused(tmp_path):
    path = tmp_path / "long.bam"
    bc.write_bam(path, [bc.rec(10, seed=1), bc.rec(65535, seed=2)])
    assert gtx.disc_bam_read(str(path))["max_l_seq"] == 65535
    bc.write_bam(path, [bc.rec(10, seed=1), bc.rec(65536, seed=2)])
    got, message = status_of(gtx.disc_bam_read, str(path))
    assert got == ERR_UNSUPPORTED and "65535" in message and str(path) in message
    bc.write_bam(path, [bc.rec(10, seed=1)], header_text="@RG\tID:a\tSM:one\n@RG\tID:b\tSM:two\n")
    got, message = status_of(gtx.disc_bam_read, str(path))
    assert got == ERR_UNSUPPORTED and "sample" in message and str(path) in message


@pytest.mark.parametrize("name", sorted(wc.SETS))
def test_the_walk_sets_definition_is_the_host_walk(tmp_path, name):
    """the second witness of tests/disc_bam_walk_cases.py: define() claims to be this walk (append_bam_block, parse_bam_core and the bound
    of 65 535 bases, in that order per record).  Every stream of the set written as a file: a sound one comes back with byte-identical
    tables, a bad one fails as its class does -- TRUNCATED: GTX_ERR_IO "truncated BAM record"; MALFORMED: GTX_ERR_IO "malformed BAM
    record"; LONG_READ: GTX_ERR_UNSUPPORTED "more than 65535 bases" --, whatever lies behind the first bad record"""
    errors = {wc.TRUNCATED: (ERR_IO, "truncated BAM record"), wc.MALFORMED: (ERR_IO, "malformed BAM record"), wc.LONG_READ: (ERR_UNSUPPORTED, "more than 65535 bases")}
    for k, s in enumerate(wc.streams(name)):
        path = tmp_path / ("%s%d.bam" % (name, k))
        bc.write_bam(path, [s.data], block=60000)
        want = s.want
        if want["status"] == wc.OK:
            got = gtx.disc_bam_read(str(path))
            assert got["stream"].tobytes() == s.data and got["offsets"].tobytes() == want["offsets"].tobytes() and got["reads"].tobytes() == want["reads"].tobytes(), s.label
            assert got["offsets"].dtype == want["offsets"].dtype and (got["max_l_seq"], got["n_cigar"], len(got["reads"])) == (want["max_l_seq"], want["n_cigar"], want["n_reads"])
        else:
            status, message = status_of(gtx.disc_bam_read, str(path))
            assert status == errors[want["status"]][0] and errors[want["status"]][1] in message, (s.label, want["status"], status, message)


def test_null_arguments():
    import ctypes as C
    L, h = gtx.lib(), C.c_void_p(77)
    assert L.gtx_disc_bam_read(None, C.byref(h)) == ERR_ARG and h.value is None
    assert L.gtx_disc_bam_read(b"x.bam", None) == ERR_ARG
    n64, n32 = C.c_uint64(9), C.c_uint32(9)
    assert L.gtx_disc_bam_stream(None, C.byref(n64), C.byref(n32)) is None and n64.value == 0
    assert L.gtx_disc_bam_reads(None, C.byref(n32), None) is None and n32.value == 0 and L.gtx_disc_bam_info(None, None, None) is None
    L.gtx_disc_bam_destroy(None)


def test_discover_files_without_a_device_opens_no_path(tmp_path):
    """GTX_ERR_NO_DEVICE is decided before any file is opened: the path does not exist, and the status is not the one of a missing file"""
    with pytest.raises(gtx.GtxError) as e:
        gtx.discover_files("ACGTACGTAC", 0, "chrT", [str(tmp_path / "missing.bam")], device=-1)
    assert e.value.status == ERR_NO_DEVICE
    for bad in (dict(n_threads=0), dict(n_threads=9), dict(bucket_size=0)):
        with pytest.raises(gtx.GtxError) as e:
            gtx.discover_files("ACGTACGTAC", 0, "chrT", [str(tmp_path / "missing.bam")], device=-1, **bad)
        assert e.value.status == ERR_ARG
    with pytest.raises(gtx.GtxError) as e:
        gtx.discover_files("ACGTACGTAC", 0, "chrT", [], device=-1)
    assert e.value.status == ERR_ARG
