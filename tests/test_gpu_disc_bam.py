"""Discovery from BAM files on the device (include/gtx.h: gtx_disc_bam_unpack, gtx_discover_files).

gtx_disc_bam_unpack over every record set of tests/disc_bam_cases.py, judged by its judge: every byte of the plane rows, the quality
rows and the CIGAR words equals the plain definition, outputs preset to 0xA5 between guards that stay untouched.  The library's grid
gives a wavefront four records wherever there are that many, so the sets of 63 and more records run the loop over a wavefront's
records.  Then the argument errors, each leaving the outputs as they were, and rows that begin behind byte 2^32 of their arrays, judged
on the device.  gtx_discover_files over the end-to-end set of
tests/disc_variants_cases.py, its three files written as BAM with names of mixed length, aux tags and members of 777 bytes: the words,
the good flags, the records, the text and the per-file statistics are those of gtx_discover_region over the arrays
tests/disc_event_cases.py makes of the same reads, and those of the host chain -- with one, three and eight threads, the smallest
capacities and max_read_len 1000.  Then an empty file and a file of unmapped reads among the others, and a damaged second file.  All
values are integers, letters or bits; there is no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import bam_writer as bw
import disc_bam_cases as bc
import disc_event_cases as dc
import disc_variants_cases as vc
import disc_variants_ref as ref
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_IO = 1, 2, 4, 7


# ---- the unpack kernel ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disc():
    L, h = gtx.lib(), C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, 0, C.byref(h)))
    yield h
    L.gtx_disc_destroy(h)


class OnDevice:
    """a file's stream and tables and its three guarded outputs on the device"""

    def __init__(self, f):
        import torch
        self.torch, self.f = torch, f
        stream, offsets, reads, self.n_cigar = f.tables
        up = lambda a: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
        self.stream, self.offsets, self.reads, self.n_bytes, self.n_reads = up(stream), up(offsets), up(reads), len(stream), len(reads)
        self.out = [torch.from_numpy(bc.guarded(n)).to("cuda:0") for n in bc.sizes(f)]
        torch.cuda.synchronize()

    def args(self, h):
        return [h, self.stream.data_ptr(), self.n_bytes, self.offsets.data_ptr(), self.reads.data_ptr(), self.n_reads, self.out[0].data_ptr() + bc.GUARD,
                self.f.plane_stride, self.out[1].data_ptr() + bc.GUARD, self.f.qual_stride, self.out[2].data_ptr() + bc.GUARD, self.n_cigar, None]

    def outputs(self):
        self.torch.cuda.synchronize()
        return [o.cpu().numpy() for o in self.out]

    def untouched(self):
        return all((o == bc.FILL).all() for o in self.outputs())


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_every_byte_equals_the_definition(disc, name):
    def run(f):
        d = OnDevice(f)
        gtx.disc_bam_unpack(*d.args(disc))
        return d.outputs()
    assert bc.judge(name, run) is None


def test_the_unpack_argument_errors(disc):
    L = gtx.lib()
    f = bc.files("wide")[1]  # (48 and 70: the smallest strides that hold its 70 bases)
    d = OnDevice(f)
    args = d.args(disc)

    def status(**changed):
        names = ["d", "d_stream", "n_bytes", "d_offsets", "d_reads", "n_reads", "d_planes", "plane_stride", "d_qual", "qual_stride", "d_cigar", "n_cigar", "stream"]
        return L.gtx_disc_bam_unpack(*[changed.get(n, a) for n, a in zip(names, args)])
    for bad in (dict(plane_stride=0), dict(plane_stride=40), dict(plane_stride=56), dict(plane_stride=32), dict(qual_stride=69), dict(qual_stride=0), dict(d=None),
                dict(d_stream=None), dict(d_offsets=None), dict(d_reads=None), dict(d_planes=None), dict(d_qual=None), dict(d_cigar=None),
                dict(d_planes=args[6] + 2), dict(d_cigar=args[10] + 1), dict(n_cigar=d.n_cigar - 1), dict(n_bytes=d.n_bytes - 2), dict(n_bytes=1 << 32)):  # (n_bytes: the check knows no name's length and allows for one byte)
        assert status(**bad) == ERR_ARG and L.gtx_last_error().startswith(b"gtx_disc_bam_unpack"), bad
    host = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, -1, C.byref(host)))
    try:
        assert status(d=host) == ERR_NO_DEVICE
    finally:
        L.gtx_disc_destroy(host)
    assert status(n_reads=0) == 0 and status(n_reads=0, d_stream=None, d_offsets=None, d_reads=None, d_planes=None, d_qual=None, d_cigar=None, n_bytes=0, n_cigar=0) == 0
    assert d.untouched()  # none of them launched anything
    assert status() == 0 and bc.file_differs(f, d.outputs()) is None


def test_rows_behind_2_32_bytes(disc):
    """65 537 records of one base and one CIGAR word at strides of 65 536: the last plane row and the last quality row begin at byte
    2^32, where `i * stride` made in 32 bits would be 0 again and the record would be written over the first one's rows.  The 8 GB stay
    on the device and are judged there -- word 0 of the four planes of group 0 and byte 0 of every quality row against the definition
    (a base of code c is bit 0 of the words b with c's bit b set), every other byte zero, the guards as they were; only the verdicts
    and the CIGAR words come back.  The emulation cannot hold this (tests/disc_bam_mutants: ad_row_product_32_bits,
    ad_qual_product_32_bits).  Skipped, with the reason, where the device refuses the 8 GB: the addressing is then held by reading only."""
    import torch
    n, stride = 65537, 65536
    assert (n - 1) * stride == 1 << 32
    i = np.arange(n, dtype=np.uint64)
    codes, quals, words = ((i * 7 + 1) % 16).astype(np.uint8), ((i * 13 + 5) % 256).astype(np.uint8), ((i * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)
    some = [0, 1, 255, n - 2, n - 1]
    small = bc.File([bc.rec(name="r", codes=[int(codes[k])], qual=[int(quals[k])], cigar=[int(words[k])], pos=100 + k % 7) for k in some], plane_stride=16, qual_stride=4)
    one = len(bc.record_bytes(small.records[0]))
    stream = np.tile(np.frombuffer(bc.record_bytes(small.records[0]), np.uint8), n).reshape(n, one).copy()
    at_cigar, at_seq, at_qual = 4 + 32 + 2, 4 + 32 + 2 + 4, 4 + 32 + 2 + 4 + 1
    assert one == at_qual + 1
    stream[:, 8:12] = (100 + i % 7).astype(np.uint32).view(np.uint8).reshape(n, 4)
    stream[:, at_cigar:at_cigar + 4] = words.view(np.uint8).reshape(n, 4)
    stream[:, at_seq] = (codes << 4) | 15
    stream[:, at_qual] = quals
    assert all(stream[k].tobytes() == bc.record_bytes(r) for k, r in zip(some, small.records))  # the records are the case module's
    want_rows = np.zeros((n, 16), np.uint8)
    for b in range(4):
        want_rows[:, 4 * b] = (codes >> b) & 1
    assert np.array_equal(want_rows[some], small.expected[0]) and np.array_equal(quals[some], small.expected[1][:, 0])  # ... and so is what they unpack to
    offsets = (np.arange(n, dtype=np.uint32) * one + 4).astype(np.uint32)
    reads = np.zeros(n, gtx.DISC_READ)
    reads["pos"], reads["flag"], reads["mapq"], reads["l_qseq"], reads["n_cigar"], reads["cigar_off"] = 100 + i % 7, 3, 60, 1, 1, np.arange(n)
    up = lambda a: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
    planes = qual = None
    try:
        try:
            planes = torch.full((bc.GUARD + n * stride + bc.GUARD,), bc.FILL, dtype=torch.uint8, device="cuda:0")
            qual = torch.full((bc.GUARD + n * stride + bc.GUARD,), bc.FILL, dtype=torch.uint8, device="cuda:0")
        except RuntimeError as e:  # (torch.OutOfMemoryError is one)
            pytest.skip("the device refuses two arrays of 4 GB: %s" % str(e).splitlines()[0])
        d_stream, d_offsets, d_reads = up(stream), up(offsets), up(reads)
        cigar = torch.from_numpy(bc.guarded(4 * n)).to("cuda:0")
        torch.cuda.synchronize()
        gtx.disc_bam_unpack(disc, d_stream.data_ptr(), stream.size, d_offsets.data_ptr(), d_reads.data_ptr(), n, planes.data_ptr() + bc.GUARD, stride,
                            qual.data_ptr() + bc.GUARD, stride, cigar.data_ptr() + bc.GUARD, n)
        torch.cuda.synchronize()
        def verdicts(out, want):
            """on the device -> (the guards are as they were, the bytes a record decides are the definition's, every other byte is zero)"""
            want = torch.from_numpy(want).to("cuda:0")
            rows = out[bc.GUARD:-bc.GUARD].view(n, stride)
            return (bool((out[:bc.GUARD] == bc.FILL).all()) and bool((out[-bc.GUARD:] == bc.FILL).all()), bool(torch.equal(rows[:, :want.shape[1]], want)),
                    int(torch.count_nonzero(rows)) == int(torch.count_nonzero(want)))
        assert verdicts(planes, want_rows) == (True, True, True)  # (the last row begins at byte 2^32 of the planes)
        assert verdicts(qual, quals.reshape(n, 1).copy()) == (True, True, True)
        got = cigar.cpu().numpy()
        assert (got[:bc.GUARD] == bc.FILL).all() and (got[-bc.GUARD:] == bc.FILL).all() and got[bc.GUARD:-bc.GUARD].tobytes() == words.tobytes()
    finally:
        planes = qual = None
        torch.cuda.empty_cache()


# ---- the region from files --------------------------------------------------------------------------------------------------------------
def as_record(k, r):
    """a read of the end-to-end set as a BAM record: names of one to 23 letters, two or three aux tags"""
    aux = bw.aux_field("NM", "C", k % 5) + bw.aux_field("RG", "Z", "g") + (bw.aux_field("AS", "i", 140 - k) if k % 3 else b"")
    return bc.rec(name="read%d" % k + "x" * (k % 19), pos=r["pos"], flag=r["flag"], mapq=r["mapq"], codes=[dc.CODE[c] for c in r["seq"]], qual=r["qual"],
                  cigar=r["cigar"], aux=aux)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """the three files of the end-to-end set, then an empty file, a file of unmapped reads, a file cut inside a record, a file that is no BAM"""
    tmp = tmp_path_factory.mktemp("disc_bam")
    _, _, files = vc.simulated_files()
    out = []
    for i, reads in enumerate(files):
        out.append(tmp / ("sample%d.bam" % i))
        bc.write_bam(out[-1], [as_record(k, r) for k, r in enumerate(reads)], block=777)
    out.append(tmp / "empty.bam")
    bc.write_bam(out[-1], [])
    out.append(tmp / "unmapped.bam")
    bc.write_bam(out[-1], [bc.rec(100 + k, n_cigar=0, pos=-1, flag=77, mapq=0, tid=-1, seed=k) for k in range(70)], block=777)
    whole = out[1].read_bytes()
    out.append(tmp / "cut.bam")
    out[-1].write_bytes(whole[:len(whole) // 2])
    out.append(tmp / "other.bam")
    out[-1].write_bytes(bw.bgzf(b"CRAM" + bytes(100)))
    return [str(p) for p in out]


def file_arrays(reference, rb, reads):
    part = dc.Part(reference, rb, reads)
    a = dc.arrays(part)
    return dict(planes=a["planes"], plane_stride=part.stride, qual=a["qual"], qual_stride=a["qual"].shape[1], reads=a["reads"], cigar=a["cigar"])


@functools.lru_cache(maxsize=None)
def from_arrays(**params):
    reference, rb, files = vc.simulated_files()
    return gtx.discover_region(reference, rb, vc.CONTIG, [file_arrays(reference, rb, reads) for reads in files], **params)


def from_files(paths, **params):
    reference, rb, _ = vc.simulated_files()
    return gtx.discover_files(reference, rb, vc.CONTIG, paths, **params)


def outputs(run):
    return run["words"].tobytes(), run["good"].tobytes(), (run["variants"].tobytes(), run["letters"], run["ids"].tobytes()), run["text"]


def test_the_files_are_the_reads(paths):
    """what the end-to-end files are for: the records' fields are the set's, the names and the aux data move the rest to every residue,
    and records straddle the members"""
    _, _, files = vc.simulated_files()
    for path, reads in zip(paths, files):
        got = gtx.disc_bam_read(path)
        assert got["reads"]["pos"].tolist() == [r["pos"] for r in reads] and got["reads"]["l_qseq"].tolist() == [len(r["seq"]) for r in reads]
        assert {int(o) % 4 for o in got["offsets"]} == {0, 1, 2, 3} and {int(got["stream"][o + 8]) % 4 for o in got["offsets"]} == {0, 1, 2, 3}
        assert len(got["stream"]) > 20 * 777


@pytest.mark.parametrize("params", [dict(), dict(n_threads=3), dict(n_threads=8), dict(first_event_cap=1, second_event_cap=1), dict(max_read_len=1000),
                                    dict(n_threads=3, first_event_cap=1, second_event_cap=1)], ids=str)
def test_the_files_give_what_the_arrays_give(paths, params):
    run, want = from_files(paths[:3], **params), from_arrays(**params)
    assert outputs(run) == outputs(want) and run["stats"] == want["stats"] and len(run["stats"]) == 3 and all(st["events"] > 0 for st in run["stats"])
    assert outputs(run) == outputs(from_arrays())


def test_the_files_give_what_the_host_chain_gives(paths):
    run, hc = from_files(paths[:3]), vc.host_chain()
    assert np.array_equal(run["words"], hc["merged"]) and run["good"].tolist() == hc["good"] and run["text"] == hc["text"]
    recs, letters, ids = vc.record_arrays(hc["recs"])
    assert run["variants"].tobytes() == recs.tobytes() and run["letters"] == letters and run["ids"].tolist() == ids.tolist()
    for st, want in zip(run["stats"], hc["wants"]):
        assert (st["n_list"], st["rounds"]["rounds_done"], st["rounds"]["pairs_aligned"], st["rounds"]["pairs_refused"]) == (len(want["lst"]), len(want["lst"]), want["trace"]["aligned"], 0)


def test_an_empty_file_and_a_file_of_unmapped_reads(paths):
    whole = from_files(paths[:3])
    for n_threads in (1, 2):
        run = from_files(paths[:5], n_threads=n_threads)
        assert outputs(run) == outputs(whole) and run["stats"][:3] == whole["stats"] and [st["events"] for st in run["stats"][3:]] == [0, 0]
    only = from_files([paths[3], paths[4], paths[3]], n_threads=3)
    assert only["text"] == ref.COLUMNS.encode() and len(only["variants"]) == 0 and len(only["good"]) == 0 and len(only["stats"]) == 3


def test_a_damaged_file_ends_the_call_with_its_status_and_path(paths):
    cut, other = paths[5], paths[6]
    for n_threads in (1, 3):
        with pytest.raises(gtx.GtxError) as e:
            from_files([paths[0], cut, paths[2]], n_threads=n_threads)
        assert e.value.status == ERR_IO and cut in str(e.value)
        with pytest.raises(gtx.GtxError) as e:  # the first failing file in file order, whichever worker is through first
            from_files([paths[0], other, cut], n_threads=n_threads)
        assert e.value.status == ERR_UNSUPPORTED and other in str(e.value)
    with pytest.raises(gtx.GtxError) as e:
        from_files([paths[0], paths[0] + ".none"])
    assert e.value.status == ERR_IO and ".none" in str(e.value)
    assert outputs(from_files(paths[:3])) == outputs(from_arrays())  # and the library goes on
