"""Discovery from BAM files with the device front (include/gtx.h: gtx_discover_files_front, gtx_discover_front): the files' members
inflated, their records walked and unpacked on the device.

The end-to-end set of tests/disc_variants_cases.py (three files, 3 kb) written twice -- in the aligned layout of tests/bam_writer.py,
where no record crosses a member, and cut into members of 777 bytes wherever they fall -- with names of mixed length and aux tags.
The device front gives the words, the good flags, the records, the text and the per-file statistics of gtx_discover_files and of
gtx_discover_region over the arrays tests/disc_event_cases.py makes of the same reads, with one, three and eight threads and the
smallest event capacities; every member went through the device, nothing fell back, and only the cut files walked a segment again.
Then an empty file and a file of unmapped reads; then the files that are not sound -- cut, no BAM, missing, a flipped payload byte, a
record whose l_seq was raised before its member's CRC was made --, each of which ends the call with the status and the path the
host front gives, after which the library goes on.  All values are integers, letters or bits; there is no tolerance."""
import functools
import struct
import zlib

import numpy as np
import pytest

import bam_writer as bw
import disc_bam_cases as bc
import disc_event_cases as dc
import disc_variants_cases as vc
import disc_variants_ref as ref
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu


def as_record(k, r):
    """a read of the end-to-end set as a BAM record: names of one to 23 letters, two or three aux tags"""
    aux = bw.aux_field("NM", "C", k % 5) + bw.aux_field("RG", "Z", "g") + (bw.aux_field("AS", "i", 140 - k) if k % 3 else b"")
    return bc.rec(name="read%d" % k + "x" * (k % 19), pos=r["pos"], flag=r["flag"], mapq=r["mapq"], codes=[dc.CODE[c] for c in r["seq"]], qual=r["qual"],
                  cigar=r["cigar"], aux=aux)


def members(data):
    """[(offset, header length, compressed length)] of a BGZF file's members (BC first, as bam_writer writes them)"""
    out, at = [], 0
    while at < len(data):
        xlen, bsize = struct.unpack_from("<H", data, at + 10)[0], struct.unpack_from("<H", data, at + 16)[0]
        out.append((at, 12 + xlen, bsize + 1 - 12 - xlen - 8))
        at += bsize + 1
    return out


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("disc_front")
    _, _, files = vc.simulated_files()
    out = dict(aligned=[], cut=[])
    for i, reads in enumerate(files):
        records = [as_record(k, r) for k, r in enumerate(reads)]
        for layout, block in (("aligned", None), ("cut", 777)):
            out[layout].append(tmp / ("%s%d.bam" % (layout, i)))
            bc.write_bam(out[layout][-1], records, block=block)
    out["empty"] = tmp / "empty.bam"
    bc.write_bam(out["empty"], [])
    out["unmapped"] = tmp / "unmapped.bam"
    bc.write_bam(out["unmapped"], [bc.rec(100 + k, n_cigar=0, pos=-1, flag=77, mapq=0, tid=-1, seed=k) for k in range(70)], block=777)
    whole = out["cut"][1].read_bytes()
    out["half"] = tmp / "half.bam"
    out["half"].write_bytes(whole[:len(whole) // 2])
    out["other"] = tmp / "other.bam"
    out["other"].write_bytes(bw.bgzf(b"CRAM" + bytes(100)))
    out["missing"] = tmp / "none.bam"
    flipped = bytearray(out["aligned"][1].read_bytes())
    at, hlen, clen = members(flipped)[1]  # (the first member of records)
    flipped[at + hlen + clen // 2] ^= 0x10
    out["flipped"] = tmp / "flipped.bam"
    out["flipped"].write_bytes(bytes(flipped))
    raw = [bc.record_bytes(as_record(k, r)) for k, r in enumerate(files[1])]
    l_seq, = struct.unpack_from("<i", raw[7], 20)
    raw[7] = raw[7][:20] + struct.pack("<i", l_seq + 500) + raw[7][24:]  # counts beyond the block; the writer makes the member's CRC of these bytes
    out["raised"] = tmp / "raised.bam"
    bc.write_bam(out["raised"], raw)
    return {k: [str(p) for p in v] if isinstance(v, list) else str(v) for k, v in out.items()}


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


def test_the_layouts_are_what_they_are_for(paths):
    """aligned: every member ends at a record's end; cut: members of 777 bytes end inside records"""
    for layout in ("aligned", "cut"):
        for path in paths[layout]:
            data = open(path, "rb").read()
            host = gtx.disc_bam_read(path)
            starts = {int(o) - 4 for o in host["offsets"]} | {len(host["stream"])}
            sizes = [len(zlib.decompress(data[at + h:at + h + c], -15)) for at, h, c in members(data)]
            header = sum(sizes) - len(host["stream"])
            ends = [int(e) - header for e in np.cumsum(sizes) if e > header]
            assert ends[-1] == len(host["stream"])
            if layout == "aligned":
                assert set(ends) <= starts
            else:
                assert len(ends) > 20 and len(set(ends) - starts) > 15


@pytest.mark.parametrize("layout", ["aligned", "cut"])
@pytest.mark.parametrize("params", [dict(), dict(n_threads=3), dict(n_threads=8), dict(first_event_cap=1, second_event_cap=1),
                                    dict(n_threads=3, first_event_cap=1, second_event_cap=1)], ids=str)
def test_the_device_front_gives_what_the_host_front_and_the_arrays_give(paths, layout, params):
    run, host, want = from_files(paths[layout], front="device", **params), from_files(paths[layout], **params), from_arrays(**params)
    assert outputs(run) == outputs(host) == outputs(want) and run["stats"] == host["stats"] == want["stats"]
    assert len(run["stats"]) == 3 and all(st["events"] > 0 for st in run["stats"]) and outputs(run) == outputs(from_arrays())
    for f in run["front"]:
        assert f["members_device"] == f["members"] > 0 and f["fell_back"] == 0 and f["segments_hit"] >= 1
        assert f["segments_rewalked"] == 0 if layout == "aligned" else f["segments_rewalked"] > 0


def test_front_0_is_the_host_front(paths):
    run, host = from_files(paths["cut"], front="host"), from_files(paths["cut"])
    assert outputs(run) == outputs(host) and run["stats"] == host["stats"]
    assert run["front"] == [dict(members=0, members_device=0, segments_hit=0, segments_rewalked=0, fell_back=0)] * 3
    with pytest.raises(gtx.GtxError) as e:
        from_files(paths["cut"], front=2)
    assert e.value.status == 1
    with pytest.raises(gtx.GtxError) as e:
        from_files(paths["cut"], front="device", device=-1)
    assert e.value.status == 2


def test_an_empty_file_and_a_file_of_unmapped_reads(paths):
    whole = from_files(paths["cut"], front="device")
    for n_threads in (1, 2):
        run = from_files(paths["cut"] + [paths["empty"], paths["unmapped"]], front="device", n_threads=n_threads)
        assert outputs(run) == outputs(whole) and run["stats"][:3] == whole["stats"] and [st["events"] for st in run["stats"][3:]] == [0, 0]
        assert [f["fell_back"] for f in run["front"]] == [0] * 5 and run["front"][4]["members_device"] == run["front"][4]["members"] > 1
    only = from_files([paths["empty"], paths["unmapped"], paths["empty"]], front="device", n_threads=3)
    assert only["text"] == ref.COLUMNS.encode() and len(only["variants"]) == 0 and len(only["good"]) == 0 and len(only["stats"]) == 3
    assert outputs(only) == outputs(from_files([paths["empty"], paths["unmapped"], paths["empty"]]))


@pytest.mark.parametrize("what", ["half", "other", "missing", "flipped", "raised"])
def test_a_file_that_is_not_sound_ends_the_call_as_the_host_front_does(paths, what):
    bad = paths[what]
    for n_threads in (1, 3):
        for files in ([paths["aligned"][0], bad, paths["cut"][2]], [bad, paths["cut"][0]]):
            with pytest.raises(gtx.GtxError) as want:
                from_files(files, n_threads=n_threads)
            with pytest.raises(gtx.GtxError) as got:
                from_files(files, front="device", n_threads=n_threads)
            assert got.value.status == want.value.status and bad in str(got.value) and str(got.value) == str(want.value)
    assert outputs(from_files(paths["cut"], front="device")) == outputs(from_arrays())  # and the library goes on


def test_the_first_failing_file_in_file_order(paths):
    with pytest.raises(gtx.GtxError) as e:
        from_files([paths["aligned"][0], paths["other"], paths["half"]], front="device", n_threads=3)
    assert e.value.status == 4 and paths["other"] in str(e.value)
