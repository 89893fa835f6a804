"""The record sets of tests/disc_bam_cases.py hold what they are for, the definition of the three outputs agrees with the library's
host repack where the two overlap (gtx_pack_planes: the plane rows), and the judge tells a right output from a wrong one.  No device."""
import numpy as np
import pytest

import disc_bam_cases as bc
from graphtyper_amd import lib as gtx


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_the_set_holds_what_it_is_for(name):
    bc.FACTS[name](bc.files(name))


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_the_plane_rows_of_the_definition_are_those_of_the_host_repack(name):
    """two statements of one layout: the definition's words from the record fields, gtx_pack_planes from the nibble rows"""
    gtx.build()
    for f in bc.files(name):
        n = len(f.records)
        seq = np.zeros((n, f.plane_stride), np.uint8)
        for i, r in enumerate(f.records):
            codes = r["codes"] + [0] * (len(r["codes"]) % 2)
            seq[i, :len(codes) // 2] = [(codes[j] << 4) | codes[j + 1] for j in range(0, len(codes), 2)]
        planes = np.zeros((n, f.plane_stride), np.uint8)
        gtx.check(gtx.lib().gtx_pack_planes(seq.ctypes.data, f.plane_stride, n, planes.ctypes.data, f.plane_stride))
        assert np.array_equal(planes, f.expected[0])


def perfect(f):
    out = []
    for n, want in zip(bc.sizes(f), f.expected):
        g = bc.guarded(n)
        g[bc.GUARD:bc.GUARD + n] = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        out.append(g)
    return out


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_the_judge_passes_the_definition_and_nothing_else(name):
    assert bc.judge(name, perfect) is None

    def spoiled(which, at):
        def run(f):
            out = perfect(f)
            out[which][at] ^= 1
            return out
        return run
    for which in range(3):
        assert "guard" in bc.judge(name, spoiled(which, 0)) and "guard" in bc.judge(name, spoiled(which, -1))
    assert "plane rows" in bc.judge(name, spoiled(0, bc.GUARD)) and "quality rows" in bc.judge(name, spoiled(1, bc.GUARD))
    assert bc.judge(name, lambda f: [g[:-1] for g in perfect(f)]).endswith("bytes for %d" % bc.sizes(bc.files(name)[0])[0])


def test_the_stream_is_the_records_as_they_lie():
    f = bc.files("shift")[0]
    stream, offsets, reads, n_cigar = f.tables
    assert stream.tobytes() == b"".join(bc.record_bytes(r) for r in f.records) and n_cigar == sum(len(r["cigar"]) for r in f.records)
    for o, r, d in zip(offsets, f.records, reads):
        assert int(stream[o + 8]) == len(r["name"]) + 1 and int(d["l_qseq"]) == len(r["codes"]) and int(d["n_cigar"]) == len(r["cigar"])
