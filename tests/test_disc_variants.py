"""gtx_disc_variants and gtx_disc_vcf_sites (include/gtx.h) through the C ABI on a gtx_disc made without a device: every case set of
tests/disc_variants_cases.py equals the plain restatement of the reference's text (tests/disc_variants_ref.py) field for field and
byte for byte; the capacity protocol (exact, one short, zero: the sizes are written and nothing else); words that do not parse and
records that reach behind their arrays are GTX_ERR_ARG; the sort's last key and the duplicate rule on records handed over directly;
and the loop closed -- the text of two sets behind a header and gtx_bgzf_compress goes through gtx_graph_from_files and gives the
graph that gtx_graph_build makes of the same records handed over directly.  No GPU is needed.  The same file under the sanitizers:
test_disc_variants_emu.py."""
import ctypes as C

import numpy as np
import pytest

import disc_variants_cases as vc
import disc_variants_ref as ref
from graphtyper_amd import lib as gtx
from oracle_lib import _p

OK, ERR_ARG, ERR_CAPACITY = 0, 1, 5


@pytest.mark.parametrize("name", sorted(vc.SETS))
def test_every_set_equals_the_restatement(name):
    for k, case in enumerate(vc.cases(name)):
        assert vc.differs(case, vc.through_lib(case)) is None, k


def variants_call(h, words, bits, n_recs, n_letters, n_ids):
    """gtx_disc_variants into arrays of these capacities, filled with 0xA5 -> (status, the three sizes, the three arrays)"""
    L = gtx.lib()
    recs, letters, ids = (np.full(max(n, 1), 0xA5, np.uint8).view(np.uint8).repeat(size).view(dtype)
                          for n, size, dtype in ((n_recs, gtx.DISC_VARIANT.itemsize, gtx.DISC_VARIANT), (n_letters, 1, np.uint8), (n_ids, 4, np.uint32)))
    n, nl, ni = C.c_uint32(77), C.c_uint64(77), C.c_uint64(77)
    rc = L.gtx_disc_variants(h, _p(words), len(words), _p(bits), _p(recs) if n_recs else None, n_recs, C.byref(n), _p(letters) if n_letters else None, n_letters,
                             C.byref(nl), _p(ids) if n_ids else None, n_ids, C.byref(ni))
    return rc, (n.value, nl.value, ni.value), (recs, letters, ids)


def untouched(arrays):
    return all((a.view(np.uint8) == 0xA5).all() for a in arrays)


@pytest.mark.parametrize("name", ["sets", "first_base", "many"])
def test_the_capacity_protocol(name):
    """exact sizes: GTX_OK; any one of the three one short, and all zero with NULL arrays: GTX_ERR_CAPACITY, the sizes written, no
    other byte; the text the same"""
    L = gtx.lib()
    case = vc.cases(name)[-1 if name != "first_base" else 3]
    a, h = vc.arrays(case), vc.host_handle(case)
    try:
        want_recs, want_letters, want_ids = vc.record_arrays(vc.expected(case)["recs"])
        sizes = (len(want_recs), len(want_letters), len(want_ids))
        assert all(sizes)
        rc, got, arrays = variants_call(h, a["words"], a["bits"], *sizes)
        assert (rc, got) == (OK, sizes) and arrays[0][:sizes[0]].tobytes() == want_recs.tobytes() and arrays[2][:sizes[2]].tolist() == want_ids.tolist()
        for short in range(3):
            caps = [s - (k == short) for k, s in enumerate(sizes)]
            rc, got, arrays = variants_call(h, a["words"], a["bits"], *caps)
            assert (rc, got) == (ERR_CAPACITY, sizes) and untouched(arrays), short
        rc, got, arrays = variants_call(h, a["words"], a["bits"], 0, 0, 0)
        assert (rc, got) == (ERR_CAPACITY, sizes) and untouched(arrays)
        text = vc.expected(case)["text"]
        args = (_p(want_recs), len(want_recs), _p(np.frombuffer(want_letters, np.uint8)), len(want_letters), _p(want_ids), len(want_ids), case.contig.encode())
        for cap, status in ((len(text), OK), (len(text) + 5, OK), (len(text) - 1, ERR_CAPACITY), (0, ERR_CAPACITY)):
            buf, n = np.full(max(cap, 1), 0xA5, np.uint8), C.c_uint64(77)
            assert L.gtx_disc_vcf_sites(*args, _p(buf) if cap else None, cap, C.byref(n)) == status and n.value == len(text)
            assert (buf[:len(text)].tobytes() == text and (buf[len(text):] == 0xA5).all()) if status == OK else untouched([buf])
    finally:
        L.gtx_disc_destroy(h)


def test_an_empty_result_and_no_words():
    L = gtx.lib()
    case = vc.cases("dropped")[6]  # every event is a dropped indel
    h = vc.host_handle(case)
    try:
        for words in (vc.arrays(case)["words"], np.zeros(0, np.uint32), np.zeros(2, np.uint32)):
            rc, got, arrays = variants_call(h, words, None, 0, 0, 0)
            assert (rc, got) == (OK, (0, 0, 0)) and untouched(arrays)
        n = C.c_uint64()
        buf = np.zeros(64, np.uint8)
        assert L.gtx_disc_vcf_sites(None, 0, None, 0, None, 0, b"chrT", _p(buf), 64, C.byref(n)) == OK and buf[:n.value].tobytes() == ref.COLUMNS.encode()
    finally:
        L.gtx_disc_destroy(h)


def test_words_that_do_not_parse_and_null_arguments():
    L = gtx.lib()
    case = vc.cases("sets")[0]
    words, h = vc.arrays(case)["words"], vc.host_handle(case)
    try:
        def status(w, handle=h):
            return variants_call(handle, np.ascontiguousarray(w, np.uint32), None, 64, 256, 64)[0]
        assert status(words) == OK
        for cut in range(1, len(words)):  # every cut of the stream
            assert status(words[:cut]) == ERR_ARG, cut
        assert status(np.concatenate([words, [0]])) == ERR_ARG  # a word behind the end
        n_table = int(words[0])
        assert n_table == 2
        bad = words.copy()
        bad[2] = ord("X")  # an SNP in the indel table
        assert status(bad) == ERR_ARG
        bad = words.copy()
        bad[2] = ord("Q")  # no such kind
        assert status(bad) == ERR_ARG
        first_event = next(i for i in range(len(words) - 2) if words[i] == case.haps[0][0][0] and words[i + 1] == ord("X") and i > 30)
        bad = words.copy()
        bad[first_event] = case.region_begin + len(case.reference)  # an SNP behind the region's last base (the reference asserts)
        assert status(bad) == ERR_ARG and b"outside the region" in L.gtx_last_error()
        two = vc.words_of((), [((10, "X", "AC"), (), ())])  # an SNP of two letters
        assert status(two) == ERR_ARG
        n, nl, ni = C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert L.gtx_disc_variants(None, _p(words), len(words), None, None, 0, C.byref(n), None, 0, C.byref(nl), None, 0, C.byref(ni)) == ERR_ARG
        assert L.gtx_disc_variants(h, None, len(words), None, None, 0, C.byref(n), None, 0, C.byref(nl), None, 0, C.byref(ni)) == ERR_ARG
        assert L.gtx_disc_variants(h, _p(words), len(words), None, None, 0, None, None, 0, C.byref(nl), None, 0, C.byref(ni)) == ERR_ARG
        assert L.gtx_disc_variants(h, _p(words), len(words), None, None, 4, C.byref(n), None, 0, C.byref(nl), None, 0, C.byref(ni)) == ERR_ARG
    finally:
        L.gtx_disc_destroy(h)


def record(pos, kind, ref_off, ref_len, alt_off, alt_len, gt_id, hap=(0, 0), anti=(0, 0)):
    r = np.zeros(1, gtx.DISC_VARIANT)
    r[0] = (pos, gt_id, ref_off, ref_len, alt_off, alt_len, hap[0], hap[1], anti[0], anti[1], ord(kind), (0, 0, 0))
    return r


def test_records_handed_over_directly():
    """what no map can hold: records equal in all but the number of INFO keys (more keys first), equal in everything (they keep their
    order: this library's rule), a duplicate in position and alleles (not written; the next record's suffix looks at it); a record that
    reaches behind the letters or the ids is GTX_ERR_ARG"""
    L = gtx.lib()
    letters, ids = b"ACAG", np.array([7, 8, 9], np.uint32)
    plain, with_anti, with_both = record(9, "X", 0, 1, 1, 1, 1), record(9, "X", 0, 1, 1, 1, 2, anti=(0, 1)), record(9, "X", 0, 1, 1, 1, 3, hap=(1, 1), anti=(2, 1))
    other = record(9, "X", 2, 1, 3, 1, 4)  # A > G
    text = gtx.disc_vcf_sites(np.concatenate([plain, other, with_anti, with_both]), letters, ids, "c").decode().split("\n")[1:-1]
    # sorted: with_both, with_anti, plain (equal alleles: the second and third are duplicates of the one in front and are not written), other
    assert text == ["c\t10\tc:10:SG\tA\tC\t0\t.\tGT_ANTI_HAPLOTYPE=9;GT_HAPLOTYPE=8;GT_ID=3", "c\t10\tc:10:SG.0\tA\tG\t0\t.\tGT_ID=4"]
    a, b = record(5, "I", 0, 1, 0, 2, 1), record(5, "I", 0, 1, 0, 2, 2)
    assert gtx.disc_vcf_sites(np.concatenate([a, b]), letters, ids, "c").decode().split("\n")[1:-1] == ["c\t6\tc:6:IG\tA\tAC\t0\t.\tGT_ID=1"]
    assert gtx.disc_vcf_sites(np.concatenate([b, a]), letters, ids, "c").decode().split("\n")[1:-1] == ["c\t6\tc:6:IG\tA\tAC\t0\t.\tGT_ID=2"]
    n = C.c_uint64()
    lb = np.frombuffer(letters, np.uint8)
    for wrong in (record(1, "X", 4, 1, 0, 1, 1), record(1, "X", 0, 5, 0, 1, 1), record(1, "X", 0, 1, 3, 2, 1), record(1, "X", 0, 1, 0xFFFFFFFF, 2, 1),
                  record(1, "X", 0, 1, 1, 1, 1, hap=(3, 1)), record(1, "X", 0, 1, 1, 1, 1, anti=(0, 4)), record(1, "X", 0, 1, 1, 1, 1, anti=(0xFFFFFFFF, 2))):
        assert L.gtx_disc_vcf_sites(_p(wrong), 1, _p(lb), len(lb), _p(ids), len(ids), b"c", None, 0, C.byref(n)) == ERR_ARG
    assert L.gtx_disc_vcf_sites(_p(plain), 1, _p(lb), len(lb), _p(ids), len(ids), None, None, 0, C.byref(n)) == ERR_ARG
    assert L.gtx_disc_vcf_sites(_p(plain), 1, _p(lb), len(lb), _p(ids), len(ids), b"c", None, 0, None) == ERR_ARG


@pytest.mark.parametrize("name", ["dropped", "sets"])
def test_the_sites_file_goes_back_into_a_graph(tmp_path, name):
    """iteration 2 reads what iteration 1 wrote: the text of gtx_disc_vcf_sites behind gtx_vcf_header's header, compressed by
    gtx_bgzf_compress, through gtx_graph_from_files -- the graph equals the one gtx_graph_build makes of the same records handed over
    directly, with the events lib.parse_events reads off GT_ID and GT_ANTI_HAPLOTYPE"""
    for k, case in enumerate(vc.cases(name)):
        got = vc.through_lib(case)
        contig_len = case.region_begin + len(case.reference)
        header = gtx.vcf_header("20260101", "test", [(case.contig, contig_len)], [])
        vz = tmp_path / ("%s_%d.vcf.gz" % (name, k))
        vz.write_bytes(gtx.bgzf_compress((header if isinstance(header, bytes) else header.encode()) + got["text"][got["text"].index(b"\n") + 1:]))
        fa = tmp_path / ("%s_%d.fa" % (name, k))
        fa.write_text(">%s\n%s%s\n" % (case.contig, "N" * case.region_begin, case.reference))
        region = "%s:%d-%d" % (case.contig, case.region_begin + 1, contig_len)
        from_file, span = gtx.graph_from_files(fa, vz, region)
        assert span == (case.region_begin, contig_len)
        lines = [ln.split("\t") for ln in got["text"].decode().split("\n")[1:-1]]
        records = [(int(c[1]) - 1, c[3], [c[4]], c[7]) for c in lines]
        assert len(records) == len(vc.expected(case)["recs"]) and (len(records) > 0 or k == 6)
        direct = gtx.graph_from_records(case.reference, records, region_begin=case.region_begin, region_end=contig_len, extend_prefix=True)
        assert set(from_file) == set(direct) and all(np.array_equal(from_file[key], direct[key]) for key in direct), k
        if records:
            assert len(direct["var_order"]) > 0 and len(direct["event_val"]) >= 2 * len(records)
