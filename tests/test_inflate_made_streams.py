"""Both DEFLATE decoders -- the host's (gtx_inflate.hpp, through gtx_inflate_raw and, under ASan / UBSan, tests/sanitize/inflate_driver)
and the device's source (gtx_inflate_dev.hpp, through the emulation tests/emu_inflate under ASan / UBSan) -- held to streams
zlib's encoder never writes: the members of tests/deflate_maker.py, an encoder that is told the structure it writes (deep codes
whatever the frequencies, forced header shapes, repeats across the alphabets, 48-bit tokens, block ends on the device's batch
of 64, stored headers at every bit), its members with one rule of RFC 1951 broken each, and streams recorded from libdeflate
(tests/golden/libdeflate_streams.bin).  The yardstick is zlib's inflate and nothing of the project: the corpus fixture asserts
that zlib takes every valid member to exactly the maker's bytes and refuses every invalid one BEFORE a decoder of the project
sees any.  No member is filtered out: what the maker makes for the seeds is what the decoders get.  The device:
test_gpu_inflate_made_streams.py."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import bam_writer as bw
import deflate_maker as dm
import emu_programs
import inflate_corpus as ic
from graphtyper_amd import lib as gtx

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = range(128)        # sixteen members of each of the maker's eight themes: the smallest range that meets test_coverage_conditions with a handful to spare
INVALID_SEEDS = range(3)  # every broken rule three times, behind lead blocks of different lengths
HEADER_RULES = {"oversubscribed_litlen", "oversubscribed_dist", "oversubscribed_cl", "incomplete_litlen", "incomplete_dist", "incomplete_cl", "one_symbol_cl", "no_end_of_block",
                "hlit_287", "hlit_288", "hdist_31", "hdist_32", "first_length_is_16", "repeat_past_total"}


def made_corpus():
    """(valid: [(name, data, stream, facts or None)], invalid: [(kind, stream, out_len, status or None, reason)]), every one held to
    zlib here"""
    valid = [("seed %d" % s,) + dm.member(s) for s in SEEDS]
    valid += [("largest tables %d" % s,) + dm.largest_tables_member(s) for s in range(5)]
    valid += [("libdeflate %s level %d" % (name, level), data, stream, None) for name, level, data, stream in ic.recorded_libdeflate()]
    for name, data, stream, _ in valid:
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == data and d.eof and d.unused_data == b"", "the maker's own fault: %s" % name
    invalid = [m for s in INVALID_SEEDS for m in dm.invalid_members(s)]
    for kind, stream, out_len, _, reason in invalid:
        assert ic.zlib_verdict(stream, out_len) is None, "the maker's own fault: zlib takes the member that is to break '%s'" % reason
    return valid, invalid


@pytest.fixture(scope="module")
def corpus():
    return made_corpus()


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """(the emulation of the device decoder, the host decoder's driver), both under ASan / UBSan"""
    d = tmp_path_factory.mktemp("inflate_drivers")
    emu, host = emu_programs.build("emu_inflate", d), str(d / "inflate_driver")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "sanitize"), "-s", "INFLATE_OUT=" + host, host])
    return emu, host


def test_corpus_is_whole(corpus):
    valid, invalid = corpus
    assert len(valid) == len(SEEDS) + 5 + 32 and len(invalid) == len(INVALID_SEEDS) * len(dm.INVALID_KINDS)
    assert {name.split(" level")[0] for name, _, _, f in valid if f is None} >= {"libdeflate bam_records", "libdeflate acgt", "libdeflate empty"}


def test_coverage_conditions(corpus):
    """what the corpus holds, from the maker's facts (conditions, not measurements: the corpus is fixed by its seeds): each shape
    the decoders' deep parts need, in at least five valid members"""
    valid, invalid = corpus
    facts = [f for _, _, _, f in valid if f is not None]

    def members(cond):
        return sum(1 for f in facts if cond(f))
    held = {
        "a 15-bit literal / length code": members(lambda f: f["max_lit_bits"] == 15),
        "a 15-bit distance code": members(lambda f: f["max_dist_bits"] == 15),
        "a distance code of 9 .. 15 bits used by a token": members(lambda f: 9 <= f["max_dist_bits_used"] <= 15),
        "a 15-bit distance code used by a token": members(lambda f: f["max_dist_bits_used"] == 15),
        "a 7-bit code-length code": members(lambda f: f["max_cl_bits"] == 7),
        "a 48-bit token": members(lambda f: f["max_token_bits"] == 48),
        "HLIT == 286": members(lambda f: f["hlit_286"]),
        "HDIST == 30": members(lambda f: f["hdist_30"]),
        "a repeat across the alphabets": members(lambda f: f["repeat_across"]),
        "a 16 on zeros": members(lambda f: f["rep16_on_zero"]),
        "a block ending on token 64": members(lambda f: f["block_end_on_batch"]),
        "a match fed by a match of the same batch": members(lambda f: f["match_fed_by_match"]),
        "length 258 as symbol 285": members(lambda f: f["len258_as_285"]),
        "length 258 as 284 + 31": members(lambda f: f["len258_as_284"]),
        "distance 32 768": members(lambda f: f["dist_32768"]),
        "distance equal to the output so far": members(lambda f: f["dist_is_output"]),
        "a one-symbol distance code that is used": members(lambda f: f["single_dist_code"]),
        "a distance alphabet without a symbol": members(lambda f: f["no_dist_code"]),
        "a literal alphabet of end-of-block alone": members(lambda f: f["eob_only_code"]),
        "an empty stored block": members(lambda f: ("stored", 0) in f["blocks"]),
        "output of 0 bytes": members(lambda f: f["out_len"] == 0),
        "output of 1 byte": members(lambda f: f["out_len"] == 1),
        "output of 65 536 bytes": members(lambda f: f["out_len"] == 65536),
        "the codes with the largest second-level tables (deflate_maker.LARGEST_TABLES)": members(lambda f: f["theme"] == "largest_tables"),
    }
    for k in range(8):
        held["a stored header at bit %d" % k] = members(lambda f: k in f["stored_offsets"])
    print("\n".join("%4d  %s" % (n, what) for what, n in held.items()))
    print("%d valid members, %d bytes inflated, %d tokens" % (len(valid), sum(len(d) for _, d, _, _ in valid), sum(f["tokens"] for f in facts)))
    assert {what: n for what, n in held.items() if n < 5} == {}
    # token counts of a block: on, just before and just behind the device's batch
    counts = {n for f in facts for kind, n in f["blocks"] if kind != "stored"}
    assert {0, 1, 63, 64, 65, 128} <= counts
    assert {kind for kind, _, _, _, _ in invalid} == set(dm.INVALID_KINDS) and HEADER_RULES <= set(dm.INVALID_KINDS)
    assert all(status == dm.BAD_STREAM for kind, _, _, status, _ in invalid if kind in HEADER_RULES)


def test_host_decoder(corpus):
    """gtx_inflate_raw: every valid member to the expected bytes -- the host refuses none, so none is left to zlib (build_table's
    `cap`: DESIGN 4.9) --, every invalid member refused"""
    valid, invalid = corpus
    for name, data, stream, _ in valid:
        assert gtx.inflate_raw(stream, len(data)) == data, name
    for kind, stream, out_len, _, reason in invalid:
        with pytest.raises(gtx.GtxError):
            gtx.inflate_raw(stream, out_len)
            pytest.fail("taken: " + reason)


def _members(streams, out_lens, crcs):
    blob, where = ic.pack(streams)
    return blob, [(off, n, 0, out_len, crc) for (off, n), out_len, crc in zip(where, out_lens, crcs)]


def test_both_decoders_under_sanitizers(corpus, drivers, tmp_path):
    """one case file for both drivers: every member in heap blocks of exactly its sizes (the host's input with the 8 bytes its
    header demands)"""
    emu, host = drivers
    valid, invalid = corpus
    data = [d for _, d, _, _ in valid]
    blob, members = _members([s for _, _, s, _ in valid], [len(d) for d in data], [zlib.crc32(d) for d in data])
    for driver in (emu, host):
        st, out = ic.run_emu(driver, tmp_path, members, blob, mode=0)
        refused = [valid[i][0] for i in range(len(valid)) if st[i] != ic.OK]
        assert refused == [], "valid members refused by %s: %s" % (os.path.basename(driver), refused)
        assert out == b"".join(data)
    wrong = [m[:4] + (m[4] ^ 0x8000,) for m in members]
    for driver in (emu, host):
        st, out = ic.run_emu(driver, tmp_path, wrong, blob, mode=0)
        assert (st == ic.CRC).all() and out == b"".join(data)
    # the invalid members: a header rule is "not a valid stream", a size names its direction, nothing else than the three
    blob, members = _members([s for _, s, _, _, _ in invalid], [n for _, _, n, _, _ in invalid], [0] * len(invalid))
    st, _ = ic.run_emu(emu, tmp_path, members, blob, mode=0, check_crc=False)
    for i, (kind, _, _, status, reason) in enumerate(invalid):
        assert st[i] in (ic.BAD_STREAM, ic.SHORT, ic.LONG), reason
        assert status is None or st[i] == status, (reason, int(st[i]))
    st, _ = ic.run_emu(host, tmp_path, members, blob, mode=0, check_crc=False)
    assert (st == 1).all(), [invalid[i][4] for i in np.nonzero(st != 1)[0]]


def test_emulated_batch_with_refused_members_between(corpus, drivers, tmp_path):
    """the batch as the device entry point takes it (test_batch_odd_offsets_outputs_back_to_back): streams at odd offsets, outputs
    back to back behind a margin, an invalid member behind every second valid one; the fill outside every member's range stays"""
    emu, _ = drivers
    valid, invalid = corpus
    rng = np.random.default_rng(8)
    picks = []
    for k, v in enumerate(valid):
        picks.append((v[2], len(v[1]), zlib.crc32(v[1]), v[1]))
        if k % 2:
            kind, stream, out_len, _, _ = invalid[(k // 2) % len(invalid)]
            picks.append((stream, out_len, 0, None))
    blob, where = ic.pack([p[0] for p in picks], rng)
    margin, gap, at, members = 77, 5, 77, []
    for (off, n), (_, out_len, crc, _) in zip(where, picks):
        members.append((off, n, at, out_len, crc))
        at += out_len + (gap if len(members) % 3 == 0 else 0)  # (most outputs touch their neighbours; some have fill between)
    out_size = at + margin
    st, out = ic.run_emu(emu, tmp_path, members, blob, mode=1, out_size=out_size, fill=0x5A)
    out = np.frombuffer(out, np.uint8)
    outside = np.ones(out_size, bool)
    for m, (_, _, _, data) in zip(members, picks):
        outside[m[2]:m[2] + m[3]] = False
    assert len(out) == out_size and (out[outside] == 0x5A).all()
    for k, (m, (_, _, _, data)) in enumerate(zip(members, picks)):
        if data is None:
            assert st[k] in (ic.BAD_STREAM, ic.SHORT, ic.LONG), k
        else:
            assert st[k] == ic.OK and out[m[2]:m[2] + m[3]].tobytes() == data, k


def made_deflate(seed):
    """deflate for tests/bam_writer.py by the maker: the bytes as the literals and matches of a few blocks with deep codes"""
    r = dm.Rand("bgzf", seed)

    def deflate(chunk):
        facts = dm.new_facts()
        o, w = dm.Output(r, len(chunk), facts), dm.BitWriter()
        cuts = sorted({r.below(len(chunk) + 1) for _ in range(r.below(4))} | {len(chunk)})
        at = 0
        for cut in cuts:
            tokens = []
            while at < cut:
                # the longest match at one of a few distances (the bytes are given here: the maker's tokens have to spell them;
                # a match that runs into itself compares through the chunk, which is the output so far)
                best = (0, 0)
                for dist in ((1, 2, 76, 151, 233, r.between(1, min(at, 32768))) if at else ()):
                    n = 0
                    while dist <= at and n < 258 and at + n < cut and chunk[at + n] == chunk[at + n - dist]:
                        n += 1
                    best = max(best, (n, dist))
                if best[0] >= 3:
                    tokens.append(o.match(*dm.len_token(best[0], alt258=r.chance(0.5)), *dm.dist_token(best[1])))
                    at += best[0]
                else:
                    tokens.append(o.literal(chunk[at]))
                    at += 1
            knobs = dict(deep=r.pick([0.3, 1.0]), deep_cl=r.pick([0.0, 1.0]), deep_dist=r.pick([0.5, 1.0]), hlit_286=r.chance(0.3), hdist_30=r.chance(0.3), pin_dist=True)
            if r.chance(0.2):
                dm.fixed_block(w, tokens, cut == len(chunk), facts)
            else:
                dm.dynamic_block(r, w, tokens, cut == len(chunk), knobs, facts)
            if cut != len(chunk) and r.chance(0.3):
                dm.stored_block(w, b"", False, facts)
                o.flush()
        assert bytes(o.out) == chunk
        return w.bytes()
    return deflate


def _records(seed, n):
    rng = np.random.default_rng(seed)
    recs = [(int(p), rng.choice([1, 2, 4, 8], size=150).astype(np.uint8)) for p in np.sort(rng.integers(0, 399000, size=n))]
    return [bw.record("r%d" % i, 0, 0, p, 60, [("M", 150)], -1, -1, 0, c, [("AS", "C", 100)]) for i, (p, c) in enumerate(recs)]


def bam_of_made_members(made, plain, seed=3, n=900, block=2500):
    """the same BAM records in two files: `plain` as tests/bam_writer.py writes it with zlib, `made` with the same bytes cut every
    `block` bytes (records run from member to member) and deflated by the maker.  Returns (records, members of `made`, its bytes inflated)"""
    bw.write_bam(plain, [("chrA", 400000)], "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:400000\n", _records(seed, n))
    raw, at, out = open(plain, "rb").read(), 0, b""
    while at < len(raw):
        size = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        out += zlib.decompress(raw[at:at + size], 31)
        at += size
    made_raw = bw.bgzf(out, block=block, deflate=made_deflate(seed))
    open(made, "wb").write(made_raw)
    # zlib first: the members are sound gzip members that hold the file's bytes
    at, back, members = 0, b"", 0
    while at < len(made_raw):
        size = int.from_bytes(made_raw[at + 16:at + 18], "little") + 1
        back += zlib.decompress(made_raw[at:at + size], 31)
        at += size
        members += 1
    assert back == out and out[:4] == b"BAM\1", "the maker's own fault"
    return n, members, out


def test_bam_of_made_members_reads_on_the_host(tmp_path):
    """the file the device test reads (test_gpu_inflate_made_streams.py), here through the host path against the same records in
    a file zlib deflated"""
    made, plain = str(tmp_path / "made.bam"), str(tmp_path / "plain.bam")
    n, members, _ = bam_of_made_members(made, plain)
    assert members > 80
    got = []
    for path in (made, plain):
        reads = gtx.Reads([path])
        r, s = reads.next(n + 10, seq_stride=160)
        reads.close()
        got.append((r.copy(), s.copy()))
    assert len(got[0][0]) == n
    assert all((got[0][0][f] == got[1][0][f]).all() for f in gtx.STREAM_RECORD.names) and got[0][1].tobytes() == got[1][1].tobytes()
