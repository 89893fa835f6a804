"""The unpack of a BAM record stream (include/gtx.h: gtx_disc_bam_unpack; kernel text graphtyper_amd/csrc/gtx_disc_bam_dev.hpp) held to
the plain definition of its three outputs, made here in numpy from the record FIELDS and never from the library: the plane rows
(the layout of gtx_pack_planes), the quality rows, the CIGAR words.  Hand-made record sets, each for one thing that can go wrong
(FACTS states what a set holds; tests/test_disc_bam_cases.py runs the facts), and judge(name, run): None, or how the outputs of the
program behind `run` differ -- shared by the emulation (tests/test_disc_bam_emu.py), the device (tests/test_gpu_disc_bam.py) and the
mutation audit (tests/disc_bam_mutants/), which asked for the sets names and far_cigar.  A set is a list of files; a file is its records and the strides it is unpacked with.  The record bytes, the
stream, the offsets and the gtx_disc_read table are written here too (SAM spec 4.2), so that what gtx_disc_bam_read returns can be
held to them (tests/test_disc_bam_read.py).  All values are bytes and words; there is no tolerance."""
import functools
import struct

import numpy as np

import bam_writer as bw
from graphtyper_amd import lib as gtx

GUARD = 64   # bytes in front of and behind every output
FILL = 0xA5  # what the outputs and their guards hold before the run
REFS = [("chrT", 1000000)]


def rec(l_seq=0, name="r", n_cigar=1, pos=100, flag=3, mapq=60, codes=None, qual=None, cigar=None, aux=b"", pad=15, seed=0, tid=0):
    """a record as its fields.  codes / qual / cigar default to `seed`'s random values; pad: the low nibble of an odd read's last byte"""
    rng = np.random.default_rng(1000 + seed)
    codes = [int(c) for c in (rng.integers(0, 16, l_seq) if codes is None else codes)]
    qual = [int(q) for q in (rng.integers(0, 256, len(codes)) if qual is None else qual)]
    cigar = [int(w) for w in (rng.integers(0, 1 << 32, n_cigar, dtype=np.uint64) if cigar is None else cigar)]
    assert len(qual) == len(codes)
    return dict(name=name, pos=pos, flag=flag, mapq=mapq, codes=codes, qual=qual, cigar=cigar, aux=bytes(aux), pad=pad, tid=tid)


def record_bytes(r):
    """the record in the file: block_size, the 32 fixed bytes, name and NUL, CIGAR words, 4-bit codes (the even base in the high nibble),
    qualities, aux data"""
    name = r["name"].encode() + b"\0"
    codes = r["codes"] + ([r["pad"]] if len(r["codes"]) % 2 else [])
    seq = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    body = struct.pack("<iiBBHHHIiii", r["tid"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(r["codes"]), -1, -1, 0)
    body += name + b"".join(struct.pack("<I", w) for w in r["cigar"]) + seq + bytes(r["qual"]) + r["aux"]
    return struct.pack("<i", len(body)) + body


class File:
    def __init__(self, records, plane_stride=None, qual_stride=None, waves=3):
        """strides: default the ones gtx_discover_files chooses; waves: the wavefronts the emulation runs the records over"""
        self.records, self.waves = records, waves
        longest = max([len(r["codes"]) for r in records] + [0])
        self.plane_stride = plane_stride or max(16, (longest + 31) // 32 * 16)
        self.qual_stride = qual_stride or max(4, (longest + 3) // 4 * 4)

    @functools.cached_property
    def tables(self):
        """-> (stream uint8, offsets uint32, reads DISC_READ, n_cigar): what gtx_disc_bam_read leaves for this file"""
        stream, offsets, reads, n_cigar = bytearray(), [], np.zeros(len(self.records), gtx.DISC_READ), 0
        for i, r in enumerate(self.records):
            offsets.append(len(stream) + 4)
            stream += record_bytes(r)
            reads[i] = (r["pos"], r["flag"], r["mapq"], 0, len(r["codes"]), len(r["cigar"]), n_cigar)
            n_cigar += len(r["cigar"])
        return np.frombuffer(bytes(stream), np.uint8), np.array(offsets, np.uint32), reads, n_cigar

    @functools.cached_property
    def expected(self):
        """the definition -> (planes uint8 (n, plane_stride), qual uint8 (n, qual_stride), cigar uint32)"""
        n = len(self.records)
        codes = np.zeros((n, 2 * self.plane_stride), np.uint8)
        qual = np.zeros((n, self.qual_stride), np.uint8)
        for i, r in enumerate(self.records):
            codes[i, :len(r["codes"])] = r["codes"]
            qual[i, :len(r["qual"])] = r["qual"]
        planes = np.zeros((n, self.plane_stride // 4), np.uint32)
        for b in range(4):  # word 4g + b: bit b of the codes of bases 32g .. 32g + 31, base 32g + j at bit j
            bits = ((codes >> b) & 1).astype(np.uint32).reshape(n, self.plane_stride // 16, 32)
            planes[:, b::4] = (bits << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)
        cigar = np.array([w for r in self.records for w in r["cigar"]], np.uint32)
        return planes.view(np.uint8).reshape(n, self.plane_stride), qual, cigar


# ---- the sets ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


def _lengths():
    return [File([rec(n, seed=k, name="len%d" % n) for k, n in enumerate(LENGTHS)]), File([rec(0, seed=1), rec(0, n_cigar=0, seed=2), rec(0, n_cigar=3, seed=3)])]


def _codes():
    """read s holds code (p + s) % 16 at base p: every code at every position; 128 bases end in a byte's low nibble, 127 in a high one,
    and the low nibble behind it, which is no base, is 15 and then 5"""
    return [File([rec(codes=[(p + s) % 16 for p in range(n)], pad=pad, seed=s) for s in range(16) for n, pad in ((128, 0), (127, 15), (127, 5))])]


def _shift():
    rng = np.random.default_rng(77)
    records = []
    for k in range(72):
        aux = bytes(rng.integers(0, 256, int(rng.integers(0, 10)), dtype=np.uint8)) if k != 71 else b""
        records.append(rec(29 + k % 5, name="n" * (k % 8), n_cigar=1 + k % 3, aux=aux, seed=k))
    return [File(records)]


CIGARS = (0, 1, 0, 63, 0, 64, 0, 0, 65, 200, 0)


def _cigars():
    return [File([rec(20 + k, n_cigar=n, seed=k) for k, n in enumerate(CIGARS)])]


def _quals():
    return [File([rec(257, qual=[255] + list(range(256)), seed=1), rec(256, qual=list(range(255, -1, -1)), seed=2), rec(3, qual=[255, 255, 255], seed=3)])]


COUNTS = (1, 63, 64, 65, 257)


def _counts():
    return [File([rec(5 + (7 * k) % 40, n_cigar=k % 4, name="c%d" % k, seed=k) for k in range(n)]) for n in COUNTS]


def _wide():
    records = [rec(33, seed=1), rec(70, seed=2), rec(1, seed=3), rec(0, seed=4)]
    return [File(records, plane_stride=96, qual_stride=131), File(records, plane_stride=48, qual_stride=70), File(records[2:], plane_stride=1024, qual_stride=1)]


NAMES = (127, 128, 129, 200, 255)  # l_read_name: the name's bytes and its NUL


def _names():
    """names whose length does not fit a signed byte, or seven bits; behind them everything at every residue again"""
    rng = np.random.default_rng(78)
    records = []
    for k in range(40):
        aux = bytes(rng.integers(0, 256, int(rng.integers(0, 10)), dtype=np.uint8))
        records.append(rec(29 + k % 5, name="m" * (NAMES[k % 5] - 1), n_cigar=1 + k % 3, aux=aux, seed=100 + k))
    return [File(records)]


FAR = (65535, 0, 1, 65, 65535, 2)


def _far_cigar():
    """CIGAR words at offsets that do not fit 16 bits, and 17"""
    return [File([rec(10 + k, n_cigar=n, seed=200 + k) for k, n in enumerate(FAR)])]


SETS = dict(lengths=_lengths, codes=_codes, shift=_shift, cigars=_cigars, quals=_quals, counts=_counts, wide=_wide, names=_names, far_cigar=_far_cigar)


@functools.lru_cache(maxsize=None)
def files(name):
    return SETS[name]()


# ---- what each set is for -----------------------------------------------------------------------------------------------------------
def starts(f):
    """per record the stream offsets of its CIGAR words, its codes and its qualities"""
    out = []
    for o, r in zip(f.tables[1], f.records):
        c = int(o) + 32 + len(r["name"]) + 1
        s = c + 4 * len(r["cigar"])
        out.append((c, s, s + (len(r["codes"]) + 1) // 2))
    return out


def facts_lengths(fs):
    assert tuple(len(r["codes"]) for r in fs[0].records) == LENGTHS and fs[0].plane_stride == 512 and fs[0].qual_stride == 1000
    assert max(len(r["codes"]) for r in fs[1].records) == 0 and (fs[1].plane_stride, fs[1].qual_stride) == (16, 4) and len(fs[1].expected[2]) == 4


def facts_codes(fs):
    seen = {(p % 64, c) for r in fs[0].records for p, c in enumerate(r["codes"])}
    assert seen == {(p, c) for p in range(64) for c in range(16)}
    last = {(len(r["codes"]) % 2, r["codes"][-1]) for r in fs[0].records}
    assert last == {(k, c) for k in (0, 1) for c in range(16)}  # every code in both nibbles of a read's last byte
    assert {r["pad"] for r in fs[0].records if len(r["codes"]) % 2} == {15, 5}  # and something that is no base behind an odd read


def facts_shift(fs):
    f = fs[0]
    assert {len(r["name"]) + 1 for r in f.records} == set(range(1, 9))
    for k in range(3):  # the words, the codes, the qualities: at every residue
        assert {s[k] % 4 for s in starts(f)} == set(range(4)) and {s[k] % 8 for s in starts(f)} == set(range(8))
    assert all(len(r["aux"]) == 0 for r in f.records[-1:]) and sum(1 for r in f.records if r["aux"]) > 40
    assert int(f.tables[1][-1]) + 32 + len(f.records[-1]["name"]) + 1 + 4 * len(f.records[-1]["cigar"]) + (len(f.records[-1]["codes"]) + 1) // 2 + len(f.records[-1]["codes"]) == len(f.tables[0])


def facts_cigars(fs):
    f = fs[0]
    assert tuple(len(r["cigar"]) for r in f.records) == CIGARS and {0, 1, 63, 64, 65, 200} == set(CIGARS)
    offs = f.tables[2]["cigar_off"].tolist()
    assert len(set(offs)) < len(offs) and offs[-1] == f.tables[3] == sum(CIGARS)  # cigar_off repeats; the last record's words would lie behind the array


def facts_quals(fs):
    assert fs[0].records[0]["qual"][0] == 255 and set(fs[0].records[0]["qual"]) == set(range(256))


def facts_counts(fs):
    assert tuple(len(f.records) for f in fs) == COUNTS and all(f.waves < len(f.records) or len(f.records) == 1 for f in fs)


def facts_wide(fs):
    longest = max(len(r["codes"]) for r in fs[0].records)
    assert fs[0].plane_stride > (longest + 31) // 32 * 16 + 16 and fs[0].qual_stride > longest + 4 and fs[0].qual_stride % 4
    assert (fs[1].plane_stride, fs[1].qual_stride) == ((longest + 31) // 32 * 16, longest)  # and the smallest that hold it
    assert fs[2].plane_stride == 1024 and fs[2].qual_stride == 1
    for f in fs:
        planes, qual, _ = f.expected
        assert not planes[:, (longest + 31) // 32 * 16:].any() and not qual[:, longest:].any()


def facts_names(fs):
    f = fs[0]
    stream, offsets = f.tables[0], f.tables[1]
    assert {int(stream[o + 8]) for o in offsets} == set(NAMES) and {len(r["name"]) + 1 for r in f.records} == set(NAMES)
    assert {len(r["cigar"]) for r in f.records} == {1, 2, 3} and {len(r["codes"]) for r in f.records} == {29, 30, 31, 32, 33}
    for n in NAMES:  # behind each length of name: the words, the codes, the qualities at every residue
        behind = [s for s, r in zip(starts(f), f.records) if len(r["name"]) + 1 == n]
        assert len(behind) == 8
    for k in range(3):
        assert {s[k] % 4 for s, r in zip(starts(f), f.records) if len(r["name"]) + 1 >= 128} == set(range(4)) and {s[k] % 4 for s in starts(f)} == set(range(4))
    assert min(NAMES) == 127 and {n - 256 if n > 127 else n for n in NAMES} != set(NAMES) and {n & 127 for n in NAMES} != set(NAMES)


def facts_far_cigar(fs):
    f = fs[0]
    assert tuple(len(r["cigar"]) for r in f.records) == FAR
    assert f.tables[2]["cigar_off"].tolist() == [0, 65535, 65535, 65536, 65601, 131136] and f.tables[3] == 131138 and 131136 > 1 << 17
    words = f.expected[2]
    assert len(words) * 4 < 1 << 20 and len({int(w) for w in words[[0, 65535, 65536, 65601, 131136, 131137]]}) == 6  # no two of the words a wrong offset would mix are equal
    for off in (65536, 65601, 131136):  # what an offset cut to 16 bits would write over, and with other words
        assert off & 0xFFFF != off and int(words[off]) != int(words[off & 0xFFFF])


FACTS = dict(lengths=facts_lengths, codes=facts_codes, shift=facts_shift, cigars=facts_cigars, quals=facts_quals, counts=facts_counts, wide=facts_wide,
             names=facts_names, far_cigar=facts_far_cigar)


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def guarded(n_bytes):
    """an output before the run: n_bytes of FILL between two guards"""
    return np.full(GUARD + n_bytes + GUARD, FILL, np.uint8)


def sizes(f):
    n = len(f.records)
    return n * f.plane_stride, n * f.qual_stride, 4 * f.tables[3]


def file_differs(f, got):
    """got: the three outputs as uint8 arrays with their guards, as guarded() made them and the run left them"""
    for what, out, want in zip(("the plane rows", "the quality rows", "the cigar words"), got, f.expected):
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        out = np.asarray(out, np.uint8)
        if len(out) != len(want) + 2 * GUARD:
            return "%s: %d bytes for %d" % (what, len(out) - 2 * GUARD, len(want))
        if (out[:GUARD] != FILL).any() or (out[GUARD + len(want):] != FILL).any():
            return "%s: a guard byte was written" % what
        wrong = np.flatnonzero(out[GUARD:GUARD + len(want)] != want)
        if len(wrong):
            at = int(wrong[0])
            return "%s: byte %d is %d for %d (%d bytes differ)" % (what, at, out[GUARD + at], want[at], len(wrong))
    return None


def judge(name, run):
    """None when the program behind `run` -- run(file) -> the three guarded outputs -- gives every file of the set `name` as the
    definition says, else what differs"""
    for k, f in enumerate(files(name)):
        how = file_differs(f, run(f))
        if how is not None:
            return "file %d: %s" % (k, how)
    return None


# ---- the emulation's files --------------------------------------------------------------------------------------------------------------
def write_case(path, f):
    """the input of tests/emu_disc_bam: uint32 n_reads, n_bytes, n_cigar, plane_stride, qual_stride, waves; the stream, the offsets, the
    gtx_disc_read table"""
    stream, offsets, reads, n_cigar = f.tables
    with open(path, "wb") as out:
        out.write(struct.pack("<6I", len(reads), len(stream), n_cigar, f.plane_stride, f.qual_stride, f.waves))
        out.write(stream.tobytes() + offsets.tobytes() + reads.tobytes())


def read_result(path, f):
    """what the program wrote -- the three outputs, each of exactly its size -- between guards of this module's making"""
    raw = np.fromfile(path, np.uint8)
    assert len(raw) == sum(sizes(f)), (len(raw), sizes(f))
    out, at = [], 0
    for n in sizes(f):
        g = guarded(n)
        g[GUARD:GUARD + n] = raw[at:at + n]
        out.append(g)
        at += n
    return out


def through(run, f):
    """run: emu_programs.run bound to a program and a directory"""
    return run(lambda path: write_case(path, f), lambda path: read_result(path, f))


# ---- the files on disk ------------------------------------------------------------------------------------------------------------------
def write_bam(path, records, header_text="@HD\tVN:1.6\n@RG\tID:g\tSM:sample\n", block=None):
    """the records (fields, or bytes as they are) as a BAM file; block: the file is cut into BGZF members of that many bytes wherever they
    fall, so that records straddle members"""
    raw = [r if isinstance(r, bytes) else record_bytes(r) for r in records]
    if block is None:
        bw.write_bam(str(path), REFS, header_text, raw)
        return
    head = b"BAM\1" + struct.pack("<i", len(header_text)) + header_text.encode() + struct.pack("<i", len(REFS))
    for name, length in REFS:
        head += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    with open(path, "wb") as out:
        out.write(bw.bgzf(head + b"".join(raw), block=block))
