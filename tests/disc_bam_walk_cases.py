"""The record walk of a BAM record stream on the device (include/gtx.h: gtx_disc_bam_walk; kernel text
graphtyper_amd/csrc/gtx_disc_bam_walk_dev.hpp) held to its definition, stated here in plain Python over the stream's bytes: define().
The definition knows no segments, no wavefronts and nothing of the library -- it is the host walk of gtx_disc_bam.cpp.

  o = 0.  A record begins with its block_size word at o.  o == n_bytes: the stream ends, OK.  Fewer than 4 bytes left, block < 32 as a
  signed 32-bit value, o + 4 + block > n_bytes: TRUNCATED at o.  l_seq < 0 or 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq >
  block: MALFORMED at o; else l_seq > 65 535: LONG_READ at o.  A sound record i is offsets[i] = o + 4 and reads[i] = (pos, flag, mapq, 0,
  l_seq, n_cigar, the sum of n_cigar in front of it); the next o is o + 4 + block.  Nothing behind the first bad record is reported; the
  records in front of it are, with their counts.

Hand-made streams, each with the cut lists it is walked with -- none, every record start, every 777 bytes, every byte of a short
stream, and the lists the set is made for --, in sets that each stand for one thing that can go wrong (FACTS states what a set holds;
tests/test_disc_bam_walk_cases.py runs the facts), and judge(name, run): None, or how the results of the program behind `run` differ
-- shared by the emulation (tests/test_disc_bam_walk_emu.py), the device (tests/test_gpu_disc_bam_walk.py) and a later mutation
audit.  What the cuts decide, the segments whose guess held and those walked again, follows from the definition's chain alone
(segments()).  All values are bytes and words; there is no tolerance."""
import functools
import struct

import numpy as np

import disc_bam_cases as bc
from graphtyper_amd import lib as gtx

OK, TRUNCATED, MALFORMED, LONG_READ = 0, 1, 2, 3
GUARD = 64   # bytes in front of and behind each table
FILL = 0xA5  # what the tables and their guards hold before the run
SHORT = 1000  # a stream of at most that many bytes is also cut at every byte


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def define(stream):
    """-> dict(status, bad_at, n_reads, n_cigar, max_l_seq, offsets [uint32], reads [DISC_READ], chain [every o the walk stood at, the
    bad one or n_bytes last])"""
    stream = bytes(stream)
    n, o, offsets, reads, n_cigar, longest, chain = len(stream), 0, [], [], 0, 0, []
    status, bad_at = OK, 0
    while True:
        chain.append(o)
        if o == n:
            break
        if n - o < 4:
            status, bad_at = TRUNCATED, o
            break
        block, = struct.unpack_from("<i", stream, o)
        if block < 32 or o + 4 + block > n:
            status, bad_at = TRUNCATED, o
            break
        _, pos, l_read_name, mapq, _, cigars, flag, l_seq = struct.unpack_from("<iiBBHHHi", stream, o + 4)
        if l_seq < 0 or 32 + l_read_name + 4 * cigars + (l_seq + 1) // 2 + l_seq > block:
            status, bad_at = MALFORMED, o
            break
        if l_seq > 65535:
            status, bad_at = LONG_READ, o
            break
        offsets.append(o + 4)
        reads.append((pos, flag, mapq, 0, l_seq, cigars, n_cigar & 0xFFFFFFFF))
        n_cigar += cigars
        longest = max(longest, l_seq)
        o += 4 + block
    table = np.zeros(len(reads), gtx.DISC_READ)
    for i, r in enumerate(reads):
        table[i] = r
    return dict(status=status, bad_at=bad_at, n_reads=len(reads), n_cigar=n_cigar, max_l_seq=longest, offsets=np.array(offsets, np.uint32), reads=table, chain=chain)


def segments(stream, cuts):
    """what the cuts decide, from the definition's chain: -> (hit, rewalked, spanned).  A segment's true entry is the chain's first o at
    or behind its start; it is hit where that is its start, spanned where that lies at or behind its end, walked again otherwise;
    behind the bad record there is no chain and a segment is none of the three."""
    chain = define(stream)["chain"]
    n = len(bytes(stream))
    if n == 0:
        return 0, 0, 0
    hit = rewalked = spanned = 0
    bounds = [0] + list(cuts) + [n]
    for b, e in zip(bounds[:-1], bounds[1:]):
        entry = next((o for o in chain if o >= b), None)
        if entry is None:
            continue
        if entry >= e:
            spanned += 1
        elif entry == b:
            hit += 1
        else:
            rewalked += 1
    return hit, rewalked, spanned


# ---- streams and their cut lists ------------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, data, own=(), label=""):
        """data: the bytes; own: the cut lists the stream is made for, as (name, [offsets])"""
        self.data, self.label = bytes(data), label
        self.own = [(name, self.valid(cuts)) for name, cuts in own]

    def valid(self, cuts):
        return sorted({int(c) for c in cuts if 0 < c < len(self.data)})

    @functools.cached_property
    def want(self):
        return define(self.data)

    @functools.cached_property
    def cut_lists(self):
        """[(name, [offsets])]: strictly ascending offsets in (0, n_bytes)"""
        n = len(self.data)
        out = [("none", []), ("every record start", self.valid(self.want["chain"])), ("every 777 bytes", self.valid(range(777, n, 777)))]
        if n <= SHORT:
            out.append(("every byte", self.valid(range(1, n))))
        return out + self.own


def starts(records):
    """the o of each record of a stream made of `records` (bytes each), and the stream's length last"""
    out, o = [], 0
    for r in records:
        out.append(o)
        o += len(r)
    return out + [o]


def patched(record, **fields):
    """a record's bytes with fields of its front overwritten: block (int32 at 0), l_read_name (byte at 12), n_cigar (uint16 at 16), l_seq
    (int32 at 20)"""
    b = bytearray(record)
    for name, value in fields.items():
        at, fmt = dict(block=(0, "<i"), l_read_name=(12, "<B"), n_cigar=(16, "<H"), l_seq=(20, "<i"))[name]
        struct.pack_into(fmt, b, at, value)
    return bytes(b)


def plain(k, l_seq=None, **more):
    """record k of a run of ordinary records: 20 .. 60 bases, zero to three cigar words, names and aux data of mixed length"""
    rng = np.random.default_rng(500 + k)
    aux = bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8))
    fields = dict(name="q%d" % k + "n" * (k % 7), n_cigar=k % 4, pos=1000 + 3 * k, flag=(k * 37) & 0xFFFF, mapq=k % 61, aux=aux, seed=k)
    fields.update(more)
    return bc.record_bytes(bc.rec(20 + (11 * k) % 41 if l_seq is None else l_seq, **fields))


def decoy(block, l_read_name=1, n_cigar=0, l_seq=0):
    """36 bytes that read as a record's front: a block_size word and 32 fixed bytes"""
    return struct.pack("<iiiBBHHHiiii", block, 0, 77, l_read_name, 9, 4680, n_cigar, 5, l_seq, -1, -1, 0)


def _align():
    recs = [plain(k) for k in range(40)]
    o = starts(recs)
    return [Stream(b"".join(recs), [("every third record", o[3:-1:3]), ("the second record alone", o[1:2]), ("the last record alone", o[-2:-1])], "40 records")]


def _straddle():
    recs = [plain(k) for k in range(12)]
    o = starts(recs)
    at = o[5]
    own = [("o + %d" % d, [at + d]) for d in (1, 2, 3, 4, 5, 12, 20, 35)]
    own.append(("all of them", [at + d for d in (1, 2, 3, 4, 5, 12, 20, 35)]))
    own.append(("in every record's block word", [x + 1 + k % 3 for k, x in enumerate(o[1:-1])]))
    return [Stream(b"".join(recs), own, "12 records")]


def _span():
    recs = [plain(0), plain(1), plain(2, l_seq=3000, n_cigar=9), plain(3), plain(4)]
    o = starts(recs)
    inside = [o[2] + d for d in (10, 700, 1400, 2100, 2800, 3500)]
    own = [("six cuts inside the long record", inside), ("and its own start and end", [o[2]] + inside + [o[3]]), ("and a cut in the record behind it", inside + [o[3] + 9])]
    return [Stream(b"".join(recs), own, "a record of 3 000 bases among four short ones")]


def _resync():
    recs = [plain(k) for k in range(30)]
    o = starts(recs)
    own = [("two misses, a hit, three misses, a hit", [o[4] + 5, o[7] + 33, o[9], o[12] + 1, o[13] + 2, o[14] + 3, o[20]]),
           ("misses up to the last record", [x + 7 for x in o[1:-2]] + [o[-2]])]
    return [Stream(b"".join(recs), own, "30 records")]


def _decoy():
    """records whose aux data read as records; a cut stands at each decoy's first byte"""
    d_two = decoy(32 + 1) + b"\0" + decoy(32 + 1 + 8, n_cigar=2) + b"\0" + bytes(8)  # two sound records that end where the carrier ends
    d_big, d_neg = decoy(0x7FFFFFFF), decoy(-16)
    d_lseq = decoy(32 + 1 + 60, l_seq=0x7FFFFFFF) + bytes(61)                        # a sound block whose l_seq is 2^31 - 1
    d_last = struct.pack("<i", 0x7FFFFFFF)                                           # the stream's last four bytes
    recs, decoys = [], []
    for k, d in enumerate((d_two, d_big, d_neg, d_lseq)):
        recs += [plain(2 * k), plain(2 * k + 1, aux=d)]
        decoys.append(sum(len(r) for r in recs) - len(d))
    recs += [plain(20), plain(21, aux=d_last)]
    n = sum(len(r) for r in recs)
    decoys.append(n - 4)
    o = starts(recs)
    own = [("at every decoy", decoys), ("at every decoy and every record start", decoys + o[1:-1]), ("at every decoy and the record behind the first", decoys + [o[2]]),
           ("two bytes in front of the end", decoys + [n - 2]), ("one byte in front of the end", [n - 1])]
    return [Stream(b"".join(recs), own, "five decoys")]


COUNTS = (0, 1, 64, 65, 257)


def _counts():
    out = [Stream(b"".join(plain(k) for k in range(n)), label="%d records" % n) for n in COUNTS]
    big = [plain(0), plain(1, n_cigar=65535), plain(2, n_cigar=0, name=""), plain(3, name="x" * 254), plain(4, l_seq=0), plain(5, l_seq=65535), plain(6)]
    o = starts(big)
    out.append(Stream(b"".join(big), [("inside the large records", [o[1] + 70000, o[1] + 200000, o[5] + 50000])], "65 535 cigar words, names of 1 and 255 bytes, 0 and 65 535 bases"))
    out.append(Stream(b"".join([plain(0), plain(1), plain(2, l_seq=65536), plain(3)]), label="65 536 bases"))
    return out


def _damage():
    recs = [plain(k) for k in range(8)]
    o = starts(recs)
    whole = b"".join(recs)
    bare = plain(30, aux=b"")  # (its counts fill its block)
    out = [Stream(whole[:o[7] + k], label="the stream ends %d bytes into a block word" % k) for k in (1, 2, 3)]
    for block in (31, 0, -1):
        out.append(Stream(b"".join(recs[:4] + [patched(recs[4], block=block)] + recs[5:]), label="block %d" % block))
    out.append(Stream(b"".join(recs[:7] + [patched(recs[7], block=len(recs[7]) - 4 + 1)]), label="a block one byte past the end"))
    out.append(Stream(b"".join(recs[:3] + [patched(bare, l_read_name=bare[12] + 1)] + recs[3:]), label="counts one byte beyond the block"))
    out.append(Stream(b"".join(recs[:3] + [patched(recs[3], l_seq=-1)] + recs[4:]), label="l_seq -1"))
    two = recs[:2] + [patched(bare, l_read_name=bare[12] + 1)] + recs[2:5] + [patched(recs[5], l_seq=-1)] + recs[6:]
    out.append(Stream(b"".join(two), [("a cut in front of each", [starts(two)[2], starts(two)[6]])], "two damaged records"))
    # damage that only a wrong guess sees: aux data whose first word is no block
    guess = recs[:3] + [plain(40, aux=struct.pack("<i", 5) + bytes(40))] + recs[3:]
    at = starts(guess)[4] - 44
    out.append(Stream(b"".join(guess), [("at the damage", [at]), ("at the damage and behind it", [at, starts(guess)[5]])], "damage only a wrong guess sees"))
    # damage that only the true chain sees: a decoy in front of a record of l_seq -1 jumps over it, and the segment ends behind the jump's start
    tail = [patched(recs[4], l_seq=-1)] + recs[5:]
    jump = len(tail[0]) + len(tail[1]) + 32 + 1  # from behind the decoy's block word to the third record behind it
    true = recs[:3] + [plain(41, aux=decoy(jump) + b"\0")] + tail
    t = starts(true)
    at = t[4] - 37
    assert at + 4 + jump == t[6]
    out.append(Stream(b"".join(true), [("a segment from the decoy into the damaged record", [at, t[4] + 10]), ("the decoy alone", [at])], "damage only the true chain sees"))
    return out


SETS = dict(align=_align, straddle=_straddle, span=_span, resync=_resync, decoy=_decoy, counts=_counts, damage=_damage)


@functools.lru_cache(maxsize=None)
def streams(name):
    return SETS[name]()


def own(s, name):
    return dict(s.own)[name]


# ---- what each set is for -----------------------------------------------------------------------------------------------------------
def facts_align(ss):
    s, = ss
    assert s.want["status"] == OK and s.want["n_reads"] == 40
    for name, cuts in s.cut_lists:
        if name not in ("every 777 bytes", "none"):
            assert len(cuts) > 0 and segments(s.data, cuts) == (len(cuts) + 1, 0, 0), name
    assert segments(s.data, own(s, "every third record"))[0] == 14


def facts_straddle(ss):
    s, = ss
    o = s.want["chain"][5]
    assert [own(s, "o + %d" % d) for d in (1, 2, 3, 4)] == [[o + 1], [o + 2], [o + 3], [o + 4]] and own(s, "o + 35")[0] < o + 36 < s.want["chain"][6]
    for name, cuts in s.own[:8]:
        assert segments(s.data, cuts) == (1, 1, 0), name  # the one cut is missed
    assert segments(s.data, own(s, "all of them")) == (1, 1, 7)  # the segments between the cuts lie inside the record
    assert segments(s.data, own(s, "in every record's block word")) == (1, 10, 1)  # (no record begins behind the last cut)


def facts_span(ss):
    s, = ss
    assert s.want["max_l_seq"] == 3000 and s.want["n_reads"] == 5
    assert segments(s.data, own(s, "six cuts inside the long record")) == (1, 1, 5)       # five segments lie wholly inside the record
    assert segments(s.data, own(s, "and its own start and end")) == (3, 0, 6)
    assert segments(s.data, own(s, "and a cut in the record behind it")) == (1, 2, 5)


def facts_resync(ss):
    s, = ss
    assert segments(s.data, own(s, "two misses, a hit, three misses, a hit")) == (3, 5, 0)
    cuts = own(s, "misses up to the last record")
    assert segments(s.data, cuts) == (2, len(cuts) - 2, 1)  # (the last miss ends at the hit: no record begins in it)


def facts_decoy(ss):
    s, = ss
    want, decoys = s.want, own(s, "at every decoy")
    assert want["status"] == OK and want["n_reads"] == 10 and len(decoys) == 5 and not set(decoys) & set(want["chain"])
    guess = [define(s.data[d:]) for d in decoys]  # what a walk from each decoy meets
    assert guess[0]["status"] == OK and guess[0]["n_reads"] >= 2 and decoys[0] + guess[0]["chain"][2] == want["chain"][2]  # two sound records whose exit is a record start
    assert decoys[0] + guess[0]["chain"][2] in own(s, "at every decoy and the record behind the first")
    assert [(g["status"], g["n_reads"]) for g in guess[1:]] == [(TRUNCATED, 0), (TRUNCATED, 0), (MALFORMED, 0), (TRUNCATED, 0)]
    assert struct.unpack_from("<i", s.data, decoys[1])[0] == 0x7FFFFFFF and struct.unpack_from("<i", s.data, decoys[2])[0] < 0
    assert struct.unpack_from("<i", s.data, decoys[3] + 20)[0] == 0x7FFFFFFF and decoys[4] == len(s.data) - 4
    assert segments(s.data, decoys) == (1, 4, 1)  # every segment that begins at a decoy is walked again or holds no record
    assert segments(s.data, own(s, "at every decoy and every record start")) == (10, 0, 5)  # ... or, cut at the carrier's end, is spanned


def facts_counts(ss):
    assert tuple(s.want["n_reads"] for s in ss[:5]) == COUNTS and len(ss[0].data) == 0 and all(s.want["status"] == OK for s in ss[:6])
    r = ss[5].want["reads"]
    assert {0, 65535} <= set(r["n_cigar"].tolist()) and {0, 65535} <= set(r["l_qseq"].tolist()) and ss[5].want["max_l_seq"] == 65535
    assert {ss[5].data[o + 8] for o in ss[5].want["offsets"].tolist()} >= {1, 255}
    assert int(r["cigar_off"][-1]) == ss[5].want["n_cigar"] - int(r["n_cigar"][-1]) > 65535
    assert (ss[6].want["status"], ss[6].want["n_reads"], ss[6].want["bad_at"]) == (LONG_READ, 2, ss[6].want["chain"][2])
    assert len(ss[3].want["chain"]) > 2 * 4 * 4 and len(ss[1].cut_lists[1][1]) == 0  # more segments than the wavefronts of a block or two, and one segment


def facts_damage(ss):
    got = [(s.label, s.want["status"], s.want["n_reads"]) for s in ss]
    assert [g[1:] for g in got[:3]] == [(TRUNCATED, 7)] * 3 and all(len(s.data) - s.want["bad_at"] in (1, 2, 3) for s in ss[:3])
    assert [g[1:] for g in got[3:6]] == [(TRUNCATED, 4)] * 3
    assert got[6][1:] == (TRUNCATED, 7) and got[7][1:] == (MALFORMED, 3) and got[8][1:] == (MALFORMED, 3)
    two = ss[9]
    assert (two.want["status"], two.want["n_reads"]) == (MALFORMED, 2) and two.want["bad_at"] == own(two, "a cut in front of each")[0]
    assert define(two.data[own(two, "a cut in front of each")[1]:])["status"] == MALFORMED  # the second one is damaged as well
    guess = ss[10]
    assert guess.want["status"] == OK and guess.want["n_reads"] == 9 and define(guess.data[own(guess, "at the damage")[0]:])["status"] == TRUNCATED
    true = ss[11]
    at, end = own(true, "a segment from the decoy into the damaged record")
    seen = define(true.data[at:])
    assert seen["status"] == OK and at + seen["chain"][1] > end > true.want["bad_at"] > at  # the guess jumps out of its segment over the damaged record
    assert (true.want["status"], true.want["n_reads"]) == (MALFORMED, 4)


FACTS = dict(align=facts_align, straddle=facts_straddle, span=facts_span, resync=facts_resync, decoy=facts_decoy, counts=facts_counts, damage=facts_damage)


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def guarded(n_bytes):
    """a table before the run: n_bytes of FILL between two guards"""
    return np.full(GUARD + n_bytes + GUARD, FILL, np.uint8)


def differs(s, cuts, got):
    """got: dict(status, bad_at, n_reads, n_cigar, max_l_seq, segments_hit, segments_rewalked, offsets, reads) -- the two tables as
    uint8 arrays of n_reads entries between guards, as guarded() made them and the run left them"""
    want = s.want
    for key in ("status", "bad_at", "n_reads", "n_cigar", "max_l_seq"):
        if int(got[key]) != int(want[key]) and not (key == "bad_at" and want["status"] == OK):
            return "%s is %d for %d" % (key, got[key], want[key])
    hit, rewalked, _ = segments(s.data, cuts)
    if (int(got["segments_hit"]), int(got["segments_rewalked"])) != (hit, rewalked):
        return "%d segments hit and %d walked again for %d and %d" % (got["segments_hit"], got["segments_rewalked"], hit, rewalked)
    for what in ("offsets", "reads"):
        table = np.ascontiguousarray(want[what]).view(np.uint8).reshape(-1)
        out = np.asarray(got[what], np.uint8)
        if len(out) != len(table) + 2 * GUARD:
            return "%s: %d bytes for %d" % (what, len(out) - 2 * GUARD, len(table))
        if (out[:GUARD] != FILL).any() or (out[GUARD + len(table):] != FILL).any():
            return "%s: a guard byte was written" % what
        wrong = np.flatnonzero(out[GUARD:GUARD + len(table)] != table)
        if len(wrong):
            at = int(wrong[0])
            return "%s: byte %d is %d for %d (%d bytes differ)" % (what, at, out[GUARD + at], table[at], len(wrong))
    return None


def judge(name, run):
    """None when the program behind `run` -- run(stream bytes, [cut list]) -> one result per cut list -- walks every stream of the set
    `name` with every one of its cut lists as the definition says, else what differs"""
    for k, s in enumerate(streams(name)):
        lists = s.cut_lists
        for (label, cuts), got in zip(lists, run(s.data, [cuts for _, cuts in lists])):
            how = differs(s, cuts, got)
            if how is not None:
                return "stream %d (%s), cuts %s: %s" % (k, s.label, label, how)
    return None


# ---- the emulation's files --------------------------------------------------------------------------------------------------------------
OUT = np.dtype([("status", np.uint32), ("max_l_seq", np.uint32), ("bad_at", np.uint64), ("n_cigar", np.uint64), ("n_reads", np.uint32), ("segments_hit", np.uint32),
                ("segments_rewalked", np.uint32), ("reserved", np.uint32)])
assert OUT.itemsize == 40


def write_case(path, data, lists, waves):
    """the input of tests/emu_disc_bam_walk: uint32 n_bytes, n_lists, waves; the stream; per list uint32 n_cuts and the cuts"""
    with open(path, "wb") as out:
        out.write(struct.pack("<3I", len(data), len(lists), waves) + data)
        for cuts in lists:
            out.write(struct.pack("<I", len(cuts)) + np.array(cuts, np.uint32).tobytes())


def read_result(path, n_lists):
    """what the program wrote -- per list gtx_bam_walk_out, n_reads offsets, n_reads gtx_disc_read, the tables of exactly that size --
    with the tables between guards of this module's making"""
    raw, at, out = np.fromfile(path, np.uint8), 0, []
    for _ in range(n_lists):
        head = raw[at:at + 40].view(OUT)[0]
        got = {k: int(head[k]) for k in OUT.names}
        at += 40
        for what, size in (("offsets", 4), ("reads", 16)):
            n = got["n_reads"] * size
            g = guarded(n)
            g[GUARD:GUARD + n] = raw[at:at + n]
            got[what] = g
            at += n
        out.append(got)
    assert at == len(raw), (at, len(raw))
    return out


def through(run, waves, data, lists):
    """run: emu_programs.run bound to a program and a directory"""
    return run(lambda path: write_case(path, data, lists, waves), lambda path: read_result(path, len(lists)))
