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
-- shared by the emulation (tests/test_disc_bam_walk_emu.py), the device (tests/test_gpu_disc_bam_walk.py) and the mutation audit
(tests/disc_bam_walk_mutants/), which asked for the sets order, precedence, smallest, odd and turns.  The definition's second witness
is the host walk itself: tests/test_disc_bam_read.py puts every stream through gtx_disc_bam_read as a file.  What the cuts decide, the segments whose guess held and those walked again, follows from the definition's chain alone
(segments()).  All values are bytes and words; there is no tolerance."""
import bisect
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
        at = bisect.bisect_left(chain, b)  # (the chain ascends)
        if at == len(chain):
            continue
        entry = chain[at]
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


def full(k, l_seq=None, **more):
    """plain(k) without aux data: its counts fill its block"""
    return plain(k, l_seq, aux=b"", **more)


def one_over(record):
    """the record with a name one byte longer than its block has room for: counts one byte beyond the block"""
    return patched(record, l_read_name=record[12] + 1)


def past_end(records, i):
    """the records with the block word of record i one byte past the end of the stream they make"""
    return records[:i] + [patched(records[i], block=sum(len(r) for r in records[i:]) - 4 + 1)] + records[i + 1:]


def _order():
    """two bad records in one stream: the first in chain order is the one reported, whatever the second is and wherever the cuts fall"""
    def stream(recs, first, second, label):
        o = starts(recs)
        own = [("every record of the stream", o[1:-1]), ("between the two bad records", [o[first + 1]]), ("inside the first bad record", [o[first] + 17])]
        return Stream(b"".join(recs), own, label)
    near = past_end([plain(0), plain(1), plain(2), one_over(full(3)), plain(4), plain(5), plain(6)], 5)
    far = past_end([plain(0), plain(1), plain(2), one_over(full(3))] + [plain(k) for k in range(4, 75)], 73)
    long_first = [plain(0), plain(1), plain(2, l_seq=65536), plain(3), one_over(full(4)), plain(5)]
    long_last = [plain(0), plain(1), one_over(full(4)), plain(3), plain(2, l_seq=65536), plain(5)]
    return [stream(near, 3, 5, "counts beyond the block, two records on a block past the end"), stream(far, 3, 73, "the same pair 70 records apart"),
            stream(long_first, 2, 4, "65 536 bases in front of counts beyond the block"), stream(long_last, 2, 4, "counts beyond the block in front of 65 536 bases")]


def _precedence():
    """l_seq beyond 65 535 in a record whose counts exceed its block: MALFORMED; in one that holds its bases: LONG_READ"""
    out = []
    for l_seq in (65536, 0x7FFFFFFF):
        recs = [plain(0), plain(1), patched(plain(2), l_seq=l_seq), plain(3), plain(4)]
        out.append(Stream(b"".join(recs), [("inside the bad record", [starts(recs)[2] + 21])], "l_seq %d in a block of %d bytes" % (l_seq, len(recs[2]) - 4)))
    recs = [plain(0), plain(1), plain(2, l_seq=65536), plain(3), plain(4)]
    out.append(Stream(b"".join(recs), [("inside the bad record", [starts(recs)[2] + 21])], "65 536 bases that are there"))
    return out


def least(k):
    """the smallest sound record: block 32, no name, no cigar word, no base -- 36 bytes, with fields of its own"""
    pos = -1 if k % 5 == 4 else (0x00F00000 + k * 0x01010101) & 0x7FFFFFFF  # (all four bytes of pos differ from record to record)
    return struct.pack("<iiiBBHHHiiii", 32, 0, pos, 0, k % 61, 4680, 0, (k * 41 + 1) & 0xFFFF, 0, -1, -1, 0)


def _smallest():
    between = [plain(0), least(1), plain(2), least(3), least(4), plain(5)]
    out = [Stream(least(0), label="alone"), Stream(b"".join(between), [("every record of the stream", starts(between)[1:-1])], "between ordinary records")]
    for n in (64, 65):
        data = b"".join(least(k) for k in range(n))
        out.append(Stream(data, [("every byte of it", range(1, len(data)))], "a run of %d" % n))
    return out


ODD = (1, 3, 65535)


def _odd():
    """an odd l_seq whose counts fill the block to the byte, and the same one byte over"""
    out = []
    for l_seq in ODD:
        for over in (False, True):
            bad = full(2, l_seq=l_seq, n_cigar=2)
            recs = [plain(0), plain(1), one_over(bad) if over else bad, plain(3)]
            out.append(Stream(b"".join(recs), [("inside it", [starts(recs)[2] + 9])], "l_seq %d, counts %s" % (l_seq, "one byte over" if over else "that fill the block")))
    return out


TURNS = (63, 64, 65, 127, 128)  # the bad record's number: lane 63 of a turn, lanes 0 and 1 of the next, and the same a turn on
BAD = (TRUNCATED, MALFORMED, LONG_READ)


def _turns():
    """one bad record at the seam of two turns of 64, between two sound records whose counts would show in the totals if they leaked"""
    out = []
    for at in TURNS:
        for status in BAD:
            recs = [plain(k) for k in range(at - 1)] + [plain(at - 1, l_seq=200, n_cigar=1000)]
            bad = {TRUNCATED: plain(at), MALFORMED: one_over(full(at, l_seq=400, n_cigar=7)), LONG_READ: plain(at, l_seq=65536, n_cigar=9)}[status]
            recs += [bad, plain(at + 1, l_seq=300, n_cigar=3000), plain(at + 2), plain(at + 3)]
            if status == TRUNCATED:
                recs = past_end(recs, at)
            o = starts(recs)
            own = [("every record of the stream", o[1:-1]), ("one record in front of the bad one", [o[at - 1]]), ("one byte into the bad one", [o[at] + 1]),
                   ("one byte into the first record", [1])]
            out.append(Stream(b"".join(recs), own, "record %d is bad (%d)" % (at, status)))
    return out


SETS = dict(align=_align, straddle=_straddle, span=_span, resync=_resync, decoy=_decoy, counts=_counts, damage=_damage, order=_order, precedence=_precedence,
            smallest=_smallest, odd=_odd, turns=_turns)


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


def fields(data, o):
    """-> (block, l_read_name, n_cigar, l_seq, the counts' sum) of the record at o"""
    block, = struct.unpack_from("<i", data, o)
    l_read_name, n_cigar, l_seq = data[o + 12], struct.unpack_from("<H", data, o + 16)[0], struct.unpack_from("<i", data, o + 20)[0]
    return block, l_read_name, n_cigar, l_seq, 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def alone(data, o):
    """the status of the record at o, were it the stream's first"""
    return define(data[o:])["status"] if define(data[o:])["n_reads"] == 0 else OK


def facts_order(ss):
    near, far, long_first, long_last = ss
    for s, apart in ((near, 2), (far, 70)):
        every = own(s, "every record of the stream")
        first, second = s.want["bad_at"], every[2 + apart]
        assert (s.want["status"], s.want["n_reads"]) == (MALFORMED, 3) and first == every[2]
        block, _, _, _, total = fields(s.data, first)
        assert total == block + 1 and first + 4 + block == every[3]  # one byte beyond a block that is sound: the chain goes on behind it
        assert second + 4 + fields(s.data, second)[0] == len(s.data) + 1 and alone(s.data, second) == TRUNCATED
        assert all(alone(s.data, o) == OK for o in every[3:2 + apart])  # sound records between the two
        assert own(s, "between the two bad records") == [every[3]] and first < own(s, "inside the first bad record")[0] < every[3]
        assert (s.want["n_cigar"], s.want["max_l_seq"]) == (sum(fields(s.data, o)[2] for o in [0] + every[:2]), max(fields(s.data, o)[3] for o in [0] + every[:2]))
    assert 2 < 3 + 2 < 64 < 3 + 70  # the pair in one turn of 64 records, and in two
    for s, (a, b) in ((long_first, (LONG_READ, MALFORMED)), (long_last, (MALFORMED, LONG_READ))):
        every = own(s, "every record of the stream")
        assert (s.want["status"], s.want["n_reads"], s.want["bad_at"]) == (a, 2, every[1]) and (alone(s.data, every[1]), alone(s.data, every[3])) == (a, b)
        assert alone(s.data, every[2]) == OK and own(s, "between the two bad records") == [every[2]]


def facts_precedence(ss):
    for s, l_seq in zip(ss, (65536, 0x7FFFFFFF, 65536)):
        o = s.want["chain"][2]
        block, _, _, got, total = fields(s.data, o)
        assert got == l_seq > 65535 and o == s.want["bad_at"] and s.want["n_reads"] == 2 and o + 4 + block < len(s.data)
        assert (s.want["status"], total > block) == ((MALFORMED, True) if s is not ss[2] else (LONG_READ, False))
        assert o < own(s, "inside the bad record")[0] < o + 4 + block


def facts_smallest(ss):
    assert len(least(0)) == 36 and fields(least(0), 0) == (32, 0, 0, 0, 32) and len({least(k)[4:] for k in range(65)}) == 65
    pos = [struct.unpack_from("<i", least(k), 8)[0] for k in range(65)]
    assert min(pos) == -1 and max(pos) > 1 << 24 and len({p & 0xFFFF for p in pos}) > 50 and len({p >> 16 for p in pos}) > 50  # pos beyond 16 bits, and none
    assert [s.want["status"] for s in ss] == [OK] * 4 and [s.want["n_reads"] for s in ss] == [1, 6, 64, 65]
    assert ss[0].data == least(0) and dict(ss[0].cut_lists)["every byte"] == list(range(1, 36))
    assert sorted(fields(ss[1].data, o)[0] for o in ss[1].want["chain"][:-1])[:3] == [32, 32, 32] and fields(ss[1].data, 0)[0] > 32 < fields(ss[1].data, ss[1].want["chain"][-2])[0]
    for s in ss[2:]:
        assert s.want["chain"] == list(range(0, len(s.data) + 1, 36)) and own(s, "every byte of it") == list(range(1, len(s.data)))
        assert segments(s.data, own(s, "every byte of it"))[:2] == (s.want["n_reads"], 0)  # every record start is a cut: nothing is walked again


def facts_odd(ss):
    assert len(ss) == 6
    for k, l_seq in enumerate(ODD):
        fits, over = ss[2 * k], ss[2 * k + 1]
        o = fits.want["chain"][2]
        assert over.want["chain"][-1] == o and (fits.want["status"], fits.want["n_reads"]) == (OK, 4) and (over.want["status"], over.want["n_reads"]) == (MALFORMED, 2)
        a, b = fields(fits.data, o), fields(over.data, o)
        assert a[3] == b[3] == l_seq and l_seq % 2 == 1 and a[4] == a[0] == b[0] and b[4] == b[0] + 1  # to the byte, and one byte over: half a byte less and it fits
        assert 32 + b[1] + 4 * b[2] + l_seq // 2 + l_seq == b[0]


def facts_turns(ss):
    assert [(s.want["bad_at"] == s.want["chain"][-1], s.want["n_reads"], s.want["status"]) for s in ss] == [(True, at, status) for at in TURNS for status in BAD]
    assert {at % 64 for at in TURNS} == {63, 0, 1} and {at // 64 for at in TURNS} == {0, 1, 2} and max(TURNS) - 1 > 64  # (and a segment walked again over more than a turn)
    for s in ss:
        every, at = [0] + own(s, "every record of the stream"), s.want["n_reads"]
        front, bad, behind = (fields(s.data, every[k]) for k in (at - 1, at, at + 1))
        assert alone(s.data, every[at - 1]) == alone(s.data, every[at + 1]) == OK and alone(s.data, every[at]) == s.want["status"]
        assert front[3] == s.want["max_l_seq"] == 200 < behind[3] == 300 and front[2] == 1000 and behind[2] == 3000  # what leaks from behind is larger than all in front
        assert s.want["n_cigar"] == 1000 + sum(k % 4 for k in range(at - 1)) and int(s.want["reads"]["cigar_off"][-1]) == s.want["n_cigar"] - 1000
        assert s.want["status"] == TRUNCATED or (bad[2] > 0 and bad[3] > 200)  # a bad record that is parsed has counts that would show, too
        assert own(s, "one record in front of the bad one") == [every[at - 1]] and own(s, "one byte into the bad one") == [every[at] + 1]
        assert len(every) == at + 4 and segments(s.data, own(s, "one byte into the first record")) == (1, 1, 0)  # one walk again of all but the first record


FACTS = dict(align=facts_align, straddle=facts_straddle, span=facts_span, resync=facts_resync, decoy=facts_decoy, counts=facts_counts, damage=facts_damage,
             order=facts_order, precedence=facts_precedence, smallest=facts_smallest, odd=facts_odd, turns=facts_turns)


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
