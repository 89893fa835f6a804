"""Case sets for the discovery events kernel (graphtyper_amd/csrc/gtx_disc_events_dev.hpp): the smallest shapes at which the walk
over a read's CIGAR can go wrong.  A set is a list of parts; a part is one region with its reads (one launch).  What a set is for
is asserted from the restatement's output (tests/disc_events_ref.py) by its entry in FACTS: no set filters or skips a case.

    parts(name)     -> [Part]                                  (made once)
    expected(name)  -> per part, per read (state, n_events, pos_end, [event tuples]) by the restatement, under the one stated
                       exception (a deletion of more than 65 535 bases is no event)
    arrays(part)    -> the arrays of gtx_disc_events_batch for a part (numpy)
    write_case / read_result: the files of tests/emu_disc_events
An event tuple: (pos, seq, len, type, hq, max_distance, reserved) -- gtx_disc_event without `read`."""
import functools
import struct

import numpy as np

import disc_events_ref as ref
from graphtyper_amd import lib as gtx

NT16 = "=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(NT16)}
OPS = {c: i for i, c in enumerate("MIDNSHP=XB")}
LENGTHS = (1, 31, 32, 33, 64, 65, 100)
BIG_BEGIN = (1 << 31) - (1 << 20)


class Part:
    def __init__(self, reference, region_begin, reads, stride=None, fill=0, event_cap=None):
        """reads: [dict(pos, cigar [words], seq, qual [ints])]; stride: bytes of a plane row (default: the smallest that holds the longest
        read); fill: the BAM code of every base of a row behind its read's l_qseq"""
        self.reference, self.region_begin, self.reads, self.fill = reference, region_begin, reads, fill
        self.stride = stride or max(16, (max([len(r["seq"]) for r in reads] + [1]) + 31) // 32 * 16)
        self.event_cap = event_cap


def cig(*ops):
    """(operation, count) pairs -> BAM words; an operation is a letter or its code"""
    return [(n << 4) | (OPS[o] if isinstance(o, str) else o) for o, n in ops]


def rd(pos, cigar, seq, qual=30):
    return dict(pos=pos, cigar=cigar, seq=seq, qual=[qual] * len(seq) if isinstance(qual, int) else list(qual), flag=3, mapq=60)


def rand_ref(n, seed):
    return "".join("ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def mutate(s, at):
    s = list(s)
    for i in at:
        s[i] = other(s[i])
    return "".join(s)


# ---- the sets -----------------------------------------------------------------------------------------------------------------
REF_BYTES = "ACGTNRYacgt-*\x00"
CODE_OFFSETS = (0, 31, 32, 33)


def _codes():
    out = []
    for n, byte in enumerate(REF_BYTES):
        base = list(rand_ref(40, 100 + n))
        for o in CODE_OFFSETS:
            base[o] = byte
        reads = []
        for code in range(16):
            for o in CODE_OFFSETS:
                seq = ["A" if c not in "ACGT" else c for c in base]
                seq[o] = NT16[code]
                reads.append(rd(500, cig(("M", 40)), "".join(seq)))
        out.append(Part("".join(base), 500, reads))
    return out


def _edge_places(read_mod, ref_off, span):
    """the block's first and last base, and bits 31 and 0 of either side's groups"""
    return sorted({0, span - 1} | {k for k in range(span) if (read_mod + k) % 32 in (31, 0) or (ref_off + k) % 32 in (31, 0)})


def _group_edges():
    reference = rand_ref(224, 2)
    reads = []
    for read_mod in (0, 1, 31):
        for ref_mod in (0, 1, 31):
            for span in (1, 31, 32, 33, 64, 65):
                ref_off = 32 + ref_mod
                for which in (_edge_places(read_mod, ref_off, span), range(span)):
                    clip = rand_ref(read_mod, 3)
                    seq = clip + mutate(reference[ref_off:ref_off + span], which)
                    ops = ([("S", read_mod)] if read_mod else []) + [("M", span)]
                    reads.append(rd(7000 + ref_off, cig(*ops), seq))
    return [Part(reference, 7000, reads)]


OTHER_OPS = ("N", "H", "P", "B", 10, 11, 12, 13, 14, 15)


def _ops():
    reference = rand_ref(100, 4)
    rb, reads = 90, []
    block = lambda a, n: mutate(reference[a:a + n], (0, n - 1))  # noqa: E731
    reads.append(rd(rb + 5, cig(("=", 10), ("X", 10), ("M", 10)), block(5, 10) + block(15, 10) + block(25, 10)))
    for op in OTHER_OPS:  # the second block is read against region offset +10: the operation between them moves nothing
        reads.append(rd(rb + 20, cig(("M", 10), (op, 5), ("M", 10)), block(20, 10) + block(30, 10)))
    reads.append(rd(rb + 8, cig(("H", 3), ("S", 4), ("M", 20)), "ACGT" + block(8, 20)))
    for op in "MIDS":  # zero counts
        reads.append(rd(rb + 40, cig(("M", 10), (op, 0), ("M", 10)), block(40, 10) + block(50, 10)))
        reads.append(rd(rb + 40, cig((op, 0), ("M", 10)), block(40, 10)))
    return [Part(reference, rb, reads)]


ODD_BASES = ("N", "=", "M")


def _indel_places(length):
    """where a base that is not A/C/G/T sits in an indel of `length` bases: its first, last, 32nd and 33rd base"""
    return sorted({p for p in (0, length - 1, 31, 32) if p < length})


def _insertions():
    reference = rand_ref(120, 5)
    rb, reads = 0, []
    for n, length in enumerate(LENGTHS):
        ins = rand_ref(length, 50 + n)
        variants = [ins] + [ins[:p] + ODD_BASES[(n + k) % 3] + ins[p + 1:] for k, p in enumerate(_indel_places(length))]
        for v in variants:
            front, back = mutate(reference[10:30], (0, 19)), mutate(reference[30:50], (0, 19))
            reads.append(rd(rb + 10, cig(("I", length), ("M", 20)), v + front))
            reads.append(rd(rb + 10, cig(("M", 20), ("I", length), ("M", 20)), front + v + back))
            reads.append(rd(rb + 10, cig(("M", 20), ("I", length)), front + v))
    front, back = mutate(reference[10:30], (0, 19)), mutate(reference[30:50], (0, 19))
    ins = rand_ref(40, 60)
    reads.append(rd(rb + 10, cig(("M", 20), ("I", 40), ("M", 20)), front + ins[:25]))  # runs past l_qseq: cut there
    reads.append(rd(rb + 10, cig(("M", 20), ("I", 40), ("M", 20)), front))             # begins at l_qseq: nothing
    reads.append(rd(rb + 10, cig(("M", 20), ("I", 40), ("M", 20)), front[:12]))        # begins behind l_qseq
    reads.append(rd(rb + 10, cig(("M", 20), ("I", 40), ("M", 20)), front + ins[:24] + "N"))  # cut, and its last base kept is no base
    return [Part(reference, rb, reads)]


SEGMENT = 160


def _deletions():
    """a segment of the region per (length, where the odd letter sits): 20 bases, the deleted stretch, 20 bases"""
    segments, reads, rb = [], [], 30000
    odd = ("N", "R", "a", "-")
    for n, length in enumerate(LENGTHS):
        for k, p in enumerate([None] + _indel_places(length)):
            seg = list(rand_ref(SEGMENT, 70 + 10 * n + k))
            if p is not None:
                seg[20 + p] = odd[(n + k) % 4]
            at = SEGMENT * len(segments)
            seg = "".join(seg)
            segments.append(seg)
            clean = "".join(c if c in "ACGT" else "A" for c in seg)
            front, back = mutate(clean[0:20], (0, 19)), mutate(clean[20 + length:40 + length], (0, 19))
            reads.append(rd(rb + at + 20, cig(("D", length), ("M", 20)), back))
            reads.append(rd(rb + at, cig(("M", 20), ("D", length), ("M", 20)), front + back))
            reads.append(rd(rb + at, cig(("M", 20), ("D", length)), front))
    reference = "".join(segments)
    size = len(reference)
    # the region's end: ref_offset + count at REF_SIZE - 1 is an event, at REF_SIZE and behind it none, and the walk ends at the next operation
    tail = mutate(reference[size - 30:size - 20], (0, 9))
    for count in (19, 20, 21, 500):
        reads.append(rd(rb + size - 30, cig(("M", 10), ("D", count), ("M", 5), ("I", 3), ("M", 5)), tail + "ACGTACGTACGTA"))
    # ... and so does the walk of a read whose deletion ends exactly at REF_SIZE with an insertion as its next operation: no event
    # at the position behind the region (the mutation audit asked for this one)
    reads.append(rd(rb + size - 30, cig(("M", 10), ("D", 20), ("I", 3), ("M", 5)), tail + "ACGTACGT"))
    return [Part(reference, rb, reads)]


REGION_SIZES = (1, 31, 32, 33, 63, 64, 65)


def _region_end():
    out = []
    for rb in (0, BIG_BEGIN):
        for size in REGION_SIZES:
            reference = rand_ref(size, 200 + size)
            inv = "".join(other(c) for c in reference)
            start = max(size - 3, 0)
            reads = [rd(rb - 1, cig(("M", 5)), "ACGTA"),                                    # in front of the region: skipped
                     rd(rb, cig(("M", size)), mutate(reference, {0, size - 1})),
                     dict(rd(rb, [], "ACGTA")),                                             # n_cigar == 0
                     rd(rb + size - 1, cig(("M", 4)), inv[-1] + "CGT"),                     # counted, one base compared
                     rd(rb + start, cig(("M", 10)), (inv[start:] + "ACGTACGTAC")[:10]),     # crosses the end, mismatches on both sides
                     rd(rb + start, cig(("S", 2), ("M", 2), ("D", 1), ("M", 10)), "AC" + (inv[start:start + 2] + "ACGTACGTACGT")[:12]),
                     rd(rb + size, cig(("M", 4)), "ACGT"),                                  # GTX_DISC_END
                     rd(rb + size + 7, cig(("M", 4)), "ACGT")]
            out.append(Part(reference, rb, reads))
    return out


def _short_rows():
    reference = rand_ref(200, 6)
    inv = "".join(other(c) for c in reference)
    rb = 64
    reads = [rd(rb + 10, cig(("M", 50)), inv[10:40]),                                   # l_qseq below the CIGAR's query length
             rd(rb + 10, cig(("M", 50)), ""),                                           # l_qseq == 0 with a CIGAR
             rd(rb + 10, cig(("S", 5), ("M", 20), ("I", 10), ("M", 20)), "ACGTA" + inv[10:30] + "ACG"),
             rd(rb + 10, cig(("M", 20), ("I", 10), ("M", 20)), inv[10:30]),
             rd(rb + 10, cig(("S", 40), ("M", 20)), inv[10:40]),                        # the S alone runs past l_qseq
             rd(rb + 10, cig(("I", 10), ("M", 20)), ""),
             rd(rb + 3, cig(("M", 100)), inv[3:36])]
    wide = Part(reference, rb, reads, stride=4 * 16 * 2, fill=15)  # rows four times as wide as needed, every bit behind l_qseq set
    # the same rows with a base behind l_qseq (A, then C): a walk that looks one base too far sees a mismatch there
    out = [wide, Part(reference, rb, reads, stride=4 * 16 * 2, fill=1), Part(reference, rb, reads, stride=4 * 16 * 2, fill=2)]
    for k in (1, 2, 3):  # l_qseq exactly 32 k in a row of minimal stride, a mismatch on its last base
        n = 32 * k
        rs = [rd(rb + 7, cig(("M", n)), mutate(reference[7:7 + n], (n - 1,))), rd(rb + 7, cig(("M", n + 5)), mutate(reference[7:7 + n], (0, n - 1))),
              rd(rb + 7, cig(("S", 1), ("M", n - 1)), "A" + mutate(reference[7:6 + n], (n - 2,))),
              rd(rb + 7, cig(("M", n - 3), ("I", 3)), mutate(reference[7:4 + n], (0,)) + "ACG"), rd(rb + 7, cig(("M", n - 3), ("I", 8)), reference[7:4 + n] + "ACG")]
        out.append(Part(reference, rb, rs, stride=16 * k, fill=15))
    return out


READ_SIZES = (1, 2, 255, 256, 257, 600, 1000)
QUALITIES = (0, 24, 25, 255)


def _quality_distance():
    reference = rand_ref(1100, 7)
    rb, reads = 12345, []
    for n, size in enumerate(READ_SIZES):
        for q in range(4):
            at = sorted({0, size // 2, size - 1})
            qual = [30] * size
            for j, p in enumerate(at):
                qual[p] = QUALITIES[(q + j) % 4]
            reads.append(rd(rb + 50 + n, cig(("M", size)), mutate(reference[50 + n:50 + n + size], at), qual))
    return [Part(reference, rb, reads)]


EVENT_COUNTS = (0, 1, 11, 12, 17, 18, 64, 250)


def event_count_reads(n_reads, reference, rb):
    """read i has EVENT_COUNTS[...] events, interleaved; the first and the last lane of every wavefront have none"""
    reads = []
    made = {}
    for i in range(n_reads):
        count = 0 if i % 64 in (0, 63) else EVENT_COUNTS[(i + i // 64) % len(EVENT_COUNTS)]
        if count not in made:
            made[count] = rd(rb + 20, cig(("M", 260)), mutate(reference[20:280], range(3, 3 + count)))
        reads.append(made[count])
    return reads


def _event_counts():
    reference = rand_ref(300, 8)
    return [Part(reference, 0, event_count_reads(130, reference, 0))]


def _simulated():
    from test_discovery import simulate
    out = []
    for seed in range(1, 7):
        reference, rb, reads = simulate(seed, n_reads=300)
        out.append(Part(reference, rb, [dict(r) for r in reads]))
    return out


LONG_DELETIONS = (65535, 65536, 66000)


def _long_deletion():
    reference = rand_ref(70000, 9)
    rb = 1000
    reads = [rd(rb + 100, cig(("M", 10), ("D", n), ("M", 10)), mutate(reference[100:110], (0,)) + mutate(reference[110 + n:120 + n], (9,))) for n in LONG_DELETIONS]
    return [Part(reference, rb, reads)]


SETS = dict(codes=_codes, group_edges=_group_edges, ops=_ops, insertions=_insertions, deletions=_deletions, region_end=_region_end, short_rows=_short_rows,
            quality_distance=_quality_distance, event_counts=_event_counts, simulated=_simulated, long_deletion=_long_deletion)


@functools.lru_cache(maxsize=None)
def parts(name):
    return SETS[name]()


def as_tuple(e):
    return (e["pos"], e["seq"], e["len"], ord(e["type"]), e["hq"], e["max_distance"], e["reserved"])


def restated(part, stated_limit=True):
    """per read (state, n_events, pos_end, [event tuples]) by the restatement; stated_limit: without the deletions of more than 65 535 bases"""
    out = []
    for r in part.reads:
        state, pos_end, events = ref.walk(part.reference, part.region_begin, r["pos"], r["cigar"], r["seq"], r["qual"])
        if stated_limit:
            events = [e for e in events if not (e["type"] == "D" and e["len"] > 0xFFFF)]
        out.append((state, len(events), pos_end, [as_tuple(e) for e in events]))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    return [restated(p) for p in parts(name)]


# ---- arrays and files -----------------------------------------------------------------------------------------------------------
def arrays(part, reads=None):
    """-> dict(planes uint32 (n, stride / 4), codes uint8 (n, 2 * stride), qual uint8 (n, qual_stride), reads DISC_READ, cigar uint32)"""
    reads = part.reads if reads is None else reads
    n, stride = len(reads), part.stride
    codes = np.full((n, 2 * stride), part.fill, np.uint8)
    qual_stride = max([len(r["seq"]) for r in reads] + [1])
    qual = np.full((n, qual_stride), 0xEE, np.uint8)
    dr = np.zeros(n, gtx.DISC_READ)
    cg, lut = [], np.zeros(256, np.uint8)
    for c, v in CODE.items():
        lut[ord(c)] = v
    known = {}
    for i, r in enumerate(reads):
        m = len(r["seq"])
        assert m <= 2 * stride
        if id(r) not in known:
            known[id(r)] = (lut[np.frombuffer(r["seq"].encode(), np.uint8)], np.array(r["qual"], np.uint8), len(cg))
            cg.extend(r["cigar"])
        codes[i, :m], qual[i, :m], off = known[id(r)]
        dr[i] = (r["pos"], r.get("flag", 3), r.get("mapq", 60), 0, m, len(r["cigar"]), off)
    bits = ((codes[:, :, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(np.uint8)          # (n, bases, plane)
    words = np.packbits(bits.reshape(n, stride // 16, 32, 4), axis=2, bitorder="little")      # (n, groups, 4 bytes, plane)
    planes = np.ascontiguousarray(words.transpose(0, 1, 3, 2)).view("<u4").reshape(n, stride // 4)
    return dict(planes=planes, codes=codes, qual=qual, reads=dr, cigar=np.array(cg + [0], np.uint32))


def total_events(part_expected):
    return sum(e[1] for e in part_expected)


def write_case(path, part, a, event_cap, counts=(0, 0), launches=1):
    """the input of tests/emu_disc_events: a header of eight uint32 and one int64, the region's bytes, and the arrays of arrays()"""
    refb = part.reference.encode("latin-1")
    with open(path, "wb") as f:
        f.write(struct.pack("<8Iq", part.stride, a["qual"].shape[1], len(a["reads"]), len(a["cigar"]), len(refb), event_cap, counts[0], counts[1],
                            part.region_begin))
        f.write(struct.pack("<I", launches))
        f.write(refb)
        for key in ("planes", "qual", "reads", "cigar"):
            f.write(np.ascontiguousarray(a[key]).tobytes())


def read_result(path, n_reads, event_cap):
    """the output of tests/emu_disc_events -> (counts, read_out, events, canary)"""
    raw = open(path, "rb").read()
    counts = np.frombuffer(raw, np.uint32, 2)
    read_out = np.frombuffer(raw, gtx.DISC_READ_OUT, n_reads, 8)
    events = np.frombuffer(raw, gtx.DISC_EVENT, event_cap, 8 + 16 * n_reads)
    assert len(raw) == 8 + 16 * n_reads + 20 * event_cap
    return counts, read_out, events


def per_read(read_out, events, limit=None):
    """what a launch left, per read: (state, n_events, pos_end, [event tuples] or None when the read's events lie behind `limit`); every
    event has to name its read"""
    out = []
    limit = len(events) if limit is None else limit
    for i, ro in enumerate(read_out):
        first, n = int(ro["first_event"]), int(ro["n_events"])
        mine = None
        if first + n <= limit:
            ev = events[first:first + n]
            assert (ev["read"] == i).all(), "read %d: an event of another read in its piece" % i
            mine = [tuple(int(x) for x in (e["pos"], e["seq"], e["len"], e["type"], e["hq"], e["max_distance"], e["reserved"])) for e in ev]
        out.append((int(ro["state"]), n, int(ro["pos_end"]), mine))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(part):
    import ctypes as C
    from oracle_lib import lib as olib, _p
    L = olib()
    L.gto_first_pass_events.restype = C.c_long
    reads, n = part.reads, len(part.reads)
    pos = np.array([r["pos"] for r in reads], np.int32)
    flag = np.array([r["flag"] for r in reads], np.uint16)
    mapq = np.array([r["mapq"] for r in reads], np.uint8)
    cg = np.array([w for r in reads for w in r["cigar"]] + [0], np.uint32)
    cg_off = np.cumsum([0] + [len(r["cigar"]) for r in reads]).astype(np.uint32)
    codes = np.array([CODE[c] for r in reads for c in r["seq"]] + [0], np.uint8)
    qual = np.array([q for r in reads for q in r["qual"]] + [0], np.uint8)
    c_off = np.cumsum([0] + [len(r["seq"]) for r in reads]).astype(np.uint32)
    refb = part.reference.encode("latin-1")
    cap, word_cap = 1 << 12, 1 << 12
    while True:
        events, read_out, words, n_words = np.zeros(cap, gtx.DISC_EVENT), np.zeros(max(n, 1), gtx.DISC_READ_OUT), np.zeros(word_cap, np.uint32), C.c_long()
        got = L.gto_first_pass_events(refb, C.c_long(len(refb)), C.c_long(part.region_begin), C.c_long(n), _p(pos), _p(flag), _p(mapq), _p(cg), _p(cg_off),
                                      _p(codes), _p(qual), _p(c_off), _p(events), C.c_long(cap), _p(read_out), _p(words), C.c_long(word_cap), C.byref(n_words))
        if got == -2:
            cap *= 8
            continue
        assert got >= 0, L.gto_last_error()
        if n_words.value > word_cap:
            word_cap = int(n_words.value)
            continue
        return per_read(read_out[:n], events[:got]), words[:n_words.value]


def oracle_events(part):
    """the oracle's walk (oracle/gto_discovery.hpp) over a part -> per read as per_read; its pass ends at the first GTX_DISC_END read"""
    return _oracle(part)[0]


def oracle_words(part):
    """the words the oracle's first pass leaves of a part (what gtx_disc_first_pass and gtx_disc_first_pass_device have to write)"""
    return _oracle(part)[1]


def before_the_end(rows):
    """the reads up to and including the first GTX_DISC_END read: the ones the reference's pass, and so the oracle, looks at"""
    for i, row in enumerate(rows):
        if row[0] == ref.END:
            return i + 1
    return len(rows)


# ---- what the sets are for --------------------------------------------------------------------------------------------------------
def kinds(rows):
    c = {"X": 0, "I": 0, "D": 0}
    for row in rows:
        for e in row[3]:
            c[chr(e[3])] += 1
    return c


def facts_codes(exp):
    ps = parts("codes")
    n = 0
    for p, rows in zip(ps, exp):
        byte = p.reference[0]
        for r, row in zip(p.reads, rows):
            for e in row[3]:
                o = e[0] - p.region_begin
                assert o in CODE_OFFSETS and byte in "ACGT" and chr(e[1]) in "ACGT" and chr(e[1]) != byte and chr(e[1]) == r["seq"][o]
                n += 1
    assert n == 4 * 3 * 4  # an upper-case A/C/G/T in the region, one of the three other bases in the read, at four offsets


def facts_group_edges(exp):
    p, rows = parts("group_edges")[0], exp[0]
    assert len(rows) == 2 * 3 * 3 * 6 and all(row[0] == ref.COUNTED for row in rows)
    both_sides = 0
    for k in range(0, len(rows), 2):
        span, read_mod = p.reads[k]["cigar"][-1] >> 4, len(p.reads[k]["seq"]) - (p.reads[k]["cigar"][-1] >> 4)
        ref_off = p.reads[k]["pos"] - p.region_begin
        places = _edge_places(read_mod, ref_off, span)
        assert rows[k + 1][1] == span and [e[0] - p.region_begin - ref_off for e in rows[k][3]] == places  # every base; the edges
        both_sides += any((read_mod + q) % 32 == 31 for q in places) and any((ref_off + q) % 32 == 0 for q in places)
    assert kinds(rows)["X"] >= 54 * 2 and both_sides >= 20


def facts_ops(exp):
    p, rows = parts("ops")[0], exp[0]
    rb = p.region_begin
    assert [e[0] - rb for e in rows[0][3]] == [5, 14, 15, 24, 25, 34]  # = and X as M
    for row in rows[1:1 + len(OTHER_OPS)]:
        assert [e[0] - rb for e in row[3]] == [20, 29, 30, 39] and row[2] == 40  # the second block is read against +10: only its two own mismatches
    assert [e[0] - rb for e in rows[1 + len(OTHER_OPS)][3]] == [8, 27]
    # zero counts move nothing; a D of no bases is an event of no bases in the reference's text (all_of over nothing holds)
    zero = rows[2 + len(OTHER_OPS):]
    assert [(row[1], row[2]) for row in zero] == [(4, 60), (2, 50), (4, 60), (2, 50), (5, 60), (3, 50), (4, 60), (2, 50)]
    assert [[(e[2], e[0] - rb) for e in row[3] if e[3] == ord("D")] for row in zero[4:6]] == [[(0, 50)], [(0, 40)]] and kinds(zero)["I"] == 0


def facts_insertions(exp):
    p, rows = parts("insertions")[0], exp[0]
    k = kinds(rows)
    n_variants = sum(1 + len(_indel_places(n)) for n in LENGTHS)
    assert k["I"] == 3 * len(LENGTHS) + 1 and k["D"] == 0
    at = 0
    for length in LENGTHS:
        for v in range(1 + len(_indel_places(length))):
            for shape in range(3):
                row, want_ins = rows[at], v == 0
                ins = [e for e in row[3] if e[3] == ord("I")]
                assert len(ins) == want_ins and all(e[2] == length and e[1] == (0 if shape == 0 else 20) for e in ins)
                # the offset moves whether the insertion is an event or not: the block behind it has its two mismatches
                assert sum(e[3] == ord("X") for e in row[3]) == (2 if shape != 1 else 4)
                at += 1
    assert at == 3 * n_variants
    cut, at_end, behind, cut_n = rows[at:at + 4]
    assert [(e[1], e[2]) for e in cut[3] if e[3] == ord("I")] == [(20, 25)] and kinds([at_end, behind, cut_n])["I"] == 0
    assert at_end[1] == 2 and behind[1] == 1


def facts_deletions(exp):
    p, rows = parts("deletions")[0], exp[0]
    size, at = len(p.reference), 0
    for length in LENGTHS:
        for v in range(1 + len(_indel_places(length))):
            for shape in range(3):
                row = rows[at]
                dels = [e for e in row[3] if e[3] == ord("D")]
                assert len(dels) == (v == 0) and all(e[2] == length for e in dels)
                assert sum(e[3] == ord("X") for e in row[3]) == (2 if shape != 1 else 4)
                seg = (at // 3) * SEGMENT
                assert row[2] == seg + {0: 40, 1: 40, 2: 20}[shape] + length
                at += 1
    assert kinds(rows[:at])["D"] == 3 * len(LENGTHS)
    e19, e20, e21, e500 = rows[at:at + 4]
    assert [e[2] for e in e19[3] if e[3] == ord("D")] == [19] and e19[2] == size - 1
    for row in (e20, e21, e500, rows[at + 4]):  # no event, and the walk ends at the next operation
        assert kinds([row]) == {"X": 2, "I": 0, "D": 0} and row[2] == size - 1


def facts_region_end(exp):
    ps = parts("region_end")
    assert len(ps) == 2 * len(REGION_SIZES) and {p.region_begin for p in ps} == {0, BIG_BEGIN}
    for p, rows in zip(ps, exp):
        size, rb = len(p.reference), p.region_begin
        assert [row[0] for row in rows] == [ref.SKIPPED, ref.COUNTED, ref.SKIPPED, ref.COUNTED, ref.COUNTED, ref.COUNTED, ref.END, ref.END]
        assert rows[1][1] == (2 if size > 1 else 1) and rows[1][2] == size - 1
        assert rows[3][1] == 1 and rows[3][3][0][0] == rb + size - 1 and rows[3][2] == size - 1  # one base compared, the clamp
        assert rows[4][1] == min(size, 3) and rows[4][2] == size - 1
        assert all(rb <= e[0] < rb + size for row in rows for e in row[3])


def facts_short_rows(exp):
    ps = parts("short_rows")
    assert ps[0].stride == 4 * 32 and [p.fill for p in ps] == [15, 1, 2, 15, 15, 15] and exp[1] == exp[0] and exp[2] == exp[0]
    ps, exp = [ps[0]] + ps[3:], [exp[0]] + exp[3:]
    rows = exp[0]
    assert [row[1] for row in rows] == [30, 0, 21, 20, 0, 0, 33] and [row[2] for row in rows] == [60, 60, 50, 50, 30, 30, 103]
    assert kinds(rows)["I"] == 1
    for k, rows in zip((1, 2, 3), exp[1:]):
        n, rb = 32 * k, ps[k].region_begin
        assert ps[k].stride == 16 * k and rows[0][3][-1][0] == rb + 7 + n - 1 and rows[0][3][-1][5] == 0
        assert [row[1] for row in rows] == [1, 2, 1, 2, 1] and rows[4][3][0][1:4] == (n - 3, 3, ord("I"))  # (the last one: cut at l_qseq)


def facts_quality_distance(exp):
    rows = exp[0]
    seen_q, at = set(), 0
    for size in READ_SIZES:
        for q in range(4):
            row = rows[at]
            places = sorted({0, size // 2, size - 1})
            assert [e[5] for e in row[3]] == [min(p, size - 1 - p) for p in places]
            assert [e[4] for e in row[3]] == [int(QUALITIES[(q + j) % 4] >= 25) for j in range(len(places))]
            seen_q |= {(QUALITIES[(q + j) % 4], e[4]) for j, e in enumerate(row[3])}
            at += 1
    assert seen_q == {(0, 0), (24, 0), (25, 1), (255, 1)} and max(e[5] for row in rows for e in row[3]) == 499


def facts_event_counts(exp):
    rows = exp[0]
    assert len(rows) == 130 and {row[1] for row in rows} == set(EVENT_COUNTS)
    assert all(rows[i][1] == 0 for i in range(len(rows)) if i % 64 in (0, 63))
    assert all(any(rows[i][1] == c for i in range(w * 64, min(w * 64 + 64, len(rows)))) for c in EVENT_COUNTS for w in (0, 1))


def facts_simulated(exp):
    assert len(exp) == 6
    total = kinds([row for rows in exp for row in rows])
    assert total["X"] >= 300 and total["I"] >= 20 and total["D"] >= 20
    assert all(len(rows) >= 250 for rows in exp)


def facts_long_deletion(exp):
    p, rows = parts("long_deletion")[0], exp[0]
    assert len(p.reference) == 70000
    assert [[e[2] for e in row[3] if e[3] == ord("D")] for row in rows] == [[65535], [], []]  # at exactly 65 535 bases the deletion is an event
    assert [row[2] for row in rows] == [120 + n for n in LONG_DELETIONS] and all(kinds([row])["X"] == 2 for row in rows)
    # ... and the reference's text makes an event of all three
    assert [[e[2] for e in row[3] if e[3] == ord("D")] for row in restated(p, stated_limit=False)] == [[n] for n in LONG_DELETIONS]


FACTS = dict(codes=facts_codes, group_edges=facts_group_edges, ops=facts_ops, insertions=facts_insertions, deletions=facts_deletions,
             region_end=facts_region_end, short_rows=facts_short_rows, quality_distance=facts_quality_distance, event_counts=facts_event_counts,
             simulated=facts_simulated, long_deletion=facts_long_deletion)
assert sorted(FACTS) == sorted(SETS)


# ---- what a launch has to leave, whatever ran it (the emulation, the device) ----------------------------------------------------------
TILING_READS = (1, 63, 64, 65, 255, 256, 257)


def tiling_part(n_reads):
    """event_counts, repeated to n_reads reads"""
    p = parts("event_counts")[0]
    return Part(p.reference, p.region_begin, event_count_reads(n_reads, p.reference, p.region_begin))


@functools.lru_cache(maxsize=None)
def tiling_expected(n_reads):
    known = {}
    p = tiling_part(n_reads)
    out = []
    for r in p.reads:  # (a handful of distinct reads)
        if id(r["cigar"]) not in known:
            known[id(r["cigar"])] = restated(Part(p.reference, p.region_begin, [r]))[0]
        out.append(known[id(r["cigar"])])
    return out


def check_launch(want, counts, read_out, events, event_cap, counts_before=(0, 0)):
    """`want`: the reads' rows by the restatement.  The reads' pieces [first_event, +n_events) are pairwise disjoint and cover
    [counts_before[0], + total) exactly; within each group of 64 consecutive reads they lie behind each other in read order; counts[1]
    has grown by the events of the reads that did not fit event_cap; every read that fits holds its right events; the state, the
    count and pos_end of every read are written whether it fits or not.  -> the number of reads that did not fit"""
    n = read_out["n_events"].astype(np.int64)
    first = read_out["first_event"].astype(np.int64)
    assert len(read_out) == len(want)
    assert [(int(ro["state"]), int(ro["n_events"]), int(ro["pos_end"])) for ro in read_out] == [row[:3] for row in want]
    total = int(n.sum())
    assert int(counts[0]) == counts_before[0] + total
    have = np.nonzero(n > 0)[0]
    if len(have):
        order = have[np.argsort(first[have], kind="stable")]
        assert first[order[0]] == counts_before[0] and (first[order[1:]] == first[order[:-1]] + n[order[:-1]]).all()
        assert first[order[-1]] + n[order[-1]] == counts_before[0] + total
    for w in range(0, len(read_out), 64):
        fw, nw = first[w:w + 64], n[w:w + 64]
        if nw.sum():
            assert (fw == fw[0] + np.concatenate([[0], np.cumsum(nw)[:-1]])).all(), "wave at read %d: not behind each other in read order" % w
    fits = first + n <= event_cap
    assert int(counts[1]) == counts_before[1] + int(n[~fits].sum())
    known = {}
    for i, w in enumerate(want):
        if n[i] and fits[i]:
            if id(w[3]) not in known:
                known[id(w[3])] = np.array(w[3], np.int64).reshape(-1, 7)
            ev = events[first[i]:first[i] + n[i]]
            assert (ev["read"] == i).all(), "read %d: an event of another read in its piece" % i
            got = np.stack([ev[k].astype(np.int64) for k in EVENT_FIELDS], axis=1)
            assert np.array_equal(got, known[id(w[3])]), "read %d: %s != %s" % (i, got[:3].tolist(), w[3][:3])
    return int((~fits & (n > 0)).sum())


EVENT_FIELDS = ("pos", "seq", "len", "type", "hq", "max_distance", "reserved")


# ---- the launch-level cases by name (what tests/disc_events_mutants runs beside the sets) -------------------------------------------
# name -> (reads, event_cap as an expression of `total`, the counters at entry, launches)
LAUNCHES = {"tiling_%d" % n: (n, "total", (0, 0), 1) for n in TILING_READS}
LAUNCHES.update(capacity_total=(257, "total", (0, 0), 1), capacity_total_minus_1=(257, "total - 1", (0, 0), 1), capacity_1=(257, "1", (0, 0), 1),
                capacity_0=(257, "0", (0, 0), 1), counters_7_3=(130, "7 + total", (7, 3), 1), two_launches=(130, "2 * total", (0, 0), 2))


def through(run, part, event_cap, counts=(0, 0), launches=1):
    """a part through tests/emu_disc_events; run(write, read): emu_programs.run with a program and a directory -> (counts, read_out,
    events)"""
    return run(lambda path: write_case(path, part, arrays(part), event_cap, counts, launches), lambda path: read_result(path, len(part.reads), event_cap))


def judge(name, run):
    """None when the program behind `run` gives the set or launch-level case `name` as the restatement says, else what differs"""
    try:
        if name in SETS:
            for k, (part, want) in enumerate(zip(parts(name), expected(name))):
                total = total_events(want)
                counts, read_out, events = through(run, part, total)
                got = per_read(read_out, events)
                wrong = [i for i in range(len(want)) if got[i] != want[i]]
                if wrong:
                    return "part %d, read %d differs from the restatement" % (k, wrong[0])
                check_launch(want, counts, read_out, events, total)
            return None
        n_reads, cap, before, launches = LAUNCHES[name]
        part, want = tiling_part(n_reads), tiling_expected(n_reads)
        total = total_events(want)
        event_cap = eval(cap, dict(total=total))
        counts, read_out, events = through(run, part, event_cap, before, launches)
        check_launch(want, counts, read_out, events, event_cap, (before[0] + (launches - 1) * total, before[1]))
        return None
    except AssertionError as e:
        return "a launch-level condition fails: %s" % (str(e)[:120] or "see check_launch")
