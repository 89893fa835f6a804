"""Case sets for the second pass up to the aligner (graphtyper_amd/csrc/gtx_disc_second_dev.hpp): the smallest shapes at which the
intake, the buckets, the list and the rounds' choice of reads can go wrong.  A set is a list of cases; a case is one file: a region,
its reads in stream order, the indel table, and -- for the rounds -- the reads' current state and entries where they are not what
the intake left.  What a set is for is asserted from the restatement's output (tests/disc_second_ref.py) by its entry in FACTS:
no set filters or skips a case.

    cases(name)     -> [Case]                                     (made once)
    expected(case)  -> what the restatement says of it: the intake, the found-bits, the list, the pairs (made once per case)
    arrays(case)    -> the arrays of gtx_disc_second_intake / gtx_disc_second_candidates for a case (numpy)
    through(run, case, ...) -> a case through tests/emu_disc_second; differs(case, got, ...) -> None, or how `got` differs
All values are integers; there is no tolerance."""
import functools
import struct

import numpy as np

import disc_event_cases as dc
import disc_second_ref as ref
from disc_event_cases import cig, mutate, other, rand_ref, rd
from graphtyper_amd import lib as gtx

NT16 = dc.NT16
BIG_BEGIN = dc.BIG_BEGIN
NO_BUCKET = gtx.DISC_NO_BUCKET


def ent(pos, kind, seq, span=1, good=False, file_index=0):
    return dict(pos=pos, type=kind, seq=seq, span=span, good=good, file_index=file_index)


class Case:
    def __init__(self, reference, region_begin, reads, table=(), bucket_size=50, file_index=0, lst=None, state=None, entries=None, stride=None, fill=0):
        """table: entries in any order (kept in table order); lst: the list as table indices (default: the plan's); state: {read: dict of
        fields that differ from what the intake left, or None for pos = -1}; entries: {read: [(table index, read_pos)]}"""
        self.part = dc.Part(reference, region_begin, reads, stride=stride, fill=fill)
        self.table = sorted(table, key=ref.table_order)
        self.bucket_size, self.file_index, self.lst, self.state, self.entries = bucket_size, file_index, lst, state or {}, entries or {}

    reference = property(lambda self: self.part.reference)
    region_begin = property(lambda self: self.part.region_begin)
    reads = property(lambda self: self.part.reads)
    n_buckets = property(lambda self: ref.n_buckets(len(self.part.reference), self.bucket_size))

    def index_of(self, pos, kind, seq):
        return next(t for t, e in enumerate(self.table) if (e["pos"], e["type"], e["seq"]) == (pos, kind, seq))


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> dict(taken: ref.intake's result, found [bool], lst, states (current), entries (per read), pairs [(read, k)] of the whole list)"""
    taken = ref.intake(case.reference, case.region_begin, case.bucket_size, case.reads)
    found = ref.found_bits(case.table, taken["events"])
    lst = list(case.lst) if case.lst is not None else ref.plan(case.table, found, case.file_index)
    states = []
    for i, s in enumerate(taken["reads"]):
        if i in case.state:
            over = case.state[i]
            s = dict(s or dict(pos=-1, pos_end=-1, score=0, num_clipped_begin=0, num_clipped_end=0, num_ins_begin=0, flags=0, mapq=0, l_qseq=0, bucket=NO_BUCKET))
            s.update(over if over is not None else dict(pos=-1))
        states.append(s)
    entries = [list(case.entries.get(i, ())) for i in range(len(case.reads))]
    pairs = ref.candidates(case.table, lst, 0, len(lst), taken, states, entries, case.region_begin, case.bucket_size)
    return dict(taken=taken, found=found, lst=lst, states=states, entries=entries, pairs=pairs)


def pairs_of(case, k0, k1):
    return [(i, k) for i, k in expected(case)["pairs"] if k0 <= k < k1]


# ---- arrays and files -----------------------------------------------------------------------------------------------------------
def second_array(case, states, entries=None):
    """per read state (None: passed over) -> DISC_SECOND_READ array, as gtx_disc_second_intake leaves it (entries None) or as the rounds
    see it"""
    out = np.zeros(len(states), gtx.DISC_SECOND_READ)
    at = 0
    for i, (s, r) in enumerate(zip(states, case.reads)):
        if s is None:
            out[i] = (-1, -1, 0, 0, 0, 0, r.get("flag", 3), r.get("mapq", 60), 0, len(r["seq"]), NO_BUCKET, 0, 0)
        else:
            n = len(entries[i]) if entries else 0
            out[i] = (s["pos"], s["pos_end"], s["score"], s["num_clipped_begin"], s["num_clipped_end"], s["num_ins_begin"], s["flags"], s["mapq"], 0, s["l_qseq"],
                      s["bucket"], at if n else 0, n)
            at += n
    return out


def table_arrays(table):
    t = np.zeros(len(table), gtx.DISC_INDEL)
    letters = b""
    for i, e in enumerate(table):
        t[i] = (e["pos"], len(e["seq"]), len(letters), e["span"], ord(e["type"]), int(e["good"]), e["file_index"])
        letters += e["seq"].encode("latin-1")
    return t, np.frombuffer(letters, np.uint8).copy()


def found_words(found):
    w = np.zeros((len(found) + 31) // 32, np.uint32)
    for t, f in enumerate(found):
        if f:
            w[t >> 5] |= np.uint32(1 << (t & 31))
    return w


@functools.lru_cache(maxsize=None)
def arrays(case):
    """-> dict(planes, reads, cigar (as dc.arrays), table DISC_INDEL, letters uint8, lst uint32, given (the rounds see a state of their
    own), state DISC_SECOND_READ, events DISC_SECOND_EVENT)"""
    a = dict(dc.arrays(case.part))
    want = expected(case)
    a["table"], a["letters"] = table_arrays(case.table)
    a["lst"] = np.array(want["lst"], np.uint32)
    a["given"] = bool(case.state or case.entries)
    a["state"] = second_array(case, want["states"], want["entries"])
    a["events"] = np.array([e for per in want["entries"] for e in per], gtx.DISC_SECOND_EVENT).reshape(-1)
    return a


def write_case(path, case, k0, k1, pair_cap, counts=(0, 0), launches=1):
    """the input of tests/emu_disc_second (its first lines)"""
    a = arrays(case)
    refb = case.reference.encode("latin-1")
    with open(path, "wb") as f:
        f.write(struct.pack("<16Iq", case.part.stride, len(a["reads"]), len(a["cigar"]), len(refb), case.bucket_size, len(a["table"]), len(a["letters"]), launches,
                            len(a["lst"]), k0, k1, len(a["events"]), pair_cap, counts[0], counts[1], int(a["given"]), case.region_begin))
        f.write(refb)
        for key in ("planes", "reads", "cigar", "table", "letters", "lst", "events"):
            f.write(np.ascontiguousarray(a[key]).tobytes())
        if a["given"]:
            f.write(a["state"].tobytes())


def read_result(path, case, pair_cap):
    raw = open(path, "rb").read()
    n, nb, nt = len(case.reads), case.n_buckets, len(case.table)
    out, at = {}, 0
    for key, dtype, count in (("second", gtx.DISC_SECOND_READ, n), ("bucket_max", np.int32, nb), ("global_max", np.int32, nb), ("max_read_size", np.uint32, 1),
                              ("bucket_reads", np.uint32, n), ("bucket_off", np.uint32, nb + 1), ("found", np.uint32, (nt + 31) // 32), ("counts", np.uint32, 2),
                              ("pairs", gtx.DISC_SECOND_PAIR, pair_cap)):
        out[key] = np.frombuffer(raw, dtype, count, at)
        at += count * np.dtype(dtype).itemsize
    assert at == len(raw)
    return out


def through(run, case, k0=0, k1=None, pair_cap=None, counts=(0, 0), launches=1):
    """a case through tests/emu_disc_second; run(write, read): emu_programs.run with a program and a directory -> the outputs by name.
    Defaults: the whole list, room for all of its pairs"""
    k1 = len(expected(case)["lst"]) if k1 is None else k1
    pair_cap = counts[0] + launches * len(pairs_of(case, k0, k1)) if pair_cap is None else pair_cap
    return run(lambda path: write_case(path, case, k0, k1, pair_cap, counts, launches), lambda path: read_result(path, case, pair_cap))


def intake_differs(case, got):
    """None, or how what an intake left differs from the restatement"""
    want = expected(case)
    taken = want["taken"]
    second = second_array(case, taken["reads"])
    for name in gtx.DISC_SECOND_READ.names:
        bad = np.nonzero(got["second"][name] != second[name])[0]
        if len(bad):
            return "read %d: %s is %d, the restatement says %d" % (bad[0], name, got["second"][name][bad[0]], second[name][bad[0]])
    if list(got["bucket_max"]) != taken["max_pos_end"]:
        return "max_pos_end differs: %s != %s" % (list(got["bucket_max"])[:8], taken["max_pos_end"][:8])
    if list(got["global_max"]) != taken["global_max_pos_end"]:
        return "global_max_pos_end differs: %s != %s" % (list(got["global_max"])[:8], taken["global_max_pos_end"][:8])
    if int(got["max_read_size"][0]) != taken["max_read_size"]:
        return "max_read_size is %d, not %d" % (got["max_read_size"][0], taken["max_read_size"])
    off = np.concatenate([[0], np.cumsum([len(b) for b in taken["bucket_reads"]])])
    if list(got["bucket_off"]) != list(off):
        return "the buckets' offsets differ"
    grouped = [i for b in taken["bucket_reads"] for i in b] + [i for i, s in enumerate(taken["reads"]) if s is None]
    if list(got["bucket_reads"]) != grouped:
        return "the grouping differs"
    if list(got["found"]) != list(found_words(want["found"])):
        return "the found-bits differ: %s != %s" % (list(got["found"]), list(found_words(want["found"])))
    return None


def pairs_differ(case, got, k0, k1, pair_cap, before=(0, 0), launches=1):
    """None, or how the pairs and counters differ: every launch appends the slice's pairs in the restatement's order at counts[0];
    counts[1] grows by those at or behind pair_cap; nothing else of the buffer is touched"""
    want = np.array(pairs_of(case, k0, k1), np.uint32).reshape(-1, 2)
    total, at, lost = len(want), before[0], before[1]
    pairs = got["pairs"]
    touched = np.zeros(pair_cap, bool)
    for _ in range(launches):
        fit = min(max(pair_cap - at, 0), total)
        have = pairs[at:at + fit]
        if not (np.array_equal(have["read"], want[:fit, 0]) and np.array_equal(have["entry"], want[:fit, 1])):
            j = next(j for j in range(fit) if (have["read"][j], have["entry"][j]) != tuple(want[j]))
            return "pair %d is %s, the restatement says %s" % (at + j, (have["read"][j], have["entry"][j]), tuple(want[j]))
        touched[at:at + fit] = True
        lost += total - fit
        at += total
    if tuple(int(c) for c in got["counts"]) != (at, lost):
        return "the counters are %s, not %s" % (tuple(got["counts"]), (at, lost))
    if not (pairs[~touched].view(np.uint8) == 0xA5).all():
        return "an entry of the pair buffer that is nobody's was written"
    return None


def differs(case, got, k0=0, k1=None, pair_cap=None, before=(0, 0), launches=1):
    k1 = len(expected(case)["lst"]) if k1 is None else k1
    pair_cap = len(got["pairs"]) if pair_cap is None else pair_cap
    return intake_differs(case, got) or pairs_differ(case, got, k0, k1, pair_cap, before, launches)


# ---- the sets -----------------------------------------------------------------------------------------------------------------
REGION_LETTERS = "ACGTNRMK" + "Z"  # (Z: a letter outside the nt16 alphabet)
LETTER_OFFSETS = (0, 31, 32, 33)


def _letters():
    out = []
    for n, letter in enumerate(REGION_LETTERS):
        base = list(rand_ref(70, 300 + n))
        for o in LETTER_OFFSETS:
            base[o] = letter
        reads = []
        for code in range(16):
            for o in LETTER_OFFSETS:
                seq = list(base[:40])
                for p in LETTER_OFFSETS:
                    seq[p] = "N"  # (an N scores +1 against any letter)
                seq[o] = NT16[code]
                reads.append(rd(900, cig(("M", 40)), "".join(seq)))
        out.append(Case("".join(base), 900, reads))
    return out


EDGE_SPANS = (31, 32, 33, 63, 64, 65)


def _group_edges():
    reference = rand_ref(224, 2)
    mods = sorted({(a, b) for a in range(32) for b in (0, 1, 31)} | {(a, b) for a in (0, 1, 31) for b in range(32)})
    reads = []
    for read_mod, ref_mod in mods:
        for span in EDGE_SPANS:
            ref_off = 32 + ref_mod
            seq = rand_ref(read_mod, 3) + mutate(reference[ref_off:ref_off + span], (0, span - 1))
            reads.append(rd(7000 + ref_off, cig(*([("S", read_mod)] if read_mod else []) + [("M", span)]), seq))
    # rows twice as wide as the longest read; behind l_qseq every base is '=' (a mismatch for a walk that looks too far), then N, then A
    return [Case(reference, 7000, reads, stride=64, fill=f) for f in (0, 15, 1)]


def _overruns():
    out = []
    for rb in (0, BIG_BEGIN):
        reference = rand_ref(100, 11)
        inv = "".join(other(c) for c in reference)
        ins = "GATTACAGAT"
        reads = [rd(rb + 90, cig(("M", 20)), inv[90:] + "ACGTACGTAC"),                        # 0 M over the region's end: 10 bases compared
                 rd(rb + 10, cig(("M", 30)), inv[10:30]),                                    # 1 M over the read's end: 20 bases compared
                 rd(rb + 85, cig(("M", 30)), inv[85:95]),                                    # 2 over both
                 rd(rb + 10, cig(("S", 40), ("M", 20)), inv[10:40]),                         # 3 the S alone runs past l_qseq
                 rd(rb + 10, cig(("M", 50)), ""),                                            # 4 l_qseq == 0 with a CIGAR
                 rd(rb + 11, cig(("M", 20), ("I", 5)), reference[11:31] + ins[:5]),          # 5 I at the read's end, whole (one position on)
                 rd(rb + 10, cig(("M", 20), ("I", 10), ("M", 5)), reference[10:30] + ins[:5]),  # 6 truncated: 5 letters, the penalty of 10
                 rd(rb + 10, cig(("M", 20), ("I", 10), ("M", 5)), reference[10:30]),         # 7 empty: nothing happens, the read offset stays
                 rd(rb + 10, cig(("M", 20), ("I", 10), ("M", 5)), reference[10:22])]         # 8 begins behind l_qseq
        for count in (9, 10, 11):                                                            # 9-11 ref_offset + count on REF_SIZE - 1 / REF_SIZE / REF_SIZE + 1
            reads.append(rd(rb + 80, cig(("M", 10), ("D", count), ("M", 5)), reference[80:90] + inv[90:95]))
        reads += [rd(rb + 99, cig(("M", 4)), inv[99] + "CGT"),                                # 12 starts on the last base of the region
                  rd(rb - 1, cig(("M", 5)), "ACGTA"),                                        # 13 one before region_begin
                  dict(rd(rb + 5, [], "ACGTA")),                                             # 14 no CIGAR
                  rd(rb + 100, cig(("M", 4)), "ACGT"),                                       # 15 at the region's end (the stated limit)
                  rd(rb + 107, cig(("M", 4)), "ACGT"),                                       # 16 behind it
                  rd(rb + 90, cig(("M", 10), ("S", 5)), reference[90:] + "ACGTA"),           # 17 the walk ends ON the region's end: the clip is not seen
                  rd(rb + 90, cig(("M", 10), ("I", 3), ("M", 2)), reference[90:] + "ACGTA")]  # 18 ... nor the insertion
        table = [ent(rb + 30, "I", ins[:5], good=True), ent(rb + 30, "I", ins, good=True), ent(rb + 90, "D", reference[90:99]), ent(rb + 90, "D", reference[90:100]),
                 ent(rb + 90, "D", reference[90:100] + "A")]
        out.append(Case(reference, rb, reads, table, bucket_size=30))
    return out


LONG = 65536


def _long_deletion():
    reference = rand_ref(70000, 9)
    rb = 1000
    reads = [rd(rb + 100, cig(("M", 10), ("D", LONG), ("M", 10)), mutate(reference[100:110], (0,)) + mutate(reference[110 + LONG:120 + LONG], (9,))),
             rd(rb + 69000, cig(("M", 50)), reference[69000:69050])]
    table = [ent(rb + 110, "D", reference[110:110 + LONG], span=2), ent(rb + 110, "D", reference[110:110 + LONG - 1], span=2, good=True)]
    return [Case(reference, rb, reads, table, bucket_size=1000)]  # 70 buckets


CLIP_SHAPES = ((("S", 5), ("M", 20)), (("M", 20), ("S", 5)), (("S", 5), ("M", 20), ("S", 7)), (("M", 20), ("S", 3), ("S", 4)), (("S", 5), ("S", 6), ("M", 20)),
               (("H", 3), ("S", 4), ("M", 20)), (("M", 20), ("S", 6), ("H", 2)), (("S", 32767), ("M", 10)), (("S", 32768), ("M", 10)), (("M", 10), ("S", 32767)),
               (("M", 10), ("S", 32768)), (("M", 10), ("S", 65535)), (("M", 10), ("S", 65536)))
CLIP_WANT = ((5, 0), (0, 5), (5, 7), (0, 4), (5, 6), (0, 4), (0, 6), (32767, 0), (-32768, 0), (0, 32767), (0, -32768), (0, -1), (0, 0))


def _clips():
    reference = rand_ref(200, 12)
    reads = []
    for shape in CLIP_SHAPES:
        seq, at = "", 50
        for op, n in shape:
            if op == "S" and n < 100:
                seq += rand_ref(n, 13)
            elif op == "M":
                seq += reference[at:at + n]
        reads.append(rd(4050, cig(*shape), seq))
    return [Case(reference, 4000, reads)]


def _ops():
    reference = rand_ref(100, 4)
    rb = 90
    block = lambda a, n: mutate(reference[a:a + n], (0, n - 1))  # noqa: E731
    reads = [rd(rb + 20, cig(("M", 10), (op, 5), ("M", 10)), block(20, 10) + "TTGCA" + block(30, 10)) for op in range(16)]
    reads += [rd(rb + 20, cig(("M", 10), (op, 0), ("M", 10)), block(20, 10) + block(30, 10)) for op in (0, 1, 2, 4)]  # zero counts
    return [Case(reference, rb, reads, [ent(rb + 30, "I", "TTGCA"), ent(rb + 30, "D", reference[30:35]), ent(rb + 30, "D", "")])]


def _lookup_region():
    reference = list(rand_ref(300, 14))
    reference[50:53] = "ACG"  # (a deletion of three bases at 50 has an insertion's letters)
    return "".join(reference)


def _ins_read(reference, rb, at, letters, back=20):
    return rd(rb + at - 20, cig(("M", 20), ("I", len(letters)), ("M", back)), reference[at - 20:at] + letters + reference[at:at + back])


def _del_read(reference, rb, at, n, back=20):
    return rd(rb + at - 20, cig(("M", 20), ("D", n), ("M", back)), reference[at - 20:at] + reference[at + n:at + n + back])


LOOKUP_MISSES = ("pos", "pos in front", "type", "longer", "shorter", "first letter", "last letter", "deletion pos", "deletion longer", "deletion shorter", "deletion letter")


def _lookups():
    reference, rb = _lookup_region(), 2000
    wrong = reference[90:93] + other(reference[93])
    table = [ent(rb + 50, "I", "ACG"), ent(rb + 80, "D", reference[80:84], good=True), ent(rb + 120, "I", "ANT"), ent(rb + 90, "D", wrong),
             ent(rb + 150, "I", "TT"), ent(rb + 150, "I", "TTA"), ent(rb + 150, "D", reference[150:152]), ent(rb + 150, "D", reference[150:153])]
    exact = [_ins_read(reference, rb, 50, "ACG"), _del_read(reference, rb, 80, 4), _ins_read(reference, rb, 120, "ANT"), _ins_read(reference, rb, 150, "TTA"),
             _del_read(reference, rb, 150, 3)]
    # (the longer one goes on with the letter that follows ACG in the table's letters: a compare that runs over an entry's end finds it)
    near = [_ins_read(reference, rb, 51, "ACG"), _ins_read(reference, rb, 49, "ACG"), _del_read(reference, rb, 50, 3), _ins_read(reference, rb, 50, "ACG" + reference[80]), _ins_read(reference, rb, 50, "AC"),
            _ins_read(reference, rb, 50, "TCG"), _ins_read(reference, rb, 50, "ACT"), _del_read(reference, rb, 81, 4), _del_read(reference, rb, 80, 5),
            _del_read(reference, rb, 80, 3), _del_read(reference, rb, 90, 4)]
    assert len(near) == len(LOOKUP_MISSES)
    return [Case(reference, rb, exact, table)] + [Case(reference, rb, [r], table) for r in near]


def _stream_order():
    reference = rand_ref(1000, 15)
    rb = 500
    m = lambda at, n: rd(rb + at, cig(("M", n)), reference[at:at + n])  # noqa: E731
    # out of position order: the long read of bucket 10 comes first, so every bucket behind it in the STREAM holds its end
    reads = [m(500, 150), m(100, 50), m(260, 30), m(120, 20), m(905, 60), m(255, 100), m(20, 10)]
    # a region at 0 whose first read ends where it begins: the running maximum is still the 0 it began with
    return [Case(reference, rb, reads), Case(reference, 0, [rd(0, cig(("I", 5)), "ACGTA"), rd(0, cig(("S", 3), ("I", 2)), "ACGTA"), rd(120, cig(("M", 20)), reference[120:140])])]


def _plan_rules():
    reference, rb = rand_ref(1200, 16), 100
    P, Q, R = 300, 600, 900
    # file 0's own indel at P with good neighbours at -61 / -60 / +60 / +61 and one the file does not hold; two indels on Q; file 1's at R
    spec = [(P, "I", "AC", False, 0), (P - 61, "I", "G", True, 1), (P - 60, "I", "GT", True, 1), (P + 60, "D", 2, True, 1), (P + 61, "D", 3, True, 1),
            (P + 10, "I", "TTT", True, 1), (Q, "I", "CA", False, 0), (Q, "D", 2, True, 0), (Q, "I", "CAT", True, 1),
            (R, "D", 4, False, 1), (R - 5, "I", "A", True, 0), (R + 200, "I", "C", True, 0)]
    table, reads = [], []
    for at, kind, what, good, file_i in spec:
        seq = what if kind == "I" else reference[at:at + what]
        table.append(ent(rb + at, kind, seq, good=good, file_index=file_i))
        if (at, kind) != (P + 10, "I"):  # the file's reads hold every indel but this one
            reads.append(_ins_read(reference, rb, at, seq) if kind == "I" else _del_read(reference, rb, at, len(seq)))
    reads.sort(key=lambda r: r["pos"])
    return [Case(reference, rb, reads, table, file_index=f) for f in (0, 1, 2)]


CAND_P, CAND_SPAN = 1000, 3
T_LOW, T_P, T_END = 0, 1, 2  # the candidates' table, in table order


def _cand_base(mrs=100):
    """an indel at CAND_P, reads of 100 bases around it whose buckets all reach over it, one list entry"""
    reference, rb = rand_ref(2000, 17), 10000
    m = lambda at, n=100: rd(rb + at, cig(("M", n)), reference[at:at + n])  # noqa: E731
    return reference, rb, m


def _candidates():
    reference, rb, m = _cand_base()
    P, S = rb + CAND_P, CAND_SPAN
    table = [ent(rb + 150, "I", "G", span=1), ent(P, "D", reference[CAND_P:CAND_P + 2], span=S), ent(rb + 1990, "I", "A", span=1)]  # T_LOW, T_P, T_END
    out = []
    # 1 the four parts of the test, each on its boundary: reads in buckets that reach over the indel, their state set by hand
    bounds = [dict(pos=P - 150, pos_end=P - 1), dict(pos=P - 150, pos_end=P),
              dict(pos=P - 150, pos_end=P - 21, num_clipped_end=10), dict(pos=P - 150, pos_end=P - 20, num_clipped_end=10),
              dict(pos=P - 250, pos_end=P - 111, num_clipped_end=60), dict(pos=P - 250, pos_end=P - 110, num_clipped_end=60),
              dict(pos=P + S, pos_end=P + S + 100), dict(pos=P + S + 1, pos_end=P + S + 101),
              dict(pos=P + S + 20, pos_end=P + S + 120, num_clipped_begin=10), dict(pos=P + S + 21, pos_end=P + S + 121, num_clipped_begin=10),
              dict(pos=P + S + 110, pos_end=P + S + 210, num_clipped_begin=60), dict(pos=P + S + 111, pos_end=P + S + 211, num_clipped_begin=60),
              dict(pos=P - 150, pos_end=P - 1, num_clipped_end=-32768), dict(pos=P + S + 1, pos_end=P + S + 101, num_clipped_begin=-32768),
              dict(pos=P - 10, pos_end=P + 90), dict(pos=P - 10, pos_end=P + 90)]
    # (the last two were taken in far behind the indel, in the last bucket of the window and in the first behind it)
    reads = [m(CAND_P - 60 + 5 * (i % 8)) for i in range(len(bounds) - 2)] + [m(CAND_P + 200), m(CAND_P + 250)]
    out.append(Case(reference, rb, reads, table, lst=[T_P], state={i: b for i, b in enumerate(bounds)}))
    # 2 the bucket rule cuts off a read the test would take: an end clip of 50, ending exactly 50 in front of the indel, alone in its bucket
    lone = rd(P - 200, cig(("M", 100), ("S", 50)), reference[CAND_P - 200:CAND_P - 100] + rand_ref(50, 18))
    out.append(Case(reference, rb, [lone, m(CAND_P - 140), m(CAND_P - 40)], table, lst=[T_P]))
    # 3 the descent stops at an empty bucket: a read far in front whose deletion carries it to the indel is reached only over full buckets
    far = rd(P - 400, cig(("M", 50), ("D", 300), ("M", 50)), reference[CAND_P - 400:CAND_P - 350] + reference[CAND_P - 50:CAND_P])
    chain = [m(CAND_P - 350 + 50 * j) for j in range(3)]  # buckets -7, -6, -5 from the indel's: begin_padded's is -4
    out.append(Case(reference, rb, [far] + chain + [m(CAND_P - 190), m(CAND_P - 20)], table, lst=[T_P]))
    out.append(Case(reference, rb, [far] + chain[:1] + chain[2:] + [m(CAND_P - 190), m(CAND_P - 20)], table, lst=[T_P]))  # bucket -6 empty
    # 4 b_end clamped at the last bucket; an entry whose window begins in bucket 0
    out.append(Case(reference, rb, [m(1850), m(1900), m(1950, 50), m(1990, 10), m(60), m(0), m(300)], table, lst=[T_END, T_LOW]))
    # 5 reads that carry the indel: as support, as anti-support, as multi-support, behind other entries, twice
    anti, multi = ref.READ_ANTI_SUPPORT, ref.READ_MULTI_SUPPORT
    carry = {0: [(T_P, 7)], 1: [(T_P, anti)], 2: [(T_P, multi)], 3: [(T_LOW, 5), (T_END, 9)], 4: [(T_LOW, 5), (T_P, 0)], 5: [(T_P, anti), (T_P, 7)],
             6: [(T_P, 7), (T_P, anti)], 7: [(T_END, anti), (T_P, anti)]}
    out.append(Case(reference, rb, [m(CAND_P - 50 + i) for i in range(9)], table, lst=[T_P], entries=carry))
    # 6 a read whose state says pos = -1, one with no bases
    out.append(Case(reference, rb, [m(CAND_P - 50), m(CAND_P - 49), m(CAND_P - 48)], table, lst=[T_P], state={0: None, 1: dict(l_qseq=0)}))
    # 7 max_read_size 100 and 250: with 250 the window begins in front of the empty bucket of 3
    long_read = rd(rb + 1500, cig(("M", 250)), reference[1500:1750])
    out.append(Case(reference, rb, [far] + chain[:1] + chain[2:] + [m(CAND_P - 190), m(CAND_P - 20), long_read], table, lst=[T_P]))
    # 8 the descent reaches bucket 0 from bucket 1
    low = rd(rb + 10, cig(("M", 50), ("D", 200), ("M", 50)), reference[10:60] + reference[260:310])
    out.append(Case(reference, rb, [low, m(60), m(240)], [ent(rb + 260, "I", "C", span=1)], lst=[0]))
    # 9 the descent stops at a bucket whose global maximum is exactly 50 in front of the indel
    reach = rd(P - 250, cig(("M", 50), ("D", 200), ("M", 50)), reference[CAND_P - 250:CAND_P - 200] + reference[CAND_P:CAND_P + 50])
    short = rd(P - 200, cig(("M", 30), ("D", 70), ("S", 50)), reference[CAND_P - 200:CAND_P - 170] + rand_ref(50, 18))  # (80 bases: max_read_size stays 100)
    out.append(Case(reference, rb, [short, reach, m(CAND_P - 40)], table, lst=[T_P]))
    return out


def facts_candidates(cs):
    P, S = cs[0].region_begin + CAND_P, CAND_SPAN
    e = [expected(c) for c in cs]
    assert sorted(i for i, _ in e[0]["pairs"]) == [1, 3, 5, 6, 8, 10, 14]  # each part of the test, on either side of its boundary; the two negative clips
    # 2: the four-part test takes the lone read, the bucket rule does not
    lone = e[1]["states"][0]
    assert lone["pos_end"] == P - 100 and lone["num_clipped_end"] == 50 and e[1]["taken"]["max_pos_end"][lone["bucket"]] == P - 50
    assert gtx.lib().gtx_disc_realign_wants(lone["pos"], lone["pos_end"], 0, 50, P, S) == 1 and [i for i, _ in e[1]["pairs"]] == [2]
    # 3: reached over full buckets, not over an empty one
    assert e[2]["states"][0]["pos_end"] == P and [i for i, _ in e[2]["pairs"]] == [0, 5] and [i for i, _ in e[3]["pairs"]] == [4]
    b_far = e[3]["states"][0]["bucket"]
    assert e[3]["taken"]["global_max_pos_end"][b_far + 2] == -1 and e[3]["taken"]["global_max_pos_end"][b_far + 1] > P - 50
    # 4: the clamp, and a window that begins in bucket 0
    c, t = cs[4], e[4]["taken"]
    assert (1990 + t["max_read_size"] + 100) // c.bucket_size > c.n_buckets - 1 and 150 - t["max_read_size"] - 100 < 0
    assert e[4]["pairs"] == [(1, 0), (2, 0), (3, 0), (4, 1)]
    assert [i for i, _ in e[5]["pairs"]] == [1, 3, 5, 7, 8]  # anti-support and other indels' entries do not keep a read out; the first entry decides
    assert [i for i, _ in e[6]["pairs"]] == [2]
    assert e[3]["taken"]["max_read_size"] == 100 and e[7]["taken"]["max_read_size"] == 250 and [i for i, _ in e[7]["pairs"]] == [0, 4]
    t = e[8]["taken"]
    assert (260 - t["max_read_size"] - 100) // cs[8].bucket_size == 1 and e[8]["states"][0]["bucket"] == 0 and [i for i, _ in e[8]["pairs"]] == [0, 2]
    t, reach = e[9]["taken"], e[9]["states"][1]
    assert t["global_max_pos_end"][16] == P - 50 and reach["bucket"] == 15 and t["max_pos_end"][15] == P + 50 and [i for i, _ in e[9]["pairs"]] == [2]
    assert gtx.lib().gtx_disc_realign_wants(reach["pos"], reach["pos_end"], 0, 0, P, S) == 1
    # the library's own four-part test agrees with the restatement on every read of these cases whose clips are not negative
    L = gtx.lib()
    for c, x in zip(cs, e):
        if len(c.table) <= T_P:
            continue
        for s in x["states"]:
            if s is not None and s["pos"] >= 0 and min(s["num_clipped_begin"], s["num_clipped_end"]) >= 0:
                r = dict(s, l_qseq=1)
                solo = dict(max_pos_end=[1 << 30], global_max_pos_end=[-1], bucket_reads=[[0]], max_read_size=100)
                want = ref.round_reads(c.table, T_P, solo, [r], [[]], c.table[T_P]["pos"] - 200, 1 << 20) == [0]
                assert bool(L.gtx_disc_realign_wants(s["pos"], s["pos_end"], s["num_clipped_begin"], s["num_clipped_end"], c.table[T_P]["pos"], c.table[T_P]["span"])) == want


def simulated_file(read_seed):
    """reads of graphtyper_amd/synth.py over a 3 kb region at 30x, with the CIGAR a mapper would give the reads over an indel site, a
    few soft clips, and the sites as a table -> (reference, region_begin, reads, table); the region is the same for every seed"""
    from graphtyper_amd import synth
    rb = 50000
    ref_idx = synth.make_reference(3000, seed=5)
    reference = synth.bases_to_str(ref_idx)
    records = synth.make_indel_records(ref_idx, every=180, seed=6, region_begin=rb)
    codes, pos = synth.make_reads(ref_idx, records, 600, seed=read_seed, region_begin=rb)
    sites, table = [], []
    for k, (p, r, alts, _) in enumerate(records):
        if len(alts[0]) > len(r):
            sites.append((p + 1, "I", alts[0][1:]))
        elif len(r) > len(alts[0]):
            sites.append((p + 1, "D", r[1:]))
        else:
            continue
        table.append(ent(p + 1, sites[-1][1], sites[-1][2], span=1 + k % 4, good=k % 2 == 0, file_index=(k // 3) % 2))
    reads = []
    for i in np.argsort(pos, kind="stable"):
        seq, start = "".join(NT16[c] for c in codes[i]), int(pos[i])
        site = next((s for s in sites if start + 10 <= s[0] <= start + 120), None)
        if site is not None and i % 3:
            a = site[0] - start
            ops = [("M", a), ("I", len(site[2])), ("M", 150 - a - len(site[2]))] if site[1] == "I" else [("M", a), ("D", len(site[2])), ("M", 150 - a)]
        elif i % 17 == 0:
            ops = [("S", 12), ("M", 138)] if i % 2 else [("M", 130), ("S", 20)]
        else:
            ops = [("M", 150)]
        reads.append(dict(rd(start, cig(*ops), seq), flag=int(1 + 2 * (i % 2) + 16 * (i % 5 == 0)), mapq=int(60 - i % 7)))
    return reference, rb, reads, table


def _simulated():
    reference, rb, reads, table = simulated_file(7)
    return [Case(reference, rb, reads, table, file_index=f) for f in (0, 1)]


SETS = dict(letters=_letters, group_edges=_group_edges, overruns=_overruns, long_deletion=_long_deletion, clips=_clips, ops=_ops, lookups=_lookups,
            stream_order=_stream_order, plan_rules=_plan_rules, candidates=_candidates, simulated=_simulated)


@functools.lru_cache(maxsize=None)
def cases(name):
    return SETS[name]()


# ---- what the sets are for --------------------------------------------------------------------------------------------------------
def scores(case):
    return [s and s["score"] for s in expected(case)["taken"]["reads"]]


def facts_letters(cs):
    assert [c.reference[0] for c in cs] == list(REGION_LETTERS)
    for c in cs:
        letter = c.reference[0]
        want = []
        for code in range(16):
            miss = NT16[code] != letter and NT16[code] != "N" and letter != "N"
            want += [40 - 5 * miss] * len(LETTER_OFFSETS)
        assert scores(c) == want
        assert sum(s == 35 for s in want) == 4 * {"N": 0, "Z": 15}.get(letter, 14)  # read A on region R is a mismatch, N on either side is none


def facts_group_edges(cs):
    assert [c.part.fill for c in cs] == [0, 15, 1] and all(c.part.stride == 64 for c in cs)
    for c in cs:
        seen = set()
        for r, s in zip(c.reads, expected(c)["taken"]["reads"]):
            span, clip = r["cigar"][-1] >> 4, len(r["seq"]) - (r["cigar"][-1] >> 4)
            assert s["score"] == span - 10 - (5 if clip else 0) and s["pos_end"] == r["pos"] + span
            seen.add((clip, (r["pos"] - c.region_begin) % 32, span))
        assert {x[0] for x in seen} == set(range(32)) and {x[1] for x in seen} == set(range(32)) and {x[2] for x in seen} == set(EDGE_SPANS)
    assert scores(cs[0]) == scores(cs[1]) == scores(cs[2])


def facts_overruns(cs):
    assert [c.region_begin for c in cs] == [0, BIG_BEGIN] and all(c.n_buckets == 4 for c in cs)
    for c in cs:
        x = expected(c)
        s, rb = x["taken"]["reads"], c.region_begin
        assert [s[i]["score"] for i in (0, 1, 2, 3, 4)] == [-40, -80, -40, -5, 0]
        assert [s[i]["pos_end"] - rb for i in (0, 1, 2, 3, 4)] == [110, 40, 115, 30, 60]
        assert [s[i]["score"] for i in (5, 6, 7, 8)] == [20 - 11, 20 - 16, 20, 12] and [s[i]["pos_end"] - rb for i in (5, 6, 7, 8)] == [31, 35, 35, 35]
        # the deletion that ends on REF_SIZE - 1 pays and leaves one base of the region to compare; the two others are dropped and pay nothing
        assert s[9]["score"] in (10 - 15 + 1, 10 - 15 - 4) and [s[i]["score"] for i in (10, 11)] == [10 - 20, 10 - 20]
        assert [s[i]["pos_end"] - rb for i in (9, 10, 11)] == [104, 95, 95]
        assert s[12]["score"] == -4 and s[12]["bucket"] == 3 and s[13:17] == [None] * 4
        assert [(r["score"], r["pos_end"] - rb, r["num_clipped_end"], r["flags"] & ref.IS_CLIPPED) for r in s[17:]] == [(10, 100, 0, 0)] * 2
        assert {e for e in x["taken"]["events"] if e[1] == "I"} == {(rb + 31, "I", "GATTA"), (rb + 30, "I", "GATTA")}  # (none at the region's end)
        # the insertion cut at the read's end is looked up by its five letters, the deletion that ends on REF_SIZE - 1 by its nine
        assert x["found"] == [True, False, True, False, False]


def facts_long_deletion(cs):
    c = cs[0]
    x = expected(c)
    assert c.n_buckets == 70 and x["taken"]["reads"][0]["score"] == 18 - 8 - (7 + LONG - 1) and x["taken"]["reads"][0]["pos_end"] == c.region_begin + 120 + LONG
    assert [len(e["seq"]) for e in c.table] == [LONG - 1, LONG] and x["found"] == [False, True]
    assert sum(len(b) > 0 for b in x["taken"]["bucket_reads"]) == 2 and x["lst"] == [1] and x["pairs"] == [(0, 0)]


def facts_clips(cs):
    s = expected(cs[0])["taken"]["reads"]
    assert [(r["num_clipped_begin"], r["num_clipped_end"]) for r in s] == list(CLIP_WANT)
    assert all(r["flags"] & ref.IS_CLIPPED for r in s) and [r["score"] for r in s[:7]] == [15, 15, 10, 10, 10, 15, 15]
    assert s[8]["pos_end"] + s[8]["num_clipped_end"] == s[8]["pos_end"] and expected(cs[0])["taken"]["max_pos_end"][1] == max(r["pos_end"] + r["num_clipped_end"] for r in s)


def facts_ops(cs):
    c = cs[0]
    s, rb = expected(c)["taken"]["reads"], c.region_begin
    by_op = {op: (s[op]["score"], s[op]["pos_end"] - rb) for op in range(16)}
    assert by_op[0][1] == 45 and by_op[7] == by_op[8] == by_op[0]  # = and X as M
    assert by_op[1] == (-11, 40) and by_op[2][1] == 45 and by_op[2][0] <= -11 and by_op[4] == (-5, 40)
    assert by_op[3][1] == 40 and all(by_op[op] == by_op[3] for op in (5, 6, 9, 10, 11, 12, 13, 14, 15))  # N and the rest move nothing
    assert not (s[3]["flags"] | s[5]["flags"]) & ref.IS_CLIPPED and s[4]["flags"] & ref.IS_CLIPPED
    assert [(r["score"], r["pos_end"] - rb) for r in s[16:]] == [(0, 40), (0, 40), (-6, 40), (-5, 40)]  # zero counts: D pays 7 + (0 - 1), S pays 5
    assert expected(c)["found"] == [True, True, True] and [e["seq"] for e in c.table][1] == ""  # the D of no bases is looked up as one


def facts_lookups(cs):
    assert expected(cs[0])["found"] == [True, True, False, True, False, True, False, True] and [e["seq"] for e in cs[0].table][3] == "ANT"
    # (table order: ..., the deletion at +90 whose last letter is wrong, I ANT, and at +150 I TT, I TTA, D 2 bases, D 3 bases, of which the
    # reads hold the second and the fourth)
    for c, what in zip(cs[1:], LOOKUP_MISSES):
        assert not any(expected(c)["found"]), what
        assert len(expected(c)["taken"]["events"]) == 1
    assert arrays(cs[0])["letters"][:4].tobytes().decode() == "ACG" + cs[0].reference[80]
    c = cs[3]
    assert c.reference[50:53] == "ACG" and next(iter(expected(c)["taken"]["events"])) == (c.region_begin + 50, "D", "ACG")  # differs from I ACG in type alone


def facts_stream_order(cs):
    t = expected(cs[0])["taken"]
    in_bucket_order, running = [], 0
    for b, m in enumerate(t["max_pos_end"]):
        running = max(running, m)
        in_bucket_order.append(running if t["bucket_reads"][b] else -1)
    assert t["global_max_pos_end"] != in_bucket_order and t["global_max_pos_end"][2] == 1150 and in_bucket_order[2] == 650
    full = [b for b, r in enumerate(t["bucket_reads"]) if r]
    assert full == [0, 2, 5, 10, 18] and t["bucket_reads"][2] == [1, 3] and t["bucket_reads"][5] == [2, 5]
    assert t["global_max_pos_end"][0] == 1465 and t["global_max_pos_end"][1] == -1
    t = expected(cs[1])["taken"]
    assert t["global_max_pos_end"][:3] == [0, -1, 140] and t["max_pos_end"][:3] == [0, -1, 140]


def facts_plan_rules(cs):
    c = cs[0]
    rb = c.region_begin
    ix = lambda at, kind, seq: c.index_of(rb + at, kind, seq)  # noqa: E731
    P, Q, R = 300, 600, 900
    x = [expected(k) for k in cs]
    assert x[0]["found"] == [i != ix(P + 10, "I", "TTT") for i in range(len(c.table))]
    # file 0: good first by position -- 60 on either side joins, 61 does not, nor the one the file does not hold; both others on Q; then its own
    assert x[0]["lst"] == [ix(P - 60, "I", "GT"), ix(P + 60, "D", c.reference[P + 60:P + 62]), ix(Q, "I", "CAT"), ix(Q, "D", c.reference[Q:Q + 2]), ix(P, "I", "AC"),
                           ix(Q, "I", "CA")]
    assert ref.table_order(c.table[ix(Q, "I", "CAT")]) < ref.table_order(c.table[ix(Q, "D", c.reference[Q:Q + 2])])  # a tie of position: table order
    assert x[1]["lst"] == [ix(R - 5, "I", "A"), ix(R, "D", c.reference[R:R + 4])] and x[2]["lst"] == [] and x[2]["pairs"] == []


def facts_simulated(cs):
    for c in cs:
        x = expected(c)
        assert len(c.reference) == 3000 and len(c.reads) == 600 and c.n_buckets == 60
        assert 4 <= sum(x["found"]) and len(x["lst"]) >= 2 and len(x["pairs"]) >= 50
        assert {"MIDNS"[w & 15] for r in c.reads for w in r["cigar"]} == set("MIDS")
    assert expected(cs[0])["lst"] != expected(cs[1])["lst"]


FACTS = dict(letters=facts_letters, group_edges=facts_group_edges, overruns=facts_overruns, long_deletion=facts_long_deletion, clips=facts_clips, ops=facts_ops,
             lookups=facts_lookups, stream_order=facts_stream_order, plan_rules=facts_plan_rules, candidates=facts_candidates, simulated=facts_simulated)
assert sorted(FACTS) == sorted(SETS)


# ---- launch shapes ----------------------------------------------------------------------------------------------------------------
SHAPE_READS = (1, 63, 64, 65, 257)
SHAPE_ENTRIES = 70


@functools.lru_cache(maxsize=None)
def shape_case(n_reads, bucket_size=150):
    """n_reads reads over a region of 300 bases and a table of SHAPE_ENTRIES indels one position apart, each in the list: with 257 reads a
    round runs over five steps of 64 reads, and the list gives slices of 0, 1, 64 and 65 entries"""
    reference, rb = rand_ref(300, 19), 700
    shapes = [rd(rb + 40 + 7 * j, cig(("M", 60 + 9 * j)), reference[40 + 7 * j:100 + 16 * j]) for j in range(8)] + [rd(rb - 3, cig(("M", 20)), "A" * 20)]
    reads = sorted((shapes[(i * 5) % len(shapes)] for i in range(n_reads)), key=lambda r: r["pos"]) if n_reads > 1 else [shapes[3]]
    table = [ent(rb + 60 + t, "I", "ACGT"[t % 4] * (1 + t % 3), span=1 + t % 5) for t in range(SHAPE_ENTRIES)]
    return Case(reference, rb, reads, table, bucket_size=bucket_size, lst=list(range(SHAPE_ENTRIES)))


# name -> (reads, bucket_size, k0, k1, pair_cap as an expression of `total` (the slice's pairs), the counters at entry, launches)
LAUNCHES = {"reads_%d" % n: (n, 150, 0, SHAPE_ENTRIES, "total", (0, 0), 1) for n in SHAPE_READS}
LAUNCHES.update(buckets_1=(65, 300, 0, SHAPE_ENTRIES, "total", (0, 0), 1), buckets_2=(65, 150, 0, SHAPE_ENTRIES, "total", (0, 0), 1),
                slice_0=(65, 50, 5, 5, "total", (0, 0), 1), slice_1=(65, 50, 5, 6, "total", (0, 0), 1), slice_64=(65, 50, 3, 67, "total", (0, 0), 1),
                slice_65=(65, 50, 5, 70, "total", (0, 0), 1), capacity_total=(257, 150, 0, SHAPE_ENTRIES, "total", (0, 0), 1),
                capacity_total_minus_1=(257, 150, 0, SHAPE_ENTRIES, "total - 1", (0, 0), 1), capacity_1=(257, 150, 0, SHAPE_ENTRIES, "1", (0, 0), 1),
                capacity_0=(257, 150, 0, SHAPE_ENTRIES, "0", (0, 0), 1), counters_7_3=(65, 150, 0, SHAPE_ENTRIES, "7 + total", (7, 3), 1),
                counters_7_3_one_short=(65, 150, 0, SHAPE_ENTRIES, "6 + total", (7, 3), 1), two_launches=(65, 150, 0, SHAPE_ENTRIES, "2 * total", (0, 0), 2),
                two_launches_one_short=(65, 150, 0, SHAPE_ENTRIES, "2 * total - 1", (0, 0), 2))
# (70 buckets: the set long_deletion)


def launch(name):
    """-> (case, k0, k1, pair_cap, counters at entry, launches)"""
    n_reads, bucket_size, k0, k1, cap, before, launches = LAUNCHES[name]
    case = shape_case(n_reads, bucket_size)
    return case, k0, k1, eval(cap, dict(total=len(pairs_of(case, k0, k1)))), before, launches


def facts_launches():
    big = shape_case(257)
    assert max(len(b) for b in expected(big)["taken"]["bucket_reads"]) > 128 and len(pairs_of(big, 0, SHAPE_ENTRIES)) > 64 * SHAPE_ENTRIES
    assert [shape_case(65, b).n_buckets for b in (300, 150, 50)] == [1, 2, 6]
    for name in LAUNCHES:
        case, k0, k1, cap, before, launches = launch(name)
        assert (k1 > k0) == (len(pairs_of(case, k0, k1)) > 0) and any(s is None for s in expected(case)["taken"]["reads"]) == (len(case.reads) > 8)


def judge(name, run):
    """None when the program behind `run` gives the set or launch shape `name` as the restatement says, else what differs"""
    if name in SETS:
        for k, case in enumerate(cases(name)):
            how = differs(case, through(run, case))
            if how is not None:
                return "case %d: %s" % (k, how)
        return None
    case, k0, k1, cap, before, launches = launch(name)
    return differs(case, through(run, case, k0, k1, cap, before, launches), k0, k1, cap, before, launches)
