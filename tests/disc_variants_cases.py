"""Case sets for discovery behind its second pass (graphtyper_amd/csrc/gtx_disc_variants.cpp: gtx_disc_variants and
gtx_disc_vcf_sites): hand-made merged results and good-bits at the smallest shapes at which the records, the base in front, the
window over the next events, the two id lists, the order of the file and its ID suffixes can go wrong -- and the end-to-end file
set of the region run (simulated_files).  A case is a region, an indel table, a haplotype map and the files' good-bits; its words
are written here (words_of), not by the library.  What a set is for is asserted from the restatement's output
(tests/disc_variants_ref.py) by its entry in FACTS: no set filters or skips a case.

    cases(name)     -> [Case]                          (made once)
    expected(case)  -> dict(recs, text): what the restatement says of it
    through(run, case) -> a case through tests/emu_disc_variants; through_lib(case) -> through the C ABI on a device -1 handle
    differs(case, got) -> None, or how `got` differs;  judge(name, run) -> the same for a whole set
All values are integers and letters; there is no tolerance."""
import ctypes as C
import functools
import struct

import numpy as np

import disc_variants_ref as ref
from disc_event_cases import cig, other, rand_ref, rd
from graphtyper_amd import lib as gtx

CONTIG = "chrT"


def ent(pos, kind, seq, good=False, span=1, file_index=0):
    return dict(pos=pos, type=kind, seq=seq, span=span, good=good, file_index=file_index)


def key(e):
    return (e["pos"], e["type"], e["seq"])


class Case:
    def __init__(self, reference, region_begin, table=(), haps=(), bits=None, contig=CONTIG):
        """table: indel entries (ent) in any order; haps: [(event, ever, always)] in any order, the sets as iterables of events; bits:
        the table entries (events) the files' second passes turned good, or None for a NULL array"""
        self.reference, self.region_begin, self.contig = reference, region_begin, contig
        self.table = sorted(table, key=lambda e: ref.event_order(key(e)))
        self.haps = sorted(((e, frozenset(ever), frozenset(always)) for e, ever, always in haps), key=lambda h: ref.event_order(h[0]))
        self.bits = None if bits is None else frozenset(bits)

    def final_good(self):
        return {key(e): bool(e["good"] or (self.bits is not None and key(e) in self.bits)) for e in self.table}

    def index_of(self, event):
        """an event's event_index in the map"""
        return 1 + [h[0] for h in self.haps].index(event)


# ---- the words, written here ------------------------------------------------------------------------------------------------------
def put_event(w, e):
    w.extend([e[0], ord(e[1]), len(e[2])])
    w.extend(ord(c) for c in e[2])


def words_of(table, haps):
    """the words of gtx_disc_merge (include/gtx.h: n_indels, per indel the event, 15 support fields, file_index, its phase entries;
    n_events, per event its "ever" and "always" sets, each in Event order)"""
    w = [len(table)]
    for e in table:
        put_event(w, key(e))
        # hq, lq, proper, first, reversed, clipped, max_mapq, max_distance, uniq_pos1..3, span, has_realignment_support, good, max_log_qual
        w.extend([9, 0, 5, 0, 4, 0, 60, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, e["span"], 1, int(e["good"]), 70])
        w.append(e["file_index"] & 0xFFFFFFFF)
        w.append(0)
    w.append(len(haps))
    for e, ever, always in haps:
        put_event(w, e)
        for s in (ever, always):
            w.append(len(s))
            for o in sorted(s, key=ref.event_order):
                put_event(w, o)
    return np.array(w, np.uint32)


def bits_words(case):
    if case.bits is None:
        return None
    w = np.zeros(max((len(case.table) + 31) // 32, 1), np.uint32)
    for t, e in enumerate(case.table):
        if key(e) in case.bits:
            w[t >> 5] |= np.uint32(1 << (t & 31))
    return w


@functools.lru_cache(maxsize=None)
def arrays(case):
    return dict(words=words_of(case.table, case.haps), bits=bits_words(case))


@functools.lru_cache(maxsize=None)
def expected(case):
    recs = ref.records(case.reference, case.region_begin, case.final_good(), case.haps)
    return dict(recs=recs, text=ref.sites_text(case.contig, recs).encode("latin-1"))


def record_arrays(recs):
    """the restatement's records in the library's layout -> (DISC_VARIANT array, letters, ids)"""
    out, letters, ids = np.zeros(len(recs), gtx.DISC_VARIANT), b"", []
    for i, r in enumerate(recs):
        ref_off = len(letters)
        letters += r["ref"].encode("latin-1")
        alt_off = len(letters)
        letters += r["alt"].encode("latin-1")
        hap_off = len(ids)
        ids.extend(r["hap"])
        anti_off = len(ids)
        ids.extend(r["anti"])
        out[i] = (r["pos"], r["gt_id"], ref_off, len(r["ref"]), alt_off, len(r["alt"]), hap_off, len(r["hap"]), anti_off, len(r["anti"]), ord(r["type"]), (0, 0, 0))
    return out, letters, np.array(ids, np.uint32)


def differs(case, got):
    """got: dict(recs, letters, ids, text) as the library leaves them -> None, or what differs from the restatement: field for field,
    byte for byte"""
    want = expected(case)
    recs, letters, ids = record_arrays(want["recs"])
    if len(got["recs"]) != len(recs):
        return "%d records, not %d" % (len(got["recs"]), len(recs))
    for i, (a, b) in enumerate(zip(got["recs"], recs)):
        if a.tobytes() != b.tobytes():
            return "record %d: %s, not %s" % (i, a, b)
    if bytes(got["letters"]) != letters:
        return "the letters"
    if np.asarray(got["ids"]).tolist() != ids.tolist():
        return "the ids"
    if bytes(got["text"]) != want["text"]:
        a, b = bytes(got["text"]).split(b"\n"), want["text"].split(b"\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        return "line %d of the text: %r, not %r" % (at, a[at:at + 1], b[at:at + 1])
    return None


# ---- through the C ABI and through the stand-alone program -----------------------------------------------------------------------
def host_handle(case):
    h = C.c_void_p()
    refb = case.reference.encode("latin-1")
    gtx.check(gtx.lib().gtx_disc_create(refb, len(refb), case.region_begin, -1, C.byref(h)))
    return h


def through_lib(case):
    a, h = arrays(case), host_handle(case)
    try:
        recs, letters, ids = gtx.disc_variants(h, a["words"], a["bits"])
    finally:
        gtx.lib().gtx_disc_destroy(h)
    return dict(recs=recs, letters=letters, ids=ids, text=gtx.disc_vcf_sites(recs, letters, ids, case.contig))


def write_case(path, case):
    """the input of tests/emu_disc_variants (its first lines)"""
    a = arrays(case)
    refb, contig = case.reference.encode("latin-1"), case.contig.encode()
    bits = a["bits"] if a["bits"] is not None else np.zeros(0, np.uint32)
    with open(path, "wb") as f:
        f.write(struct.pack("<qQQIII", case.region_begin, len(refb), len(a["words"]), int(a["bits"] is not None), len(bits), len(contig)))
        f.write(refb)
        f.write(a["words"].tobytes())
        f.write(bits.tobytes())
        f.write(contig)


SHORT = ("records", "letters", "ids", "text")  # the capacities the program also runs one short of


def read_result(path):
    raw = open(path, "rb").read()
    rc, n, n_letters, n_ids = struct.unpack_from("<IIQQ", raw, 0)
    at = 24
    out = dict(rc=rc)
    out["recs"] = np.frombuffer(raw, gtx.DISC_VARIANT, n, at)
    at += n * gtx.DISC_VARIANT.itemsize
    out["letters"] = raw[at:at + n_letters]
    at += n_letters
    out["ids"] = np.frombuffer(raw, np.uint32, n_ids, at)
    at += 4 * n_ids
    rc_text, n_text = struct.unpack_from("<IQ", raw, at)
    at += 12
    out["rc_text"], out["text"] = rc_text, raw[at:at + n_text]
    at += n_text
    out["short"] = {}
    for name in SHORT:
        out["short"][name] = struct.unpack_from("<iQQQI", raw, at)  # status (-1: not run, the size is 0), the three sizes or the length, untouched
        at += 32
    assert at == len(raw)
    return out


def through(run, case):
    """a case through tests/emu_disc_variants; run(write, read): emu_programs.run with a program and a directory"""
    return run(lambda path: write_case(path, case), read_result)


def short_differs(case, got):
    """the runs with one output one entry short: GTX_ERR_CAPACITY (5), the sizes all the same, nothing else written"""
    recs, letters, ids = record_arrays(expected(case)["recs"])
    sizes = dict(records=len(recs), letters=len(letters), ids=len(ids), text=len(expected(case)["text"]))
    for name in SHORT:
        status, a, b, c, untouched = got["short"][name]
        if sizes[name] == 0:
            if status != -1:
                return "%s: a run one short of nothing" % name
            continue
        want = (5, sizes["text"], 0, 0, 1) if name == "text" else (5, sizes["records"], sizes["letters"], sizes["ids"], 1)
        if (status, a, b, c, untouched) != want:
            return "one short in %s: %s, not %s" % (name, (status, a, b, c, untouched), want)
    return None


# ---- the sets -----------------------------------------------------------------------------------------------------------------------
def snp(reference, rb, pos, k=1):
    return (pos, "X", other(reference[pos - rb], k) if reference[pos - rb] in "ACGT" else "ACGT"[k % 4])


def ins(pos, seq):
    return (pos, "I", seq)


def dele(reference, rb, pos, n):
    return (pos, "D", reference[pos - rb:pos - rb + n])


def alone(events):
    return [(e, (), ()) for e in events]


def good_table(events, good=True):
    return [ent(e[0], e[1], e[2], good=good) for e in events if e[1] != "X"]


FRONT = "ACGTR"  # the letter in front of an indel, or under an SNP; R: none of A, C, G, T


def _kinds():
    """X, I and D with each of A / C / G / T, and a letter that is none of them, under or in front: events 200 apart, nothing relates"""
    out = []
    for rb in (0, 70000):
        base = list(rand_ref(3300, 41))
        events = []
        for k, letter in enumerate(FRONT):
            for j, kind in enumerate("XID"):
                p = 200 * (3 * k + j) + 100
                base[p - (kind != "X")] = letter
                events.append((kind, rb + p))
        reference = "".join(base)
        evs = [snp(reference, rb, p, 1 + k % 3) if kind == "X" else ins(p, "GA"[:1 + k % 2] + "T" * (k % 3)) if kind == "I" else dele(reference, rb, p, 1 + k % 3)
               for k, (kind, p) in enumerate(events)]
        out.append(Case(reference, rb, good_table(evs), alone(evs)))
    return out


def _first_base():
    """an insertion and a deletion at the region's first position (no base in front inside the region: the text's failure return),
    beside the same two one position on (the base in front is the region's first), for a region at 0 and one elsewhere; and an
    insertion at the position behind the region's last base, whose base in front is the last"""
    out = []
    for rb in (0, 12345):
        reference = rand_ref(400, 43)
        for evs in ([ins(rb, "C")], [ins(rb, "CAG")], [dele(reference, rb, rb, 2)], [ins(rb, "TT"), dele(reference, rb, rb, 3), snp(reference, rb, rb)],
                    [ins(rb + 1, "G"), dele(reference, rb, rb + 1, 2)], [ins(rb + len(reference), "A")], [ins(rb + len(reference) + 1, "A")]):
            out.append(Case(reference, rb, good_table(evs), alone(evs)))
    return out


def _dropped():
    rb = 3000
    reference = rand_ref(900, 44)
    a, bad, c = snp(reference, rb, rb + 100), dele(reference, rb, rb + 130, 2), snp(reference, rb, rb + 160)
    d = ins(rb + 180, "AC")
    out = []
    # a bad indel between two kept events: the id behind it is named by the event in front, and the GT_IDs have a gap
    out.append(Case(reference, rb, good_table([bad], False) + good_table([d]), alone([a, bad, c, d])))
    # bad in the table but set in good_bits: kept
    out.append(Case(reference, rb, good_table([bad], False) + good_table([d]), alone([a, bad, c, d]), bits=[bad]))
    # good_bits given and empty, and a bit for an entry that is good already
    out.append(Case(reference, rb, good_table([bad], False) + good_table([d]), alone([a, bad, c, d]), bits=[]))
    out.append(Case(reference, rb, good_table([bad], False) + good_table([d]), alone([a, bad, c, d]), bits=[d]))
    # absent from the table: the assert's other arm
    out.append(Case(reference, rb, good_table([d]), alone([a, bad, c, d])))
    # the first and the last event of the map dropped; every indel dropped; more than 32 table entries with the bit in the second word
    out.append(Case(reference, rb, good_table([bad, d], False), alone([bad, c, d])))
    out.append(Case(reference, rb, good_table([bad, d], False), alone([bad, d])))
    many = [ins(rb + 10 + 20 * k, "A" * (1 + k % 3)) for k in range(40)]
    out.append(Case(reference, rb, good_table(many, False), alone(many), bits=[many[33], many[0], many[31], many[32]]))
    return out


def _window():
    """next events at +99, +100 and +101 of an SNP, of an insertion and of a deletion: the scan ends at next.pos >= pos + 100 of the
    EVENT's position (not the record's, which is one down for an indel)"""
    rb = 500
    reference = rand_ref(1200, 45)
    out = []
    for first in (snp(reference, rb, rb + 50), ins(rb + 50, "GG"), dele(reference, rb, rb + 50, 2)):
        nxt = [snp(reference, rb, rb + 50 + d) for d in (99, 100, 101)]
        out.append(Case(reference, rb, good_table([first]), alone([first] + nxt)))
        out.append(Case(reference, rb, good_table([first]), alone([first, nxt[1]])))
        near = [ins(rb + 50 + 99, "T"), dele(reference, rb, rb + 50 + 100, 1)]
        out.append(Case(reference, rb, good_table([first] + near), alone([first] + near)))
    return out


def _sets():
    rb = 0
    reference = rand_ref(700, 46)
    a = snp(reference, rb, 100)
    always, ever_only, neither = snp(reference, rb, 105), snp(reference, rb, 120), snp(reference, rb, 150)
    bad = ins(108, "CC")
    good = dele(reference, rb, 140, 3)
    haps = [(a, [always, ever_only, bad, good], [always, bad]),  # bad: a dropped indel that sits in `always` -- and is named nowhere
            (always, [ever_only], []), (ever_only, [], []), (neither, [], []), (bad, [good], [good]), (good, [neither], [neither])]
    out = [Case(reference, rb, good_table([bad], False) + good_table([good]), haps)]
    # the same with the indel kept: now it is named, and it names
    out.append(Case(reference, rb, good_table([bad], False) + good_table([good]), haps, bits=[bad]))
    # `always` without `ever` (the merge can leave that): GT_HAPLOTYPE all the same -- `always` is looked at first
    out.append(Case(reference, rb, (), [(a, [], [always]), (always, [], [])]))
    # sets that name events which are not in the map, or lie in front
    ghost = snp(reference, rb, 110, 2)
    out.append(Case(reference, rb, (), [(a, [ghost], [ghost]), (always, [a], [a])]))
    return out


def _same_place():
    rb = 900
    reference = rand_ref(600, 47)
    p = rb + 200
    two = [snp(reference, rb, p, 1), snp(reference, rb, p, 2)]
    three = two + [snp(reference, rb, p, 3)]
    indels = [ins(p + 1, "AG"), dele(reference, rb, p + 1, 2)]
    out = [Case(reference, rb, (), alone(two)), Case(reference, rb, (), alone(three)), Case(reference, rb, good_table(indels), alone(indels)),
           # an SNP at p beside an insertion and a deletion at p + 1: one POS, three kinds
           Case(reference, rb, good_table(indels), alone(two[:1] + indels)),
           # two insertions and two deletions of one place: the shorter REF / ALT first, and the suffixes run on over both kinds (one type code)
           Case(reference, rb, good_table(indels + [ins(p + 1, "A"), dele(reference, rb, p + 1, 1)]), alone(three + indels + [ins(p + 1, "A"), dele(reference, rb, p + 1, 1)])),
           # an insertion of one letter at the region's first base: its type code is the SNP's, so it shares the SNPs' suffixes
           Case(reference, rb, good_table([ins(rb, "G")]), alone([ins(rb, "G"), snp(reference, rb, rb, 1), snp(reference, rb, rb, 2)]))]
    # equal in everything but the number of INFO keys: cannot come from one map (the alleles name the event); the sort's last key is
    # reached through records handed to gtx_disc_vcf_sites directly (test_disc_variants.py)
    return out


WIDE = 16000  # vcf.cpp:797


def _wide():
    """deletions whose REF + ALT have 16 000 letters (written) and more (left out of the text, present in the records), the long one
    with a neighbour of its place and type behind it"""
    rb = 100
    reference = rand_ref(WIDE + 300, 48)
    p = rb + 50
    at_limit, over = dele(reference, rb, p, WIDE - 2), dele(reference, rb, p + 5, WIDE - 1)  # REF has one letter more, ALT one
    small, other_ins = dele(reference, rb, p + 5, 1), ins(p + 5, "T")
    evs = [at_limit, over, small, other_ins, snp(reference, rb, p + 2)]
    return [Case(reference, rb, good_table(evs), alone(evs)), Case(reference, rb, good_table([over]), alone([over]))]


def _many():
    """1 100 SNPs seven positions apart (up to 14 next events each) with sets drawn at random, an indel every tenth place: ids of four digits"""
    rb = 20000
    reference = rand_ref(8000, 49)
    rng = np.random.default_rng(50)
    evs = []
    for k in range(1100):
        p = rb + 20 + 7 * k
        evs.append(snp(reference, rb, p, 1 + k % 3) if k % 10 else (ins(p, "ACG"[:1 + k % 3]) if k % 20 else dele(reference, rb, p, 2)))
    haps = []
    for i, e in enumerate(evs):
        nxt = [o for o in evs[i + 1:i + 20] if o[0] < e[0] + 120]
        draw = rng.integers(0, 3, len(nxt))
        haps.append((e, [o for o, d in zip(nxt, draw) if d > 0], [o for o, d in zip(nxt, draw) if d == 2]))
    indels = [e for e in evs if e[1] != "X"]
    table = [ent(e[0], e[1], e[2], good=k % 3 == 0) for k, e in enumerate(indels)]
    return [Case(reference, rb, table, haps, bits=[e for k, e in enumerate(indels) if k % 3 == 1])]


SETS = dict(kinds=_kinds, first_base=_first_base, dropped=_dropped, window=_window, sets=_sets, same_place=_same_place, wide=_wide, many=_many)


@functools.lru_cache(maxsize=None)
def cases(name):
    return SETS[name]()


# ---- what the sets are for --------------------------------------------------------------------------------------------------------
def lines(case):
    return expected(case)["text"].decode("latin-1").split("\n")[1:-1]


def facts_kinds(cs):
    for c in cs:
        recs = expected(c)["recs"]
        assert len(recs) == 15 and [r["gt_id"] for r in recs] == list(range(1, 16)) and not any(r["hap"] or r["anti"] for r in recs)
        seen = set()
        for r in recs:
            at = r["pos"] - c.region_begin
            letter = c.reference[at]
            seen.add((r["type"], letter))
            if r["type"] == "X":
                assert r["ref"] == letter and len(r["alt"]) == 1 and r["alt"] != letter  # (the region's letter as it is, R too)
            else:
                front = letter if letter in "ACGT" else "N"
                assert r["ref"][0] == front and r["alt"][0] == front and (len(r["ref"]) == 1) != (len(r["alt"]) == 1)
                assert (r["type"] == "I") == (len(r["alt"]) > 1)
        assert seen == {(k, f) for k in "XID" for f in FRONT}
        assert len(lines(c)) == 15 and all("\tN" in ln for ln in lines(c) if ":IG" in ln and c.reference[int(ln.split("\t")[1]) - 1 - c.region_begin] == "R")


def facts_first_base(cs):
    empty = 0
    for c in cs:
        for r in expected(c)["recs"]:
            if r["type"] == "X":
                continue
            event_pos = c.haps[r["gt_id"] - 1][0][0]
            inside = c.region_begin < event_pos <= c.region_begin + len(c.reference)
            if inside:  # the base in front is in the region: the first or the last base included
                assert r["pos"] == event_pos - 1 and r["ref"][0] == r["alt"][0] == c.reference[event_pos - 1 - c.region_begin]
            else:  # the failure return: an empty allele, the event's own position
                assert r["pos"] == event_pos and "" in (r["ref"], r["alt"])
                empty += 1
    assert empty == 2 * 6 and {c.region_begin for c in cs} == {0, 12345}
    texts = [expected(c)["text"] for c in cs]
    assert any(b"\t\tC\t0" in t for t in texts) and any(b":SG\t\tC" in t for t in texts) and any(b":IG\t\tCAG" in t for t in texts)  # an empty REF column
    assert any(t.count(b"\t\t0\t.") == 1 for t in texts)  # an empty ALT column: the deletion


def facts_dropped(cs):
    first, by_bit, empty_bits, other_bit, absent = (expected(c)["recs"] for c in cs[:5])
    assert [r["gt_id"] for r in first] == [1, 3, 4] and first[0]["anti"] == [3, 4]  # the gap; the ids behind the dropped one are its neighbours'
    assert [r["gt_id"] for r in by_bit] == [1, 2, 3, 4] and by_bit[0]["anti"] == [2, 3, 4]
    assert empty_bits == first and other_bit == first and absent == first
    assert cs[4].table != cs[0].table and len(cs[4].table) == 1
    assert [r["gt_id"] for r in expected(cs[5])["recs"]] == [2] and expected(cs[6])["recs"] == [] and expected(cs[6])["text"] == ref.COLUMNS.encode()
    assert [r["gt_id"] for r in expected(cs[7])["recs"]] == [1, 32, 33, 34] and len(cs[7].table) == 40


def facts_window(cs):
    for k, c in enumerate(cs):
        recs = expected(c)["recs"]
        assert recs[0]["hap"] == [] and recs[0]["anti"] == ([2] if k % 3 != 1 else [])  # +99 is in, +100 ends the scan, +101 is never seen
        assert len(c.haps) == (4, 2, 3)[k % 3]
    assert [expected(c)["recs"][0]["type"] for c in cs] == ["X"] * 3 + ["I"] * 3 + ["D"] * 3
    assert expected(cs[3])["recs"][0]["pos"] == cs[3].haps[0][0][0] - 1  # the record is one down, the window is the event's


def facts_sets(cs):
    dropped, kept, always_only, ghosts = (expected(c)["recs"] for c in cs)
    a = dropped[0]
    # always -> GT_HAPLOTYPE; ever only -> nowhere; neither -> GT_ANTI_HAPLOTYPE; the dropped indel in `always` -> nowhere
    assert [r["gt_id"] for r in dropped] == [1, 2, 4, 5, 6] and a["hap"] == [2] and a["anti"] == [6]
    assert cs[0].index_of(cs[0].haps[2][0]) == 3 and cs[0].haps[2][0][1] == "I"
    assert [r["gt_id"] for r in kept] == [1, 2, 3, 4, 5, 6] and kept[0]["hap"] == [2, 3] and kept[0]["anti"] == [6] and kept[2]["hap"] == [5]
    assert always_only[0]["hap"] == [2] and always_only[0]["anti"] == []
    assert ghosts[0]["hap"] == [] and ghosts[0]["anti"] == [2] and ghosts[1]["hap"] == ghosts[1]["anti"] == []
    assert b"GT_ANTI_HAPLOTYPE=6;GT_HAPLOTYPE=2;GT_ID=1\n" in expected(cs[0])["text"]


def facts_same_place(cs):
    def ids(c):
        return [ln.split("\t")[2] for ln in lines(c)]
    p = cs[0].haps[0][0][0] + 1
    assert ids(cs[0]) == ["chrT:%d:SG" % p, "chrT:%d:SG.0" % p] and ids(cs[1]) == ids(cs[0]) + ["chrT:%d:SG.1" % p]
    assert ids(cs[2]) == ["chrT:%d:IG" % p, "chrT:%d:IG.0" % p] and [ln.split("\t")[3:5] for ln in lines(cs[2])][0][0] == cs[2].reference[p - 1 - cs[2].region_begin]
    assert ids(cs[3]) == ["chrT:%d:SG" % p, "chrT:%d:IG" % p, "chrT:%d:IG.0" % p] and len({ln.split("\t")[1] for ln in lines(cs[3])}) == 1
    assert ids(cs[4]) == ["chrT:%d:SG" % p, "chrT:%d:SG.0" % p, "chrT:%d:SG.1" % p] + ["chrT:%d:IG" % p] + ["chrT:%d:IG.%d" % (p, k) for k in range(3)]
    alts = [ln.split("\t")[3:5] for ln in lines(cs[4])][3:]
    assert [len(a[1]) for a in alts[:2]] == [2, 3] and [len(a[0]) for a in alts[2:]] == [2, 3]  # insertions in front of deletions, the shorter first
    first = cs[5].region_begin + 1
    assert ids(cs[5]) == ["chrT:%d:SG" % first, "chrT:%d:SG.0" % first, "chrT:%d:SG.1" % first] and lines(cs[5])[2].split("\t")[3:5] == ["", "G"]  # (SNPs first)


def facts_wide(cs):
    recs = expected(cs[0])["recs"]
    sizes = sorted(len(r["ref"]) + len(r["alt"]) for r in recs)
    assert sizes[-2:] == [WIDE, WIDE + 1] and len(recs) == 5 and len(lines(cs[0])) == 4
    ids = [ln.split("\t")[2] for ln in lines(cs[0])]
    p = cs[0].region_begin + 50
    # behind the insertion of its place the short deletion is .0; the long one would have been .1
    assert ids == ["chrT:%d:IG" % p, "chrT:%d:SG" % (p + 3), "chrT:%d:IG" % (p + 5), "chrT:%d:IG.0" % (p + 5)]
    assert len(lines(cs[0])[0].split("\t")[3]) == WIDE - 1
    assert len(expected(cs[1])["recs"]) == 1 and expected(cs[1])["text"] == ref.COLUMNS.encode()


def facts_many(cs):
    (c,) = cs
    recs = expected(c)["recs"]
    assert len(c.haps) == 1100 and 1000 < len(recs) < 1100 and recs[-1]["gt_id"] == 1100
    assert 10 <= max(len(r["hap"]) + len(r["anti"]) for r in recs) <= 14 and any(i >= 1000 for r in recs for i in r["hap"]) and any(i >= 1000 for r in recs for i in r["anti"])
    assert sum(1 for r in recs if r["type"] != "X") == len([e for e in c.table if c.final_good()[key(e)]]) == 74
    assert b"GT_ID=1100\n" in expected(c)["text"]


FACTS = dict(kinds=facts_kinds, first_base=facts_first_base, dropped=facts_dropped, window=facts_window, sets=facts_sets, same_place=facts_same_place,
             wide=facts_wide, many=facts_many)


def judge(name, run):
    """None when the program behind `run` gives the set `name` as the restatement says -- the records, the text, and GTX_ERR_CAPACITY
    with nothing written for every output one entry short --, else what differs"""
    for k, case in enumerate(cases(name)):
        got = through(run, case)
        how = ("status %d / %d" % (got["rc"], got["rc_text"])) if (got["rc"], got["rc_text"]) != (0, 0) else differs(case, got) or short_differs(case, got)
        if how is not None:
            return "case %d: %s" % (k, how)
    return None



# ---- the end-to-end file set: three files over one region, for gtx_discover_region --------------------------------------------------
E2E_BEGIN = 50000
E2E_LENGTH = 3000
E2E_SITES = 2000  # the sites lie in the region's first 2 kb: every site costs the restatement its reads' alignments
E2E_EVERY = 40
E2E_SNP_EVERY = 160  # an SNP eight positions behind every fourth site: close enough to be always together
E2E_FILES = ((14, 420), (18, 260), (37, 120))  # (seed, reads): three samples at about 21x, 13x and 6x
NT16 = "=ACMGRSVTWYHKDBN"


def second_haplotype(ref_idx, records, seed, region_begin):
    """the sample's second haplotype as synth.make_reads builds it -- rebuilt here from that function's first draw (which records the
    sample carries) -> (its base indices, under each the region offset of the reference base it is aligned to, -1: inserted).
    facts_simulated holds every read to its CIGAR, so a change of that draw would be noticed."""
    take = np.random.default_rng(seed).random(len(records)) < 0.5
    hap, at, cur = [], [], 0
    for (p, r, alts, _), t in zip(records, take):
        p -= region_begin
        hap.extend(ref_idx[cur:p])
        at.extend(range(cur, p))
        alt = alts[0] if t else r
        hap.extend("ACGT".index(c) for c in alt)
        at.extend([p] + [-1] * (len(alt) - 1) if len(alt) > len(r) else range(p, p + len(alt)))
        cur = p + len(r)
    hap.extend(ref_idx[cur:])
    at.extend(range(cur, len(ref_idx)))
    return np.array(hap, np.uint8), np.array(at)


def runs_of(at):
    """the aligned reference offsets of a read's bases (-1: inserted) -> (the offset of its first aligned base, [[operation, count]]): no
    gap within five bases of an end -- what lies outside such an indel is clipped, as a mapper clips it"""
    runs, p = [], None
    for a in at:
        if a != -1 and p is not None and a > p + 1:
            runs.append(["D", int(a) - p - 1])
        op = "I" if a == -1 else "M"
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
        p = int(a) if a != -1 else p
    start = int(next(a for a in at if a != -1))
    lead = tail = 0
    while runs[0][0] != "M" or runs[0][1] <= 5:
        op, k = runs.pop(0)
        lead += k if op != "D" else 0
        start += k if op != "I" else 0
    while runs[-1][0] != "M" or runs[-1][1] <= 5:
        op, k = runs.pop()
        tail += k if op != "D" else 0
    return start, ([["S", lead]] if lead else []) + runs + ([["S", tail]] if tail else [])


def mapped_reads(ref_idx, records, n, seed, region_begin):
    """n reads of synth.make_reads with the CIGAR a mapper gives each: a read of the sample's second haplotype carries the insertions
    and deletions it covers (runs_of); every other read is one M"""
    from graphtyper_amd import synth
    codes, pos = synth.make_reads(ref_idx, records, n, seed=seed, region_begin=region_begin)
    hap, at = second_haplotype(ref_idx, records, seed, region_begin)
    hap_codes, ref_codes = (1 << hap).astype(np.uint8), (1 << ref_idx).astype(np.uint8)
    first_at = {}
    for s, a in enumerate(at):  # where on the second haplotype a read with a given POS may begin: at the base, or in the insertion behind it
        if a != -1:
            last = a
        first_at.setdefault(int(last), []).append(s)
    reads = []
    for i in np.argsort(pos, kind="stable"):
        row, start = codes[i], int(pos[i]) - region_begin
        known = row != 15
        plain = int(((ref_codes[start:start + len(row)] != row) & known).sum()) if start + len(row) <= len(ref_idx) else len(row)
        fits = [(int(((hap_codes[s:s + len(row)] != row) & known).sum()), s) for s in first_at.get(start, ()) if s + len(row) <= len(hap)]
        ops = [["M", len(row)]]
        if fits and min(fits)[0] < plain:
            s = min(fits)[1]
            start, ops = runs_of(at[s:s + len(row)])
        seq = "".join(NT16[c] for c in row)
        reads.append(dict(rd(start + region_begin, cig(*[(o, k) for o, k in ops]), seq), flag=int(1 + 2 * (i % 2 == 0) + 16 * (i % 3 == 0) + 64 * (i % 4 < 2)),
                          mapq=int(60 - i % 7)))
    reads.sort(key=lambda r: r["pos"])
    return reads


@functools.lru_cache(maxsize=None)
def simulated_files():
    """-> (reference, region_begin, [the reads of each file]): one region of 3 kb with an SNP, an insertion or a deletion every 40
    positions of its first 2 kb (synth.make_indel_records) and an SNP eight positions behind every fourth of them
    (synth.make_snp_records), three samples that each carry their own half of the sites, at three depths"""
    from graphtyper_amd import synth
    ref_idx = synth.make_reference(E2E_LENGTH, seed=5)
    records = synth.make_indel_records(ref_idx[:E2E_SITES], every=E2E_EVERY, seed=6, region_begin=E2E_BEGIN)
    records += synth.make_snp_records(ref_idx[:E2E_SITES], every=E2E_SNP_EVERY, seed=7, region_begin=E2E_BEGIN, first=E2E_EVERY // 2 + 2 * E2E_EVERY + 8)
    records.sort(key=lambda r: r[0])
    return synth.bases_to_str(ref_idx), E2E_BEGIN, [mapped_reads(ref_idx, records, n, seed, E2E_BEGIN) for seed, n in E2E_FILES]


def facts_simulated(hc):
    """what the end-to-end set is for, over host_chain()'s result"""
    table, good, recs, haps = hc["table"], hc["good"], hc["recs"], hc["haps"]
    assert len(hc["files"]) == 3 and len(hc["reference"]) == E2E_LENGTH
    # every read is the haplotype its CIGAR says: a mapper's alignment, not a guess
    for reads in hc["files"]:
        for r in reads:
            at, q, miss = r["pos"] - hc["region_begin"], 0, 0
            for w in r["cigar"]:
                op, n = "MIDNSHP=X"[w & 15], w >> 4
                if op == "M":
                    miss += sum(1 for a, b in zip(hc["reference"][at:at + n], r["seq"][q:q + n]) if a != b and b != "N")
                at += n if op in "MD" else 0
                q += n if op in "MIS" else 0
            assert q == len(r["seq"]) and miss <= 12, (r["pos"], miss)
    assert sum(1 for e in table if e["good"]) >= 1  # an indel good at the merge
    turned = [t for t, e in enumerate(table) if not e["good"] and good[t]]
    assert len(turned) >= 1 and all(any(w["good"][t] and t in w["lst"] for w in hc["wants"]) for t in turned)  # bad at the merge, good after its file's rounds
    final = {key(e): g for e, g in zip(table, good)}
    events = [h[0] for h in haps]

    def kept(e):
        return e[1] == "X" or final.get(e, False)
    # bad to the end, and therefore dropped, with a kept event behind it inside another record's window
    assert any(kept(x) and any(not kept(events[j]) and events[j][0] < x[0] + 100 and any(kept(events[k]) and events[k][0] < x[0] + 100 for k in range(j + 1, len(events)))
                               for j in range(i + 1, len(events))) for i, x in enumerate(events))
    assert [r["gt_id"] for r in recs] != list(range(1, len(recs) + 1))  # (the ids have gaps)
    assert any(r["hap"] for r in recs) and any(r["anti"] for r in recs)
    assert all(len(w["lst"]) > 0 for w in hc["wants"]) and sum(w["trace"]["refused"] for w in hc["wants"]) == 0 and sum(w["trace"]["aligned"] for w in hc["wants"]) > 50
    assert hc["text"].count(b"\n") == 1 + len(recs)


@functools.lru_cache(maxsize=None)
def host_chain():
    """the region run on the host through what exists: the oracle's first pass and merge (test_discovery.oracle_full / oracle_merge),
    the restatement of each file's second pass (disc_rounds_cases.expected), then the records and the text of this module's restatement
    -> dict(reference, region_begin, files, merged [words], table [ent], wants [per file, disc_rounds_cases.expected], good [per table
            entry, final], haps, recs, text)"""
    import disc_rounds_cases as rc
    import disc_second_cases as sc
    import test_discovery as td
    reference, rb, files = simulated_files()
    merged = None
    for f, reads in enumerate(files):
        words = td.oracle_full(reference, rb, reads, file_i=f)[0]
        merged = words if merged is None else td.oracle_merge(merged, words)
    entries, letters = gtx.disc_indel_table(merged)
    table = [ent(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), bool(e["good"]), int(e["span"]), int(e["file_index"]))
             for e in entries]
    wants = [rc.expected(sc.Case(reference, rb, reads, table, file_index=f)) for f, reads in enumerate(files)]
    good = [bool(e["good"]) or any(w["good"][t] for w in wants) for t, e in enumerate(table)]
    haps = sorted(((e, frozenset(sets[0]), frozenset(sets[1])) for e, sets in td.parse_result(merged)[1].items()), key=lambda h: ref.event_order(h[0]))
    recs = ref.records(reference, rb, {key(e): g for e, g in zip(table, good)}, haps)
    return dict(reference=reference, region_begin=rb, files=files, merged=merged, table=table, wants=wants, good=good, haps=haps, recs=recs,
                text=ref.sites_text(CONTIG, recs).encode("latin-1"))
