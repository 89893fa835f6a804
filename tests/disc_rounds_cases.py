"""Case sets for the second pass from the aligner on (graphtyper_amd/csrc/gtx_disc_rounds_dev.hpp): small files -- a region of 1 to 3
kb, at most about 200 reads, at most 20 list entries -- at which the rounds, the windows, the decision, the lists, the counters and
the final decision can go wrong.  A case is a disc_second_cases.Case (a region, its reads in stream order, the indel table, the
list); every case starts where the intake leaves it: no entries, counters of zero.  What a set is for is asserted from the
restatement's trace (tests/disc_rounds_ref.py) in tests/test_disc_rounds_cases.py: no set filters or skips a case.

    cases(name)      -> [Case]                       (made once)
    expected(case)   -> what the restatement says: the reads' final state and lists, the counters, the trace, the good-bits, and the
                        state in front of every round (made once per case)
    witness(case)    -> the same from the library's host pieces strung by a loop, the counters counted off the lists
    room(case)       -> the event array's model: per round the entries in use in front of it and the size of its new lists
    judge(name, run) -> None, or how the program behind `run` (a build of tests/emu_disc_rounds) differs on the set, the round shape,
                        the launch shape or the final decision `name` (NAMES): what tests/test_disc_rounds_emu.py asserts and what
                        the mutation audit (tests/disc_rounds_mutants) asks of a changed header
The sets copies, search, own_ends, purity and fields are made for the windows' text (apply_event): scene() builds them.
All values are integers or bits; there is no tolerance."""
import copy
import ctypes as C
import functools

import numpy as np

import disc_rounds_ref as ref
import disc_second_cases as sc
import realign_ref as realign
from disc_event_cases import cig, rand_ref, rd
from disc_second_cases import Case, ent
from graphtyper_amd import lib as gtx

OUTCOME = {realign.NO_PADDING: "NO_PADDING", realign.BETTER: "BETTER", realign.SAME_OVERLAPPING: "SAME_OVERLAPPING", realign.SAME: "SAME",
           realign.WORSE: "WORSE", "refused": "refused"}


def sequences(case):
    return [r["seq"] for r in case.reads]


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> dict(lst, taken, states, entries, support, trace, good, before [per round k: (states, entries, support) in front of it, and
    one more: the end])"""
    want = sc.expected(case)
    states, entries = copy.deepcopy(want["states"]), [[] for _ in case.reads]
    support = ref.clear_support(case.table)
    before = [copy.deepcopy((states, entries, support))]
    trace = ref.rounds(case.reference, case.region_begin, case.bucket_size, case.table, want["lst"], 0, len(want["lst"]), want["taken"], states, entries, support,
                       sequences(case), after_round=lambda k: before.append(copy.deepcopy((states, entries, support))))
    return dict(lst=want["lst"], taken=want["taken"], states=states, entries=entries, support=support, trace=trace,
                good=ref.good_after(case.table, want["lst"], support), before=before)


def room(case):
    """the event array as gtx.h states it: per round (entries the reads hold in front of it, entries of its new lists); a run needs
    max(live + new) entries, and with fewer stops in front of the first round whose live + new does not fit"""
    want = expected(case)
    out = []
    for k in range(len(want["lst"])):
        entries_before, entries_after = want["before"][k][1], want["before"][k + 1][1]
        live = sum(len(e) for e in entries_before)
        new = sum(len(b) for a, b in zip(entries_before, entries_after) if a != b)
        out.append((live, new))
    return out


# ---- the second witness: the library's host pieces strung by a loop -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness(case):
    """gtx_disc_realign_wants, gtx_disc_realign_target and gtx_disc_realign_decide (host code, a gtx_disc without a device) around
    realign_ref's alignment.  The lists are kept as the text has them; the counters are NOT kept along the way but counted off the
    lists at the end (an entry's holders), max_mapq off every list a read ever had.
    -> dict(states, entries, support, aligned, refused, skipped)"""
    L = gtx.lib()
    want = sc.expected(case)
    table, lst, taken = case.table, want["lst"], want["taken"]
    states, entries = copy.deepcopy(want["states"]), [[] for _ in case.reads]
    seqs = sequences(case)
    ever = [set() for _ in table]  # per entry: the mapq values of the reads that ever held it with read_pos >= 0
    h = C.c_void_p()
    refb = case.reference.encode("latin-1")
    gtx.check(L.gtx_disc_create(refb, len(refb), case.region_begin, -1, C.byref(h)))
    aligned = refused = skipped = 0
    try:
        for k, t in enumerate(lst):
            indel = table[t]
            this = (indel["pos"], indel["type"], indel["seq"])
            begin = max(0, indel["pos"] - taken["max_read_size"] - 100 - case.region_begin)
            if begin >= len(case.reference) or indel["pos"] + taken["max_read_size"] + 100 - case.region_begin < begin or gtx.disc_realign_target(h, taken["max_read_size"], [this])[3] == 0:
                skipped += 1
                continue
            for i in sc.ref.round_reads(table, t, taken, states, entries, case.region_begin, case.bucket_size):
                s = states[i]
                assert L.gtx_disc_realign_wants(s["pos"], s["pos_end"], s["num_clipped_begin"], s["num_clipped_end"], indel["pos"], indel["span"]) == 1
                own = [(table[te]["pos"], table[te]["type"], table[te]["seq"]) for te, _ in entries[i]]
                letters, ref_pos, begin_padded, bits = gtx.disc_realign_target(h, taken["max_read_size"], [this] + own)
                if len(seqs[i]) > 256 or len(letters) > 2048:
                    refused += 1
                    continue
                res = realign.align(realign.codes_of(seqs[i]), realign.codes_of(letters))
                aligned += 1
                d = gtx.disc_realign_decide(res + (0,), len(seqs[i]), ref_pos, begin_padded, case.region_begin, s["score"], indel["pos"])
                if d["outcome"] == gtx.REALIGN_WORSE:
                    entries[i] = entries[i] + [(t, -1)]
                elif d["outcome"] == gtx.REALIGN_SAME_OVERLAPPING:
                    entries[i] = entries[i] + [(t, -2)]
                elif d["outcome"] == gtx.REALIGN_BETTER:
                    entries[i] = [(t, 0)] + [(te, 0 if (bits >> (e + 1)) & 1 else -1) for e, (te, _) in enumerate(entries[i])]
                    s.update(pos=sc.ref.i32(int(d["pos"])), pos_end=sc.ref.i32(int(d["pos_end"])), score=res[0], num_clipped_begin=sc.ref.i16(int(d["num_clipped_begin"])),
                             num_clipped_end=sc.ref.i16(int(d["num_clipped_end"])), num_ins_begin=sc.ref.i16(int(d["num_ins_begin"])))
                    for te, read_pos in entries[i]:
                        if read_pos >= 0 and s["mapq"] < 255:
                            ever[te].add(s["mapq"])
    finally:
        L.gtx_disc_destroy(h)
    return dict(states=states, entries=entries, support=holders(case, states, entries, ever), aligned=aligned, refused=refused, skipped=skipped)


def holders(case, states, entries, ever=None):
    """the counters counted off the lists: per entry the reads that hold it (max_mapq: from `ever`, or None)"""
    out = ref.clear_support(case.table)
    for s, per in zip(states, entries):
        for t, read_pos in per:
            if read_pos == -1:
                out[t]["anti_count"] += 1
            elif read_pos == -2:
                out[t]["multi_count"] += 1
            else:
                out[t]["hq_count"] += 1
                out[t]["sequence_reversed"] += 1 if s["flags"] & 16 else 0
                out[t]["proper_pairs"] += 1 if s["flags"] & 2 else 0
    for t, info in enumerate(out):
        info["max_mapq"] = max(ever[t], default=0) if ever is not None else None
    return out


# ---- arrays ---------------------------------------------------------------------------------------------------------------------------
SUPPORT_FIELDS = ("hq_count", "anti_count", "multi_count", "sequence_reversed", "proper_pairs", "max_mapq")


def support_array(support):
    out = np.zeros(len(support), gtx.DISC_SECOND_SUPPORT)
    for t, info in enumerate(support):
        out[t] = tuple(info[f] for f in SUPPORT_FIELDS)
    return out


def state_differs(case, want_states, want_entries, want_support, second, events, support):
    """None, or how the reads' state, their lists (read through first_event / n_events) and the counters differ from (states, entries,
    support) of the restatement"""
    lists = [[(int(e["indel"]), int(e["read_pos"])) for e in events[r["first_event"]:r["first_event"] + r["n_events"]]] for r in second]
    for i, (s, r) in enumerate(zip(want_states, second)):
        if s is None:
            if r["pos"] != -1 or r["n_events"] != 0:
                return "read %d was passed over and has changed" % i
            continue
        for name in ("pos", "pos_end", "score", "num_clipped_begin", "num_clipped_end", "num_ins_begin", "flags", "mapq", "l_qseq", "bucket"):
            if int(r[name]) != s[name]:
                return "read %d: %s is %d, the restatement says %d" % (i, name, r[name], s[name])
        if lists[i] != want_entries[i]:
            return "read %d: its list is %s, the restatement says %s" % (i, lists[i], want_entries[i])
    for t, info in enumerate(want_support):
        for name in SUPPORT_FIELDS:
            if int(support[t][name]) != info[name]:
                return "entry %d: %s is %d, the restatement says %d" % (t, name, support[t][name], info[name])
    return None


# ---- the sets -------------------------------------------------------------------------------------------------------------------------
def hap_seq(reference, start, length, indels):
    """`length` letters of the haplotype that carries `indels` [(region offset, type, letters)], from region offset `start` on"""
    out, p = [], start
    by_pos = {pos: (kind, seq) for pos, kind, seq in indels}
    while len(out) < length:
        if p in by_pos:
            kind, seq = by_pos[p]
            if kind == 'I':
                out.extend(seq)
            else:
                p += len(seq)
                by_pos.pop(p - len(seq))
                continue
            by_pos.pop(p)
        out.append(reference[p])
        p += 1
    return "".join(out[:length])


FLAGS = (3, 0, 16, 2, 18, 19)
MAPQS = (60, 254, 255, 10, 11)


def dress(reads):
    """every combination of the reversed and proper-pair flags, mapq at and around 255 and 10"""
    for i, r in enumerate(reads):
        r["flag"], r["mapq"] = FLAGS[i % len(FLAGS)], MAPQS[(i // 2) % len(MAPQS)]
    return reads


def _chain(rb, lst=None):
    """two indels 40 apart and reads of the haplotype that carries both: made BETTER in the first round, candidates of the second with an
    entry of their own that the second window applies; reads of the reference (WORSE); reads that end at the indel (SAME_OVERLAPPING
    with region_begin 0, SAME with a large one); reads with a clip of other letters in front of it (SAME)"""
    reference = rand_ref(1200, 31)
    d300, i340 = (300, 'D', reference[300:303]), (341, 'I', "GATC")
    d343 = (343, 'D', reference[343:345])  # within three positions of the insertion: in its window the purity test refuses the insertion
    d600 = (600, 'D', reference[600:605])
    both = [d300, i340]
    reads = []
    for start in (270, 280, 290):
        reads.append(rd(rb + start, cig(("M", 60)), hap_seq(reference, start, 60, both)))       # carries both
    for start in (265, 285):
        reads.append(rd(rb + start, cig(("M", 45)), hap_seq(reference, start, 45, [d300])))     # the deletion alone
        reads.append(rd(rb + start, cig(("M", 45)), reference[start:start + 45]))               # the reference over the deletion
    for start in (310, 325):
        reads.append(rd(rb + start, cig(("M", 45)), hap_seq(reference, start, 45, [i340])))     # the insertion alone
        reads.append(rd(rb + start, cig(("M", 45)), reference[start:start + 45]))               # the reference over the insertion
        reads.append(rd(rb + start, cig(("M", 45)), hap_seq(reference, start, 45, [d343])))     # the deletion beside the insertion
    reads.append(rd(rb + 260, cig(("M", 40)), reference[260:300]))                              # ends at the deletion
    reads.append(rd(rb + 303, cig(("M", 40)), reference[303:343]))                              # begins behind it
    reads.append(rd(rb + 250, cig(("M", 40), ("S", 6)), reference[250:290] + "".join("ACGT"[("ACGT".index(c) + 2) % 4] for c in reference[290:296])))  # a clip of other letters
    reads.append(rd(rb + 337, cig(("S", 4), ("M", 40)), "GATC" + reference[341:381]))           # begins with the inserted letters
    reads.append(rd(rb + 339, cig(("S", 2), ("M", 40)), "TC" + reference[341:381]))             # begins inside them (num_ins_begin > 0)
    for start in (570, 580, 590):
        reads.append(rd(rb + start, cig(("M", 50)), hap_seq(reference, start, 50, [d600])))
        reads.append(rd(rb + start, cig(("M", 30), ("S", 20)), hap_seq(reference, start, 50, [d600])))
    reads.append(rd(rb + 575, cig(("M", 50)), reference[575:625]))
    reads.sort(key=lambda r: r["pos"])
    table = [ent(rb + p, k, s, span=3) for p, k, s in (d300, i340, d343, d600)]
    return Case(reference, rb, dress(reads), table, lst=lst)


def _edges(rb):
    """indels at the region's ends: one at its first base (entry k does not apply: the round is skipped), one whose deletion runs to the
    region's last base (the end test fails), one near each end whose reads align at the window's first or last letter (NO_PADDING)"""
    reference = rand_ref(1000, 32)
    first = (0, 'D', reference[0:2])
    at_end = (996, 'D', reference[996:1000])
    near_begin, near_end = (30, 'D', reference[30:33]), (960, 'I', "TTAGG")
    reads = [rd(rb + 0, cig(("M", 50)), hap_seq(reference, 0, 50, [near_begin])),   # at the window's first letter
             rd(rb + 0, cig(("M", 50)), reference[0:50]),
             rd(rb + 5, cig(("M", 50)), hap_seq(reference, 5, 50, [near_begin])),
             rd(rb + 10, cig(("M", 50)), reference[10:60]),
             rd(rb + 940, cig(("M", 50)), hap_seq(reference, 940, 50, [near_end])),
             rd(rb + 950, cig(("M", 50)), reference[950:1000]),                        # at the window's last letter
             rd(rb + 945, cig(("M", 50)), hap_seq(reference, 945, 50, [near_end])),
             rd(rb + 955, cig(("M", 44)), reference[955:999])]
    reads.sort(key=lambda r: r["pos"])
    table = [ent(rb + p, k, s) for p, k, s in (first, at_end, near_begin, near_end)]
    return Case(reference, rb, dress(reads), table)


def _limits():
    """the aligner's limits: reads of 256 and 257 bases; max_read_size 925, so that a deletion of two leaves a window of 2 048 letters and
    a deletion of one a window of 2 049"""
    reference = rand_ref(3000, 33)
    d2, d1 = (1500, 'D', reference[1500:1502]), (1560, 'D', reference[1560:1561])
    reads = [rd(100, cig(("M", 925)), reference[100:1025]),                               # sets max_read_size; far from both indels
             rd(1400, cig(("M", 256)), hap_seq(reference, 1400, 256, [d2])),
             rd(1401, cig(("M", 257)), hap_seq(reference, 1401, 257, [d2])),
             rd(1480, cig(("M", 60)), hap_seq(reference, 1480, 60, [d2])),
             rd(1530, cig(("M", 60)), hap_seq(reference, 1530, 60, [d1])),
             rd(1531, cig(("M", 60)), reference[1531:1591])]
    return Case(reference, 0, dress(reads), [ent(p, k, s) for p, k, s in (d2, d1)])


SHAPE_PAIRS = (0, 1, 4, 5, 63, 64, 65)


def shape_case(n_pairs):
    """a round of n_pairs pairs (equal reads of the reference over a deletion); windows of 383, 385, 447 and 449 letters -- one letter
    more or less than a multiple of 64; n_pairs == 0: a list of one entry whose round has no reads"""
    reference = rand_ref(1000, 34)
    events = [(400, 'D', reference[400:417]), (500, 'D', reference[500:515]), (600, 'I', rand_ref(47, 35)), (700, 'I', rand_ref(49, 36))]
    reads = []
    for pos, _, _ in events:
        reads += [rd(pos - 15, cig(("M", 30)), reference[pos - 15:pos + 15]) for _ in range(n_pairs)]
    if n_pairs == 0:
        reads = [rd(20, cig(("M", 30)), reference[20:50])]
        events = events[:1]
    return Case(reference, 0, dress(reads), [ent(p, k, s) for p, k, s in events])


# ---- sets made for the windows' text: a read takes an entry of its own in one round and meets it again in a later round's window -------
def scene(reference, rb, rounds, reads, span=3):
    """a case whose list is `rounds` [(region offset, type, letters)] in that order (an entry may be named again).  A read of the
    reference over an indel is WORSE in that indel's round and holds it as anti-support from then on; a read of a haplotype is
    BETTER and holds it with read_pos 0: either way every later window of the read tries the entry"""
    events = sorted(set(rounds))
    case = Case(reference, rb, dress(reads), [ent(rb + p, k, s, span=span) for p, k, s in events])
    case.lst = tuple(case.index_of(rb + p, k, s) for p, k, s in rounds)
    return case


def plain(reference, rb, start, length=60):
    return rd(rb + start, cig(("M", length)), reference[start:start + length])


def carrying(reference, rb, start, indels, length=60):
    return rd(rb + start, cig(("M", length)), hap_seq(reference, start, length, indels))


def event(reference, at, kind, size, seed=0):
    """(at, 'D', the region's letters) or (at, 'I', letters of `seed`)"""
    return (at, kind, reference[at:at + size] if kind == 'D' else rand_ref(size, 50 + seed))


COPY_SIZES = (1, 63, 64, 65, 130)
COPY_AT = 300  # the large event's region offset: a window of a 100-base file begins 200 in front of it


def copy_case(kind, size, over, seed):
    """one large event E at COPY_AT and a deletion of two 12 in front of it, a region cut so that E's window has `over` letters more
    than a multiple of 64 once E is applied, a read of the reference over both: round 0 applies E as entry k, round 1 applies it as
    the read's own entry behind the small deletion (found after walking back)"""
    after = 64 * ((399 - size if kind == 'D' else 399 + size) // 64) + over  # the largest multiple a window of at most 400 letters reaches
    window = after + size if kind == 'D' else after - size
    reference = rand_ref(COPY_AT - 200 + window, 60 + seed)
    big, small = event(reference, COPY_AT, kind, size, seed), event(reference, COPY_AT - 12, 'D', 2)
    return scene(reference, 0, [big, small], [plain(reference, 0, COPY_AT - 30)])


def _copies():
    out, seed = [], 0
    for kind in "DI":
        for size in COPY_SIZES:
            for over in ((-1, 0, 1) if size in (63, 64, 65) else (0,)):
                out.append(copy_case(kind, size, over, seed))
                seed += 1
    # an insertion 64 letters in front of the region's end: the letters behind it are exactly one step of the moving loop
    reference = rand_ref(364, 89)
    out.append(scene(reference, 0, [(300, 'I', "GATTA"), event(reference, 288, 'D', 2)], [plain(reference, 0, 270)]))
    out += _copies_at_the_end()
    return out


def _copies_at_the_end():
    """the region's end cuts the windows: an own insertion at the window's last letter (the last position at which one applies), and
    an own deletion that leaves exactly one letter behind it; entry k is a deletion of two in front of either"""
    reference = rand_ref(500, 90)
    last = (499, 'I', "GAT")
    to_last = event(reference, 470, 'D', 29)   # 470 + 29 == 499: the region's last letter stays
    k_del, k_ins = event(reference, 452, 'D', 2), (452, 'I', "CA")
    at_end = [plain(reference, 0, 439), plain(reference, 0, 440)]
    return [scene(reference, 0, [last, event(reference, 452, 'D', 1)], at_end),  # behind a deletion of one the position is the window's length
            scene(reference, 0, [last, k_ins], at_end),   # behind an insertion the search walks forward to the last index
            scene(reference, 0, [last, k_del], at_end),   # behind a deletion the position is no index of the window any more
            scene(reference, 0, [to_last, k_del], [plain(reference, 0, 425), plain(reference, 0, 430)])]


def _search():
    """the search for an own entry's position behind what the window has applied already: own entries in front of entry k and behind
    it, two in front of a third, an insertion whose letters the search walks over, and positions that a deletion has taken away"""
    reference = rand_ref(800, 91)
    D, I = lambda at, n: event(reference, at, 'D', n), lambda at, s: (at, 'I', s)  # noqa: E731
    lists = [[D(310, 3), I(320, "GA"), D(340, 2), I(349, "TC"), D(330, 2)],        # own D and I in front of entry k and behind it
             [D(325, 2), I(345, "CAT"), I(312, rand_ref(20, 92))],                 # k inserts 20 letters: the walk forward crosses them
             [D(310, 3), D(318, 2), I(345, "GG"), D(332, 2)],                      # two in front: the index is off by their sum and k's
             [D(325, 2), I(333, "AC"), D(320, 20)],                                # k removes both positions
             [D(320, 12), I(326, "AC"), I(350, "T")],                              # an own deletion removes the position of the next own entry
             [I(308, "AT"), D(320, 2), D(335, 2)]]                                 # an own insertion in front of everything: found at once
    return [scene(reference, rb, lst, [plain(reference, rb, 300), plain(reference, rb, 297)]) for lst in lists for rb in ((0, 5000) if lst is lists[0] else (0,))]


OWN_END_AT = 400  # entry k of the own_ends set


def own_end_case(reference, k, t):
    """entry k, a deletion t that k's window refuses by its end test (or just does not), and four reads over k: of the reference (t and
    k as anti-support), of k's haplotype with a CIGAR of all M (a poor score at the intake: BETTER in t's round, so t is held with
    read_pos 0 when k's window refuses it, and BETTER again), of k's haplotype with its true CIGAR (WORSE in t's round: t is held as
    anti-support already when the read is made BETTER), and of the reference in front of t (equal: multi-support)"""
    start = k[0] - 8
    true_cigar = cig(("M", 8), ("D" if k[1] == 'D' else "I", len(k[2])), ("M", 52 if k[1] == 'D' else 52 - len(k[2])))
    reads = [plain(reference, 0, start), carrying(reference, 0, start, [k]), rd(start, true_cigar, hap_seq(reference, start, 60, [k])),
             plain(reference, 0, t[0] - 60)]
    reads.sort(key=lambda r: r["pos"])
    return scene(reference, 0, [t, k], reads)


def _own_ends():
    """a deletion of a read's own whose end test fails in entry k's window.  By its first arm: k's window ends 200 letters behind k
    inside the region, and the deletion begins 45 behind k and ends one letter in front of the window's last, on it, and one past it.
    By its second arm: the deletion's span holds entry k, an insertion or a deletion"""
    reference = rand_ref(1000, 93)
    K = OWN_END_AT
    k = event(reference, K, 'D', 2)
    out = [own_end_case(reference, k, event(reference, K + 45, 'D', 200 - 45 + over)) for over in (-1, 0, 1)]
    out.append(own_end_case(reference, (K, 'I', "GA"), event(reference, K - 5, 'D', 10)))
    out.append(own_end_case(reference, k, event(reference, K - 4, 'D', 10)))
    return out


def _purity():
    """the three positions on either side of an own entry: at the window's first and last indices (the region cuts the window), and
    one to four positions behind an insertion and behind a deletion that entry k applied"""
    reference = rand_ref(400, 94)
    R = len(reference)
    out = []
    for rb in (0, 3000):
        for at in (1, 2, 3):   # the window's index 1, 2, 3: max(0, pos - 3)
            own = event(reference, at, 'D', 2) if at != 2 else (at, 'I', "TG")
            out.append(scene(reference, rb, [own, event(reference, 30, 'D', 2)], [plain(reference, rb, 0), plain(reference, rb, 4)]))
    for back in (3, 2, 1):     # n - 3 .. n - 1: min(n, pos + 3)
        for kind in "ID" if back > 1 else "I":
            own = (R - back, 'I', "AG") if kind == 'I' else event(reference, R - back, 'D', 1)
            out.append(scene(reference, 0, [own, (R - 30, 'I', "C")], [plain(reference, 0, R - 63), plain(reference, 0, R - 62), plain(reference, 0, R - 61)]))
    for behind in (1, 2, 3, 4):
        out.append(scene(reference, 0, [event(reference, 230 + behind, 'D', 2), (230, 'I', "TTG")], [plain(reference, 0, 200)]))
        out.append(scene(reference, 0, [(231 + behind, 'I', "AC"), event(reference, 230, 'D', 2)], [plain(reference, 0, 200)]))
    for in_front in (3, 2):    # in front of a deletion that entry k applied: the jump lies at the index of k, pos + 3 is the first not looked at
        out.append(scene(reference, 0, [(240 - in_front, 'I', "AC"), event(reference, 240, 'D', 2)], [plain(reference, 0, 200)]))
    return out


def _fields():
    """what a read that is made BETTER takes along, and max_mapq.  Case 0: an insertion of 52 letters at the region's last base, and a
    read that is ten other letters and then the inserted letters from the second to the last but one: its alignment begins on the
    run of equal ref_pos values that ends with the window, so the num_ins loop is stopped by its bound; a read of 20 letters of the
    region and 40 others (num_clipped_end 40).  Case 1: the own_ends case of a deletion over entry k, whose read of k's haplotype has
    mapq 254, is t's only holder and lets go of it in k's round.  Case 2: the only holder has mapq 255"""
    reference = rand_ref(600, 95)
    R = len(reference)
    letters = rand_ref(52, 96)
    ins = (R - 1, 'I', letters)
    junk = "".join("ACGT"[("ACGT".index(c) + 1) % 4] for c in letters[1:10] + letters[0])  # (its last letter is not the insertion's first)
    others = "".join("ACGT"[("ACGT".index(c) + 2) % 4] for c in reference[R - 40:R])
    first = scene(reference, 0, [ins], [rd(R - 60, cig(("M", 60)), reference[R - 60:R - 40] + others),
                                        rd(R - 51, cig(("S", 10), ("M", 50)), junk + letters[1:51])])
    k, t = event(reference, 300, 'D', 2), event(reference, 296, 'D', 10)
    fill = [plain(reference, 0, 100), plain(reference, 0, 101)]
    lets_go = scene(reference, 0, [t, k], fill + [carrying(reference, 0, 292, [k])])             # read 2: mapq 254
    sole = scene(reference, 0, [k], fill * 2 + [carrying(reference, 0, 292, [k])])               # read 4: mapq 255
    # (case 3) an entry 300 positions in front of the region: end_padded is negative, the window has no letters, the round is skipped
    far = Case(reference, 5000, dress([plain(reference, 5000, 0)]), [ent(4700, 'D', "AC"), ent(5030, 'D', reference[30:32])])
    # (case 4) a deletion that runs to the region's last base and no read near it: the round's arena is the plain window alone, and what
    # lies behind the window lies behind the arena
    alone = Case(reference, 0, dress([plain(reference, 0, 100)]), [ent(R - 4, 'D', reference[R - 4:R])])
    # (case 5) :2086-2087 with region_begin 7 and an indel at offset 300: a read of the reference that begins 7 behind it overlaps it as the
    # text has it, one that begins 8 behind it does not
    left = scene(reference, 7, [k], [plain(reference, 7, 306), plain(reference, 7, 307), plain(reference, 7, 308)], span=10)
    return [first, lets_go, sole, far, alone, left]


@functools.lru_cache(maxsize=None)
def cases(name):
    return SETS[name]()


SETS = {
    "copies": _copies,
    "search": _search,
    "own_ends": _own_ends,
    "purity": _purity,
    "fields": _fields,
    "chain": lambda: [_chain(0), _chain(7), _chain(5000)],
    "again": lambda: [_chain(0, lst=(0, 1, 0, 2, 1, 3, 0))],  # a list that names an entry again: has_indel_event's first-entry rule
    "edges": lambda: [_edges(0), _edges(1000)],
    "limits": lambda: [_limits()],
}


def simulated_words_case(files, f, table):
    """file f of disc_second_cases.simulated_file()s over one region with the merged table"""
    reference, rb, reads, _ = files[f]
    return Case(reference, rb, reads, table, file_index=f)


# ---- the final decision on hand-made counters -----------------------------------------------------------------------------------------
def decide_rows():
    """[(entry, support dict, what the row is for)]: every threshold of :2187-2194 and of is_good_indel at its edge, one step to either side"""
    good = dict(hq_count=10, lq_count=0, anti_count=0, multi_count=0, sequence_reversed=5, proper_pairs=5, max_mapq=60)
    rows = []

    def row(what, kind="D", size=3, span=1, was_good=False, **over):
        s = dict(good)
        s.update(over)
        s["span"] = span
        rows.append((ent(1000 + 10 * len(rows), kind, "A" * size, span=span, good=was_good), s, what))

    # is_good_count: the three arms.  hq 7 passes is_good_indel's hq_count > 6; with hq below 7 the second test fails whatever the first says,
    # so the arms of 4 and 3 are shown through their count alone (good only when both hold)
    for span in (4, 5, 14, 15):
        for hq in (3, 4, 5, 7):
            row("span %d hq %d" % (span, hq), span=span, hq_count=hq, sequence_reversed=1)
    # count on 4.5, 5.0 and 5.5 exactly: insertions, correction (size / 2 + 8) / 8; deletions, (size / 3 + 10) / 10
    for hq, size in ((4, 2), (4, 4), (4, 6), (8, 0), (7, 4)):
        row("insertion hq %d size %d" % (hq, size), kind="I", size=size, span=15, hq_count=hq, sequence_reversed=1)
    for hq, size in ((3, 15), (4, 7), (4, 8), (5, 3), (5, 2), (7, 0)):
        row("deletion hq %d size %d" % (hq, size), size=size, span=15, hq_count=hq, sequence_reversed=1)
    for hq in (6, 7, 9, 10):
        for mapq in (10, 11):
            row("hq %d max_mapq %d" % (hq, mapq), hq_count=hq, max_mapq=mapq, sequence_reversed=1)
    for rev, anti in ((0, 0), (1, 0), (9, 0), (10, 0), (10, 1), (11, 1)):
        row("sequence_reversed %d depth %d" % (rev, 10 + anti), sequence_reversed=rev, anti_count=anti)
    for pp in (4, 5):
        row("proper_pairs %d" % pp, proper_pairs=pp)
    # 3 * log_qual: hq 8 -> gt00 56; anti 1: gt_alt min(9, 7) = 7 -> 49 -> 147; the edge of 50 needs log_qual 16 / 17:
    # hq 7, anti 5: gt00 49, gt_alt min(12, 35) = 12 -> 37; hq 7, anti 30: min(37, 210) = 37 -> 12 -> 36 < 50; anti 32: 39 -> 10 -> 30;
    # hq 7, anti 26: 33 -> 16 -> 48 < 50; anti 25: 32 -> 17 -> 51 >= 50 (then qual / depth decides: 51 / 32 < 3.5)
    for anti in (25, 26):
        row("3 * log_qual at anti %d" % anti, hq_count=7, anti_count=anti, sequence_reversed=1)
    # qual / depth on 3.5: hq 10, anti 2: gt00 70, gt_alt min(12, 14) = 12 -> 58 -> 174; depth 12 + multi: 174 / 3.5 = 49.71..; hq 7 anti 0
    # multi m: qual 3 * (49 - min(7, 0) = 49) = 147, depth 7 + m: 147 / 42 = 3.5 exactly at m = 35
    for multi in (34, 35, 36):
        row("qual / depth at multi %d" % multi, hq_count=7, multi_count=multi, sequence_reversed=1)
    # is_good_count alone (the program gives it beside the decision): each arm with its span, its hq_count and its count on the bound and
    # one step to the side that fails.  Insertions: correction (size / 2 + 8) / 8 -- size 2: 1.125, 4: 1.25, 6: 1.375, 12: 1.75; deletions:
    # (size / 3 + 10) / 10 -- size 15: 1.5, 39: 2.3, 14: 1.4666..
    for span in (4, 5):
        row("arm 2 span %d hq 4 count 5.0" % span, kind="I", size=4, span=span, hq_count=4)
        row("arm 2 span %d hq 3 count 5.25" % span, kind="I", size=12, span=span, hq_count=3)
        row("arm 2 span %d hq 4 count 4.5" % span, kind="I", size=2, span=span, hq_count=4)
    for span in (14, 15):
        row("arm 3 span %d hq 3 count 4.5" % span, size=15, span=span, hq_count=3)
        row("arm 3 span %d hq 2 count 4.6" % span, size=39, span=span, hq_count=2)
        row("arm 3 span %d hq 3 count 4.4" % span, size=14, span=span, hq_count=3)
    row("arm 1 span 4 hq 5 count 5.5", size=3, span=4, hq_count=5)
    row("arm 1 span 4 hq 5 count 5.33", size=2, span=4, hq_count=5)
    row("arm 1 span 4 hq 4 count 5.5", kind="I", size=6, span=4, hq_count=4)
    # the widths the decision reads through: the reference's counters are uint16_t, its max_mapq uint8_t.  Each row is good, or bad, only
    # because its counter is read through that width.  hq_count 65546 reads as 10: qual 210 over a depth of 10 + 51 is below 3.5 (at 32
    # bits: far above); with 50 it is 3.5
    row("hq_count 65536 + 10 multi 51", hq_count=65536 + 10, multi_count=51)
    row("hq_count 65536 + 10 multi 50", hq_count=65536 + 10, multi_count=50)
    row("hq_count 65536 + 4 count 4.5", kind="I", size=2, span=5, hq_count=65536 + 4)  # is_good_count reads it as 4
    row("anti_count 65536", anti_count=65536)                      # reads as 0 (at 32 bits: no quality left)
    row("multi_count 65536", multi_count=65536)                    # reads as 0 (at 32 bits: qual / depth far below 3.5)
    row("sequence_reversed 65536 + 5", sequence_reversed=65536 + 5)  # reads as 5 (at 32 bits: every read reversed, and more)
    row("proper_pairs 65536 + 4", proper_pairs=65536 + 4)          # reads as 4: not above 4
    for mapq in (10, 11):
        row("hq 7 max_mapq 256 + %d" % mapq, hq_count=7, max_mapq=256 + mapq, sequence_reversed=1)  # read as 10 and 11
    # get_log_qual's floor: gt00 70 is below gt_alt min(10 + 100, 700): the quality is 0, not the difference of two unsigned numbers
    row("log_qual floor at anti 100", anti_count=100)
    row("good already", was_good=True)
    return rows


# ---- a case through tests/emu_disc_rounds ---------------------------------------------------------------------------------------------
def write_case(path, case, k0, k1, event_cap, before=0, tamper=None, lists=None):
    """the input of tests/emu_disc_rounds: the file as the intake left it, or -- before = k -- as the restatement has it in front of round k;
    tamper(reads' array, table): changes either in place (an input no intake and no table maker would leave); lists: the entries in use"""
    import struct
    a, want = sc.arrays(case), expected(case)
    taken = want["taken"]
    states, entries, support = want["before"][before]
    entries = entries if lists is None else lists
    second, table = sc.second_array(case, states, entries), a["table"].copy()
    if tamper is not None:
        tamper(second, table)
    events = np.full(event_cap, 0xA5A5A5A5, np.uint32).repeat(2).view(gtx.DISC_SECOND_EVENT)
    flat = [e for per in entries for e in per]
    events[:len(flat)] = np.array(flat, gtx.DISC_SECOND_EVENT).reshape(-1)
    grouped = [i for b in taken["bucket_reads"] for i in b] + [i for i, s in enumerate(taken["reads"]) if s is None]
    off = np.concatenate([[0], np.cumsum([len(b) for b in taken["bucket_reads"]])])
    refb = case.reference.encode("latin-1")
    with open(path, "wb") as f:
        f.write(struct.pack("<11Iq", case.part.stride, len(a["reads"]), len(refb), case.bucket_size, len(a["table"]), len(a["letters"]), len(want["lst"]), k0, k1,
                            event_cap, len(flat), case.region_begin))
        f.write(refb)
        for x, dtype in ((a["planes"], None), (second, None), (table, None), (a["letters"], None), (want["lst"], np.uint32), (events, None),
                         (taken["max_pos_end"], np.int32), (taken["global_max_pos_end"], np.int32), ([taken["max_read_size"]], np.uint32), (grouped, np.uint32),
                         (off, np.uint32), (support_array(support), None)):
            f.write(np.ascontiguousarray(x if dtype is None else np.array(x, dtype)).tobytes())


def read_result(path, case, event_cap):
    """-> dict(status, used, stats, second, events, support, windows [(k, read or None, letters, ref_pos, applied flags)], syncs [per
    window: the mem_sync calls of its build])"""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, np.uint32, 9)
    at = 36
    out = dict(status=int(head[0]), used=int(head[1]), stats=dict(zip(("rounds_done", "rounds_skipped", "pairs_aligned", "pairs_refused", "windows_built",
                                                                       "compactions", "events_wanted"), (int(v) for v in head[2:]))))
    for key, dtype, count in (("second", gtx.DISC_SECOND_READ, len(case.reads)), ("events", gtx.DISC_SECOND_EVENT, event_cap),
                              ("support", gtx.DISC_SECOND_SUPPORT, len(case.table))):
        out[key] = np.frombuffer(raw, dtype, count, at)
        at += count * np.dtype(dtype).itemsize
    out["windows"], out["syncs"] = [], []
    while at < len(raw):
        k, read, n, n_entries, syncs = (int(v) for v in np.frombuffer(raw, np.uint32, 5, at))
        at += 20
        out["syncs"].append(syncs)
        letters, ref_pos, flags = raw[at:at + n], np.frombuffer(raw, np.int32, n, at + n), list(raw[at + 5 * n:at + 5 * n + n_entries])
        at += 5 * n + n_entries
        out["windows"].append((k, None if read == 0xFFFFFFFF else read, letters, ref_pos, flags))
    assert at == len(raw)
    return out


def through(run, case, k0=0, k1=None, event_cap=None, before=0, tamper=None, lists=None):
    """a case through tests/emu_disc_rounds; run(write, read): emu_programs.run with a program and a directory.  Defaults: the whole
    list, room for every list ever made (a round whose pairs might all grow can compact all the same: gtx.h)"""
    k1 = len(expected(case)["lst"]) if k1 is None else k1
    event_cap = sum(new for _, new in room(case)) if event_cap is None else event_cap
    return run(lambda path: write_case(path, case, k0, k1, event_cap, before, tamper, lists), lambda path: read_result(path, case, event_cap))


# ---- the judge: what a program has to give for a set, a launch shape or the final decision -------------------------------------------
def case_of(name, k=0):
    return shape_case(int(name[5:])) if name.startswith("shape") else cases(name)[k]


def round_counts(case, k):
    """-> (skipped, aligned, refused, windows built) of round k, off the restatement's trace"""
    want = expected(case)
    r = want["trace"]["rounds"][k]
    assert r["k"] == k
    if r["skipped"]:
        return 1, 0, 0, 1
    own = sum(1 for i, _, _, _ in r["visits"] if want["before"][k][1][i])
    refused = sum(1 for _, o, _, _ in r["visits"] if o == "refused")
    return 0, len(r["visits"]) - refused, refused, 1 + own


@functools.lru_cache(maxsize=None)
def windows_wanted(case):
    """per round [(read or None: the plain window, letters, ref_pos values, applied flags of the read's entries, mem_sync calls)] in
    the order of the slots: what gtx_disc_realign_target (the library's host function) makes of the same events.  The calls: one
    behind the window's letters, two per step of 64 of every shifted copy, one behind an insertion's letters (the header's text)"""
    want = expected(case)
    L, h = gtx.lib(), C.c_void_p()
    refb = case.reference.encode("latin-1")
    gtx.check(L.gtx_disc_create(refb, len(refb), case.region_begin, -1, C.byref(h)))
    mrs = want["taken"]["max_read_size"]
    as_event = lambda e: (e["pos"], e["type"], e["seq"])  # noqa: E731
    out = []
    try:
        for r in want["trace"]["rounds"]:
            indel = case.table[want["lst"][r["k"]]]
            if max(0, indel["pos"] - mrs - 100 - case.region_begin) >= len(case.reference) or indel["pos"] + mrs + 100 < case.region_begin:
                states, entries, _ = want["before"][r["k"]]
                pairs = sc.ref.round_reads(case.table, want["lst"][r["k"]], want["taken"], states, entries, case.region_begin, case.bucket_size)
                out.append([(None, b"", [], [], 1)] + [(i, b"", [], [0] * len(entries[i]), 1) for i in pairs if entries[i]])
                continue
            letters, ref_pos, begin, _ = gtx.disc_realign_target(h, mrs, [as_event(indel)])
            n0 = min(len(case.reference), indel["pos"] + mrs + 100 - case.region_begin) - begin
            size = len(indel["seq"])
            steps = 0 if r["skipped"] else -(-(n0 - size - (indel["pos"] - case.region_begin - begin)) // 64) if indel["type"] == 'D' else \
                -(-(n0 - (indel["pos"] - case.region_begin - begin)) // 64)
            k_syncs = 1 + (0 if r["skipped"] else 2 * steps + (indel["type"] == 'I'))
            n1 = n0 if r["skipped"] else n0 - size if indel["type"] == 'D' else n0 + size
            per = [(None, letters, list(ref_pos), [], k_syncs)]
            if r["skipped"]:  # entry k did not apply: the windows of the round's pairs are the plain one, no entry of theirs is tried
                states, entries, _ = want["before"][r["k"]]
                for i in sc.ref.round_reads(case.table, want["lst"][r["k"]], want["taken"], states, entries, case.region_begin, case.bucket_size):
                    if entries[i]:
                        per.append((i, letters, list(ref_pos), [0] * len(entries[i]), 1))
            for (i, _, _, _), seen in ([] if r["skipped"] else zip(r["visits"], r["own"])):
                own = [case.table[t] for t, _ in want["before"][r["k"]][1][i]]
                if own:
                    letters, ref_pos, _, bits = gtx.disc_realign_target(h, mrs, [as_event(e) for e in [indel] + own])
                    n, syncs = n1, k_syncs
                    for e, x in zip(own, seen):
                        if x["applied"]:
                            size = len(e["seq"])
                            syncs += 2 * -(-(n - size - x["index"]) // 64) if e["type"] == 'D' else 2 * -(-(n - x["index"]) // 64) + 1
                            n += -size if e["type"] == 'D' else size
                    assert n == len(letters)
                    per.append((i, letters, list(ref_pos), [(bits >> (e + 1)) & 1 for e in range(len(own))], syncs))
            out.append(per)
    finally:
        L.gtx_disc_destroy(h)
    return out


def counters_differ_from_the_holders(case, second, events, support):
    """None, or the entry whose counters are not the reads that hold it in the program's own lists (the holders' equation)"""
    held = {}
    for r in second:
        for e in events[int(r["first_event"]):int(r["first_event"]) + int(r["n_events"])]:
            key = "anti_count" if e["read_pos"] == -1 else "multi_count" if e["read_pos"] == -2 else "hq_count"
            names = [key] + ([f for f, bit in (("sequence_reversed", 16), ("proper_pairs", 2)) if int(r["flags"]) & bit] if key == "hq_count" else [])
            for f in names:
                held[(int(e["indel"]), f)] = held.get((int(e["indel"]), f), 0) + 1
    for t in range(len(case.table)):
        for f in SUPPORT_FIELDS[:-1]:
            if int(support[t][f]) != held.get((t, f), 0):
                return "entry %d: %s is %d, its holders are %d" % (t, f, support[t][f], held.get((t, f), 0))
    return None


def slice_differs(run, case, k0=0, k1=None, event_cap=None, compacts=False):
    """the rounds [k0, k1) from the restatement's state in front of round k0, in an event array of event_cap entries -> None, or how
    the program differs: the status (5 with events_wanted in front of the first round that does not fit), the reads' state, their
    lists, the counters (and the holders' equation), the statistics, and every window, ref_pos value and applied flag"""
    want = expected(case)
    k1 = len(want["lst"]) if k1 is None else k1
    cap = sum(new for _, new in room(case)) if event_cap is None else event_cap
    got = through(run, case, k0, k1, cap, before=k0)
    stop = next((k for k in range(k0, k1) if sum(room(case)[k]) > cap), None)
    end = k1 if stop is None else stop
    if got["status"] != (0 if stop is None else 5):
        return "status %d" % got["status"]
    states, entries, support = want["before"][end]
    how = state_differs(case, states, entries, support, got["second"], got["events"], got["support"]) or \
        counters_differ_from_the_holders(case, got["second"], got["events"], got["support"])
    if how is not None:
        return how
    if want["trace"]["floors"] != 0:
        return "a floor acts in the restatement"
    counts = [round_counts(case, k) for k in range(k0, end)]
    stats = dict(rounds_done=end - k0, rounds_skipped=sum(c[0] for c in counts), pairs_aligned=sum(c[1] for c in counts), pairs_refused=sum(c[2] for c in counts),
                 windows_built=sum(c[3] for c in counts), compactions=got["stats"]["compactions"], events_wanted=0 if stop is None else sum(room(case)[stop]))
    if got["stats"] != stats:
        return "the statistics are %s, not %s" % (got["stats"], stats)
    if compacts and got["stats"]["compactions"] < 1:
        return "no compaction"
    if any(int(r["n_events"]) == 0 and int(r["first_event"]) != 0 for r in got["second"]):
        return "a read without entries whose first_event is not 0"
    if got["used"] > cap or any(int(r["first_event"]) + int(r["n_events"]) > got["used"] for r in got["second"]):
        return "a list lies behind the entries in use"
    wanted = [(k,) + w for k in range(k0, min(k1, end + 1)) for w in windows_wanted(case)[k]]
    if len(got["windows"]) != len(wanted):
        return "%d windows, not %d" % (len(got["windows"]), len(wanted))
    for (k, read, letters, ref_pos, flags), syncs, (k_, read_, letters_, ref_pos_, flags_, syncs_) in zip(got["windows"], got["syncs"], wanted):
        if (k, read) != (k_, read_):
            return "the window of round %s, read %s where that of round %s, read %s should be" % (k, read, k_, read_)
        if letters != letters_ or list(ref_pos) != ref_pos_ or flags != flags_:
            what = "letters" if letters != letters_ else "ref_pos values" if list(ref_pos) != ref_pos_ else "applied flags %s, not %s" % (flags, flags_)
            return "round %d, read %s: the window's %s differ from gtx_disc_realign_target's" % (k, read, what)
        if syncs != syncs_:
            return "round %d, read %s: %d mem_sync calls, the text has %d" % (k, read, syncs, syncs_)
    return None


def case_differs(run, case):
    """the whole list, and -- the state after every round -- every [0, k)"""
    n = len(expected(case)["lst"])
    for k in [n] + list(range(1, n)):
        how = slice_differs(run, case, 0, k)
        if how is not None:
            return "rounds [0, %d): %s" % (k, how)
    return None


SLICED = ("again", 0)     # the case of the slice and event-array shapes
COPIED = ("copies", 21)   # the insertion of 130 letters: its lists in an array that is exactly large enough, and one entry short


def launches():
    """name -> what the shape is (made once: the names need the restatement's list)"""
    out = {"slice_%d" % k: ("slice", k) for k in range(len(expected(case_of(*SLICED))["lst"]) + 1)}
    out.update(array_exact=("array", SLICED, 0), array_one_short=("array", SLICED, -1), copies_array_exact=("array", COPIED, 0),
               copies_array_one_short=("array", COPIED, -1), letters_missing=("letters_missing",), lists_shared=("lists_shared",),
               entry_behind_the_table=("entry_behind_the_table",))
    return out


LAUNCHES = tuple(sorted(launches()))
SHAPES = tuple("shape%d" % n for n in SHAPE_PAIRS)
NAMES = tuple(sorted(SETS)) + SHAPES + LAUNCHES + ("decide",)  # what judge() knows: the sets, the launch shapes, the final decision


def launch_differs(name, run):
    what = launches()[name]
    if what[0] == "slice":   # [0, k) then -- from the restatement's state in front of round k -- [k, n)
        case, k = case_of(*SLICED), what[1]
        return slice_differs(run, case, 0, k) or slice_differs(run, case, k, None)
    if what[0] == "array":
        case = case_of(*what[1])
        need = max(live + new for live, new in room(case))
        return slice_differs(run, case, event_cap=need + what[2], compacts=what[2] == 0 and need < sum(new for _, new in room(case)))
    case = case_of("fields", 0)  # one entry, an insertion; two reads
    if name == "letters_missing":
        # the entry's letters lie behind the table's letters (no table maker leaves that): it is not applied, its round is skipped
        def no_letters(second, table):
            table["seq_off"] = len(sc.arrays(case)["letters"]) - 1
        got = through(run, case, tamper=no_letters)
        if got["status"] != 0 or got["stats"]["rounds_skipped"] != 1 or got["stats"]["pairs_aligned"] != 0 or (got["support"].view(np.uint32) != 0).any():
            return "an entry whose letters are not there was applied: %s" % (got["stats"],)
        return None
    if name == "entry_behind_the_table":
        # a read's list names an entry the table does not have: nothing is made of it -- no letters, no window, no counter --, and it stays in
        # the read's list as what could not be applied
        got = through(run, case, event_cap=8, lists=[[(len(case.table), -1)], []])
        lists = [[(int(e["indel"]), int(e["read_pos"])) for e in got["events"][r["first_event"]:r["first_event"] + r["n_events"]]] for r in got["second"]]
        if got["status"] != 0 or lists != [[(0, 0), (len(case.table), -1)], [(0, 0)]] or int(got["support"][0]["hq_count"]) != 2:
            return "status %d, lists %s" % (got["status"], lists)
        return None
    # two reads that name the same entries, more between them than the array holds: the compaction leaves the array alone and the run
    # ends with the program's status 2 (the library: GTX_ERR_ARG), not with a store behind the copy
    def shared(second, table):
        second["first_event"], second["n_events"] = 0, 2

    def write(path):
        write_case(path, case, 0, 1, 3, 0, shared, lists=[[(0, -1), (0, -1)], []])
    import emu_programs
    try:
        run(write, lambda path: read_result(path, case, 3))
    except emu_programs.Died as e:
        return None if e.how == "the program dies (exit status 2)" else e.how
    return "lists that share their entries were taken"


def decide_differs(run):
    """decide_rows() through the program: is_good_count and the whole decision of every row against the restatement's"""
    import struct
    rows = decide_rows()
    table, _ = sc.table_arrays([e for e, _, _ in rows])

    def write(path):
        with open(path, "wb") as f:
            f.write(struct.pack("<11Iq", 0xFFFFFFFF, 0, 0, 0, len(rows), 0, 0, 0, 0, 0, 0, 0))
            f.write(table.tobytes())
            f.write(support_array([s for _, s, _ in rows]).tobytes())
    got = run(write, lambda path: np.frombuffer(open(path, "rb").read(), np.uint8).reshape(len(rows), 2))
    for (e, s, what), (count, good) in zip(rows, got):
        held = ref.as_the_reference_holds(s)
        if bool(count) != ref.is_good_count(e, held):
            return "row '%s': is_good_count is %d" % (what, count)
        if bool(good) != ref.good_after([dict(e, good=False)], [0], [s])[0]:
            return "row '%s': the decision is %d" % (what, good)
    return None


def judge(name, run):
    """None when the program behind `run` (emu_programs.run with a build of tests/emu_disc_rounds) gives the set, the launch shape
    or the final decision `name` as the restatement says, else a short text: how it differs"""
    try:
        if name == "decide":
            return decide_differs(run)
        if name in LAUNCHES:
            return launch_differs(name, run)
        if name in SHAPES:
            return case_differs(run, case_of(name))
        for k, case in enumerate(cases(name)):
            how = case_differs(run, case)
            if how is not None:
                return "case %d: %s" % (k, how)
        return None
    except (ValueError, IndexError, AssertionError, OverflowError) as e:  # what the program wrote cannot be read as a result
        return "no result that can be read (%s)" % type(e).__name__
