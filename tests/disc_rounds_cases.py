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
            if begin >= len(case.reference) or gtx.disc_realign_target(h, taken["max_read_size"], [this])[3] == 0:
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


@functools.lru_cache(maxsize=None)
def cases(name):
    return SETS[name]()


SETS = {
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
    row("good already", was_good=True)
    return rows


# ---- a case through tests/emu_disc_rounds ---------------------------------------------------------------------------------------------
def write_case(path, case, k0, k1, event_cap, before=0):
    """the input of tests/emu_disc_rounds: the file as the intake left it, or -- before = k -- as the restatement has it in front of round k"""
    import struct
    a, want = sc.arrays(case), expected(case)
    taken = want["taken"]
    states, entries, support = want["before"][before]
    second = sc.second_array(case, states, entries)
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
        for x, dtype in ((a["planes"], None), (second, None), (a["table"], None), (a["letters"], None), (want["lst"], np.uint32), (events, None),
                         (taken["max_pos_end"], np.int32), (taken["global_max_pos_end"], np.int32), ([taken["max_read_size"]], np.uint32), (grouped, np.uint32),
                         (off, np.uint32), (support_array(support), None)):
            f.write(np.ascontiguousarray(x if dtype is None else np.array(x, dtype)).tobytes())


def read_result(path, case, event_cap):
    """-> dict(status, used, stats, second, events, support, windows [(k, read or None, letters, ref_pos, applied flags)])"""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, np.uint32, 9)
    at = 36
    out = dict(status=int(head[0]), used=int(head[1]), stats=dict(zip(("rounds_done", "rounds_skipped", "pairs_aligned", "pairs_refused", "windows_built",
                                                                       "compactions", "events_wanted"), (int(v) for v in head[2:]))))
    for key, dtype, count in (("second", gtx.DISC_SECOND_READ, len(case.reads)), ("events", gtx.DISC_SECOND_EVENT, event_cap),
                              ("support", gtx.DISC_SECOND_SUPPORT, len(case.table))):
        out[key] = np.frombuffer(raw, dtype, count, at)
        at += count * np.dtype(dtype).itemsize
    out["windows"] = []
    while at < len(raw):
        k, read, n, n_entries = (int(v) for v in np.frombuffer(raw, np.uint32, 4, at))
        at += 16
        letters, ref_pos, flags = raw[at:at + n], np.frombuffer(raw, np.int32, n, at + n), list(raw[at + 5 * n:at + 5 * n + n_entries])
        at += 5 * n + n_entries
        out["windows"].append((k, None if read == 0xFFFFFFFF else read, letters, ref_pos, flags))
    assert at == len(raw)
    return out


def through(run, case, k0=0, k1=None, event_cap=None, before=0):
    """a case through tests/emu_disc_rounds; run(write, read): emu_programs.run with a program and a directory.  Defaults: the whole
    list, room for every list ever made (a round whose pairs might all grow can compact all the same: gtx.h)"""
    k1 = len(expected(case)["lst"]) if k1 is None else k1
    event_cap = sum(new for _, new in room(case)) if event_cap is None else event_cap
    return run(lambda path: write_case(path, case, k0, k1, event_cap, before), lambda path: read_result(path, case, event_cap))
