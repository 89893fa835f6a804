"""A plain restatement of discovery's second pass from the aligner on, written line by line from the reference's text: the rounds of
realign_to_indels (src/typer/caller.cpp:1876-2171), Alignment::has_indel_event / add_indel_event / replace_indel_events
(src/typer/read.cpp:13-116) and the good-support decision at the end (:2179-2229 with EventSupport::is_good_indel and get_log_qual,
src/typer/event.cpp:95-106, :273-291).  Sequential, dicts and lists only; the alignment is tests/realign_ref.py's (paw is absent
from the reference's tree: the model its text states is the definition), the reads a round visits are tests/disc_second_ref.py's.
This file is the definition the library's rounds are held to (include/gtx.h: gtx_disc_second_rounds, gtx_disc_second_decide).

Where the reference is undefined or asserts, the library's stated rules: a window that begins behind the region's end has no
letters, so entry k does not apply and the round is skipped like one of :1905; a pair the aligner refuses (a read of more than 256
bases, a window of more than 2 048 letters) is not aligned in that round, its read stays as it was.

    support of a table entry: dict(hq_count, lq_count, anti_count, multi_count, sequence_reversed, proper_pairs, max_mapq, span)
    a read's entries: [(table index, read_pos)]"""
import disc_second_ref as second
import realign_ref as realign
from disc_second_ref import PAD, READ_ANTI_SUPPORT, READ_MULTI_SUPPORT, i16, i32

IS_SEQ_REVERSED, IS_PROPER_PAIR = 16, 2  # constants.hpp.in
MAX_READ, MAX_TARGET = 256, 2048          # the aligner's limits (include/gtx.h)


def clear_support(table):
    """EventSupport::clear() per entry, and its span"""
    return [dict(hq_count=0, lq_count=0, anti_count=0, multi_count=0, sequence_reversed=0, proper_pairs=0, max_mapq=0, span=e["span"]) for e in table]


def add_indel_event(entries, support, pos, flags, mapq, t, trace):
    """read.cpp:29-55"""
    info = support[t]
    if pos == READ_ANTI_SUPPORT:
        info["anti_count"] += 1
    elif pos == READ_MULTI_SUPPORT:
        info["multi_count"] += 1
    else:
        info["hq_count"] += 1
        if flags & IS_SEQ_REVERSED:
            info["sequence_reversed"] += 1
        if flags & IS_PROPER_PAIR:
            info["proper_pairs"] += 1
        if mapq < 255 and mapq > info["max_mapq"]:
            info["max_mapq"] = mapq
    entries.append((t, pos))


def replace_indel_events(entries, support, flags, mapq, new_entries, trace):
    """read.cpp:57-116; entries is changed in place"""
    for t, read_pos in entries:                 # lower count on old events
        info = support[t]
        if read_pos == READ_ANTI_SUPPORT:
            info["anti_count"] -= 1
        elif read_pos == READ_MULTI_SUPPORT:
            info["multi_count"] -= 1
        else:
            info["hq_count"] -= 1
            if flags & IS_SEQ_REVERSED:
                if info["sequence_reversed"] > 0:   # :76
                    info["sequence_reversed"] -= 1
                else:
                    trace["floors"] += 1
            if flags & IS_PROPER_PAIR:
                if info["proper_pairs"] > 0:        # :83
                    info["proper_pairs"] -= 1
                else:
                    trace["floors"] += 1
        trace["lowered"] += 1
    for t, read_pos in new_entries:             # increase count on new events
        info = support[t]
        if read_pos == READ_ANTI_SUPPORT:
            info["anti_count"] += 1
        elif read_pos == READ_MULTI_SUPPORT:
            info["multi_count"] += 1
        else:
            info["hq_count"] += 1
            if flags & IS_SEQ_REVERSED:
                info["sequence_reversed"] += 1
            if flags & IS_PROPER_PAIR:
                info["proper_pairs"] += 1
            if mapq < 255 and mapq > info["max_mapq"]:
                info["max_mapq"] = mapq
    entries[:] = new_entries


def how_applied(ref_pos, pos_, type_, event_size, offset):
    """what apply_indel_event (event.cpp:293-396, tests/realign_ref.py) will meet on these ref_pos values -- looked at, nothing is
    changed: dict(search: 'outside' (the position is not an index of the window) | 'at once' | 'walked forward' | 'walked back' |
    'not found', index (where the search ended), pure (None when the search failed), past / differs: the two arms of a deletion's end
    test, pos + size >= n and ref_pos[pos + size] != position + size (None where the arm is not evaluated))"""
    want = pos_ - offset
    n = len(ref_pos)
    out = dict(search="outside", index=None, pure=None, past=None, differs=None)
    if want <= 0 or want >= n:
        return out
    pos = want
    out["search"] = "at once"
    if ref_pos[pos] != want:
        while pos + 1 < n and ref_pos[pos] < want:
            pos += 1
        forward = pos - want
        while pos > 0 and ref_pos[pos] > want:
            pos -= 1
        out["search"] = "not found" if ref_pos[pos] != want else "walked forward" if forward else "walked back"
    out["index"] = pos
    if out["search"] == "not found":
        return out
    window = ref_pos[max(0, pos - 3):min(n, pos + 3)]
    out["pure"] = all(b == a + 1 for a, b in zip(window, window[1:]))
    if out["pure"] and type_ == 'D':
        out["past"] = pos + event_size >= n
        if not out["past"]:
            out["differs"] = ref_pos[pos + event_size] != want + event_size
    return out


def rounds(reference, region_begin, bucket_size, table, lst, k0, k1, taken, states, entries, support, sequences, after_round=None):
    """:1876-2171 for the list entries k0 .. k1 - 1.  taken: the intake's result (its bucket arrays stay as they are); states, entries,
    support: changed in place; sequences: per read its letters.  after_round(k): called behind every round.
    -> trace: dict(rounds [per round: dict(k, skipped, visits [(read, outcome or 'refused', applied bits, window length)], own [per
    visit, per entry of the read: how_applied() in front of its apply_indel_event, with t, read_pos and applied])], aligned, refused,
    skipped, windows, floors, lowered)"""
    ref_size = len(reference)
    trace = dict(rounds=[], aligned=0, refused=0, skipped=0, windows=0, floors=0, lowered=0)
    for k in range(k0, k1):
        t = lst[k]
        indel = table[t]
        this = dict(k=k, skipped=False, visits=[], own=[])
        trace["rounds"].append(this)
        begin_padded = max(0, indel["pos"] - taken["max_read_size"] - 2 * PAD - region_begin)  # :1890
        end_padded = indel["pos"] + taken["max_read_size"] + 2 * PAD - region_begin            # :1892
        if begin_padded >= ref_size or end_padded < begin_padded:  # (:1891 asserts otherwise; the library's rule)
            new_ref = []
        else:
            new_ref = list(reference[begin_padded:] if end_padded >= ref_size else reference[begin_padded:end_padded])  # :1894-1896
        ref_pos = list(range(len(new_ref)))     # :1897-1898
        trace["windows"] += 1
        if not realign.apply_indel_event(new_ref, ref_pos, indel["pos"], indel["type"], indel["seq"], begin_padded + region_begin):  # :1902
            this["skipped"] = True              # :1905
            trace["skipped"] += 1
            if after_round:
                after_round(k)
            continue
        new_ref_stable, ref_pos_stable = list(new_ref), list(ref_pos)  # :1915-1916
        for i in second.round_reads(table, t, taken, states, entries, region_begin, bucket_size):  # :1911-1958
            read = states[i]
            applied_events = [(t, 0)]           # :1965-1966
            bits = 1
            if entries[i]:
                trace["windows"] += 1
            seen = []
            this["own"].append(seen)
            for e, (te, held_as) in enumerate(entries[i]):  # :1968 (every table entry has realignment support, :2924)
                ev = table[te]
                seen.append(dict(how_applied(ref_pos, ev["pos"], ev["type"], len(ev["seq"]), begin_padded + region_begin), t=te, read_pos=held_as))
                if realign.apply_indel_event(new_ref, ref_pos, ev["pos"], ev["type"], ev["seq"], begin_padded + region_begin):  # :1975
                    applied_events.append((te, 0))                    # :1986
                    bits |= 2 << e
                else:
                    applied_events.append((te, READ_ANTI_SUPPORT))    # :1999
                seen[-1]["applied"] = bool(bits & (2 << e))
            old_score = read["score"]           # :2004
            window = "".join(new_ref)
            if len(sequences[i]) > MAX_READ or len(window) > MAX_TARGET:  # the stated limit
                trace["refused"] += 1
                this["visits"].append((i, "refused", bits, len(window)))
                new_ref, ref_pos = list(new_ref_stable), list(ref_pos_stable)
                continue
            score, clip_begin, clip_end, database_begin, database_end = realign.align(realign.codes_of(sequences[i]), realign.codes_of(window))  # :2007
            trace["aligned"] += 1
            outcome = None
            if database_begin == 0 or database_end == len(new_ref):  # :2025
                outcome = realign.NO_PADDING
            elif score <= old_score:            # :2066
                if score < old_score:           # :2069
                    add_indel_event(entries[i], support, READ_ANTI_SUPPORT, read["flags"], read["mapq"], t, trace)  # :2084
                    outcome = realign.WORSE
                elif indel["pos"] >= ref_pos[database_begin] + begin_padded and indel["pos"] <= ref_pos[database_end] + begin_padded:  # :2086-2087
                    add_indel_event(entries[i], support, READ_MULTI_SUPPORT, read["flags"], read["mapq"], t, trace)  # :2097
                    outcome = realign.SAME_OVERLAPPING
                else:
                    outcome = realign.SAME
            else:
                replace_indel_events(entries[i], support, read["flags"], read["mapq"], applied_events, trace)  # :2110
                read["pos"] = i32(ref_pos[database_begin] + region_begin + begin_padded)     # :2136
                read["pos_end"] = i32(ref_pos[database_end] + region_begin + begin_padded)   # :2137
                read["score"] = i32(score)                                                    # :2138
                read["num_clipped_begin"] = i16(clip_begin)                                   # :2139
                read["num_clipped_end"] = i16(len(sequences[i]) - clip_end)                   # :2140
                num_ins = 0                                                                   # :2144
                while database_begin + num_ins + 1 < len(ref_pos) and ref_pos[database_begin + num_ins] == ref_pos[database_begin + num_ins + 1]:
                    num_ins += 1
                read["num_ins_begin"] = i16(num_ins)                                          # :2152
                outcome = realign.BETTER
            this["visits"].append((i, outcome, bits, len(window)))
            new_ref, ref_pos = list(new_ref_stable), list(ref_pos_stable)  # :2034, :2100, :2164
        if after_round:
            after_round(k)
    return trace


def get_log_qual(count, anti_count, eps):
    """event.cpp:95-106 (uint32_t)"""
    gt00 = (count * eps) & 0xFFFFFFFF
    gt01 = (count + anti_count) & 0xFFFFFFFF
    gt11 = (anti_count * eps) & 0xFFFFFFFF
    gt_alt = min(gt01, gt11)
    return gt00 - gt_alt if gt00 > gt_alt else 0


def is_good_indel(info, eps=7):
    """event.cpp:273-291"""
    depth = info["hq_count"] + info["lq_count"] + info["anti_count"] + info["multi_count"]
    if info["hq_count"] <= 6 or info["sequence_reversed"] <= 0 or info["sequence_reversed"] >= depth or info["proper_pairs"] <= 4 or \
            (info["hq_count"] < 10 and info["max_mapq"] <= 10):
        return False
    qual = 3 * get_log_qual(info["hq_count"] + info["lq_count"], info["anti_count"], eps)
    if qual < 50:
        return False
    qd = float(qual) / float(depth)
    return qd >= 3.5


def as_the_reference_holds(info):
    """the counters through the widths of the reference's EventSupport (event.hpp: uint16_t, max_mapq uint8_t): the library counts in
    32 bits and reads through these (include/gtx.h: gtx_disc_second_decide)"""
    return dict(info, **{f: info[f] & (0xFF if f == "max_mapq" else 0xFFFF) for f in ("hq_count", "lq_count", "anti_count", "multi_count", "sequence_reversed",
                                                                                       "proper_pairs", "max_mapq")})


def is_good_count(indel, info):
    """:2187-2194 of one entry, its counters as the reference holds them"""
    size = len(indel["seq"])
    correction = float(size / 2.0 + 8.0) / 8.0 if indel["type"] == 'I' else float(size / 3.0 + 10.0) / 10.0  # :2187-2188
    count = correction * (info["hq_count"] + info["lq_count"])                                               # :2190
    return (info["hq_count"] >= 5 and count >= 5.5) or (info["span"] >= 5 and info["hq_count"] >= 4 and count >= 5.0) or \
        (info["span"] >= 15 and info["hq_count"] >= 3 and count >= 4.5)                                      # :2192-2194


def good_after(table, lst, support):
    """:2179-2229 -> per table entry: it had no good support and has it now (an entry that is good already is left alone)"""
    out = [False] * len(table)
    for t in lst:
        indel, info = table[t], as_the_reference_holds(support[t])
        if indel["good"]:                       # :2184
            continue
        if is_good_count(indel, info) and is_good_indel(info):  # :2219
            out[t] = True
    return out
