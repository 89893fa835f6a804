"""A plain restatement of discovery's second pass up to the aligner, written line by line from the reference's text
(parallel_second_pass, src/typer/caller.cpp:2633-2751): the intake of a file's reads (read_hts_and_return_realignment_indels,
:2232-2509), the buckets (:2490-2500, include/graphtyper/typer/bucket.hpp:33-43), the file's list of indels (:2641-2735 with
:2914-2946) and the reads an indel's round looks at (realign_to_indels, :1876-1958).  Strings, lists, sets and dicts only: it knows
nothing of bit planes, groups of 32 bases, atomics, scans or sorted arrays.  It follows the text, not the comments:

  * the file's buckets are made new (:2649-2650), so add_indel_event_to_bucket inserts a fresh EventSupport whose
    has_realignment_support is false (event.hpp:101): every I and D that reaches the score pays 7 + (count - 1) * 1, and :2404 is
    never taken.  The CIGAR indels live in the bucket's map (here: the set `events`), never in the global table.
  * score, pos_end and end_with_clip are int32_t (read.hpp:43-45, :2491), the clip counts int16_t (read.hpp:46-47); the penalty of
    :2402 / :2437 is unsigned arithmetic.  The conversions are two's complement.

Where the reference is undefined, the library's stated rules (include/gtx.h): the bases of an M behind the region's end or behind
the read's last base are not compared and add nothing; a read that starts at or behind the region's end is passed over.

A second, independent statement of the score and the ends is column_statement(): the CIGAR expanded into alignment columns, and
the columns counted.  tests/test_disc_second_emu.py holds the two to each other.

    A read: dict(pos, cigar [raw BAM words], seq [seq_nt16_str letters], flag, mapq).
    A table entry: dict(pos, type 'I' | 'D', seq, span, good, file_index); the table is in Event order (table_order).
    A read's state: dict(pos, pos_end, score, num_clipped_begin, num_clipped_end, num_ins_begin, flags, mapq, l_qseq, bucket) or None
    when the intake passes it over; a read's entries: [(table index, read_pos)]."""

CIGAR_MAP = ['M', 'I', 'D', 'N', 'S', 'H', 'P', '=', 'X', 'B', '*', '*', '*', '*', '*', '*']  # caller.cpp:2258-2259
SCORE_MATCH, SCORE_MISMATCH, SCORE_GAP_OPEN, SCORE_GAP_EXTEND, SCORE_CLIP = 1, 4, 7, 1, 5  # constants.hpp.in:49-53
IS_CLIPPED = 8192                                                                           # constants.hpp.in:94
READ_ANTI_SUPPORT, READ_MULTI_SUPPORT = -1, -2                                              # read.hpp:15-16
PAD = 50                                                                                    # caller.cpp:1863
NEARBY_BP = 60                                                                              # caller.cpp:2685


def i16(v):
    return ((v & 0xFFFF) ^ 0x8000) - 0x8000


def i32(v):
    return ((v & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def u32(v):
    return v & 0xFFFFFFFF


def n_buckets(ref_size, bucket_size):
    """every read that is not passed over lies below it; NUM_BUCKETS and the resizes of bucket.cpp:95-96 differ only in empty buckets"""
    return (ref_size - 1) // bucket_size + 1


def table_order(entry):
    """Event::operator< (src/typer/event.cpp:173-181): position; insertions before deletions; the sequence"""
    return (entry["pos"], (entry["type"] == 'D') + 2 * (entry["type"] == 'X'), entry["seq"])


def intake_read(reference, region_begin, read, events):
    """:2247-2491 for one read.  events: the file's bucket maps as one set of (pos, type, letters), which a CIGAR indel joins.
    -> (state without its bucket, end_with_clip) or None"""
    ref_size = len(reference)
    pos, cigar, sequence = read["pos"], read["cigar"], read["seq"]
    if len(cigar) == 0 or pos < region_begin:  # :2247
        return None
    read_offset = 0                             # :2267
    ref_offset = pos - region_begin             # :2270
    if ref_offset >= ref_size:                  # :2283 the reference ends the process; the library passes the read over
        return None
    flags = read["flag"]                        # :2305
    score = 0                                   # :2322
    num_clipped_begin = num_clipped_end = 0     # read.hpp:46-47
    for i, word in enumerate(cigar):            # :2324
        if ref_offset >= ref_size:              # :2326
            break
        operation = CIGAR_MAP[word & 15]        # :2342
        count = word >> 4                       # :2343
        if operation in ('M', '=', 'X'):        # :2348-2350
            for r in range(min(count, ref_size - ref_offset, max(len(sequence) - read_offset, 0))):  # :2355 (the stated limit cuts it)
                alt = sequence[r + read_offset]             # :2357
                ref = reference[ref_offset + r]
                if alt != ref and alt != 'N' and ref != 'N':  # :2359
                    score = i32(score - SCORE_MISMATCH)
                else:
                    score = i32(score + SCORE_MATCH)
            read_offset += count                # :2369
            ref_offset += count                 # :2370
        elif operation == 'I':                  # :2374
            begin = read_offset if read_offset < len(sequence) else len(sequence)                     # :2378
            end = read_offset + count if read_offset + count < len(sequence) else len(sequence)       # :2381
            if begin == end:                    # :2385 (the read offset stays)
                continue
            events.add((u32(region_begin + ref_offset), 'I', sequence[begin:end]))                    # :2392-2399
            score = i32(score - u32(SCORE_GAP_OPEN + u32(count - 1) * SCORE_GAP_EXTEND))              # :2401-2402 (fresh support: never :2404)
            read_offset += count                # :2407
        elif operation == 'D':                  # :2411
            if ref_offset + count >= ref_size:  # :2415 nothing happens, the loop goes on
                continue
            events.add((u32(region_begin + ref_offset), 'D', reference[ref_offset:ref_offset + count]))  # :2427-2434
            score = i32(score - u32(SCORE_GAP_OPEN + u32(count - 1) * SCORE_GAP_EXTEND))              # :2436-2437
            ref_offset += count                 # :2440
        elif operation == 'S':                  # :2444
            read_offset += count                # :2446
            flags |= IS_CLIPPED                 # :2447
            score = i32(score - SCORE_CLIP)     # :2448
            if i == 0:                          # :2450
                num_clipped_begin = i16(count)  # :2452
            else:
                num_clipped_end = i16(count)    # :2480 (every other S; the last one wins)
        # :2484 anything else moves neither the reference nor the read
    pos_end = i32(region_begin + ref_offset)    # :2489
    end_with_clip = i32(pos_end + num_clipped_end)  # :2491
    state = dict(pos=pos, pos_end=pos_end, score=score, num_clipped_begin=num_clipped_begin, num_clipped_end=num_clipped_end, num_ins_begin=0,
                 flags=flags, mapq=read["mapq"], l_qseq=len(sequence))
    return state, end_with_clip


def intake(reference, region_begin, bucket_size, reads):
    """the whole file (:2649-2651, :2243-2506) -> dict(reads [state or None], max_pos_end, global_max_pos_end [per bucket],
    bucket_reads [per bucket, the stream indices in stream order], max_read_size, events)"""
    ref_size = len(reference)
    nb = n_buckets(ref_size, bucket_size)
    max_pos_end, global_of, bucket_reads = [-1] * nb, [-1] * nb, [[] for _ in range(nb)]  # :2649-2650, bucket.hpp:36-37
    max_read_size = 100                         # :2651
    global_max_pos_end = 0                      # :2241
    events, states = set(), []
    for i, read in enumerate(reads):
        got = intake_read(reference, region_begin, read, events)
        if got is None:
            states.append(None)
            continue
        state, end_with_clip = got
        bucket_index = (read["pos"] - region_begin) // bucket_size  # :2273
        if len(read["seq"]) > max_read_size:    # :2276
            max_read_size = len(read["seq"])
        if end_with_clip > max_pos_end[bucket_index]:               # :2493
            max_pos_end[bucket_index] = end_with_clip               # :2495
            global_max_pos_end = max(global_max_pos_end, end_with_clip)  # :2496
        global_of[bucket_index] = global_max_pos_end                # :2499
        bucket_reads[bucket_index].append(i)                        # :2500
        state["bucket"] = bucket_index
        states.append(state)
    return dict(reads=states, max_pos_end=max_pos_end, global_max_pos_end=global_of, bucket_reads=bucket_reads, max_read_size=max_read_size, events=events)


def found_bits(table, events):
    """is_indel_in_bucket (src/typer/bucket.cpp:66-79) per table entry: the file holds the event (Event::operator==, event.cpp:163-166)"""
    return [(u32(e["pos"]), e["type"], e["seq"]) in events for e in table]


def plan(table, found, file_index):
    """:2914-2946 and :2641-2735 -> the file's list as table indices.  The library's rule where the reference leaves the outcome to
    std::sort: every indel once, ties in table order"""
    own = [t for t, e in enumerate(table) if not e["good"] and e["file_index"] == file_index]  # :2926, :2944
    if len(own) == 0:                           # :2641
        return []
    nearby = []
    for indel in own:                           # :2687
        t = indel
        while t != 0:                           # :2692
            t -= 1
            if table[t]["good"] and table[t]["pos"] + NEARBY_BP >= table[indel]["pos"]:   # :2696
                if found[t]:                    # :2699
                    nearby.append(t)
        t = indel + 1                           # :2705
        while t != len(table):                  # :2707
            if table[t]["good"] and table[t]["pos"] - NEARBY_BP <= table[indel]["pos"]:   # :2709
                if found[t]:                    # :2712
                    nearby.append(t)
            t += 1
    chosen = sorted(set(own) | set(nearby))     # every indel once (:2720-2726 under the library's rule)
    return sorted(chosen, key=lambda t: (not table[t]["good"], table[t]["pos"], t))  # :2728-2735, ties in table order


def has_indel_event(entries, t):
    """Alignment::has_indel_event (src/typer/read.cpp:13-22): the first entry that names the indel decides"""
    for table_index, read_pos in entries:
        if table_index == t:
            return read_pos != READ_ANTI_SUPPORT
    return False


def round_reads(table, t, taken, states, entries, region_begin, bucket_size):
    """the reads the round of table entry t looks at, in its order of visit (:1876-1958).  taken: intake()'s result (the bucket
    maxima are the intake's); states / entries: the reads' CURRENT state and entries"""
    indel = table[t]
    indel_span = indel["pos"] + indel["span"]   # :1880
    max_read_size = taken["max_read_size"]
    nb = len(taken["max_pos_end"])
    begin_padded = max(0, indel["pos"] - max_read_size - 2 * PAD - region_begin)  # :1890
    end_padded = indel["pos"] + max_read_size + 2 * PAD - region_begin             # :1892
    b = begin_padded // bucket_size             # :1911
    b_end = min(nb - 1, end_padded // bucket_size)  # :1912
    if b >= nb or end_padded < 0:               # :1891, :1913 assert otherwise
        return []
    while b > 0 and taken["global_max_pos_end"][b] > indel["pos"] - PAD:  # :1919
        b -= 1
    out = []
    while b <= b_end:                           # :1923
        if taken["max_pos_end"][b] <= indel["pos"] - PAD:  # :1929
            b += 1
            continue
        for i in taken["bucket_reads"][b]:      # :1932
            r = states[i]
            if r is None or r["pos"] < 0 or r["l_qseq"] == 0:  # :1941
                continue
            if has_indel_event(entries[i], t):  # :1945
                continue
            if (r["num_clipped_end"] == 0 and r["pos_end"] < indel["pos"]) or \
               (r["pos_end"] + r["num_clipped_end"] + min(r["num_clipped_end"], PAD) < indel["pos"]) or \
               (r["num_clipped_begin"] == 0 and r["pos"] > indel_span) or \
               (r["pos"] - r["num_clipped_begin"] - min(r["num_clipped_begin"], PAD) > indel_span):  # :1948-1955
                continue
            out.append(i)
        b += 1
    return out


def candidates(table, lst, k0, k1, taken, states, entries, region_begin, bucket_size):
    """the (read, list position) pairs of the rounds k0 .. k1 - 1 of a list, in the reference's order of visit"""
    return [(i, k) for k in range(k0, k1) for i in round_reads(table, lst[k], taken, states, entries, region_begin, bucket_size)]


# ---- the second statement: alignment columns ------------------------------------------------------------------------------------
def inside(reference, region_begin, read):
    """the CIGAR stays inside the read and the region: its query length is l_qseq, and the reference offset stays below REF_SIZE
    through every operation (so no operation is cut, dropped or undefined)"""
    if len(read["cigar"]) == 0 or read["pos"] < region_begin:
        return False
    q, r = 0, read["pos"] - region_begin
    for word in read["cigar"]:
        op, count = CIGAR_MAP[word & 15], word >> 4
        if count == 0:
            return False
        if op in ('M', '=', 'X'):
            q, r = q + count, r + count
        elif op in ('I', 'S'):
            q += count
        elif op == 'D':
            r += count
        if r >= len(reference):
            return False
    return q == len(read["seq"])


def column_statement(reference, region_begin, read):
    """for a read that is inside(): the alignment written out as columns (read letter or None, region letter or None), soft clips as
    runs of their own, then counted -> (score, pos_end, num_clipped_begin, num_clipped_end, clipped)"""
    columns, clips = [], []
    q, r = 0, read["pos"] - region_begin
    n_ops = len(read["cigar"])
    for i, word in enumerate(read["cigar"]):
        op, count = CIGAR_MAP[word & 15], word >> 4
        for _ in range(count):
            if op in ('M', '=', 'X'):
                columns.append((read["seq"][q], reference[r], i))
                q, r = q + 1, r + 1
            elif op == 'I':
                columns.append((read["seq"][q], None, i))
                q += 1
            elif op == 'D':
                columns.append((None, reference[r], i))
                r += 1
            elif op == 'S':
                q += 1
        if op == 'S':
            clips.append((i, count))
    pairs = [(a, g) for a, g, _ in columns if a is not None and g is not None]
    mismatches = sum(1 for a, g in pairs if a != g and 'N' not in (a, g))
    gap_runs = {}
    for a, g, i in columns:
        if a is None or g is None:
            gap_runs[i] = gap_runs.get(i, 0) + 1
    score = (len(pairs) - mismatches) - 4 * mismatches - sum(7 + (n - 1) for n in gap_runs.values()) - 5 * len(clips)
    pos_end = read["pos"] + sum(1 for a, g, _ in columns if g is not None)
    begin = [n for i, n in clips if i == 0]
    end = [n for i, n in clips if i != 0]
    assert n_ops > 0
    return score, pos_end, i16(begin[0]) if begin else 0, i16(end[-1]) if end else 0, len(clips) > 0
