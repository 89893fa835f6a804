"""The realignment of reads to indel haplotypes restated in plain Python (include/gtx.h: gtx_disc_realign_*): the alignment as
its definition reads, over full tables, and the reference's text around it -- apply_indel_event
(src/typer/event.cpp:293-396), the window (src/typer/caller.cpp:1890-1907), the overlap test (:1941-1958) and the decision
(:2025-2153).  Nothing here is shared with the library's sources; the tests hold the library to this file."""
import functools

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND, CLIP = 1, -4, 7, 1, 5  # include/graphtyper/constants.hpp.in:49-53
PAD = 50  # caller.cpp:1863
OK, BAD_PAIR, TOO_LONG = 0, 1, 2
MAX_READ, MAX_TARGET = 256, 2048
NO_PADDING, BETTER, SAME_OVERLAPPING, SAME, WORSE = 0, 1, 2, 3, 4
NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
CODE_LETTER = "=ACMGRSVTWYHKDBN"


def nt16(letter):
    """htslib's seq_nt16_table over letters (either case) and '='; anything else is N.  letter: a one-letter str, or a byte's
    value (what iterating over bytes gives): a byte that is no ASCII character is no letter"""
    if isinstance(letter, int):
        if not 0 <= letter < 128:
            return 15
        letter = chr(letter)
    return NT16.get(letter.upper(), 15)


def codes_of(text):
    """text: str or bytes"""
    return tuple(nt16(c) for c in text)


UNIT = 1 << 24  # a value is score * UNIT + (4095 - db) * 4096 + (4095 - cb): integer order is then "higher score, smaller db, smaller cb"


@functools.lru_cache(maxsize=None)
def align(q, t):
    """q, t: tuples of 4-bit codes -> (score, clip_begin, clip_end, target_begin, target_end), by the definition over full tables"""
    m, n = len(q), len(t)
    assert 1 <= m < 4096 and 1 <= n < 4096
    NEG = -10 ** 6 * UNIT
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    best_key, best_value = None, None  # key: (score, -j, -i)
    OPEN, EXTEND = GAP_OPEN * UNIT, GAP_EXTEND * UNIT
    for i in range(1, m + 1):
        qi = q[i - 1]
        start = (0 if i == 1 else -CLIP) * UNIT + (4095 - (i - 1))
        pay = CLIP if i < m else 0
        Hi, Ei, Fi, Hu, Fu = H[i], E[i], F[i], H[i - 1], F[i - 1]
        row_best, row_j, row_value = -10 ** 6, 0, 0  # within a row the smaller j wins a tie: strict "greater" in column order
        for j in range(1, n + 1):
            tj = t[j - 1]
            S, d = start + (4096 - j) * 4096, Hu[j - 1]  # (the ifs are max(): a call costs as much as the rest of the cell)
            if d > S:
                S = d
            S += UNIT if (qi == tj or qi == 15 or tj == 15) else MISMATCH * UNIT
            e, x = Hi[j - 1] - OPEN, Ei[j - 1] - EXTEND
            if x > e:
                e = x
            f, x = Hu[j] - OPEN, Fu[j] - EXTEND
            if x > f:
                f = x
            Ei[j], Fi[j] = e, f
            h = S if S > e else e
            Hi[j] = h if h > f else f
            score = S >> 24
            if score > row_best:
                row_best, row_j, row_value = score, j, S
        key = (row_best - pay, -row_j, -i)
        if best_key is None or key > best_key:
            best_key, best_value = key, row_value
    origin = best_value & (UNIT - 1)
    return best_key[0], 4095 - (origin & 4095), -best_key[2], 4095 - (origin >> 12), -best_key[1]


def result(reads, targets, pair):
    """what gtx_disc_realign_batch writes for `pair` = (read, target): (score, clip_begin, clip_end, target_begin, target_end,
    status); reads: tuples of codes, targets: strings of letters"""
    r, w = pair
    if r >= len(reads) or w >= len(targets) or len(reads[r]) == 0 or len(targets[w]) == 0:
        return (0, 0, 0, 0, 0, BAD_PAIR)
    if len(reads[r]) > MAX_READ or len(targets[w]) > MAX_TARGET:
        return (0, 0, 0, 0, 0, TOO_LONG)
    return align(tuple(reads[r]), codes_of(targets[w])) + (OK,)


def result_in_arena(reads, arena, off, pair):
    """the same for windows given as the entry point takes them: `arena` (bytes) holds the letters, window w is
    arena[off[w]:off[w + 1]], len(off) - 1 windows, off[-1] the arena's size.  A window whose offsets are not in order, or whose
    end lies behind off[-1], is a bad pair."""
    r, w = pair
    n_targets = len(off) - 1
    if r >= len(reads) or w >= n_targets or len(reads[r]) == 0:
        return (0, 0, 0, 0, 0, BAD_PAIR)
    t0, t1 = int(off[w]), int(off[w + 1])
    if t1 <= t0 or t1 > int(off[n_targets]):
        return (0, 0, 0, 0, 0, BAD_PAIR)
    if len(reads[r]) > MAX_READ or t1 - t0 > MAX_TARGET:
        return (0, 0, 0, 0, 0, TOO_LONG)
    return align(tuple(reads[r]), codes_of(bytes(arena[t0:t1]))) + (OK,)


# ---- the reference's text around the aligner -------------------------------------------------------------------------------
def apply_indel_event(sequence, ref_positions, pos_, type_, letters, offset):
    """event.cpp:293-396 over two lists, changed in place; letters: the event's sequence (a deletion's: only its length counts)"""
    ref_pos = pos_ - offset
    if ref_pos <= 0:
        return False
    pos = ref_pos
    event_size, seq_size = len(letters), len(sequence)
    if pos >= seq_size:
        return False
    if ref_positions[pos] != ref_pos:
        while pos + 1 < seq_size and ref_positions[pos] < ref_pos:
            pos += 1
        while pos > 0 and ref_positions[pos] > ref_pos:
            pos -= 1
        if ref_positions[pos] != ref_pos:
            return False
    begin, end = max(0, pos - 3), min(len(ref_positions), pos + 3)
    prev = ref_positions[begin]
    for p in range(begin + 1, end):
        if ref_positions[p] == prev + 1:
            prev += 1
        else:
            return False
    if type_ == "D":
        if pos + event_size >= len(ref_positions) or ref_positions[pos + event_size] != ref_pos + event_size:
            return False
        del sequence[pos:pos + event_size]
        del ref_positions[pos:pos + event_size]
    elif type_ == "I":
        sequence[pos:pos] = list(letters)
        ref_positions[pos + 1:pos + 1] = [pos + 1] * event_size
    else:
        return False
    return True


def target(reference, region_begin, max_read_size, events):
    """caller.cpp:1890-1907 and :1968-2002.  events: [(pos, type, letters)], events[0] the indel being realigned to ->
    (letters, ref_pos, begin_padded, applied bits)"""
    REF_SIZE = len(reference)
    pos = events[0][0]
    begin_padded = max(0, pos - max_read_size - 2 * PAD - region_begin)
    assert begin_padded < REF_SIZE
    end_padded = pos + max_read_size + 2 * PAD - region_begin
    new_ref = list(reference[begin_padded:] if end_padded >= REF_SIZE else reference[begin_padded:end_padded])
    ref_pos = list(range(len(new_ref)))
    applied = 0
    if apply_indel_event(new_ref, ref_pos, *events[0], begin_padded + region_begin):
        applied = 1
        for e, ev in enumerate(events[1:], 1):
            if apply_indel_event(new_ref, ref_pos, *ev, begin_padded + region_begin):
                applied |= 1 << e
    return "".join(new_ref), ref_pos, begin_padded, applied


def wants(pos, pos_end, num_clipped_begin, num_clipped_end, indel_pos, span):
    """caller.cpp:1941-1958"""
    indel_span = indel_pos + span
    if pos < 0:
        return 0
    if ((num_clipped_end == 0 and pos_end < indel_pos) or
            (pos_end + num_clipped_end + min(num_clipped_end, PAD) < indel_pos) or
            (num_clipped_begin == 0 and pos > indel_span) or
            (pos - num_clipped_begin - min(num_clipped_begin, PAD) > indel_span)):
        return 0
    return 1


def decide(res, read_len, ref_pos, begin_padded, region_begin, old_score, indel_pos):
    """caller.cpp:2025-2153.  res: (score, clip_begin, clip_end, target_begin, target_end) ->
    (outcome, pos, pos_end, num_clipped_begin, num_clipped_end, num_ins_begin), zeros unless BETTER"""
    score, clip_begin, clip_end, database_begin, database_end = res[:5]
    if database_begin == 0 or database_end == len(ref_pos):
        return (NO_PADDING, 0, 0, 0, 0, 0)
    if score <= old_score:
        if score < old_score:
            return (WORSE, 0, 0, 0, 0, 0)
        if ref_pos[database_begin] + begin_padded <= indel_pos <= ref_pos[database_end] + begin_padded:
            return (SAME_OVERLAPPING, 0, 0, 0, 0, 0)
        return (SAME, 0, 0, 0, 0, 0)
    num_ins = 0
    while database_begin + num_ins + 1 < len(ref_pos) and ref_pos[database_begin + num_ins] == ref_pos[database_begin + num_ins + 1]:
        num_ins += 1
    return (BETTER, ref_pos[database_begin] + region_begin + begin_padded, ref_pos[database_end] + region_begin + begin_padded, clip_begin,
            read_len - clip_end, num_ins)
