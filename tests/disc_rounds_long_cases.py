"""Cases of the second pass from the aligner on for a gtx_disc with gtx_disc_set_max_read_len(d, 1000): files whose longest read has
more than 256 bases, so that every round's window (2 x max_read_size + 200 letters) is beyond the default aligner's 2 048 letters
or its reads beyond 256 bases.  The restatement is tests/disc_rounds_ref.py with the long limits (1 000 bases, 4 095 letters) set
for the length of a call: expected_long(case); disc_rounds_cases.expected(case) stays what a default object does.  What a case is
for is asserted from the two traces in tests/test_disc_rounds_long_cases.py.  All values are integers or bits."""
import functools

import disc_rounds_cases as rc
import disc_rounds_ref as ref
from disc_rounds_cases import Case, cig, dress, ent, hap_seq, rand_ref, rd

MAX_READ_LONG, MAX_TARGET_LONG = 1000, 4095


@functools.lru_cache(maxsize=None)
def expected_long(case):
    """disc_rounds_cases.expected under the long limits (made once per case; the module's constants are put back)"""
    saved = ref.MAX_READ, ref.MAX_TARGET
    ref.MAX_READ, ref.MAX_TARGET = MAX_READ_LONG, MAX_TARGET_LONG
    try:
        return rc.expected.__wrapped__(case)
    finally:
        ref.MAX_READ, ref.MAX_TARGET = saved


def room_long(case):
    """disc_rounds_cases.room over expected_long"""
    want = expected_long(case)
    out = []
    for k in range(len(want["lst"])):
        a, b = want["before"][k][1], want["before"][k + 1][1]
        out.append((sum(len(e) for e in a), sum(len(y) for x, y in zip(a, b) if x != y)))
    return out


@functools.lru_cache(maxsize=None)
def limits_turned_round():
    """the reads of disc_rounds_cases' `limits` case: on a long-mode object nobody is refused"""
    return rc._limits()


@functools.lru_cache(maxsize=None)
def one_read_of_1000():
    """one read of 1 000 bases that carries a deletion of two (its own round: one pair of 1 000 x 2 198), and reads of 60 bases over a
    deletion of two in front of it and an insertion of 60 letters behind it, neither of which the long read reaches: max_read_size
    is 1 000, so the windows have 2 198 .. 2 260 letters and a default object refuses every pair"""
    reference = rand_ref(4200, 41)
    d_own = (2000, 'D', reference[2000:2002])
    d_front, i_behind = (1440, 'D', reference[1440:1442]), (2570, 'I', rand_ref(60, 42))
    reads = [rd(1500, cig(("M", 1000)), hap_seq(reference, 1500, 1000, [d_own]))]
    for k, start in enumerate(range(1392, 1432, 4)):  # ten reads of the deletion's haplotype, two of the reference
        reads.append(rd(start, cig(("M", 60)), hap_seq(reference, start, 60, [d_front])))
    reads += [rd(1400, cig(("M", 60)), reference[1400:1460]), rd(1415, cig(("M", 60)), reference[1415:1475])]
    for start in (2530, 2540, 2550):                  # reads that run into the inserted letters, one of the reference
        reads.append(rd(start, cig(("M", 60)), hap_seq(reference, start, 60, [i_behind])))
    reads.append(rd(2545, cig(("M", 60)), reference[2545:2605]))
    reads.sort(key=lambda r: r["pos"])
    return Case(reference, 0, dress(reads), [ent(p, k, s) for p, k, s in (d_own, d_front, i_behind)])


def _of_600(rb, region):
    """a file whose longest read has 600 bases (windows of about 1 400 letters): for a deletion of three, reads of 257, 300 and 600
    bases of its haplotype (BETTER), of the reference over it (WORSE) and of the reference up to it (equal; overlapping with
    region_begin 0), and -- 100 letters in front of the region's end -- an insertion whose reads touch the window's last letter"""
    reference = rand_ref(region, 43)
    d = (1000, 'D', reference[1000:1003])
    ins = (region - 100, 'I', "GATTC")
    reads = []
    for m in (257, 300, 600):
        start = 1000 - m // 2
        reads.append(rd(rb + start, cig(("M", m)), hap_seq(reference, start, m, [d])))
        reads.append(rd(rb + start + 3, cig(("M", m)), reference[start + 3:start + 3 + m]))
        reads.append(rd(rb + 1000 - m, cig(("M", m)), reference[1000 - m:1000]))
    reads.append(rd(rb + region - 300, cig(("M", 300)), reference[region - 300:region]))                # to the region's last base
    reads.append(rd(rb + region - 130, cig(("M", 60)), hap_seq(reference, region - 130, 60, [ins])))
    reads.sort(key=lambda r: r["pos"])
    return Case(reference, rb, dress(reads), [ent(rb + p, k, s) for p, k, s in (d, ins)])


@functools.lru_cache(maxsize=None)
def longest_600():
    return [_of_600(0, 2000), _of_600(5000, 2000)]


def all_cases():
    return [("limits_turned_round", limits_turned_round()), ("one_read_of_1000", one_read_of_1000())] + [("longest_600_%d" % i, c) for i, c in enumerate(longest_600())]


def outcomes(trace):
    return {rc.OUTCOME[v[1]] for r in trace["rounds"] for v in r["visits"]}
