"""Pair sets of the long realignment's tests (test_realign_long_emu.py on the host emulation, test_gpu_realign_long.py on the
device): reads of 257 .. 1 000 bases and windows of up to 4 095 letters, what a gtx_disc aligns after
gtx_disc_set_max_read_len(d, 1000).  Each set is (reads, targets, pairs) as in realign_cases.py and is held to
tests/realign_ref.py field by field, with the long limits applied here (result(): realign_ref's own constants stay as they are).

The restatement does about 0.6 M cells a second, so the shapes are as small as the boundaries allow.  Cells per set: row_boundaries
2.9 M, column_boundaries 3.4 M, both_limits 8.3 M (its three pairs are 4.1 M, 2.2 M and 2.0 M), clips 0.7 M, ties 1.1 M,
mixed_batch 0.4 M, rows_behind_the_read 0.5 M; the two fact sets (planted, reversed) do not go through the restatement."""
import functools
import random

import numpy as np

import realign_cases as rc
import realign_ref as rr
from realign_cases import as_tuples, codes, other, rnd  # noqa: F401

MAX_READ_LONG, MAX_TARGET_LONG = 1000, 4095
BAD, TOO_LONG = (0, 0, 0, 0, 0, rr.BAD_PAIR), (0, 0, 0, 0, 0, rr.TOO_LONG)


def result(reads, targets, pair, max_read=MAX_READ_LONG):
    """realign_ref.result under the limits in force on an object with gtx_disc_set_max_read_len(d, max_read): max_read <= 256 is
    the default (256 bases, 2 048 letters), else max_read bases and 4 095 letters"""
    r, w = pair
    if r >= len(reads) or w >= len(targets) or len(reads[r]) == 0 or len(targets[w]) == 0:
        return BAD
    long_mode = max_read > rr.MAX_READ
    if len(reads[r]) > (max_read if long_mode else rr.MAX_READ) or len(targets[w]) > (MAX_TARGET_LONG if long_mode else rr.MAX_TARGET):
        return TOO_LONG
    t = targets[w]
    return rr.align(tuple(reads[r]), rr.codes_of(t)) + (rr.OK,)


def stride_of(reads):
    """the narrowest plane rows that hold the longest read within the long limit"""
    return (max([len(r) for r in reads if len(r) <= MAX_READ_LONG] + [1]) + 31) // 32 * 16


def arrays(reads, targets, pairs, plane_stride=None, dirty=False):
    return rc.arrays(reads, targets, pairs, plane_stride=plane_stride or stride_of(reads), dirty=dirty)


def edited(rng, text):
    """`text` less a 3-base gap, with two substitutions: three letters shorter"""
    r = list(text)
    n = len(r)
    if n >= 12:
        for k in (n // 5, n // 2):
            r[k] = other(rng, r[k])
        del r[2 * n // 3:2 * n // 3 + 3]
    return "".join(r)


ROW_M = (256, 257, 319, 320, 321, 383, 384, 385, 511, 512, 513, 767, 768, 769, 959, 960, 961, 999, 1000)
ROW_N = (97, 130)


def row_boundaries():
    """every m at which a lane's last row, the number of rows per lane or the number of lanes changes, each against windows of 97
    and 130 letters cut around a planted copy (the window is a piece of the read with two substitutions and a 3-base gap) and
    against one unrelated window"""
    rng = random.Random(101)
    reads, targets, pairs = [], [rnd(rng, 33)], []
    for m in ROW_M:
        r = rnd(rng, m)
        reads.append(codes(r))
        for n in ROW_N:
            a = rng.randrange(0, m - n - 3)
            targets.append(edited(rng, r[a:a + n + 3]))
            assert len(targets[-1]) == n
            pairs.append((len(reads) - 1, len(targets) - 1))
        pairs.append((len(reads) - 1, 0))
    return reads, targets, pairs


COLUMN_N = (1, 63, 64, 65, 2047, 2048, 2049, 4094, 4095)


def column_boundaries():
    """reads of 40 and 257 bases against windows at the sizes where a block of 64 columns, the short limit and the long limit
    end; the copy planted at the window's first base, its last base, and across letters 2 047 / 2 048; 4 096 letters: too long.
    The read of 40 meets every size, the read of 257 all but 2 047 and 2 048 (1.05 M cells more for two shapes that only differ
    from 2 049 on the short side of the dispatch, which the read of 40 takes there)."""
    rng = random.Random(103)
    reads, targets, pairs = [], [], []

    def add(m, n, where):
        if m >= n:
            r = rnd(rng, m)
            a = rng.randrange(0, m - n + 1)
            t = r[a:a + n]
        else:
            t = rnd(rng, n)
            a = {"first": 0, "last": n - m, "across": 2047 - m // 2}[where]
            r = t[a:a + m]
        reads.append(codes(r))
        targets.append(t)
        pairs.append((len(reads) - 1, len(targets) - 1))

    places = {2047: ("first",), 2048: ("last",), 2049: ("across", "last"), 4094: ("first", "across"), 4095: ("last", "first")}
    for n in COLUMN_N:
        for where in places.get(n, ("first", "last")):
            add(40, n, where)
        if n < 2047:
            add(257, n, "first")  # (the window is a piece of the read)
        elif n > 2048:
            add(257, n, places[n][0])
    add(40, 4096, "last")
    return reads, targets, pairs


def both_limits():
    """1 000 x 4 095 with the read equal to the window's last 1 000 letters (score 1 000, db 3 095, cb 0: the top of every field
    at once); 1 000 x 2 200, the workload's own shape, the read carrying a 2-base deletion and a 5-base insertion against its
    haplotype window; 961 x 2 049"""
    rng = random.Random(107)
    t0 = rnd(rng, 4095)
    hap = rnd(rng, 2200)
    r1 = hap[600:900] + hap[902:1300] + rnd(rng, 5) + hap[1300:1597]
    assert len(r1) == 1000
    t2 = rnd(rng, 2049)
    r2 = list(t2[500:1461])
    for k in (100, 480, 900):
        r2[k] = other(rng, r2[k])
    return [codes(t0[-1000:]), codes(r1), codes("".join(r2))], [t0, hap, t2], [(0, 0), (1, 1), (2, 2)]


NOT_LETTERS = rc.NOT_LETTERS


def clips():
    """windows of at most 200 letters: reads of 1 000 bases of which only the last 30 and only the first 30 align, reads of which only one base aligns;
    N bases in read and window; lower case and bytes that are no letters in the window"""
    rng = random.Random(109)
    reads, targets, pairs = [], [], []

    def add(r, t):
        reads.append(r if isinstance(r, tuple) else codes(r))
        targets.append(t)
        pairs.append((len(reads) - 1, len(targets) - 1))

    t = rnd(rng, 200)
    add(rnd(rng, 969) + other(rng, t[49]) + t[50:80], t)    # (the base in front of the copy is not the window's)
    add(t[120:150] + other(rng, t[150]) + rnd(rng, 969), t)  # (nor the one behind it)
    add("A" * 998 + "C", "G" * 50 + "C" + "G" * 49)  # one base aligns, the read's last of 999: -5 to start there, +1, nothing to pay
    add("A" * 998 + "C" + "A", "G" * 99 + "C")       # the same base as the last but one: -9, as every mismatch in row 1 -- the rule names (1, 1)
    t = list(rnd(rng, 200))
    r = list("".join(t[20:180]) + rnd(rng, 240))
    for k in (30, 31, 90, 150):
        t[k] = "N"
    for k in (5, 63, 64, 100, 159, 300):
        r[k] = "N"
    add("".join(r), "".join(t))
    t = rnd(rng, 150)
    differs = list(t)
    raw = bytearray("".join(c.lower() if i % 3 else c for i, c in enumerate(t)).encode())
    for k, b in zip((20, 33, 64, 90, 120, 149), NOT_LETTERS):
        raw[k] = b
        differs[k] = other(rng, t[k])  # (as N the byte matches, as the letter it replaced it would not)
    add(rnd(rng, 80) + "".join(differs[10:]) + rnd(rng, 80), bytes(raw))
    return reads, targets, pairs


def ties():
    """tandem repeats of period 1, 2, 7 and 64, reads of 300 and 520 bases inside the repeat and longer than it, windows of 600 ..
    700: equal scores that differ only in db, cb, j or i"""
    rng = random.Random(113)
    reads, targets, pairs = [], [], []

    def add(r, t):
        assert len(r) in (300, 520) and 600 <= len(t) <= 700
        reads.append(codes(r))
        targets.append(t)
        pairs.append((len(reads) - 1, len(targets) - 1))

    add("A" * 300, rnd(rng, 200, "CGT") + "A" * 200 + rnd(rng, 200, "CGT"))  # longer than the repeat
    add("AC" * 260, rnd(rng, 100) + "AC" * 225 + rnd(rng, 100))            # longer than the repeat
    u = "ACGGTCA"
    add(u * 42 + u[:6], rnd(rng, 150) + u * 57 + rnd(rng, 151))              # inside the repeat
    u = rnd(rng, 64)
    add(u * 8 + u[:8], rnd(rng, 64) + u * 8 + rnd(rng, 64))                  # one unit's start longer than the repeat
    return reads, targets, pairs


def mixed_batch():
    """short pairs, long pairs, bad pairs, a read of 1 001 bases and a window of 4 096 letters, interleaved so that neighbours of
    every kind meet in one workgroup of four wavefronts; 27 pairs.  Eight reads and read index 8: the lengths end right there;
    the empty read meets the long window too (an empty pair is bad before it is short or long)"""
    rng = random.Random(127)
    t = rnd(rng, 150)
    long_t = rnd(rng, 2049)
    r300 = rnd(rng, 300)
    targets = [t, long_t, rnd(rng, 4096), "", edited(rng, r300[100:233])]
    reads = [codes(t[30:90]), codes(r300), codes(rnd(rng, 257)), (), codes(rnd(rng, 1001)), codes(long_t[2020:2049]), codes(t[60:140]), codes(t[10:50])]
    S, L, B, X = [(0, 0), (6, 0), (0, 0), (6, 0)], [(1, 4), (2, 0), (5, 1), (1, 0)], [(3, 0), (0, 3), (8, 0), (0, 5), (0xFFFFFFFF, 0), (3, 1)], [(4, 0), (0, 2), (4, 2)]
    pairs = [S[0], L[0], B[0], X[0],  L[1], L[2], S[1], S[2],  B[1], B[2], L[3], X[1],  X[2], S[3], S[0], L[0],  B[3], X[0], B[4], B[5],
             L[1], X[1], L[0], S[1],  S[2], B[1], L[2]]
    assert len(pairs) % 4 == 3
    return reads, targets, pairs


def rows_behind_the_read():
    """read lengths that leave a lane's last rows behind the read's last base, over a short window that ends with the read's last 40
    bases and N or '=' right behind them: rows that do not exist must not score there.  And a read of 200 bases against 2 049
    letters: the one shape that takes four rows per lane in the long kernel (129 .. 256 bases are the short kernel's unless the
    window is long)"""
    rng = random.Random(139)
    reads, targets, pairs = [], [], []
    for m, tail in ((257, "NNN"), (511, "==="), (513, "N=N"), (999, "NNNN")):
        r = rnd(rng, m)
        reads.append(codes(r))
        targets.append(rnd(rng, 10) + r[-40:] + tail + rnd(rng, 10))
        pairs.append((len(reads) - 1, len(targets) - 1))
    t = rnd(rng, 2049)
    reads.append(codes(edited(rng, t[1800:2003])))
    targets.append(t)
    pairs.append((len(reads) - 1, len(targets) - 1))
    return reads, targets, pairs


def kind_of(reads, targets, pair):
    """'short', 'long' (aligned in long mode only), 'bad' or 'beyond' (too long in either mode)"""
    a, b = result(reads, targets, pair, 0), result(reads, targets, pair)
    return "bad" if b == BAD else "beyond" if b == TOO_LONG else "long" if a == TOO_LONG else "short"


SETS = {"row_boundaries": row_boundaries, "column_boundaries": column_boundaries, "both_limits": both_limits, "clips": clips, "ties": ties,
        "mixed_batch": mixed_batch, "rows_behind_the_read": rows_behind_the_read}


@functools.lru_cache(maxsize=None)
def get(name):
    return SETS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's results of a set under the long limits, computed once"""
    reads, targets, pairs = get(name)
    return [result(reads, targets, p) for p in pairs]


# the sets as the entry point takes them, and row_boundaries over other rows: exactly as wide as each read (one batch per m; the
# emulation gives every pair rows of its own size anyway), and rows of 1 024 bases with every bit behind a read's end set
def _short_row_case():
    """a length beyond what the plane row holds: too long, whatever the limit in force says"""
    reads, targets, pairs = [(1,) * 300, (2,) * 290], ["ACGT" * 20], [(0, 0), (1, 0), (0, 0)]
    planes, plane_stride, lens, seq, off, pr = arrays(reads, targets, pairs)
    assert plane_stride == 160
    lens[0] = 321
    return (planes, plane_stride, lens, seq, off, pr), [TOO_LONG, result(reads, targets, (1, 0)), TOO_LONG]


def _offsets_case():
    """hand-made offsets: a window of 2 100 letters that ends behind the arena's 100, and one whose offsets are not in order: bad
    pairs, of which nothing but the offsets may be read"""
    reads, pairs = [codes("ACGT" * 10)], [(0, 0), (0, 1), (0, 0)]
    planes, plane_stride, lens, _, _, pr = arrays(reads, [], pairs)
    return (planes, plane_stride, lens, np.frombuffer(b"ACGT" * 25, np.uint8).copy(), np.array([0, 2100, 100], np.uint32), pr), [BAD] * 3


ENTRY = {"offsets_by_hand": _offsets_case, "row_boundaries_wide_dirty": lambda: (arrays(*get("row_boundaries"), plane_stride=512, dirty=True), expected("row_boundaries")),
         "short_row": _short_row_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """a set or an entry-point case as ((planes, plane_stride, lens, seq, off, pairs), the expected tuples)"""
    if name in SETS:
        return arrays(*get(name)), expected(name)
    return ENTRY[name]()


def row_case(m):
    """the three pairs of row_boundaries' read of m bases over plane rows exactly as wide as that read (dirty behind its end)"""
    reads, targets, pairs = get("row_boundaries")
    k = ROW_M.index(m)
    mine = pairs[3 * k:3 * k + 3]
    assert all(p[0] == k for p in mine)
    return arrays([reads[k]], targets, [(0, w) for _, w in mine], plane_stride=(m + 31) // 32 * 16, dirty=True), expected("row_boundaries")[3 * k:3 * k + 3]


# ---- facts that do not go through the restatement ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(n_pairs=60, seed=131):
    """a read that is a copy of 257 .. 1 000 window letters with k <= 5 substitutions, each at least 40 bases from either end
    and from each other, scores exactly m - 5k with cb 0, clip_end m and target_begin the copy's place (through a substitution:
    at least 40 - 4 more, around it by a clip or a gap: less) -> (reads, targets, pairs), the expected tuples"""
    rng = random.Random(seed)
    reads, targets, pairs, want = [], [], [], []
    for p in range(n_pairs):
        m, n = (rng.randrange(257, 1001), rng.randrange(2049, 4096)) if p >= 4 else ((257, 2049), (1000, 4095), (257, 4095), (1000, 2049))[p]
        t = rnd(rng, n)
        at = rng.choice((0, n - m, rng.randrange(0, n - m + 1)))
        r = list(t[at:at + m])
        places = []
        for _ in range(p % 6):
            k = rng.randrange(40, m - 40)
            if all(abs(k - x) >= 40 for x in places):
                places.append(k)
                r[k] = other(rng, r[k])
        reads.append(codes("".join(r)))
        targets.append(t)
        pairs.append((p, p))
        want.append((m - 5 * len(places), 0, m, at, at + m, rr.OK))
    return (reads, targets, pairs), want


@functools.lru_cache(maxsize=None)
def reversed_pairs(n_couples=40, seed=137):
    """couples (q, t), (reversed q, reversed t) -- pairs 2k and 2k + 1 -- whose scores are equal because the model is symmetric
    under reversal; m in 257 .. 1 000, n in 2 049 .. 4 095; every other read carries substitutions, an N and a gap, the rest
    are unrelated letters"""
    rng = random.Random(seed)
    reads, targets, pairs = [], [], []
    for k in range(n_couples):
        m, n = rng.randrange(257, 1001), rng.randrange(2049, 4096)
        t = rnd(rng, n)
        if k % 2 == 0:
            a = rng.randrange(0, n - m - 3)
            r = list(edited(rng, t[a:a + m + 3]))
            r[m // 7] = "N"
            r = "".join(r)
        else:
            r = rnd(rng, m)
        assert len(r) == m
        for q, w in ((r, t), (r[::-1], t[::-1])):
            reads.append(codes(q))
            targets.append(w)
            pairs.append((len(reads) - 1, len(targets) - 1))
    return reads, targets, pairs


# ---- through tests/emu_realign_long -----------------------------------------------------------------------------------------
def write_case(path, max_read, planes, plane_stride, lens, seq, off, pr):
    """the case file of tests/emu_realign_long: the limit in force, then the case file of tests/emu_realign"""
    with open(path, "wb") as f:
        f.write(np.array([max_read, plane_stride, len(lens), len(off) - 1, len(pr), len(seq)], np.uint32).tobytes())
        f.write(planes.tobytes())
        f.write(lens.tobytes() + b"\0\0" * (len(lens) & 1))
        f.write(off.tobytes())
        f.write(seq.tobytes() + b"\0" * (-len(seq) % 4))
        f.write(pr.tobytes())


def through(run, arrays_, max_read=MAX_READ_LONG):
    """what arrays() returns through tests/emu_realign_long; run(write, read): emu_programs.run with a program and a directory ->
    the results as tuples"""
    from graphtyper_amd import lib as gtx
    return run(lambda path: write_case(path, max_read, *arrays_), lambda path: as_tuples(np.fromfile(path, gtx.REALIGN_RESULT)))


# what the mutation audit (tests/realign_long_mutants) runs: the sets, the entry-point case, the planted pairs, the short
# kernel's simulated set on a long-mode object, and mixed_batch at a limit of 257
AUDIT_CASES = sorted(SETS) + sorted(ENTRY) + ["planted", "short_simulated", "mixed_batch_257", "rows_exact"]


def judge(name, run):
    """None when the program behind `run` gives the case `name` as expected, else how it differs"""
    if name == "planted":
        (reads, targets, pairs), want = planted()
        got = through(run, arrays(reads, targets, pairs))
    elif name == "short_simulated":
        arrays_, want = rc.case("simulated")
        got = through(run, arrays_)
    elif name == "mixed_batch_257":
        reads, targets, pairs = get("mixed_batch")
        want = [result(reads, targets, p, 257) for p in pairs]
        got = through(run, arrays(reads, targets, pairs), 257)
    elif name == "rows_exact":
        got, want = [], []
        for m in ROW_M:
            a, w = row_case(m)
            got += through(run, a)
            want += w
    else:
        arrays_, want = case(name)
        got = through(run, arrays_)
    return None if got == want else "differs from what is expected"
