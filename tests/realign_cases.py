"""Pair sets of the realignment tests (test_realign_emu.py on the host emulation, test_gpu_realign.py on the device): each is
(reads, targets, pairs) -- reads as tuples of 4-bit codes, targets as strings of letters, pairs as (read, target) -- and each
is held to tests/realign_ref.py field by field."""
import functools
import itertools
import random

import numpy as np

import realign_ref as rr

ACGT = "ACGT"
M_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
N_SIZES = (1, 2, 63, 64, 65, 300, 2048)


def rnd(rng, n, alphabet=ACGT):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(rng, c):
    return rng.choice([x for x in ACGT if x != c])


def codes(text):
    return rr.codes_of(text)


def cross(n):
    """every m of M_SIZES against a window of n letters: a piece of the window with a substitution and (where there is room) a
    deleted base when the read is shorter than the window, letters of its own around the whole window when it is longer"""
    rng = random.Random(1000 + n)
    target = rnd(rng, n)
    reads = []
    for m in M_SIZES:
        if m < n:
            a = rng.randrange(0, n - m)
            r = list(target[a:a + m + 1])
            if m > 20:
                r[m // 3] = other(rng, r[m // 3])
                del r[2 * m // 3]
            r = "".join(r[:m])
        else:
            k = rng.randrange(0, m - n + 1)
            r = rnd(rng, k) + target + rnd(rng, m - n - k)
        assert len(r) == m
        reads.append(codes(r))
    return reads, [target], [(i, 0) for i in range(len(reads))]


def indels_at_rows():
    """an insertion and a deletion of 1, 7 and 30 bases that begin at query rows 62, 63, 64 and at a lane's last row, for every R"""
    rng = random.Random(7)
    reads, targets, pairs = [], [], []
    for R, m in ((1, 64), (2, 128), (3, 192), (4, 256)):
        rows = {62, 63, 64, R * 9, R * (m // R - 12)}  # R * k: the last row lane k - 1 owns
        for row in sorted(rows):
            for length in (1, 7, 30):
                for kind in "ID":
                    t = rnd(rng, m + 140)
                    a = 50
                    left = t[a:a + row - 1]  # query rows 1 .. row - 1
                    if kind == "I":
                        r = left + rnd(rng, length) + t[a + row - 1:]
                    else:
                        r = left + t[a + row - 1 + length:]
                    reads.append(codes(r[:m]))
                    targets.append(t)
                    pairs.append((len(reads) - 1, len(targets) - 1))
    return reads, targets, pairs


def mismatch_runs_and_clips():
    rng = random.Random(11)
    reads, targets, pairs = [], [], []

    def add(r, t):
        reads.append(codes(r))
        targets.append(t)
        pairs.append((len(reads) - 1, len(targets) - 1))

    for run in (7, 8, 12, 20):  # a run of mismatches in the middle: an insertion plus a deletion (2 * 7 + run - 1 ... ) against 4 * run
        t = rnd(rng, 220)
        r = list(t[60:160])
        for k in range(45, 45 + run):
            r[k] = other(rng, r[k])
        add("".join(r), t)
    # two close mismatches near an end: `a` bases between them, `b` behind the last.  Through them: a + b - 8; the clip: -5.
    for a, b in ((1, 3), (1, 2), (1, 1), (0, 4), (0, 3), (0, 2), (2, 2), (2, 1), (3, 1)):
        for where in ("begin", "end", "both"):
            t = rnd(rng, 200)
            r = list(t[50:130])
            if where in ("end", "both"):
                for k in (len(r) - 1 - b, len(r) - 2 - b - a):
                    r[k] = other(rng, r[k])
            if where in ("begin", "both"):
                for k in (b, b + 1 + a):
                    r[k] = other(rng, r[k])
            add("".join(r), t)
    # junk ends that must be clipped
    t = rnd(rng, 300)
    add(rnd(rng, 25) + t[100:180] + rnd(rng, 30), t)
    return reads, targets, pairs


def codes_n_iupac():
    rng = random.Random(13)
    reads, targets, pairs = [], [], []
    t = rnd(rng, 180)
    base = t[40:120]
    with_n = list(t)
    for k in (60, 61, 90):
        with_n[k] = "N"
    iupac = list(t)
    iupac[70] = "R"  # code 5: a mismatch against A (1) and against G (4), a match against a read's R only
    iupac[71] = "="
    targets += [t, "".join(with_n), "".join(iupac), "N" * 100]
    r_n = list(codes(base))
    for k in (5, 30, 31, 79):
        r_n[k] = 15
    r_iu = list(codes(base))
    r_iu[30] = 5 if r_iu[30] != 5 else 3
    r_iu[50] = 0
    reads += [codes(base), tuple(r_n), tuple(r_iu), (15,) * 40]
    pairs = [(r, w) for r in range(4) for w in range(4)]
    return reads, targets, pairs


def ties():
    """equally good alignments: all four end points must follow the rule"""
    rng = random.Random(17)
    reads, targets, pairs = [], [], []

    def add(r, t):
        reads.append(codes(r))
        targets.append(t)
        pairs.append((len(reads) - 1, len(targets) - 1))

    left, right = rnd(rng, 40), rnd(rng, 40)
    for unit, copies in (("A", 30), ("AC", 15), ("ACG", 10)):
        t = left + unit * copies + right
        add(unit * 5, t)                                              # inside the repeat
        add((unit * 40)[:70], t)                                      # longer than the repeat: clips or gaps
        add(left[-20:] + unit * (copies + 2) + right[:20], t)         # an insertion of two units in the repeat
        add(left[-20:] + unit * (copies - 2) + right[:20], t)         # a deletion of two units
        add(left[-20:] + unit * (copies + 1) + right[:20], t)
        add(left[-20:] + unit * (copies - 1) + right[:20], t)
    piece = rnd(rng, 35)
    add(piece, rnd(rng, 30) + piece + rnd(rng, 50) + piece + rnd(rng, 30))  # two places, equally good
    add(piece[:20] + rnd(rng, 3) + piece[20:], rnd(rng, 30) + piece + rnd(rng, 50) + piece + rnd(rng, 30))
    add("A" * 64, "A" * 64)
    add("A" * 65, "A" * 64)
    add("AC" * 64, "AC" * 100)
    return reads, targets, pairs


def no_padding():
    """alignments that touch column 0 or column n"""
    rng = random.Random(19)
    t = rnd(rng, 200)
    reads = [codes(t[:60]), codes(t[140:]), codes(t), codes(rnd(rng, 10) + t[:50]), codes(t[150:] + rnd(rng, 10)), codes(t[1:61]), codes(t[139:199])]
    return reads, [t], [(i, 0) for i in range(len(reads))]


def bad_and_long():
    """pairs with bad indices and with sizes beyond the limits between good ones"""
    rng = random.Random(23)
    t = rnd(rng, 150)
    targets = [t, rnd(rng, 2049), "", rnd(rng, 2048)]
    reads = [codes(t[30:90]), codes(rnd(rng, 257)), (), codes(rnd(rng, 300)), codes(t[60:140])]
    pairs = [(0, 0), (5, 0), (0, 4), (4, 0), (1, 0), (0, 1), (0, 0), (2, 0), (0, 2), (3, 1), (4, 3), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (4, 0), (1, 4)]
    return reads, targets, pairs


SIMULATED_REGION_BEGIN = 20000


def n_behind_the_read():
    """read lengths that leave a lane's last rows behind the read's last base (m no multiple of R), over a window that has the
    read in it with N or '=' right behind: rows that do not exist must not score there (forced by the mutation audit of
    tests/realign_mutants: a kernel whose rows behind the read paid nothing passed every other set)"""
    rng = random.Random(53)
    reads, targets, pairs = [], [], []
    for m in (65, 127, 130, 131, 190, 193, 253, 254, 255):
        for tail in ("NNN", "===", "N=N"):
            r = rnd(rng, m)
            reads.append(codes(r))
            targets.append(rnd(rng, 30) + r + tail + rnd(rng, 30))
            pairs.append((len(reads) - 1, len(targets) - 1))
    return reads, targets, pairs


def bad_indices():
    """an even number of reads and of windows, with pairs that name the read and the window one behind the last (the arrays of
    lengths and of offsets end right there) between good ones"""
    rng = random.Random(47)
    t = rnd(rng, 90)
    reads, targets = [codes(t[10:50]), codes(t[40:80])], [t, t[::-1]]
    return reads, targets, [(0, 0), (2, 0), (1, 0), (0, 2), (1, 1), (2, 2), (3, 1), (1, 3), (0, 1)]


@functools.lru_cache(maxsize=None)
def simulated(seed=5, n_pairs=300):
    """simulated reads with substitutions, indels and soft-clipped junk ends over windows gtx_disc_realign_target makes from
    simulated indels; several reads per window, the pairs shuffled.  Also returns the windows' (ref_pos, begin_padded, indel)."""
    import ctypes as C
    from graphtyper_amd import lib as gtx
    rng = random.Random(seed)
    region_begin, max_read = SIMULATED_REGION_BEGIN, 60
    reference = rnd(rng, 3000)
    h = C.c_void_p()
    gtx.check(gtx.lib().gtx_disc_create(reference.encode(), len(reference), region_begin, -1, C.byref(h)))
    reads, targets, pairs, windows = [], [], [], []
    try:
        while len(pairs) < n_pairs:
            pos = region_begin + rng.randrange(100, len(reference) - 100)
            kind = rng.choice("ID")
            length = rng.choice((1, 2, 3, 7, 15, 30))
            event = (pos, kind, rnd(rng, length))
            letters, ref_pos, begin_padded, applied = gtx.disc_realign_target(h, max_read, [event])
            assert (letters.decode(), list(ref_pos), begin_padded, applied) == rr.target(reference, region_begin, max_read, [event])
            if not applied & 1:
                continue
            w = len(targets)
            targets.append(letters.decode())
            windows.append((ref_pos, begin_padded, event))
            at = pos - begin_padded - region_begin  # the indel's index in the window
            for _ in range(rng.randrange(3, 8)):
                hap = targets[w] if rng.random() < 0.7 else reference[begin_padded:begin_padded + len(letters)]
                m = rng.randrange(30, max_read + 1)
                a = max(0, min(len(hap) - m, at - rng.randrange(0, m)))
                r = list(hap[a:a + m])
                for k in range(len(r)):
                    if rng.random() < 0.02:
                        r[k] = other(rng, r[k])
                if rng.random() < 0.15 and len(r) > 20:
                    k = rng.randrange(5, len(r) - 5)
                    r[k:k] = list(rnd(rng, rng.randrange(1, 4)))
                if rng.random() < 0.15 and len(r) > 20:
                    k = rng.randrange(5, len(r) - 8)
                    del r[k:k + rng.randrange(1, 4)]
                if rng.random() < 0.2:
                    r[:rng.randrange(1, 12)] = list(rnd(rng, rng.randrange(1, 12)))
                if rng.random() < 0.2:
                    r[-rng.randrange(1, 12):] = list(rnd(rng, rng.randrange(1, 12)))
                reads.append(codes("".join(r)[:max_read]))
                pairs.append((len(reads) - 1, w))
    finally:
        gtx.lib().gtx_disc_destroy(h)
    pairs = pairs[:n_pairs]
    rng.shuffle(pairs)
    return reads, targets, pairs, windows


def exhaustive(alphabet, m_max, n_max):
    """every read of up to m_max and every window of up to n_max letters of `alphabet`, each read against each window"""
    def strings(longest):
        return ["".join(s) for k in range(1, longest + 1) for s in itertools.product(alphabet, repeat=k)]

    reads, targets = [codes(r) for r in strings(m_max)], strings(n_max)
    return reads, targets, [(r, w) for r in range(len(reads)) for w in range(len(targets))]


def exhaustive_ac():
    """{A,C}, m <= 5, n <= 6: 62 reads x 126 windows = 7 812 pairs, where tie-breaks and the E / F / S maxima at equal score decide"""
    return exhaustive("AC", 5, 6)


def exhaustive_acn():
    """{A,C,N}, m <= 4, n <= 4: 120 reads x 120 windows = 14 400 pairs"""
    return exhaustive("ACN", 4, 4)


REVERSED_N = (64, 65, 300)


def reversed_pairs():
    """couples (q, t), (reversed q, reversed t) -- pairs 2k and 2k + 1 -- whose scores are equal because the model is symmetric
    under reversal (the end points need not be): a witness for reads of more than 64 bases that does not go through the
    restatement.  For every m of M_SIZES and n of REVERSED_N: a read cut from the window (the whole window with letters of its
    own around it when the read is the longer) with two substitutions, an N and a deleted base, and a read of unrelated letters."""
    rng = random.Random(29)
    reads, targets, pairs = [], [], []

    def add(r, t):
        for rr_, tt in ((r, t), (r[::-1], t[::-1])):
            reads.append(codes(rr_))
            targets.append(tt)
            pairs.append((len(reads) - 1, len(targets) - 1))

    for m in M_SIZES:
        for n in REVERSED_N:
            t = rnd(rng, n)
            if m < n:
                a = rng.randrange(0, n - m)
                r = list(t[a:a + m + 1])
            else:
                k = rng.randrange(0, m - n + 1)
                r = list(rnd(rng, k) + t + rnd(rng, m + 1 - n - k))
            if m >= 8:
                for k in (m // 5, m // 2):
                    r[k] = other(rng, r[k])
                r[m // 3] = "N"
                del r[2 * m // 3]
            r = "".join(r[:m])
            assert len(r) == m
            add(r, t)
            add(rnd(rng, m), t)
    return reads, targets, pairs


def limits():
    """the largest sizes: 256 bases against 2048 letters with the read at the window's last 256 letters and at its first 256,
    and one base against 2048 letters of which only the last matches"""
    rng = random.Random(31)
    t = rnd(rng, 2048)
    reads = [codes(t[-256:]), codes(t[:256]), codes("C")]
    return reads, [t, "A" * 2047 + "C"], [(0, 0), (1, 0), (2, 1)]


def decision_cases():
    """(set, reads, pairs, windows) of the sets that have window records: simulated(), and no_padding with a plain window (the
    simulated windows are padded well, so none of their alignments touches an end)"""
    reads, _, pairs, windows = simulated()
    yield "simulated", reads, pairs, windows
    reads, targets, pairs = get("no_padding")
    yield "no_padding", reads, pairs, [(np.arange(len(targets[0]), dtype=np.int32), 400, (SIMULATED_REGION_BEGIN + 500, "D", "A"))]


def decisions(name, results, old_deltas=(-1, 0, 1)):
    """the arguments of the decision for every pair of a set of decision_cases() over `results` (tuples) -- old_score = score + each delta; the
    indel's position as a contig position (what the reference's text passes) and as a region position (what its comparison with
    ref_pos + begin_padded would need to hold) -- and the restatement's decision"""
    reads, pairs, windows = next(c[1:] for c in decision_cases() if c[0] == name)
    out = []
    for res, (r, w) in zip(results, pairs):
        ref_pos, begin_padded, event = windows[w]
        for d in old_deltas:
            for indel_pos in (event[0], event[0] - SIMULATED_REGION_BEGIN):
                args = (res[:5], len(reads[r]), ref_pos, begin_padded, SIMULATED_REGION_BEGIN, res[0] + d, indel_pos)
                out.append((args, rr.decide(res, len(reads[r]), list(ref_pos), *args[3:])))
    return out


def outcomes(name):
    return {d[0] for _, d in decisions(name, expected(name))}


SETS = {"bad_indices": bad_indices, "n_behind_the_read": n_behind_the_read, "exhaustive_ac": exhaustive_ac, "exhaustive_acn": exhaustive_acn, "reversed_pairs": reversed_pairs, "limits": limits, "indels_at_rows": indels_at_rows, "mismatch_runs_and_clips": mismatch_runs_and_clips, "codes_n_iupac": codes_n_iupac, "ties": ties,
        "no_padding": no_padding, "bad_and_long": bad_and_long, "simulated": lambda: simulated()[:3]}
SETS.update({"cross_n%d" % n: functools.partial(cross, n) for n in N_SIZES})


@functools.lru_cache(maxsize=None)
def get(name):
    return SETS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's results of a set, computed once"""
    reads, targets, pairs = get(name)
    return [rr.result(reads, targets, p) for p in pairs]


# ---- the arrays the entry point (and the emulation's case file) take ---------------------------------------------------------
def arrays(reads, targets, pairs, plane_stride=None, dirty=False):
    """plane_stride: the rows' stride when it is to be wider than the longest read needs; dirty: every plane bit at and behind
    position len(read) of a row is 1 in all four planes (the lengths stay as they are)"""
    from graphtyper_amd import lib as gtx
    longest = max([len(r) for r in reads if len(r) <= rr.MAX_READ] + [1])
    if plane_stride is None:
        plane_stride = (longest + 31) // 32 * 16
    assert plane_stride % 16 == 0 and plane_stride >= (longest + 31) // 32 * 16
    cd = np.zeros((len(reads), plane_stride * 2), np.uint8)
    for i, r in enumerate(reads):
        k = min(len(r), plane_stride * 2)  # (a read beyond the limits keeps its length; its row holds its first bases only)
        cd[i, :k] = r[:k]
        if dirty:
            cd[i, k:] = 15
    planes = gtx.planes_reference(cd, plane_stride)
    lens = np.array([len(r) for r in reads], np.uint16)
    off = np.zeros(len(targets) + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in targets])
    seq = np.frombuffer(b"".join(t if isinstance(t, bytes) else t.encode() for t in targets), np.uint8).copy()
    pr = np.array(pairs, np.uint32).reshape(-1, 2).view(gtx.REALIGN_PAIR).reshape(-1)
    return planes, plane_stride, lens, seq, off, pr


def as_tuples(results):
    return [(int(r["score"]), int(r["clip_begin"]), int(r["clip_end"]), int(r["target_begin"]), int(r["target_end"]), int(r["status"])) for r in results]


# ---- paths of the entry point that arrays() alone never takes ---------------------------------------------------------------
NOT_LETTERS = (ord("-"), ord("*"), 0x00, 0xC1, 0xE1, 0x1D)  # (0xC1, 0xE1: 'A' and 'a' with the top bit set; 0x1D: '=' less the case bit)


def _offsets_case():
    """hand-made offsets over one arena: unused letters in front, windows that share letters, windows whose offsets are not in
    order and one that ends behind the arena's end, between good ones"""
    rng = random.Random(37)
    arena = rnd(rng, 300).encode()
    # windows 0 and 2 share [100, 237); 1 and 4: off[w + 1] < off[w]; 3 ends at 400, behind the arena's 300; 5 is empty
    off = np.array([37, 237, 100, 300, 400, 150, 150, 290, 300], np.uint32)
    reads = [codes(arena[60:120].decode()), codes(arena[120:200].decode()), codes(arena[160:280].decode())]
    pairs = [(r, w) for w in range(len(off) - 1) for r in range(len(reads))]
    planes, plane_stride, lens, _, _, pr = arrays(reads, [], pairs)
    return (planes, plane_stride, lens, np.frombuffer(arena, np.uint8).copy(), off, pr), [rr.result_in_arena(reads, arena, off, p) for p in pairs]


def _front_case():
    reads, targets, pairs = get("ties")
    planes, plane_stride, lens, seq, off, pr = arrays(reads, targets, pairs)
    front = np.frombuffer(rnd(random.Random(41), 37).encode(), np.uint8)
    return (planes, plane_stride, lens, np.concatenate([front, seq]), off + np.uint32(37), pr), expected("ties")


def _letters_case(how):
    reads, targets, pairs = get("codes_n_iupac")
    if how == "lower":
        targets = [t.lower() for t in targets]
    else:
        targets = ["".join(c.lower() if (k * 7 + i) % 3 else c for i, c in enumerate(t)) for k, t in enumerate(targets)]
    assert all(a != b.upper() or a == "=" * len(a) for a, b in zip(targets, get("codes_n_iupac")[1]))
    return arrays(reads, targets, pairs), expected("codes_n_iupac")


def _not_letters_case():
    """bytes that are no letters act as N: the results are those of the window with an N in their places"""
    rng = random.Random(43)
    t = rnd(rng, 120)
    at = (20, 33, 34, 50, 64, 90)
    raw, with_n = bytearray(t.encode()), list(t)
    for k, b in zip(at, NOT_LETTERS):
        raw[k], with_n[k] = b, "N"
    differs = list(t)  # the reads differ from the window's own letters at those places: as N they match, as anything else they do not
    for k in at:
        differs[k] = other(rng, t[k])
    differs = "".join(differs)
    reads = [codes(differs[10:70]), codes(differs[30:100]), codes(differs[15:40] + differs[41:95])]
    pairs = [(r, 0) for r in range(3)]
    want = [rr.result(reads, ["".join(with_n)], p) for p in pairs]
    assert want == [rr.result_in_arena(reads, bytes(raw), [0, len(raw)], p) for p in pairs]
    assert want != [rr.result(reads, [t], p) for p in pairs]
    return arrays(reads, [bytes(raw)], pairs), want


def _short_row_case():
    """a length beyond what the plane row holds: too long, whatever the limit on reads says"""
    planes, plane_stride, lens, seq, off, pr = arrays([(1,) * 40, (2,) * 33], ["ACGT" * 20], [(0, 0), (1, 0), (0, 0)])
    assert plane_stride == 32
    lens[0] = 65
    return (planes, plane_stride, lens, seq, off, pr), [(0, 0, 0, 0, 0, rr.TOO_LONG), rr.result([(1,) * 40, (2,) * 33], ["ACGT" * 20], (1, 0)), (0, 0, 0, 0, 0, rr.TOO_LONG)]


def _rows_case(name, wide=False, dirty=False):
    def make():
        tight = arrays(*get(name))[1]
        return arrays(*get(name), plane_stride=4 * tight if wide else tight, dirty=dirty), expected(name)
    return make


ENTRY = {"wide_ties": _rows_case("ties", wide=True), "wide_cross_n65": _rows_case("cross_n65", wide=True),  # rows four times as wide as needed
         "dirty_ties": _rows_case("ties", dirty=True), "dirty_cross_n65": _rows_case("cross_n65", dirty=True),
         "wide_dirty_ties": _rows_case("ties", wide=True, dirty=True), "wide_bad_and_long": _rows_case("bad_and_long", wide=True),  # (rows that could hold 257 bases)
         "short_row": _short_row_case, "offsets_by_hand": _offsets_case, "letters_in_front": _front_case,
         "lower_case": lambda: _letters_case("lower"), "mixed_case": lambda: _letters_case("mixed"), "not_letters": _not_letters_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """a pair set or an entry-point case as ((planes, plane_stride, lens, seq, off, pairs), the expected tuples)"""
    if name in SETS:
        return arrays(*get(name)), expected(name)
    return ENTRY[name]()


def write_case(path, planes, plane_stride, lens, seq, off, pr):
    """the case file of tests/emu_realign"""
    with open(path, "wb") as f:
        f.write(np.array([plane_stride, len(lens), len(off) - 1, len(pr), len(seq)], np.uint32).tobytes())
        f.write(planes.tobytes())
        f.write(lens.tobytes() + b"\0\0" * (len(lens) & 1))
        f.write(off.tobytes())
        f.write(seq.tobytes() + b"\0" * (-len(seq) % 4))
        f.write(pr.tobytes())


def through(run, arrays):
    """what arrays() returns through tests/emu_realign; run(write, read): emu_programs.run with a program and a directory -> the
    results as tuples"""
    from graphtyper_amd import lib as gtx
    return run(lambda path: write_case(path, *arrays), lambda path: as_tuples(np.fromfile(path, gtx.REALIGN_RESULT)))


def judge(name, run):
    """None when the program behind `run` gives the pair set or entry-point case `name` as the restatement does, else how it differs"""
    arrays, want = case(name)
    return None if through(run, arrays) == want else "differs from the restatement"
