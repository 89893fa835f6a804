"""Pair sets of the realignment tests (test_realign_emu.py on the host emulation, test_gpu_realign.py on the device): each is
(reads, targets, pairs) -- reads as tuples of 4-bit codes, targets as strings of letters, pairs as (read, target) -- and each
is held to tests/realign_ref.py field by field."""
import functools
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


@functools.lru_cache(maxsize=None)
def simulated(seed=5, n_pairs=300):
    """simulated reads with substitutions, indels and soft-clipped junk ends over windows gtx_disc_realign_target makes from
    simulated indels; several reads per window, the pairs shuffled.  Also returns the windows' (ref_pos, begin_padded, indel)."""
    import ctypes as C
    from graphtyper_amd import lib as gtx
    rng = random.Random(seed)
    region_begin, max_read = 20000, 60
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


SETS = {"indels_at_rows": indels_at_rows, "mismatch_runs_and_clips": mismatch_runs_and_clips, "codes_n_iupac": codes_n_iupac, "ties": ties,
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
def arrays(reads, targets, pairs):
    from graphtyper_amd import lib as gtx
    longest = max([len(r) for r in reads if len(r) <= rr.MAX_READ] + [1])
    plane_stride = (longest + 31) // 32 * 16
    cd = np.zeros((len(reads), plane_stride * 2), np.uint8)
    for i, r in enumerate(reads):
        k = min(len(r), plane_stride * 2)  # (a read beyond the limits keeps its length; its row holds its first bases only)
        cd[i, :k] = r[:k]
    planes = gtx.planes_reference(cd, plane_stride)
    lens = np.array([len(r) for r in reads], np.uint16)
    off = np.zeros(len(targets) + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in targets])
    seq = np.frombuffer("".join(targets).encode(), np.uint8).copy()
    pr = np.array(pairs, np.uint32).reshape(-1, 2).view(gtx.REALIGN_PAIR).reshape(-1)
    return planes, plane_stride, lens, seq, off, pr


def as_tuples(results):
    return [(int(r["score"]), int(r["clip_begin"]), int(r["clip_end"]), int(r["target_begin"]), int(r["target_end"]), int(r["status"])) for r in results]
