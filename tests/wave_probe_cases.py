"""The wave policy's probe (graphtyper_amd/csrc/wave_probe.hpp): its input sets, and in plain Python what it must write for a set --
the definition of every primitive of the policy's table (graph_dev.hpp), taken from neither implementation.  Both sides are held to
it word for word: the sequential wave by tests/test_wave_seq.py (tests/emu_wave), the hardware wave by tests/test_gpu_wave.py
(gtx_wave_probe).  All values are integers; there is no tolerance."""
import random

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
LANES = 64

# the layout (the WP_* constants of wave_probe.hpp; test_wave_seq.py reads the header and compares)
IN = dict(A=0, B=64, FLAG=128, K=192, FIRST=193, START32=194, START64=195, WORDS=200)
OUT = dict(SHIFT=0, SHIFT2=64, SCAN=128, CLAIM=192, ACLAIM=256, FROM_LANE=320, UNI32=321, UNI64=322, BALLOT=324, SUM=326, MAX=327,
           SCAN_TOTAL=328, CLAIM_CTR=329, ACLAIM_CTR=330, ADD32=331, ADD64=332, SUB32=334, MAXU32=335, OR64=336, MAXI32=338, OR32=339,
           WORDS=340)
NO_SLOT = M32

# where a DPP row ends and the next begins (15 | 16, 31 | 32: the second is also the boundary of the wavefront's halves), and the ends
EDGE_LANES = (0, 15, 16, 31, 32, 63)


class Set:
    def __init__(self, name, a, b, flag, k, first, start32, start64):
        assert len(a) == len(b) == len(flag) == LANES
        self.name, self.a, self.b, self.flag = name, [x & M32 for x in a], [x & M32 for x in b], [bool(x) for x in flag]
        self.k, self.first, self.start32, self.start64 = k, first & M32, start32 & M32, start64 & M64

    def words(self):
        w = np.zeros(IN["WORDS"], dtype=np.uint32)
        w[IN["A"]:IN["A"] + LANES] = self.a
        w[IN["B"]:IN["B"] + LANES] = self.b
        w[IN["FLAG"]:IN["FLAG"] + LANES] = [3 if f else 0 for f in self.flag]  # (a flag is "not zero")
        w[IN["K"]], w[IN["FIRST"]], w[IN["START32"]] = self.k, self.first, self.start32
        w[IN["START64"]], w[IN["START64"] + 1] = self.start64 & M32, self.start64 >> 32
        return w


def signed(x):
    return x - (1 << 32) if x & 0x80000000 else x


def expected(s):
    """the words a probe of set `s` must write: the definition"""
    o = [0] * OUT["WORDS"]

    def put(name, v):
        if isinstance(v, list):
            o[OUT[name]:OUT[name] + len(v)] = v
        else:
            o[OUT[name]] = v

    def put64(name, v):
        o[OUT[name]], o[OUT[name] + 1] = v & M32, v >> 32

    a, b, k = s.a, s.b, s.k & 63
    in_flag = [l for l in range(LANES) if s.flag[l]]
    wide = [(a[l] << 32) | b[l] for l in range(LANES)]
    # shift_up: every lane's value one lane up, lane 0 receives `first`; in place it is the same, so twice is two lanes up
    put("SHIFT", [s.first] + a[:-1])
    put("SHIFT2", [s.first, s.first] + a[:-2])
    # excl_scan: lane l gets the sum of the lanes below it, total the sum of all 64; sums wrap modulo 2^32
    put("SCAN", [sum(a[:l]) & M32 for l in range(LANES)])
    put("SCAN_TOTAL", sum(a) & M32)
    put("SUM", sum(a) & M32)
    put("MAX", max(a))
    put("FROM_LANE", a[k])
    # uni: the value all lanes hold
    put("UNI32", s.first ^ k)
    put64("UNI64", (s.first << 32) | s.start32)
    # ballot: bit l is lane l's flag
    put64("BALLOT", sum(1 << l for l in in_flag))
    # claim_u32: the wave takes n = first once; every lane gets the old value
    put("CLAIM", [s.start32] * LANES)
    put("CLAIM_CTR", (s.start32 + s.first) & M32)
    # atomic_claim_u32: the lanes that call it get base + their rank among the callers, in lane order
    put("ACLAIM", [(s.start32 + in_flag.index(l)) & M32 if s.flag[l] else NO_SLOT for l in range(LANES)])
    put("ACLAIM_CTR", (s.start32 + len(in_flag)) & M32)
    # the atomics: every flagged lane's contribution has arrived
    put("ADD32", (s.start32 + sum(b[l] for l in in_flag)) & M32)
    put("SUB32", (s.start32 - sum(b[l] for l in in_flag)) & M32)
    put("MAXU32", max([s.start32] + [b[l] for l in in_flag]))
    put("MAXI32", max([signed(s.start32)] + [signed(b[l]) for l in in_flag]) & M32)
    or32, or64 = s.start32, s.start64
    for l in in_flag:
        or32 |= b[l]
        or64 |= wide[l]
    put("OR32", or32)
    put64("ADD64", (s.start64 + sum(wide[l] for l in in_flag)) & M64)
    put64("OR64", or64)
    return np.array(o, dtype=np.uint32)


def flag_patterns(rng):
    return [("none", [0] * LANES), ("all", [1] * LANES), ("lane0", [1] + [0] * 63), ("lane63", [0] * 63 + [1]),
            ("alternating", [l & 1 for l in range(LANES)]), ("random", [rng.getrandbits(1) for _ in range(LANES)])]


def make_sets():
    rng = random.Random(20240611)
    r32 = lambda: rng.getrandbits(32)
    flags = flag_patterns(rng)
    sets = []
    # the maximum at each edge lane (the others below 2^31, so it is the only one), k there too, and each flag pattern once
    for i, p in enumerate(EDGE_LANES):
        a = [rng.getrandbits(31) for _ in range(LANES)]
        a[p] = 0x80000000 | rng.getrandbits(31)
        name, flag = flags[i]
        sets.append(Set("max_at_%d_flags_%s" % (p, name), a, [r32() for _ in range(LANES)], flag, p, r32(), r32(), rng.getrandbits(64)))
    lane = list(range(LANES))
    # values equal to the lane index: what went where is readable off the output; k beyond 63 (the low six bits count)
    sets.append(Set("lane_index", lane, [l + 1 for l in lane], [1] * LANES, 64 + 15, 1000, 0, 0))
    # all equal, and large: the sums wrap (64 x 0x84000001 = 0x40 mod 2^32 at the top lane, earlier inside the scan), every lane holds the maximum
    sets.append(Set("all_equal", [0x84000001] * LANES, [0x84000001] * LANES, [1] * LANES, 31, 0x84000001, M32, M64))
    # random 32-bit values, with a k of the other edge lanes than above
    for i, p in enumerate(EDGE_LANES):
        name, flag = flags[(i + 3) % 6]
        sets.append(Set("random_k_%d_flags_%s" % (p, name), [r32() for _ in range(LANES)], [r32() for _ in range(LANES)], flag, p, r32(), r32(),
                        rng.getrandbits(64)))
    # counters that start above every contribution, as unsigned and as signed numbers: the maxima stay where they are
    small = [rng.getrandbits(20) for _ in range(LANES)]
    sets.append(Set("start_above_unsigned", small, small, [1] * LANES, 16, 5, M32, 1 << 63))
    sets.append(Set("start_above_signed", small, [x | 0x80000000 for x in small], [1] * LANES, 32, 5, 0x7FFFFFFF, 0))
    # ... and below every one: the signed minimum against negative contributions, zero against unsigned ones
    sets.append(Set("start_below_signed", small, [x | 0x80000000 for x in small], flags[4][1], 15, 0, 0x80000000, 0))
    return sets


SETS = make_sets()
# how many sets a call gets: one wavefront of a workgroup of four; a full workgroup; a full one and a partly filled one; all of them
COUNTS = (1, 4, 5, len(SETS))


def case_words(n):
    return np.concatenate([s.words() for s in SETS[:n]])


def expected_words(n):
    return np.concatenate([expected(s) for s in SETS[:n]])


def differences(n, got):
    """[] or (set, output field, lane or word, got, want) of the first words that differ"""
    want, bad = expected_words(n), []
    assert got.shape == want.shape, (got.shape, want.shape)
    fields = sorted((v, k) for k, v in OUT.items() if k != "WORDS")
    for at in np.nonzero(got != want)[0][:8]:
        s, w = divmod(int(at), OUT["WORDS"])
        start, field = [f for f in fields if f[0] <= w][-1]
        bad.append((SETS[s].name, field, w - start, hex(int(got[at])), hex(int(want[at]))))
    return bad
