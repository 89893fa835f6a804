"""A DEFLATE encoder that is told the structure it writes instead of choosing it (test harness only; written from RFC 1951).
zlib's encoder uses a small corner of the format: codes from real frequency counts, one way of writing a block header, block
ends where its heuristics put them.  This one draws the structure from a seed: the kinds and sizes of the blocks, every length
and distance symbol with its extra bits at 0, at the maximum and in between, matches that read what the match before wrote,
complete prefix codes from flat to 1, 2, 3, ..., 15 whatever the symbols' frequencies are, block headers with HLIT / HDIST
forced, repeats that run from the literal lengths into the distance lengths, a 16 that repeats a zero.  It knows what it wrote,
so it says so (`facts`) and no parser is needed; and it writes members with ONE rule of the format broken on purpose.

    member(seed)          -> (expected bytes, stream, facts)                      a valid member
    largest_tables_member(seed) -> the same, with the codes whose second-level tables are the largest (LARGEST_TABLES)
    invalid_members(seed) -> [(kind, stream, out_len, status or None, reason)]    one per rule

The yardstick of both is zlib's inflate (tests/test_inflate_made_streams.py asserts it before any decoder of the project sees a
member); nothing of the project is used here.  The draws use random.Random(seed).random() only: that sequence is the same on
every Python 3."""
import random

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
BATCH = 64  # the device decoder's batch of tokens (gtx_inflate_dev.hpp: INFL_TOKENS)
MAX_OUT = 65536
BAD_STREAM, SHORT, LONG = 1, 2, 3  # the statuses of include/gtx.h an invalid member is expected to get (None: any of the three)
THEMES = ("any", "full", "deep48", "chains", "counts", "tiny", "wide_header", "stored")
INVALID_KINDS = ("oversubscribed_litlen", "oversubscribed_dist", "oversubscribed_cl", "incomplete_litlen", "incomplete_dist", "incomplete_cl",
                 "one_symbol_cl", "no_end_of_block", "hlit_287", "hlit_288", "hdist_31", "hdist_32", "first_length_is_16", "repeat_past_total",
                 "fixed_litlen_286", "fixed_litlen_287", "fixed_dist_30", "fixed_dist_31", "distance_before_output", "ends_inside_code",
                 "out_len_one_over", "out_len_one_under")


class Rand:
    """the draws, on random.Random.random() alone"""

    def __init__(self, *seed):
        self.r = random.Random("deflate_maker %s" % (seed,))

    def below(self, n):
        return min(int(self.r.random() * n), n - 1)

    def between(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def chance(self, p):
        return self.r.random() < p

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def shuffled(self, seq):
        seq = list(seq)
        for i in range(len(seq) - 1, 0, -1):
            j = self.below(i + 1)
            seq[i], seq[j] = seq[j], seq[i]
        return seq

    def extra(self, bits):
        """a value of `bits` extra bits: 0, the maximum, or anything"""
        top = (1 << bits) - 1
        return (0, top, self.below(top + 1))[self.below(3)]


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, bits):
        """`bits` bits of value, the lowest first (header fields, extra bits)"""
        self.acc |= value << self.n
        self.n += bits
        self.total += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data
        self.total += 8 * len(data)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """the codes of RFC 1951 3.2.2 for the lengths, each already reversed: a Huffman code goes out highest bit first"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lens:
        if n == 0:
            out.append(0)
            continue
        c = nxt[n] & ((1 << n) - 1)  # (lengths broken on purpose may run over: the header is refused before a code is read)
        nxt[n] += 1
        out.append(int(format(c, "0%db" % n)[::-1], 2))
    return out


def split_code(r, n, max_bits, deep):
    """the lengths of a complete prefix code of n >= 2 symbols, made by splitting leaves; `deep` is the chance that a split
    takes the deepest leaf that may still be split: 0 gives flat codes, 1 gives 1, 2, 3, ..., max_bits"""
    assert 2 <= n <= 1 << max_bits
    leaves = [1, 1]
    while len(leaves) < n:
        can = [i for i, d in enumerate(leaves) if d < max_bits]
        if r.chance(deep):
            m = max(leaves[i] for i in can)
            can = [i for i in can if leaves[i] == m]
        d = leaves.pop(r.pick(can))
        leaves += [d + 1, d + 1]
    return leaves


def len_token(length, alt258=False):
    if length == 258:
        return (27, 31) if alt258 else (28, 0)
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return s, length - LEN_BASE[s]


def dist_token(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def new_facts():
    return dict(max_lit_bits=0, max_dist_bits=0, max_cl_bits=0, max_dist_bits_used=0, max_token_bits=0, repeat_across=0, rep16_on_zero=0,
                match_fed_by_match=0, block_end_on_batch=0, stored_offsets=[], hlit_286=0, hdist_30=0, len258_as_285=0, len258_as_284=0,
                dist_32768=0, dist_is_output=0, single_dist_code=0, no_dist_code=0, eob_only_code=0, blocks=[], tokens=0)


class Output:
    """the bytes the tokens stand for, and the device's batches: which match reads from a match of its own batch, and whether
    a block's end finds the batch just written"""

    def __init__(self, r, limit, facts):
        self.r, self.out, self.limit, self.facts = r, bytearray(), limit, facts
        self.batch_n, self.batch_matches, self.prev_match = 0, [], 0

    def room(self):
        return self.limit - len(self.out)

    def _count(self):
        self.facts["tokens"] += 1
        self.batch_n += 1
        if self.batch_n == BATCH:
            self.batch_n, self.batch_matches = 0, []

    def flush(self):
        self.batch_n, self.batch_matches = 0, []

    def literal(self, byte):
        self.out.append(byte)
        self.prev_match = 0
        self._count()
        return (byte,)

    def match(self, ls, lex, ds, dex, check=True):
        length, dist = LEN_BASE[ls] + lex, DIST_BASE[ds] + dex
        pos = len(self.out)
        if check:
            assert 1 <= dist <= pos and length <= self.room() and length <= 258
        src, src_end = pos - dist, pos - dist + min(length, dist)
        if any(src < e and src_end > b for b, e in self.batch_matches):
            self.facts["match_fed_by_match"] += 1
        self.batch_matches.append((pos, pos + length))
        if dist >= length:
            self.out += self.out[src:src + length]
        else:
            self.out += (bytes(self.out[src:]) * (length // dist + 1))[:length]
        f = self.facts
        f["len258_as_285"] += ls == 28
        f["len258_as_284"] += (ls, lex) == (27, 31)
        f["dist_32768"] += dist == 32768
        f["dist_is_output"] += dist == pos
        self.prev_match = length
        self._count()
        return (ls, lex, ds, dex)

    def random_match(self, mode):
        """a match the output so far and the room allow, or None"""
        r, have, room = self.r, len(self.out), self.room()
        if have == 0 or room < 3:
            return None
        ls = r.below(29)
        lex = r.extra(LEN_EXTRA[ls])
        if LEN_BASE[ls] + lex > room:
            ls, lex = len_token(r.between(3, min(room, 258)), alt258=r.chance(0.5))
        length = LEN_BASE[ls] + lex
        if mode == "chain" and self.prev_match:
            dist = r.between(1, min(self.prev_match, have))          # reads what the match before wrote
        elif mode == "one":
            dist = 1
        elif mode == "all":
            dist = have if have <= 32768 else 32768
        elif mode == "far" and have >= 32768:
            dist = 32768
        elif mode == "short":
            dist = r.between(1, min(length, have, 32768))            # shorter than the length (or as long)
        else:
            ok = [s for s in range(30) if DIST_BASE[s] <= have]
            ds = r.pick(ok)
            dist = min(DIST_BASE[ds] + r.extra(DIST_EXTRA[ds]), have)
        ds, dex = dist_token(dist)
        return self.match(ls, lex, ds, dex)


def write_tokens(bw, tokens, lit_lens, dist_lens, facts):
    lit_codes, dist_codes = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if len(t) == 1:
            assert lit_lens[t[0]]
            bw.put(lit_codes[t[0]], lit_lens[t[0]])
            facts["max_token_bits"] = max(facts["max_token_bits"], lit_lens[t[0]])
            continue
        ls, lex, ds, dex = t
        assert lit_lens[257 + ls] and dist_lens[ds]
        bw.put(lit_codes[257 + ls], lit_lens[257 + ls])
        if ls < 29:
            bw.put(lex, LEN_EXTRA[ls])
        bw.put(dist_codes[ds], dist_lens[ds])
        if ds < 30:
            bw.put(dex, DIST_EXTRA[ds])
        bits = lit_lens[257 + ls] + (LEN_EXTRA[ls] if ls < 29 else 0) + dist_lens[ds] + (DIST_EXTRA[ds] if ds < 30 else 0)
        facts["max_token_bits"] = max(facts["max_token_bits"], bits)
        facts["max_dist_bits_used"] = max(facts["max_dist_bits_used"], dist_lens[ds])
    bw.put(lit_codes[256], lit_lens[256])


def assign(r, n_total, symbols, lens, pinned):
    """lens to the symbols at random, the pinned symbols taking the longest"""
    out = [0] * n_total
    order = sorted(pinned) + r.shuffled(sorted(set(symbols) - set(pinned)))
    for s, n in zip(order, sorted(lens, reverse=True)[:len(pinned)] + r.shuffled(sorted(lens, reverse=True)[len(pinned):])):
        out[s] = n
    return out


def run_length_code(r, seq, hlit, cross_ok, plain, facts, first_16=False, past_total=False):
    """the lengths of both alphabets as (code-length symbol, extra value, extra bits): plain lengths or 16 / 17 / 18 at random,
    with partial repeat counts; a repeat may run from the literal lengths into the distance lengths where cross_ok"""
    ops, i, n = [], 0, len(seq)
    if first_16:
        ops.append((16, 0, 2))  # (nothing to repeat: the rule broken)
        i = 3
    if past_total:
        n -= 1
    while i < n:
        v, run = seq[i], 1
        stop = n if cross_ok or i >= hlit else hlit
        while i + run < stop and seq[i + run] == v:
            run += 1
        k = 0
        if run >= 3 and not r.chance(plain):
            if i > 0 and seq[i - 1] == v and (v != 0 or r.chance(0.35)):
                k = r.between(3, min(run, 6))
                ops.append((16, k - 3, 2))
                facts["rep16_on_zero"] += v == 0
            elif v == 0 and run >= 11 and r.chance(0.7):
                k = min(run, 138) if r.chance(0.5) else r.between(11, min(run, 138))
                ops.append((18, k - 11, 7))
            elif v == 0:
                k = r.between(3, min(run, 10))
                ops.append((17, k - 3, 3))
        if k:
            facts["repeat_across"] += i < hlit < i + k
            i += k
        else:
            ops.append((v, 0, 0))
            i += 1
    if past_total:
        ops.append((18, 0, 7))  # (eleven zeros where one length is left: the rule broken)
    return ops


def dynamic_block(r, bw, tokens, last, knobs, facts, rule=None):
    """one dynamic block of the tokens, with codes and a header as the knobs say; `rule`: the one rule to break"""
    deep = knobs.get("deep", 0.0)
    used_lit = {t[0] if len(t) == 1 else 257 + t[0] for t in tokens} | {256}
    used_dist = {t[2] for t in tokens if len(t) == 4}
    pin_lit, pin_dist = set(), set()
    if knobs.get("pin48"):
        for t in [t for t in tokens if t == (27, 31, 29, 8191)] + tokens:
            if len(t) == 4 and LEN_EXTRA[t[0]] == 5 and DIST_EXTRA[t[2]] == 13:
                pin_lit, pin_dist, deep = {257 + t[0]}, {t[2]}, 1.0
                break
    if knobs.get("pin_dist") and used_dist:
        pin_dist = pin_dist or {r.pick(sorted(used_dist))}
    # the symbols of the codes: those used and a random set of others
    spare_lit = r.shuffled(sorted(set(range(286)) - used_lit))
    spare_dist = r.shuffled(sorted(set(range(30)) - used_dist))
    n_lit = len(used_lit) + (0 if r.chance(0.2) else r.below(min(40, len(spare_lit)) + 1) if r.chance(0.7) else r.below(len(spare_lit) + 1))
    n_dist = len(used_dist) + (0 if r.chance(0.3) else r.below(len(spare_dist) + 1))
    if len(used_dist) == 1 and r.chance(0.5):
        n_dist = 1  # the one-symbol code of length 1
    elif deep >= 0.9 or rule:
        n_lit, n_dist = max(n_lit, 18), max(n_dist, 17 if used_dist or pin_dist or rule or r.chance(0.5) else 0)
    if rule:  # (symbols nobody uses, for the rules that take one away)
        n_lit, n_dist = max(n_lit, len(used_lit) + 2), max(n_dist, len(used_dist) + 2)
    n_lit, n_dist = min(n_lit, 286), min(n_dist, 30)
    if n_lit == 1 and not knobs.get("eob_only", True):
        n_lit = 2
    lit_syms = sorted(used_lit) + spare_lit[:n_lit - len(used_lit)]
    dist_syms = sorted(used_dist) + spare_dist[:n_dist - len(used_dist)]
    lit_lens = assign(r, 288, lit_syms, [1] if n_lit == 1 else split_code(r, n_lit, 15, deep), pin_lit)
    dist_lens = assign(r, 32, dist_syms, [] if n_dist == 0 else [1] if n_dist == 1 else split_code(r, n_dist, 15, knobs.get("deep_dist", deep)), pin_dist)
    if knobs.get("counts"):  # the numbers of codes per length given: every symbol of both alphabets has a code
        (lit_counts, dist_counts), n_lit, n_dist = knobs["counts"], 286, 30
        lit_lens = assign(r, 288, range(286), [n for n, c in lit_counts.items() for _ in range(c)], set())
        dist_lens = assign(r, 32, range(30), [n for n, c in dist_counts.items() for _ in range(c)], set())
    facts["eob_only_code"] += n_lit == 1
    facts["single_dist_code"] += n_dist == 1 and bool(used_dist)
    facts["no_dist_code"] += n_dist == 0
    hlit = 286 if knobs.get("hlit_286") else max(257, max(s for s in range(286) if lit_lens[s]) + 1)
    hdist = 30 if knobs.get("hdist_30") else max([1] + [s + 1 for s in range(30) if dist_lens[s]])
    written_lit, written_dist = list(lit_lens), list(dist_lens)  # (what the header says; the tokens use the sound code)
    if rule in ("oversubscribed_litlen", "oversubscribed_dist"):
        w = written_lit if rule.endswith("litlen") else written_dist
        s = r.pick([s for s in range(len(w)) if w[s] > 1])
        w[s] -= 1
    if rule in ("incomplete_litlen", "incomplete_dist"):
        w, used = (written_lit, used_lit) if rule.endswith("litlen") else (written_dist, used_dist)
        w[r.pick([s for s in range(len(w)) if w[s] and s not in used])] = 0
    if rule == "no_end_of_block":  # the code stays complete: the length goes to a literal nobody uses
        s = r.pick([s for s in range(256) if not written_lit[s]])
        written_lit[s], written_lit[256] = written_lit[256], 0
        hlit = max(hlit, 257)
    hlit_field, hdist_field = hlit - 257, hdist - 1
    if rule in ("hlit_287", "hlit_288"):
        hlit = int(rule[-3:])
        hlit_field = hlit - 257
    if rule in ("hdist_31", "hdist_32"):
        hdist = int(rule[-2:])
        hdist_field = hdist - 1
    seq = written_lit[:hlit] + written_dist[:hdist]
    ops = run_length_code(r, seq, hlit, knobs.get("cross", True), knobs.get("plain", 0.3), facts, rule == "first_length_is_16", rule == "repeat_past_total")
    # the code-length code
    used_cl = {o[0] for o in ops}
    spare_cl = r.shuffled(sorted(set(range(19)) - used_cl))
    n_cl = len(used_cl) + r.below(len(spare_cl) + 1)
    if knobs.get("deep_cl", 0) >= 0.9:
        n_cl = max(n_cl, 9)
    n_cl = min(19, max(n_cl, len(used_cl) + 1 if rule else 2, 3 if rule else 2))
    cl_syms = sorted(used_cl) + spare_cl[:n_cl - len(used_cl)]
    cl_lens = assign(r, 19, cl_syms, split_code(r, n_cl, 7, knobs.get("deep_cl", deep)), set())
    written_cl = list(cl_lens)
    if rule == "oversubscribed_cl":
        written_cl[r.pick([s for s in range(19) if written_cl[s] > 1])] -= 1
    if rule == "one_symbol_cl":  # (one code of length 1: what the other two alphabets may be, and this one may not)
        written_cl = [int(s == min(used_cl)) for s in range(19)]
    if rule == "incomplete_cl":
        written_cl[r.pick([s for s in range(19) if written_cl[s] and s not in used_cl])] = 0
    hclen = max(4, max(i + 1 for i in range(19) if written_cl[CL_ORDER[i]]))
    if not rule:
        f = facts
        f["max_lit_bits"], f["max_dist_bits"], f["max_cl_bits"] = max(f["max_lit_bits"], max(lit_lens)), max(f["max_dist_bits"], max(dist_lens)), max(f["max_cl_bits"], max(cl_lens))
        f["hlit_286"] += hlit == 286
        f["hdist_30"] += hdist == 30
    bw.put(int(last), 1)
    bw.put(2, 2)
    bw.put(hlit_field, 5)
    bw.put(hdist_field, 5)
    bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(written_cl[CL_ORDER[i]], 3)
    cl_codes = canonical(cl_lens)
    for sym, extra, bits in ops:
        bw.put(cl_codes[sym], cl_lens[sym])
        bw.put(extra, bits)
    write_tokens(bw, tokens, lit_lens, dist_lens, facts)


def fixed_block(bw, tokens, last, facts):
    bw.put(int(last), 1)
    bw.put(1, 2)
    write_tokens(bw, tokens, FIXED_LIT, FIXED_DIST, facts)


def stored_block(bw, data, last, facts):
    facts["stored_offsets"].append(bw.total % 8)
    bw.put(int(last), 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xFFFF, 16)
    bw.raw(data)


def tokens_of_block(r, o, count, knobs, fill=False):
    """`count` tokens (fewer when the room runs out; as many as fill the room when `fill`)"""
    tokens = []
    p_match, modes = knobs.get("p_match", 0.5), knobs.get("modes", ("sym", "sym", "one", "all", "far", "short", "chain"))
    alphabet = knobs.get("alphabet", 256)
    while (fill or len(tokens) < count) and o.room() > 0:
        t = o.random_match(r.pick(modes)) if r.chance(p_match) else None
        tokens.append(t if t is not None else o.literal(r.below(alphabet)))
    return tokens


def member(seed, theme=None):
    """the valid member of the seed: (expected bytes, stream, facts)"""
    r = Rand(seed)
    theme = THEMES[seed % len(THEMES)] if theme is None else theme
    facts = new_facts()
    facts["theme"] = theme
    limit = MAX_OUT if theme == "full" else MAX_OUT - 258 if theme == "deep48" else r.pick([0, 1]) if theme == "tiny" else r.pick([r.between(2, 300), r.between(300, 20000), r.between(20000, MAX_OUT)])
    o, bw = Output(r, limit, facts), BitWriter()
    n_blocks = r.between(3, 8) if theme == "stored" else r.between(1, 8)
    for b in range(n_blocks):
        last = b == n_blocks - 1
        fill = last and theme in ("full", "deep48")
        kind = r.pick(("dynamic", "dynamic", "dynamic", "fixed", "stored"))
        if theme == "stored":  # Huffman blocks of any length with a stored block behind each: its header at any bit
            kind = "stored" if b % 2 == 1 else r.pick(("dynamic", "fixed"))
        if fill and kind == "stored":
            kind = "dynamic"
        if kind == "stored":
            n = min(r.pick([0, 0, 1, r.between(2, 700)]), o.room())
            if theme == "stored" and b == 1:
                n = 0  # an empty stored block between two Huffman blocks (when the member has a third)
            data = bytes(r.below(256) for _ in range(n))
            stored_block(bw, data, last, facts)
            o.out += data
            o.flush()
            facts["blocks"].append(("stored", n))
            continue
        to_batch = BATCH - o.batch_n
        count = r.pick([0, 1, 63, 64, 65, 128, to_batch, to_batch + BATCH, r.between(2, 400), r.between(2, 3000)])
        if theme == "counts":
            count = r.pick([0, 1, 63, 64, 65, 128, to_batch, to_batch])
        knobs = dict(p_match=r.pick([0.0, 0.1, 0.5, 0.9]), alphabet=r.pick([1, 4, 30, 256]), deep=r.pick([0.0, 0.3, 0.7, 1.0]), deep_cl=r.pick([0.0, 0.5, 1.0]),
                     deep_dist=r.pick([0.0, 0.5, 1.0]), plain=r.pick([0.0, 0.3, 0.8]), cross=r.chance(0.8), hlit_286=r.chance(0.25), hdist_30=r.chance(0.25),
                     pin_dist=r.chance(0.3))
        if theme in ("full", "deep48"):
            knobs["p_match"] = r.pick([0.5, 0.9])
            count = r.between(100, 2000)
        if theme == "deep48":
            knobs.update(pin48=True, deep=1.0, deep_dist=1.0, deep_cl=1.0, modes=("far", "all", "sym", "short"))
        if theme == "chains":
            knobs.update(p_match=0.95, modes=("chain", "chain", "chain", "short", "one"))
        if theme == "wide_header":
            knobs.update(hlit_286=True, hdist_30=True, cross=True, plain=r.pick([0.0, 0.2]), alphabet=r.pick([4, 30]))
        before = facts["tokens"]
        if theme == "deep48" and fill:
            # length 258 as 284 + 31 at distance 32 768, each under a 15-bit code: the 48 bits a token has at most
            tokens = tokens_of_block(r, o, count, knobs, fill)
            o.limit = MAX_OUT
            tokens.append(o.match(27, 31, 29, 8191))
        else:
            tokens = tokens_of_block(r, o, count, knobs, fill)
        if kind == "fixed":
            fixed_block(bw, tokens, last, facts)
        else:
            dynamic_block(r, bw, tokens, last, knobs, facts)
        if facts["tokens"] > before and o.batch_n == 0:
            facts["block_end_on_batch"] += 1
        facts["blocks"].append((kind, len(tokens)))
    facts["out_len"] = len(o.out)
    return bytes(o.out), bw.bytes(), facts


# The complete codes whose second-level tables are the largest a decoder with an 11-bit (literal / length) and an 8-bit (distance)
# first level and zlib's way of sizing the second levels can meet -- 292 and 144 entries; found by a walk over the numbers of codes
# per length in the manner of zlib's enough.c --, as {length: codes}
LARGEST_TABLES = ({1: 1, 2: 1, 3: 1, 5: 2, 12: 233, 13: 45, 14: 1, 15: 2}, {1: 1, 2: 1, 3: 1, 4: 1, 6: 2, 9: 13, 10: 5, 11: 1, 12: 1, 13: 1, 14: 1, 15: 2})


def largest_tables_member(seed):
    """a valid member of two dynamic blocks with the codes of LARGEST_TABLES: (expected bytes, stream, facts)"""
    r = Rand("largest tables", seed)
    facts = new_facts()
    facts["theme"] = "largest_tables"
    o, bw = Output(r, 30000, facts), BitWriter()
    for last in (False, True):
        knobs = dict(p_match=0.6, counts=LARGEST_TABLES, plain=r.pick([0.0, 0.5]))
        tokens = tokens_of_block(r, o, r.between(300, 1500), knobs)
        dynamic_block(r, bw, tokens, last, knobs, facts)
        facts["blocks"].append(("dynamic", len(tokens)))
    facts["out_len"] = len(o.out)
    return bytes(o.out), bw.bytes(), facts


def invalid_members(seed):
    """one member per broken rule: [(kind, stream, out_len, the status it must get or None = bad stream / short / long, reason)]"""
    out = []
    for k, kind in enumerate(INVALID_KINDS):
        r = Rand(seed, kind)
        facts = new_facts()
        o, bw = Output(r, 4000, facts), BitWriter()
        knobs = dict(p_match=0.5, alphabet=30, deep=r.pick([0.0, 0.5, 1.0]), plain=0.3, eob_only=False)
        if kind == "incomplete_cl":
            knobs["deep"] = 0.0  # (a flat code: few lengths, so the code-length code has a symbol to spare)
        # a sound block in front, of any kind and length: the broken block's header begins at any bit
        lead = tokens_of_block(r, o, r.between(1, 80), knobs)
        if r.chance(0.5):
            fixed_block(bw, lead, False, facts)
        else:
            dynamic_block(r, bw, lead, False, knobs, facts)
        status, reason = BAD_STREAM, kind.replace("_", " ")
        if kind.startswith("fixed_"):
            tokens = tokens_of_block(r, o, r.between(0, 20), knobs)
            bad = int(kind[-3:]) - 257 if "litlen" in kind else int(kind[-2:])
            # (the symbol stands where a token may: the codes 286 / 287 and 30 / 31 of the fixed block exist and mean nothing)
            tokens.append((bad, 0, 0, 0) if "litlen" in kind else (r.below(8), 0, bad, 0))
            fixed_block(bw, tokens, True, facts)
            reason = "a fixed block uses %s symbol %s" % ("literal / length" if "litlen" in kind else "distance", kind[-3:] if "litlen" in kind else kind[-2:])
        elif kind == "distance_before_output":
            tokens = tokens_of_block(r, o, r.between(0, 20), knobs)
            ds, dex = dist_token(len(o.out) + 1)
            tokens.append(o.match(0, 0, ds, dex, check=False))
            dynamic_block(r, bw, tokens, True, knobs, facts)
            reason = "a match reaches one byte in front of the output"
        elif kind in ("ends_inside_code", "out_len_one_over", "out_len_one_under"):
            tokens = tokens_of_block(r, o, r.between(30, 200), dict(knobs, alphabet=256, deep=0.0))
            dynamic_block(r, bw, tokens, True, dict(knobs, deep=0.0), facts)
        else:
            tokens = tokens_of_block(r, o, r.between(1, 80), knobs)
            dynamic_block(r, bw, tokens, True, knobs, facts, rule=kind)
        stream, out_len = bw.bytes(), len(o.out)
        if kind == "distance_before_output":
            out_len = 4000  # (room for whatever a decoder that took the match would write)
        if kind == "ends_inside_code":
            stream, status, reason = stream[:-r.between(2, 6)], None, "the stream ends inside the last block's codes"
        if kind == "out_len_one_over":
            out_len, status, reason = out_len + 1, SHORT, "the stream holds one byte less than out_len"
        if kind == "out_len_one_under":
            out_len, status, reason = out_len - 1, LONG, "the stream holds one byte more than out_len"
        out.append((kind, stream, out_len, status, reason))
    return out
