"""Hand-made graphs for the tables of the position-hinted pass (gtx_ctx_hint_table 0..6): every set is a reference string and variant
records, a few hundred to a few thousand bases, with the sequences planted that a random reference does not produce -- repeated 32-mers,
16-mers shared by 16 / 17 / 64 / 65 keys, halves at a chosen distance, merged sites whose alleles spell one k-mer, windows at the region's
ends, reference nodes of 254 / 255 / 256 bases.  The restatement (tests/hint_tables_ref.py) over the oracle's index says what the tables
have to be; FACTS[name] shows, from the restatement alone, that the set holds the shape it is for.

What no graph of the constructor reaches, and is therefore in no set:
  * an alternative allele with an N: the constructor drops it (an IUPAC letter it keeps: `plain`; N, other IUPAC letters and a character that
    is no letter at all arrive through the reference string, also as a site's reference allele: `letters`);
  * a site index of HINT_NO_SITE or more: 65 535 sites are no small graph (the limit is stated in the restatement all the same);
  * GTX_HINT_WINDOWS' cap of 16 384 windows, for the same reason.
"""
import functools

import numpy as np

import hint_tables_ref as H
from graphtyper_amd import lib as gtx
from oracle_lib import Oracle

REGION_BEGIN = 1000
K = 32


def rnd(n, seed):
    rs = np.random.RandomState(seed)
    return "".join("ACGT"[i] for i in rs.randint(0, 4, n))


def other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def subst(s, *at):
    s = list(s)
    for i in at:
        s[i] = other(s[i])
    return "".join(s)


class Ref:
    """a reference string under construction: plant() overwrites, snp() / record() add variant records (0-based offsets in the string)"""

    def __init__(self, n, seed):
        self.s, self.recs = list(rnd(n, seed)), []

    def plant(self, at, text):
        assert 0 <= at and at + len(text) <= len(self.s)
        self.s[at:at + len(text)] = text
        return at

    def text(self, at, n):
        return "".join(self.s[at:at + n])

    def snp(self, at, n_alt=1, alts=None):
        c = self.s[at]
        self.recs.append((REGION_BEGIN + at, c, alts or [other(c, k) for k in range(1, n_alt + 1)], "."))

    def record(self, at, n_ref, alts, info="."):
        self.recs.append((REGION_BEGIN + at, self.text(at, n_ref), list(alts), info))

    def done(self, **kw):
        return dict(ref="".join(self.s), recs=sorted(self.recs), **kw)


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
def _plain():
    r = Ref(1500, 11)
    r.snp(100, 1)
    r.snp(200, 2)
    r.snp(300, 3)
    r.snp(500, alts=[other(r.s[500]), other(r.s[500], 2), other(r.s[500], 3), other(r.s[500])])  # five alleles (one twice), each one base
    # a SNP whose alternative k-mers also occur elsewhere: the 63 bases around it, with the other allele, planted again
    r.snp(700, 1)
    r.plant(900, subst(r.text(669, 63), 31))
    # SNPs whose allele keys are not alone with their halves (no HINT_SNP_GROUP): the 16 bases behind the k-mer's half with the SNP occur once
    # more; the first 16 bases of the k-mer WITH THE OTHER ALLELE occur once more
    r.snp(1100, 1)
    r.plant(1200, r.text(1111, 16))
    r.snp(1300, 1)
    r.plant(1400, subst(r.text(1295, 16), 5))
    # an alternative allele that is an IUPAC letter (the constructor keeps it), and one of two bases whose first is not the reference's
    r.snp(600, alts=["Y" if r.s[600] != "C" else "R"])
    r.record(800, 1, [other(r.s[800]) + "T"])
    # ... and a T beside the IUPAC letter: the letter has no key of its own, and the T's key is labelled with the T's allele number
    r.plant(1450, "A")
    r.snp(1450, alts=["T", "Y"])
    return r.done()


def _repeats():
    r = Ref(1600, 12)
    r.plant(600, r.text(100, 40))              # a 40-mer twice: nine 32-mers with two labels each
    r.plant(800, subst(r.text(300, 32), 5))    # a copy with one substitution: a neighbour on another interval
    r.plant(1000, subst(r.text(400, 32), 5, 25))  # a copy with one substitution in each half: no neighbour, no shared half
    return r.done()


FAR_DISTANCES = (1, 2, 3, 4, 7, 8)


def _far():
    r = Ref(2400, 13)
    for side in range(2):
        for i, d in enumerate(FAR_DISTANCES):
            a = 100 + 60 * (len(FAR_DISTANCES) * side + i)
            k = r.text(a, K)
            at = [16 + 2 * j for j in range(d)] if side == 0 else [2 * j for j in range(d)]  # the OTHER half differs in d bases
            r.plant(a + 1000, subst(k, *at))
    return r.done()


CROWDS = (16, 17, 64, 65)


def crowd_at(n):
    return 100 + sum(40 * m for m in CROWDS[:CROWDS.index(n)])


def _crowded():
    r = Ref(100 + 40 * sum(CROWDS) + 300, 14)
    for ci, n in enumerate(CROWDS):
        half = rnd(16, 140 + ci)
        for j in range(n):  # n keys with that first half (the 32-mers in between are random)
            r.plant(crowd_at(n) + 40 * j, half)
    return r.done()


def _crowded_nb():
    """neighbour labels adding up to 16 and to 17 (HINT_NB_MAX): one record whose 16 / 17 alternative alleles are the reference allele's six bases
    with one substitution each -- every k-mer over all six has that many neighbours, each with the k-mer's own interval on its own site; a k-mer
    with three of the six in either half keeps both half groups below HINT_HE_CAP"""
    r = Ref(1200, 15)
    for at, n_alt, twice in ((200, 16, 0), (450, 17, 0), (700, 15, 1), (950, 15, 2)):
        ref6 = r.text(at, 6)
        alts = [ref6[:j] + other(ref6[j], k) + ref6[j + 1:] for j in range(6) for k in (1, 2, 3)][:n_alt]
        r.record(at, 6, alts + alts[:1] * twice)  # (an allele listed two / three times: ONE neighbour key with that many labels)
    return r.done()


def _multi():
    r = Ref(1200, 16)
    # two overlapping records, merged (add_all_variants): 2 x 2, 4 x 2, 3 x 3 and 5 x 2 alleles of two bases; the k-mer that starts on the
    # second base is spelled by 2, 4, 3 and 5 of them
    for at, n1, n2, dup in ((100, 1, 1, False), (300, 3, 1, False), (500, 2, 2, False), (700, 3, 1, True)):
        c = r.s[at]
        r.recs.append((REGION_BEGIN + at, c, [other(c, k) for k in range(1, n1 + 1)] + ([other(c)] if dup else []), "."))
        r.snp(at + 1, n2)
    # one record of six alleles of three bases, five of which end alike (one of them listed twice): five labels with allele numbers below 8
    # for the k-mer that starts on the second base, and no neighbour (the sixth allele differs in two bases)
    c, d = r.s[900], r.text(901, 2)
    r.record(900, 3, [other(c, 1) + d, other(c, 2) + d, other(c, 3) + d, other(c, 1) + d, c + subst(d, 0, 1)])
    return r.done(add_all_variants=True)


def _two():
    r = Ref(2000, 17)
    # two neighbouring sites (records that touch but do not overlap stay two sites): 2 + 2 alleles, 4 + 4 (allele numbers up to 3), and 5 + 2
    # (an allele number 4)
    r.snp(100, 1)
    r.snp(101, 1)
    r.snp(300, 3)
    r.snp(301, 3)
    r.snp(500, alts=[other(r.s[500]), other(r.s[500], 2), other(r.s[500], 3), other(r.s[500])])
    r.snp(501, 1)
    # ... and a pair with a copy of the 62 bases around it that has one substitution behind the pair: the k-mers over the pair and that place
    # have a neighbour with a label on a foreign interval
    r.snp(800, 1)
    r.snp(801, 1)
    r.plant(1100, subst(r.text(770, 62), 40))  # (offset 810)
    # a SNP, an insertion of one base behind the next base, a SNP: the k-mer over the first two that ends behind the insertion's place has a
    # neighbour with ITS start and another end (the path that ends on the inserted base); the k-mer over the last two that starts on the
    # insertion's place has one with its end and another start
    r.snp(1429, 1)
    t = [c for c in "ACGT" if c not in (r.s[1430], r.s[1431])][0]
    r.record(1430, 1, [r.s[1430] + t])
    r.snp(1440, 1)
    # three SNPs in a row: three labels on three sites
    for at in (1700, 1701, 1702):
        r.snp(at, 1)
    return r.done()


def _letters():
    r = Ref(900, 18)
    r.plant(200, "N")
    r.plant(400, "R")
    r.plant(600, "Y")
    r.snp(600, alts=["C"])  # an IUPAC letter as a site's reference allele
    r.snp(700, 1)
    r.plant(800, "x")  # no IUPAC letter: equal to no read base
    return r.done()


def _nodes():
    r = Ref(40 + 254 + 1 + 255 + 1 + 256 + 1 + 300 + 3 + 50, 19)
    at = 40
    r.snp(at, 1)  # (the first node: 40 bases)
    for ln in (254, 255, 256, 300):
        at += 1 + ln
        if ln == 300:
            r.record(at, 3, [r.text(at, 1)])  # a deletion behind the node of 300
        else:
            r.snp(at, 1)
    return r.done()


def _windows():
    r = Ref(2600, 20)
    r.record(60, 1, [r.text(60, 1) + rnd(1, 201)])       # an insertion, less than 160 behind the region's start
    for at, n in ((400, 63), (600, 64), (800, 65)):      # alleles of 63, 64 and 65 bases (the base in front of the insertion is the allele's first)
        r.record(at, 1, [r.text(at, 1) + rnd(n - 1, 200 + n)])
    r.record(1000, 5, [r.text(1000, 1)])                 # a deletion: an allele of one base against five
    r.snp(1200, 1)
    r.snp(1231, 1)                                       # 30 bases between two SNPs: windows
    r.snp(1400, 1)
    r.snp(1432, 1)                                       # 31: none
    # 8 and 9 alleles: one base against one, two or three others
    for at, n in ((1600, 7), (1800, 8)):
        c = r.s[at]
        r.recs.append((REGION_BEGIN + at, c, [other(c, 1 + k % 3) + "ACGT"[k // 3] * (k // 3) for k in range(n)], "."))
    r.record(2200, 64, [r.text(2200, 1)])                # reference alleles of 64 and of 65 bases
    r.record(2350, 65, [r.text(2350, 1)])
    r.record(2540, 1, [r.text(2540, 1) + rnd(2, 202)])   # less than 160 in front of the region's end
    return r.done()


def _pruned():
    """the index sweep refuses a walk that takes two bases of a node whose event is among its own anti events (walk_is_kept): the 31
    reference 32-mers that hold both bases of this reference allele are in no key -- and one of them is planted again further on: a key whose
    one label lies elsewhere"""
    r = Ref(1500, 22)
    r.record(300, 2, [subst(r.text(300, 2), 0, 1)], "RE=5;RA=5")
    r.plant(500, r.text(285, K))
    # ... and the same behind a SNP, planted again under two SNPs: the keys of the 32-mers over both sites have their two labels elsewhere
    r.snp(900, 1)
    r.record(910, 2, [subst(r.text(910, 2), 0, 1)], "RE=6;RA=6")
    r.plant(1180, r.text(880, 65))
    r.snp(1200, 1)
    r.snp(1210, 1)
    return r.done()


def _sv():
    r = Ref(700, 21)
    r.snp(100, 1)
    r.record(300, 1, [r.text(300, 1) + rnd(5, 210)])
    r.snp(500, 2)
    return r.done(is_sv_graph=True)


SIZE_LENGTHS = (64 * 5 - 1, 64 * 5, 64 * 5 + 1, 256 * 2 - 1, 256 * 2 + 1)


def _size(n, windows):
    def make():
        r = Ref(n, 300 + n)
        r.snp(100, 1)
        if windows:
            r.record(200, 1, [r.text(200, 1) + rnd(3, 310)])
        return r.done()
    return make


SETS = dict(plain=_plain, repeats=_repeats, far=_far, crowded=_crowded, crowded_nb=_crowded_nb, multi=_multi, two=_two, letters=_letters, nodes=_nodes,
            windows=_windows, pruned=_pruned, sv=_sv)
for _n in SIZE_LENGTHS:
    SETS["size%d" % _n] = _size(_n, False)
    SETS["size%dw" % _n] = _size(_n, True)
NAMES = list(SETS)


class Built:
    def __init__(self, name):
        c = SETS[name]()
        self.name, self.ref, self.recs = name, c["ref"], c["recs"]
        self.aav, self.sv = bool(c.get("add_all_variants")), bool(c.get("is_sv_graph"))
        self.graph = gtx.graph_from_records(self.ref, self.recs, region_begin=REGION_BEGIN, add_all_variants=self.aav, is_sv_graph=self.sv)
        self.oracle = Oracle(self.ref, self.recs, region_begin=REGION_BEGIN, add_all_variants=self.aav, is_sv_graph=self.sv)
        og = self.oracle.graph()
        assert np.array_equal(og["dna"], self.graph["dna"])  # (the node offsets of the library's dict point into the oracle's characters)
        self.r = H.HintTablesRef(self.oracle.index_dump(), og, self.graph, is_sv_graph=self.sv)
        assert self.r.first == REGION_BEGIN + 1 and self.r.n == len(self.ref)  # table position p = offset p of the reference string
        self.want = self.r.tables()

    def context(self, device):
        return gtx.Context(self.graph, device=device, is_sv_graph=self.sv)

    # ---- reading the expected tables
    def x(self, p):
        return int(self.want[0][2 * p])

    def y(self, p):
        return int(self.want[0][2 * p + 1])

    def tail(self, p):
        return int(self.want[2][2 * p]), int(self.want[2][2 * p + 1])

    def plane_code(self, p):
        return sum(((int(self.want[1][4 * (p >> 5) + b]) >> (p & 31)) & 1) << b for b in range(4))

    def key_at(self, p):
        """number of the key that is the reference 32-mer at p (-1: not indexed)"""
        s = self.ref[p:p + K]
        if len(s) < K or any(c not in "ACGT" for c in s):
            return -1
        v = 0
        for c in s:
            v = (v << 2) | "ACGT".index(c)
        return self.r.find(v)

    def alleles(self, site):
        g = self.r.g
        fv = int(g["ref_first_var"][site])
        return [bytes(self.r.dna[int(g["var_dna"][fv + a]):int(g["var_dna"][fv + a] + g["var_len"][fv + a])]).decode() for a in range(int(g["ref_nvar"][site]))]

    def far(self, p):
        return (self.y(p) >> H.FAR_LEFT_SHIFT) & 3, (self.y(p) >> H.FAR_RIGHT_SHIFT) & 3

    def window(self, site_at, allele=1):
        """(window number, first table position) of the window of the site whose variant nodes start at reference offset site_at"""
        for w, (site, a, len_a, len_0, so) in enumerate(self.r.win):
            if so == REGION_BEGIN + 1 + site_at and a == allele:
                return w, self.r.win_base + w * H.WIN_STRIDE
        return None


@functools.lru_cache(maxsize=None)
def built(name):
    return Built(name)


def compare(name, tables):
    """None, or how `tables` (seven arrays of words) differ from the restatement for set `name`: table, position and field"""
    return H.compare(tables, built(name).want)


# ---- the facts -----------------------------------------------------------------------------------------------------------------------
def flag_names(x):
    return {nm for nm, lo, ln in H.X_FIELDS[:8] if (x >> lo) & 1}


def _facts_plain(b):
    ref = b.ref
    assert flag_names(b.x(20)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"} and b.x(20) >> 16 == H.NO_SITE and b.far(20) == (3, 3)
    assert b.y(20) & 0xFFFF == 80 | (20 << 8) and b.y(20) & H.NEAR_FREE
    for site, (at, nv) in enumerate(((100, 2), (200, 3), (300, 4))):
        for off in (0, 15, 16, 31):
            p = at - off
            want = {"SINGLE_OK", "EXACT_OK", "PAR", "ALT_OK"} | ({"L1"} if off < 16 else {"R1"})
            assert flag_names(b.x(p)) == want, (at, off, flag_names(b.x(p)))
            assert b.x(p) >> 16 == site
            idx = {"ACGT".index(s): a for a, s in enumerate(b.alleles(site)) if a}
            assert (b.x(p) >> 8) & 0xFF == sum(a << (2 * base) for base, a in idx.items())
            y = b.y(p)
            assert (y >> 16) & 31 == off and y & H.SNP_GROUP and (y >> 22) & 3 == "ACGT".index(ref[at]) and (y >> 24) & 7 == nv
            assert not y & H.NEAR_FREE  # (the other alleles' halves are in the filters)
        assert flag_names(b.x(at - 32)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"} and flag_names(b.x(at + 1)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"}
        t = b.tail(at - 1)
        assert t[1] == site and t[0] & 3 == 3 and (t[0] >> 2) & 7 == nv and (t[0] >> 8) & 0xFF == int(b.r.g["ref_len"][site + 1])
        assert [(t[0] >> (16 + 4 * a)) & 15 for a in range(4)] == [1 << "ACGT".index(s) for s in b.alleles(site)] + [0] * (4 - nv)
        assert b.tail(at) == (0, 0)  # (on the site itself: no reference node)
    # HINT_SNP_GROUP at k-mer offset 5 of the SNPs at 1100 and 1300, and one place further on where the planted 16 bases are no half of the k-mer
    k = b.key_at(1095)
    assert b.r.gsize[1][k] == 3 and b.key_at(1200 - 16) in b.r.group[1][k] and b.r.gsize[0][k] == 1
    assert "ALT_OK" in flag_names(b.x(1095)) and not b.y(1095) & H.SNP_GROUP and b.y(1096) & H.SNP_GROUP and "ALT_OK" in flag_names(b.x(1096))
    k = b.key_at(1295)
    ka = [n for n in b.r.neighbours(k)]
    assert len(ka) == 1 and b.r.gsize[0][k] == 1 and b.r.gsize[1][k] == 2 and b.r.group[0][ka[0]] == sorted([ka[0], b.key_at(1400)])
    assert "ALT_OK" in flag_names(b.x(1295)) and not b.y(1295) & H.SNP_GROUP and b.y(1296) & H.SNP_GROUP and "ALT_OK" in flag_names(b.x(1296))
    # an IUPAC letter as the other allele, an allele of two bases: no HINT_ALT_OK at any offset (the k-mer that ENDS on the two-base allele's
    # first base is indexed on this very interval), no HINT_TAIL_OK
    site = int(b.r.tail[1449][1])
    assert sorted(b.alleles(site)) == ["A", "T", "Y"] and b.tail(1449) == (H.TAIL_NODE, site)
    for off in (0, 15, 16, 31):
        assert flag_names(b.x(1450 - off)) & {"SINGLE_OK", "ALT_OK"} == {"SINGLE_OK"}, off
    for at in (600, 800):
        site = int(b.r.tail[at - 1][1])
        assert len(b.alleles(site)) == 2 and (b.alleles(site)[1] in "YR" if at == 600 else len(b.alleles(site)[1]) == 2)
        assert b.tail(at - 1) == (H.TAIL_NODE, site)
        for off in (0, 15, 16, 31) if at == 600 else (15, 16, 31):  # (the k-mer that starts on the two-base allele's site: two intervals)
            assert flag_names(b.x(at - off)) & {"SINGLE_OK", "ALT_OK"} == {"SINGLE_OK"}, (at, off)
    s = b.ref[769:800] + b.alleles(int(b.r.tail[799][1]))[1][0]
    k = b.r.find(sum("ACGT".index(c) << (2 * (31 - j)) for j, c in enumerate(s)))
    assert k >= 0 and b.r.labels_of(k)[0][:2] == (REGION_BEGIN + 770, REGION_BEGIN + 801)
    # five alleles: no HINT_ALT_OK over it, no HINT_TAIL_OK in front of it
    assert int(b.r.g["ref_nvar"][3]) == 5 and b.alleles(3)[1] == b.alleles(3)[2]
    for off in (0, 15, 16, 31):
        assert "ALT_OK" not in flag_names(b.x(500 - off)) and "SINGLE_OK" in flag_names(b.x(500 - off))
    assert b.tail(499) == (H.TAIL_NODE, 3)
    # the SNP whose other allele's k-mers occur elsewhere as well: two labels there, no HINT_ALT_OK
    for off in (0, 15, 16, 31):
        k = b.key_at(900 + 31 - off)
        assert k >= 0 and len(b.r.labels_of(k)) == 2
        assert flag_names(b.x(700 - off)) & {"SINGLE_OK", "ALT_OK"} == {"SINGLE_OK"}


def _facts_repeats(b):
    for d in range(9):
        k = b.key_at(100 + d)
        assert k == b.key_at(600 + d) and len({l[:2] for l in b.r.labels_of(k)}) == 2
        assert b.x(100 + d) == b.x(600 + d) == H.NO_SITE << 16  # nothing set
    k, k2 = b.key_at(300), b.key_at(800)
    assert b.r.neighbours(k) == [k2] and b.r.labels_of(k2)[0][:2] != b.r.labels_of(k)[0][:2]
    assert flag_names(b.x(300)) == {"SINGLE_OK", "L1"} and flag_names(b.x(800)) == {"SINGLE_OK", "L1"}  # (they share the last 16 bases)
    assert b.far(300) == (3, 0)
    k = b.key_at(400)
    assert b.r.neighbours(k) == [] and b.r.gsize[0][k] == 1 and b.r.gsize[1][k] == 1
    assert flag_names(b.x(400)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"} and not b.y(400) & H.NEAR_FREE and b.y(350) & H.NEAR_FREE


def _facts_far(b):
    code = {1: 0, 2: 0, 3: 1, 4: 2, 7: 2, 8: 3}
    for side in range(2):
        for i, d in enumerate(FAR_DISTANCES):
            p = 100 + 60 * (len(FAR_DISTANCES) * side + i)
            k = b.key_at(p)
            assert b.r.nearest_sharer(k, side) == d and b.r.nearest_sharer(k, 1 - side) is None, (side, d)
            want = (code[d], 3) if side == 0 else (3, code[d])
            assert b.far(p) == want and b.far(p + 1000) == want, (side, d, b.far(p))
    assert b.far(50) == (3, 3)  # none


def _facts_crowded(b):
    for n in CROWDS:
        for j in (0, n - 1):
            p = crowd_at(n) + 40 * j
            k = b.key_at(p)
            assert b.r.gsize[0][k] == n and b.r.gsize[1][k] == 1 and b.r.neighbours(k) == []
            d = b.r.nearest_sharer(k, 0)
            assert d >= 3  # (sixteen random bases: far enough that only the group's size decides)
            want = {"SINGLE_OK", "R1"} | ({"EXACT_OK"} if n <= 16 else set())
            assert flag_names(b.x(p)) == want, (n, j, flag_names(b.x(p)))
            assert (b.far(p)[0] != 0) == (n <= 64) and b.far(p)[1] == 3, (n, b.far(p))
            # ... and the 32-mer that ENDS with the planted 16: the same for the last halves
            p -= 16
            k = b.key_at(p)
            assert b.r.gsize[1][k] == n and b.r.gsize[0][k] == 1 and b.r.neighbours(k) == [] and b.r.nearest_sharer(k, 1) >= 3
            assert flag_names(b.x(p)) == {"SINGLE_OK", "L1"} | ({"EXACT_OK"} if n <= 16 else set()), (n, j, flag_names(b.x(p)))
            assert (b.far(p)[1] != 0) == (n <= 64) and b.far(p)[0] == 3, (n, b.far(p))


def _facts_crowded_nb(b):
    for at, n_alt in ((200, 16), (450, 17)):
        p = at - 13  # the six bases at offsets 13..18 of the k-mer
        k = b.key_at(p)
        assert b.r.nb[k] == n_alt and len(b.r.neighbours(k)) == n_alt and (b.r.gsize[0][k], b.r.gsize[1][k]) == (n_alt - 8, 10)
        own = b.r.labels_of(k)
        assert len(own) == 1 and all(b.r.labels_of(nbk)[0][:3] == own[0][:3] for nbk in b.r.neighbours(k))
        assert flag_names(b.x(p)) == ({"SINGLE_OK", "EXACT_OK", "PAR"} if n_alt <= 16 else {"SINGLE_OK"}), (n_alt, flag_names(b.x(p)))
        k = b.key_at(at)  # all six in the first half: one group of them all (HINT_HE_CAP: 17 and 18 keys)
        assert b.r.gsize[1][k] == n_alt + 1 and flag_names(b.x(at)) == {"SINGLE_OK", "L1"}
    # labels, not keys, add up: 15 neighbour keys with 16 and with 17 labels
    for at, labels in ((700, 16), (950, 17)):
        k = b.key_at(at - 13)
        assert len(b.r.neighbours(k)) == 15 and b.r.nb[k] == labels and max(b.r.gsize[0][k], b.r.gsize[1][k]) <= 10
        assert flag_names(b.x(at - 13)) == ({"SINGLE_OK", "EXACT_OK", "PAR"} if labels <= 16 else {"SINGLE_OK"})


def _own(b, p):
    k = b.key_at(p)
    return sorted(b.r.labels_of(k)) if k >= 0 else []


def _facts_multi(b):
    g = b.r.g
    assert [int(v) for v in g["ref_nvar"][:5]] == [4, 8, 9, 10, 6] and all(int(x) == 2 for x in g["var_len"][:31]) and all(int(x) == 3 for x in g["var_len"][31:37])
    own = _own(b, 901)
    assert len(own) == 5 and max(o[3] for o in own) < H.MASK_BITS and len({o[:3] for o in own}) == 1 and b.x(901) == H.NO_SITE << 16 and b.r.nb[b.key_at(901)] == 0
    seen = {}
    for site, at in enumerate((100, 300, 500, 700)):
        p = at + 1  # the k-mer that starts on the alleles' second base
        own = _own(b, p)
        assert all(o[:3] == (REGION_BEGIN + 1 + p, REGION_BEGIN + p + K, site) for o in own)
        seen[site] = (len(own), max(o[3] for o in own), flag_names(b.x(p)), (b.x(p) >> 8) & 0xFF, b.x(p) >> 16)
    # 2 and 4 alleles spell the k-mer: HINT_MULTI with their set
    assert seen[0][:1] == (2,) and seen[0][2] >= {"MULTI", "EXACT_OK"} and "SINGLE_OK" not in seen[0][2] and seen[0][4] == 0
    assert seen[1][:1] == (4,) and seen[1][2] >= {"MULTI", "EXACT_OK"} and seen[1][4] == 1
    for site in (0, 1):
        assert seen[site][3] == sum(1 << o[3] for o in _own(b, (100, 300)[site] + 1))
    # three labels, one of them allele 8: nothing (the byte holds allele numbers below HINT_MASK_BITS)
    assert seen[2][:2] == (3, 8) and seen[2][2] == set() and seen[2][4] == H.NO_SITE
    assert seen[3][0] == 5 and seen[3][2] == set() and seen[3][4] == H.NO_SITE  # five labels: more than HINT_OWN_MAX
    # ... against allele 7: the second base of allele 7 of the site of 8, in that allele's window, is spelled by four alleles, 7 among them
    w, q0 = b.window(300, 7)
    x = b.x(q0 + H.WIN_BEFORE + 1)
    assert flag_names(x) >= {"MULTI", "EXACT_OK"} and (x >> 8) & 0x80 and bin((x >> 8) & 0xFF).count("1") == 4 and x >> 16 == 1
    # one label naming an alternative allele: a window's k-mer that starts on the allele's first base
    w, q0 = b.window(100, 1)
    x = b.x(q0 + H.WIN_BEFORE)
    assert flag_names(x) >= {"MULTI", "EXACT_OK"} and (x >> 8) & 0xFF == 1 << 1 and x >> 16 == 0


def _facts_two(b):
    # the k-mers over both sites of a pair: two labels, one per site
    def pair(at):
        out = []
        for p in range(at - 30, at + 1):
            own = _own(b, p)
            out.append((p, own, flag_names(b.x(p)), (b.x(p) >> 8) & 0xFF, b.x(p) >> 16))
        return out
    for p, own, names, alleles, site in pair(100):
        assert [o[2:] for o in own] == [(0, 0), (1, 0)] and names >= {"TWO", "EXACT_OK", "PAR"} and "SINGLE_OK" not in names
        assert alleles == 0x11 and site == 0
    for p, own, names, alleles, site in pair(300):
        assert [o[2:] for o in own] == [(2, 0), (3, 0)] and "TWO" in names and alleles == 0x11 and site == 2
    # alleles 3 against 4: in the windows of the pairs' alternative alleles the labels name those alleles
    w3, q3 = b.window(300, 3)
    x = b.x(q3 + H.WIN_BEFORE - 10)
    assert "TWO" in flag_names(x) and (x >> 8) & 0xFF == 0x18 and x >> 16 == 2
    w4, q4 = b.window(500, 4)
    x = b.x(q4 + H.WIN_BEFORE - 10)
    assert flag_names(x) == set() and x >> 16 == H.NO_SITE  # an allele number 4 does not fit HINT_TWO's four bits
    w1, q1 = b.window(500, 1)
    assert "TWO" in flag_names(b.x(q1 + H.WIN_BEFORE - 10))
    # neighbour labels on one of the own sites (the pairs above: HINT_PAR) against a foreign one
    for p, own, names, alleles, site in pair(800):
        if p < 779:
            continue  # (the copy spells these k-mers itself: three labels)
        foreign = [lb for nbk in b.r.neighbours(b.key_at(p)) for lb in b.r.labels_of(nbk) if lb[2] == H.INVALID]
        assert [o[2:] for o in own] == [(6, 0), (7, 0)] and len(foreign) == 1 and names == set() and site == H.NO_SITE, (p, names)


def _facts_two_more(b):
    site = int(b.r.tail[1428][1])
    for p, first in ((1400, site), (1430, site + 1)):
        k = b.key_at(p)
        own = b.r.labels_of(k)
        assert [o[2:] for o in own] == [(first, 0), (first + 1, 0)] and flag_names(b.x(p)) == set()
        odd = [lb for n in b.r.neighbours(k) for lb in b.r.labels_of(n) if lb[:2] != own[0][:2]]
        assert len(odd) == 2 and all(lb[2] in (first, first + 1) for lb in odd)  # on the own sites, on another interval
        assert all((lb[0] == own[0][0]) == (p == 1400) and (lb[1] == own[0][1]) == (p == 1430) for lb in odd)
    assert "TWO" in flag_names(b.x(1401)) and "TWO" in flag_names(b.x(1399))
    s3 = int(b.r.tail[1699][1])
    assert [o[2:] for o in _own(b, 1690)] == [(s3, 0), (s3 + 1, 0), (s3 + 2, 0)] and flag_names(b.x(1690)) == set()
    assert [o[2:] for o in _own(b, 1669)] == [(s3, 0)] and "TWO" in flag_names(b.x(1670)) and flag_names(b.x(1671)) == set()


def _facts_letters(b):
    assert b.plane_code(800) == 0 and b.x(790) == H.NO_SITE << 16
    assert b.plane_code(200) == 15 and b.plane_code(400) == 5 and b.plane_code(600) == 10 and b.plane_code(199) == 1 << "ACGT".index(b.ref[199])
    for at in (200, 400, 600):
        for p in range(at - 31, at + 1):  # the 32 positions whose k-mer is invalid
            assert b.x(p) == H.NO_SITE << 16 and b.y(p) >> 16 == 0, (at, p)
        assert "SINGLE_OK" in flag_names(b.x(at - 32)) and "SINGLE_OK" in flag_names(b.x(at + 1))
    assert b.tail(599) == (H.TAIL_NODE, 0)  # a reference allele that is no A/C/G/T: not a SNP a walk may cross the simple way
    assert b.tail(699)[0] & H.TAIL_OK


def _facts_nodes(b):
    g = b.r.g
    assert [int(x) for x in g["ref_len"]] == [40, 254, 255, 256, 300, 49]
    starts = [int(x) - REGION_BEGIN - 1 for x in g["ref_order"]]
    assert b.y(0) & 0xFFFF == 40 and (b.y(39) & 0xFF, (b.y(39) >> 8) & 0xFF) == (1, 39)  # the first position; room / back
    for r, ln in ((1, 254), (2, 255), (3, 256), (4, 300)):
        s = starts[r]
        assert b.y(s) & 0xFFFF == min(255, ln) and b.y(s + 1) & 0xFFFF == min(255, ln - 1) | (1 << 8)
        assert (b.y(s + ln - 1) & 0xFF, (b.y(s + ln - 1) >> 8) & 0xFF) == (1, min(255, ln - 1))
        if ln >= 256:
            assert (b.y(s + 255) >> 8) & 0xFF == 255 and (b.y(s + 254) >> 8) & 0xFF == 254
    # the next node's length in the tail entry of the node in front: 254, 255, 255 (256), 255 (300)
    assert [(b.tail(starts[r])[0] >> 8) & 0xFF for r in range(4)] == [254, 255, 255, 255]
    assert all(b.tail(starts[r]) [0] & 3 == 3 and b.tail(starts[r])[1] == r for r in range(4))
    assert b.tail(starts[4]) == (H.TAIL_NODE, 4) and b.tail(starts[4] + 299) == (H.TAIL_NODE, 4)  # an indel site behind the node
    assert b.tail(starts[5]) == (0, 0) and b.tail(len(b.ref) - 1) == (0, 0)  # the last node has no tail entry
    n = len(b.ref)
    for p in range(n - 31, n):  # the last 31 positions: no k-mer
        assert b.x(p) == H.NO_SITE << 16 and b.y(p) == (n - p) | (min(255, p - starts[5]) << 8)
    assert "SINGLE_OK" in flag_names(b.x(n - 32))
    assert b.y(starts[1] - 1) & 0xFFFF == 0  # on a site: in no reference node


def _facts_windows(b):
    r = b.r
    with_windows = {so - REGION_BEGIN - 1: (site, a, len_a) for site, a, len_a, len_0, so in r.win if a == 1}
    assert sorted(with_windows) == [60, 400, 600, 1000, 1200, 1231, 1600, 2200, 2540]
    assert [len(b.alleles(with_windows[2200][0] + d)[0]) for d in (0, 1)] == [64, 65]  # ... a reference allele of 65 bases: no window
    assert [with_windows[at][2] for at in (60, 400, 600, 1000)] == [2, 63, 64, 1] and len(b.alleles(3)[1]) == 65  # ... 65 bases: no window
    assert sum(1 for w in r.win if w[4] == REGION_BEGIN + 1 + 1600) == 7 and int(r.g["ref_nvar"][with_windows[1600][0]]) == 8
    assert int(r.g["ref_nvar"][with_windows[1600][0] + 1]) == 9 and 1800 not in with_windows  # nine alleles: none
    assert 1400 not in with_windows and 1432 not in with_windows  # 31 bases between: each SNP stands alone
    # less than 160 behind the region's start: the window's first 100 positions have no base
    w, q0 = b.window(60)
    assert [b.plane_code(q0 + i) for i in (0, 99)] == [15, 15] and b.plane_code(q0 + 100) == 1 << "ACGT".index(b.ref[0])
    assert b.x(q0 + 99) == H.NO_SITE << 16 and b.x(q0 + 100) == b.x(0) and b.tail(q0 + 99) == (0, 0) and b.tail(q0 + 100) == b.tail(0)
    # ... in front of its end: the linear reference stops 59 bases behind the site
    w, q0 = b.window(2540)
    last = q0 + H.WIN_BEFORE + 3 + (len(b.ref) - 2541) - 1
    assert b.plane_code(last) == 1 << "ACGT".index(b.ref[-1]) and b.plane_code(last + 1) == 15 and b.x(last + 1) == H.NO_SITE << 16
    assert b.y(last) & 0xFFFF == 1 | (58 << 8) and b.y(last + 1) == 0
    # the window's own site loses HINT_TAIL_OK, another site keeps it
    w, q0 = b.window(1231)
    site = r.win[w][0]
    assert b.tail(1230)[0] & H.TAIL_OK and b.tail(1230)[1] == site and b.tail(q0 + H.WIN_BEFORE - 1) == (H.TAIL_NODE, site)
    assert b.tail(q0 + H.WIN_BEFORE - 32) == b.tail(1199) and b.tail(1199)[0] & H.TAIL_OK and b.tail(1199)[1] == site - 1
    # k-mers that just reach / just do not reach into the allele, on either side (the allele of 63 bases)
    w, q0 = b.window(400)
    assert (b.x(q0 + H.WIN_BEFORE - 32), b.y(q0 + H.WIN_BEFORE - 32)) == (b.x(400 - 32), b.y(400 - 32))
    x = b.x(q0 + H.WIN_BEFORE - 31)  # (the allele's first base is the reference allele's: both alleles spell the k-mer that ends on it)
    assert flag_names(x) == {"MULTI", "EXACT_OK"} and (x >> 8) & 0xFF == 3 and x >> 16 == 1 and x == b.x(400 - 31)
    # (one place on, and on the allele's last base, the reference path's k-mer is one substitution away on another interval: nothing)
    assert b.x(q0 + H.WIN_BEFORE - 30) == H.NO_SITE << 16 and b.x(q0 + H.WIN_BEFORE + 62) == H.NO_SITE << 16
    x = b.x(q0 + H.WIN_BEFORE + 61)  # one label, naming the alternative allele
    assert flag_names(x) == {"MULTI", "EXACT_OK"} and (x >> 8) & 0xFF == 2 and x >> 16 == 1
    assert (b.x(q0 + H.WIN_BEFORE + 63), b.y(q0 + H.WIN_BEFORE + 63)) == (b.x(401), b.y(401))
    # special positions as a label's start and end
    assert r.win_order(w, H.WIN_BEFORE) == REGION_BEGIN + 1 + 400 and r.win_order(w, H.WIN_BEFORE + 1) == H.SPECIAL_START + 1
    assert (int(r.special[0][1]), int(r.special[1][1])) == (REGION_BEGIN + 1 + 400, REGION_BEGIN + 1 + 401)
    # local + 32 > 384: none
    w, q0 = b.window(600)
    assert b.x(q0 + 353) == H.NO_SITE << 16 and b.y(q0 + 353) >> 16 == 0 and "SINGLE_OK" in flag_names(b.x(q0 + 352))
    # the deletion: the window's path leaves out the four bases
    w, q0 = b.window(1000)
    assert [b.plane_code(q0 + H.WIN_BEFORE + i) for i in range(3)] == [1 << "ACGT".index(c) for c in b.ref[1000] + b.ref[1005:1007]]
    x = b.x(q0 + H.WIN_BEFORE - 10)
    assert flag_names(x) >= {"MULTI", "EXACT_OK"} and (x >> 8) & 0xFF == 2 and "SINGLE_OK" in flag_names(b.x(1000 - 10))


def _facts_pruned(b):
    assert b.alleles(0) == [b.ref[300:302], subst(b.ref[300:302], 0, 1)]
    for p in range(270, 301):  # both bases of the reference allele: not indexed here
        k = b.key_at(p)
        assert (k >= 0) == (p == 285) and b.x(p) == H.NO_SITE << 16 and b.far(p) == ((3, 3) if p == 285 else (0, 0)), p
    assert [lb[:3] for lb in b.r.labels_of(b.key_at(285))] == [(REGION_BEGIN + 501, REGION_BEGIN + 532, H.INVALID)]
    assert flag_names(b.x(500)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"}
    for p in range(880, 901):  # over the SNP and both bases: the key's labels are the two of the copy, 300 further on
        own = _own(b, p)
        assert [(o[0] - REGION_BEGIN - 1, o[3]) for o in own] == [(p + 300, 0)] * 2 and own[1][2] == own[0][2] + 1 and b.x(p) == H.NO_SITE << 16, p
        assert "TWO" in flag_names(b.x(p + 300))
    for p in (269, 301):  # one base of it: the reference allele's label
        assert flag_names(b.x(p)) >= {"SINGLE_OK"} and b.x(p) >> 16 == 0


def _facts_sv(b):
    assert len(b.want[5]) == 0 and len(b.want[6]) == 0 and not b.want[2].any()  # no windows, no tail entries
    for at in (100, 300, 500):
        for p in range(at - 31, at + 1):
            k = b.key_at(p)
            assert k >= 0 and b.r.labels_of(k)[0][2] != H.INVALID and b.x(p) == H.NO_SITE << 16  # no flags on variant labels
    assert flag_names(b.x(20)) == {"SINGLE_OK", "EXACT_OK", "L1", "R1"}


def _facts_size(b):
    n, windows = len(b.ref), b.name.endswith("w")
    base = (n // 64 + 5) * 64
    total = base + H.WIN_STRIDE + 256 if windows else n
    assert len(b.want[0]) == 2 * total and len(b.want[2]) == 2 * total and len(b.want[1]) == 4 * (total // 32 + 8)
    assert b.r.win_base == base and len(b.r.win) == (1 if windows else 0)
    if windows:
        for t in (0, 2):
            assert not b.want[t][2 * n:2 * base].any() and not b.want[t][2 * (base + H.WIN_STRIDE):].any()  # every padding word is zero
        assert not b.want[1][4 * ((n + 31) // 32):4 * (base // 32)].any() and not b.want[1][4 * ((base + H.WIN_STRIDE) // 32):].any()
    else:
        assert not b.want[1][4 * ((n + 31) // 32):].any()
    if n % 32:  # the planes of the last partial group
        q = n // 32
        assert all(int(b.want[1][4 * q + pl]) >> (n % 32) == 0 for pl in range(4))
        assert sum(int(b.want[1][4 * q + pl]) for pl in range(4)) != 0


def _facts_two_all(b):
    _facts_two(b)
    _facts_two_more(b)


FACTS = dict(plain=_facts_plain, repeats=_facts_repeats, far=_facts_far, crowded=_facts_crowded, crowded_nb=_facts_crowded_nb, multi=_facts_multi,
             two=_facts_two_all, letters=_facts_letters, nodes=_facts_nodes, windows=_facts_windows, pruned=_facts_pruned, sv=_facts_sv)
for _name in NAMES:
    if _name.startswith("size"):
        FACTS[_name] = _facts_size


# ---- the sets through the stand-alone program (tests/emu_hint_tables) --------------------------------------------------------------
def write_case(name):
    """the case file of tests/emu_hint_tables: the set's graph as gtx_graph_build made it"""
    b = built(name)

    def write(path):
        g = b.graph
        with open(path, "wb") as f:
            f.write(np.array([int(b.sv), len(g["ref_order"]), len(g["var_order"]), len(g["dna"]), len(g["event_val"])], np.uint32).tobytes())
            for k in ("ref_order", "ref_len", "ref_dna_off", "ref_nvar", "ref_first_var", "var_order", "var_len", "var_dna_off", "var_out_ref"):
                f.write(np.ascontiguousarray(g[k], np.uint32).tobytes())
            f.write(np.ascontiguousarray(g["dna"], np.uint8).tobytes())
            if len(g["event_val"]):
                f.write(np.ascontiguousarray(g["event_off"], np.uint32).tobytes())
                f.write(np.ascontiguousarray(g["event_val"], np.int64).tobytes())
    return write


def read_tables(path):
    raw, at, out = open(path, "rb").read(), 0, []
    for _ in range(7):
        n = int(np.frombuffer(raw, np.uint64, 1, at)[0])
        out.append(np.frombuffer(raw, np.uint32, n, at + 8).copy())
        at += 8 + 4 * n
    assert at == len(raw)
    return out


def judge(name, run):
    """None, or how the tables the program wrote for set `name` differ from the restatement.  run(write, read): emu_programs.run"""
    return compare(name, run(write_case(name), read_tables))
