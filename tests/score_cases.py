"""Hand-made records and items for the scoring stage (gtx_score_batch* -> gtx_score_triage_kernel -> gtx_score_kernel -> gtx_score_big_kernel,
i.e. score_item and everything under it in graphtyper_amd/csrc/score_core.hpp): the case sets, what the restatement (tests/score_ref.py)
expects of each, a fact test per set that proves from the restatement's per-item output that the set reaches what it is for, and the
case files of the stand-alone program tests/emu_score.  All values are integers and every comparison is exact.

The graph (gtx.graph_from_records): sites 0..19 lie 8 positions apart and have 2, 3, 4, 2, ... alleles (one read spans 16 of them),
site 20 has 7 alleles, site 21 has 64, sites 22..25 are SNPs at 700, 795 (3 alleles), 800 and 1000: 23 is the last near site of 22
and 24 the first far one.  A record's positions only have to satisfy what the scorer reads of them (the reference reach of a path's
two ends against the order of its sites), so a path is placed around its sites, not aligned to the sequence.
No set here brings a cell's max_log_score to 0xFFFF - 8 (the guard of explain_to_score): the item orders that do, and gtx_scores_replay
over them, are tests/replay_cases.py."""
import collections
from fractions import Fraction
import functools
import itertools
import struct

import numpy as np

import score_ref as ref
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth

RB = 40000
SITE_CNUM = [(2, 3, 4, 2)[k % 4] for k in range(20)] + [7, 64, 2, 3, 2, 2]
SITE_POS = [100 + 8 * k for k in range(20)] + [400, 500, 700, 795, 800, 1000]
PAIRED, REVERSED, FIRST, SECOND = 1, 16, 64, 128
MAX_HAPS = 8  # SCORE_MAX_HAPS of score_core.hpp: sites in the per-thread tables of the first scoring pass
GUARD_SCORE = 0xFFFF - 8


@functools.lru_cache(maxsize=None)
def graph_inputs():
    rng = np.random.default_rng(5)
    bases = synth.make_reference(1200, seed=77)
    recs = []
    for p, cnum in zip(SITE_POS, SITE_CNUM):
        b = int(bases[p])
        if cnum <= 4:
            alts = ["ACGT"[(b + j) % 4] for j in range(1, cnum)]
        else:  # insertions behind the base
            alts = []
            while len(alts) < cnum - 1:
                s = "ACGT"[b] + synth.bases_to_str(rng.integers(0, 4, size=int(rng.integers(5, 9)), dtype=np.uint8))
                if s not in alts:
                    alts.append(s)
        recs.append((p + RB, "ACGT"[b], alts, None))
    return synth.bases_to_str(bases), recs, RB


@functools.lru_cache(maxsize=None)
def graph():
    ref_s, recs, rb = graph_inputs()
    return gtx.graph_from_records(ref_s, recs, region_begin=rb)


@functools.lru_cache(maxsize=None)
def host_ctx(params=()):
    """a context without a device: the layout tables"""
    ctx = gtx.Context(graph(), device=-1, **dict(params))
    assert ctx.hap_cnum.tolist() == SITE_CNUM
    return ctx


@functools.lru_cache(maxsize=None)
def facts():
    f = ref.Facts.of(host_ctx())
    assert f.near_last[22] == 23 and f.near_last[0] == 12 and f.near_last[20] == 20 and len(f.special_ref_reach) > 0
    return f


def order(site):
    return facts().hap_order[site]


# ---- records ------------------------------------------------------------------------------------------------------------------------
def G(size=150, sites=(), mm=0, read_len=150, n_paths=1, vary="", start=None, end=None, rs=0, has_var=None, per_path=None):
    """one GenotypePaths: n_paths paths of `size` read bases over `sites` = [(site, alleles), ...] (per_path: a list of such lists, one
    per path); size 0: no path.  The paths lie around their sites (every site overlapping) unless start / end say otherwise; path j > 0
    has its start, its end or both moved by j positions (`vary`), which is what all_paths_unique looks at."""
    if size == 0:
        return dict(read_len=read_len, paths=[], has_var=False)
    lists = per_path if per_path is not None else [list(sites)] * n_paths
    orders = [order(s) for lst in lists for s, _ in lst]
    s0 = start if start is not None else (min(orders) - 20 if orders else RB + 10)
    e0 = end if end is not None else (max(orders) + 20 if orders else s0 + size - 1)
    paths = []
    for j, lst in enumerate(lists):
        paths.append((s0 + (j if vary in ("start", "both") else 0), e0 + (j if vary in ("end", "both") else 0), rs, rs + size - 1, mm,
                      [(s, sorted(a)) for s, a in lst]))
    return dict(read_len=read_len, paths=paths, has_var=has_var)


def record_words(g, rec_words):
    """a GenotypePaths as record words (include/gtx.h:286-299)"""
    f = facts()
    w = [len(g["paths"]), 0]
    longest, any_site = 0, False
    for start, end, rs, re, mm, sites in g["paths"]:
        longest = max(longest, re - rs + 1)
        w += [start, end, rs | re << 16, mm | len(sites) << 16]
        for site, alleles in sites:
            assert site < f.n_hap and all(a < f.hap_cnum[site] for a in alleles), "what the kernel may index with"
            any_site = True
            mask = sum(1 << a for a in alleles)
            w += [site, mask & 0xFFFFFFFF, mask >> 32]
    has_var = any_site if g.get("has_var") is None else g["has_var"]
    w[1] = longest | g["read_len"] << 16 | (ref.REC_HAS_VARIANTS if has_var else 0)
    assert len(w) <= rec_words, "the record does not fit its slot"
    return w + [0] * (rec_words - len(w))


class Case:
    """records, items and what goes with them; notes[i]: what item i is there for (read by the fact tests)"""

    def __init__(self, rec_words=64, n_samples=1, near=True, spread=False, **params):
        """spread: an item that names no sample gets the next one in turn (two items whose results a wrong selection would swap must not
        add to the same cells, or the sums come out the same)"""
        self.rec_words, self.n_samples, self.near, self.params = rec_words, n_samples, near, tuple(sorted(params.items()))
        self.spread = spread
        self.par = ref.Params(**params)
        self.rows, self.item_rows, self.notes = [], [], []
        self.mult = None
        self.compact_reads = set()  # reads whose forward record lies in d_compact

    def read(self, fwd, rev=None, compact=False):
        """a read's two records -> its align_index.  rev None: an empty record of the read's length"""
        rev = rev if rev is not None else dict(read_len=fwd["read_len"], paths=[], has_var=False)
        self.rows += [record_words(fwd, self.rec_words), record_words(rev, self.rec_words)]
        if compact:
            assert not any(p[5] for p in fwd["paths"]) and len(fwd["paths"]) <= 1
            self.compact_reads.add(len(self.rows) // 2 - 1)
        return len(self.rows) // 2 - 1

    def _meta(self, ai, flag, mapq, score_diff):
        return (ai, flag, mapq, score_diff, 0, 0)

    def _sample(self, sample):
        return sample if sample is not None else len(self.item_rows) % self.n_samples if self.spread else 0

    def single(self, ai, flag=0, mapq=60, score_diff=0, sample=None, note=None):
        sample = self._sample(sample)
        self.item_rows.append((self._meta(ai, flag, mapq, score_diff), self._meta(ref.INVALID, 0, 0, 0), sample, 0))
        self.notes.append(note)

    def pair(self, a1, a2, flag1=PAIRED | FIRST, flag2=PAIRED | SECOND, mapq=(60, 60), score_diff=(0, 0), sample=None, kind=0, note=None):
        sample = self._sample(sample)
        self.item_rows.append((self._meta(a1, flag1, mapq[0], score_diff[0]), self._meta(a2, flag2, mapq[1], score_diff[1]), sample, kind))
        self.notes.append(note)

    def leftover(self, ai, flag=PAIRED | FIRST, mapq=60, score_diff=0, sample=None, note=None):
        """include/gtx.h:226-228: second = the same record with IS_FIRST_IN_PAIR | IS_SEQ_REVERSED toggled"""
        self.pair(ai, ai, flag, flag ^ (FIRST | REVERSED), (mapq, mapq), (score_diff, score_diff), sample, gtx.ITEM_LEFTOVER, note)

    @property
    def n_reads(self):
        return len(self.rows) // 2

    @functools.cached_property
    def records(self):
        return np.array(self.rows, np.uint32).reshape(-1)

    @functools.cached_property
    def items(self):
        a = np.zeros(len(self.item_rows), gtx.SCORE_ITEM)
        for i, (m1, m2, sample, kind) in enumerate(self.item_rows):
            for name, m in (("first", m1), ("second", m2)):
                for field, v in zip(("align_index", "flag", "mapq", "score_diff", "pos", "isize"), m):
                    a[name][field][i] = v
            a["sample"][i], a["kind"][i] = sample, kind
            assert sample < self.n_samples and m1[0] < self.n_reads and (m2[0] == ref.INVALID or m2[0] < self.n_reads)
        return a

    @functools.cached_property
    def side(self):
        """the side array of gtx_align_batch_flags as the aligner would have left it, with GTX_TASK_COMPACT on the compact reads"""
        words = self.records.reshape(-1, self.rec_words)
        s = ((words[:, 1] >> 31) & 1).astype(np.uint8)
        for r in self.compact_reads:
            s[2 * r] |= 2
        return s

    @functools.cached_property
    def compact(self):
        """d_compact: the compact reads' forward records as dense 8-word rows (every other row: words that mean nothing)"""
        c = np.full((max(self.n_reads, 1), 8), 0xDEADBEEF, np.uint32)
        for r in self.compact_reads:
            c[r] = self.records.reshape(-1, self.rec_words)[2 * r, :8]
        return c.reshape(-1)

    @functools.cached_property
    def records_beside_compact(self):
        """d_records of a compact call: the slots of the compact reads hold what the caller left there (here: a record that would add)"""
        w = self.records.reshape(-1, self.rec_words).copy()
        decoy = record_words(G(150, [(0, [1])]), self.rec_words) if self.rec_words >= 9 else [0] * self.rec_words
        for r in self.compact_reads:
            w[2 * r] = decoy
        return w.reshape(-1)


# ---- the sets -----------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 62, 63, 94, 95, 96, 150)


def make_single():
    c = Case(n_samples=70, spread=True)
    for lf, lr in itertools.product(LENGTHS, LENGTHS):
        c.single(c.read(G(lf, [(0, [1])]), G(lr, [(3, [1])])), note=("lengths", lf, lr))
    for size in (95, 150):
        for mf, mr in ((0, 1), (1, 1), (2, 1)):
            c.single(c.read(G(size, [(0, [1])], mm=mf), G(size, [(3, [1])], mm=mr)), note=("mismatches", mf, mr))
    for lf in (94, 95, 150):  # the reverse slot of a forward-only read is never looked at: here it holds a better record
        c.single(c.read(G(lf, [(0, [1])]), G(150, [(3, [1])])), flag=gtx.FLAG_FORWARD_ONLY, note=("forward_only", lf))
    c.single(c.read(G(150), G(150)), note=("no_variant",))
    c.single(c.read(G(150), G(150)), flag=gtx.FLAG_FORWARD_ONLY, note=("no_variant",))
    c.single(c.read(G(150, [(0, [1])], has_var=False), G(96, [(3, [1])], has_var=False)), note=("no_variant_bit",))
    return [c]


def facts_single(cases, exp):
    (c,), (s,) = cases, exp
    seen = collections.Counter()
    for note, it in zip(c.notes, s.items):
        if note[0] == "lengths":
            lf, lr = note[1:]
            want = 1 if lf > lr and lf > 94 else 2 if lr > lf and lr > 94 else 1 if lf == lr and lf > 94 else 0
            assert it["trivial"] == (lf == lr == 0) and (it["trivial"] or it["which"] == want)
            seen[want] += 1
            if want:
                assert it["reads"][0]["good"] and [x["site"] for x in it["reads"][0]["sites"]] == [0 if want == 1 else 3]
        elif note[0] == "mismatches":
            assert it["which"] == (2 if note[2] < note[1] else 1)
        elif note[0] == "forward_only":
            assert it["which"] == (1 if note[1] > 94 else 0) and all(x["site"] == 0 for r in it["reads"] for x in r["sites"])
        else:
            assert it["trivial"]
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and sum(seen.values()) == 49


def _pair_case(c, t, mm=(0, 0, 0, 0), n_paths=(1, 1, 1, 1), alt=(1, 1, 1, 1), read_len=150, note=None, **kw):
    """a mate pair whose four orientations have the longest paths t = (T11, T12, T21, T22) of compare_pair_of_genotype_paths: pair 1 =
    (first mate forward, second mate reverse), pair 2 = (first mate reverse, second mate forward); orientation k lies on site k"""
    g = [G(t[k], [(k, [1 if alt[k] else 0])], mm=mm[k], n_paths=n_paths[k], read_len=read_len) for k in range(4)]
    c.pair(c.read(g[0], g[2]), c.read(g[3], g[1]), note=note, **kw)


def make_pairs():
    c = Case(n_samples=70, spread=True)
    P = _pair_case
    P(c, (150, 150, 150, 100), note=("perfect_one", 1))
    P(c, (100, 150, 150, 150), note=("perfect_one", 2))
    P(c, (150, 150, 150, 150), mm=(0, 1, 1, 1), note=("perfect_mismatches", 1))
    P(c, (150, 150, 150, 150), mm=(1, 1, 0, 1), note=("perfect_mismatches", 2))
    P(c, (150, 150, 150, 150), n_paths=(1, 1, 1, 2), note=("perfect_paths", 1))
    P(c, (150, 150, 150, 150), n_paths=(2, 1, 1, 1), note=("perfect_paths", 2))
    P(c, (150, 150, 150, 150), alt=(1, 0, 0, 0), note=("perfect_alt_calls", 1))
    P(c, (150, 150, 150, 150), alt=(0, 0, 0, 0), note=("perfect_alt_calls", 1))
    P(c, (150, 150, 150, 150), alt=(0, 0, 1, 0), note=("perfect_alt_calls", 2))
    for m in (93, 94, 95):
        P(c, (m, 80, 0, 0), note=("rule63" if m < 94 else "longer", 1))
        P(c, (80, m, 0, 0), note=("rule63" if m < 94 else "longer", 1))
        P(c, (0, 0, m, 80), note=("rule63" if m < 94 else "longer", 2))
        P(c, (0, 0, 80, m), note=("rule63" if m < 94 else "longer", 2))
        P(c, (m, 80, 92, 80), note=("last" if m < 94 else "longer", 1))
        P(c, (92, 80, 80, m), note=("last" if m < 94 else "longer", 1 if m < 94 else 2))
    for t, which in (((93, 63, 0, 0), 1), ((93, 62, 0, 0), 1), ((0, 0, 93, 63), 2), ((0, 0, 62, 93), 1), ((0, 0, 93, 62), 1), ((0, 0, 63, 63), 2), ((63, 62, 0, 0), 1)):
        rule = "rule63" if min(x for x in t if x) >= 63 else "last"
        P(c, t, note=(rule, which))
    # equal maxima of at least 94: the mismatches of the longest, capped at 10 (reads of 600 bases keep 11 mismatches legal)
    for m1, m2, which in ((9, 10, 1), (10, 9, 2), (10, 11, 0), (11, 10, 0), (9, 11, 1), (11, 9, 2), (10, 10, 0)):
        P(c, (500, 450, 500, 450), mm=(m1, 0, m2, 0), read_len=600, note=("mismatches" if which else "tie", which))
        P(c, (450, 500, 450, 500), mm=(0, m1, 0, m2), read_len=600, note=("mismatches" if which else "tie", which))
    P(c, (500, 500, 500, 450), mm=(3, 1, 2, 0), read_len=600, note=("mismatches", 1))  # the lower of two equally long ones
    P(c, (100, 150, 150, 100), mm=(0, 0, 1, 0), note=("mismatches", 1))  # one read of each pair is whole: neither pair is perfect
    P(c, (500, 450, 500, 460), read_len=600, note=("minimum", 1))
    P(c, (500, 460, 500, 450), read_len=600, note=("minimum", 2))
    P(c, (460, 500, 500, 450), read_len=600, note=("minimum", 2))
    P(c, (500, 450, 450, 500), read_len=600, note=("tie", 0))
    P(c, (94, 94, 94, 94), note=("tie", 0))
    # two records with the same IS_FIRST_IN_PAIR: nothing is added
    P(c, (150, 150, 150, 100), flag1=PAIRED | FIRST, flag2=PAIRED | FIRST, note=("orientation", None))
    P(c, (150, 150, 150, 100), flag1=PAIRED | SECOND, flag2=PAIRED | SECOND | REVERSED, note=("orientation", None))
    # the mates the other way round and on the reverse strand: which orientation goes where follows the flags
    P(c, (150, 150, 150, 100), flag1=PAIRED | SECOND, flag2=PAIRED | FIRST, note=("perfect_one", 2))
    P(c, (150, 150, 150, 100), flag1=PAIRED | FIRST | REVERSED, flag2=PAIRED | SECOND | REVERSED, note=("perfect_one", 2))
    # a read whose mate never came: the better orientation "pair" of the read with itself, its first member alone
    for lf, lr, which in ((150, 100, 1), (100, 150, 2), (150, 150, 1), (93, 0, 1), (0, 93, 2), (94, 94, 0)):
        c.leftover(c.read(G(lf, [(0, [1])]), G(lr, [(3, [1])])), note=("leftover", which))
    c.leftover(c.read(G(150, [(0, [1])]), G(100, [(3, [1])])), flag=PAIRED | SECOND | REVERSED, note=("leftover", 1))  # (the copy is the first in pair)
    # either mate aligned forward only: its reverse slot holds a better record that is never looked at
    decoy = G(150, [(5, [1])])
    c.pair(c.read(G(150, [(0, [1])]), decoy), c.read(G(150, [(3, [1])]), G(150, [(1, [1])])), flag1=PAIRED | FIRST | gtx.FLAG_FORWARD_ONLY,
           note=("forward_only", 1))
    c.pair(c.read(G(150, [(0, [1])]), G(150, [(2, [1])])), c.read(G(150, [(3, [1])]), decoy), flag2=PAIRED | SECOND | gtx.FLAG_FORWARD_ONLY,
           note=("forward_only", 2))
    c.pair(c.read(G(150, [(0, [1])]), decoy), c.read(G(150, [(3, [1])]), decoy), flag1=PAIRED | FIRST | gtx.FLAG_FORWARD_ONLY,
           flag2=PAIRED | SECOND | REVERSED | gtx.FLAG_FORWARD_ONLY, note=("forward_only", 1))  # (a concordant pair: both aligned forward only)
    return [c]


def facts_pairs(cases, exp):
    (c,), (s,) = cases, exp
    rules = collections.Counter()
    for note, it in zip(c.notes, s.items):
        assert not it["trivial"]
        if note[0] == "leftover":
            assert it["kind"] == "leftover" and it["which"] == note[1] and len(it["reads"]) == (1 if note[1] else 0)
        elif note[0] == "forward_only":
            assert it["which"] == note[1] and 5 not in {x["site"] for r in it["reads"] for x in r["sites"]}
        else:
            assert (it["rule"], it["which"]) == note, (note, it["rule"], it["which"])
            rules[(it["rule"], it["which"])] += 1
    want = {(r, w) for r in ("perfect_one", "perfect_mismatches", "perfect_paths", "perfect_alt_calls", "longer", "mismatches", "minimum", "rule63")
            for w in (1, 2)} | {("tie", 0), ("last", 1), ("orientation", None)}
    assert set(rules) == want
    added = [bool(it["reads"]) and any(r["sites"] for r in it["reads"]) for it in s.items]
    assert not any(a for a, n in zip(added, c.notes) if n[0] in ("tie", "orientation")) and sum(added) > 40


def make_goodness():
    out = []
    for params in ({}, dict(hq_reads=True), dict(is_sv_graph=True), dict(is_segment_calling=True)):
        c = Case(n_samples=31, spread=True, **params)
        big = G(150, [(3, [1])])
        for size in (62, 63, 64):  # a first path of that size that is not the whole read, reached through a pair whose other mate decides
            c.pair(c.read(G(size, [(0, [1])])), c.read(G(0), big), note=("size", size, False))
        for size in (89, 90):      # ... that is the whole read
            c.pair(c.read(G(size, [(0, [1])], read_len=size)), c.read(G(0), big), note=("size", size, True))
        for mm, size, read_len in ((4, 100, 100), (5, 100, 100), (6, 100, 100), (2, 120, 150), (3, 120, 150), (4, 120, 150), (2, 100, 100),
                                   (3, 100, 100), (6, 200, 200), (7, 200, 200), (8, 200, 200), (5, 200, 250), (9, 300, 300), (6, 240, 250)):
            c.single(c.read(G(size, [(0, [1])], mm=mm, read_len=read_len)), note=("ratio", mm, size, size == read_len))
        for vary in ("", "start", "end", "both"):
            for size in (120, 150):
                c.single(c.read(G(size, [(0, [1])], n_paths=3, vary=vary)), note=("paths", vary, size == 150))
        # two paths that start apart and end on two special positions (inside an insertion of site 20) with one reference reach: unique
        special = ref.SPECIAL_START + 2
        c.single(c.read(G(120, per_path=[[(20, [1])], [(20, [0])]], vary="both", start=order(20) - 60, end=special)), note=("special", special))
        c.pair(c.read(G(150, [(0, [1])])), c.read(G(0), G(150, [(3, [1])], mm=8)), note=("bad_mate",))
        c.pair(c.read(G(150, [(0, [1])])), c.read(G(0), G(150, [(3, [1])], mm=1)), note=("good_mates",))
        c.leftover(c.read(G(150, [(0, [1])])), note=("good_leftover",))
        out.append(c)
    return out


def facts_goodness(cases, exp):
    for c, s in zip(cases, exp):
        par = c.par
        strict = par.hq_reads or par.is_sv_graph
        top = 0.03 if par.is_sv_graph else 0.035 if par.hq_reads else 0.05
        for note, it in zip(c.notes, s.items):
            reads = it["reads"]
            if par.is_segment_calling and it["kind"] == "single":
                assert not reads
            elif note[0] == "size":
                size, fully = note[1:]
                want = (size >= 63 if not fully else True) and not (strict and (not fully or size < 90))
                assert reads[0]["good"] == want and reads[1]["good"], (c.params, note)
            elif note[0] == "ratio":
                mm, size, fully = note[1:]
                want = Fraction(mm, size) <= Fraction(str(top if fully else 0.025)) and not (strict and not fully)
                assert reads[0]["good"] == want, (c.params, note)
            elif note[0] == "paths":
                vary, fully = note[1:]
                assert reads[0]["good"] == ((fully or vary != "both") and not (strict and not fully))
                if reads[0]["good"]:
                    assert reads[0]["unique"] == (vary != "both")
            elif note[0] == "special":
                f = facts()
                assert f.ref_reach(note[1]) == f.ref_reach(note[1] + 1) != note[1] and reads[0]["good"] == (not strict) and (strict or reads[0]["unique"])
            elif note[0] in ("bad_mate", "good_mates"):
                assert [r["good"] for r in reads] == [True, note[0] == "good_mates"]
                assert bool(reads[0]["sites"]) == (note[0] == "good_mates" or not par.is_segment_calling)
            else:
                assert bool(reads[0]["sites"]) == (not par.is_segment_calling)
    assert [c.params for c in cases] == [(), (("hq_reads", True),), (("is_sv_graph", True),), (("is_segment_calling", True),)]


MASKS = ([0], [1], [2], [0, 1], [1, 2], [])


def make_coverage():
    c = Case(n_samples=2)
    for n in (1, 2, 3):
        for seq in itertools.product(range(len(MASKS)), repeat=n):
            fwd = G(150, per_path=[[(2, MASKS[k])] for k in seq], has_var=True)
            c.single(c.read(fwd), sample=0, note=("masks", seq, False))
            c.pair(c.read(fwd), c.read(G(0), G(150)), sample=1, note=("masks", seq, True))
    for masks in ([[63]], [[63], [63]], [[63], [0]], [[63], [5]], [list(range(64))], [[31], [32]]):
        fwd = G(150, per_path=[[(21, m)] for m in masks])
        c.single(c.read(fwd), sample=0, note=("allele63", tuple(map(tuple, masks)), False))
        c.pair(c.read(fwd), c.read(G(0), G(150)), sample=1, note=("allele63", tuple(map(tuple, masks)), True))
    return [c]


def facts_coverage(cases, exp):
    (c,), (s,) = cases, exp
    transitions, outcomes = set(), set()
    for note, it in zip(c.notes, s.items):
        sites = it["reads"][0]["sites"]
        seq = [MASKS[k] for k in note[1]] if note[0] == "masks" else [list(m) for m in note[1]]
        cov = ref.NO_COVERAGE
        for m in seq:
            for add in ([] if not m else [min(m)] if len(m) == 1 else [1, 0 if 0 in m else 2]):
                new = ref.add_coverage(cov, add)
                transitions.add((cov if cov >= 0xFFFD else "allele", "ref" if add == 0 else "same" if add == cov else "other"))
                cov = new
        if not any(seq):
            assert not sites  # a site whose only masks are empty
            continue
        assert len(sites) == 1 and sites[0]["coverage"] == cov and sites[0]["explains"] == frozenset(a for m in seq for a in m)
        outcomes.add(("ref" if cov == 0 else "alt" if cov < ref.MULTI_REF_COVERAGE else cov, note[2]))
    assert outcomes == {(k, pp) for k in ("ref", "alt", ref.MULTI_REF_COVERAGE, ref.MULTI_ALT_COVERAGE) for pp in (False, True)}
    # from every state (none, one allele, MULTI_ALT, MULTI_REF) with the reference allele, the same allele and another one
    assert transitions >= {
        (ref.NO_COVERAGE, "ref"), (ref.NO_COVERAGE, "other"), ("allele", "ref"), ("allele", "same"), ("allele", "other"),
        (ref.MULTI_ALT_COVERAGE, "ref"), (ref.MULTI_ALT_COVERAGE, "other"), (ref.MULTI_REF_COVERAGE, "ref"), (ref.MULTI_REF_COVERAGE, "other")}
    assert s.gt_cov[facts().allele_off[21] + 63] > 0 and any(63 in x["explains"] and len(x["explains"]) == 64 for it in s.items for r in it["reads"] for x in r["sites"])


def make_epsilon_stats():
    c = Case(n_samples=3)
    site = [(1, [2])]
    for mm in range(10):
        c.single(c.read(G(200, site, mm=mm, read_len=200)), note=("eps", max(12 - mm, 8) - 4))
    o = order(1)
    for deduct in itertools.product((False, True), repeat=4):  # not unique, bad mapq, clipped, not overlapping
        nu, bad, clip, off = deduct
        g = G(120 if clip else 150, site, mm=1, n_paths=2 if nu else 1, vary="both", start=o - (2 if off else 20), end=o + 30)
        want = max(12 - 1 - 3 * nu - 2 * bad - 3 * clip - off, 8) - 4
        c.single(c.read(g), mapq=24 if bad else 25, sample=1, note=("eps", want if not (nu and clip) else None))
    for ds, de, over in ((2, 30, False), (3, 30, True), (30, 3, False), (30, 4, True), (3, 4, True), (2, 3, False)):
        c.single(c.read(G(150, site, start=o - ds, end=o + de)), sample=2, note=("overlapping", over))
    for mapq in (0, 24, 25, 254, 255):
        c.single(c.read(G(150, site)), mapq=mapq, sample=2, note=("mapq", mapq))
    for sd in (0, 1, 255):
        c.single(c.read(G(150, site)), score_diff=sd, sample=2, note=("score_diff", sd))
    for read_len, size in ((150, 150), (150, 149), (182, 95)):
        c.single(c.read(G(size, site, read_len=read_len)), sample=2, note=("clipped", read_len - size))
        c.single(c.read(G(size, per_path=[[(2, [1])], [(2, [0])]], read_len=read_len)), sample=2, note=("clipped", read_len - size))
    for flag in (0, REVERSED, FIRST, FIRST | REVERSED):
        c.single(c.read(G(150, [(4, [1])])), flag=flag, note=("strand", flag))
        c.single(c.read(G(0), G(150, [(4, [0])])), flag=flag, note=("strand", flag ^ REVERSED))
        c.pair(c.read(G(150, [(7, [1])])), c.read(G(0), G(150, [(8, [1])])), flag1=PAIRED | flag, flag2=PAIRED | (flag ^ FIRST), note=("strand_pair", flag))
    # IS_MAPQ_BAD of a mate: on its forward orientation only (update_paths sets it on geno1 alone, alignment.cpp:500-501, :519)
    for mapq in ((24, 60), (25, 60), (60, 24), (60, 25), (10, 10)):
        c.pair(c.read(G(150, [(10, [1])])), c.read(G(0), G(150, [(11, [1])])), mapq=mapq, sample=1, note=("mapq_pair", mapq, (mapq[0] < 25, False)))
        c.pair(c.read(G(0), G(150, [(12, [1])])), c.read(G(150, [(13, [1])])), mapq=mapq, sample=1, note=("mapq_pair", mapq, (False, mapq[1] < 25)))
    for mm, read_len in ((0, 150), (1, 150), (256, 6000), (257, 6000)):  # mismatches_to_stats takes a uint8_t: 256 counts as none
        c.single(c.read(G(read_len, [(9, [1])], mm=mm, read_len=read_len)), note=("mismatches", mm))
    return [c]


def facts_epsilon_stats(cases, exp):
    (c,), (s,) = cases, exp
    f = facts()
    seen = collections.defaultdict(set)
    for note, it in zip(c.notes, s.items):
        r = it["reads"][0] if it["reads"] else None
        if note[0] == "eps" and note[1] is not None:
            assert r["good"] and r["sites"][0]["eps"] == note[1]
            seen["eps"].add(note[1])
        elif note[0] == "overlapping":
            assert r["sites"][0]["overlapping"] == note[1]
        elif note[0] in ("mapq", "score_diff", "clipped", "strand", "mismatches"):
            assert r["good"] and r["sites"]
            seen[note[0]].add(note[1])
        elif note[0] == "mapq_pair":
            assert [bool(x["flags"] & ref.IS_MAPQ_BAD) for x in it["reads"]] == list(note[2]) and [x["sites"][0]["eps"] for x in it["reads"]] == [6 if b else 8 for b in note[2]]
        elif note[0] == "strand_pair":
            assert len(it["reads"]) == 2 and all(x["good"] for x in it["reads"])
    assert seen["eps"] == {4, 5, 6, 7, 8} and seen["mapq"] == {0, 24, 25, 254, 255} and seen["clipped"] == {0, 1, 87}
    a = f.n_hap + 6 * (f.allele_off[4])
    assert all(s.stat_u32[a + 6 * al + k] > 0 for al in (0, 1) for k in (2, 3, 4, 5))  # every strand counter of both alleles of site 4
    a9 = f.n_hap + 6 * (f.allele_off[9] + 1)
    assert s.stat_u32[a9 + 1] == (1 * 1000) // 150 + (1 * 1000) // 6000 and s.stat_u32[a9 + 4] == 4  # 256 -> 0, 257 -> 1
    _below_guard(s)


def make_connections():
    out = []
    for near in (True, False):
        c = Case(n_samples=2, near=near)
        sets = {1: ([1], [1]), 2: ([1], [0, 1]), 3: ([1], [0, 1, 2]), 4: ([0, 1], [1, 2]), 6: ([0, 1], [0, 1, 2]), 9: ([0, 1, 2], [1, 2, 3])}
        for product, (a, b) in sets.items():
            c.single(c.read(G(150, [(1, a), (2, b)])), note=("product", product))
            c.single(c.read(G(150, [(17, a), (23, b if max(b) < 3 else [0, 1, 2])])), sample=1, note=("product", product))
        c.single(c.read(G(150, [(19, [1]), (20, list(range(7)))])), note=("product", 7))
        c.single(c.read(G(150, [(21, list(range(64))), (22, [1])])), note=("product", 64))
        c.single(c.read(G(150, [(6, [3]), (2, [1]), (1, [2])])), note=("descending",))
        c.single(c.read(G(150, per_path=[[(6, [3]), (1, [2])], [(2, [1]), (1, [0])]])), note=("two_paths",))
        c.single(c.read(G(150, [(22, [1]), (23, [2])])), sample=1, note=("near_edge", True))
        c.single(c.read(G(150, [(22, [1]), (24, [1])])), sample=1, note=("near_edge", False))
        c.single(c.read(G(150, [(0, [1]), (12, [1]), (13, [1])])), sample=1, note=("near_edge", None))
        far = G(0)
        # the mates' cross links: apart, with a shared site, the second mate's site in front of the first's, a set of 64 alleles
        c.pair(c.read(G(150, [(1, [1]), (2, [1, 2])])), c.read(far, G(150, [(23, [0, 2]), (24, [1])])), note=("cross", "apart"))
        c.pair(c.read(G(150, [(1, [1]), (2, [1, 2])])), c.read(far, G(150, [(2, [2, 3]), (5, [1])])), note=("cross", "shared"))
        c.pair(c.read(G(150, [(10, [1]), (11, [0])])), c.read(far, G(150, [(3, [1]), (10, [1])])), sample=1, note=("cross", "in_front"))
        c.pair(c.read(G(150, [(21, list(range(64)))])), c.read(far, G(150, [(25, [1]), (20, [0, 6])])), sample=1, note=("cross", "sixty_four"))
        c.pair(c.read(G(150, [(1, [1])])), c.read(far, G(150, [(2, [])], has_var=True)), note=("cross", "empty"))
        out.append(c)
    return out


def facts_connections(cases, exp):
    f = facts()
    for c, s in zip(cases, exp):
        log = collections.Counter()
        for (sample, h1, b1, h2, b2, count), k in s.conn_log.items():
            assert h1 < h2 and b1 < f.hap_cnum[h1] and b2 < f.hap_cnum[h2]
            assert not (c.near and h2 <= f.near_last[h1])
            log[(sample, h1, h2, count)] += k
        if c.near:
            assert sum(s.conn_near.values()) > 0 and (1, 22, 24, 1) in log and not any(k[1:3] == (22, 23) for k in log)
            assert (1, 0, 13, 1) in log and not any(k[1:3] == (0, 12) for k in log)
        else:
            assert not s.conn_near and (1, 22, 23, 1) in log
            # repeat = 6 / weight from weight 3 on, else 1: products 1, 2, 3, 4, 6, 7, 9 (and 64) give 1, 1, 2, 1, 1, 0, 0 (0)
            assert log[(0, 1, 2, 1)] >= 1 + 2 + 4 + 6 and log[(0, 1, 2, 2)] >= 3 and (0, 19, 20, 1) not in log and (0, 21, 22, 1) not in log
            assert log[(1, 21, 25, 1)] == 64 and log[(1, 20, 21, 1)] == 128  # cross links count a set of 64 alleles
            assert (0, 2, 5, 1) in log and log[(1, 3, 10, 1)] == 2 and log[(1, 3, 11, 1)] == 1 and log[(1, 10, 11, 1)] == 2
        for note, it in zip(c.notes, s.items):
            if note[0] == "product":
                n = [len(x["explains"]) for x in it["reads"][0]["sites"]]
                assert n[0] * n[1] == note[1], note


def make_site_tables():
    c = Case(rec_words=128, n_samples=2)
    alleles = lambda sites: [(s, [1]) for s in sites]  # noqa: E731
    for n in (1, 7, 8, 9, 16):
        c.single(c.read(G(150, alleles(range(n)))), note=("sites", n, 0))
        c.single(c.read(G(150, per_path=[alleles(range(n)), alleles(range(n - 1, -1, -1))])), sample=1, note=("sites", n, 0))
        c.single(c.read(G(150, per_path=[alleles(range(0, n, 2)), alleles(range(1, n, 2)) or alleles([0])])), sample=1, note=("sites", n, 0))
    # nine sites of which one has only empty masks: eight entries
    c.single(c.read(G(150, alleles(range(8)) + [(8, [])])), note=("sites", 8, 0))
    for n1, n2 in ((8, 8), (8, 9), (9, 8), (9, 9), (1, 16), (4, 4)):
        c.pair(c.read(G(150, alleles(range(n1)))), c.read(G(0), G(150, alleles(range(4, 4 + n2)))), sample=1, note=("sites", n1, n2))
    c.leftover(c.read(G(150, alleles(range(9)))), note=("sites", 9, 0))
    return [c]


def second_pass_items(s):
    """the items some read of which fills more than SCORE_MAX_HAPS = 8 table entries: the first pass gives them up (nothing added) and
    the second pass (gtx_score_big_kernel) redoes them whole"""
    return [i for i, it in enumerate(s.items) if any(len(r["sites"]) > MAX_HAPS for r in it["reads"])]


def facts_site_tables(cases, exp):
    (c,), (s,) = cases, exp
    big = second_pass_items(s)
    for i, (note, it) in enumerate(zip(c.notes, s.items)):
        assert [len(r["sites"]) for r in it["reads"]] == [n for n in note[1:] if n], note
        assert (i in big) == (max(note[1:]) > 8)
    assert len(big) == 3 + 3 + 3 + 1 + 1 and len(s.items) - len(big) == 12
    _below_guard(s)


def make_record_forms():
    out = []
    one = lambda nvar, **kw: G(150, [(k, [1]) for k in range(nvar)], **kw)  # noqa: E731
    for rec_words, nvars in ((8, (0,)), (12, (0, 1, 2)), (16, (0, 1, 2, 3)), (18, (0, 1, 2, 3, 4)), (32, (0, 1, 2, 3, 4, 8))):
        c = Case(rec_words=rec_words, n_samples=2)
        for nvar in nvars:
            c.single(c.read(one(nvar)), flag=gtx.FLAG_FORWARD_ONLY, note=("one_path", nvar))
            c.single(c.read(one(nvar), one(min(nvar, 1), mm=1)), sample=1, note=("one_path", nvar))
            if nvar:  # the forward record in d_compact (no site: what the position-hinted pass leaves there), the reverse one decides
                c.single(c.read(G(100), one(nvar), compact=True), sample=1, note=("compact", nvar))
                c.pair(c.read(one(0), compact=True), c.read(G(0), one(nvar)), note=("compact", nvar))
        if rec_words >= 16:
            c.single(c.read(G(150, per_path=[[(0, [1])], [(0, [0])]])), note=("two_paths",))
            c.single(c.read(G(150, per_path=[[], [(0, [0])]])), note=("two_paths",))
        if rec_words >= 12:
            c.single(c.read(G(150, [(0, [1])], has_var=False)), flag=gtx.FLAG_FORWARD_ONLY, note=("no_variant_bit",))
            c.pair(c.read(G(150, [(0, [1])], has_var=False)), c.read(G(0), G(150, [(1, [1])], has_var=False)), note=("no_variant_bit",))
        c.single(c.read(one(0), compact=True), flag=gtx.FLAG_FORWARD_ONLY, note=("compact", 0))
        out.append(c)
    return out


def facts_record_forms(cases, exp):
    assert [c.rec_words for c in cases] == [8, 12, 16, 18, 32]
    for c, s in zip(cases, exp):
        words = c.records.reshape(-1, c.rec_words)
        for note, it, row in zip(c.notes, s.items, c.item_rows):
            if note[0] == "no_variant_bit" or note[1:] == (0,):
                assert it["trivial"]
            elif note[0] in ("one_path", "compact"):
                assert sum(len(r["sites"]) for r in it["reads"]) == note[1]
            if note[0] == "one_path":
                # the staging of score_visit: whole record within 16 words, rec_words a multiple of 4
                assert (words[2 * row[0][0], 6 + 3 * note[1]:] == 0).all() and words[2 * row[0][0], 0] == 1
        assert c.compact_reads
        plain, dense = restate(c), restate(c, compact=True)  # the same sums from the records in their slots and from d_compact
        assert all(plain.dense(a) == dense.dense(a) for a in ref.Sums.ARRAYS) and plain.conn_log == dense.conn_log
    staged = {(c.rec_words, n[1]) for c in cases for n in c.notes if n[0] == "one_path" and c.rec_words % 4 == 0 and 6 + 3 * n[1] <= min(16, c.rec_words)}
    assert (16, 3) in staged and (32, 3) in staged and (32, 4) not in staged and (18, 3) not in staged and (12, 2) in staged


LANE_COUNTS = (1, 63, 64, 65, 127, 128, 129)


def make_lanes():
    out = []
    kinds = [lambda c: c.read(G(150)),                                     # trivial
             lambda c: c.read(G(150, [(0, [1])], mm=9)),                   # not good
             lambda c: c.read(G(94, [(0, [1])]), G(94, [(0, [1])])),       # a selection result of 0
             lambda c: c.read(G(150, [(0, [1])])),                         # good on a 2-allele site
             lambda c: c.read(G(150, [(20, [1, 5])]))]                     # good on a 7-allele site
    for n in LANE_COUNTS:
        c = Case(n_samples=3)
        reads = [k(c) for k in kinds]
        for i in range(n):
            c.single(reads[i % 5], sample=i % 3, mapq=60 if i % 2 else 255, note=("alternating", i % 5))
        out.append(c)
    c = Case(n_samples=70)
    r = c.read(G(150, [(1, [1]), (2, [2])], mm=1))
    for i in range(64):
        c.single(r, sample=5, mapq=254, score_diff=255, note=("equal",))
    out.append(c)
    c = Case(n_samples=70)  # groups of 1 .. 5 equal items interleaved: each group's items are equal among themselves, on a site of their own
    groups = [(size, c.read(G(150, [(k, [1])])), 10 + k) for k, size in enumerate((1, 2, 3, 4, 5, 5, 4, 3, 2, 1))]
    lanes = [g for g in groups for _ in range(g[0])]
    order_ = [lanes[(7 * i) % len(lanes)] for i in range(len(lanes))]  # (30 lanes, 7 is coprime: neighbours differ)
    for size, r, sample in order_ + order_:
        c.single(r, sample=sample, note=("group", size))
    out.append(c)
    c = Case(n_samples=64)  # 64 samples on the 7-allele site: 64 x 28 log_score counters against a table of 256
    r = c.read(G(150, [(20, list(range(7)))]))
    for i in range(64):
        c.single(r, sample=i, note=("samples",))
    out.append(c)
    c = Case(n_samples=2)  # equal counters, different addends: the same site and sample with different epsilons, mapq and score_diff
    for i in range(64):
        c.single(c.read(G(150, [(0, [1])], mm=i % 4)), mapq=(30, 40, 50, 254)[i // 16], score_diff=i % 3, sample=(i // 8) % 2, note=("addends", i % 4))
    out.append(c)
    return out


def facts_lanes(cases, exp):
    assert tuple(len(c.item_rows) for c in cases[:7]) == LANE_COUNTS
    for c, s in zip(cases[:7], exp[:7]):
        for note, it in zip(c.notes, s.items):
            k = note[1]
            assert it["trivial"] == (k == 0) and (k != 2 or it["which"] == 0) and (k != 1 or it["reads"][0]["good"] is False)
            assert (k < 3) or len(it["reads"][0]["sites"]) == 1
    assert len(cases[7].item_rows) == 64 and len({r for r in cases[7].item_rows}) == 1
    sizes = collections.Counter(n[1] for n in cases[8].notes[:30])
    assert sizes == {1: 2, 2: 4, 3: 6, 4: 8, 5: 10} and len(cases[8].item_rows) == 60  # on both sides of GTX_WAVE_GROUP_MIN = 4
    assert all(cases[8].item_rows[i] != cases[8].item_rows[i + 1] for i in range(59))
    assert len(exp[9].log_score) == 64 * 28 > 256
    assert len({it["reads"][0]["sites"][0]["eps"] for it in exp[10].items}) == 4
    for s in exp:
        _below_guard(s)


MANY_ITEMS = 1000003
MANY_ITEMS_SANITIZED = 4099


def make_many_items(n_items=MANY_ITEMS):
    """n_items items that name 64 shared reads, spread over 70 samples x 16 + 2 sites; by multiplicity for the restatement"""
    c = Case(n_samples=70)
    reads = [c.read(G(150, [(k % 16, [1]), ((k % 16 + 5) % 16, [k % 2])], mm=k % 3)) for k in range(48)]
    reads += [c.read(G(150, [(22 if k % 2 else 24, [k % 2])], mm=k % 3)) for k in range(16)]
    i = np.arange(n_items, dtype=np.int64)
    which = (i * 37 + i // 64) % 64
    sample = (i // 7) % 70
    mapq = np.where(which >= 48, 254, 60)
    a = np.zeros(n_items, gtx.SCORE_ITEM)
    a["first"]["align_index"] = np.array(reads)[which]
    a["first"]["flag"] = gtx.FLAG_FORWARD_ONLY
    a["first"]["mapq"] = mapq
    a["second"]["align_index"] = ref.INVALID
    a["sample"] = sample
    # the distinct items and how often each occurs
    key = which * 70 + sample
    counts = np.bincount(key, minlength=64 * 70)
    c.all_items = a
    for k in np.nonzero(counts)[0]:
        c.single(reads[k // 70], flag=gtx.FLAG_FORWARD_ONLY, mapq=254 if k // 70 >= 48 else 60, sample=int(k % 70), note=("distinct", int(counts[k])))
    c.mult = counts[np.nonzero(counts)[0]]
    return [c]


def facts_many_items(cases, exp):
    (c,), (s,) = cases, exp
    assert len(c.all_items) == MANY_ITEMS and int(c.mult.sum()) == MANY_ITEMS
    cells = [v for i, v in s.hap_u32.items() if i % 4 == 0]
    adds = collections.Counter()
    for it, row, k in zip(s.items, c.item_rows, c.mult):
        for x in it["reads"][0]["sites"]:
            adds[(row[2], x["site"])] += int(k)
    assert len(adds) == len(cells) >= 128 and max(adds.values()) <= 8000 and max(cells) < GUARD_SCORE  # no cell passes 8 000 adds (of at most 8)
    assert min(s.stat_u64[h] for h in (22, 24)) > 1 << 32
    _below_guard(s)


def _below_guard(s):
    assert all(v < GUARD_SCORE for i, v in s.hap_u32.items() if i % 4 == 0), "a cell at the guard of explain_to_score"


MAKERS = dict(single=make_single, pairs=make_pairs, goodness=make_goodness, coverage=make_coverage, epsilon_stats=make_epsilon_stats,
              connections=make_connections, site_tables=make_site_tables, record_forms=make_record_forms, lanes=make_lanes,
              many_items=make_many_items)
FACTS = dict(single=facts_single, pairs=facts_pairs, goodness=facts_goodness, coverage=facts_coverage, epsilon_stats=facts_epsilon_stats,
             connections=facts_connections, site_tables=facts_site_tables, record_forms=facts_record_forms, lanes=facts_lanes,
             many_items=facts_many_items)
SETS = sorted(MAKERS)
SANITIZED = [s for s in SETS if s != "many_items"]  # (many_items at full size is device + restatement only)
AUDITED = SANITIZED + ["aligned_records"]           # what runs through tests/emu_score whole: the hand-made sets and the aligner-made one


@functools.lru_cache(maxsize=None)
def cases(name):
    return MAKERS[name]()


def restate(case, items=None, mult=None, compact=False):
    """the restatement's sums of a case (or of other items over the case's records); compact: the compact reads' forward records
    taken from d_compact, their slots holding something else"""
    use_compact = compact
    return ref.score(facts(), case.par, case.records_beside_compact if use_compact else case.records, case.rec_words,
                     case.items if items is None else items, case.n_samples, multiplicity=case.mult if items is None else mult, near=case.near,
                     compact=case.compact if use_compact else None, side=case.side if use_compact else None)


@functools.lru_cache(maxsize=None)
def expected(name):
    out = [restate(c) for c in cases(name)]
    for s in out:
        _below_guard(s)
    return out


# ---- what a backend gave, and how it differs -------------------------------------------------------------------------------------------
class Got:
    """the accumulators a backend left: arrays by the names of score_ref.Sums.ARRAYS (conn_near None when there is none), conn_log
    [conn_cap, 6], conn_count [2]"""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)


def differences(case, want, got, conn_cap=None):
    """field by field: where `got` differs from the sums `want` -> list of (what, index, got, wanted), at most a few.  conn_cap: the
    log's capacity (None: large enough): the log holds min(cap, total) entries that are a sub-multiset of the expected one, and
    conn_count[1] the rest."""
    out = []
    for name in ref.Sums.ARRAYS:
        g = getattr(got, name)
        if name == "conn_near" and not case.near:
            assert g is None
            continue
        w = np.array(want.dense(name), np.uint64)
        if len(g) != len(w):
            out.append((name, "length", len(g), len(w)))
            continue
        bad = np.nonzero(np.asarray(g).astype(np.uint64) != w)[0]
        out += [(name, int(i), int(g[i]), int(w[i])) for i in bad[:3]]
    total = sum(want.conn_log.values())
    cap = total if conn_cap is None else conn_cap
    kept, dropped = min(cap, total), total - min(cap, total)
    # (conn_count[0] counts every claim: what was appended is the smaller of it and the capacity)
    if min(int(got.conn_count[0]), cap) != kept or int(got.conn_count[1]) != dropped:
        out.append(("conn_count", 0, tuple(int(x) for x in got.conn_count), (kept, dropped)))
    else:
        log = collections.Counter(tuple(int(x) for x in e) for e in np.asarray(got.conn_log).reshape(-1, 6)[:kept])
        extra = log - want.conn_log
        if extra or (dropped == 0 and log != want.conn_log):
            out.append(("conn_log", 0, sorted(extra.items())[:3], sorted((want.conn_log - log).items())[:3]))
    return out


# ---- aligned_records: records only the aligner can make (external: in the context's arena; wide: sets of more than 64 alleles) ----------
class Aligned:
    """one backend's records over a handful of reads, hand-made items over them, and what goes with them (the fields of a Case that
    differences(), through() and the oracle read)"""
    near, params, compact_reads, par, mult = True, (), (), ref.Params(), None

    def __init__(self, name, Backend, graph_inputs_, codes, pos, rec_words, n_samples):
        import harness
        self.name, self.rec_words, self.n_samples, self.graph_inputs = name, rec_words, n_samples, graph_inputs_
        ref_s, recs, rb, add_all = graph_inputs_
        self.b = Backend(gtx.graph_from_records(ref_s, recs, region_begin=rb, add_all_variants=add_all))
        self.ctx = self.b.ctx
        seq, lens = harness.pack_ragged(list(codes))
        self.records = self.b.align(seq, harness.read_meta(lens, pos=pos), rec_words=rec_words)
        self.big = self.b.big_records()[0]
        self.facts = ref.Facts.of(self.ctx)
        self.n_reads = len(codes)
        self.parsed = [ref.parse_record(self.records, 2 * r * rec_words, self.big) for r in range(self.n_reads)]

    def make_items(self, reads, more_pairs=()):
        """singles, concordant pairs of neighbours and of `more_pairs` (both forward records: the second mate's flag says reversed),
        leftovers"""
        rows = []
        for k, r in enumerate(reads):
            rows.append(((r, 0, 60 if k % 3 else 20, k % 4, 0, 0), (ref.INVALID, 0, 0, 0, 0, 0), k % self.n_samples, 0))
        for k, (r1, r2) in enumerate(list(zip(reads, reads[1:])) + list(more_pairs)):
            rows.append(((r1, PAIRED | FIRST, 60, 0, 0, 0), (r2, PAIRED | SECOND | REVERSED, 30, 1, 0, 0), k % self.n_samples, 0))
        for k, r in enumerate(reads[::3]):
            f1 = PAIRED | FIRST
            rows.append(((r, f1, 60, 0, 0, 0), (r, f1 ^ (FIRST | REVERSED), 60, 0, 0, 0), k % self.n_samples, gtx.ITEM_LEFTOVER))
        a = np.zeros(len(rows), gtx.SCORE_ITEM)
        for i, (m1, m2, sample, kind) in enumerate(rows):
            for name, m in (("first", m1), ("second", m2)):
                for field, v in zip(("align_index", "flag", "mapq", "score_diff", "pos", "isize"), m):
                    a[name][field][i] = v
            a["sample"][i], a["kind"][i] = sample, kind
        self.items = a
        return self

    def restate(self):
        return ref.score(self.facts, self.par, self.records, self.rec_words, self.items, self.n_samples, big_records=self.big)

    def backend_score(self):
        """-> (Got, the backend's harness.Accumulators)"""
        acc = self.b.score(self.items, self.records, self.n_samples, rec_words=self.rec_words)
        return Got(log_score=acc.log_score, gt_cov=acc.gt_cov, hap_u32=acc.hap_u32, stat_u64=acc.stat_u64, stat_u32=acc.stat_u32,
                   conn_near=acc.conn_near, conn_log=acc.conn_log.reshape(-1, 6), conn_count=acc.conn_count), acc


def largest_set(g):
    return max((len(a) for p in g.paths for _, a in p.vars), default=0)


def aligned_records(Backend):
    """-> [external, wide]: reads over two and more sites of this module's graph at rec_words = 8 (every record with a site is in the
    arena), and reads over a 100-allele site with a SNP 40 bases in front of it (records with GTX_REC_WIDE: the one way to
    gtx_score_wide_kernel; a read that ends on the site's first base is explained by all 100 alleles).  The wide graph is
    scenarios.wide_site_case's site A and SNPs, without its site of more than 1 000 alleles (whose genotype triangle of two million
    entries is what tests/calls_cases.py is for), plus that SNP."""
    import scenarios
    ref_s, recs, rb = graph_inputs()
    bases = np.array(["ACGT".index(ch) for ch in ref_s], np.uint8)
    codes, pos = [], []
    for start in (60, 90, 120, 180, 330, 440, 660):
        for alt in (False, True):
            r = bases[start:start + 150].copy()
            if alt:
                for p, cnum in zip(SITE_POS, SITE_CNUM):
                    if start <= p < start + 150 and cnum <= 4 and (p // 8) % 2:
                        r[p - start] = (int(r[p - start]) + 1) % 4
            codes.append(synth._CODE_OF_BASE[r])
            pos.append(start + rb)
    ext = Aligned("external", Backend, (ref_s, recs, rb, False), codes, np.array(pos, np.int64), 8, 3)
    ext.make_items(list(range(ext.n_reads)))
    rb2 = 20000
    ref2, recs2, codes2, pos2, (pA, pB) = scenarios.wide_site_case(region_begin=rb2)
    q = pA - 40
    recs3 = sorted([r for r in recs2 if not pB <= r[0] - rb2 <= pB + 12] + [(q + rb2, ref2[q], ["ACGT"[("ACGT".index(ref2[q]) + 1) % 4]], None)],
                   key=lambda r: r[0])
    take = [i for i in range(len(codes2)) if pA - 170 <= pos2[i] - rb2 < pA + 30][::3]
    wide = Aligned("wide", Backend, (ref2, recs3, rb2, True), [codes2[i] for i in take], np.array([pos2[i] for i in take], np.int64), 64, 2)
    reads = [r for r, g in enumerate(wide.parsed) if g.paths]
    big = [r for r in reads if largest_set(wide.parsed[r]) > 64]
    others = [r for r in reads if wide.parsed[r].has_var and r not in big][:3]
    wide.make_items(reads, [(b, o) for b in big[:2] for o in others] + [(o, b) for b in big[:2] for o in others])
    return [ext, wide]


@functools.lru_cache(maxsize=None)
def aligned_on_the_emulation():
    """the two sets over the emulation's records, and what the restatement expects of them"""
    import harness
    sets = aligned_records(harness.EmuBackend)
    return sets, [a.restate() for a in sets]


def facts_aligned_records(sets, exp):
    ext, wide = sets
    words = ext.records.reshape(-1, 8)
    with_sites = [r for r, g in enumerate(ext.parsed) if g.has_var]
    assert len(with_sites) >= 12 and all((int(words[2 * r, 0]) >> 16) & ref.ST_EXTERNAL for r in with_sites)
    assert max(len({s for p in g.paths for s, _ in p.vars}) for g in ext.parsed) > MAX_HAPS  # (and the second pass reads the arena too)
    assert any(any(a != frozenset([0]) for p in g.paths for _, a in p.vars) for g in ext.parsed)
    heads = wide.records.reshape(-1, 64)
    used = sorted({int(x) for x in wide.items["first"]["align_index"]})
    assert len(used) >= 10 and sum(bool(int(heads[2 * r, 1]) & ref.REC_WIDE) for r in used) >= 5
    assert any(max(a, default=0) >= 64 for r in used for p in wide.parsed[r].paths for _, a in p.vars)
    assert max(wide.facts.hap_cnum) == 100 and not any(int(heads[2 * r, 1]) & ref.REC_WIDE and not (int(heads[2 * r, 0]) >> 16) & ref.ST_EXTERNAL for r in used)
    # explain sets of more than 64 alleles, left out of the connections (vcf_writer.cpp:593, :614; the cross links take their keys from
    # the same maps): inside one read next to another site, and in a pair on the first and on the second mate next to the other's site
    inside, first, second = 0, 0, 0
    for it in exp[1].items:
        n = [[(x["site"], len(x["explains"])) for x in r["sites"]] for r in it["reads"]]
        inside += any(len(r) > 1 and max(k for _, k in r) > 64 for r in n)
        if it["kind"] == "pair" and len(n) == 2 and n[0] and n[1]:
            first += any(k > 64 for _, k in n[0]) and any(s not in dict(n[0]) for s, _ in n[1])
            second += any(k > 64 for _, k in n[1]) and any(s not in dict(n[1]) for s, _ in n[0])
    assert inside > 0 and first > 0 and second > 0, (inside, first, second)
    site = max(range(wide.facts.n_hap), key=lambda h: wide.facts.hap_cnum[h])
    assert not any(site in (e[1], e[3]) and e[5] != 1 for e in exp[1].conn_log)  # (what the site's small sets add are single counts)
    for s in exp:
        assert sum(s.hap_u32.values()) > 0 and {it["kind"] for it in s.items} == {"single", "pair", "leftover"}
        _below_guard(s)


# ---- the oracle as second witness -------------------------------------------------------------------------------------------------
def ctx_of(case):
    """the host context whose tables a case's arrays are laid out by"""
    return case.ctx if isinstance(case, Aligned) else host_ctx(case.params)


def facts_of(case):
    return case.facts if isinstance(case, Aligned) else facts()


def dense_arrays(case, sums, conn_cap=1 << 16):
    """the sums as the arrays of harness.Accumulators (what harness.canonical_scores reads)"""
    import harness
    acc = harness.Accumulators(ctx_of(case), case.n_samples, conn_cap=conn_cap, near=case.near)
    for name in ref.Sums.ARRAYS:
        if name != "conn_near" or case.near:
            getattr(acc, name)[:] = np.array(sums.dense(name), np.uint64).astype(getattr(acc, name).dtype)
    log = [e for e, k in sums.conn_log.items() for _ in range(k)]
    acc.conn_log[:6 * len(log)] = np.array(log, np.uint32).reshape(-1)
    acc.conn_count[0] = len(log)
    return acc


def held_to_the_oracle(case):
    """the items of a case the oracle can be asked about: all but those whose records carry sites without saying so in word 1 (a bit
    of the product's record format that the oracle's GenotypePaths do not have)"""
    return [i for i, note in enumerate(case.notes) if note[0] != "no_variant_bit"]


def oracle_scores(case, items):
    """gto_scores_dump of an oracle genotyper that was given the items over the case's records (OracleGenotyper.push_paths)"""
    from oracle_lib import Oracle
    ref_s, recs, rb, add_all = case.graph_inputs if isinstance(case, Aligned) else graph_inputs() + (False,)
    og = Oracle(ref_s, recs, region_begin=rb, is_sv_graph=case.par.is_sv_graph, hq_reads=case.par.hq_reads, add_all_variants=add_all).genotyper(case.n_samples, 1)
    og.push_paths(items, case.records, case.rec_words, big_records=getattr(case, "big", None), is_segment_calling=case.par.is_segment_calling)
    return og.scores()


# ---- case files of tests/emu_score --------------------------------------------------------------------------------------------------
def write_case(path, case, items, cap, compact=None, log_cap=0):
    """see tests/emu_score/emu_score.cpp.  compact: the compact reads' forward records in d_compact (None: where the case has any);
    log_cap: the first log block of tests/emu_replay"""
    ctx = ctx_of(case)
    f = facts_of(case)
    g = ctx.g
    big = getattr(case, "big", None)
    big = np.zeros(0, np.uint32) if big is None else np.ascontiguousarray(big, np.uint32)
    n_ref = len(g["ref_order"])
    assert n_ref >= f.n_hap
    compact = bool(case.compact_reads) if compact is None else compact
    records = case.records_beside_compact if compact else case.records
    with open(path, "wb") as fh:
        fh.write(struct.pack("<16I", n_ref, f.n_hap, len(f.special_ref_reach), case.n_samples, case.rec_words, case.n_reads, len(items), cap,
                             int(case.near), int(case.par.is_sv_graph), int(case.par.hq_reads), int(case.par.is_segment_calling), int(compact), len(big),
                             int(max(f.hap_cnum) > 64), log_cap))
        fh.write(struct.pack("<3Q", f.total_tri, f.total_allele, f.total_near))
        for name in ("ref_order", "ref_len", "ref_nvar"):
            fh.write(np.ascontiguousarray(g[name], np.uint32).tobytes())
        fh.write(np.array(f.tri_off, np.uint64).tobytes() + np.array(f.allele_off, np.uint64).tobytes())
        fh.write(np.array(f.near_last, np.uint32).tobytes() + np.array(f.near_off, np.uint64).tobytes())
        fh.write(np.array(f.special_ref_reach, np.uint32).tobytes())
        fh.write(np.ascontiguousarray(records, np.uint32).tobytes() + np.ascontiguousarray(items).tobytes())
        if compact:
            fh.write(case.compact.tobytes() + case.side.tobytes())
        fh.write(big.tobytes())


def read_result(path, case, cap, more=None):
    """more: what parses the bytes behind emu_score's own (tests/emu_replay writes some) -> Got.more"""
    f = facts_of(case)
    raw = np.fromfile(path, np.uint8)
    sizes = ref.Sums(f, case.n_samples).sizes()
    at, arrays = 0, {}
    for name, dtype in (("log_score", np.uint32), ("gt_cov", np.uint32), ("hap_u32", np.uint32), ("stat_u64", np.uint64), ("stat_u32", np.uint32),
                        ("conn_near", np.uint32)):
        n = sizes[name] if (name != "conn_near" or case.near) else 0
        arrays[name] = raw[at:at + n * np.dtype(dtype).itemsize].view(dtype).copy()
        at += n * np.dtype(dtype).itemsize
    if not case.near:
        arrays["conn_near"] = None
    arrays["conn_log"] = raw[at:at + cap * 24].view(np.uint32).copy().reshape(-1, 6)
    at += cap * 24
    arrays["conn_count"] = raw[at:at + 8].view(np.uint32).copy()
    arrays["errors"] = int(raw[at + 8:at + 12].view(np.uint32)[0])
    if more is None:
        assert at + 12 == len(raw)
    else:
        arrays["more"] = more(raw[at + 12:])
    return Got(**arrays)


def through(run, case, want, items=None, conn_cap=None, compact=None):
    """a case through tests/emu_score; run(write, read): emu_programs.run with a program and a directory -> Got"""
    cap = sum(want.conn_log.values()) + 16 if conn_cap is None else conn_cap
    return run(lambda path: write_case(path, case, case.items if items is None else items, cap, compact), lambda path: read_result(path, case, cap))


def sanitized_many_items():
    """many_items at the size that runs under the sanitizers: the first 4 099 items, the restatement by multiplicity"""
    (c,) = cases("many_items")
    items = c.all_items[:MANY_ITEMS_SANITIZED]
    key = collections.Counter((int(it["first"]["align_index"]), int(it["sample"])) for it in items)
    mult = [key[(row[0][0], row[2])] for row in c.item_rows]
    return c, items, restate(c, c.items, mult)


def judge(name, run):
    """None when the program behind `run` gives the set `name` as the restatement does, else how it differs"""
    if name == "many_items":
        c, items, want = sanitized_many_items()
        got = through(run, c, want, items)
        return "differs from the restatement" if differences(c, want, got) or got.errors else None
    if name == "aligned_records":
        for a, want in zip(*aligned_on_the_emulation()):
            got = through(run, a, want)
            if differences(a, want, got) or got.errors:
                return "differs from the restatement (%s)" % a.name
        return None
    for case, want in zip(cases(name), expected(name)):
        for compact in ((True, False) if case.compact_reads else (None,)):  # (dense rows in d_compact, and every record in its slot)
            got = through(run, case, want, compact=compact)
            if differences(case, want, got) or got.errors:
                return "differs from the restatement"
    if name == "connections":  # the log's capacity reached exactly, one short, none at all
        case, want = cases(name)[1], expected(name)[1]
        total = sum(want.conn_log.values())
        for cap in (total, total - 1, 0):
            if differences(case, want, through(run, case, want, conn_cap=cap), conn_cap=cap):
                return "differs from the restatement at conn_cap %d" % cap
    return None
