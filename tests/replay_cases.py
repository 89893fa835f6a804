"""Hand-made item orders for the saturation replay (gtx_scores_replay, _compact, _log, _apply: gtx_score_replay_kernel and
gtx_score_replay_wide_kernel, the replay branch of apply_recent in graphtyper_amd/csrc/score_core.hpp, replay_collect / replay_store in
gtx_api.hip and replay_cells in score_replay.hpp) on the graph, the records and the Case of tests/score_cases.py: the sets, what the
restatement (score_ref.score for the unguarded sums, score_ref.replay for the guard, call by call) expects of each, and a fact test per
set that proves from the restatement's output that the set reaches what it is for.  All values are integers, every comparison is exact.

A sample is a scenario of its own (a cell is sample * n_hap + site).  A scenario brings a cell to a chosen level with a prefix of whole,
unique, error-free reads (epsilon 8; mostly as pairs whose mates both lie over the site: 16 per item), a few reads of epsilon 4..7 at
the prefix's start setting the level's last bits, and then makes the calls it is about (a read with m mismatches has epsilon 8 - m).
The distinct items are few (Case.items, restated once); the sequence names them by index (RCase.sequence)."""
import collections
import functools
import itertools

import numpy as np

import score_cases as sc
import score_ref as ref
from graphtyper_amd import lib as gtx
from score_cases import FIRST, G, PAIRED, REVERSED, SECOND

GUARD = ref.SATURATION_GUARD  # 65 527
LIMIT = 0xFFFF
EPSILONS = (4, 5, 6, 7, 8)


class RCase(sc.Case):
    """a Case whose items are the distinct ones; seq: the item sequence as indices into them"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.seq, self._reads, self.scenarios = [], {}, {}

    def rd(self, site, alleles=(1,), eps=8, rev=False, good=True):
        """a whole read over one site with that epsilon (rev: the record lies in the reverse slot); not good: 9 mismatches in 150"""
        key = (site, tuple(alleles), eps, rev, good)
        if key not in self._reads:
            g = G(150, [(site, list(alleles))], mm=8 - eps if good else 9)
            self._reads[key] = self.read(G(0), g) if rev else self.read(g)
        return self._reads[key]

    def last(self):
        return len(self.item_rows) - 1

    def one(self, sample, site, eps, alleles=(1,), note=None):
        """a one-read item: one call of that epsilon -> its index"""
        self.single(self.rd(site, alleles, eps), sample=sample, note=note or ("call", eps))
        return self.last()

    def two(self, sample, site, e1, e2, alleles=(1,), which=1, flags="plain", good=(True, True), note=None):
        """a pair both of whose mates lie over the site: the calls e1 then e2 (the read that is first in the pair first).  which: the
        orientation pair that is selected (1: first mate forward, second reverse; 2: the other two records); flags "swapped": the
        item's first record is the second mate; "reversed": both records carry IS_SEQ_REVERSED (then the other orientation pair wins)"""
        m1, m2 = (e1, e2) if flags != "swapped" else (e2, e1)  # epsilons of the item's first and second record
        g1, g2 = (good[0], good[1]) if flags != "swapped" else (good[1], good[0])
        first_rev = (which == 2) != (flags != "plain")      # which slot of the item's first record is looked at
        a1, a2 = self.rd(site, alleles, m1, rev=first_rev, good=g1), self.rd(site, alleles, m2, rev=not first_rev, good=g2)
        f1, f2 = {"plain": (PAIRED | FIRST, PAIRED | SECOND), "swapped": (PAIRED | SECOND, PAIRED | FIRST),
                  "reversed": (PAIRED | FIRST | REVERSED, PAIRED | SECOND | REVERSED)}[flags]
        self.pair(a1, a2, flag1=f1, flag2=f2, sample=sample, note=note or ("pair", e1, e2))
        return self.last()

    def prefix(self, sample, site, level, alleles=(1,)):
        """items that bring the cell from 0 to `level`, every call accepted -> list of item indices"""
        r = level % 8
        smalls = [] if r == 0 else [r] if r >= 4 else [4, r + 4]
        rest = level - sum(smalls)
        assert rest % 8 == 0 and rest >= 0
        out = [self.one(sample, site, e, alleles, note=("prefix",)) for e in smalls]
        if rest // 16:
            out += [self.two(sample, site, 8, 8, alleles, note=("prefix",))] * (rest // 16)
        if rest % 16:
            out.append(self.one(sample, site, 8, alleles, note=("prefix",)))
        return out

    def finish(self):
        self.sequence = np.array(self.seq, np.int64)
        self.mult = np.bincount(self.sequence, minlength=len(self.item_rows))
        self.all_items = self.items[self.sequence]
        return self


TAIL_ALLELES = ((0,), (1,), (0, 1))


def tail(c, sample, site, epsilons, sets=TAIL_ALLELES):
    return [c.one(sample, site, e, sets[(j + e) % len(sets)], note=("tail", j, e)) for j, e in enumerate(epsilons)]


# ---- boundary ---------------------------------------------------------------------------------------------------------------------
BOUNDARY_LEVELS = range(65515, 65528)
THREE_AT = 65521


def boundary_scenarios():
    out = [("sum", s, ()) for s in (65526, 65527, 65528)]
    for level in BOUNDARY_LEVELS:
        for n in (1, 2):
            out += [("tail", level, t) for t in itertools.product(EPSILONS, repeat=n)]
    out += [("tail", THREE_AT, t) for t in itertools.product(EPSILONS, repeat=3)]
    return out


BOUNDARY_PARTS = 4  # (so that one launch -- and one run of the oracle -- stays at half a million items)


def make_boundary():
    scen = boundary_scenarios()
    out = []
    for part in range(BOUNDARY_PARTS):
        mine = scen[part::BOUNDARY_PARTS]
        c = RCase(n_samples=len(mine))
        for sample, (kind, level, t) in enumerate(mine):
            c.scenarios[sample] = (kind, level, t)
            c.seq += c.prefix(sample, 0, level) + tail(c, sample, 0, t)
        out.append(c.finish())
    return out


def walk(level, epsilons):
    """the guard by hand: -> (final level, which calls were accepted)"""
    took = []
    for e in epsilons:
        took.append(level < LIMIT - e)
        level += e if took[-1] else 0
    return level, took


def facts_boundary(cases, exp):
    nh = sc.facts().n_hap
    outcomes, finals, small_after_large = set(), set(), 0
    # 518 scenarios; an item adds at most 16 to a cell (two reads of epsilon 8), so a level of 65 515 and more takes 4 095 items at the
    # least: 518 x 4 095 = 2 121 210 is the floor for these scenarios, and the set stays within 4 items a scenario of it
    n_scenarios = sum(len(c.scenarios) for c in cases)
    assert n_scenarios == 3 + 13 * 30 + 125 == 518
    assert n_scenarios * 4095 <= sum(len(c.sequence) for c in cases) <= n_scenarios * 4099
    for c, s, r, sample, (kind, level, t) in ((c, s, r, k, v) for c, (s, r) in zip(cases, exp) for k, v in c.scenarios.items()):
        cell = sample * nh
        unguarded = s.hap_u32[cell * 4]
        assert unguarded == level + sum(t)
        assert (cell in r.marked) == (unguarded >= GUARD)
        final, took = walk(level, t)
        assert r.head[cell] == final
        if kind == "sum":
            assert (cell in r.marked) == (level >= 65527)
            if cell in r.marked:  # everything is accepted: the replayed row is the unordered one
                assert r.head[cell] == level and r.rows[cell] == [s.log_score[sample * sc.facts().total_tri + k] for k in range(3)]
            continue
        outcomes |= set(zip(t, took))
        small_after_large += any(not took[i] and took[j] and t[j] < t[i] for i in range(len(t)) for j in range(i + 1, len(t)))
        if cell in r.marked:
            finals.add(final)
    assert outcomes == {(e, a) for e in EPSILONS for a in (False, True)}
    assert small_after_large > 10 and finals == set(range(65527, 65535))
    assert sorted(level for c in cases for kind, level, t in c.scenarios.values() if kind == "sum") == [65526, 65527, 65528]


# ---- order_within_item ---------------------------------------------------------------------------------------------------------------
ORDER_LEVEL = 65523


def make_order_within_item():
    c = RCase(n_samples=40)
    sample = itertools.count()

    def scenario(name, build, want):
        k = next(sample)
        c.scenarios[k] = (name, want)
        c.seq += c.prefix(k, 0, ORDER_LEVEL) + build(k)

    for e1, e2, want in ((8, 4, 65531), (4, 8, 65527)):
        for which in (1, 2):
            for flags in ("plain", "swapped", "reversed"):
                scenario(("pair", e1, e2, which, flags), lambda k: [c.two(k, 0, e1, e2, (0,), which=which, flags=flags)], want)
        scenario(("singles", e1, e2), lambda k: [c.one(k, 0, e1, (0,)), c.one(k, 0, e2, (0,))], want)
        # only the second read is good: its call carries order 1 and stands alone; then the other epsilon as an item of its own
        scenario(("second_only", e1, e2), lambda k: [c.two(k, 0, 8, e1, (0,), good=(False, True)), c.one(k, 0, e2, (0,))], want)

        def leftover(k):
            c.leftover(c.rd(0, (0,), e1), sample=k, note=("leftover", e1))
            return [c.last(), c.one(k, 0, e2, (0,))]
        scenario(("leftover", e1, e2), leftover, want)

    def beside(k):  # a whole read whose path begins two positions in front of the site: not overlapping, epsilon 7; then epsilon 4
        o = sc.order(0)
        c.single(c.read(G(150, [(0, [0])], start=o - 2, end=o + 30)), sample=k, note=("beside",))
        return [c.last(), c.one(k, 0, 4, (0,))]
    scenario(("beside", 7, 4), beside, 65534)  # (with epsilon 8 the second call would be refused at 65 531)
    return [c.finish()]


def facts_order_within_item(cases, exp):
    (c,), ((s, r),) = cases, exp
    nh = sc.facts().n_hap
    seen = collections.Counter()
    by_cell = collections.defaultdict(list)
    for e in r.log:
        by_cell[e[1]].append(e)
    for sample, (name, want) in c.scenarios.items():
        cell = sample * nh
        assert cell in r.marked and s.hap_u32[cell * 4] == ORDER_LEVEL + name[1] + name[2] and r.head[cell] == want, name
        last_items = sorted({e[0] for e in by_cell[cell]})[-2:]
        if name[0] == "pair":
            # both calls belong to one item: nothing but the order field tells them apart, and the call of order 0 has epsilon e1
            two = [e for e in by_cell[cell] if e[0] == last_items[-1]]
            assert [(e[2], e[3]) for e in two] == [(0, name[1]), (1, name[2])], name
            note = s.items[c.sequence[last_items[-1]]]
            assert note["which"] == name[3] and note["kind"] == "pair"
            seen[name[3:]] += 1
        elif name[0] == "second_only":
            item = [e for e in by_cell[cell] if e[0] == last_items[0]]
            assert [(e[2], e[3]) for e in item] == [(1, name[1])] and not s.items[c.sequence[last_items[0]]]["reads"][0]["good"]
        elif name[0] == "leftover":
            assert s.items[c.sequence[last_items[0]]]["kind"] == "leftover"
        elif name[0] == "beside":
            site = s.items[c.sequence[last_items[0]]]["reads"][0]["sites"][0]
            assert not site["overlapping"] and site["eps"] == 7 and walk(ORDER_LEVEL, (8, 4))[0] == 65531
    assert set(seen) == {(w, f) for w in (1, 2) for f in ("plain", "swapped", "reversed")} and all(v == 2 for v in seen.values())
    assert walk(ORDER_LEVEL, (8, 4))[0] == 65531 and walk(ORDER_LEVEL, (4, 8))[0] == 65527


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
MASK_SITES = {1: 3, 2: 4, 20: 7, 21: 64}
MASK_LEVEL = 65521


def mask_sets(cnum):
    sets = [(0,), (cnum - 1,), (0, 1), tuple(range(cnum))]
    if cnum == 64:
        sets += [(31,), (32,), (31, 32), (63,)]
    return sets


def make_masks():
    scen = [(site, e) for site, cnum in MASK_SITES.items() for e in mask_sets(cnum)]
    c = RCase(n_samples=len(scen), rec_words=64)
    for sample, (site, e) in enumerate(scen):
        cnum = MASK_SITES[site]
        other = tuple(a for a in range(cnum) if a not in e)[:2] or (1,)
        c.scenarios[sample] = (site, e, other)
        # accepted (65 529), a refused call of another set, accepted (65 534)
        c.seq += c.prefix(sample, site, MASK_LEVEL, (1,)) + [c.one(sample, site, 8, e), c.one(sample, site, 7, other), c.one(sample, site, 5, e)]
    return [c.finish()]


def facts_masks(cases, exp):
    (c,), ((s, r),) = cases, exp
    f = sc.facts()
    assert [f.hap_cnum[h] for h in MASK_SITES] == list(MASK_SITES.values())
    bits = set()
    for sample, (site, e, other) in c.scenarios.items():
        cell = sample * f.n_hap + site
        assert cell in r.marked and r.head[cell] == 65534 and s.hap_u32[4 * cell] == MASK_LEVEL + 20
        masks = [x[4] for x in r.log if x[1] == cell][-3:]
        assert masks == [sum(1 << a for a in e), sum(1 << a for a in other), sum(1 << a for a in e)]
        bits |= {m for m in masks}
        # the refused call shows in the unordered row and not in the replayed one
        base = sample * f.total_tri + f.tri_off[site]
        unordered = [s.log_score[base + k] for k in range(len(r.rows[cell]))]
        assert unordered != r.rows[cell] and all(u >= v for u, v in zip(unordered, r.rows[cell]))
    assert {1 << 31, 1 << 32, (1 << 31) | (1 << 32), 1 << 63, (1 << 64) - 1, 1, 3} <= bits


# ---- many_cells ------------------------------------------------------------------------------------------------------------------------
MANY_SAMPLES = 3


def many_cells_plan():
    """cell -> ("marked", level, tail) / ("below", 65526) / ("small", sum)"""
    nh = sc.facts().n_hap
    last = MANY_SAMPLES * nh - 1
    plan = {}
    for k, cell in enumerate((0, nh, 31, 32, 33, 63, 64, last)):  # (0 and n_hap: one site in two samples; 31, 32, 33: three sites of one)
        plan[cell] = ("marked", 65516 + k, ((8, 4, 5), (7, 8, 4), (8, 8, 4, 6))[k % 3])
    for cell in (1, 30, 34, 62, 65, last - 1):
        plan[cell] = ("below", 65526)
    for cell in (2, 29, 35, 61, 66):
        plan[cell] = ("small", 20)
    return plan


def make_many_cells():
    c = RCase(n_samples=MANY_SAMPLES)
    nh = sc.facts().n_hap
    lanes = []
    for cell, what in sorted(many_cells_plan().items()):
        sample, site = divmod(cell, nh)
        if what[0] == "marked":
            lanes.append(c.prefix(sample, site, what[1]) + tail(c, sample, site, what[2], ((0,), (1,))))
        else:
            lanes.append(c.prefix(sample, site, what[1]))
    # the calls on all of them interleaved in item order: lane k's j-th item stands at a place that grows with j for every k
    places = sorted((j * (1.0 + 0.01 * k) / len(lane), k, j) for k, lane in enumerate(lanes) for j in range(len(lane)))
    c.seq = [lanes[k][j] for _, k, j in places]
    return [c.finish()]


def facts_many_cells(cases, exp):
    (c,), ((s, r),) = cases, exp
    plan = many_cells_plan()
    nh = sc.facts().n_hap
    assert nh == 26 and {0, 31, 32, 33, 63, 64, MANY_SAMPLES * nh - 1} <= {cell for cell, w in plan.items() if w[0] == "marked"}
    assert r.marked == {cell for cell, w in plan.items() if w[0] == "marked"} and not r.unsupported
    for cell, what in plan.items():
        if what[0] == "marked":
            assert r.head[cell] == walk(what[1], what[2])[0] and s.hap_u32[4 * cell] == what[1] + sum(what[2])
        else:
            assert r.head[cell] == s.hap_u32[4 * cell] == what[1] and cell not in r.rows
    # interleaved: between the first and the last call on a marked cell lie calls on every other one
    first = {cell: min(e[0] for e in r.log if e[1] == cell) for cell in r.marked}
    last = {cell: max(e[0] for e in r.log if e[1] == cell) for cell in r.marked}
    assert max(first.values()) < min(last.values())
    runs = sum(1 for a, b in zip(r.log, r.log[1:]) if a[1] != b[1])
    assert runs > 1000


# ---- tables_and_forms ----------------------------------------------------------------------------------------------------------------
def make_tables_and_forms():
    out = []
    # reads over 9 .. 16 sites on a cell at the guard: tables of more than SCORE_MAX_HAPS entries
    c = RCase(n_samples=2, rec_words=128)
    for sample in (0, 1):
        c.seq += c.prefix(sample, 3, 65500 + sample)
    for n in range(9, 17):
        sites = [(k, [1]) for k in range(n)]
        for sample, mm in ((0, n % 4), (1, (n + 1) % 4)):
            c.single(c.read(G(150, sites, mm=mm)), sample=sample, note=("sites", n))
            c.seq.append(c.last())
    c.pair(c.read(G(150, [(k, [1]) for k in range(9)])), c.read(G(0), G(150, [(k, [0]) for k in range(12)], mm=2)), sample=0, note=("sites", 9, 12))
    c.seq.append(c.last())
    c.leftover(c.read(G(150, [(k, [1]) for k in range(10)], mm=3)), sample=1, note=("sites", 10))
    c.seq.append(c.last())
    out.append(c.finish())
    # rec_words 16 (a record of up to three sites lies in its slot whole) with the first mate's forward record in d_compact, and
    # rec_words 8 likewise (a record in its slot has no room for a site: the sites come from a 9th .. word only with rec_words >= 9,
    # so at 8 words the reads with sites are the aligner's, in the arena: aligned_replay())
    c = RCase(n_samples=2, rec_words=16)
    plain = c.read(G(150), compact=True)
    for sample, level in ((0, 65517), (1, 65519)):
        e = level % 8
        c.single(c.read(G(150, [(0, [1]), (1, [2])], mm=8 - e)), sample=sample, note=("prefix",))
        c.seq.append(c.last())
        c.pair(plain, c.read(G(0), G(150, [(0, [1])])), sample=sample, note=("compact_prefix",))
        c.seq += [c.last()] * ((level - e) // 8)
        for mm, alleles in ((3, [1]), (0, [0]), (1, [0, 1]), (4, [1])):
            c.pair(plain, c.read(G(0), G(150, [(0, alleles), (2, [3])], mm=mm)), sample=sample, note=("compact_tail", 8 - mm))
            c.seq.append(c.last())
            c.single(c.read(G(100), G(150, [(0, alleles)], mm=mm), compact=True), sample=sample, note=("compact_tail", 8 - mm))
            c.seq.append(c.last())
    out.append(c.finish())
    return out


def facts_tables_and_forms(cases, exp):
    big, forms = cases
    (s, r), (s2, r2) = exp
    nh = sc.facts().n_hap
    assert r.marked == {3, nh + 3}
    assert {len(it["reads"][0]["sites"]) for it, n in zip(s.items, big.notes) if n[0] == "sites" and len(n) == 2} == set(range(9, 17))
    for cell in r.marked:
        took = r.head[cell]
        assert GUARD <= took < s.hap_u32[4 * cell], "a call has to be refused"
    assert forms.compact_reads and forms.rec_words == 16 and r2.marked == {0, nh}
    for cell in r2.marked:
        assert GUARD <= r2.head[cell] < s2.hap_u32[4 * cell]
    plain, dense = sc.restate(forms), sc.restate(forms, compact=True)
    assert all(plain.dense(a) == dense.dense(a) for a in ref.Sums.ARRAYS)


# ---- log_growth --------------------------------------------------------------------------------------------------------------------
LOG_FIRST_CAP = 1 << 20  # replay_collect's first log block
GROWTH_SITES = 16


def make_log_growth(n_items=(LOG_FIRST_CAP // GROWTH_SITES, LOG_FIRST_CAP // GROWTH_SITES + 1)):
    """one sample, reads over 16 sites each: n items make 16 n log entries"""
    out = []
    for n in n_items:
        c = RCase(n_samples=1, rec_words=64)
        kinds = []
        for k, mm in enumerate((0, 1, 2, 4, 0)):
            c.single(c.read(G(150, [(h, [(h + k) % 2]) for h in range(GROWTH_SITES)], mm=mm)), sample=0, note=("sixteen", 8 - mm))
            kinds.append(c.last())
        i = np.arange(n)
        c.seq = list(np.array(kinds)[(i * 7 + i // 1000) % 5])
        out.append(c.finish())
    return out


def facts_log_growth(cases, exp):
    for c, (s, r), n in zip(cases, exp, (65536, 65537)):
        assert len(c.sequence) == n and len(r.log) == 16 * n and len(r.marked) == 16
        assert all(GUARD <= r.head[cell] < LIMIT for cell in r.marked)
    assert len(exp[0][1].log) == LOG_FIRST_CAP and len(exp[1][1].log) == LOG_FIRST_CAP + 16


# ---- halves ------------------------------------------------------------------------------------------------------------------------
def make_halves():
    """the item orders of many_cells at a size whose cuts are cheap: five cells of two samples, interleaved"""
    c = RCase(n_samples=2)
    lanes = []
    for k, (sample, site) in enumerate(((0, 0), (0, 5), (1, 0), (1, 7), (1, 12))):
        lanes.append(c.prefix(sample, site, 65517 + k) + tail(c, sample, site, ((8, 5, 4), (6, 8, 7, 4))[k % 2]))
    lanes.append(c.prefix(1, 9, 65526))
    places = sorted((j * (1.0 + 0.01 * k) / len(lane), k, j) for k, lane in enumerate(lanes) for j in range(len(lane)))
    c.seq = [lanes[k][j] for _, k, j in places]
    return [c.finish()]


def facts_halves(cases, exp):
    (c,), ((s, r),) = cases, exp
    assert len(r.marked) == 5 and len(r.log) > 20000
    cut = len(c.sequence) * 2 // 5
    assert 0 < sum(e[0] < cut for e in r.log) < len(r.log)
    assert any(r.head[cell] < s.hap_u32[4 * cell] for cell in r.marked)


# ---- records only the aligner can make: in the arena (rec_words 8), and with wide allele sets ---------------------------------------
def _single_items(reads, n_samples):
    a = np.zeros(len(reads) * n_samples, gtx.SCORE_ITEM)
    a["first"]["align_index"] = np.repeat(np.array(reads, np.uint32), n_samples)
    a["first"]["mapq"] = 60
    a["second"]["align_index"] = ref.INVALID
    a["sample"] = np.tile(np.arange(n_samples, dtype=np.uint32), len(reads))
    return a


def _restate_aligned(a, mult=None):
    return ref.score(a.facts, a.par, a.records, a.rec_words, a.items, a.n_samples, multiplicity=mult, big_records=a.big)


def _calls_of(note):
    return [(x["site"], x["eps"], x["explains"]) for r in note["reads"] for x in r["sites"]]


def aligned_replay(Backend):
    """score_cases.aligned_records(Backend) -> [external, wide] with item orders that bring cells to the guard:
    external: one read of sample 0 (its record in the arena) again and again up to just under the guard, then every item three times;
    wide: the same on a read of sample 0 that lies on sites of at most 64 alleles (its cells are replayed, by the wide kernel), a read
    of sample 1 over the 100-allele site until that cell stands at the guard (unsupported: the one cell the library leaves as it
    is), then every item twice."""
    ext, wide = sc.aligned_records(Backend)
    for a in (ext, wide):
        reads = sorted({int(x) for x in a.items["first"]["align_index"]})
        a.items = np.concatenate([a.items, _single_items(reads, a.n_samples)])
        a.first_single = len(a.items) - len(reads) * a.n_samples
        a.notes = [("aligned",)] * len(a.items)
        once = _restate_aligned(a)
        singles = [(d, _calls_of(once.items[d])) for d in range(a.first_single, len(a.items))]
        seq = []
        if a is ext:
            d0, calls = next((d, c) for d, c in singles if a.items["sample"][d] == 0 and len(c) >= 2)
            seq += [d0] * (65519 // max(e for _, e, _ in calls))
        else:
            big = max(range(a.facts.n_hap), key=lambda h: a.facts.hap_cnum[h])
            d0, calls = next((d, c) for d, c in singles if a.items["sample"][d] == 0 and c and all(a.facts.hap_cnum[h] <= 64 for h, _, _ in c))
            seq += [d0] * (65519 // max(e for _, e, _ in calls))
            d1, calls1 = min(((d, c) for d, c in singles if a.items["sample"][d] == 1 and any(h == big for h, _, _ in c)),
                             key=lambda dc: max(len(x) for h, _, x in dc[1] if h == big))
            seq += [d1] * (65540 // min(e for h, e, _ in calls1 if h == big) + 1)
            a.big_site, a.big_cell = big, a.facts.n_hap + big
        a.prefix_len = len(seq)
        seq += list(range(len(a.items))) * (3 if a is ext else 2)
        a.sequence = np.array(seq, np.int64)
        a.mult = np.bincount(a.sequence, minlength=len(a.items))
        a.all_items = a.items[a.sequence]
    return [ext, wide]


def expected_aligned(sets):
    out = []
    for a in sets:
        s = _restate_aligned(a, a.mult)
        out.append((s, ref.replay(s, a.sequence.tolist())))
    return out


def facts_aligned(sets, exp):
    ext, wide = sets
    (s, r), (sw, rw) = exp
    words = ext.records.reshape(-1, 8)
    touched = {int(ext.all_items["first"]["align_index"][e[0]]) for e in r.log}
    assert ext.rec_words == 8 and r.marked and not r.unsupported and any((int(words[2 * x, 0]) >> 16) & ref.ST_EXTERNAL for x in touched)
    for a, (s_, r_) in zip(sets, exp):
        assert any(r_.head[cell] < s_.hap_u32[4 * cell] for cell in r_.marked), "a call has to be refused"
        assert any(e[0] >= a.prefix_len for e in r_.log) and {note["kind"] for note in s_.items} == {"single", "pair", "leftover"}
    assert wide.facts.hap_cnum[wide.big_site] == 100 and rw.unsupported == {wide.big_cell} and len(rw.marked) >= 1
    assert any(wide.facts.hap_cnum[cell] == 2 for cell in rw.marked if cell < wide.facts.n_hap), "a SNP's cell of sample 0 at the guard"
    head, row = rw.beyond[wide.big_cell]
    assert GUARD <= head < sw.hap_u32[4 * wide.big_cell] and len(row) == 5050


def reference_arrays_wide(wide, acc, rw):
    """`acc` with the one cell the library leaves unreplayed set to what the reference has there: the rest of the arrays can then be
    compared with the oracle as a whole"""
    f = wide.facts
    head, row = rw.beyond[wide.big_cell]
    sample, site = divmod(wide.big_cell, f.n_hap)
    acc.hap_u32[4 * wide.big_cell] = head | 0x80000000
    base = sample * f.total_tri + f.tri_off[site]
    acc.log_score[base:base + len(row)] = row
    return acc


# ---- a marked cell that no item of the replay touches -------------------------------------------------------------------------------
UNTOUCHED = (1, 7)  # (sample, site) of `halves`: at the guard, and left without a call


def without_cell(case, s, cell):
    """the places of the sequence whose item makes no call on `cell`: every other cell keeps all its calls, in their order"""
    nh = sc.facts_of(case).n_hap
    touches = np.array([any(note["sample"] * nh + x["site"] == cell for r_ in note["reads"] for x in r_["sites"]) for note in s.items])
    keep = np.nonzero(~touches[case.sequence])[0]
    assert 0 < len(keep) < len(case.sequence)
    return keep


def untouched_case():
    """-> (case, s, r, cell, the places kept, r without that cell: what a replay over the kept items has to leave)"""
    (case,), ((s, r),) = cases("halves"), expected("halves")
    cell = UNTOUCHED[0] * sc.facts().n_hap + UNTOUCHED[1]
    assert cell in r.marked and len(r.marked) > 1
    keep = without_cell(case, s, cell)
    head = dict(r.head)
    head[cell] = s.hap_u32[4 * cell]
    partial = r._replace(head=head, rows={c: row for c, row in r.rows.items() if c != cell}, marked=r.marked - {cell},
                         log=[e for e in r.log if e[1] != cell])
    # the other cells' calls are all among the kept items, in their order: the walk over the kept items alone gives the same
    again = ref.replay(s, case.sequence[keep].tolist())
    assert all(again.rows[c] == partial.rows[c] and again.head[c] == partial.head[c] for c in partial.rows) and not any(e[1] == cell for e in again.log)
    return case, s, r, cell, keep, partial


def finalize_count(acc):
    """what gtx_scores_finalize reports of a copy of the arrays: the cells at the guard that carry no mark"""
    import ctypes as C
    import harness
    ls, cov, hap = acc.log_score.copy(), acc.gt_cov.copy(), acc.hap_u32.copy()
    n = C.c_uint64()
    gtx.check(gtx.lib().gtx_scores_finalize(harness._p(ls), len(ls), harness._p(cov), len(cov), harness._p(hap), len(hap) // 4, C.byref(n)))
    return int(n.value)


MAKERS = dict(boundary=make_boundary, order_within_item=make_order_within_item, masks=make_masks, many_cells=make_many_cells,
              tables_and_forms=make_tables_and_forms, log_growth=make_log_growth, halves=make_halves)
FACTS = dict(boundary=facts_boundary, order_within_item=facts_order_within_item, masks=facts_masks, many_cells=facts_many_cells,
             tables_and_forms=facts_tables_and_forms, log_growth=facts_log_growth, halves=facts_halves)
FACTS_ALIGNED = facts_aligned
SETS = sorted(MAKERS)
N_CASES = dict(boundary=BOUNDARY_PARTS, order_within_item=1, masks=1, many_cells=1, tables_and_forms=2, log_growth=2, halves=1)
CASE_IDS = [(name, k) for name in SETS for k in range(N_CASES[name])]


@functools.lru_cache(maxsize=None)
def cases(name):
    return MAKERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """per case: (the unguarded sums of score_ref.score, what score_ref.replay makes of them)"""
    out = []
    for c in cases(name):
        s = sc.restate(c)
        out.append((s, ref.replay(s, c.sequence.tolist())))
    return out


# ---- arrays ------------------------------------------------------------------------------------------------------------------------
def overlay(case, acc, r, mark=True):
    """the replayed heads (with the mark) and rows of `r` put into the arrays of a harness.Accumulators that hold the unguarded sums"""
    f = sc.facts_of(case)
    for cell, row in r.rows.items():
        sample, site = divmod(cell, f.n_hap)
        acc.hap_u32[4 * cell] = r.head[cell] | (0x80000000 if mark else 0)
        base = sample * f.total_tri + f.tri_off[site]
        acc.log_score[base:base + len(row)] = row
    return acc


def conn_cap_of(s):
    return sum(s.conn_log.values()) + 16


def expected_arrays(case, s, r):
    """what a block holds after gtx_score_batch and gtx_scores_replay"""
    return overlay(case, sc.dense_arrays(case, s, conn_cap=conn_cap_of(s)), r)


def log_tuples(entries):
    """gtx.REPLAY_ENTRY array -> sorted list of (item, cell, order, epsilon, mask)"""
    e = np.asarray(entries)
    assert not e["pad"].any()
    return sorted(zip(e["item"].tolist(), e["cell"].tolist(), (e["order_eps"] >> 8).tolist(), (e["order_eps"] & 0xFF).tolist(),
                      (e["mask_lo"].astype(np.uint64) | (e["mask_hi"].astype(np.uint64) << np.uint64(32))).tolist()))


@functools.lru_cache(maxsize=None)
def oracle_of(name, k):
    """the oracle's two streams of one hand-made case"""
    case = cases(name)[k]
    return oracle_streams(case, case.all_items)


def oracle_streams(case, items):
    """(gto_scores_dump, gto_calls_dump) of an oracle genotyper given the items one by one, in order, through its guarded explain_to_score"""
    from oracle_lib import Oracle
    ref_s, recs, rb, add_all = case.graph_inputs if isinstance(case, sc.Aligned) else sc.graph_inputs() + (False,)
    og = Oracle(ref_s, recs, region_begin=rb, is_sv_graph=case.par.is_sv_graph, hq_reads=case.par.hq_reads, add_all_variants=add_all).genotyper(case.n_samples, 1)
    og.push_paths(items, case.records, case.rec_words, big_records=getattr(case, "big", None), is_segment_calling=case.par.is_segment_calling)
    return og.scores(), og.calls()


# ---- tests/emu_replay -----------------------------------------------------------------------------------------------------------------
def _replay_tail(raw):
    head = raw[:20].view(np.uint32)
    entries = raw[20:].view(gtx.REPLAY_ENTRY)
    assert len(entries) == int(head[2])
    return dict(n_replayed=int(head[0]), n_unsupported=int(head[1]), passes=int(head[3]), again=int(head[4]), entries=entries.copy())


def through_replay(run, case, s, items=None, log_cap=1 << 20, compact=None):
    """a case through tests/emu_replay; run(write, read): emu_programs.run with the program and a directory -> score_cases.Got whose
    arrays are those after the replay and whose `more` holds the counts and the log"""
    cap = conn_cap_of(s)
    items = case.all_items if items is None else items
    return run(lambda path: sc.write_case(path, case, items, cap, compact, log_cap=log_cap), lambda path: sc.read_result(path, case, cap, more=_replay_tail))


def replay_differences(case, s, r, got, passes=None):
    """where what tests/emu_replay wrote differs from the restatement -> list, at most a few"""
    out = []
    want = expected_arrays(case, s, r)
    m = got.more
    if (m["n_replayed"], m["n_unsupported"], m["again"]) != (len(r.marked), len(r.unsupported), 0) or got.errors:
        out.append(("counts", m["n_replayed"], m["n_unsupported"], m["again"], got.errors))
    if passes is not None and m["passes"] != passes:
        out.append(("passes", m["passes"], passes))
    if log_tuples(m["entries"]) != sorted(r.log):
        out.append(("log", len(m["entries"]), len(r.log)))
    for name in ("log_score", "gt_cov", "hap_u32", "stat_u64", "stat_u32", "conn_near"):
        g, w = getattr(got, name), getattr(want, name)
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0] if len(g) == len(w) else [-1]
        out += [(name, int(i), int(g[i]), int(w[i])) for i in bad[:3]]
    if int(got.conn_count[0]) != sum(s.conn_log.values()) or int(got.conn_count[1]):
        out.append(("conn_count", tuple(int(x) for x in got.conn_count)))
    return out


SANITIZED_GROWTH = (12288, 12289)  # log_growth at a size the sanitizers take in a second: the first log block is full, or 16 short
SANITIZED_GROWTH_CAP = GROWTH_SITES * SANITIZED_GROWTH[0]


@functools.lru_cache(maxsize=None)
def sanitized_log_growth():
    cs = make_log_growth(SANITIZED_GROWTH)
    out = []
    for c in cs:
        s = sc.restate(c)
        out.append((c, s, ref.replay(s, c.sequence.tolist())))
    return out


def judge(name, run):
    """None when the program behind `run` gives the set `name` as the restatement does, else how it differs"""
    if name == "log_growth":
        for (c, s, r), passes in zip(sanitized_log_growth(), (1, 2)):
            if replay_differences(c, s, r, through_replay(run, c, s, log_cap=SANITIZED_GROWTH_CAP), passes):
                return "differs from the restatement (%d passes)" % passes
        return None
    if name == "aligned_records":
        sets = aligned_on_the_emulation()
        for a, (s, r) in zip(*sets):
            if replay_differences(a, s, r, through_replay(run, a, s)):
                return "differs from the restatement (%s)" % a.name
        return None
    for k, (case, (s, r)) in enumerate(zip(cases(name), expected(name))):
        for compact in ((True, False) if case.compact_reads else (None,)):
            n_log = len(r.log)
            for log_cap in ((1 << 20,) if name != "halves" else (n_log, n_log - 1, 0)):
                if replay_differences(case, s, r, through_replay(run, case, s, log_cap=log_cap, compact=compact), None if name != "halves" else 1 + (log_cap < n_log)):
                    return "differs from the restatement (case %d)" % k
    return None


@functools.lru_cache(maxsize=None)
def aligned_on_the_emulation():
    import harness
    sets = aligned_replay(harness.EmuBackend)
    return sets, expected_aligned(sets)


AUDITED = SETS + ["aligned_records"]
