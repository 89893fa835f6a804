"""Hand-made accumulators for the call stage (gtx_calls_batch -> gtx_calls_kernel -> call_cell, graphtyper_amd/csrc/score_core.hpp):
the case sets, what the restatement (tests/calls_ref.py) expects of each, a fact test per set that proves from those expectations
that the set reaches what it is for, the same state put into an oracle genotyper (OracleGenotyper.set_hap_samples), and the case
files of the stand-alone program tests/emu_calls.  All values are integers and every comparison is exact.

The graphs (gtx.graph_from_records; a haplotype is a site, its shape the number of alleles):
  bi         one bi-allelic SNP (n_hap 1): a row of the table is a sample
  shapes     sites of 2, 3, 4 and 7 alleles (n_hap 4)
  layout255  2, 3, 4, 7, 2 alleles (n_hap 5)      layout513  2, 3, 4, 7, 2, 2, 3, 4, 7 alleles (n_hap 9)
  layout257  257 sites that cycle through 2, 3, 4, 7 alleles: 257 is prime, so 257 cells are 257 haplotypes of one sample
  wide       scenarios.wide_site_case: a site of 100 alleles, one of more than 1000, SNPs
No row holds a log score of 0x10000 or more: that is outside what the reference can hold (gtx_scores_replay comes first)."""
import functools
import itertools
import struct

import numpy as np

import calls_ref as ref
import harness
import scenarios
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth
from oracle_lib import Oracle

RB = 40000
SHAPES = {"bi": [2], "shapes": [2, 3, 4, 7], "layout255": [2, 3, 4, 7, 2], "layout513": [2, 3, 4, 7, 2, 2, 3, 4, 7],
          "layout257": [(2, 3, 4, 7)[k % 4] for k in range(257)]}
DELTAS = list(range(91)) + [254, 255, 256, 1000, 65534]          # pl_deltas: d and e of a row (mx, mx - d, mx - e)
COV_EDGES = [0, 1, 0xFFFE, 0xFFFF, 0x10000, 0xFFFFFFFF]          # a gt_cov word
U8_EDGES = [0, 1, 254, 255, 256, 0xFFFFFFFF]                     # hap_u32[1..3]
MARKS = [0, 0x80000000 | 0x1234, 0xFFFFFFFF]                     # hap_u32[0]: max_log_score, bit 31 = the replay mark
MAX_SCORE = 0xFFFE


# ---- graphs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_inputs(key):
    """(reference string, records, region begin, add_all_variants)"""
    if key == "wide":
        ref_s, recs, _, _, _ = scenarios.wide_site_case(region_begin=20000)
        return ref_s, recs, 20000, True
    shapes = SHAPES[key]
    rng = np.random.default_rng(1000 + len(shapes))
    bases = synth.make_reference(80 + 40 * len(shapes), seed=900 + len(shapes))
    recs = []
    for k, cnum in enumerate(shapes):
        p = 40 + 40 * k
        b = int(bases[p])
        if cnum <= 4:
            alts = ["ACGT"[(b + j) % 4] for j in range(1, cnum)]
        else:  # insertions behind the base, as scenarios.wide_site_case makes its 100 alleles
            alts = []
            while len(alts) < cnum - 1:
                s = "ACGT"[b] + synth.bases_to_str(rng.integers(0, 4, size=int(rng.integers(5, 9)), dtype=np.uint8))
                if s not in alts:
                    alts.append(s)
        recs.append((p + RB, "ACGT"[b], alts, None))
    return synth.bases_to_str(bases), recs, RB, False


@functools.lru_cache(maxsize=None)
def graph(key):
    ref_s, recs, rb, add_all = graph_inputs(key)
    return gtx.graph_from_records(ref_s, recs, region_begin=rb, add_all_variants=add_all)


@functools.lru_cache(maxsize=None)
def host_ctx(key):
    """a context without a device: the layout tables"""
    ctx = gtx.Context(graph(key), device=-1)
    if key in SHAPES:
        assert ctx.hap_cnum.tolist() == SHAPES[key], (key, ctx.hap_cnum)
    else:
        cnum = np.sort(ctx.hap_cnum)
        assert cnum[-2] == 100 and cnum[-1] > 1000
    return ctx


@functools.lru_cache(maxsize=None)
def layout(key):
    return layout_of(host_ctx(key))


def layout_of(c):
    """the layout tables of a context as plain Python values"""
    return dict(hap_cnum=[int(x) for x in c.hap_cnum], tri_off=[int(x) for x in c.tri_off], allele_off=[int(x) for x in c.allele_off],
                n_hap=c.n_hap, total_tri=c.total_tri, total_allele=c.total_allele)


def n_tri(cnum):
    return cnum * (cnum + 1) // 2


def xy_of(i):
    """(x, y) of the i-th genotype, y outermost"""
    y = 0
    while i > y:
        i -= y + 1
        y += 1
    return i, y


# ---- a case: one graph, n_samples, the three raw arrays ------------------------------------------------------------------
class Case:
    def __init__(self, key, n_samples):
        self.key, self.n_samples, self.lay = key, n_samples, layout(key)
        L = self.lay
        self.log_score = np.zeros(n_samples * L["total_tri"], np.uint32)
        self.gt_cov = np.zeros(n_samples * L["total_allele"], np.uint32)
        self.hap_u32 = np.zeros(n_samples * L["n_hap"] * 4, np.uint32)
        self.notes = {}  # (sample, hap) -> what the cell is there for (read by the fact tests)

    def cells(self):
        return self.n_samples * self.lay["n_hap"]

    def put(self, s, h, scores=None, cov=None, cu=None, note=None):
        L = self.lay
        cnum = L["hap_cnum"][h]
        if scores is not None:
            assert len(scores) == n_tri(cnum) and max(scores) < 0x10000
            t = s * L["total_tri"] + L["tri_off"][h]
            self.log_score[t:t + len(scores)] = scores
        if cov is not None:
            assert len(cov) == cnum
            a = s * L["total_allele"] + L["allele_off"][h]
            self.gt_cov[a:a + cnum] = cov
        if cu is not None:
            assert len(cu) == 4 and cu[2] <= cu[1]  # raw ambiguous_alt <= ambiguous: a read that counts for the second counts for the first
            self.hap_u32[(s * L["n_hap"] + h) * 4:(s * L["n_hap"] + h) * 4 + 4] = cu
        if note is not None:
            self.notes[(s, h)] = note

    def row(self, s, h):
        """(scores, cov, cu) of a cell as lists"""
        L = self.lay
        cnum = L["hap_cnum"][h]
        t = s * L["total_tri"] + L["tri_off"][h]
        a = s * L["total_allele"] + L["allele_off"][h]
        c = (s * L["n_hap"] + h) * 4
        return self.log_score[t:t + n_tri(cnum)].tolist(), self.gt_cov[a:a + cnum].tolist(), self.hap_u32[c:c + 4].tolist()


def from_rows(key, rows_by_hap):
    """rows_by_hap[h]: list of dict(scores=, cov=, cu=, note=); cell (s, h) takes row s of its haplotype, and once those are used up
    goes round again without a note"""
    case = Case(key, max(len(r) for r in rows_by_hap))
    for h, rows in enumerate(rows_by_hap):
        for s in range(case.n_samples):
            r = dict(rows[s % len(rows)])
            if s >= len(rows):
                r.pop("note", None)
            case.put(s, h, **r)
    return case


def plain_scores(cnum, top=0, mx=5000):
    """a row without ties: the maximum at genotype `top`"""
    return [mx if i == top else mx - 10 - 3 * i for i in range(n_tri(cnum))]


# ---- the sets --------------------------------------------------------------------------------------------------------------
def pl_delta_rows():
    rows = set()
    for d, e in itertools.product(DELTAS, DELTAS):
        for mx in (max(d, e), MAX_SCORE):
            rows.update(itertools.permutations((mx, mx - d, mx - e)))
    return sorted(rows)


def make_pl_deltas():
    rows = pl_delta_rows()
    case = Case("bi", len(rows))
    case.log_score[:] = np.array(rows, np.uint32).reshape(-1)  # (n_hap 1, three genotypes: a row of the table is a sample's row)
    case.gt_cov[:] = np.arange(2 * len(rows)) % 7
    return [case]


def make_ties():
    rows_by_hap = []
    for cnum in SHAPES["shapes"]:
        n = n_tri(cnum)
        rows = [dict(scores=[0] * n, note=("equal", 0)), dict(scores=[MAX_SCORE] * n, note=("equal", MAX_SCORE))]
        for p in range(n):
            rows.append(dict(scores=[5000 if i == p else 5000 - 1 - (7 * i + p) % 40 for i in range(n)], note=("single", p)))
        for p, q in itertools.combinations(range(n), 2):
            mx = MAX_SCORE if (p + q) % 2 else 300
            rows.append(dict(scores=[mx if i in (p, q) else mx - 1 - (5 * i + q) % 60 for i in range(n)], note=("pair", p, q)))
        rows_by_hap.append(rows)
    return [from_rows("shapes", rows_by_hap)]


def make_gq():
    rows_by_hap = []
    for cnum in SHAPES["shapes"]:
        n = n_tri(cnum)
        rows = []
        for z in range(n):  # one zero, every other PL 255
            rows.append(dict(scores=[3000 if i == z else 3000 - 85 - 11 * i for i in range(n)], note=("only_255", z)))
            for q in range(n):
                if q != z:
                    for delta in (1, 84, 85):  # the next-lowest PL (3, 253, 255) in front of and behind the zero
                        rows.append(dict(scores=[3000 if i == z else 3000 - delta if i == q else 2000 - i for i in range(n)], note=("next", z, q, delta)))
        rows_by_hap.append(rows)
    return [from_rows("shapes", rows_by_hap)]


def make_depth_clamps():
    counters = [(a, b, p) for a in U8_EDGES for b in U8_EDGES if b <= a for p in U8_EDGES]
    rows_by_hap = [[] for _ in SHAPES["shapes"]]
    k = 0
    for c0, c1 in itertools.product(COV_EDGES, COV_EDGES):  # bi-allelic: every word x every counter
        for a, b, p in counters:
            rows_by_hap[0].append(dict(cov=[c0, c1], cu=[MARKS[k % 3], a, b, p]))
            k += 1
    rows_by_hap[0] += [dict(cov=[0xFFFF, 1], cu=[0, 255, 0, 0], note=("ref_clamps",)),
                       dict(cov=[0, 3], cu=[0, 300, 280, 0], note=("ref_zero",)),  # both stop at 255: the difference is 0, not 20
                       dict(cov=[5, 3], cu=[0, 300, 256, 300], note=("ref_is_cov0", 5)),
                       dict(cov=[0xFFFE, 0], cu=[0, 1, 0, 0], note=("ref_reaches", 0xFFFF)),
                       dict(cov=[0, 0xFFFE], cu=[0, 2, 2, 0], note=("alt_clamps",))]
    for m, mark in enumerate(MARKS):  # hap_u32[0] changes nothing: three cells that differ in it alone
        rows_by_hap[0].append(dict(cov=[17, 0x10003], cu=[mark, 256, 3, 254], note=("mark", m)))
    for h in (1, 2):  # 3 and 4 alleles: every combination of words, the counters going round
        for j, cov in enumerate(itertools.product(COV_EDGES, repeat=SHAPES["shapes"][h])):
            a, b, p = counters[(5 * j + h) % len(counters)]
            rows_by_hap[h].append(dict(cov=list(cov), cu=[MARKS[j % 3], a, b, p]))
    rng = np.random.default_rng(77)
    rows_by_hap[3].append(dict(cov=[0xFFFF] * 7, cu=[0, 0, 0, 0], note=("alt_clamps",)))
    rows_by_hap[3].append(dict(cov=[1, 0xFFFFFFFF, 0x10000, 0xFFFFFFFF, 0x10000, 0xFFFF, 0xFFFFFFFF], cu=[0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], note=("alt_clamps",)))
    rows_by_hap[3].append(dict(cov=[0, 10000, 10000, 10000, 10000, 10000, 15535], cu=[0, 0, 0, 0], note=("alt_reaches", 0xFFFF)))
    rows_by_hap[3].append(dict(cov=[0, 10000, 10000, 10000, 10000, 10000, 15280], cu=[0, 254, 0, 0], note=("alt_reaches", 0xFFFE)))
    for j in range(2000):
        a, b, p = counters[int(rng.integers(len(counters)))]
        rows_by_hap[3].append(dict(cov=[COV_EDGES[int(x)] for x in rng.integers(0, 6, size=7)], cu=[MARKS[j % 3], a, b, p]))
    for h, cnum in enumerate(SHAPES["shapes"]):
        for r in rows_by_hap[h]:
            r["scores"] = plain_scores(cnum, top=1)
    return [from_rows("shapes", rows_by_hap)]


def random_cell(rng, cnum, edges):
    """edges False: a row with one maximum, words and counters that stay below every clamp, sums included (a clamp would hide a word
    read from the neighbour's row), all of them different from cell to cell; True: values from the edge lists as often as uniform ones"""
    n = n_tri(cnum)
    if not edges:
        mx = int(rng.integers(100, MAX_SCORE))
        scores = (mx - rng.integers(1, 84, size=n)).tolist()  # (below the PL cap: every delta has a PL of its own)
        scores[int(rng.integers(n))] = mx
        amb = int(rng.integers(2, 250))
        return dict(scores=scores, cov=rng.integers(1, 9000, size=cnum).tolist(),
                    cu=[MARKS[int(rng.integers(3))], amb, int(rng.integers(0, amb - 1)), int(rng.integers(0, 250))])
    mx = int(rng.choice([0, 1, 84, 85, 86, 255, 1000, MAX_SCORE, int(rng.integers(0, MAX_SCORE + 1))]))
    scores = [max(0, mx - int(rng.choice(DELTAS))) if rng.random() < 0.5 else int(rng.integers(0, mx + 1)) for _ in range(n)]
    if rng.random() < 0.9:
        scores[int(rng.integers(n))] = mx
    word = lambda lst: int(rng.choice(lst)) if rng.random() < 0.5 else int(rng.integers(0, 1 << 32))  # noqa: E731
    amb, alt = sorted((word(U8_EDGES), word(U8_EDGES)), reverse=True)
    return dict(scores=scores, cov=[word(COV_EDGES) for _ in range(cnum)], cu=[word(MARKS), amb, alt, word(U8_EDGES)])


def random_case(key, n_samples, seed, edges, skip=()):
    rng = np.random.default_rng(seed)
    case = Case(key, n_samples)
    for s in range(n_samples):
        for h, cnum in enumerate(case.lay["hap_cnum"]):
            if h not in skip:
                case.put(s, h, **random_cell(rng, cnum, edges))
    return case


LAYOUT_CELLS = {"layout255": 255, "shapes": 256, "layout257": 257, "layout513": 513}  # cells against a grid of (cells + 255) / 256 blocks


def make_layout():
    return [random_case(key, cells // len(SHAPES[key]), 300 + cells, False) for key, cells in LAYOUT_CELLS.items()]


def make_random():
    return [random_case("layout513", 300, 11, True), random_case("shapes", 129, 12, True)]


MANY_CELLS_SAMPLES = 4445          # x 9 haplotypes = 40 005 cells: 157 blocks of 256, the last one with 69 cells
MANY_CELLS_SAMPLES_SANITIZED = 228  # x 9 = 2 052 cells: what runs through tests/emu_calls under the sanitizers


def make_many_cells(n_samples=MANY_CELLS_SAMPLES):
    return [random_case("layout513", n_samples, 13, False)]


def make_wide():
    L = layout("wide")
    h100 = L["hap_cnum"].index(100)
    hbig = max(range(L["n_hap"]), key=lambda h: L["hap_cnum"][h])
    rng = np.random.default_rng(21)
    cases = []
    for k in range(2):
        case = random_case("wide", 2, 30 + k, True, skip=(h100, hbig))  # (the SNPs; the two wide sites follow)
        for h in (h100, hbig):
            cnum = L["hap_cnum"][h]
            n = n_tri(cnum)
            low = (np.arange(n) * 7 + h) % 300 + 1
            if k == 0:  # the maximum on the last genotype, and on the first
                for s, top in ((0, n - 1), (1, 0)):
                    scores = 40000 - low
                    scores[top] = 40000
                    case.put(s, h, scores=scores.tolist(), cov=((np.arange(cnum) * 37) % 900).tolist(), cu=[0, 9, 4, 7], note=("single", top))
            else:  # two maxima far apart; seeded random rows
                p, q = n // 7, n - 5
                scores = MAX_SCORE - low
                scores[[p, q]] = MAX_SCORE
                case.put(0, h, scores=scores.tolist(), cov=[0xFFFF] * cnum, cu=[MARKS[1], 255, 255, 0], note=("pair", p, q))
                scores = rng.integers(0, MAX_SCORE, size=n) if h == h100 else 20000 - rng.integers(1, 120, size=n)
                top = int(rng.integers(n))
                scores[top] = MAX_SCORE if h == h100 else 20000
                case.put(1, h, scores=scores.tolist(), cov=rng.integers(0, 200, size=cnum).tolist(), cu=[0, 300, 20, 256], note=("single", top))
        cases.append(case)
    return cases


MAKERS = dict(pl_deltas=make_pl_deltas, ties=make_ties, gq=make_gq, depth_clamps=make_depth_clamps, layout=make_layout, wide=make_wide,
              random=make_random, many_cells=make_many_cells)
SETS = sorted(MAKERS)
SANITIZED = [s for s in SETS if s != "many_cells"]  # (many_cells at full size is device + restatement only)


@functools.lru_cache(maxsize=None)
def cases(name):
    return MAKERS[name]()


def restate(case):
    """the restatement's (phred uint8 [n_samples * total_tri], calls SAMPLE_CALL [n_samples * n_hap]) of a case"""
    return restate_arrays(case.lay, case.n_samples, case.log_score, case.gt_cov, case.hap_u32)


def restate_arrays(lay, n_samples, log_score, gt_cov, hap_u32):
    """the same of any three accumulator arrays; lay: a layout, or the context it is taken from"""
    lay = lay if isinstance(lay, dict) else layout_of(lay)
    phred, rows = ref.calls(lay, n_samples, log_score.tolist(), gt_cov.tolist(), hap_u32.tolist())
    calls = np.zeros(len(rows), gtx.SAMPLE_CALL)
    for k, field in enumerate(ref.FIELDS):
        calls[field] = [r[k] for r in rows]
    return np.array(phred, np.uint8), calls


@functools.lru_cache(maxsize=None)
def expected(name):
    return [restate(c) for c in cases(name)]


def differences(case, want, got):
    """field by field: where (phred, calls) `got` differs from `want` -> list of (what, index, got, wanted), at most a few"""
    out = []
    for what, g, w in [("phred", got[0], want[0])] + [(f, got[1][f], want[1][f]) for f in ref.FIELDS + ("reserved",)]:
        if len(g) != len(w):
            out.append((what, "length", len(g), len(w)))
            continue
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        out += [(what, int(i), int(g[i]), int(w[i])) for i in bad[:3]]
    return out


# ---- the oracle as second witness -------------------------------------------------------------------------------------------
def oracle_calls(case):
    """gto_calls_dump over an oracle genotyper whose HapSamples hold the case's values, clamped to what the reference can hold"""
    ref_s, recs, rb, add_all = graph_inputs(case.key)
    og = Oracle(ref_s, recs, region_begin=rb, add_all_variants=add_all).genotyper(case.n_samples, 1)
    L = case.lay
    tri = case.log_score.reshape(case.n_samples, L["total_tri"])
    cov = np.minimum(case.gt_cov, 0xFFFF).reshape(case.n_samples, L["total_allele"])
    cu = np.minimum(case.hap_u32, 0xFF).reshape(case.n_samples, L["n_hap"], 4)
    assert int(case.log_score.max(initial=0)) <= 0xFFFF
    ls, gc = [], []
    for h, cnum in enumerate(L["hap_cnum"]):  # haplotype by haplotype, sample by sample
        ls.append(tri[:, L["tri_off"][h]:L["tri_off"][h] + n_tri(cnum)].reshape(-1))
        gc.append(cov[:, L["allele_off"][h]:L["allele_off"][h] + cnum].reshape(-1))
    assert og.set_hap_samples(np.concatenate(ls), np.concatenate(gc), cu[:, :, 1].T, cu[:, :, 2].T, cu[:, :, 3].T) == case.cells()
    return og.calls()


def canonical(case, phred, calls):
    return harness.canonical_calls(host_ctx(case.key), phred, calls, case.n_samples)


# ---- case files of tests/emu_calls --------------------------------------------------------------------------------------------
def write_case(path, case):
    """uint32 n_hap, n_samples; uint64 total_tri, total_allele; hap_cnum [n_hap] uint32; tri_off, allele_off [n_hap] uint64; the three
    arrays"""
    L = case.lay
    with open(path, "wb") as f:
        f.write(struct.pack("<IIQQ", L["n_hap"], case.n_samples, L["total_tri"], L["total_allele"]))
        f.write(np.array(L["hap_cnum"], np.uint32).tobytes() + np.array(L["tri_off"], np.uint64).tobytes() + np.array(L["allele_off"], np.uint64).tobytes())
        f.write(case.log_score.tobytes() + case.gt_cov.tobytes() + case.hap_u32.tobytes())


def read_result(path, case):
    """phred [n_samples * total_tri], calls [n_samples * n_hap]: the program's two output blocks, whole"""
    raw = np.fromfile(path, np.uint8)
    n = case.n_samples * case.lay["total_tri"]
    assert len(raw) == n + case.cells() * gtx.SAMPLE_CALL.itemsize
    return raw[:n].copy(), raw[n:].view(gtx.SAMPLE_CALL).copy()


def through(run, case):
    """a case through tests/emu_calls; run(write, read): emu_programs.run with a program and a directory -> (phred, calls)"""
    return run(lambda path: write_case(path, case), lambda path: read_result(path, case))


def judge(name, run):
    """None when the program behind `run` gives the set `name` as the restatement does, else how it differs"""
    for case, want in zip(cases(name), expected(name)):
        if differences(case, want, through(run, case)):
            return "differs from the restatement"
    return None


# ---- the fact tests: from the expected values, that a set reaches what it is for ------------------------------------------------
def _cells_with(case, want, kind):
    """(note, phred row, call) of the cells whose note starts with `kind`"""
    L = case.lay
    for (s, h), note in sorted(case.notes.items()):
        if note[0] == kind:
            t = s * L["total_tri"] + L["tri_off"][h]
            yield note, L["hap_cnum"][h], want[0][t:t + n_tri(L["hap_cnum"][h])], want[1][s * L["n_hap"] + h]


def _gt(call):
    return int(call["gt_first"]), int(call["gt_second"])


def facts_pl_deltas(exp):
    (case,), ((phred, calls),) = cases("pl_deltas"), exp
    rows = case.log_score.reshape(-1, 3).astype(np.int64)
    deltas = set((rows.max(axis=1)[:, None] - rows).reshape(-1).tolist())
    assert {84, 85, 86} <= deltas and set(DELTAS) <= deltas
    seen = set(phred.tolist())
    assert seen == {ref.pl_exact(d) for d in range(85)} | {255} and 253 in seen and 254 not in seen and len(seen) == 86
    assert ref.pl_exact(84) == 253 and ref.pl_exact(85) == 256  # (hence the cap: 85 is the first delta whose PL is 255)
    for mx in (0, MAX_SCORE):  # the cap's neighbours at both ends of the score range
        for d in (84, 85):
            hit = np.nonzero((rows.max(axis=1) == max(mx, d)) & (rows == max(mx, d) - d).any(axis=1))[0]
            assert len(hit) > 0
    assert len({tuple(r) for r in rows.tolist()}) == len(rows)  # every permutation once


def facts_ties(exp):
    (case,), (want,) = cases("ties"), exp
    for note, cnum, row, call in _cells_with(case, want, "equal"):
        assert not row.any() and _gt(call) == (0, 0) and call["gq"] == 0
    singles, pairs = {}, {}
    for note, cnum, row, call in _cells_with(case, want, "single"):
        assert _gt(call) == xy_of(note[1]) and (row == 0).sum() == 1 and call["gq"] > 0
        singles.setdefault(cnum, set()).add(_gt(call))
    for note, cnum, row, call in _cells_with(case, want, "pair"):
        assert _gt(call) == xy_of(min(note[1:])) and (row == 0).sum() == 2 and call["gq"] == 0
        pairs.setdefault(cnum, set()).add(note[1:])
    assert len(list(_cells_with(case, want, "equal"))) == 2 * 4
    for cnum in (3, 4, 7):
        n = n_tri(cnum)
        assert singles[cnum] == {xy_of(i) for i in range(n)} and len(pairs[cnum]) == n * (n - 1) // 2


def facts_gq(exp):
    (case,), (want,) = cases("gq"), exp
    seen = set()
    for note, cnum, row, call in _cells_with(case, want, "only_255"):
        assert call["gq"] == 255 and (row == 0).sum() == 1 and (row == 255).sum() == len(row) - 1 and _gt(call) == xy_of(note[1])
    for note, cnum, row, call in _cells_with(case, want, "next"):
        _, z, q, delta = note
        assert call["gq"] == {1: 3, 84: 253, 85: 255}[delta] == row[q] and row[z] == 0 and (np.delete(row, [z, q]) == 255).all()
        seen.add((cnum, delta, q < z))
    assert seen == {(cnum, delta, before) for cnum in SHAPES["shapes"] for delta in (1, 84, 85) for before in (False, True)}


def facts_depth_clamps(exp):
    (case,), (want,) = cases("depth_clamps"), exp
    L = case.lay
    gt_cov = case.gt_cov.reshape(case.n_samples, -1)
    cu = case.hap_u32.reshape(case.n_samples, L["n_hap"], 4)
    for h, cnum in enumerate(L["hap_cnum"]):  # every word and every counter takes every edge value
        words = gt_cov[:, L["allele_off"][h]:L["allele_off"][h] + cnum]
        assert all(set(COV_EDGES) <= set(words[:, a].tolist()) for a in range(cnum))
        assert all(set(U8_EDGES) <= set(cu[:, h, k].tolist()) for k in (1, 2, 3)) and set(MARKS) <= set(cu[:, h, 0].tolist())
    assert (cu[:, :, 2] <= cu[:, :, 1]).all()
    for note, cnum, row, call in _cells_with(case, want, "ref_clamps"):
        assert call["ref_total_depth"] == 0xFFFF and call["ambiguous_depth"] == 255
    for note, cnum, row, call in _cells_with(case, want, "ref_zero"):
        assert call["ref_total_depth"] == 0 and call["ambiguous_depth"] == 255
    for note, cnum, row, call in _cells_with(case, want, "ref_is_cov0"):
        assert call["ref_total_depth"] == note[1] and call["alt_proper_pair_depth"] == 255
    for note, cnum, row, call in _cells_with(case, want, "ref_reaches"):
        assert call["ref_total_depth"] == note[1]
    for note, cnum, row, call in _cells_with(case, want, "alt_reaches"):
        assert call["alt_total_depth"] == note[1]
    clamped = list(_cells_with(case, want, "alt_clamps"))
    assert len(clamped) == 3 and all(call["alt_total_depth"] == 0xFFFF for _, _, _, call in clamped)
    marks = [call.tobytes() for _, _, _, call in _cells_with(case, want, "mark")]
    assert len(marks) == 3 and len(set(marks)) == 1
    assert {0, 1, 254, 255} <= set(want[1]["ambiguous_depth"].tolist()) and {0, 1, 254, 255} <= set(want[1]["alt_proper_pair_depth"].tolist())
    assert (want[1]["gt_first"] == 0).all() and (want[1]["gt_second"] == 1).all()  # (plain_scores(top=1): the depths are what varies)


def _shifted(case, s, h, which, by):
    """what the restatement makes of cell (s, h) with one of its three rows read `by` words off; None where that leaves the array"""
    L = case.lay
    cnum = L["hap_cnum"][h]
    t = s * L["total_tri"] + L["tri_off"][h] + (by if which == 0 else 0)
    a = s * L["total_allele"] + L["allele_off"][h] + (by if which == 1 else 0)
    c = (s * L["n_hap"] + h) * 4 + (by if which == 2 else 0)
    if min(t, a, c) < 0 or t + n_tri(cnum) > len(case.log_score) or a + cnum > len(case.gt_cov) or c + 4 > len(case.hap_u32):
        return None
    return ref.call_cell(case.log_score[t:t + n_tri(cnum)].tolist(), case.gt_cov[a:a + cnum].tolist(), case.hap_u32[c:c + 4].tolist(), check=False)


def facts_layout(exp):
    """The issue asks that a cell's neighbours in each array hold larger maxima and counters, so that an offset or a stride that is one
    off changes some field; a literal reading cannot hold for both neighbours at once (a row's last word would have to exceed the
    next row's maximum and that row's first word this one's), so the property itself is proved here: for every cell and each of
    the three arrays, the row read one word to the left or to the right gives another result."""
    assert [c.cells() for c in cases("layout")] == [255, 256, 257, 513]
    for case in cases("layout"):
        seen = {}
        for s in range(case.n_samples):
            for h, cnum in enumerate(case.lay["hap_cnum"]):
                scores, cov, cu = case.row(s, h)
                for what, r in (("scores", scores), ("cov", cov), ("cu", cu[1:])):
                    assert seen.setdefault((what, cnum, tuple(r)), (s, h)) == (s, h)  # every cell's rows differ from every other cell's
                here = _shifted(case, s, h, 0, 0)
                for which in range(3):
                    for by in (-1, 1):
                        there = _shifted(case, s, h, which, by)
                        assert there is None or there != here, (case.key, s, h, which, by)
        assert set(case.lay["hap_cnum"]) == {2, 3, 4, 7}


def facts_wide(exp):
    got = set()
    for case, want in zip(cases("wide"), exp):
        assert sorted(case.lay["hap_cnum"])[-2] == 100 and max(case.lay["hap_cnum"]) > 1000 and case.n_samples == 2
        for note, cnum, row, call in _cells_with(case, want, "single"):
            n = n_tri(cnum)
            assert _gt(call) == xy_of(note[1]) and row[note[1]] == 0
            got.add((cnum > 100, "first" if note[1] == 0 else "last" if note[1] == n - 1 else "inside"))
        for note, cnum, row, call in _cells_with(case, want, "pair"):
            assert _gt(call) == xy_of(note[1]) and call["gq"] == 0 and note[2] - note[1] > n_tri(cnum) // 2 and call["alt_total_depth"] == 0xFFFF
            got.add((cnum > 100, "pair"))
    assert got >= {(big, what) for big in (False, True) for what in ("first", "last", "pair")}
    assert xy_of(n_tri(100) - 1) == (99, 99)


def facts_random(exp):
    for case, want in zip(cases("random"), exp):
        assert (want[1]["gq"] == 0).any() and (want[1]["gq"] == 255).any() and (want[1]["ref_total_depth"] == 0xFFFF).any()
        assert (case.hap_u32.reshape(-1, 4)[:, 0] >> 31).any() and (want[0] == 253).any()
    assert sum(c.cells() for c in cases("random")) > 3000


def facts_many_cells(exp):
    (case,) = cases("many_cells")
    assert case.cells() >= 40003 and case.cells() % 256 not in (0, 255) and set(case.lay["hap_cnum"]) == {2, 3, 4, 7}
    assert MANY_CELLS_SAMPLES_SANITIZED * case.lay["n_hap"] == 2052


FACTS = dict(pl_deltas=facts_pl_deltas, ties=facts_ties, gq=facts_gq, depth_clamps=facts_depth_clamps, layout=facts_layout, wide=facts_wide,
             random=facts_random, many_cells=facts_many_cells)
