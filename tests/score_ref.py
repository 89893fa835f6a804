"""A plain restatement of what one score item -- an unpaired read, a mate pair, a read whose mate never came -- adds to the score
accumulators, written from the reference's text and from the layouts in include/gtx.h (the record words :286-299, gtx_score_item
:205-235, gtx_score_buffers :412-446) -- not from the kernels (graphtyper_amd/csrc/score_core.hpp: score_item and everything under
it), which it is there to judge.

  update_unpaired_read_paths        src/typer/alignment.cpp:365-455       the better orientation of one read, its flags
  update_paths                      src/typer/alignment.cpp:482-545       the flags of both orientations of a mate
  get_better_paths                  src/typer/alignment.cpp:557-620       the four orientations of two mates put in their places
  compare_pair_of_genotype_paths    src/typer/genotype_paths.cpp:943-974  (one read), :976-1169 (a pair)
  all_paths_unique / _fully_aligned src/typer/genotype_paths.cpp:219-231, :836-845
  are_genotype_paths_good           src/typer/vcf_writer.cpp:28-60
  update_haplotype_scores_geno      src/typer/vcf_writer.cpp:88-141 (one read), :143-250 (a pair: the mates' cross links)
  push_to_haplotype_scores          src/typer/vcf_writer.cpp:503-676
  Haplotype::add_coverage           src/graph/haplotype.cpp:180-227
  *_to_stats, coverage_to_gts       src/graph/haplotype.cpp:229-361
  Haplotype::explain_to_score       src/graph/haplotype.cpp:462-585       (score(): without the guard at :560; replay(): the guard, call by call)
  Graph::get_ref_reach_pos          src/graph/graph.cpp:1784-1795
  the leftover read                 src/utilities/hts_parallel_reader.cpp:719-745

Plain Python integers, sets and dicts throughout.  The one place the reference leaves the integers is the mismatch ratio of
are_genotype_paths_good, a double quotient compared with a double literal: ratio_exceeds() below makes that comparison exactly -- the
correctly rounded quotient, as a rational, against the literal's exact value -- and test_score_emu.py shows where that differs from
the comparison of the unrounded quotient (only on the literal 0.03, whose double lies below 3/100).

Contract of a record (what the aligner leaves and a hand-made record has to keep): longest_path_length is the largest size
(read_end_index - read_start_index + 1) of its paths, and it is the read's length only where every path's is (push_to_haplotype_scores
asserts at :512 that "the longest path is the read" and "every path is the read" are one fact; a record where they differ is refused here); every site index is below
n_hap and every allele of a mask below the site's number of alleles; bit 31 of word 1 says whether some path carries a site (a
record that has sites and does not say so adds nothing: the scorer's first stage reads that bit alone).
Out of scope: the reference-depth track of SV calling, records with GTX_REC_WIDE sets only through
big_records()."""
import collections
from fractions import Fraction

INVALID = 0xFFFFFFFF
SPECIAL_START = 0xD0000000                       # include/graphtyper/constants.hpp.in
IS_PROPER_PAIR, IS_UNMAPPED, IS_SEQ_REVERSED, IS_FIRST_IN_PAIR, IS_MAPQ_BAD = 2, 4, 16, 64, 4096
EPSILON_0_EXPONENT = 12
NO_COVERAGE, MULTI_ALT_COVERAGE, MULTI_REF_COVERAGE = 0xFFFF, 0xFFFE, 0xFFFD   # include/graphtyper/graph/haplotype.hpp:86-88
FLAG_FORWARD_ONLY, ITEM_LEFTOVER = 0x8000, 1    # include/gtx.h
ST_EXTERNAL, REC_HAS_VARIANTS, REC_WIDE, WIDE_MASK_WORDS = 16, 0x80000000, 0x40000000, 80
THRESHOLDS = (0.05, 0.025, 0.03, 0.035)          # the literals of vcf_writer.cpp:41-55


def ratio_exceeds(mismatches, size, literal):
    """static_cast<double>(mismatches) / static_cast<double>(size) > literal (vcf_writer.cpp:38-55), made exactly: IEEE division rounds
    the quotient to the nearest double, a Python float is that double, and the two doubles are compared as rationals"""
    return Fraction(float(mismatches) / float(size)) > Fraction(literal)


def ratio_exceeds_unrounded(mismatches, size, literal):
    """the same comparison of the quotient itself, unrounded, with the literal's exact value"""
    return Fraction(mismatches, size) > Fraction(literal)


# ---- records ----------------------------------------------------------------------------------------------------------------
Path = collections.namedtuple("Path", "start end rs re mm vars")   # vars: list of (site, frozenset of alleles)
Geno = collections.namedtuple("Geno", "paths longest read_len has_var")


def path_size(p):
    return p.re - p.rs + 1


def parse_record(words, at, big_records=None):
    """the record that starts at words[at] (include/gtx.h:286-299) -> Geno"""
    w0, w1 = int(words[at]), int(words[at + 1])
    n_paths, status = w0 & 0xFFFF, w0 >> 16
    longest, read_len = w1 & 0xFFFF, (w1 >> 16) & 0x3FFF
    mw = WIDE_MASK_WORDS if w1 & REC_WIDE else 2
    w, k = words, at + 2
    if status & ST_EXTERNAL:
        w, k = big_records, int(words[at + 2])
    paths = []
    for _ in range(n_paths):
        start, end, rsre, mmnv = (int(w[k + j]) for j in range(4))
        k += 4
        sites = []
        for _v in range(mmnv >> 16):
            site = int(w[k])
            alleles = frozenset(32 * x + a for x in range(mw) for a in range(32) if (int(w[k + 1 + x]) >> a) & 1)
            sites.append((site, alleles))
            k += 1 + mw
        paths.append(Path(start, end, rsre & 0xFFFF, rsre >> 16, mmnv & 0xFFFF, sites))
    return Geno(paths, longest, read_len, bool(w1 & REC_HAS_VARIANTS))


# ---- the graph's facts ---------------------------------------------------------------------------------------------------------
class Facts:
    """what the scorer needs of a graph: gtx_ctx_haplotypes, gtx_ctx_near_pairs, gtx_ctx_score_layout, the special positions' reference
    reach (gtx_ctx_special_positions), as plain Python values"""

    def __init__(self, hap_order, hap_cnum, tri_off, allele_off, near_last, near_off, total_near, special_ref_reach):
        self.hap_order = [int(x) for x in hap_order]
        self.hap_cnum = [int(x) for x in hap_cnum]
        self.tri_off = [int(x) for x in tri_off]
        self.allele_off = [int(x) for x in allele_off]
        self.near_last = [int(x) for x in near_last]
        self.near_off = [int(x) for x in near_off]
        self.total_near = int(total_near)
        self.special_ref_reach = [int(x) for x in special_ref_reach]
        self.n_hap = len(self.hap_cnum)
        self.total_tri = sum(c * (c + 1) // 2 for c in self.hap_cnum)
        self.total_allele = sum(self.hap_cnum)

    @classmethod
    def of(cls, ctx):
        return cls(ctx.hap_order, ctx.hap_cnum, ctx.tri_off, ctx.allele_off, ctx.near_last, ctx.near_off, ctx.total_near, ctx.special_positions()[0])

    def ref_reach(self, pos):
        """Graph::get_ref_reach_pos (graph.cpp:1784-1795)"""
        if pos >= SPECIAL_START and pos - SPECIAL_START < len(self.special_ref_reach):
            return self.special_ref_reach[pos - SPECIAL_START]
        return pos


Params = collections.namedtuple("Params", "is_sv_graph hq_reads is_segment_calling", defaults=(False, False, False))


# ---- the selection -------------------------------------------------------------------------------------------------------------
def compare_single(g1, g2):
    """compare_pair_of_genotype_paths, one read (genotype_paths.cpp:943-974) -> 1, 2 or 0"""
    t1, t2, minimum = g1.longest, g2.longest, 94
    if t1 > t2 and t1 > minimum:
        return 1
    if t2 > t1 and t2 > minimum:
        return 2
    if t2 == t1 and t1 > minimum:
        m1, m2 = g1.paths[0].mm, g2.paths[0].mm
        return 1 if m1 < m2 else 2 if m2 < m1 else 1
    return 0


def alternative_call_count(g):
    """genotype_paths.cpp:1053-1066: sites of any path whose set does not hold allele 0 (an empty set counts)"""
    return sum(0 not in alleles for p in g.paths for _, alleles in p.vars)


def compare_pairs(g11, g12, g21, g22):
    """compare_pair_of_genotype_paths, two pairs (genotype_paths.cpp:976-1169) -> 1, 2 or 0; also which rule decided"""
    t11, t12, t21, t22 = (g.longest if g.paths else 0 for g in (g11, g12, g21, g22))
    max1, max2 = max(t11, t12), max(t21, t22)
    perfect1, perfect2 = g11.read_len, g12.read_len
    minimum = 94
    is1 = t11 >= perfect1 and t12 >= perfect2
    is2 = t21 >= perfect1 and t22 >= perfect2
    if is1 or is2:
        if is1 and is2:
            m1, m2 = g11.paths[0].mm + g12.paths[0].mm, g21.paths[0].mm + g22.paths[0].mm
            if m1 != m2:
                return (1 if m1 < m2 else 2), "perfect_mismatches"
            n1, n2 = len(g11.paths) + len(g12.paths), len(g21.paths) + len(g22.paths)
            if n1 != n2:
                return (1 if n1 < n2 else 2), "perfect_paths"
            c1, c2 = alternative_call_count(g11) + alternative_call_count(g12), alternative_call_count(g21) + alternative_call_count(g22)
            return (1 if c1 >= c2 else 2), "perfect_alt_calls"
        return (1 if is1 else 2), "perfect_one"
    if max2 >= minimum and max2 > max1:
        return 2, "longer"
    if max1 >= minimum and max1 > max2:
        return 1, "longer"
    if max1 >= minimum and max2 >= minimum:
        m1 = m2 = 10
        if t11 == max1:
            m1 = min(m1, g11.paths[0].mm)
        if t12 == max1:
            m1 = min(m1, g12.paths[0].mm)
        if t21 == max2:
            m2 = min(m2, g21.paths[0].mm)
        if t22 == max2:
            m2 = min(m2, g22.paths[0].mm)
        if m1 != m2:
            return (1 if m1 < m2 else 2), "mismatches"
        if min(t11, t12) < min(t21, t22):
            return 1, "minimum"
        if min(t21, t22) < min(t11, t12):
            return 2, "minimum"
        return 0, "tie"
    if max2 == 0 and t11 >= 63 and t12 >= 63:
        return 1, "rule63"
    if max1 == 0 and t21 >= 63 and t22 >= 63:
        return 2, "rule63"
    return 1, "last"


# ---- goodness --------------------------------------------------------------------------------------------------------------------
def all_paths_fully_aligned(g):
    return all(path_size(p) == g.read_len for p in g.paths)


def all_paths_unique(facts, g):
    """genotype_paths.cpp:219-231"""
    p0 = g.paths[0]
    return not any(facts.ref_reach(p0.start) != facts.ref_reach(p.start) and facts.ref_reach(p0.end) != facts.ref_reach(p.end) for p in g.paths[1:])


def is_good(facts, par, g):
    """are_genotype_paths_good (vcf_writer.cpp:28-60)"""
    if not g.paths:
        return False
    fully = all_paths_fully_aligned(g)
    size0, mm0 = path_size(g.paths[0]), g.paths[0].mm
    if not fully and (not all_paths_unique(facts, g) or size0 < 63):
        return False
    if ratio_exceeds(mm0, size0, 0.05):
        return False
    if not fully and ratio_exceeds(mm0, size0, 0.025):
        return False
    if par.is_sv_graph and (not fully or size0 < 90 or ratio_exceeds(mm0, size0, 0.03)):
        return False
    if par.hq_reads and (not fully or size0 < 90 or ratio_exceeds(mm0, size0, 0.035)):
        return False
    return True


# ---- the sums ----------------------------------------------------------------------------------------------------------------------
def add_coverage(coverage, c):
    """Haplotype::add_coverage (haplotype.cpp:180-227)"""
    if coverage == NO_COVERAGE:
        return c
    if coverage == MULTI_ALT_COVERAGE:
        return MULTI_REF_COVERAGE if c == 0 else coverage
    if coverage == MULTI_REF_COVERAGE:
        return coverage
    if coverage != c:
        return MULTI_REF_COVERAGE if coverage == 0 or c == 0 else MULTI_ALT_COVERAGE
    return coverage


class Sums:
    """every array of gtx_score_buffers as unsaturated sums: index -> Python integer (what is not there is 0); the connection log as a
    multiset of (sample, h1, b1, h2, b2, count); `dropped` stays 0 here (conn_cap is the caller's)"""
    ARRAYS = ("log_score", "gt_cov", "hap_u32", "stat_u64", "stat_u32", "conn_near")

    def __init__(self, facts, n_samples):
        self.facts, self.n_samples = facts, n_samples
        for name in self.ARRAYS:
            setattr(self, name, collections.Counter())
        self.conn_log = collections.Counter()
        self.dropped = 0
        self.items = []  # per item: what was decided

    def sizes(self):
        f, n = self.facts, self.n_samples
        return dict(log_score=n * f.total_tri, gt_cov=n * f.total_allele, hap_u32=n * f.n_hap * 4, stat_u64=f.n_hap + 2 * f.total_allele,
                    stat_u32=f.n_hap + 6 * f.total_allele, conn_near=n * f.total_near)

    def dense(self, name):
        """one array as a list of Python integers"""
        out = [0] * self.sizes()[name]
        for i, v in getattr(self, name).items():
            assert 0 <= i < len(out), (name, i)
            out[i] = v
        return out

    def connection(self, sample, h1, b1, h2, b2, count, k, near):
        """HapSample::connections[b1][h2][b2] += count (vcf_writer.cpp:119-139, :229-249), into the dense counters of the near pairs
        (include/gtx.h:419-424) or the log"""
        f = self.facts
        assert h2 > h1
        if near and h2 <= f.near_last[h1]:
            first = f.allele_off[h1 + 1]
            width = f.allele_off[f.near_last[h1]] + f.hap_cnum[f.near_last[h1]] - first
            self.conn_near[sample * f.total_near + f.near_off[h1] + b1 * width + (f.allele_off[h2] - first) + b2] += count * k
        else:
            self.conn_log[(sample, h1, b1, h2, b2, count)] += k


def explain_epsilon(mismatches, non_unique, flags, fully_aligned, overlapping):
    """the exponent of explain_to_score (haplotype.cpp:470-501); no read of a genotyping run has a low-quality base (qual2 is empty)"""
    e = EPSILON_0_EXPONENT - mismatches
    if non_unique:
        e -= 3
    if flags & IS_MAPQ_BAD:
        e -= 2
    if not fully_aligned:
        e -= 3
    if not overlapping:
        e -= 1
    return max(e, 8) - 4


def push_to_haplotype_scores(sums, g, flags, mapq, score_diff, proper_pair, sample, k, note):
    """vcf_writer.cpp:503-676 for one good GenotypePaths, k times -> new_connections: {(hap, allele): [(hap2, allele2), ...]}"""
    f = sums.facts
    clipped_bp = g.read_len - g.longest
    fully_aligned = clipped_bp == 0
    if fully_aligned != all_paths_fully_aligned(g) or g.longest != max(path_size(p) for p in g.paths):
        raise ValueError("a record whose longest_path_length is not what its paths say (vcf_writer.cpp:509-512)")
    non_unique = not all_paths_unique(f, g)
    mismatches = g.paths[0].mm
    recent, explains, coverage = {}, {}, {}
    for p in g.paths:
        for site, alleles in p.vars:
            if not alleles:
                continue
            order = f.hap_order[site]  # Path::var_order of the site (include/gtx.h:293)
            overlapping = f.ref_reach(p.start) + 3 <= order and f.ref_reach(p.end) - 3 > order
            recent[site] = recent.get(site, False) or overlapping
            explains.setdefault(site, set()).update(alleles)
            cov = coverage.get(site, NO_COVERAGE)
            if len(alleles) == 1:
                cov = add_coverage(cov, min(alleles))
            else:
                cov = add_coverage(cov, 1)
                cov = add_coverage(cov, 0 if 0 in alleles else 2)
            coverage[site] = cov
    new_connections = {}
    order_of_sites = sorted(recent)  # std::map
    for i, h1 in enumerate(order_of_sites):
        n1 = len(explains[h1])
        if n1 == 0 or n1 > 64:
            continue
        for b1 in sorted(explains[h1]):
            conn = new_connections.setdefault((h1, b1), [])
            for h2 in order_of_sites[i + 1:]:
                n2 = len(explains[h2])
                if n2 == 0 or n2 > 64:
                    continue
                weight = n1 * n2
                repeat = 6 // weight if weight >= 3 else 1
                for b2 in sorted(explains[h2]):
                    conn.extend([(h2, b2)] * repeat)
    nh = f.n_hap
    for h in order_of_sites:
        cov = coverage[h]
        cnum, aoff, toff = f.hap_cnum[h], f.allele_off[h], f.tri_off[h]
        assert all(a < cnum for a in explains[h]), "an allele the site does not have"
        unique_allele = cov < MULTI_REF_COVERAGE
        if clipped_bp != 0:                                  # clipped_reads_to_stats (haplotype.cpp:229-244)
            if cov != NO_COVERAGE:
                sums.stat_u32[h] += k
            if unique_allele:
                sums.stat_u64[nh + 2 * (aoff + cov) + 0] += k * ((clipped_bp * 1000) // g.read_len)
        if mapq != 255:                                      # mapq_to_stats (:246-261)
            if cov != NO_COVERAGE:
                sums.stat_u64[h] += k * mapq * mapq
            if unique_allele:
                sums.stat_u64[nh + 2 * (aoff + cov) + 1] += k * mapq * mapq
        if unique_allele:
            s32 = nh + 6 * (aoff + cov)
            forward, first = (flags & IS_SEQ_REVERSED) == 0, (flags & IS_FIRST_IN_PAIR) != 0
            sums.stat_u32[s32 + (2 if forward and first else 3 if first else 4 if forward else 5)] += k   # strand_to_stats (:263-287)
            mm8 = mismatches & 0xFF                          # mismatches_to_stats (:289-300) takes a uint8_t
            if mm8 != 0:
                sums.stat_u32[s32 + 1] += k * ((mm8 * 1000) // g.read_len)
            if score_diff != 0:                              # score_diff_to_stats (:302-313)
                sums.stat_u32[s32 + 0] += k * score_diff
        eps = explain_epsilon(mismatches, non_unique, flags, fully_aligned, recent[h])
        cell = (sample * nh + h) * 4
        sums.hap_u32[cell + 0] += k * eps                    # max_log_score (haplotype.cpp:563)
        ls = sample * f.total_tri + toff
        for y in range(cnum):                                # haplotype.cpp:566-583: genotype (x, y), x <= y, is entry y (y + 1) / 2 + x
            if y in explains[h]:
                for x in range(y + 1):
                    sums.log_score[ls + y * (y + 1) // 2 + x] += k * (eps if x in explains[h] else eps - 1)
            else:                                            # (only the explained x change such a row: a site may have 2 559 alleles)
                for x in explains[h]:
                    if x <= y:
                        sums.log_score[ls + y * (y + 1) // 2 + x] += k * (eps - 1)
        if cov == MULTI_REF_COVERAGE:                        # coverage_to_gts (:315-361)
            sums.hap_u32[cell + 1] += k
        elif cov == MULTI_ALT_COVERAGE:
            sums.hap_u32[cell + 1] += k
            sums.hap_u32[cell + 2] += k
            if proper_pair:
                sums.hap_u32[cell + 3] += k
        elif cov != NO_COVERAGE:
            sums.gt_cov[sample * f.total_allele + aoff + cov] += k
            if cov > 0 and proper_pair:
                sums.hap_u32[cell + 3] += k
        note["sites"].append(dict(site=h, explains=frozenset(explains[h]), coverage=cov, eps=eps, overlapping=recent[h]))
    note.update(fully=fully_aligned, unique=not non_unique, mismatches=mismatches)
    return new_connections


def commit(sums, merged, sample, k, near):
    """vcf_writer.cpp:119-139 / :229-249: one count per entry of every key's list; entries of one key towards one (hap2, allele2) that
    come from one read's `repeat` are one log entry of that count"""
    for (h1, b1), targets in merged.items():
        for (h2, b2), count in collections.Counter(targets).items():
            sums.connection(sample, h1, b1, h2, b2, count, k, near)


class _Meta:
    def __init__(self, m):
        self.align_index, self.flag, self.mapq, self.score_diff = int(m["align_index"]), int(m["flag"]), int(m["mapq"]), int(m["score_diff"])


def orientations(records, rec_words, meta, big_records, compact=None, side=None):
    """the two GenotypePaths of a record: (read, 0) and (read, 1) -- the second empty for a read aligned forward only (include/gtx.h:205-211);
    a forward record whose side byte carries GTX_TASK_COMPACT is taken from `compact` (include/gtx.h:360-371)"""
    at = meta.align_index * 2 * rec_words
    if compact is not None and int(side[2 * meta.align_index]) & 2:
        fwd = parse_record(compact, meta.align_index * 8, None)
    else:
        fwd = parse_record(records, at, big_records)
    if meta.flag & FLAG_FORWARD_ONLY:
        return fwd, Geno([], 0, fwd.read_len, False)
    return fwd, parse_record(records, at + rec_words, big_records)


def score(facts, par, records, rec_words, items, n_samples, multiplicity=None, big_records=None, near=True, compact=None, side=None):
    """gtx_score_batch as the reference would have it: every item's call of genotype_only() that reaches the VcfWriter
    (hts_parallel_reader.cpp:283-337, :733-744) -> Sums.  multiplicity[i]: how often item i occurs (the sums are linear in the items)."""
    sums = Sums(facts, n_samples)
    for i, it in enumerate(items):
        k = 1 if multiplicity is None else int(multiplicity[i])
        first, second = _Meta(it["first"]), _Meta(it["second"])
        sample, kind = int(it["sample"]), int(it["kind"])
        note = dict(kind="single" if second.align_index == INVALID else "leftover" if kind & ITEM_LEFTOVER else "pair", which=None, rule=None,
                    trivial=False, reads=[], sample=sample)
        sums.items.append(note)
        assert sample < n_samples
        if k == 0:
            continue
        g1 = orientations(records, rec_words, first, big_records, compact, side)
        if second.align_index == INVALID:
            if not (g1[0].has_var or g1[1].has_var):
                note["trivial"] = True
                continue
            which = compare_single(*g1)                      # update_unpaired_read_paths (alignment.cpp:365-455)
            note["which"] = which
            if which == 0:
                continue
            core_flag = first.flag & 0x7FFF
            geno = g1[which - 1]
            flags = (core_flag if which == 1 else core_flag ^ IS_SEQ_REVERSED) & ~IS_PROPER_PAIR
            if first.mapq < 25:
                flags |= IS_MAPQ_BAD
            if par.is_segment_calling:                       # vcf_writer.cpp:95-96
                continue
            good = is_good(facts, par, geno)
            read = dict(good=good, sites=[], flags=flags)
            note["reads"].append(read)
            if good:                                         # ml_insert_size stays INSERT_SIZE_WHEN_NOT_PROPER_PAIR: not a proper pair
                commit(sums, push_to_haplotype_scores(sums, geno, flags, first.mapq, first.score_diff, False, sample, k, read), sample, k, near)
            continue
        g2 = orientations(records, rec_words, second, big_records, compact, side)
        if not any(g.has_var for g in g1 + g2):
            note["trivial"] = True
            continue
        genos = []                                           # update_paths (alignment.cpp:482-545): (geno, flags, mapq, score_diff)
        for g, m in ((g1, first), (g2, second)):
            core_flag = m.flag & 0x7FFF
            f1 = core_flag & ~IS_PROPER_PAIR
            if m.mapq < 25:
                f1 |= IS_MAPQ_BAD
            genos.append([g[0], f1, m.mapq, m.score_diff])
            genos.append([g[1], (core_flag ^ IS_SEQ_REVERSED) & ~IS_PROPER_PAIR, m.mapq, m.score_diff])
        arr = [None] * 4                                     # get_better_paths (alignment.cpp:557-620)
        for e in genos:
            arr[((e[1] & IS_FIRST_IN_PAIR) != 0) + 2 * ((e[1] & IS_SEQ_REVERSED) == 0)] = e
        if any(e is None for e in arr):
            note["rule"] = "orientation"
            continue
        pair1, pair2 = (arr[3], arr[0]), (arr[1], arr[2])
        which, rule = compare_pairs(pair1[0][0], pair1[1][0], pair2[0][0], pair2[1][0])
        note["which"], note["rule"] = which, rule
        if which == 0:
            continue
        better = pair1 if which == 1 else pair2
        for e in better:
            e[1] |= IS_PROPER_PAIR
        good = [is_good(facts, par, e[0]) for e in better]
        reads = [dict(good=good[j], sites=[], flags=better[j][1]) for j in range(2)]
        if kind & ITEM_LEFTOVER:                             # hts_parallel_reader.cpp:733-744: better.first alone, the one-read overload
            note["reads"].append(reads[0])
            if not par.is_segment_calling and good[0]:
                e = better[0]                                # ml_insert_size was set by update_paths: a proper pair
                commit(sums, push_to_haplotype_scores(sums, e[0], e[1], e[2], e[3], True, sample, k, reads[0]), sample, k, near)
            continue
        note["reads"] += reads
        if par.is_segment_calling and not (good[0] and good[1]):   # vcf_writer.cpp:167-168
            continue
        con = [push_to_haplotype_scores(sums, e[0], e[1], e[2], e[3], True, sample, k, reads[j]) if good[j] else {} for j, e in enumerate(better)]
        merged = {}                                          # vcf_writer.cpp:186-227
        for key1, targets in con[0].items():
            merged[key1] = list(targets) + [key2 for key2 in con[1] if key2[0] > key1[0]]
        for key2, targets in con[1].items():
            if key2 in merged:
                merged[key2] += list(targets)
            else:
                merged[key2] = list(targets)
            merged[key2] += [key1 for key1 in con[0] if key1[0] > key2[0]]
        # (a log entry is one read's count towards one target: the mates' own connections and the cross links are committed apart)
        commit(sums, con[0], sample, k, near)
        commit(sums, con[1], sample, k, near)
        cross = {key: list((collections.Counter(merged[key]) - collections.Counter(con[0].get(key, [])) - collections.Counter(con[1].get(key, []))).elements())
                 for key in merged}
        for (h1, b1), targets in cross.items():
            for h2, b2 in targets:
                sums.connection(sample, h1, b1, h2, b2, 1, k, near)
    return sums


# ---- the guard, call by call -------------------------------------------------------------------------------------------------------
SATURATION_GUARD = 0xFFFF - 8   # explain_to_score refuses a call when max_log_score >= 0xFFFF - epsilon, and epsilon <= 8
Replayed = collections.namedtuple("Replayed", "head rows marked unsupported log beyond")


def replay(sums, sequence, item_base=0):
    """Haplotype::explain_to_score with its guard (haplotype.cpp:560-584) over the items `sequence` -- indices into the distinct items
    that `sums` = score(...) was made of, with multiplicity = how often each occurs in the sequence -- in the order the reference makes
    the calls: item by item; within an item the first read of the better pair, then the second (vcf_writer.cpp:170-184; the one-read
    overload :88-141 and the leftover read make one call per site); within a read one call per site, each on a cell of its own.
      head[cell]    max_log_score with the guard, cell = sample * n_hap + site, for every cell that was added to
      rows[cell]    the guarded genotype triangle (entry y (y + 1) / 2 + x) of every marked cell
      marked        the cells whose unguarded sum is >= 0xFFFF - 8 on a site of at most 64 alleles; unsupported: those on a larger site
      log           (item + item_base, cell, order, epsilon, mask) of every call on a marked cell: order = which read of the item
      beyond[cell]  (max_log_score, triangle) with the guard of every unsupported cell: what the reference has there (not in the log)
    A cell whose unguarded sum stays below 0xFFFF - 8 never had a call refused: max_log_score only grows, so before every call it was
    below 0xFFFF - 8 <= 0xFFFF - epsilon; its guarded values are the sums of score() and it is not walked."""
    f = sums.facts
    nh = f.n_hap
    head = {i // 4: v for i, v in sums.hap_u32.items() if i % 4 == 0}
    at_guard = {cell for cell, v in head.items() if v >= SATURATION_GUARD}
    marked = {cell for cell in at_guard if f.hap_cnum[cell % nh] <= 64}
    calls = []  # per distinct item: its calls on marked cells (cell, order, epsilon, mask, addends of the triangle)
    for note in sums.items:
        mine = []
        for order, read in enumerate(note["reads"]):
            for x in read["sites"]:
                cell = note["sample"] * nh + x["site"]
                if cell not in at_guard:
                    continue
                eps, explains, adds, i = x["eps"], x["explains"], [], 0
                for y in range(f.hap_cnum[x["site"]]):           # haplotype.cpp:566-583
                    for xx in range(y + 1):
                        if xx in explains and y in explains:
                            adds.append((i, eps))
                        elif xx in explains or y in explains:
                            adds.append((i, eps - 1))
                        i += 1
                mine.append((cell, order, eps, sum(1 << a for a in explains), adds))
        calls.append(mine)
    state = {cell: [0, [0] * (f.hap_cnum[cell % nh] * (f.hap_cnum[cell % nh] + 1) // 2)] for cell in at_guard}
    log = []
    for pos, d in enumerate(sequence):
        for cell, order, eps, mask, adds in calls[d]:
            if cell in marked:
                log.append((pos + item_base, cell, order, eps, mask))
            st = state[cell]
            if st[0] < 0xFFFF - eps:                             # haplotype.cpp:560
                st[0] += eps
                row = st[1]
                for i, v in adds:
                    row[i] += v
    for cell in marked:
        head[cell] = state[cell][0]
    return Replayed(head, {cell: state[cell][1] for cell in marked}, marked, at_guard - marked, log,
                    {cell: tuple(state[cell]) for cell in at_guard - marked})
