"""A plain restatement of the genotype call of one (sample, haplotype) cell, written from the reference's text and from the
layout in include/gtx.h:547-561 -- not from the kernel (graphtyper_amd/csrc/score_core.hpp: call_cell), which it is there to judge.

  get_haplotype_phred           src/typer/vcf.cpp:47-82        PL of every genotype from the cell's log scores
  SampleCall::SampleCall        src/typer/sample_call.cpp:34-61   the two depth sums, each stopped at 0xFFFF
  SampleCall::get_gt_call       src/typer/sample_call.cpp:78-106  the first genotype (x <= y, y outermost) with PL 0
  SampleCall::get_gq            src/typer/sample_call.cpp:108-129 0 as soon as two PLs are 0, else the lowest PL that is not 0
  HapSample::increment_*        src/graph/haplotype.cpp:19-44     the u8 / u16 counters stop at 0xFF / 0xFFFF, each on its own

Plain Python integers throughout; PL is computed with `decimal` at 60 digits and rounded half away from zero (std::llround),
so nothing here depends on how a double rounds.  test_calls_emu.py proves, for every delta a u16 row can hold, that the
reference's double product rounds to the same integer.

Contract: every log score is below 0x10000 (the reference keeps them in uint16_t; gtx_scores_replay is what brings a cell of the
product back under that limit) -- a value beyond it is refused here, not clamped.  The accumulators are the product's raw uint32
sums (gt_cov words, hap_u32 = [max_log_score | replay mark, ambiguous, ambiguous_alt, alt_proper_pair] per cell)."""
import decimal

_CTX = decimal.Context(prec=60, rounding=decimal.ROUND_HALF_UP)
TEN_LOG10_2 = _CTX.multiply(_CTX.log10(decimal.Decimal(2)), decimal.Decimal(10))  # 3.0102999566398119521373889472449302676818988146210854131...
PL_CAP = 255
_pl = []


def pl_exact(delta):
    """round-half-away-from-zero of delta * 10 log10(2), no cap"""
    return int(_CTX.multiply(decimal.Decimal(delta), TEN_LOG10_2).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP, context=_CTX))


def pl_of(delta):
    """vcf.cpp:69-78: the row starts as 255 and an entry is overwritten only where the rounded score is < 255"""
    return pl_table()[delta]


def pl_table():
    """pl_of for every delta two uint16 scores can have, worked out once"""
    if not _pl:
        _pl.extend(min(pl_exact(delta), PL_CAP) if delta < 100 else PL_CAP for delta in range(0x10000))
        assert pl_exact(99) > PL_CAP  # (the product grows with delta: from here on the cap)
    return _pl


def phred_row(scores):
    """get_haplotype_phred (vcf.cpp:47-82)"""
    mx = max(scores)
    if min(scores) == mx:  # vcf.cpp:58-66: all scores equal -> all zero
        return [0] * len(scores)
    table = pl_table()
    return [table[mx - v] for v in scores]


def gt_call(phred, cnum):
    """SampleCall::get_gt_call (sample_call.cpp:78-106)"""
    i = 0
    for y in range(cnum):
        for x in range(y + 1):
            if phred[i] == 0:
                return x, y
            i += 1
    raise AssertionError("no PL is 0")  # (sample_call.cpp:98-104: cannot happen, the maximum's PL is 0)


def gq_of(phred):
    """SampleCall::get_gq (sample_call.cpp:108-129)"""
    seen_zero = False
    next_lowest = 255
    for p in phred:
        if p == 0:
            if seen_zero:
                return 0
            seen_zero = True
        elif p < next_lowest:
            next_lowest = p
    return next_lowest


def call_cell(scores, cov, counters, check=True):
    """one cell: scores [n_tri], cov [cnum] raw words, counters = the cell's four hap_u32 words ->
    (phred [n_tri], (gt_first, gt_second, ref_total_depth, alt_total_depth, gq, ambiguous_depth, alt_proper_pair_depth))"""
    if max(scores) >= 0x10000:
        raise ValueError("a log score of 0x10000 or more is outside what the reference can hold (gtx_scores_replay comes first)")
    cnum = len(cov)
    assert cnum > 1 and len(scores) == cnum * (cnum + 1) // 2  # sample_call.cpp:44
    phred = phred_row(scores)
    coverage = [min(c, 0xFFFF) for c in cov]                           # haplotype.cpp:33-38
    ambiguous, ambiguous_alt, alt_pp = (min(c, 0xFF) for c in counters[1:4])  # haplotype.cpp:19-31, 40-44 (counters[0] is not a depth)
    assert ambiguous >= ambiguous_alt or not check                     # sample_call.cpp:45 (check=False: rows that are no cell's, calls_cases.facts_layout)
    ref_total = min(0xFFFF, coverage[0] + ambiguous - ambiguous_alt)   # sample_call.cpp:48-52
    alt_total = min(0xFFFF, sum(coverage[1:]) + ambiguous)             # sample_call.cpp:55-57
    x, y = gt_call(phred, cnum)
    return phred, (x, y, ref_total, alt_total, gq_of(phred), ambiguous, alt_pp)


FIELDS = ("gt_first", "gt_second", "ref_total_depth", "alt_total_depth", "gq", "ambiguous_depth", "alt_proper_pair_depth")


def calls(layout, n_samples, log_score, gt_cov, hap_u32):
    """The whole call stage.  layout: dict(hap_cnum, tri_off, allele_off -- one entry per haplotype --, n_hap, total_tri, total_allele);
    the three accumulators as flat sequences of Python integers laid out as include/gtx.h says: log_score [n_samples * total_tri] at
    sample * total_tri + tri_off[hap], gt_cov [n_samples * total_allele] at sample * total_allele + allele_off[hap], hap_u32
    [n_samples * n_hap * 4] at (sample * n_hap + hap) * 4.
    -> (phred: list [n_samples * total_tri] in the layout of log_score, calls: list [n_samples * n_hap] of 7-tuples in the order of
    FIELDS, index sample * n_hap + hap)"""
    n_hap, total_tri, total_allele = layout["n_hap"], layout["total_tri"], layout["total_allele"]
    assert len(log_score) == n_samples * total_tri and len(gt_cov) == n_samples * total_allele and len(hap_u32) == n_samples * n_hap * 4
    phred = [None] * (n_samples * total_tri)
    out = []
    for s in range(n_samples):
        for h in range(n_hap):
            cnum = layout["hap_cnum"][h]
            n_tri = cnum * (cnum + 1) // 2
            t = s * total_tri + layout["tri_off"][h]
            a = s * total_allele + layout["allele_off"][h]
            c = (s * n_hap + h) * 4
            row, call = call_cell(log_score[t:t + n_tri], gt_cov[a:a + cnum], hap_u32[c:c + 4])
            phred[t:t + n_tri] = row
            out.append(call)
    assert None not in phred  # the triangles tile the row of a sample
    return phred, out
