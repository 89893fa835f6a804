"""The call stage on hand-made accumulators, on the host: the case sets of tests/calls_cases.py through three statements of the
reference's call -- the plain restatement (tests/calls_ref.py), the oracle (oracle/gto.hpp sample_calls(), its HapSamples set by
hand) and the kernel's own text (call_cell, graphtyper_amd/csrc/score_core.hpp) run as a stand-alone program over heap blocks of
exactly the arrays' sizes under AddressSanitizer / UBSan (tests/emu_calls).  All values are integers; there is no tolerance.
The device: test_gpu_calls.py.  What the sets notice: test_calls_mutants.py."""
import decimal
import functools

import numpy as np
import pytest

import calls_cases as cc
import calls_ref as ref
import emu_programs
import harness
import scenarios
from graphtyper_amd import lib as gtx
from oracle_lib import Oracle

@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_calls", tmp_path_factory.mktemp("emu_calls"))


def run_emu(exe, tmp_path, case):
    return cc.through(functools.partial(emu_programs.run, exe, tmp_path), case)  # (no sanitizer report, or emu_programs.Died)


def test_the_double_product_rounds_like_the_exact_one():
    """PL = llround(double(delta) * 3.0102999566398119...) in the reference and in call_cell; the restatement rounds the exact product.
    For every delta a uint16 row can hold the two are the same integer: the exact product is never closer than 1.4e-5 to a half
    (closest at delta 48 107), and the double product is off by less than 3e-11 -- the constant by half an ulp of [2, 4), 2^-52,
    times 65 535 = 1.5e-11; the product, below 2^18, by half an ulp, 2^-36 = 1.5e-11 -- so both lie on the same side.
    84 -> 253 and 85 -> 256: 254 is never a PL and 85 is the first delta at the cap."""
    c = float("3.01029995663981195213738894724493026768189881462108541")  # the literal of vcf.cpp:73
    half = decimal.Decimal("0.5")
    margin, at = None, None
    for delta in range(0x10000):
        product = float(delta) * c  # (IEEE double, as in C++)
        assert int(decimal.Decimal(product).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP)) == ref.pl_exact(delta), delta
        exact = decimal.Decimal(delta) * ref.TEN_LOG10_2
        away = abs(exact - exact.to_integral_value(rounding=decimal.ROUND_FLOOR) - half)
        assert abs(decimal.Decimal(product) - exact) < decimal.Decimal("3e-11")
        if margin is None or away < margin:
            margin, at = away, delta
    assert at == 48107 and decimal.Decimal("1.4e-5") < margin < decimal.Decimal("1.5e-5"), (at, margin)
    assert (ref.pl_exact(84), ref.pl_exact(85), ref.pl_of(84), ref.pl_of(85), ref.pl_of(65535)) == (253, 256, 253, 255, 255)
    assert abs(ref.TEN_LOG10_2 - decimal.Decimal("3.01029995663981195213738894724493026768189881462108541")) < decimal.Decimal("1e-50")


def test_the_restatement_by_hand():
    """three cells worked out by hand from the reference's text"""
    # scores 10, 7, 10 over 2 alleles: PL 0, 9, 0 -> GT 0/0 (the first zero), GQ 0; depths 5 + 3 - 1 and 2 + 3
    assert ref.call_cell([10, 7, 10], [5, 2], [0x80000009, 3, 1, 4]) == ([0, 9, 0], (0, 0, 7, 5, 0, 3, 4))
    # all equal and not zero: all PL 0
    assert ref.call_cell([9, 9, 9], [0, 0], [0, 0, 0, 0]) == ([0, 0, 0], (0, 0, 0, 0, 0, 0, 0))
    # maximum on 1/1 by 84, 85: PL 253, 255, 0 -> GQ 253; both ambiguous counters stop at 255 on their own; the sums stop at 0xFFFF
    assert ref.call_cell([916, 915, 1000], [0xFFFF, 0x12345], [0, 300, 280, 256]) == ([253, 255, 0], (1, 1, 0xFFFF, 0xFFFF, 253, 255, 255))
    assert ref.call_cell([916, 915, 1000], [0, 7], [0, 300, 280, 256])[1][2:4] == (0, 262)
    with pytest.raises(ValueError):
        ref.call_cell([0x10000, 0, 0], [0, 0], [0, 0, 0, 0])


@pytest.mark.parametrize("name", cc.SETS)
def test_the_set_holds_what_it_is_for(name):
    cc.FACTS[name](cc.expected(name))


@pytest.mark.parametrize("name", cc.SANITIZED)
def test_the_oracle_equals_the_restatement(name):
    for k, (case, (phred, calls)) in enumerate(zip(cc.cases(name), cc.expected(name))):
        got, want = cc.oracle_calls(case), cc.canonical(case, phred, calls)
        assert len(got) == len(want)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (k, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", cc.SANITIZED)
def test_every_field_equals_the_restatement(emu, tmp_path, name):
    for k, (case, want) in enumerate(zip(cc.cases(name), cc.expected(name))):
        got = run_emu(emu, tmp_path, case)
        assert cc.differences(case, want, got) == [], k


def test_many_cells_at_the_size_that_runs_under_the_sanitizers(emu, tmp_path):
    (case,) = cc.make_many_cells(cc.MANY_CELLS_SAMPLES_SANITIZED)
    assert case.cells() == 2052
    assert cc.differences(case, cc.restate(case), run_emu(emu, tmp_path, case)) == []


def test_the_emulation_library_agrees(tmp_path):
    """harness.EmuBackend.calls (tests/emu/libgtx_emu.so, what the CPU suite's scenarios go through) on two of the sets"""
    for name in ("depth_clamps", "layout"):
        for case, want in zip(cc.cases(name), cc.expected(name)):
            b = harness.EmuBackend(cc.graph(case.key))
            acc = harness.Accumulators(b.ctx, case.n_samples)
            acc.log_score[:], acc.gt_cov[:], acc.hap_u32[:] = case.log_score, case.gt_cov, case.hap_u32
            assert cc.differences(case, want, b.calls(acc, case.n_samples)) == []


# ---- the pooled tail: a state in which the reference itself reaches a clamp ---------------------------------------------------------
def pooled_tail_inputs():
    rb = 500000
    return (rb,) + scenarios.paired_case("snp100", n_ref=3000, n_pairs=260, region_begin=rb, n_samples=2)


def pooled_tail_case(Backend):
    """A small paired run merged k times into one oracle genotyper (Genotyper::merge_from adds, and stops the u8 / u16 counters as the
    reference's increments do) against the product's accumulators times k: some cell's raw ambiguous depth and some cell's raw
    alt-proper-pair depth pass 255 while every max_log_score * k stays under the guard of explain_to_score."""
    rb, ref_s, recs, codes, rec = pooled_tail_inputs()
    o = Oracle(ref_s, recs, region_begin=rb)
    b = Backend(gtx.graph_from_records(ref_s, recs, region_begin=rb))
    st = gtx.Stream(b.ctx.params, 1)
    a_seq, a_meta, items = st.push(rec, gtx.pack_nibbles(codes))
    acc = b.score(items, b.align(a_seq, a_meta), 2)
    cells = acc.hap_u32.reshape(-1, 4).astype(np.int64)
    k = int((0xFFFF - 9) // cells[:, 0].max())  # the largest k that keeps every cell under the guard
    assert k >= 2 and (cells[:, 0] * k < 0xFFFF - 8).all()
    assert (cells[:, 1] * k > 255).any() and (cells[:, 3] * k > 255).any(), (k, cells.max(axis=0))
    og = o.genotyper(2, 1)
    for _ in range(k):
        part = o.genotyper(2, 1)
        part.push(list(codes), flags=rec["flag"], tid=rec["tid"], mtid=rec["mtid"], pos=rec["pos"], isize=rec["isize"], mapq=rec["mapq"],
                  score_diff=rec["score_diff"], name=rec["name_id"], sample=rec["sample"], rg=rec["rg"])
        og.merge(part)
    for a in (acc.log_score, acc.gt_cov, acc.hap_u32, acc.stat_u64, acc.stat_u32):
        a *= k
    phred, calls = b.calls(acc, 2)
    assert (calls["ambiguous_depth"] == 255).any() and (calls["alt_proper_pair_depth"] == 255).any()
    assert np.array_equal(harness.canonical_calls(b.ctx, phred, calls, 2), og.calls())
    want = cc.restate_arrays(b.ctx, 2, acc.log_score, acc.gt_cov, acc.hap_u32)
    assert np.array_equal(phred, want[0]) and np.array_equal(calls, want[1])
    names = ["POOL0", "POOL1"]
    text = b.ctx.vcf_records("chrT", names, acc.gt_cov, acc.stat_u64, acc.stat_u32, phred, calls)
    assert text == og.vcf_records("chrT", names) and text.count(b"\n") == b.ctx.n_hap + 1


def test_the_pooled_tail_on_the_emulation():
    pooled_tail_case(harness.EmuBackend)
