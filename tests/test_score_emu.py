"""The scoring stage on hand-made records, on the host: the case sets of tests/score_cases.py through the plain restatement
(tests/score_ref.py) and through the kernels' own text (item_is_trivial / score_item, graphtyper_amd/csrc/score_core.hpp) run as a
stand-alone program over heap blocks of exactly the arrays' sizes under AddressSanitizer / UBSan (tests/emu_score).  All values are
integers; there is no tolerance.  The device: test_gpu_score.py.  What the sets notice: test_score_mutants.py."""
import functools

import numpy as np
import pytest

import emu_programs
import harness
import score_cases as sc
import score_ref as ref
from score_cases import G


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_score", tmp_path_factory.mktemp("emu_score"))


def runner(exe, tmp_path):
    return functools.partial(emu_programs.run, exe, tmp_path)  # (no sanitizer report, or emu_programs.Died)


def test_the_double_ratio_judges_like_the_exact_one():
    """are_genotype_paths_good compares double(mismatches) / double(size) with the double literals 0.05, 0.025, 0.03 and 0.035
    (vcf_writer.cpp:38-55).  Over every (mismatches, size) with 1 <= size <= 1000 and 0 <= mismatches <= size: for 0.05, 0.025 and 0.035
    -- literals whose doubles lie ABOVE the decimal -- the double comparison gives the verdict of the exact quotient against the
    literal's exact value.  The double of 0.03 lies BELOW 3/100, and the quotients that are exactly 3/100 round to that very double:
    for (3k, 100k) the double comparison says "not above" where the exact one says "above".  Nowhere else do the two differ.  The
    reference's double arithmetic is the definition, so the restatement (score_ref.ratio_exceeds) compares the correctly rounded
    quotient -- a read with 3 mismatches in 100 bases is good on an SV graph."""
    differ = {}
    for literal in ref.THRESHOLDS:
        num, den = ref.Fraction(literal).as_integer_ratio()
        for size in range(1, 1001):
            m = np.arange(size + 1)
            rounded = (m.astype(np.float64) / np.float64(size)) > np.float64(literal)
            exact = np.array([int(x) * den > num * size for x in m])
            for x in np.nonzero(rounded != exact)[0]:
                differ.setdefault(literal, []).append((int(x), size, bool(rounded[x])))
    assert differ == {0.03: [(3 * k, 100 * k, False) for k in range(1, 11)]}
    for m, s, lit in ((5, 100, 0.05), (6, 100, 0.05), (3, 120, 0.025), (3, 100, 0.03), (7, 200, 0.035), (4, 100, 0.03), (9, 300, 0.03)):
        assert ref.ratio_exceeds(m, s, lit) == (float(m) / float(s) > lit)
    assert not ref.ratio_exceeds(3, 100, 0.03) and ref.ratio_exceeds_unrounded(3, 100, 0.03) and not ref.ratio_exceeds_unrounded(5, 100, 0.05)


def test_the_restatement_by_hand():
    """three items worked out by hand from the reference's text"""
    f = sc.facts()
    nh = f.n_hap
    # one read, forward, 1 mismatch, on allele 2 of site 1 (3 alleles): epsilon 12 - 1 = 11 -> 7; genotypes 0/2 and 1/2 get 6, 2/2 gets 7
    c = sc.Case()
    c.single(c.read(G(150, [(1, [2])], mm=1)), mapq=60, score_diff=9)
    s = ref.score(f, c.par, c.records, c.rec_words, c.items, 1)
    t, a = f.tri_off[1], f.allele_off[1]
    assert dict(s.log_score) == {t + 3: 6, t + 4: 6, t + 5: 7} and dict(s.gt_cov) == {a + 2: 1} and dict(s.hap_u32) == {4: 7}
    assert dict(s.stat_u64) == {1: 3600, nh + 2 * (a + 2) + 1: 3600}
    assert dict(s.stat_u32) == {nh + 6 * (a + 2) + 0: 9, nh + 6 * (a + 2) + 1: 6, nh + 6 * (a + 2) + 4: 1} and not s.conn_log and not s.conn_near
    # the same read clipped by 30 bases with mapq 24 on two near sites: epsilon 12 - 1 - 2 - 3 = 6 -> 4 (the floor), one connection
    c = sc.Case()
    c.single(c.read(G(120, [(1, [2]), (0, [0, 1])], mm=1)), mapq=24, flag=sc.FIRST)
    s = ref.score(f, c.par, c.records, c.rec_words, c.items, 1)
    assert dict(s.hap_u32) == {0: 4, 1: 1, 4: 4}  # site 0: ambiguous with the reference; site 1: allele 2
    assert s.stat_u32[0] == 1 and s.stat_u32[1] == 1 and s.stat_u64[nh + 2 * (a + 2)] == 200 and s.stat_u64[0] == 576  # 30 * 1000 / 150
    width = f.allele_off[f.near_last[0]] + f.hap_cnum[f.near_last[0]] - f.allele_off[1]
    assert dict(s.conn_near) == {f.near_off[0] + 0 * width + 2: 1, f.near_off[0] + 1 * width + 2: 1} and not s.conn_log  # weight 2: repeat 1
    # a proper pair: mate 1 on alt allele 1 of site 3, mate 2 on site 25 (far): one cross link in the log, alt_proper_pair_depth on both
    c = sc.Case()
    c.pair(c.read(G(150, [(3, [1])])), c.read(G(0), G(150, [(25, [1])])))
    s = ref.score(f, c.par, c.records, c.rec_words, c.items, 1)
    assert dict(s.conn_log) == {(0, 3, 1, 25, 1, 1): 1} and s.hap_u32[3 * 4 + 3] == 1 and s.hap_u32[25 * 4 + 3] == 1 and s.hap_u32[3 * 4] == 8
    assert s.items[0]["rule"] == "perfect_one" and [r["flags"] for r in s.items[0]["reads"]] == [1 | 2 | 64, 1 | 2 | 16 | 128]
    with pytest.raises(ValueError):  # longest_path_length is not what the paths say
        bad = sc.Case()
        g = G(150, [(0, [1])])
        g["paths"].append((g["paths"][0][0], g["paths"][0][1], 0, 99, 0, []))
        bad.single(bad.read(g))
        ref.score(f, bad.par, bad.records, bad.rec_words, bad.items, 1)


@pytest.mark.parametrize("name", sc.SETS)
def test_the_set_holds_what_it_is_for(name):
    sc.FACTS[name](sc.cases(name), sc.expected(name))


@pytest.mark.parametrize("name", sc.SANITIZED)
def test_the_oracle_equals_the_restatement(name):
    """the second witness: the oracle's scoring (oracle/gto.hpp) over the same hand-made paths, through harness.canonical_scores (which
    applies the reference's u8 / u16 clamps to the restatement's sums)"""
    for k, case in enumerate(sc.cases(name)):
        keep = sc.held_to_the_oracle(case)
        items = case.items[keep]
        want = sc.restate(case, items, None if case.mult is None else [case.mult[i] for i in keep])
        got = sc.oracle_scores(case, items)
        canonical = harness.canonical_scores(sc.host_ctx(case.params), sc.dense_arrays(case, want))
        assert len(got) == len(canonical), k
        bad = np.nonzero(got != canonical)[0]
        assert len(bad) == 0, (k, bad[:5], got[bad[:5]], canonical[bad[:5]])


@pytest.mark.parametrize("name", sc.SANITIZED)
def test_every_array_equals_the_restatement(emu, tmp_path, name):
    assert sc.judge(name, runner(emu, tmp_path)) is None
    for k, (case, want) in enumerate(zip(sc.cases(name), sc.expected(name))):  # (once more for the message)
        got = sc.through(runner(emu, tmp_path), case, want)
        assert sc.differences(case, want, got) == [] and got.errors == 0, k


def test_many_items_at_the_size_that_runs_under_the_sanitizers(emu, tmp_path):
    case, items, want = sc.sanitized_many_items()
    assert len(items) == 4099 and sum(len(it["reads"]) for it in want.items) > 2000  # (distinct items that occur among them)
    got = sc.through(runner(emu, tmp_path), case, want, items)
    assert sc.differences(case, want, got) == [] and got.errors == 0


def test_the_emulation_library_agrees():
    """harness.EmuBackend.score (tests/emu/libgtx_emu.so, what the CPU suite's scenarios go through) on two of the sets"""
    for name in ("site_tables", "goodness"):
        for case, want in zip(sc.cases(name), sc.expected(name)):
            b = harness.EmuBackend(sc.graph(), **dict(case.params))
            acc = b.score(case.items, case.records, case.n_samples, rec_words=case.rec_words, near=case.near)
            got = sc.Got(log_score=acc.log_score, gt_cov=acc.gt_cov, hap_u32=acc.hap_u32, stat_u64=acc.stat_u64, stat_u32=acc.stat_u32,
                         conn_near=acc.conn_near, conn_log=acc.conn_log.reshape(-1, 6), conn_count=acc.conn_count)
            assert sc.differences(case, want, got, conn_cap=acc.conn_cap) == []


def test_aligned_records_on_the_host(emu, tmp_path):
    """records in the arena (rec_words = 8) and records with wide allele sets, made by the aligner, under hand-made items: the
    restatement == the oracle over the same words and arena == the emulation library == the kernels' text under the sanitizers"""
    sets, exp = sc.aligned_on_the_emulation()
    sc.facts_aligned_records(sets, exp)
    for a, want in zip(sets, exp):
        got, acc = a.backend_score()
        assert sc.differences(a, want, got, conn_cap=acc.conn_cap) == [], a.name
        oracle = sc.oracle_scores(a, a.items)
        assert np.array_equal(harness.canonical_scores(a.ctx, sc.dense_arrays(a, want)), oracle), a.name
        assert np.array_equal(harness.canonical_scores(a.ctx, acc), oracle), a.name
        got = sc.through(runner(emu, tmp_path), a, want)
        assert sc.differences(a, want, got) == [] and got.errors == 0, a.name
