"""The saturation replay's two witnesses before any kernel is asked: every set of tests/replay_cases.py reaches what it is for (the
fact tests, from the restatement's output), and the oracle -- the items one by one, in order, through its guarded explain_to_score
(OracleGenotyper.push_paths) -- gives what the restatement (score_ref.score + score_ref.replay) gives, cell by cell."""
import time

import numpy as np
import pytest

import harness
import replay_cases as rc
import score_cases as sc


@pytest.mark.parametrize("name", rc.SETS)
def test_the_set_reaches_what_it_is_for(name):
    rc.FACTS[name](rc.cases(name), rc.expected(name))


@pytest.mark.parametrize("name,k", rc.CASE_IDS)
def test_the_oracle_gives_what_the_restatement_gives(name, k):
    case, (s, r) = rc.cases(name)[k], rc.expected(name)[k]
    assert len(rc.cases(name)) == rc.N_CASES[name]
    want = harness.canonical_scores(sc.ctx_of(case), rc.expected_arrays(case, s, r))
    got, _ = rc.oracle_of(name, k)
    assert len(got) == len(want) and np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_the_walk_over_a_million_calls_takes_seconds():
    """log_growth: the restatement's sequential walk over 2^20 calls, timed (about a second of CPU)"""
    case = rc.cases("log_growth")[0]
    s = rc.expected("log_growth")[0][0]
    t0 = time.process_time()
    r = rc.ref.replay(s, case.sequence.tolist())
    took = time.process_time() - t0
    print("replay of %d calls: %.2f s" % (len(r.log), took))
    assert len(r.log) == 1 << 20


@pytest.fixture(scope="module")
def aligned():
    sets = rc.aligned_replay(harness.EmuBackend)
    return sets, rc.expected_aligned(sets)


def test_the_aligners_records_reach_what_they_are_for(aligned):
    rc.FACTS_ALIGNED(*aligned)


def test_the_oracle_gives_what_the_restatement_gives_on_the_aligners_records(aligned):
    """records in the arena, and a graph with a 100-allele site: there the oracle also confirms the restatement's guarded value of the one
    cell that the library does not replay"""
    (ext, wide), exp = aligned
    for a, (s, r) in zip((ext, wide), exp):
        acc = rc.expected_arrays(a, s, r)
        if a is wide:
            rc.reference_arrays_wide(wide, acc, r)
        want = harness.canonical_scores(a.ctx, acc)
        got, _ = rc.oracle_streams(a, a.all_items)
        assert len(got) == len(want) and np.array_equal(got, want), (a.name, np.nonzero(got != want)[0][:10])
