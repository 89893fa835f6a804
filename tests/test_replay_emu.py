"""The saturation replay on the host: every set of tests/replay_cases.py through the emulation backend (harness.EmuBackend: the kernel
source in replay mode, the library's mark_cells_at_guard and replay_cells) -- the log, the replayed heads and rows and the calls against
the restatement and the oracle, every other word of the accumulators as it was.  And through tests/emu_replay: the kernels' text in replay mode as the library runs it (the tables of the second
pass, the wide ones on a wide graph; a log block of exactly its capacity; a bitmap of exactly (n_cells + 31) / 32 words), then
mark_cells_at_guard and replay_cells as they are, as a stand-alone program under AddressSanitizer / UBSan.  The same on the device:
test_gpu_replay.py.  What the sets notice: test_replay_mutants.py."""
import functools

import numpy as np
import pytest

import emu_programs
import harness
import replay_cases as rc
import score_cases as sc


@functools.lru_cache(maxsize=None)
def backend(params=()):
    return harness.EmuBackend(sc.graph(), **dict(params))


def emulated(b, case, s, r, oracle, patch=None):
    """score, log, replay and calls of one case on the emulation -> the accumulators afterwards"""
    acc = b.score(case.all_items, case.records, case.n_samples, rec_words=case.rec_words)
    before = [a.copy() for a in acc.arrays()]
    entries = b.score_replay_log(case.all_items, case.records, acc, rec_words=case.rec_words, cap=1 << 21)
    assert rc.log_tuples(entries) == sorted(r.log)
    assert all(np.array_equal(x, y) for x, y in zip(before, acc.arrays())), "the log pass wrote to the accumulators"
    assert b.score_replay(case.all_items, case.records, acc, rec_words=case.rec_words) == len(r.marked)
    want = harness.Accumulators(b.ctx, case.n_samples)
    for dst, src in zip(want.arrays(), before):
        dst[...] = src
    rc.overlay(case, want, r)
    for name, x, y in zip(("log_score", "gt_cov", "hap_u32", "stat_u64", "stat_u32", "conn_log", "conn_count", "conn_near"), want.arrays(), acc.arrays()):
        assert np.array_equal(x, y), name
    assert b.score_replay(case.all_items, case.records, acc, rec_words=case.rec_words) == 0  # (a replayed cell is marked and left alone)
    if patch:
        patch(acc)
    scores, calls = oracle
    got = harness.canonical_scores(b.ctx, acc)
    assert len(got) == len(scores) and np.array_equal(got, scores)
    phred, sample_calls = b.calls(acc, case.n_samples)
    assert np.array_equal(harness.canonical_calls(b.ctx, phred, sample_calls, case.n_samples), calls)
    return acc


@pytest.mark.parametrize("name,k", rc.CASE_IDS)
def test_the_emulation_equals_both_witnesses(name, k):
    case, (s, r) = rc.cases(name)[k], rc.expected(name)[k]
    emulated(backend(case.params), case, s, r, rc.oracle_of(name, k))


def test_a_marked_cell_that_no_item_touches_keeps_its_sum_and_gets_no_mark():
    """gtx_scores_replay over the items that leave one cell at the guard without a call: that cell is not counted, its head word and
    row stay as they were, without the mark, gtx_scores_finalize reports it, and a later replay with all items still replays it"""
    case, s, r, cell, keep, partial = rc.untouched_case()
    b = backend(case.params)
    acc = b.score(case.all_items, case.records, case.n_samples, rec_words=case.rec_words)
    before = [a.copy() for a in acc.arrays()]
    assert rc.finalize_count(acc) == len(r.marked)
    assert b.score_replay(case.all_items[keep], case.records, acc, rec_words=case.rec_words) == len(r.marked) - 1
    want = harness.Accumulators(b.ctx, case.n_samples)
    for dst, src in zip(want.arrays(), before):
        dst[...] = src
    rc.overlay(case, want, partial)
    assert all(np.array_equal(x, y) for x, y in zip(want.arrays(), acc.arrays()))
    assert acc.hap_u32[4 * cell] == s.hap_u32[4 * cell] >= rc.GUARD and rc.finalize_count(acc) == 1
    assert b.score_replay(case.all_items, case.records, acc, rec_words=case.rec_words) == 1
    rc.overlay(case, want, r)
    assert all(np.array_equal(x, y) for x, y in zip(want.arrays(), acc.arrays())) and rc.finalize_count(acc) == 0


def test_the_aligners_records_and_the_wide_graph_on_the_emulation():
    """records in the arena; on the graph with a 100-allele site the emulation's replay takes the wide tables, as the library does"""
    sets = rc.aligned_replay(harness.EmuBackend)
    for a, (s, r) in zip(sets, rc.expected_aligned(sets)):
        patch = (lambda acc: rc.reference_arrays_wide(a, acc, r)) if a.name == "wide" else None
        emulated(a.b, a, s, r, rc.oracle_streams(a, a.all_items), patch)


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_replay", tmp_path_factory.mktemp("emu_replay"))


@pytest.mark.parametrize("name", rc.AUDITED)
def test_the_sanitized_program_equals_the_restatement(emu, tmp_path, name):
    """log_growth at 12 288 and 12 289 items against a first log block of 16 x 12 288 entries: filled exactly, and a second pass"""
    assert rc.judge(name, functools.partial(emu_programs.run, emu, tmp_path)) is None
