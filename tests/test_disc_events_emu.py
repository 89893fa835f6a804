"""The discovery events kernel's source (graphtyper_amd/csrc/gtx_disc_events_dev.hpp) run 64 reads at a time through a sequential
wave under AddressSanitizer / UBSan (tests/emu_disc_events -- a stand-alone program), against the plain restatement of the
reference's walk (tests/disc_events_ref.py) and against the oracle (oracle/gto_discovery.hpp), event by event: per read its state,
n_events, pos_end and the events [first_event, first_event + n_events) in order, every field.  All values are integers; there is
no tolerance.  Every read runs over heap blocks of exactly its sizes, the event buffer has exactly event_cap entries, and there
is no sanitizer report.  Then the launch-level conditions that need no device: the tiling of the event buffer, its capacity,
counters that are not zero at entry.  The device: test_gpu_disc_events.py."""
import functools

import numpy as np
import pytest

import disc_event_cases as dc
import disc_events_ref as ref
import emu_programs


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_events", tmp_path_factory.mktemp("emu_disc_events"))


def run_emu(exe, tmp_path, part, event_cap, counts=(0, 0), launches=1):
    return dc.through(functools.partial(emu_programs.run, exe, tmp_path), part, event_cap, counts, launches)


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_the_set_holds_what_it_is_for(name):
    dc.FACTS[name](dc.expected(name))


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_the_oracle_equals_the_restatement(name):
    """the two statements of the reference's walk, held to each other; the oracle's pass ends at the first GTX_DISC_END read, as the
    reference's does, so the reads behind one are the restatement's alone"""
    for k, (part, want) in enumerate(zip(dc.parts(name), dc.expected(name))):
        got = dc.oracle_events(part)
        upto = dc.before_the_end(want)
        wrong = [(k, i, got[i], want[i]) for i in range(upto) if got[i] != want[i]]
        assert wrong == [], wrong[:3]
        assert all(row[:3] == (ref.SKIPPED, 0, 0) for row in got[upto:])


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_every_event_equals_the_restatement(emu, tmp_path, name):
    for k, (part, want) in enumerate(zip(dc.parts(name), dc.expected(name))):
        total = dc.total_events(want)
        counts, read_out, events = run_emu(emu, tmp_path, part, total)
        got = dc.per_read(read_out, events)
        wrong = [(k, i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
        assert wrong == [], wrong[:3]
        assert dc.check_launch(want, counts, read_out, events, total) == 0 and tuple(counts) == (total, 0)


@pytest.mark.parametrize("n_reads", dc.TILING_READS)
def test_the_pieces_tile_the_event_buffer(emu, tmp_path, n_reads):
    part, want = dc.tiling_part(n_reads), dc.tiling_expected(n_reads)
    total = dc.total_events(want)
    counts, read_out, events = run_emu(emu, tmp_path, part, total)
    assert dc.check_launch(want, counts, read_out, events, total) == 0 and (n_reads < 2 or total > 0)


@pytest.mark.parametrize("cap", ["total", "total - 1", "1", "0"])
def test_a_read_fits_or_is_counted_as_overflow(emu, tmp_path, cap):
    """event_cap of all events, one fewer, 1 and 0 (no event buffer at all): the buffer has exactly event_cap entries, so a store behind
    it stops the program"""
    part, want = dc.tiling_part(257), dc.tiling_expected(257)
    total = dc.total_events(want)
    event_cap = eval(cap, dict(total=total))
    counts, read_out, events = run_emu(emu, tmp_path, part, event_cap)
    lost = dc.check_launch(want, counts, read_out, events, event_cap)
    assert (lost == 0) == (cap == "total") and (cap != "0" or int(counts[1]) == total)
    if cap == "1":  # the one read with a single event that comes first fits
        assert sum(1 for ro in read_out if ro["n_events"] and ro["first_event"] + ro["n_events"] <= 1) == 1


def test_counters_that_are_not_zero_at_entry(emu, tmp_path):
    part, want = dc.tiling_part(130), dc.tiling_expected(130)
    total = dc.total_events(want)
    counts, read_out, events = run_emu(emu, tmp_path, part, 7 + total, counts=(7, 3))
    assert dc.check_launch(want, counts, read_out, events, 7 + total, (7, 3)) == 0 and tuple(counts) == (7 + total, 3)
    assert (events[:7].view(np.uint8) == 0xA5).all()  # nobody's
    # two launches in a row on one event buffer accumulate: the second one's pieces lie behind the first one's
    counts, read_out, events = run_emu(emu, tmp_path, part, 2 * total, launches=2)
    assert dc.check_launch(want, counts, read_out, events, 2 * total, (total, 0)) == 0 and tuple(counts) == (2 * total, 0)
    assert (events[:total]["read"] < 130).all() and (events[:total]["reserved"] == 0).all()  # the first launch's events are still there
