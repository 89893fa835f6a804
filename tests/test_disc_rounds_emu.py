"""The rounds' kernel source (graphtyper_amd/csrc/gtx_disc_rounds_dev.hpp, with gtx_disc_second_dev.hpp for a round's pairs and
gtx_realign_dev.hpp for the alignments) run through a sequential wave under AddressSanitizer / UBSan (tests/emu_disc_rounds -- a
stand-alone program), against the plain restatement (tests/disc_rounds_ref.py), through disc_rounds_cases.judge -- the judge of the
mutation audit (tests/disc_rounds_mutants), so that the audit and these tests ask the same of the same names.  Per case the whole
list and every [0, k): the reads' state, each read's list, the six counters (against the restatement after every round, and
against the holders of the program's own lists), the statistics against the restatement's trace, and every window, ref_pos value
and applied flag against gtx_disc_realign_target.  Every array is a heap block of exactly its size -- a round's arena exactly the
sum of its slots -- and there is no sanitizer report.  All values are integers; there is no tolerance.  The device:
test_gpu_disc_rounds.py."""
import functools

import pytest

import disc_rounds_cases as rc
import emu_programs
from test_disc_rounds_cases import ALL, case_of


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_rounds", tmp_path_factory.mktemp("emu_disc_rounds"))


@pytest.fixture
def run(emu, tmp_path):
    return functools.partial(emu_programs.run, emu, tmp_path)


def test_the_judge_knows_what_the_tests_run():
    assert sorted({name for name, _ in ALL}) == sorted(rc.SETS) + sorted(rc.SHAPES) and len(set(rc.NAMES)) == len(rc.NAMES)


@pytest.mark.parametrize("name,k", ALL)
def test_every_case_equals_the_restatement(run, name, k):
    assert rc.case_differs(run, case_of(name, k)) is None


@pytest.mark.parametrize("name", rc.LAUNCHES)
def test_slices_and_the_event_array(run, name):
    """[0, k) then -- from the restatement's state in front of round k -- [k, n), for every k; the array exactly large enough (with
    compactions where the lists ever made need more) and one entry short: status 5, events_wanted, the state in front of the round
    that does not fit; a table entry whose letters are not there; lists that share their entries"""
    assert rc.judge(name, run) is None


def test_the_final_decision(run):
    assert rc.judge("decide", run) is None
