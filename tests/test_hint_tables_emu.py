"""The host build of the position-hinted pass' tables (gtx_host.cpp over index_build.hpp) as a stand-alone program under
AddressSanitizer / UBSan (tests/emu_hint_tables), every set of tests/hint_tables_cases.py through hint_tables_cases.judge -- the judge
of the mutation audit (tests/hint_tables_mutants), so that the audit and these tests ask the same of the same names: all seven tables
equal the restatement word for word, and there is no sanitizer report."""
import functools

import pytest

import emu_programs
import hint_tables_cases as tc


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_hint_tables", tmp_path_factory.mktemp("emu_hint_tables"))


@pytest.fixture
def run(emu, tmp_path):
    return functools.partial(emu_programs.run, emu, tmp_path)


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_set_equals_the_restatement(run, name):
    assert tc.judge(name, run) is None
