"""graphtyper_amd/csrc/gtx_disc_variants.cpp as a stand-alone program under AddressSanitizer / UBSan (tests/emu_disc_variants): every
case set of tests/disc_variants_cases.py through gtx_disc_variants and gtx_disc_vcf_sites with heap blocks of exactly their sizes for
every input and output, and again with each output one entry short -- GTX_ERR_CAPACITY, the sizes, nothing else written.  The
records, the letters, the ids and the text equal the plain restatement (tests/disc_variants_ref.py) field for field and byte for
byte, and there is no sanitizer report.  Nothing is loaded into Python under a sanitizer."""
import functools

import pytest

import disc_variants_cases as vc
import emu_programs


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_variants", tmp_path_factory.mktemp("emu_disc_variants"))


@pytest.mark.parametrize("name", sorted(vc.SETS))
def test_every_set_equals_the_restatement(emu, tmp_path, name):
    assert vc.judge(name, functools.partial(emu_programs.run, emu, tmp_path)) is None


def test_the_program_equals_the_library(emu, tmp_path):
    """the same bytes from the program and from libgtx.so's entry points (one source file, two builds)"""
    for name in ("first_base", "same_place"):
        for case in vc.cases(name):
            a, b = vc.through(functools.partial(emu_programs.run, emu, tmp_path), case), vc.through_lib(case)
            assert a["recs"].tobytes() == b["recs"].tobytes() and bytes(a["letters"]) == bytes(b["letters"]) and bytes(a["text"]) == bytes(b["text"])
            assert a["ids"].tolist() == b["ids"].tolist()


def test_words_that_do_not_parse_stop_the_program_with_the_librarys_message(emu, tmp_path):
    """a cut word stream: the program reports GTX_ERR_ARG's message and no sanitizer finding (no read behind the words)"""
    case = vc.cases("sets")[0]
    words = vc.arrays(case)["words"]
    for cut in (1, 3, len(words) // 2, len(words) - 1):
        short = vc.Case(case.reference, case.region_begin, case.table, case.haps, case.bits)
        vc.arrays(short)["words"] = words[:cut].copy()  # (the dict that arrays() keeps for this case)
        with pytest.raises(emu_programs.Died) as died:
            vc.through(functools.partial(emu_programs.run, emu, tmp_path), short)
        assert "exit status 3" in died.value.how and "not a result of gtx_disc_merge" in str(died.value) and "Sanitizer" not in str(died.value)
