"""The unpack kernel's source (graphtyper_amd/csrc/gtx_disc_bam_dev.hpp) run record by record through a sequential wave under
AddressSanitizer / UBSan (tests/emu_disc_bam -- a stand-alone program), against the plain definition of its three outputs
(tests/disc_bam_cases.py): every byte of the plane rows, the quality rows and the CIGAR words.  Every record's stream bytes sit in a
heap block of exactly the record's size and every record's outputs in blocks of exactly their sizes; the program then runs the text
once more over the launch's own arrays (BamBatch: the stream in one block, every record at its own address residue) and insists on
the same bytes; there is no sanitizer report.  The records run over three wavefronts, so that a wavefront takes several.  The device:
test_gpu_disc_bam.py."""
import functools

import pytest

import disc_bam_cases as bc
import emu_programs


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_bam", tmp_path_factory.mktemp("emu_disc_bam"))


@pytest.mark.parametrize("name", sorted(bc.SETS))
def test_every_byte_equals_the_definition(emu, tmp_path, name):
    assert bc.judge(name, functools.partial(bc.through, functools.partial(emu_programs.run, emu, tmp_path))) is None


@pytest.mark.parametrize("waves", [1, 2, 64, 300])
def test_the_records_over_any_number_of_wavefronts(emu, tmp_path, waves):
    """one wavefront for all 257 records, more wavefronts than records"""
    f = bc.files("counts")[-1]
    g = bc.File(f.records, waves=waves)
    assert bc.file_differs(g, bc.through(functools.partial(emu_programs.run, emu, tmp_path), g)) is None
