"""The record walk's source (graphtyper_amd/csrc/gtx_disc_bam_walk_dev.hpp) -- guess, resolve and emit as the library launches them --
run through a sequential wave under AddressSanitizer / UBSan (tests/emu_disc_bam_walk -- a stand-alone program), against the plain
definition of what a walk leaves (tests/disc_bam_walk_cases.py): the status and its offset, the counts, every byte of the two tables,
and the segments whose guess held and those walked again.  The stream sits in a heap block of exactly its bytes and every output in a
block of exactly its size, so whatever a guessed walk meets -- decoys, damage, the stream's last bytes -- no load leaves the stream;
there is no sanitizer report.  Every set runs over 1, 2, 3 and 300 wavefronts: more segments than wavefronts and the reverse, and the
same bytes each time.  The device: test_gpu_disc_bam_walk.py."""
import functools

import pytest

import disc_bam_walk_cases as wc
import emu_programs


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_disc_bam_walk", tmp_path_factory.mktemp("emu_disc_bam_walk"))


@pytest.mark.parametrize("waves", [1, 2, 3, 300])
@pytest.mark.parametrize("name", sorted(wc.SETS))
def test_every_walk_equals_the_definition(emu, tmp_path, name, waves):
    assert wc.judge(name, functools.partial(wc.through, functools.partial(emu_programs.run, emu, tmp_path), waves)) is None


def test_a_list_that_is_no_list_is_refused(emu, tmp_path):
    data = wc.streams("align")[0].data
    for cuts in ([0], [len(data)], [100, 100], [200, 100]):
        with pytest.raises(emu_programs.Died) as e:
            wc.through(functools.partial(emu_programs.run, emu, tmp_path), 3, data, [cuts])
        assert "exit status 2" in e.value.how
