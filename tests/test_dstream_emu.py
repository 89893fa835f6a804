"""The device record stream's source (graphtyper_amd/csrc/gtx_dstream_dev.hpp) -- classify, compare, emit_tasks, walk, emit_items and
finish as the library launches them, a stable host sort and host loops in the place of the rocPRIM calls between them -- run through a
sequential wave under AddressSanitizer / UBSan (tests/emu_dstream -- a stand-alone program), against the plain definition of what a push
leaves (tests/dstream_cases.py): the status, the counts, every byte of the plane rows, the read meta and the items.  A push's records
and rows sit in heap blocks of exactly their bytes, its outputs in blocks of exactly the entries the definition leaves and the workspace
in blocks of exactly max_batch (+ parked_cap) entries, so no load or store leaves its array; there is no sanitizer report.  Every set
runs under every one of its scripts -- whole, one record a push, cut at 1, 63, 64, 65 and inside its runs and pairs -- over 1, 2, 3 and
300 wavefronts: more tiles than wavefronts and the reverse, and the same bytes each time.  The device: test_gpu_dstream.py."""
import functools

import pytest

import dstream_cases as dc
import emu_programs


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_dstream", tmp_path_factory.mktemp("emu_dstream"))


@pytest.mark.parametrize("waves", [1, 2, 3, 300])
@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_every_push_equals_the_definition(emu, tmp_path, name, waves):
    assert dc.judge(name, functools.partial(dc.through, functools.partial(emu_programs.run, emu, tmp_path), waves)) is None
