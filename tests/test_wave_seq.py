"""The sequential side of the wave policy (tests/wave_seq.hpp), the one stand-in every host emulation of a kernel's text runs on, held
to the policy's contract (graphtyper_amd/csrc/graph_dev.hpp: the table): the probe's text (wave_probe.hpp) as a stand-alone program
under AddressSanitizer / UBSan (tests/emu_wave) against the plain statement of tests/wave_probe_cases.py, word for word.
The hardware side, on the same sets against the same statement: test_gpu_wave.py."""
import functools
import os
import re

import numpy as np
import pytest

import emu_programs
import wave_probe_cases as wc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graphtyper_amd", "csrc", "wave_probe.hpp")


@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return emu_programs.build("emu_wave", tmp_path_factory.mktemp("emu_wave"))


def through(run, n):
    def write(path):
        with open(path, "wb") as f:
            f.write(np.array([n], dtype=np.uint32).tobytes() + wc.case_words(n).tobytes())
    return run(write, lambda path: np.fromfile(path, dtype=np.uint32))


def test_the_layout_is_the_headers():
    text = open(HEADER).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bWP_(IN_\w+|OUT_\w+) = (\d+)\b", text)}
    want = {"IN_" + k: v for k, v in wc.IN.items()}
    want.update({"OUT_" + k: v for k, v in wc.OUT.items()})
    assert got == want


def test_the_definition_by_hand():
    """the lane-index set worked out by hand: a = 0 .. 63, b = 1 .. 64, all lanes flagged, k = 79 (lane 15), first 1000, counters at 0"""
    s = next(s for s in wc.SETS if s.name == "lane_index")
    o, O = wc.expected(s), wc.OUT
    assert list(o[O["SHIFT"]:O["SHIFT"] + 4]) == [1000, 0, 1, 2] and o[O["SHIFT"] + 63] == 62
    assert list(o[O["SHIFT2"]:O["SHIFT2"] + 4]) == [1000, 1000, 0, 1] and o[O["SHIFT2"] + 63] == 61
    assert list(o[O["SCAN"]:O["SCAN"] + 5]) == [0, 0, 1, 3, 6] and o[O["SCAN"] + 63] == 1953
    assert (o[O["SCAN_TOTAL"]], o[O["SUM"]], o[O["MAX"]], o[O["FROM_LANE"]], o[O["UNI32"]]) == (2016, 2016, 63, 15, 1000 ^ 15)
    assert (o[O["BALLOT"]], o[O["BALLOT"] + 1]) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert list(o[O["CLAIM"]:O["CLAIM"] + 64]) == [0] * 64 and o[O["CLAIM_CTR"]] == 1000
    assert list(o[O["ACLAIM"]:O["ACLAIM"] + 64]) == list(range(64)) and o[O["ACLAIM_CTR"]] == 64
    assert (o[O["ADD32"]], o[O["SUB32"]], o[O["MAXU32"]], o[O["MAXI32"]], o[O["OR32"]]) == (2080, 2**32 - 2080, 64, 64, 127)
    assert (o[O["ADD64"]], o[O["ADD64"] + 1], o[O["OR64"]], o[O["OR64"] + 1]) == (2080, 2016, 127, 63)


def test_the_sets_hold_what_they_are_for():
    names = [s.name for s in wc.SETS]
    assert len(set(names)) == len(names) and max(wc.COUNTS) == len(names) and set(wc.COUNTS) >= {1, 4, 5}
    at_max = {s.a.index(max(s.a)) for s in wc.SETS if s.name.startswith("max_at_") and s.a.count(max(s.a)) == 1}
    assert at_max == set(wc.EDGE_LANES) and {s.k for s in wc.SETS} >= set(wc.EDGE_LANES)
    masks = {sum(1 << l for l in range(64) if s.flag[l]) for s in wc.SETS}
    assert {0, 2**64 - 1, 1, 1 << 63, 0xAAAAAAAAAAAAAAAA} <= masks and len(masks) >= 6
    assert any(sum(s.a) > wc.M32 for s in wc.SETS) and any(s.a == list(range(64)) for s in wc.SETS) and any(len(set(s.a)) == 1 for s in wc.SETS)


@pytest.mark.parametrize("n", wc.COUNTS)
def test_the_sequential_wave_equals_the_definition(emu, tmp_path, n):
    got = through(functools.partial(emu_programs.run, emu, tmp_path), n)  # (no sanitizer report, or emu_programs.Died)
    assert wc.differences(n, got) == []
