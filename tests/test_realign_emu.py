"""The realignment kernel's source (graphtyper_amd/csrc/gtx_realign_dev.hpp) run pair by pair through a sequential wave under
AddressSanitizer / UBSan (tests/emu_realign), against the plain restatement of the alignment's definition (tests/realign_ref.py):
every field of every result is equal -- all values are integers, there is no tolerance -- and there is no sanitizer report.
Every pair within the limits runs over heap blocks of exactly its sizes.  The device: test_gpu_realign.py."""
import os
import subprocess

import numpy as np
import pytest

import realign_cases as rc
from graphtyper_amd import lib as gtx

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="session")
def emu_realign(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_realign") / "emu_realign")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_realign"), "-s", "OUT=" + out])
    return out


def run_emu(emu, tmp_path, reads, targets, pairs):
    planes, plane_stride, lens, seq, off, pr = rc.arrays(reads, targets, pairs)
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(np.array([plane_stride, len(reads), len(targets), len(pr), len(seq)], np.uint32).tobytes())
        f.write(planes.tobytes())
        f.write(lens.tobytes() + b"\0\0" * (len(lens) & 1))
        f.write(off.tobytes())
        f.write(seq.tobytes() + b"\0" * (-len(seq) % 4))
        f.write(pr.tobytes())
    subprocess.run([emu, case, out], check=True, stdout=subprocess.DEVNULL, timeout=600)
    return rc.as_tuples(np.fromfile(out, gtx.REALIGN_RESULT))


@pytest.mark.parametrize("name", sorted(rc.SETS))
def test_every_field_equals_the_restatement(emu_realign, tmp_path, name):
    reads, targets, pairs = rc.get(name)
    got, want = run_emu(emu_realign, tmp_path, reads, targets, pairs), rc.expected(name)
    assert len(got) == len(want)
    wrong = [(i, pairs[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert wrong == [], wrong[:5]


def test_the_sets_hold_what_they_are_for():
    """the hand-made sets do reach the paths they are named after"""
    want = rc.expected("mismatch_runs_and_clips")
    reads, _, pairs = rc.get("mismatch_runs_and_clips")
    # a run of 12 mismatches: an insertion plus a deletion (2 * (7 + 11) = 36 lost; chance matches may give a little back) beats
    # pairing them (12 * 4 = 48 lost) and beats the clip
    assert want[2][0] >= 100 - 12 - 2 * (7 + 11) > 100 - 12 - 48 and (want[2][1], want[2][2]) == (0, 100)
    clipped = [w for w, p in zip(want, pairs) if w[1] > 0 or w[2] < len(reads[p[0]])]
    assert 5 <= len(clipped) < len(want) - 5  # some clips win, some lose
    assert {w[5] for w in rc.expected("bad_and_long")} == {0, 1, 2}
    n = len(rc.get("no_padding")[1][0])
    assert all(w[3] == 0 or w[4] == n for w in rc.expected("no_padding")[:5])
    assert len(rc.get("simulated")[2]) == 300
