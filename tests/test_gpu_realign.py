"""gtx_disc_realign_batch on the device (include/gtx.h): the pair sets of tests/realign_cases.py -- the ones the host emulation
runs in test_realign_emu.py -- against the plain restatement of the alignment's definition (tests/realign_ref.py).  Every field
of every result is equal: all values are integers, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import realign_cases as rc
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def disc():
    h = C.c_void_p()
    gtx.check(gtx.lib().gtx_disc_create(b"ACGT" * 8, 32, 0, 0, C.byref(h)))
    yield h
    gtx.lib().gtx_disc_destroy(h)


def run(disc, reads, targets, pairs):
    planes, plane_stride, lens, seq, off, pr = rc.arrays(reads, targets, pairs)
    return gtx.disc_realign_batch(disc, planes, plane_stride, lens, len(reads), seq, off, len(targets), pr, len(pr))


@pytest.mark.parametrize("name", sorted(rc.SETS))
def test_every_field_equals_the_restatement(disc, name):
    reads, targets, pairs = rc.get(name)
    got, want = rc.as_tuples(run(disc, reads, targets, pairs)), rc.expected(name)
    assert len(got) == len(want)
    wrong = [(i, pairs[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert wrong == [], wrong[:5]


def test_a_number_of_pairs_that_is_no_multiple_of_the_workgroup(disc):
    reads, targets, pairs = rc.get("ties")
    want = rc.expected("ties")
    for k in (1, 2, 3, 5, len(pairs) - (len(pairs) % 4 == 0)):
        assert k % 4 != 0
        assert rc.as_tuples(run(disc, reads, targets, pairs[:k])) == want[:k]


def test_bad_pairs_leave_their_neighbours_right(disc):
    reads, targets, pairs = rc.get("bad_and_long")
    got, want = rc.as_tuples(run(disc, reads, targets, pairs)), rc.expected("bad_and_long")
    assert got == want
    assert [w[5] for w in want].count(gtx.REALIGN_OK) >= 4 and gtx.REALIGN_BAD_PAIR in [w[5] for w in want] and gtx.REALIGN_TOO_LONG in [w[5] for w in want]
    # a read its plane row cannot hold is too long, whatever its length says
    planes, plane_stride, lens, seq, off, pr = rc.arrays([(1,) * 40], ["ACGT" * 20], [(0, 0), (0, 0)])
    assert plane_stride == 32
    lens[0] = 65
    out = gtx.disc_realign_batch(disc, planes, plane_stride, lens, 1, seq, off, 1, pr, 2)
    assert [int(s) for s in out["status"]] == [gtx.REALIGN_TOO_LONG] * 2


def test_the_same_call_twice_gives_the_same_bytes(disc):
    reads, targets, pairs = rc.get("simulated")
    a, b = run(disc, reads, targets, pairs), run(disc, reads, targets, pairs)
    assert a.tobytes() == b.tobytes()


def test_no_pairs_and_no_device(disc):
    import torch
    L = gtx.lib()
    planes, plane_stride, lens, seq, off, pr = rc.arrays(*rc.get("no_padding"))
    assert len(gtx.disc_realign_batch(disc, planes, plane_stride, lens, len(lens), seq, off, len(off) - 1, pr[:0], 0)) == 0
    assert L.gtx_disc_realign_batch(disc, None, 16, None, 0, None, torch.zeros(1, dtype=torch.int32, device="cuda:0").data_ptr(), 0, None, 0, None, None) == 0
    host = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT" * 8, 32, 0, -1, C.byref(host)))
    try:
        d = [torch.zeros(64, dtype=torch.uint8, device="cuda:0") for _ in range(6)]
        rcode = L.gtx_disc_realign_batch(host, d[0].data_ptr(), 16, d[1].data_ptr(), 1, d[2].data_ptr(), d[3].data_ptr(), 1, d[4].data_ptr(), 1, d[5].data_ptr(), None)
        assert rcode == 2 and b"without a device" in L.gtx_last_error()  # GTX_ERR_NO_DEVICE
        torch.cuda.synchronize()
        assert not d[5].cpu().numpy().any()  # nothing ran
    finally:
        L.gtx_disc_destroy(host)
