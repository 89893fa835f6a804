"""gtx_disc_realign_batch on the device (include/gtx.h): the pair sets of tests/realign_cases.py -- the ones the host emulation
runs in test_realign_emu.py -- against the plain restatement of the alignment's definition (tests/realign_ref.py, itself held to
the enumeration of tests/realign_brute.py).  Every field of every result is equal: all values are integers, there is no
tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import realign_cases as rc
import realign_ref as rr
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def disc():
    h = C.c_void_p()
    gtx.check(gtx.lib().gtx_disc_create(b"ACGT" * 8, 32, 0, 0, C.byref(h)))
    yield h
    gtx.lib().gtx_disc_destroy(h)


def run_arrays(disc, arrays):
    """arrays: what rc.arrays returns; one launch"""
    planes, plane_stride, lens, seq, off, pr = arrays
    return gtx.disc_realign_batch(disc, planes, plane_stride, lens, len(lens), seq, off, len(off) - 1, pr, len(pr))


def run(disc, reads, targets, pairs):
    return run_arrays(disc, rc.arrays(reads, targets, pairs))


@functools.lru_cache(maxsize=None)
def device_results(disc_value, name):
    """a set's results on the device, computed once for the tests that look at them"""
    return rc.as_tuples(run_arrays(C.c_void_p(disc_value), rc.case(name)[0]))


@pytest.mark.parametrize("name", sorted(rc.SETS) + sorted(rc.ENTRY))
def test_every_field_equals_the_restatement(disc, name):
    """the pair sets (each one batch of one launch), and the cases of the entry point's other paths: rows wider than the reads,
    set bits behind a read's last base, offsets made by hand, letters in lower case and bytes that are no letters"""
    arrays, want = rc.case(name)
    got = device_results(disc.value, name)
    assert len(got) == len(want)
    wrong = [(i, tuple(arrays[5][i]), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert wrong == [], wrong[:5]


def test_a_pair_and_its_reversal_score_alike(disc):
    """the model is symmetric under reversal: a check of reads over 64 bases that does not go through the restatement"""
    reads, _, pairs = rc.get("reversed_pairs")
    got = device_results(disc.value, "reversed_pairs")
    assert len(got) == 2 * 2 * len(rc.M_SIZES) * len(rc.REVERSED_N) and all(g[5] == gtx.REALIGN_OK for g in got)
    assert [(pairs[k], got[k], got[k + 1]) for k in range(0, len(got), 2) if got[k][0] != got[k + 1][0]] == []


def test_a_stream_that_is_not_the_null_stream(disc):
    import torch
    arrays, want = rc.case("simulated")
    planes, plane_stride, lens, seq, off, pr = arrays
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (planes, lens, seq, off, pr)]
    out = torch.zeros(len(pr) * gtx.REALIGN_RESULT.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    gtx.disc_realign_batch(disc, dev[0].data_ptr(), plane_stride, dev[1].data_ptr(), len(lens), dev[2].data_ptr(), dev[3].data_ptr(), len(off) - 1,
                           dev[4].data_ptr(), len(pr), out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy().view(gtx.REALIGN_RESULT)
    assert got.tobytes() == run_arrays(disc, arrays).tobytes()
    assert rc.as_tuples(got) == want


def test_a_batch_of_ten_thousand_workgroups(disc):
    """40 003 pairs: 10 001 workgroups, the last with three live wavefronts"""
    planes, plane_stride, lens, seq, off, pr = rc.case("simulated")[0]
    want = np.array(rc.expected("simulated"), np.int64)
    k = 40003
    index = np.arange(k) % len(pr)
    got = run_arrays(disc, (planes, plane_stride, lens, seq, off, pr[index]))
    assert len(got) == k
    fields = np.stack([got[f].astype(np.int64) for f in ("score", "clip_begin", "clip_end", "target_begin", "target_end", "status")], axis=1)
    wrong = np.nonzero((fields != want[index]).any(axis=1))[0]
    assert len(wrong) == 0, (wrong[:5], fields[wrong[:5]], want[index][wrong[:5]])


def test_device_results_through_the_decision(disc):
    """the device's result of every pair that has a window record -- simulated(), and no_padding for the outcome simulated()'s
    padded windows never reach -- through gtx_disc_realign_decide with old_score one below, at and one above: all six fields
    equal the restatement's decision over the restatement's result"""
    seen = set()
    for name, want_outcomes in (("simulated", {rr.BETTER, rr.SAME_OVERLAPPING, rr.SAME, rr.WORSE}), ("no_padding", {rr.NO_PADDING, rr.BETTER, rr.SAME, rr.WORSE})):
        on_device, by_restatement = rc.decisions(name, device_results(disc.value, name)), rc.decisions(name, rc.expected(name))
        assert len(on_device) == len(by_restatement) == 6 * len(rc.expected(name))
        wrong = []
        for (args, _), (_, want) in zip(on_device, by_restatement):
            d = gtx.disc_realign_decide(args[0] + (gtx.REALIGN_OK,), *args[1:])
            got = (int(d["outcome"]), int(d["pos"]), int(d["pos_end"]), int(d["num_clipped_begin"]), int(d["num_clipped_end"]), int(d["num_ins_begin"]))
            if got != want:
                wrong.append((args[0], args[5], args[6], got, want))
        assert wrong == [], wrong[:5]
        assert {want[0] for _, want in by_restatement} == want_outcomes
        seen |= want_outcomes
    assert len(seen) == 5


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
