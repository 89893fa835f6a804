"""gtx_disc_realign_batch on the device for a gtx_disc with gtx_disc_set_max_read_len(d, 1000) (include/gtx.h): the pair sets of
tests/realign_long_cases.py -- the ones the host emulation runs in test_realign_long_emu.py -- against the plain restatement of
the alignment's definition (tests/realign_ref.py).  Every field of every result is equal: all values are integers, there is no
tolerance.  A default object keeps its limits, and a pair within them gives the same bytes on either object."""
import ctypes as C
import functools

import numpy as np
import pytest

import realign_cases as rc
import realign_long_cases as lc
import realign_ref as rr
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu


def make_disc(device=0):
    h = C.c_void_p()
    gtx.check(gtx.lib().gtx_disc_create(b"ACGT" * 8, 32, 0, device, C.byref(h)))
    return h


@pytest.fixture(scope="module")
def disc():
    h = make_disc()
    gtx.disc_set_max_read_len(h, gtx.MAX_READ_LONG)
    yield h
    gtx.lib().gtx_disc_destroy(h)


@pytest.fixture(scope="module")
def default_disc():
    h = make_disc()
    yield h
    gtx.lib().gtx_disc_destroy(h)


def run_arrays(disc, arrays):
    planes, plane_stride, lens, seq, off, pr = arrays
    return gtx.disc_realign_batch(disc, planes, plane_stride, lens, len(lens), seq, off, len(off) - 1, pr, len(pr))


@functools.lru_cache(maxsize=None)
def device_results(disc_value, name):
    return rc.as_tuples(run_arrays(C.c_void_p(disc_value), lc.case(name)[0]))


def differences(pairs, got, want):
    assert len(got) == len(want)
    return [(i, tuple(pairs[i]), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]][:5]


@pytest.mark.parametrize("name", sorted(lc.SETS) + sorted(lc.ENTRY))
def test_every_field_equals_the_restatement(disc, name):
    arrays, want = lc.case(name)
    assert differences(arrays[5], device_results(disc.value, name), want) == []


def test_rows_exactly_as_wide_as_the_read(disc):
    for m in lc.ROW_M:
        arrays, want = lc.row_case(m)
        assert differences(arrays[5], rc.as_tuples(run_arrays(disc, arrays)), want) == [], m


def test_planted_alignments(disc):
    """60 pairs over windows of 2 049 .. 4 095: score m - 5k, cb 0, clip_end m, target_begin the copy's place"""
    (reads, targets, pairs), want = lc.planted()
    assert len(pairs) == 60
    assert differences(pairs, rc.as_tuples(run_arrays(disc, lc.arrays(reads, targets, pairs))), want) == []


def test_a_pair_and_its_reversal_score_alike(disc):
    reads, targets, pairs = lc.reversed_pairs()
    got = rc.as_tuples(run_arrays(disc, lc.arrays(reads, targets, pairs)))
    assert len(got) == 80 and all(g[5] == gtx.REALIGN_OK for g in got)
    assert all(257 <= len(r) <= 1000 for r in reads) and all(2049 <= len(t) <= 4095 for t in targets)
    assert [(pairs[k], got[k], got[k + 1]) for k in range(0, len(got), 2) if got[k][0] != got[k + 1][0]] == []
    assert len({g[0] for g in got}) > 20  # (not one score for all)


def test_a_default_object_keeps_its_limits_and_the_short_pairs_their_bytes(disc, default_disc):
    reads, targets, pairs = lc.get("mixed_batch")
    arrays = lc.case("mixed_batch")[0]
    kinds = [lc.kind_of(reads, targets, p) for p in pairs]
    by_default, by_long = run_arrays(default_disc, arrays), run_arrays(disc, arrays)
    assert differences(pairs, rc.as_tuples(by_default), [lc.result(reads, targets, p, 0) for p in pairs]) == []
    assert kinds.count("long") >= 5 and all(t == lc.TOO_LONG for t, k in zip(rc.as_tuples(by_default), kinds) if k == "long")
    keep = np.array([k != "long" for k in kinds])
    assert keep.sum() >= 15 and by_default[keep].tobytes() == by_long[keep].tobytes()


def test_the_short_sets_on_a_long_mode_object(disc, default_disc):
    arrays, want = rc.case("simulated")
    got = run_arrays(disc, arrays)
    assert rc.as_tuples(got) == want
    assert got.tobytes() == run_arrays(default_disc, arrays).tobytes()


def test_the_setter():
    L = gtx.lib()
    long_pair = lc.arrays([lc.codes("ACGT" * 70)], ["ACGT" * 80], [(0, 0)])  # 280 bases
    ok = lc.result([lc.codes("ACGT" * 70)], ["ACGT" * 80], (0, 0))
    assert ok == (280, 0, 280, 0, 280, gtx.REALIGN_OK)
    for device in (0, -1):
        h = make_disc(device)
        try:
            for n in (0, 256, 257, 1000):
                assert L.gtx_disc_set_max_read_len(h, n) == 0, n
            for n in (255, 1001, 1, 0xFFFFFFFF):
                assert L.gtx_disc_set_max_read_len(h, n) == 1 and b"gtx_disc_set_max_read_len: max_read_len must be" in L.gtx_last_error(), n  # GTX_ERR_ARG
            with pytest.raises(gtx.GtxError):
                gtx.disc_set_max_read_len(h, 1001)
            if device == 0:  # a refused value leaves the limit in force (1 000), 279 refuses 280 bases, 0 and 256 are the default again
                assert rc.as_tuples(run_arrays(h, long_pair)) == [ok]
                for n, want in ((279, lc.TOO_LONG), (280, ok), (256, lc.TOO_LONG), (1000, ok), (0, lc.TOO_LONG)):
                    gtx.disc_set_max_read_len(h, n)
                    assert rc.as_tuples(run_arrays(h, long_pair)) == [want], n
        finally:
            L.gtx_disc_destroy(h)
    assert L.gtx_disc_set_max_read_len(None, 0) == 1
    assert (gtx.REALIGN_MAX_TARGET_LONG, gtx.MAX_READ_LONG) == (4095, 1000)


def on_device(arrays, n_out, guard=0):
    import torch
    planes, plane_stride, lens, seq, off, pr = arrays
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (planes, lens, seq, off, pr)]
    out = torch.full((n_out * gtx.REALIGN_RESULT.itemsize + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return dev, out


def test_a_stream_that_is_not_the_null_stream_and_guard_bytes(disc):
    """both launches go to the caller's stream, and nothing is written behind d_out's last result"""
    import torch
    arrays, want = lc.case("mixed_batch")
    planes, plane_stride, lens, seq, off, pr = arrays
    dev, out = on_device(arrays, len(pr), guard=256)
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    gtx.disc_realign_batch(disc, dev[0].data_ptr(), plane_stride, dev[1].data_ptr(), len(lens), dev[2].data_ptr(), dev[3].data_ptr(), len(off) - 1,
                           dev[4].data_ptr(), len(pr), out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    host = out.cpu().numpy()
    assert (host[-256:] == 0x5A).all()
    got = host[:-256].view(gtx.REALIGN_RESULT)
    assert rc.as_tuples(got) == want
    assert got.tobytes() == run_arrays(disc, arrays).tobytes()


def test_the_same_call_twice_gives_the_same_bytes(disc):
    arrays = lc.case("row_boundaries")[0]
    assert run_arrays(disc, arrays).tobytes() == run_arrays(disc, arrays).tobytes()


def test_the_grids_edge(disc):
    """4 003 pairs cycling through row_boundaries: 1 001 workgroups, the last with three live wavefronts"""
    planes, plane_stride, lens, seq, off, pr = lc.case("row_boundaries")[0]
    want = np.array(lc.expected("row_boundaries"), np.int64)
    k = 4003
    index = np.arange(k) % len(pr)
    got = run_arrays(disc, (planes, plane_stride, lens, seq, off, pr[index]))
    assert len(got) == k
    fields = np.stack([got[f].astype(np.int64) for f in ("score", "clip_begin", "clip_end", "target_begin", "target_end", "status")], axis=1)
    wrong = np.nonzero((fields != want[index]).any(axis=1))[0]
    assert len(wrong) == 0, (wrong[:5], fields[wrong[:5]], want[index][wrong[:5]])


def test_device_results_through_the_decision(disc):
    """the device's results of both_limits through gtx_disc_realign_decide, with old_score one below, at and one above and plain
    window records: all six fields equal the restatement's decision over the restatement's result"""
    reads, targets, pairs = lc.get("both_limits")
    got, want = device_results(disc.value, "both_limits"), lc.expected("both_limits")
    seen = set()
    for (r, w), g, e in zip(pairs, got, want):
        ref_pos = np.arange(len(targets[w]), dtype=np.int32)
        for delta in (-1, 0, 1):
            for indel_pos in (5000 + e[3] + 10, 5000 - 300):
                args = (len(reads[r]), ref_pos, 5000, 20000, e[0] + delta, indel_pos)
                d = gtx.disc_realign_decide(g[:5] + (gtx.REALIGN_OK,), *args)
                have = (int(d["outcome"]), int(d["pos"]), int(d["pos_end"]), int(d["num_clipped_begin"]), int(d["num_clipped_end"]), int(d["num_ins_begin"]))
                assert have == rr.decide(e, args[0], list(ref_pos), *args[2:]), (g, e, delta, indel_pos)
                seen.add(have[0])
    assert seen == {rr.NO_PADDING, rr.BETTER, rr.SAME_OVERLAPPING, rr.SAME, rr.WORSE}
