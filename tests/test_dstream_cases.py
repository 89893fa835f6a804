"""What the hand-made record sets of tests/dstream_cases.py are for (FACTS), and the definition held to its second witness: define()
equals the host's gtx_stream_push writing plane rows (lib.Stream after set_planes) on every set under every script, push by push --
the status, the plane rows, the read meta, the items and the counts.  What the host does not have is left out by name: a push that
only max_batch or parked_cap refuses is not sent to the host (the device stream leaves its state alone then), and a stream is not
followed behind a push the host fails half-way -- the IS_FIRST_IN_PAIR clash, which the device stream undoes."""
import ctypes as C

import numpy as np
import pytest

import dstream_cases as dc
from graphtyper_amd import lib as gtx


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_the_set_holds_what_it_is_for(name):
    dc.FACTS[name](dc.cases(name))


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_the_scripts_of_a_case_leave_the_same_bytes(name):
    """whole, one record a push, cut: the outputs of the pushes one after the other are the same bytes"""
    for c in dc.cases(name):
        if c.splits_agree:
            totals = {script: c.total(script) for script, _ in c.scripts}
            assert len(set(totals.values())) == 1, (c.label, [s for s, t in totals.items() if t != totals[c.scripts[0][0]]])


def host_push(stream, c, q):
    """gtx_stream_push over the push's records with its capacities -> (status, planes, meta, items)"""
    recs, rows = np.ascontiguousarray(c.recs[q.lo:q.hi]), np.ascontiguousarray(c.rows[q.lo:q.hi])
    n = q.hi - q.lo
    planes, meta, items = np.zeros((max(q.align_cap, 1), c.plane_stride), np.uint8), np.zeros(max(q.align_cap, 1), gtx.READ_META), np.zeros(max(q.item_cap, 1), gtx.SCORE_ITEM)
    some = np.zeros(64, np.uint8)  # (an empty array has no address to give)
    na, ni = C.c_uint32(), C.c_uint32()
    rc = gtx.lib().gtx_stream_push(stream.h, gtx._p(recs if n else some), gtx._p(rows if n else some), c.seq_stride, n, gtx._p(planes), gtx._p(meta), q.align_cap, C.byref(na),
                                   gtx._p(items), q.item_cap, C.byref(ni))
    return rc, planes[:na.value], meta[:na.value], items[:ni.value]


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_the_definition_equals_the_host_stream(name):
    compared = 0
    for c in dc.cases(name):
        params = gtx.Params(75, 0, 0, c.p["force_align_both_orientations"], 0, c.p["sam_flag_filter"], 0, 0, 0, c.p["max_read_len"])
        for script, pushes in c.scripts:
            stream = gtx.Stream(params, c.n_read_groups)
            stream.set_planes(c.plane_stride)
            host_state = dc.new_state()  # the definition with what the host has: no max_batch, no parked_cap
            for q, want in zip(pushes, c.want(script)):
                recs, rows = c.recs[q.lo:q.hi], c.rows[q.lo:q.hi]
                host_want = dc.define(c.p, c.n_read_groups, host_state, recs, rows, c.plane_stride, align_cap=q.align_cap, item_cap=q.item_cap)
                if want["status"] != host_want[4]:
                    assert (want["status"], host_want[4]) == (dc.ERR_CAPACITY, dc.OK), (c.label, script, q)  # only the device stream's two limits refuse it
                    continue
                host_state = host_want[3]
                rc, planes, meta, items = host_push(stream, c, q)
                assert rc == want["status"], (c.label, script, q, rc, gtx.lib().gtx_last_error())
                if rc != dc.OK:
                    if gtx.lib().gtx_last_error().endswith(b"IS_FIRST_IN_PAIR"):
                        break  # (the host stopped half-way through the batch: its stream is no longer the definition's)
                    assert stream.counts() == dict(zip(("records", "duplicated", "parked"), want["counts"])), (c.label, script, q)
                    continue
                assert planes.tobytes() == want["planes"].tobytes() and meta.tobytes() == want["meta"].tobytes() and items.tobytes() == want["items"].tobytes(), (c.label, script, q)
                assert stream.counts() == dict(zip(("records", "duplicated", "parked"), want["counts"])), (c.label, script, q)
                compared += 1
    assert compared > 0


def test_creation_refuses_what_the_device_stream_does_not_do():
    """decided before a device is looked for: SV graphs, max_read_len as gtx_stream_create, no read group or record; then no device"""
    L, h = gtx.lib(), C.c_void_p()

    def status(n_read_groups=1, device=-1, max_batch=16, parked_cap=16, **fields):
        p = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 0)
        for k, v in fields.items():
            setattr(p, k, v)
        return L.gtx_dstream_create(C.byref(p), n_read_groups, device, max_batch, parked_cap, C.byref(h))

    assert status(is_sv_graph=1) == dc.ERR_UNSUPPORTED and b"SV" in L.gtx_last_error()
    for bad in (dict(max_read_len=256), dict(max_read_len=1001), dict(max_read_len=300, no_second_pass=1), dict(n_read_groups=0), dict(max_batch=0),
                dict(max_batch=1 << 27, parked_cap=1 << 27)):
        assert status(**bad) == dc.ERR_ARG, bad
    assert status() == 2 and status(max_read_len=1000) == 2 and h.value is None  # GTX_ERR_NO_DEVICE
    assert L.gtx_dstream_push(None, None, None, 80, 0, None, 80, None, 0, None, 0, None, None, None) == dc.ERR_ARG
    assert L.gtx_dstream_finish(None, None) == dc.ERR_ARG and L.gtx_dstream_counts(None, None, None, None) == dc.ERR_ARG
