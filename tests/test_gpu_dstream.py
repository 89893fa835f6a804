"""The record stream's decisions on the device (include/gtx.h: gtx_dstream_push).

Every case of tests/dstream_cases.py under every one of its scripts, judged by its judge: the status, the counts and every byte of the
plane rows, the read meta and the items equal the plain definition.  A script's pushes write into one block per output, preset to 0xA5,
each push's part sized to exactly what the definition leaves with a guard behind it that stays untouched.  Then the launch shapes (1, 63,
64, 65, 257 and 5 000 records a push), two runs that leave the same bytes, a stream that is not the null stream, the refusals, what a
failing push says of its reason (gtx_last_error), gtx_dstream_finish beside gtx_stream_finish, and the
stream's outputs going straight into gtx_align_batch_planes and gtx_score_batch_flags without a host copy: the accumulators of the host
stream's run.  All values are bytes and words; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import dstream_cases as dc
import harness
import scenarios
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu

ERR_NO_DEVICE = 2


def on_device(a):
    import torch
    flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([flat, np.zeros(64, np.uint8)])).to("cuda:0")  # (never empty)


def params_of(c):
    return gtx.Params(75, 0, 0, c.p["force_align_both_orientations"], 0, c.p["sam_flag_filter"], 0, 0, 0, c.p["max_read_len"])


def device_run(c, pushes, rooms, stream=None):
    """dc.judge's `run` over the library: one stream object, the pushes one after the other"""
    import torch
    ds = gtx.DeviceStream(params_of(c), c.n_read_groups, 0, c.max_batch, c.parked_cap)
    d_recs, d_rows = on_device(c.recs), on_device(c.rows)
    sizes = dict(planes=c.plane_stride, meta=gtx.READ_META.itemsize, items=gtx.SCORE_ITEM.itemsize)
    at, ends = {k: [] for k in sizes}, dict.fromkeys(sizes, 0)
    for room in rooms:
        for k in sizes:
            at[k].append(ends[k])
            ends[k] += (room[1] if k == "items" else room[0]) * sizes[k] + dc.GUARD
    out = {k: torch.full((ends[k] + 64,), dc.FILL, dtype=torch.uint8, device="cuda:0") for k in sizes}
    assert all(out[k].data_ptr() % 16 == 0 for k in sizes)
    torch.cuda.synchronize()
    heads = []
    for j, q in enumerate(pushes):
        rc, na, ni = ds.push_raw(d_recs.data_ptr() + q.lo * gtx.STREAM_RECORD.itemsize, d_rows.data_ptr() + q.lo * c.seq_stride, c.seq_stride, q.hi - q.lo,
                                 out["planes"].data_ptr() + at["planes"][j], c.plane_stride, out["meta"].data_ptr() + at["meta"][j], q.align_cap,
                                 out["items"].data_ptr() + at["items"][j], q.item_cap, stream)
        n = ds.counts()
        heads.append(dict(status=rc, n_align=na, n_items=ni, counts=(n["records"], n["duplicated"], n["parked"])))
    torch.cuda.synchronize()
    host = {k: out[k].cpu().numpy() for k in sizes}
    for j, (room, got) in enumerate(zip(rooms, heads)):
        for k in sizes:
            got[k] = host[k][at[k][j]:at[k][j] + (room[1] if k == "items" else room[0]) * sizes[k] + dc.GUARD]
    return heads


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_every_push_equals_the_definition(name):
    assert dc.judge(name, device_run) is None


def model():
    return dc.cases("model")[0]


def test_launch_shapes_and_two_runs():
    """pushes of 1, 63, 64, 65 and 257 records one after the other, then the rest; and 5 000 in one push: twice, the same bytes"""
    c = model()
    bounds = np.cumsum([0, 1, 63, 64, 65, 257]).tolist() + [len(c.recs)]
    for pushes in ([dc.push(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])], [dc.push(0, len(c.recs))]):
        wants = c.want_of(pushes)
        rooms = dc.rooms_of(pushes, wants)
        runs = [device_run(c, pushes, rooms) for _ in range(2)]
        for j, (q, room, want) in enumerate(zip(pushes, rooms, wants)):
            assert dc.differs(c, q, room, want, runs[0][j]) is None, (j, q)
            assert all(np.array_equal(runs[0][j][k], runs[1][j][k]) for k in ("planes", "meta", "items")) and runs[0][j]["counts"] == runs[1][j]["counts"]


def test_a_stream_that_is_not_the_null_stream():
    import torch
    c = model()
    script, pushes = c.scripts[2]
    side = torch.cuda.Stream()
    gots = device_run(c, pushes, c.rooms(script), stream=C.c_void_p(side.cuda_stream))
    for j, (q, room, want, got) in enumerate(zip(pushes, c.rooms(script), c.want(script), gots)):
        assert dc.differs(c, q, room, want, got) is None, (j, q)


def test_the_refusals():
    import torch
    L, h = gtx.lib(), C.c_void_p()

    def create(device=0, n_read_groups=1, max_batch=16, parked_cap=16, **fields):
        p = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 0)
        for k, v in fields.items():
            setattr(p, k, v)
        return L.gtx_dstream_create(C.byref(p), n_read_groups, device, max_batch, parked_cap, C.byref(h))

    assert create(device=-1) == ERR_NO_DEVICE and create(device=torch.cuda.device_count()) == ERR_NO_DEVICE
    assert create(is_sv_graph=1) == dc.ERR_UNSUPPORTED and b"SV" in L.gtx_last_error()
    for bad in (dict(max_read_len=256), dict(max_read_len=1001), dict(max_read_len=300, no_second_pass=1), dict(n_read_groups=0), dict(max_batch=0)):
        assert create(**bad) == dc.ERR_ARG, bad
    assert create(max_read_len=1000) == dc.OK
    L.gtx_dstream_destroy(h)
    # a push whose arguments are refused leaves the stream alone
    c = dc.cases("dups_runs")[0]
    ds = gtx.DeviceStream(params_of(c), 1, 0, len(c.recs), len(c.recs))
    d_recs, d_rows = on_device(c.recs), on_device(c.rows)
    n = len(c.recs)
    out = [torch.full((n * size + 64,), dc.FILL, dtype=torch.uint8, device="cuda:0") for size in (80, 20, 40)]
    torch.cuda.synchronize()
    args = dict(d_recs=d_recs.data_ptr(), d_seq=d_rows.data_ptr(), seq_stride=c.seq_stride, n=n, d_planes=out[0].data_ptr(), plane_stride=80, d_meta=out[1].data_ptr(), align_cap=n,
                d_items=out[2].data_ptr(), item_cap=n)
    for bad in (dict(plane_stride=40), dict(plane_stride=0), dict(d_planes=args["d_planes"] + 4), dict(seq_stride=0), dict(d_recs=None), dict(d_items=None), dict(d_meta=args["d_meta"] + 2)):
        assert ds.push_raw(**dict(args, **bad))[0] == dc.ERR_ARG, bad
    assert ds.counts() == dict(records=0, duplicated=0, parked=0)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == dc.FILL).all() for o in out)
    rc, na, ni = ds.push_raw(**args)
    want, = c.want("whole")
    assert (rc, na, ni) == (dc.OK, len(want["meta"]), len(want["items"])) and ds.counts()["duplicated"] == want["counts"][1]
    ds.finish()
    assert ds.counts()["parked"] == 0


def case_labelled(name, start):
    c, = [c for c in dc.cases(name) if c.label.startswith(start)]
    return c


def test_a_failing_push_says_which_record_and_how_many_wait():
    """the four words of the download that no output carries reach the caller as gtx_last_error: the length of the FIRST record beyond
    max_read_len -- a record the filter drops, in front of a read group out of range; a shorter one in front of a longer one -- and
    the mates that would wait.  The numbers are the definition's (dstream_cases.define: reason)"""
    L = gtx.lib()
    for c, status, why, message in (
            (case_labelled("limits", "a read of 257 bases in front of a read group out of range"), dc.ERR_UNSUPPORTED, (dc.WHY_LONG, 2, 257, 0),
             b"gtx_dstream_push: a read of 257 bases (the stream's max_read_len is 256)"),
            (case_labelled("fail_order", "a read of 300 bases behind a read of 260"), dc.ERR_UNSUPPORTED, (dc.WHY_LONG, 1, 260, 0),
             b"gtx_dstream_push: a read of 260 bases (the stream's max_read_len is 256)"),
            (case_labelled("limits", "parked_cap one over"), dc.ERR_CAPACITY, (dc.WHY_PARKED, 0, 0, 3),
             b"gtx_dstream_push: 3 mates wait at the end of the push, the stream was made with parked_cap 2")):
        want, = c.want("whole")
        assert (want["status"], want["reason"]) == (status, why)
        got, = device_run(c, dict(c.scripts)["whole"], c.rooms("whole"))
        assert got["status"] == status and L.gtx_last_error() == message, (c.label, got["status"], L.gtx_last_error())
        assert got["counts"] == (0, 0, 0)


def test_a_mate_of_a_read_parked_before_finish_waits_anew():
    """gtx_dstream_finish forgets the parked mates as gtx_stream_finish does: the second mate of a read parked before it makes no item and
    waits itself -- the device stream and the host stream side by side, byte for byte, the carried record and next_align_index kept"""
    import torch
    b = dc.Builder()
    b.add(dc.bases(40, 1), pos=100, flag=dc.PAIRED | dc.FIRST | dc.MATE_REVERSED, isize=200, name=1, sample=1)
    b.add(dc.bases(40, 2), pos=101, name=2)
    b.add(dc.bases(40, 2), pos=101, flag=dc.PAIRED | dc.SECOND | dc.REVERSED, isize=-200, name=1, sample=2)  # (a duplicate of the record carried over finish)
    b.add(dc.bases(40, 3), pos=102, name=3)
    c = b.case("a mate on either side of finish")
    cuts = ((0, 2), (2, 4))
    # without finish the second push pairs the two
    unfinished = c.want_of([dc.push(lo, hi) for lo, hi in cuts])
    assert [len(w["items"]) for w in unfinished] == [1, 2] and unfinished[1]["counts"] == (4, 1, 0)
    hs = gtx.Stream(params_of(c), 1)
    hs.set_planes(c.plane_stride)
    ds = gtx.DeviceStream(params_of(c), 1, 0, len(c.recs), len(c.recs))
    for k, (lo, hi) in enumerate(cuts):
        recs, rows = np.ascontiguousarray(c.recs[lo:hi]), np.ascontiguousarray(c.rows[lo:hi])
        host = hs.push(recs, rows)
        d_recs, d_rows = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to("cuda:0"), torch.from_numpy(rows).to("cuda:0")
        dev = [t.cpu().numpy() for t in ds.push(d_recs, d_rows, c.plane_stride)]
        assert [len(x) for x in host] == ([2, 2, 1], [1, 1, 1])[k]  # (tasks: the second push's first record is a duplicate; items: the unpaired ones only)
        for h, d in zip(host, dev):
            assert h.tobytes() == d.tobytes(), (k, h, d)
        assert ds.counts() == hs.counts() and ds.counts()["parked"] == 1
        if k == 0:
            hs.finish()
            ds.finish()
            assert ds.counts() == hs.counts() == dict(records=2, duplicated=0, parked=0)
    assert ds.counts() == dict(records=4, duplicated=1, parked=1)
    assert host[2]["first"]["align_index"].tolist() == [2] and host[2]["second"]["align_index"].tolist() == [dc.INVALID]


def test_the_outputs_go_straight_into_alignment_and_scoring():
    """6 000 pairs pushed in three parts through the device stream, its plane rows, meta and items never leaving the device: the
    accumulators are those of the host stream's run"""
    import torch
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=40000, n_pairs=6000, n_samples=3)
    b = harness.GpuBackend(gtx.graph_from_records(ref, recs, region_begin=500000))
    seq = gtx.pack_nibbles(codes)
    n = len(rec)
    cuts = [0, n // 3, 2 * n // 3, n]
    L = gtx.lib()

    def scores(d_planes, d_meta, d_items, n_align, n_items):
        acc = harness.Accumulators(b.ctx, 3)
        devs = [b._dev(a) for a in acc.arrays()]
        buf = acc.buffers([d.data_ptr() for d in devs])
        d_rec = torch.zeros(n_align * 2 * harness.REC_WORDS, dtype=torch.int32, device="cuda:0")
        d_fl = torch.zeros(n_align * 2, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gtx.check(L.gtx_align_batch_planes(b.ctx.h, d_planes.data_ptr(), 80, d_meta.data_ptr(), n_align, d_rec.data_ptr(), harness.REC_WORDS, d_fl.data_ptr(), None))
        gtx.check(L.gtx_score_batch_flags(b.ctx.h, d_items.data_ptr(), n_items, d_rec.data_ptr(), harness.REC_WORDS, d_fl.data_ptr(), C.byref(buf), None))
        torch.cuda.synchronize()
        assert b.ctx.error_count() == 0
        for host, dev in zip(acc.arrays(), devs):
            host[...] = dev.cpu().numpy().view(host.dtype)
        return harness.canonical_scores(b.ctx, acc)

    # the host stream
    hs = gtx.Stream(b.ctx.params, 1)
    hs.set_planes(80)
    parts = [hs.push(rec[lo:hi], seq[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    planes, meta, items = (np.concatenate([p[k] for p in parts]) for k in range(3))
    want = scores(on_device(planes), on_device(meta), on_device(items), len(meta), len(items))
    # the device stream
    ds = gtx.DeviceStream(b.ctx.params, 1, 0, n, n)
    d_recs, d_rows = on_device(rec), on_device(seq)
    d_planes, d_meta, d_items = (torch.zeros(n * size + 64, dtype=torch.uint8, device="cuda:0") for size in (80, 20, 40))
    torch.cuda.synchronize()
    na = ni = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rc, a, i = ds.push_raw(d_recs.data_ptr() + lo * 56, d_rows.data_ptr() + lo * seq.shape[1], seq.shape[1], hi - lo, d_planes.data_ptr() + na * 80, 80,
                               d_meta.data_ptr() + na * 20, n - na, d_items.data_ptr() + ni * 40, n - ni)
        gtx.check(rc)
        na, ni = na + a, ni + i
    assert (na, ni) == (len(meta), len(items)) and ds.counts() == hs.counts()
    got = scores(d_planes, d_meta, d_items, na, ni)
    assert want.sum() > 0 and np.array_equal(got, want)
