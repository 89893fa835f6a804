"""The record stream's decisions on the device (include/gtx.h: gtx_dstream_push).

Every case of tests/dstream_cases.py under every one of its scripts, judged by its judge: the status, the counts and every byte of the
plane rows, the read meta and the items equal the plain definition.  A script's pushes write into one block per output, preset to 0xA5,
each push's part sized to exactly what the definition leaves with a guard behind it that stays untouched.  Then the launch shapes (1, 63,
64, 65, 257 and 5 000 records a push), two runs that leave the same bytes, a stream that is not the null stream, the refusals, and the
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
