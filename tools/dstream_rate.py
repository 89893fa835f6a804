#!/usr/bin/env python
"""What a push of the device record stream costs beside the host's: gtx_dstream_push against gtx_stream_push on one host thread, over the
same records -- shaped like a position-sorted BAM of two read groups and three samples of 150-base reads: pairs with inserts of 300 +- 50,
a duplicate behind one template in ten, a filtered record behind 6 %, 4 % of the templates unpaired -- at 10 k, 100 k and 1 M records a
push, the device's inputs and outputs resident.
  device  HIP events around the call on the caller's stream (the call ends by waiting for that stream), and the host's clock around
          it; a stream object of its own per repeat, made outside the timed window (a push changes the stream's state)
  host    the host's clock around gtx_stream_push writing plane rows, a stream object of its own per repeat
The two leave the same tasks and items (checked: the counts at every size, every byte at the smallest).  Warm-up pushes, then
--repeats timed ones per path, alternating; medians with the extremes.
  python tools/dstream_rate.py [--sizes 10000,100000,1000000] [--repeats 10] [--out profiles/dstream_rate.json]
The device time split by launch comes from a run of its own under the profiler, whose kernel statistics this tool adds to the file:
  rocprofv3 --kernel-trace --stats -d DIR -o dstream -- python tools/dstream_rate.py --sizes 1000000 --repeats 3 --device-only
  python tools/dstream_rate.py --kernel-stats DIR --out profiles/dstream_rate.json"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from graphtyper_amd import lib as gtx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10000,100000,1000000")
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--kernel-stats", default="", help="a directory rocprofv3 --kernel-trace --stats wrote: its kernel statistics go into --out, nothing is run")
ap.add_argument("--out", default="")
L_READ, SEQ_STRIDE, PLANE_STRIDE, N_RG = 150, 80, 80, 2
PAIRED, REVERSED, MATE_REVERSED, FIRST, SECOND = 1, 16, 32, 64, 128


def model(n, seed):
    """-> (STREAM_RECORD [n], rows [n, SEQ_STRIDE]) in stream order"""
    rng = np.random.default_rng(seed)
    t = int(n / 1.9) + 64  # templates: more than n records, the tail is cut off (mates that never come)
    pos = 10000 + np.cumsum(rng.integers(0, 4, t))
    unpaired = rng.random(t) < 0.04
    ins = np.clip(rng.normal(300, 50, t), 160, 600).astype(np.int64)
    concordant = rng.random(t) < 0.9
    rg, sample, name = rng.integers(0, N_RG, t), rng.integers(0, 3, t), np.arange(t, dtype=np.uint64)
    idx = np.arange(t)
    second, dup, dropped = idx[~unpaired], idx[rng.random(t) < 0.1], idx[rng.random(t) < 0.06]
    first_flag = np.where(unpaired, 0, PAIRED | FIRST | np.where(concordant, MATE_REVERSED, 0))
    # (position, order at that position, flag, isize, name, template, row of the table of sequences)
    parts = [(pos, np.zeros(t, np.int64), first_flag, np.where(unpaired, 0, ins), name, idx, idx),
             (pos[second] + ins[second] - L_READ, np.ones(len(second), np.int64), np.full(len(second), PAIRED | SECOND | REVERSED), -ins[second], name[second], second, t + second),
             (pos[dup], np.zeros(len(dup), np.int64), np.zeros(len(dup), np.int64), np.zeros(len(dup), np.int64), name[dup] + (1 << 33), dup, dup),
             (pos[dropped], np.zeros(len(dropped), np.int64), np.full(len(dropped), 256), np.zeros(len(dropped), np.int64), name[dropped] + (1 << 34), dropped, 2 * t + dropped)]
    p, order, flag, isize, nm, tmpl, row = (np.concatenate([part[k] for part in parts]) for k in range(7))
    # stable: a template's duplicate and its dropped record stay right behind it
    by = np.lexsort((np.concatenate([np.full(len(part[0]), k) for k, part in enumerate(parts)]), tmpl, order, p))[:n]
    assert len(by) == n
    recs = np.zeros(n, gtx.STREAM_RECORD)
    recs["flag"], recs["pos"], recs["isize"], recs["name_id"] = flag[by], p[by], isize[by], nm[by]
    recs["rg"], recs["sample"] = rg[tmpl[by]], sample[tmpl[by]]
    recs["mapq"], recs["score_diff"], recs["l_qseq"] = rng.integers(0, 61, n), rng.integers(0, 40, n), L_READ
    recs["n_cigar"], recs["cigar_front"] = 1, (L_READ << 4)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (3 * t, L_READ), dtype=np.uint8)]
    return recs, gtx.pack_nibbles(codes[row[by]], SEQ_STRIDE)


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def merge_kernel_stats(directory, out_path):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_stats.csv under " + directory)
    kernels = []
    for row in csv.DictReader(open(files[-1])):
        kernels.append(dict(name=row["Name"][:120], calls=int(row["Calls"]), total_ns=int(float(row["TotalDurationNs"])), average_ns=float(row["AverageNs"]),
                            percent=float(row["Percentage"])))
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["kernels_of_1M_record_pushes"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own (warm-up pushes included)", kernels=kernels)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["kernels_of_1M_record_pushes"], indent=1))


def main():
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)
    import torch
    if not torch.cuda.is_available():
        sys.exit("dstream_rate: no GPU (a rate is measured on the device or not at all)")
    L = gtx.lib()
    params = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 0)
    rows_out = []
    for size in [int(s) for s in args.sizes.split(",")]:
        recs, rows = model(size, 2024)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
        d_recs, d_rows = dev(recs), dev(rows)
        d_planes, d_meta, d_items = (torch.zeros(size * k, dtype=torch.uint8, device="cuda:0") for k in (PLANE_STRIDE, 20, 40))
        h_planes, h_meta, h_items = np.zeros((size, PLANE_STRIDE), np.uint8), np.zeros(size, gtx.READ_META), np.zeros(size, gtx.SCORE_ITEM)
        stream = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        device_ms, call_ms, host_ms, got = [], [], [], {}
        for rep in range(args.warmup + args.repeats):
            ds = gtx.DeviceStream(params, N_RG, 0, size, size)
            torch.cuda.synchronize()
            e0.record(stream)
            t0 = time.perf_counter()
            rc, na, ni = ds.push_raw(d_recs.data_ptr(), d_rows.data_ptr(), SEQ_STRIDE, size, d_planes.data_ptr(), PLANE_STRIDE, d_meta.data_ptr(), size,
                                     d_items.data_ptr(), size, C.c_void_p(stream.cuda_stream))
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            gtx.check(rc)
            got["device"] = (na, ni, ds.counts())
            del ds
            if not args.device_only:
                hs = gtx.Stream(params, N_RG)
                hs.set_planes(PLANE_STRIDE)
                a, i = C.c_uint32(), C.c_uint32()
                t2 = time.perf_counter()
                gtx.check(L.gtx_stream_push(hs.h, gtx._p(recs), gtx._p(rows), SEQ_STRIDE, size, gtx._p(h_planes), gtx._p(h_meta), size, C.byref(a), gtx._p(h_items), size,
                                            C.byref(i)))
                t3 = time.perf_counter()
                got["host"] = (a.value, i.value, hs.counts())
                assert got["host"] == got["device"], got
            if rep >= args.warmup:
                device_ms.append(e0.elapsed_time(e1))
                call_ms.append(1e3 * (t1 - t0))
                if not args.device_only:
                    host_ms.append(1e3 * (t3 - t2))
        na, ni, counts = got["device"]
        if not args.device_only and size == min(int(s) for s in args.sizes.split(",")):
            torch.cuda.synchronize()
            assert d_planes.cpu().numpy()[:na * PLANE_STRIDE].tobytes() == h_planes[:na].tobytes() and d_meta.cpu().numpy()[:na * 20].tobytes() == h_meta[:na].tobytes()
            assert d_items.cpu().numpy()[:ni * 40].tobytes() == h_items[:ni].tobytes()
        row = dict(records=size, tasks=na, items=ni, counts=counts, device_event_ms=spread(device_ms), device_call_ms=spread(call_ms),
                   device_records_per_s=size / (1e-3 * statistics.median(device_ms)))
        if not args.device_only:
            row.update(host_ms=spread(host_ms), host_records_per_s=size / (1e-3 * statistics.median(host_ms)))
            row["device_over_host"] = row["device_records_per_s"] / row["host_records_per_s"]
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc.update(what="gtx_dstream_push (HIP events on the caller's stream; inputs and outputs resident) beside gtx_stream_push on one host thread, the same records",
                   device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, pushes=rows_out)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
