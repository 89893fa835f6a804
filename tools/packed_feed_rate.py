#!/usr/bin/env python3
"""The PCIe-fed leg of bench.py (extra_pcie_fed) once with plane rows and once with packed 2-bit rows + exception list
(gtx_align_batch_packed), alternating in one process, on cfg2: inputs in pinned host memory, copied per step in `chunks`
parts on a copy stream into two staging sets while the previous part is aligned and scored.  Per layout: reads/s, host bytes
per read, PCIe GB/s, and whether the step's calls equal a resident run.  One JSON line per round and layout, then a summary.
    python tools/packed_feed_rate.py [--reads N] [--steps S] [--rounds R] [--chunks C]
    python tools/packed_feed_rate.py --unpack-only [--reads N]     gtx_packed_kernel and gtx_planes_kernel over N resident reads,
                                                                   5 launches each (for a kernel trace)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from graphtyper_amd import lib as gtx, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--chunks", type=int, default=4)
ap.add_argument("--unpack-only", action="store_true")
args = ap.parse_args()

device = torch.device("cuda", 0)
L = gtx.lib()
ref, records, ref_str = bench.cfg2_graph_inputs(synth)
ctx = gtx.Context(gtx.graph_from_records(ref_str, records, region_begin=bench.REGION_BEGIN), device=0)
n = args.reads
d_seq, d_pos = bench.make_reads_on_device(torch, ref, records, n, seed=bench.CFG2_READ_SEED, device=device)
nib = d_seq.cpu().numpy()
PACKED_STRIDE = 40  # 150 bases
t0 = time.perf_counter()
rows, exc_start, exc = gtx.pack_2bit(nib, np.full(n, bench.READ_LEN, np.uint32), PACKED_STRIDE)
pack_s = time.perf_counter() - t0

if args.unpack_only:
    d_rows, d_start, d_exc = (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device) for a in (rows, exc_start, exc))
    d_planes = torch.empty(n * 80, dtype=torch.uint8, device=device)
    for _ in range(5):
        gtx.check(L.gtx_packed_to_planes(ctx.h, d_rows.data_ptr(), PACKED_STRIDE, d_start.data_ptr(), d_exc.data_ptr(), len(exc), n,
                                         d_planes.data_ptr(), 80, None))
    for _ in range(5):
        gtx.check(L.gtx_reads_to_planes(ctx.h, d_seq.data_ptr(), 80, n, d_planes.data_ptr(), 80, None))
    torch.cuda.synchronize()
    print(json.dumps({"reads": n, "exceptions": int(len(exc)), "launches_each": 5}))
    sys.exit(0)

w = bench.Workload(torch, gtx, ctx, device, d_seq, d_pos, 1, hint=True)
del d_seq
d_planes, d_meta, d_items = w.sets[0]
chunks = args.chunks
c = n // chunks
assert c * chunks == n and bench.PLANE_INPUT
sp = w.sp
fl = w.d_flags.data_ptr() if w.d_flags is not None else None
copy_stream = torch.cuda.Stream(device=device)
meta_h, items_h = d_meta.cpu().pin_memory(), d_items.cpu().pin_memory()
plane_h = d_planes.cpu().pin_memory()
rows_h = torch.from_numpy(rows).pin_memory()
start_h = torch.from_numpy(exc_start.view(np.int32)).pin_memory()
exc_h = torch.from_numpy(exc.view(np.int16)).pin_memory()
cut = [int(exc_start[k * c]) for k in range(chunks + 1)]
exc_cap = max(max(cut[k + 1] - cut[k] for k in range(chunks)), 1)


def staging(kind):
    sets = []
    for _ in range(2):
        s = dict(meta=torch.empty((c, gtx.READ_META.itemsize), dtype=torch.uint8, device=device),
                 items=torch.empty((c, gtx.SCORE_ITEM.itemsize), dtype=torch.uint8, device=device))
        if kind == "planes":
            s["seq"] = torch.empty((c, 80), dtype=torch.uint8, device=device)
        else:
            s["seq"] = torch.empty((c, PACKED_STRIDE), dtype=torch.uint8, device=device)
            s["start"] = torch.empty(c + 1, dtype=torch.int32, device=device)
            s["exc"] = torch.empty(exc_cap, dtype=torch.int16, device=device)
        sets.append(s)
    return sets


stages = {"planes": staging("planes"), "packed": staging("packed")}
ready = [torch.cuda.Event() for _ in range(2)]
free = [torch.cuda.Event() for _ in range(2)]


def one_step(kind):
    stage = stages[kind]
    with torch.cuda.stream(w.stream):
        gtx.check(L.gtx_scores_zero(ctx.h, C.byref(w.buf), sp))
    for k in range(chunks):
        b = k & 1
        s = stage[b]
        a, e = k * c, (k + 1) * c
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(free[b])
            s["meta"].copy_(meta_h[a:e], non_blocking=True)
            s["items"].copy_(items_h[a:e], non_blocking=True)
            if kind == "planes":
                s["seq"].copy_(plane_h[a:e], non_blocking=True)
            else:
                s["seq"].copy_(rows_h[a:e], non_blocking=True)
                s["start"].copy_(start_h[a:e + 1], non_blocking=True)
                if cut[k + 1] > cut[k]:
                    s["exc"][:cut[k + 1] - cut[k]].copy_(exc_h[cut[k]:cut[k + 1]], non_blocking=True)
            ready[b].record(copy_stream)
        with torch.cuda.stream(w.stream):
            w.stream.wait_event(ready[b])
            d_rec = w.d_rec.data_ptr() + 4 * 2 * bench.REC_WORDS * a
            d_fl = (fl + 2 * a) if fl else None
            if kind == "planes":
                gtx.check(L.gtx_align_batch_planes(ctx.h, s["seq"].data_ptr(), 80, s["meta"].data_ptr(), c, d_rec, bench.REC_WORDS, d_fl, sp))
            else:
                # (the chunk's exc_start values are offsets from its first: copied as they are, no rebasing)
                gtx.check(L.gtx_align_batch_packed(ctx.h, s["seq"].data_ptr(), PACKED_STRIDE, s["start"].data_ptr(), s["exc"].data_ptr(),
                                                   cut[k + 1] - cut[k], s["meta"].data_ptr(), c, d_rec, bench.REC_WORDS, d_fl, sp))
            gtx.check(L.gtx_score_batch_flags(ctx.h, s["items"].data_ptr(), c, w.d_rec.data_ptr(), bench.REC_WORDS, fl, C.byref(w.buf), sp))
            free[b].record(w.stream)
    with torch.cuda.stream(w.stream):
        gtx.check(L.gtx_calls_batch(ctx.h, C.byref(w.buf), w.d_phred.data_ptr(), w.d_calls.data_ptr(), sp))


# the resident run: what every host-fed step has to reproduce
w.steps_done = 0
w.step()
torch.cuda.synchronize()
want_calls, want_phred = w.d_calls.clone(), w.d_phred.clone()
bytes_per_read = {"planes": 80 + gtx.READ_META.itemsize + gtx.SCORE_ITEM.itemsize,
                  "packed": PACKED_STRIDE + gtx.READ_META.itemsize + gtx.SCORE_ITEM.itemsize + (4.0 * (n + chunks) + 2.0 * len(exc)) / n}
results = {"planes": [], "packed": []}
for b in range(2):
    free[b].record(w.stream)
for r in range(args.rounds):
    for kind in ("planes", "packed"):
        one_step(kind)  # (warm-up of this layout)
        torch.cuda.synchronize()
        w.d_calls.zero_()
        w.d_phred.zero_()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_step(kind)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        same = bool(torch.equal(want_calls, w.d_calls)) and bool(torch.equal(want_phred, w.d_phred))
        done = n * args.steps
        line = {"round": r, "layout": kind, "reads_per_s": done / dt, "ms_per_step": 1000.0 * dt / args.steps,
                "host_bytes_per_read": round(bytes_per_read[kind], 3), "pcie_gbs": done * bytes_per_read[kind] / dt / 1e9,
                "calls_equal_resident_run": same}
        results[kind].append(line)
        print(json.dumps(line), flush=True)
best = {k: max(x["reads_per_s"] for x in v) for k, v in results.items()}
print(json.dumps({"summary": True, "reads": n, "chunks": chunks, "steps": args.steps, "rounds": args.rounds, "exceptions": int(len(exc)),
                  "host_pack_s": round(pack_s, 3), "best_reads_per_s": best, "packed_over_planes": best["packed"] / best["planes"],
                  "all_calls_equal": all(x["calls_equal_resident_run"] for v in results.values() for x in v)}), flush=True)
w.close()
