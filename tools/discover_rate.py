#!/usr/bin/env python
"""What a region's discovery costs as one call -- gtx_discover_region, from host arrays to the sites file -- beside the same stages
called piece by piece from the binding (gtx_disc_events_batch, lib.disc_first_pass_device, gtx_disc_merge, lib.disc_second_file per
file: the chain a Python host had before the region call existed), on four files of one sample over a 50 kb and a 1 Mb region: the
simulated 30x alignments of tools/disc_rate.py, the reads of each file drawn on their own.  gtx_discover_region is timed with one
and with four threads; all three between device synchronises on the host's clock, one warm-up and --repeats timed runs, medians with
the extremes, milliseconds.  The chain's time includes its uploads (torch) as the region call's includes its own; the region call
also writes the records and the text, which the chain does not.  `waits`: per file the rounds' share -- launches and waits more than
work -- measured as the second pass alone on one thread.  A first measurement, not a bar; the results are checked against the
restatement by the tests, not here (the three texts of a region are compared with each other).
  python tools/discover_rate.py [--repeats R] [--regions 50000,1000000] [--out profiles/discover_rate.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disc_rate import BUCKET, COVERAGE, L_READ, alignments  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402

N_FILES, STRIDE, QUAL_STRIDE = 4, 80, 160


def timed(fn, repeats):
    fn()  # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


def region(ref_len, seed, repeats):
    L = gtx.lib()
    files, ref = [], None
    for f in range(N_FILES):
        ref, reads, cigar, codes, qual = alignments(ref_len, seed, read_seed=1000 * seed + f)
        files.append(dict(planes=gtx.pack_planes(gtx.pack_nibbles(codes, stride=STRIDE), STRIDE), plane_stride=STRIDE, qual=qual, qual_stride=QUAL_STRIDE, reads=reads,
                          cigar=cigar))
    last = {}

    def in_one_call(n_threads):
        last[n_threads] = gtx.discover_region(ref, 0, "chr1", files, n_threads=n_threads)

    def piece_by_piece():
        h = C.c_void_p()
        gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
        try:
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
            merged = np.zeros(0, np.uint32)
            for f, a in enumerate(files):
                n = len(a["reads"])
                d_planes, d_qual, d_reads, d_cigar = dev(a["planes"]), dev(a["qual"]), dev(a["reads"]), dev(a["cigar"])
                cap = 16 * n
                d_events = torch.zeros(cap * gtx.DISC_EVENT.itemsize, dtype=torch.uint8, device="cuda:0")
                d_counts, d_out = torch.zeros(16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * gtx.DISC_READ_OUT.itemsize + 16, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                gtx.check(L.gtx_disc_events_batch(h, d_planes.data_ptr(), STRIDE, d_qual.data_ptr(), QUAL_STRIDE, d_reads.data_ptr(), d_cigar.data_ptr(), n,
                                                  d_events.data_ptr(), cap, d_counts.data_ptr(), d_out.data_ptr(), None))
                words = gtx.disc_first_pass_device(h, d_planes.data_ptr(), STRIDE, d_reads.data_ptr(), d_cigar.data_ptr(), d_out.data_ptr(), n, d_events.data_ptr(),
                                                   d_counts.data_ptr(), BUCKET, file_index=f, cap=1 << 20)
                out, n_words = np.zeros(len(merged) + len(words) + 16, np.uint32), C.c_uint64()
                gtx.check(L.gtx_disc_merge(gtx._p(merged) if len(merged) else None, len(merged), gtx._p(words), len(words), gtx._p(out), len(out), C.byref(n_words)))
                merged = out[:n_words.value].copy()
            good = None
            for f, a in enumerate(files):
                got = gtx.disc_second_file(h, ref_len, a["planes"], STRIDE, a["reads"], a["cigar"], merged, f, bucket_size=BUCKET)
                good = got["good"] if good is None else good | got["good"]
            last["chain"] = (merged, good)
        finally:
            torch.cuda.synchronize()
            L.gtx_disc_destroy(h)

    row = {"region_bases": ref_len, "files": N_FILES, "reads_per_file": len(files[0]["reads"]),
           "discover_region_1_thread": timed(lambda: in_one_call(1), repeats), "discover_region_4_threads": timed(lambda: in_one_call(4), repeats),
           "piece_by_piece_from_the_binding": timed(piece_by_piece, repeats)}
    one, four = last[1], last[4]
    assert one["text"] == four["text"] and np.array_equal(one["words"], four["words"]) and np.array_equal(one["words"], last["chain"][0])
    entries, _ = gtx.disc_indel_table(one["words"])
    assert np.array_equal(one["good"], entries["good"].astype(bool) | last["chain"][1])
    # the rounds' share: every file's second pass alone, on one thread, from arrays that are on the device already
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
    dev = lambda a: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
    on_device = [(dev(a["planes"]), dev(a["reads"]), dev(a["cigar"]), len(a["reads"])) for a in files]
    torch.cuda.synchronize()

    def second_passes():
        for f, (p, r, c, n) in enumerate(on_device):
            gtx.disc_second_file_c(h, p.data_ptr(), STRIDE, r.data_ptr(), c.data_ptr(), n, one["words"], f, bucket_size=BUCKET, state=False)

    row["second_passes_alone_1_thread"] = timed(second_passes, repeats)
    torch.cuda.synchronize()
    L.gtx_disc_destroy(h)
    row.update(records=int(len(one["variants"])), table_entries=int(len(one["good"])), entries_good_at_the_end=int(one["good"].sum()), text_bytes=len(one["text"]),
               list_entries=[st["n_list"] for st in one["stats"]], rounds_done=[st["rounds"]["rounds_done"] for st in one["stats"]],
               pairs_aligned=[st["rounds"]["pairs_aligned"] for st in one["stats"]], pairs_refused=[st["rounds"]["pairs_refused"] for st in one["stats"]])
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--regions", default="50000,1000000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"tool": "tools/discover_rate.py", "device_name": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
           "read_length": L_READ, "coverage": COVERAGE, "bucket_size": BUCKET,
           "regions": [region(int(r), 7 + i, args.repeats) for i, r in enumerate(args.regions.split(","))]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
