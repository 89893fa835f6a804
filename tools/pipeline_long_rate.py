#!/usr/bin/env python3
"""BAM files -> VCF text through gtx_pipeline_run at 150, 2 x 250 and 1 000-base reads, and what a gtx_regions_run with
max_read_len = 1 000 holds on the device.
  python tools/pipeline_long_rate.py [--frags N] [--chunk C] [--threads T]
Per leg: reads/s over the call, the decode / push / enqueue split of gtx_pipeline_stats, and whether the VCF text equals a
resident run of the same reads (gtx_stream_push -> gtx_align_batch_planes -> gtx_score_batch_flags in one batch)."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import threading
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import harness  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402
from test_gpu_pipeline_long_reads import RB, NAMES, ragged_case, write_bams, text_of, resident, _region_jobs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frags", type=int, default=60000, help="fragments (pairs or unpaired reads) per leg")
ap.add_argument("--chunk", type=int, default=65536)
ap.add_argument("--threads", type=int, default=2, help="pipeline threads (one BAM file per sample, two samples)")
ap.add_argument("--conn-cap", type=int, default=1 << 24, help="far-pair connections the accumulator blocks log (1 000-base reads span many sites)")
ap.add_argument("--regions", type=int, default=8, help="regions of the gtx_regions_run memory check (0: skip)")
args = ap.parse_args()
L = gtx.lib()
tmp = Path(tempfile.mkdtemp(prefix="gtx_long_rate_"))

LEGS = [("150", [150], 0), ("2x250", [250], 0), ("1000", [1000], 1000)]
for name, lengths, max_len in LEGS:
    t0 = time.perf_counter()
    ref, recs, codes, rec = ragged_case(lengths, args.frags, seed=17, n_ref=200000, dup_frac=0.05, n_rate=0.001)
    paths = write_bams(tmp, rec, codes, tag=name)
    t_write = time.perf_counter() - t0
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0, max_read_len=max_len)
    pitch = max(80, (max(lengths) + 31) // 32 * 16)
    _, want = resident(ctx, paths, pitch, args.conn_cap)
    for rep in range(2):
        buf = gtx.ScoreBuffers()
        gtx.check(L.gtx_scores_alloc(ctx.h, 2, args.conn_cap, C.byref(buf), None))
        t1 = time.perf_counter()
        st = gtx.pipeline_run(ctx, paths, args.threads, buf, harness.REC_WORDS, len(rec), chunk=args.chunk, region="chr7")
        t_run = time.perf_counter() - t1
        text = text_of(ctx, buf)
        L.gtx_scores_free(ctx.h, C.byref(buf))
        print("%-6s %7d records (%d tasks): %.2f M reads/s over the call (%.3f s, loop %.3f s) | thread-s decode %.3f push %.3f enqueue %.3f | "
              "failed %d refused %d dropped %d | VCF equals resident run: %s | BAM written in %.1f s" % (
                  name, st["records"], st["tasks"], st["records"] / t_run / 1e6, t_run, st["loop_s"], st["decode_s"], st["push_s"], st["enqueue_s"],
                  st["records_failed"], st["score_items_refused"], st["connections_dropped"], text == want, t_write), flush=True)
    ctx.close()
    for q in paths:
        os.remove(q)

if args.regions:
    # device memory while a max_read_len = 1 000 run is under way: the least free memory a poller saw, against what was free before
    # (the library's device cache emptied first, so that the growth is what the run allocates)
    cases = [(RB + 40000 * r, ragged_case([150, 250, 400, 1000], 600, seed=40 + r, region_begin=RB + 40000 * r)) for r in range(args.regions)]
    params = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 1000)
    jobs, keep, want = _region_jobs(torch, cases, 512, params)
    torch.cuda.synchronize()
    for rep in range(2):
        L.gtx_device_cache_release()
        torch.cuda.empty_cache()
        free0, total = torch.cuda.mem_get_info(0)
        low = [free0]
        done = threading.Event()

        def poll():
            while not done.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
                time.sleep(0.002)

        th = threading.Thread(target=poll)
        th.start()
        t1 = time.perf_counter()
        got, st = jobs.run(NAMES, contig="chr7", rec_words=harness.REC_WORDS, conn_cap=args.conn_cap, params=params)
        t_run = time.perf_counter() - t1
        done.set()
        th.join()
        print("regions (max_read_len 1000): %d regions in %.2f s, %d builders / %d device / %d text threads, peak device growth %.2f GB "
              "(of %.0f GB), texts equal the oracle's: %s" % (args.regions, t_run, st["n_builders"], st["n_device_threads"], st["n_text_threads"],
                                                           (free0 - low[0]) / 1e9, total / 1e9, got == want), flush=True)
    del keep
