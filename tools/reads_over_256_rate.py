#!/usr/bin/env python3
"""Reads of 300 and 1 000 bases through a context made with max_read_len = 1000 (the long reads' two passes): reads/s of
gtx_align_batch on the snp100 and cfg3 graphs, the share of tasks that reach tier 2 (the exact pass), and the CPU oracle's
rate on the same reads (align + score, oracle_lib.sharded_genotyper on `threads` host threads).  Unpaired reads, forward only,
0.5 % substitutions, 0.1 % N; the device batch is `n` reads, tiled from 160 k distinct ones; 64-word record slots and a
256 MB arena for the longer records.
    python tools/reads_over_256_rate.py [n] [threads] [cpu_reads]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from graphtyper_amd import lib as gtx, synth  # noqa: E402
import harness  # noqa: E402
from oracle_lib import Oracle, sharded_genotyper  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
cpu_reads = int(sys.argv[3]) if len(sys.argv) > 3 else 160_000  # (sharded_genotyper: a thread per 10 000 reads at most)
rb = 1_000_000
ref = synth.make_reference(400_000, seed=42)
for kind in ("snp100", "cfg3"):
    recs = synth.make_snp_records(ref, 100, seed=7, region_begin=rb) if kind == "snp100" else synth.make_cfg3_records(ref, 100, seed=14, region_begin=rb)
    aav = kind == "cfg3"
    g = gtx.graph_from_records(synth.bases_to_str(ref), recs, region_begin=rb, add_all_variants=aav)
    ctx = gtx.Context(g, device=0, max_read_len=1000, big_record_words=1 << 26)
    for read_len in (300, 1000):
        codes, pos = synth.make_reads(ref, recs, 160_000, read_len=read_len, seed=5, region_begin=rb)
        order = np.argsort(pos, kind="stable")
        codes, pos = codes[order], pos[order]
        packed = gtx.pack_nibbles(codes)
        idx = np.arange(n) % len(codes)
        meta = harness.read_meta(np.full(n, read_len, np.uint16), flags=np.full(n, gtx.FLAG_FORWARD_ONLY), pos=pos[idx])
        d_seq = torch.from_numpy(packed[idx].reshape(-1)).to("cuda:0")
        d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1)).to("cuda:0")
        rec_words = 64
        d_rec = torch.zeros(n * 2 * rec_words, dtype=torch.int32, device="cuda:0")
        def run():
            gtx.check(gtx.lib().gtx_align_batch(ctx.h, d_seq.data_ptr(), packed.shape[1], d_meta.data_ptr(), n, d_rec.data_ptr(), rec_words, None))
        run()
        ctx.rewind_big_records()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 3
        t0.record()
        for _ in range(reps):
            ctx.rewind_big_records()
            run()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / reps
        tiers = ctx.long_pass_tasks()
        heads = d_rec.view(n, 2, rec_words)[:, 0, 0].cpu().numpy().view(np.uint32)
        over = int((((heads >> 16) & gtx.ST_ERROR_MASK) != 0).sum())
        # the oracle on the host, on the first cpu_reads of the same (position-sorted) reads
        o = Oracle(synth.bases_to_str(ref), recs, region_begin=rb, add_all_variants=aav)
        m = min(cpu_reads, len(codes))
        c0 = time.time()
        _, used = sharded_genotyper(o, codes[:m], pos[:m], threads=threads)
        cpu_s = time.time() - c0
        print("%-6s %4d bp  gpu %8.1f ms / %d reads = %10.0f reads/s   tier 1 tasks %d, tier 2 %d (%.4f %%), refused %d, overflow %d   "
              "oracle %d threads: %8.0f reads/s" % (kind, read_len, ms, n, n / ms * 1e3, tiers[0], tiers[1], 100.0 * tiers[1] / max(tiers[0], 1),
                                                 tiers[4], over, used, m / cpu_s), flush=True)
