#!/usr/bin/env python
"""What a file's rounds cost -- discovery's second pass from the aligner on, gtx_disc_second_rounds over the whole list of
gtx_disc_second_plan -- on the simulated 30x alignments of tools/disc_rate.py over a 50 kb and a 1 Mb region.  The indel table comes
from the device's own first pass over the same reads (file 0); in front of every run the intake is made again (it resets the
reads' state), the counters are cleared and the event array is empty.  A whole file's rounds are timed between device events on a
stream of its own (the call waits for the stream several times a round: the grid sizes come from counts), one warm-up and --repeats
timed runs; medians with the extremes beside the host's clock, milliseconds.  The record is a first measurement, not a bar; the
results are checked against the restatement by the tests, not here.
  python tools/disc_rounds_rate.py [--repeats R] [--out profiles/disc_rounds_rate.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disc_rate import BUCKET, COVERAGE, L_READ, alignments  # noqa: E402
from disc_second_rate import timed_ms  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402


def region(ref_len, seed, repeats):
    L = gtx.lib()
    ref, reads, cigar, codes, qual = alignments(ref_len, seed)
    n, stride = len(reads), 80
    planes = gtx.pack_planes(gtx.pack_nibbles(codes, stride=stride), stride)
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
    zeros = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device="cuda:0")  # noqa: E731
    d_planes, d_qual, d_reads, d_cigar = dev(planes), dev(qual), dev(reads), dev(cigar)
    cap = 16 * n
    d_events, d_counts, d_out = zeros(cap * gtx.DISC_EVENT.itemsize), zeros(8), zeros(n * gtx.DISC_READ_OUT.itemsize)
    torch.cuda.synchronize()
    gtx.check(L.gtx_disc_events_batch(h, d_planes.data_ptr(), stride, d_qual.data_ptr(), 160, d_reads.data_ptr(), d_cigar.data_ptr(), n, d_events.data_ptr(), cap,
                                      d_counts.data_ptr(), d_out.data_ptr(), None))
    words = gtx.disc_first_pass_device(h, d_planes.data_ptr(), stride, d_reads.data_ptr(), d_cigar.data_ptr(), d_out.data_ptr(), n, d_events.data_ptr(),
                                       d_counts.data_ptr(), BUCKET, file_index=0, cap=1 << 20)
    entries, letters = gtx.disc_indel_table(words)
    nt, nb = len(entries), gtx.disc_second_buckets(ref_len, BUCKET)
    d_table, d_letters = zeros(nt * gtx.DISC_INDEL.itemsize), zeros(len(letters))
    gtx.check(L.gtx_disc_indel_table_upload(h, gtx._p(entries) if nt else None, nt, gtx._p(letters) if len(letters) else None, len(letters), d_table.data_ptr(),
                                            d_letters.data_ptr(), None))
    o = dict(second=zeros(n * gtx.DISC_SECOND_READ.itemsize), bucket_max=zeros(4 * nb), global_max=zeros(4 * nb), max_read_size=zeros(4), bucket_reads=zeros(4 * n),
             bucket_off=zeros(4 * (nb + 1)), found=zeros(4 * ((nt + 31) // 32)))
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def intake():
        gtx.check(L.gtx_disc_second_intake(h, d_planes.data_ptr(), stride, d_reads.data_ptr(), d_cigar.data_ptr(), n, BUCKET, d_table.data_ptr(), d_letters.data_ptr(), nt,
                                           len(letters), o["second"].data_ptr(), o["bucket_max"].data_ptr(), o["global_max"].data_ptr(), o["max_read_size"].data_ptr(),
                                           o["bucket_reads"].data_ptr(), o["bucket_off"].data_ptr(), o["found"].data_ptr(), s))

    intake()
    torch.cuda.synchronize()
    found = o["found"].cpu().numpy()[:4 * ((nt + 31) // 32)].view(np.uint32)
    lst = gtx.disc_second_plan(entries, found, 0)
    d_lst = dev(np.concatenate([lst, np.zeros(4, np.uint32)]).astype(np.uint32))
    event_cap = 2 * n
    d_ev, d_support = zeros(event_cap * gtx.DISC_SECOND_EVENT.itemsize), zeros(nt * gtx.DISC_SECOND_SUPPORT.itemsize)
    last = {}

    def before():
        intake()
        d_support.zero_()
        torch.cuda.synchronize()

    def rounds():
        status, used, stats = gtx.disc_second_rounds(h, d_planes.data_ptr(), stride, d_lst.data_ptr(), 0, len(lst), d_table.data_ptr(), d_letters.data_ptr(), nt, len(letters),
                                                     o["second"].data_ptr(), n, d_ev.data_ptr(), event_cap, 0, BUCKET, o["bucket_max"].data_ptr(),
                                                     o["global_max"].data_ptr(), o["max_read_size"].data_ptr(), o["bucket_reads"].data_ptr(), o["bucket_off"].data_ptr(),
                                                     d_support.data_ptr(), s)
        assert status == 0, "the event array of %d entries is too small" % event_cap
        last.update(stats, events_in_use=used)

    row = {"region_bases": ref_len, "reads": n, "table_entries": nt, "list_entries": int(len(lst)), "rounds": timed_ms(rounds, stream, repeats, before=before)}
    torch.cuda.synchronize()
    support = d_support.cpu().numpy()[:nt * gtx.DISC_SECOND_SUPPORT.itemsize].view(gtx.DISC_SECOND_SUPPORT)
    row.update({k: last[k] for k in ("rounds_done", "rounds_skipped", "pairs", "pairs_aligned", "pairs_refused", "windows_built", "compactions", "events_in_use")})
    row["entries_with_good_support_after"] = int(gtx.disc_second_decide(entries, lst, support).sum())
    if last["rounds_done"]:
        row["ms_per_round"] = round(row["rounds"]["median_ms"] / last["rounds_done"], 4)
    L.gtx_disc_destroy(h)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--regions", default="50000,1000000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"tool": "tools/disc_rounds_rate.py", "device_name": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
           "read_length": L_READ, "coverage": COVERAGE, "bucket_size": BUCKET,
           "regions": [region(int(r), 7 + i, args.repeats) for i, r in enumerate(args.regions.split(","))]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
