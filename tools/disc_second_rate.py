#!/usr/bin/env python
"""What discovery's second pass costs up to the aligner, on the simulated 30x alignments of tools/disc_rate.py over a 50 kb and a
1 Mb region: the indel table comes from the device's own first pass over the same reads (file 0), then
  intake      gtx_disc_second_intake over all reads
  candidates  gtx_disc_second_candidates over the whole list of gtx_disc_second_plan, and over every table entry as a list
each timed with device events on a stream of its own around the call (the calls wait for the stream before they return), one
warm-up and --repeats timed runs; medians with the extremes, milliseconds.  At the 50 kb size the outputs are first checked against
the restatement (tests/disc_second_ref.py through tests/disc_second_cases.py).
  python tools/disc_second_rate.py [--repeats R] [--out profiles/disc_second_rate.json]"""
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

CHECKED_BASES = 50000


def timed_ms(fn, stream, repeats, before=lambda: None):
    before()
    fn()  # warm-up
    times, walls = [], []
    for _ in range(repeats):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before()
        torch.cuda.synchronize()
        t = time.perf_counter()
        begin.record(stream)
        fn()
        end.record(stream)
        end.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
        times.append(begin.elapsed_time(end))
    # (host_median_ms: the host's clock around the same call and the wait for its last event -- what the caller's thread pays)
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
            "host_median_ms": round(statistics.median(walls), 3)}


def check_against_the_restatement(ref, reads, cigar, codes, entries, letters, got, lists):
    """the device's arrays of one region against tests/disc_second_cases.py's comparison, list by list"""
    import disc_second_cases as sc
    nib_letter = {1: "A", 2: "C", 4: "G", 8: "T"}
    rs = []
    for r, row in zip(reads, codes):
        words = [int(w) for w in cigar[r["cigar_off"]:r["cigar_off"] + r["n_cigar"]]]
        rs.append(dict(pos=int(r["pos"]), cigar=words, seq="".join(nib_letter[int(c)] for c in row[:r["l_qseq"]]), qual=[30] * int(r["l_qseq"]), flag=int(r["flag"]),
                       mapq=int(r["mapq"])))
    table = [sc.ent(int(e["pos"]), chr(e["type"]), letters[e["seq_off"]:e["seq_off"] + e["len"]].tobytes().decode(), int(e["span"]), bool(e["good"]), int(e["file_index"]))
             for e in entries]
    for name, lst, pairs, counts in lists:
        case = sc.Case(ref, 0, rs, table, bucket_size=BUCKET, lst=[int(t) for t in lst], stride=80)
        how = sc.differs(case, dict(got, pairs=pairs, counts=counts))
        assert how is None, "the %s list differs from the restatement: %s" % (name, how)
        if name == "plan":
            assert [int(t) for t in lst] == sc.ref.plan(table, sc.expected(case)["found"], 0)


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
    # the table: the device's own first pass over these reads as file 0
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

    row = {"region_bases": ref_len, "reads": n, "buckets": nb, "table_entries": nt, "intake": timed_ms(intake, stream, repeats)}
    torch.cuda.synchronize()
    down = lambda t, dtype, count: t.cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype).copy()  # noqa: E731
    got = dict(second=down(o["second"], gtx.DISC_SECOND_READ, n), bucket_max=down(o["bucket_max"], np.int32, nb), global_max=down(o["global_max"], np.int32, nb),
               max_read_size=down(o["max_read_size"], np.uint32, 1), bucket_reads=down(o["bucket_reads"], np.uint32, n), bucket_off=down(o["bucket_off"], np.uint32, nb + 1),
               found=down(o["found"], np.uint32, (nt + 31) // 32))
    row["entries_found_in_the_file"] = int(sum(bin(int(w)).count("1") for w in got["found"]))
    lists = []
    for name, lst in (("plan", gtx.disc_second_plan(entries, got["found"], 0)), ("every_entry", np.arange(nt, dtype=np.uint32))):
        d_lst, d_pair_counts = dev(np.concatenate([lst, np.zeros(4, np.uint32)]).astype(np.uint32)), zeros(8)

        def rounds(d_pairs, pair_cap):
            gtx.check(L.gtx_disc_second_candidates(h, d_lst.data_ptr(), 0, len(lst), d_table.data_ptr(), nt, o["second"].data_ptr(), n, None, 0, BUCKET,
                                                   o["bucket_max"].data_ptr(), o["global_max"].data_ptr(), o["max_read_size"].data_ptr(), o["bucket_reads"].data_ptr(),
                                                   o["bucket_off"].data_ptr(), d_pairs, pair_cap, d_pair_counts.data_ptr(), s))

        rounds(None, 0)  # how many pairs there are
        torch.cuda.synchronize()
        total = int(down(d_pair_counts, np.uint32, 2)[0])
        d_pairs = zeros(total * gtx.DISC_SECOND_PAIR.itemsize)
        row["candidates_" + name] = dict(timed_ms(lambda: rounds(d_pairs.data_ptr(), total), stream, repeats, before=d_pair_counts.zero_), list_entries=int(len(lst)),
                                         pairs=total)
        torch.cuda.synchronize()
        lists.append((name, lst, down(d_pairs, gtx.DISC_SECOND_PAIR, total), down(d_pair_counts, np.uint32, 2)))
    if ref_len <= CHECKED_BASES:
        check_against_the_restatement(ref, reads, cigar, codes, entries, letters, got, lists)
        row["checked_against_the_restatement"] = True
    torch.cuda.synchronize()
    L.gtx_disc_destroy(h)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--regions", default="50000,1000000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"tool": "tools/disc_second_rate.py", "device_name": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
           "read_length": L_READ, "coverage": COVERAGE, "bucket_size": BUCKET,
           "regions": [region(int(r), 7 + i, args.repeats) for i, r in enumerate(args.regions.split(","))]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
