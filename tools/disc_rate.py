#!/usr/bin/env python
"""What discovery's first pass costs behind the events kernel, on simulated 30x alignments of 150-base reads over a 50 kb and a 1 Mb
region (a diploid sample: a SNP every ~300 bases, a short indel every ~1500, 0.4 % base errors, 2 % of the reads at 12 %):
  host    gtx_disc_events_batch, the downloads of the events, the read states and the counts, gtx_disc_first_pass_haplotypes
  device  gtx_disc_events_batch, gtx_disc_first_pass_haplotypes_device (no per-read or per-event array comes down)
Both over the same device inputs and with the same result words (checked).  One warm-up and --repeats timed runs per path, each in
a timed region of its own that a device synchronise bounds; medians with the extremes, milliseconds.
  python tools/disc_rate.py [--repeats R] [--out profiles/disc_rate.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphtyper_amd import lib as gtx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--regions", default="50000,1000000")
ap.add_argument("--out", default="")
L_READ, COVERAGE, BUCKET = 150, 30, 50


def alignments(ref_len, seed, read_seed=None):
    """-> (reference str, reads gtx.DISC_READ, cigar words, codes [n, 160], qual [n, 160]), sorted by position.  read_seed: the reads
    are drawn from a generator of their own, so that several files of one region and one sample can be made (tools/discover_rate.py)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, ref_len).astype(np.int8)
    haps = [ref.copy(), ref.copy()]
    snps = np.arange(200, ref_len - 200, 300) + rng.integers(0, 100, len(np.arange(200, ref_len - 200, 300)))
    for p in snps:
        alt = (ref[p] + rng.integers(1, 4)) % 4
        for h in (0, 1):
            if h == 1 or rng.random() < 0.5:
                haps[h][p] = alt
    sites = np.arange(900, ref_len - 400, 1500)  # an indel each: (length > 0: insertion, < 0: deletion), on haplotype 1, half of them on both
    kinds = np.where(rng.random(len(sites)) < 0.5, 1, -1) * rng.integers(1, 9, len(sites))
    on_both = rng.random(len(sites)) < 0.5
    inserted = rng.integers(0, 4, (len(sites), 8)).astype(np.int8)
    n = ref_len * COVERAGE // L_READ
    if read_seed is not None:
        rng = np.random.default_rng(read_seed)
    start = np.sort(rng.integers(0, ref_len - L_READ - 10, n))
    hap = rng.integers(0, 2, n)
    j = np.arange(L_READ)
    # the indel a read carries: the first site inside [start + 10, start + 130) if its haplotype has it
    si = np.searchsorted(sites, start + 10)
    has = (si < len(sites))
    si = np.minimum(si, len(sites) - 1)
    has &= (sites[si] < start + 130) & ((hap == 1) | on_both[si])
    k = np.where(has, sites[si] - start, L_READ)  # bases in front of it
    ln = np.where(has, kinds[si], 0)
    ins_len, del_len = np.maximum(ln, 0), np.maximum(-ln, 0)
    src = start[:, None] + j[None, :] + np.where(j[None, :] >= k[:, None], del_len[:, None] - ins_len[:, None], 0)
    both_haps = np.stack(haps)
    codes = both_haps[hap[:, None], src]
    in_ins = (j[None, :] >= k[:, None]) & (j[None, :] < (k + ins_len)[:, None])
    codes = np.where(in_ins, inserted[si[:, None], np.clip(j[None, :] - k[:, None], 0, 7)], codes)
    noisy = rng.random(n) < 0.02
    err = rng.random((n, L_READ)) < np.where(noisy, 0.12, 0.004)[:, None]
    codes = np.where(err, (codes + rng.integers(1, 4, (n, L_READ))) % 4, codes).astype(np.uint8)
    nib = np.zeros((n, 160), np.uint8)
    nib[:, :L_READ] = np.array([1, 2, 4, 8], np.uint8)[codes]
    qual = np.zeros((n, 160), np.uint8)
    qual[:, :L_READ] = np.where(rng.random((n, L_READ)) < 0.15, rng.integers(2, 25, (n, L_READ)), rng.integers(25, 41, (n, L_READ)))
    reads = np.zeros(n, gtx.DISC_READ)
    reads["pos"], reads["mapq"], reads["l_qseq"] = start, rng.choice([60, 60, 60, 37, 12], n), L_READ
    reads["flag"] = rng.choice([1 | 2 | 64, 1 | 2 | 128 | 16, 1 | 64 | 16, 1 | 2 | 128 | 32], n)
    reads["n_cigar"] = np.where(has, 3, 1)
    reads["cigar_off"] = np.concatenate([[0], np.cumsum(reads["n_cigar"])[:-1]])
    cigar = np.zeros(int(reads["n_cigar"].sum()) + 1, np.uint32)
    off = reads["cigar_off"]
    cigar[off[~has]] = L_READ << 4
    cigar[off[has]] = k[has] << 4
    cigar[off[has] + 1] = np.where(ln[has] > 0, (ins_len[has] << 4) | 1, (del_len[has] << 4) | 2)
    cigar[off[has] + 2] = (L_READ - k[has] - ins_len[has]) << 4
    return "".join("ACGT"[c] for c in ref), reads, cigar, nib, qual


def median_ms(fn, repeats):
    fn()  # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


def region(ref_len, seed):
    L = gtx.lib()
    ref, reads, cigar, codes, qual = alignments(ref_len, seed)
    n, stride = len(reads), 80
    nib = gtx.pack_nibbles(codes, stride=stride)
    planes = gtx.pack_planes(nib, stride)
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
    d_planes, d_qual, d_reads, d_cigar = dev(planes), dev(qual), dev(reads), dev(cigar)
    cap = 16 * n
    d_events = torch.zeros(cap * gtx.DISC_EVENT.itemsize, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(n * gtx.DISC_READ_OUT.itemsize, dtype=torch.uint8, device="cuda:0")
    _p = gtx._p
    result = {}

    def events():
        d_counts.zero_()
        torch.cuda.synchronize()
        gtx.check(L.gtx_disc_events_batch(h, d_planes.data_ptr(), stride, d_qual.data_ptr(), 160, d_reads.data_ptr(), d_cigar.data_ptr(), n, d_events.data_ptr(),
                                          cap, d_counts.data_ptr(), d_out.data_ptr(), None))

    def host():
        events()
        torch.cuda.synchronize()
        counts = d_counts.cpu().numpy()
        assert counts[1] == 0
        ev = d_events[:int(counts[0]) * gtx.DISC_EVENT.itemsize].cpu().numpy().view(gtx.DISC_EVENT)
        ro = d_out.cpu().numpy().view(gtx.DISC_READ_OUT)
        words, nw = np.zeros(1 << 20, np.uint32), C.c_uint64()
        rc = L.gtx_disc_first_pass_haplotypes(h, _p(reads), _p(cigar), _p(ro), n, _p(ev), len(ev), _p(nib), stride, BUCKET, 0, _p(words), len(words), C.byref(nw))
        if rc == 5 and nw.value > len(words):  # (as the device path's helper does: once more with the size the call names)
            words = np.zeros(int(nw.value), np.uint32)
            rc = L.gtx_disc_first_pass_haplotypes(h, _p(reads), _p(cigar), _p(ro), n, _p(ev), len(ev), _p(nib), stride, BUCKET, 0, _p(words), len(words), C.byref(nw))
        gtx.check(rc)
        result["host"], result["events"] = words[:nw.value], int(counts[0])

    def device():
        events()
        result["device"] = gtx.disc_first_pass_device(h, d_planes.data_ptr(), stride, d_reads.data_ptr(), d_cigar.data_ptr(), d_out.data_ptr(), n,
                                                      d_events.data_ptr(), d_counts.data_ptr(), BUCKET, file_index=0, cap=1 << 20)

    row = {"region_bases": ref_len, "reads": n, "events_only": median_ms(events, args.repeats), "host": median_ms(host, args.repeats),
           "device": median_ms(device, args.repeats)}
    assert np.array_equal(result["host"], result["device"]), "the two paths disagree"
    row["events"], row["result_words"] = result["events"], int(len(result["device"]))
    row["host_over_device"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 2)
    L.gtx_disc_destroy(h)
    return row


if __name__ == "__main__":  # (tools/disc_second_rate.py takes alignments() from here)
    args = ap.parse_args()
    out = {"tool": "tools/disc_rate.py", "device_name": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
           "read_length": L_READ, "coverage": COVERAGE, "bucket_size": BUCKET,
           "regions": [region(int(r), 7 + i) for i, r in enumerate(args.regions.split(","))]}
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
