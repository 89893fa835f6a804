#!/usr/bin/env python
"""Inflate rates on BAM files of 150-base reads, GB/s of inflated bytes, at two deflate levels:
  kernel      gtx_inflate_batch alone on members resident on the device (HIP events around the launch)
  bgzf_call   gtx_inflate_bgzf: host buffer -> device -> host buffer, with its copies and the member parse
  reads_host  gtx_reads_* over the file with the host's team (GTX_BGZF_THREADS=16), record parsing included
  reads_dev   the same with gtx_reads_set_inflate_device, at several ring depths (GTX_BGZF_DEVICE_RING), with what
              gtx_reads_inflate_counts says became of the members
One warm-up and --repeats timed runs each, the median reported with the extremes; one process, one device.
  python tools/inflate_rate.py [--reads N] [--repeats R] [--out profiles/inflate_rate.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

os.environ.setdefault("GTX_BGZF_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphtyper_amd import lib as gtx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=600000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--levels", default="1,6")
ap.add_argument("--rings", default="256,1024,4096", help="GTX_BGZF_DEVICE_RING values of the reads_dev legs")
ap.add_argument("--out", default="")
args = ap.parse_args()


def bam_bytes(n, seed=1):
    """an uncompressed BAM stream of n unpaired 150-base reads, sorted, one read group"""
    rng = np.random.default_rng(seed)
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:250000000\n@RG\tID:a\tSM:person0\n"
    head = b"BAM\1" + np.int32(len(text)).tobytes() + text + np.int32(1).tobytes() + np.int32(5).tobytes() + b"chr1\0" + np.int32(250000000).tobytes()
    rec = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"), ("flag", "<u2"),
                    ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("tlen", "<i4"), ("name", "S8"), ("cigar", "<u4"), ("seq", "u1", 75), ("qual", "u1", 150),
                    ("aux", "u1", 9)])
    a = np.zeros(n, rec)
    a["block_size"], a["l_name"], a["mapq"], a["bin"], a["n_cigar"], a["l_seq"], a["mtid"], a["mpos"] = rec.itemsize - 4, 8, 60, 4680, 1, 150, -1, -1
    a["pos"] = np.sort(rng.integers(0, 200000000, n))
    a["name"] = np.char.add("r", np.char.zfill(np.arange(n).astype("U6"), 6)).astype("S8")
    a["cigar"] = 150 << 4
    codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=(n, 150))
    a["seq"] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    a["qual"] = np.minimum(40, rng.geometric(0.15, size=(n, 150)) + 20).astype(np.uint8)
    a["aux"] = np.frombuffer(b"RGZa\0ASC\x64", np.uint8)  # RG:Z:a, AS:C:100
    return head + a.tobytes()


def members_of(raw):
    at, rows = 0, []
    while at < len(raw):
        bsize = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        isize = int.from_bytes(raw[at + bsize - 4:at + bsize], "little")
        if isize:
            rows.append((at + 18, bsize - 26, int.from_bytes(raw[at + bsize - 8:at + bsize - 4], "little"), isize))
        at += bsize
    m = np.zeros(len(rows), gtx.INFLATE_MEMBER)
    m["in_off"], m["in_len"], m["crc32"], m["out_len"] = (np.array(c, np.uint64) for c in zip(*rows))
    m["out_off"] = np.concatenate([[0], np.cumsum(m["out_len"][:-1], dtype=np.uint64)])
    return m


def timed(f, repeats):
    f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        t.append(r if isinstance(r, float) else time.perf_counter() - t0)
    return t


def read_all(path, device):
    reads = gtx.Reads([path])
    if device:
        reads.set_inflate_device(0)
    recs = np.zeros(65536, gtx.STREAM_RECORD)
    seq = np.zeros((65536, 80), np.uint8)
    n, total = C.c_uint32(1), 0
    while n.value:
        gtx.check(gtx.lib().gtx_reads_next(reads.h, recs.ctypes.data, seq.ctypes.data, 80, 65536, C.byref(n)))
        total += n.value
    reads.close()
    assert total == args.reads, total


result = {"reads": args.reads, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "GTX_BGZF_THREADS": os.environ["GTX_BGZF_THREADS"],
          "levels": {}}
plain = bam_bytes(args.reads)
inflater = gtx.Inflater(0)
L = gtx.lib()
with tempfile.TemporaryDirectory() as tmp:
    for level in (int(x) for x in args.levels.split(",")):
        raw = gtx.bgzf_compress(plain, level)
        path = os.path.join(tmp, "l%d.bam" % level)
        open(path, "wb").write(raw)
        m = members_of(raw)
        d_in = torch.from_numpy(np.frombuffer(raw + bytes(8), np.uint8).copy()).cuda()
        d_m = torch.from_numpy(m.view(np.uint8).copy()).cuda()
        d_out = torch.zeros(len(plain), dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(len(m), dtype=torch.int32, device="cuda")
        legs = {}
        for crc in (1, 0):
            def kernel():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                inflater.batch(d_in.data_ptr(), len(raw), d_m.data_ptr(), len(m), d_out.data_ptr(), len(plain), d_st.data_ptr(), bool(crc),
                               torch.cuda.current_stream().cuda_stream)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / 1e3
            legs["kernel_crc%d" % crc] = timed(kernel, args.repeats)
            assert not d_st.any().item() and d_out.cpu().numpy().tobytes() == plain
        out = np.zeros(len(plain), np.uint8)
        n = C.c_uint64()
        legs["bgzf_call"] = timed(lambda: gtx.check(L.gtx_inflate_bgzf(inflater.h, raw, len(raw), out.ctypes.data, len(out), C.byref(n), 1)), args.repeats)
        assert out.tobytes() == plain
        legs["reads_host"] = timed(lambda: read_all(path, False), args.repeats)
        counts = {}
        for ring in (int(x) for x in args.rings.split(",")):
            os.environ["GTX_BGZF_DEVICE_RING"] = str(ring)
            before = gtx.reads_inflate_counts()
            legs["reads_dev_ring%d" % ring] = timed(lambda: read_all(path, True), args.repeats)
            # members per run: by the device, fell back to the host, inflated by the reader itself
            counts["ring%d" % ring] = [(a - b) // (args.repeats + 1) for a, b in zip(gtx.reads_inflate_counts(), before)]
        result["levels"][str(level)] = {"members": len(m), "compressed_bytes": len(raw), "inflated_bytes": len(plain), "reads_dev_members_device_fallback_reader": counts,
                                        "GBps": {k: {"median": round(len(plain) / statistics.median(v) / 1e9, 3), "min": round(len(plain) / max(v) / 1e9, 3),
                                                     "max": round(len(plain) / min(v) / 1e9, 3)} for k, v in legs.items()}}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    open(args.out, "w").write(text + "\n")
