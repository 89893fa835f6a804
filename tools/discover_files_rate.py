#!/usr/bin/env python
"""What a region's discovery costs from BAM files -- gtx_discover_files: read, inflate, one upload, the unpack kernel, then what
gtx_discover_region does -- beside gtx_discover_region from host arrays, on the inputs of tools/discover_rate.py: four files of one
sample at 30x over a 50 kb and a 1 Mb region, each written once as a BAM file (one read group, names of nine bytes, two aux tags) and
read from the page cache.  In one process, with one and with four threads:
  (a) files            gtx_discover_files from the four paths
  (b) arrays           gtx_discover_region over arrays made beforehand from the same reads: its time leaves out making them
  (c) arrays_made      the arrays made on the host in every run -- gtx_pack_planes over the nibble rows, copies of the quality rows, the
                       reads and the CIGAR words -- and then (b): what a caller has to do today, WITHOUT the BAM parsing it would also need
and the pieces of (a) called one by one over the four files on one thread: gtx_disc_bam_read (read and inflate), the upload of the
stream and the two tables (torch, from pageable memory as the library's is), gtx_disc_bam_unpack (the call: it reads the two tables
back for its checks, which gtx_discover_files does on its host copies).  One warm-up and --repeats timed runs between device
synchronises on the host's clock; medians with the extremes, milliseconds.  A first measurement, not a bar; (a) and (b) are compared
byte for byte here, against the restatement by the tests.
The device front (gtx_discover_files_front, front 1: members inflated, records walked and unpacked on the device) runs beside them in
the same process, over two layouts of the same records: "cut" -- the files above, cut by gtx_bgzf_compress wherever members fall, so
that every member but the first ends inside a record and the walk resolves the whole file on one wavefront (all misses) -- and
"aligned" -- htslib's layout, no record crosses a member (all hits):
  (d) files_device     gtx_discover_files_front, front 1, from the four paths of a layout
and its pieces over the four files on one thread: the file read and its members' headers parsed (numpy / Python here, C in the
library), the upload of the compressed bytes and the descriptors (torch, pageable), gtx_inflate_batch, gtx_disc_bam_walk for the
counts alone and with the tables (the second includes the first); the unpack kernel is the one of (a).
  python tools/discover_files_rate.py [--repeats R] [--regions 50000,1000000] [--out profiles/discover_files_rate.json]"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disc_rate import BUCKET, COVERAGE, L_READ, alignments  # noqa: E402
from discover_rate import N_FILES, QUAL_STRIDE, STRIDE, timed  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402


MEMBER = 0xff00  # the input bytes gtx_bgzf_compress gives a member at most


def write_bam(path, ref_len, reads, cigar, nibbles, qual, aligned_path=None):
    """the reads as a BAM file of one read group, compressed by the library's BGZF writer; aligned_path: the same bytes once more, in
    members that end where records end (the header in members of its own)"""
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n@RG\tID:g\tSM:sample\n" % ref_len
    out = [b"BAM\1", struct.pack("<i", len(text)), text.encode(), struct.pack("<ii", 1, 5), b"chr1\0", struct.pack("<i", ref_len)]
    aux = b"RGZg\0NMC\1"
    for i, r in enumerate(reads):
        name = b"r%07d\0" % (i % 10000000)
        words = cigar[r["cigar_off"]:r["cigar_off"] + r["n_cigar"]].astype("<u4").tobytes()
        body = struct.pack("<iiBBHHHIiii", 0, int(r["pos"]), len(name), int(r["mapq"]), 4680, int(r["n_cigar"]), int(r["flag"]), int(r["l_qseq"]), -1, -1, 0)
        body += name + words + nibbles[i, :(r["l_qseq"] + 1) // 2].tobytes() + qual[i, :r["l_qseq"]].tobytes() + aux
        out += [struct.pack("<i", len(body)), body]
    with open(path, "wb") as f:
        f.write(gtx.bgzf_compress(b"".join(out)))
    if aligned_path is None:
        return
    head, records = b"".join(out[:6]), [out[k] + out[k + 1] for k in range(6, len(out), 2)]
    chunks, chunk = [head[at:at + MEMBER] for at in range(0, len(head), MEMBER)], []
    size = 0
    for r in records:
        if size + len(r) > MEMBER and chunk:
            chunks.append(b"".join(chunk))
            chunk, size = [], 0
        chunk.append(r)
        size += len(r)
    if chunk:
        chunks.append(b"".join(chunk))
    with open(aligned_path, "wb") as f:
        f.write(b"".join(gtx.bgzf_compress(c, with_eof=False) for c in chunks) + gtx.bgzf_compress(b""))


def members_of(data):
    """a BGZF file's bytes -> (INFLATE_MEMBER descriptors of the members with data, out_off the running sum of ISIZE; the inflated size)"""
    rows, at, total = [], 0, 0
    while at < len(data):
        xlen, = struct.unpack_from("<H", data, at + 10)
        bsize, = struct.unpack_from("<H", data, at + 16)  # (BC is the first subfield of every member the library writes)
        crc, isize = struct.unpack_from("<II", data, at + bsize + 1 - 8)
        if isize:
            rows.append((at + 12 + xlen, total, bsize + 1 - 12 - xlen - 8, isize, crc, 0))
        total += isize
        at += bsize + 1
    return np.array(rows, gtx.INFLATE_MEMBER), total


def device_front(L, paths, tables, ref, repeats):
    """the pieces of the device front over the files of one layout, called one by one on this thread"""
    row, host = {}, []

    def read_and_parse():
        host[:] = []
        for p in paths:
            with open(p, "rb") as f:
                data = f.read()
            host.append((np.frombuffer(data + bytes(8), np.uint8),) + members_of(data))
    row["read_and_parse"] = timed(read_and_parse, repeats)
    row["members"] = [int(len(m)) for _, m, _ in host]
    on_device = []

    def upload():
        on_device[:] = [(torch.from_numpy(d).to("cuda:0"), torch.from_numpy(m.view(np.uint8)).to("cuda:0")) for d, m, _ in host]
    row["upload"] = timed(upload, repeats)
    inflater = gtx.Inflater(0)
    outs = [(torch.zeros(total + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(len(m) + 4, dtype=torch.int32, device="cuda:0")) for _, m, total in host]

    def inflate():
        for (d, m, total), (dd, dm), (o, st) in zip(host, on_device, outs):
            inflater.batch(dd.data_ptr(), len(d) - 8, dm.data_ptr(), len(m), o.data_ptr(), total, st.data_ptr())
    row["inflate"] = timed(inflate, repeats)
    assert all(int(st.abs().sum()) == 0 for _, st in outs)
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
    headers = [total - len(t["stream"]) for (_, _, total), t in zip(host, tables)]
    cuts = [[int(e) - hd for e in (m["out_off"] + m["out_len"]).tolist() if hd < e < total] for (_, m, total), hd in zip(host, headers)]
    counts = []

    def walk_count():
        counts[:] = [gtx.disc_bam_walk(h, o.data_ptr() + hd, total - hd, c)[1] for (_, _, total), (o, _), hd, c in zip(host, outs, headers, cuts)]
    row["walk_count"] = timed(walk_count, repeats)
    made = [(torch.zeros(4 * len(t["reads"]) + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * len(t["reads"]) + 16, dtype=torch.uint8, device="cuda:0"))
            for t in tables]

    def walk_tables():
        for (_, _, total), (o, _), hd, c, (offs, reads), t in zip(host, outs, headers, cuts, made, tables):
            gtx.disc_bam_walk(h, o.data_ptr() + hd, total - hd, c, offs.data_ptr(), reads.data_ptr(), len(t["reads"]))
    row["walk_count_and_emit"] = timed(walk_tables, repeats)
    for (offs, reads), t, c in zip(made, tables, counts):  # the device's tables are the host walk's
        assert (c["status"], c["n_reads"], c["n_cigar"]) == (0, len(t["reads"]), t["n_cigar"])
        assert offs.cpu().numpy()[:-16].tobytes() == t["offsets"].tobytes() and reads.cpu().numpy()[:-16].tobytes() == t["reads"].tobytes()
    row["segments"] = [len(c) + 1 for c in cuts]
    row["segments_hit"] = [c["segments_hit"] for c in counts]
    row["segments_rewalked"] = [c["segments_rewalked"] for c in counts]
    torch.cuda.synchronize()
    L.gtx_disc_destroy(h)
    inflater.close()
    return row


def outputs(run):
    return run["words"].tobytes(), run["good"].tobytes(), run["variants"].tobytes(), run["letters"], run["ids"].tobytes(), run["text"]


def region(ref_len, seed, repeats, tmp):
    L = gtx.lib()
    made, paths, aligned, ref = [], [], [], None
    for f in range(N_FILES):
        ref, reads, cigar, codes, qual = alignments(ref_len, seed, read_seed=1000 * seed + f)
        nibbles = gtx.pack_nibbles(codes, stride=STRIDE)
        made.append((nibbles, qual, reads, cigar))
        paths.append(os.path.join(tmp, "r%d_f%d.bam" % (ref_len, f)))
        aligned.append(os.path.join(tmp, "r%d_f%d_aligned.bam" % (ref_len, f)))
        write_bam(paths[-1], ref_len, reads, cigar, nibbles, qual, aligned[-1])

    def arrays():
        return [dict(planes=gtx.pack_planes(n, STRIDE), plane_stride=STRIDE, qual=q.copy(), qual_stride=QUAL_STRIDE, reads=r.copy(), cigar=c.copy()) for n, q, r, c in made]
    before, last = arrays(), {}

    def files(n_threads):
        last["files", n_threads] = gtx.discover_files(ref, 0, "chr1", paths, n_threads=n_threads)

    def files_device(layout, n_threads):
        last["device", layout, n_threads] = run = gtx.discover_files(ref, 0, "chr1", aligned if layout == "aligned" else paths, n_threads=n_threads, front="device")
        front = run.pop("front")
        assert all(f["fell_back"] == 0 and f["members_device"] == f["members"] and (f["segments_rewalked"] == 0) == (layout == "aligned") for f in front), front

    def from_arrays(n_threads, fresh):
        last["arrays", n_threads] = gtx.discover_region(ref, 0, "chr1", arrays() if fresh else before, n_threads=n_threads)

    row = {"region_bases": ref_len, "files": N_FILES, "reads_per_file": len(made[0][2]), "bam_bytes": [os.path.getsize(p) for p in paths]}
    for n_threads in (1, 4):
        row["threads_%d" % n_threads] = {"a_files": timed(lambda: files(n_threads), repeats), "b_arrays": timed(lambda: from_arrays(n_threads, False), repeats),
                                         "c_arrays_made": timed(lambda: from_arrays(n_threads, True), repeats),
                                         "d_files_device_cut": timed(lambda: files_device("cut", n_threads), repeats),
                                         "d_files_device_aligned": timed(lambda: files_device("aligned", n_threads), repeats)}
    assert len({outputs(r) for r in last.values()}) == 1  # one result, whichever way
    # the pieces of (a), over the four files, on this thread
    handles = []

    def read_all():
        while handles:
            L.gtx_disc_bam_destroy(handles.pop())
        for p in paths:
            h = C.c_void_p()
            gtx.check(L.gtx_disc_bam_read(p.encode(), C.byref(h)))
            handles.append(h)
    row["read_and_inflate"] = timed(read_all, repeats)
    while handles:
        L.gtx_disc_bam_destroy(handles.pop())
    tables = [gtx.disc_bam_read(p) for p in paths]
    row["stream_bytes"] = [int(len(t["stream"])) for t in tables]
    on_device = []

    def upload():
        on_device[:] = [[torch.from_numpy(t[k].view(np.uint8)).to("cuda:0") for k in ("stream", "offsets", "reads")]
                        for t in tables]
    row["upload"] = timed(upload, repeats)
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(ref.encode(), len(ref), 0, 0, C.byref(h)))
    plane_stride, qual_stride = max(16, (L_READ + 31) // 32 * 16), max(4, (L_READ + 3) // 4 * 4)
    outs = [(torch.zeros(len(t["reads"]) * plane_stride + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(len(t["reads"]) * qual_stride + 16, dtype=torch.uint8, device="cuda:0"),
             torch.zeros(4 * t["n_cigar"] + 16, dtype=torch.uint8, device="cuda:0")) for t in tables]

    def unpack():
        for t, (s, o, r), (p, q, c) in zip(tables, on_device, outs):
            gtx.disc_bam_unpack(h, s.data_ptr(), len(t["stream"]), o.data_ptr(), r.data_ptr(), len(t["reads"]), p.data_ptr(), plane_stride, q.data_ptr(), qual_stride,
                                c.data_ptr(), t["n_cigar"])
    row["unpack_calls"] = timed(unpack, repeats)
    # the same calls by the device's clock (the kernels and the read-backs between two events): one more run
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    unpack()
    end.record()
    torch.cuda.synchronize()
    row["unpack_calls_by_the_device_clock_ms"] = round(start.elapsed_time(end), 3)
    for (p, q, c), (n, qq, r, cg) in zip(outs, made):  # what the kernel left is what the host repack makes
        assert np.array_equal(p.cpu().numpy()[:-16].reshape(len(r), plane_stride), gtx.pack_planes(n, plane_stride))
        assert np.array_equal(q.cpu().numpy()[:-16].reshape(len(r), qual_stride)[:, :L_READ], qq[:, :L_READ])
        assert np.array_equal(c.cpu().numpy()[:-16].view(np.uint32), cg[:int(r["n_cigar"].sum())])
    torch.cuda.synchronize()
    L.gtx_disc_destroy(h)
    row["aligned_bam_bytes"] = [os.path.getsize(p) for p in aligned]
    row["device_front_cut"] = device_front(L, paths, tables, ref, repeats)
    row["device_front_aligned"] = device_front(L, aligned, tables, ref, repeats)
    one = last["files", 1]
    row.update(records=int(len(one["variants"])), text_bytes=len(one["text"]))
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--regions", default="50000,1000000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = {"tool": "tools/discover_files_rate.py", "device_name": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "repeats": args.repeats,
               "read_length": L_READ, "coverage": COVERAGE, "bucket_size": BUCKET,
               "regions": [region(int(r), 7 + i, args.repeats, tmp) for i, r in enumerate(args.regions.split(","))]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
