"""gtx_pipeline_run and gtx_regions_run over reads longer than 160 bases: 2 x 250 pairs on a default context, reads of up to
1 000 bases with gtx_params::max_read_len = 1 000 (batches of different plane pitches, mates and duplicates across them), reads
longer than the context takes, and region runs of both.  Every text is the oracle's."""
import ctypes as C

import numpy as np
import pytest

import bam_writer as bw
import harness
import scenarios
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

RB = 310000
NAMES = ["person0", "person1"]
ERR_UNSUPPORTED = 4  # GTX_ERR_UNSUPPORTED


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


def ragged_case(lengths, n_frags, seed, n_ref=20000, n_samples=2, region_begin=RB, n_rate=0.002, dup_frac=0.15, zone=0):
    """a position-sorted stream of FR pairs (mates of independent lengths), same-strand pairs, unpaired reads, duplicates
    right behind their original and secondary records, read lengths drawn from `lengths`, a few N bases.  zone != 0: a
    fragment starting in the k-th stretch of `zone` bases draws from the k-th of the lists in `lengths` (cyclically).  Returns
    (reference string, records, [codes of read i], STREAM_RECORD array)."""
    rng = np.random.default_rng(seed)
    ref = synth.make_reference(n_ref, seed=seed + 200)
    recs = synth.make_snp_records(ref, 100, seed=seed + 6, region_begin=region_begin)
    haps = []  # haplotype 1 of every sample: the reference with a random half of the SNPs
    for s_ in range(n_samples):
        take = np.random.default_rng(1000 + s_).random(len(recs)) < 0.5
        haps.append(ref.copy())
        for (p, _, alts, _), t in zip(recs, take):
            if t:
                haps[-1][p - region_begin] = "ACGT".index(alts[0])
    rows = []

    def bases(hap, at, n):
        x = hap[at:at + n].copy()
        e = rng.random(n) < 0.005
        x[e] = (x[e] + rng.integers(1, 4, size=int(e.sum()))) % 4
        c = np.array([1, 2, 4, 8], np.uint8)[x]
        c[rng.random(n) < n_rate] = 15
        return c

    for i in range(n_frags):
        sample = int(rng.integers(n_samples))
        hap = haps[sample] if rng.random() < 0.5 else ref
        start = int(rng.integers(0, n_ref - 1700))
        pick = lengths[(start // zone) % len(lengths)] if zone else lengths
        la, lb = int(rng.choice(pick)), int(rng.choice(pick))
        ins = int(rng.integers(max(la, lb) + 10, max(la, lb) + 600))
        a, b = bases(hap, start, la), bases(hap, start + ins - lb, lb)
        mapq = 10 if rng.random() < 0.1 else 60
        kind = rng.random()
        if kind < 0.1:  # same strand: both orientations are aligned
            rows.append((start, a, 1 | 64, ins, mapq, sample, i))
            rows.append((start + ins - lb, b, 1 | 128, -ins, mapq, sample, i))
        elif kind < 0.25:
            rows.append((start, a, 0, 0, mapq, sample, i))
        else:
            rows.append((start, a, 1 | 2 | 32 | 64, ins, mapq, sample, i))
            rows.append((start + ins - lb, b, 1 | 2 | 16 | 128, -ins, mapq, sample, i))
        if rng.random() < (dup_frac if la > 256 else dup_frac / 3):  # an unpaired duplicate right behind its original
            rows.append((start, a, 0, 0, 60, sample, 10_000_000 + i))
        if rng.random() < 0.03:  # dropped by the flag filter (secondary)
            rows.append((start, a, 256, 0, 60, sample, 20_000_000 + i))
    rows.sort(key=lambda r: r[0])
    rec = np.zeros(len(rows), gtx.STREAM_RECORD)
    codes = []
    for k, (p, c, flag, isize, mapq, sample, name) in enumerate(rows):
        codes.append(c)
        rec[k]["flag"], rec[k]["mapq"], rec[k]["score_diff"] = flag, mapq, int(rng.integers(0, 60))
        rec[k]["pos"], rec[k]["isize"], rec[k]["l_qseq"] = p + region_begin, isize, len(c)
        rec[k]["sample"], rec[k]["name_id"] = sample, name
    return synth.bases_to_str(ref), recs, codes, rec


def write_bams(tmp_path, rec, codes, tag="", n_samples=2):
    """one BAM file per sample (a read group each), records in stream order"""
    per = {s: [] for s in range(n_samples)}
    for i in range(len(rec)):
        r = rec[i]
        sd = int(r["score_diff"])
        aux = [("AS", "C", 140), ("XS", "C", 140 - sd)] if sd else [("AS", "C", 100), ("XS", "C", 100)]
        per[int(r["sample"])].append(bw.record("q%d" % int(r["name_id"]), int(r["flag"]), 0, int(r["pos"]), int(r["mapq"]), [("M", len(codes[i]))], 0, 0,
                                               int(r["isize"]), codes[i], aux))
    paths = []
    for s in range(n_samples):
        paths.append(str(tmp_path / ("%sSAMP%d.bam" % (tag, s))))
        bw.write_bam(paths[-1], [("chr7", RB + 200000)], "@HD\tVN:1.6\n@SQ\tSN:chr7\tLN:%d\n@RG\tID:a%d\tSM:person%d\n" % (RB + 200000, s, s), per[s])
    return paths


def stream_chunks(paths, chunk):
    """the merged record stream of the files (gtx_reads, as one pipeline thread reads it) in chunks, with each record's codes"""
    reads = gtx.Reads(paths, region="chr7")
    out = []
    while True:
        srec, sseq = reads.next(chunk, seq_stride=500)
        if len(srec) == 0:
            break
        codes = []
        for i in range(len(srec)):
            L = int(srec["l_qseq"][i])
            nib = sseq[i, :(L + 1) // 2]
            codes.append(np.stack([nib >> 4, nib & 15], axis=1).reshape(-1)[:L])
        out.append((srec, sseq, codes))
    n_rg = reads.n_read_groups
    reads.close()
    return out, n_rg


def pitch_of(srec):
    return max(80, (int(srec["l_qseq"].max()) + 31) // 32 * 16)


def oracle_text(ref, recs, paths):
    """the oracle fed the files' merged stream -> VCF text"""
    chunks, n_rg = stream_chunks(paths, 1 << 16)
    og = Oracle(ref, recs, region_begin=RB).genotyper(2, n_rg)
    for srec, _, codes in chunks:
        og.push(codes, flags=srec["flag"], tid=srec["tid"], mtid=srec["mtid"], pos=srec["pos"], isize=srec["isize"], mapq=srec["mapq"],
                score_diff=srec["score_diff"], name=srec["name_id"], sample=srec["sample"], rg=srec["rg"])
    return og.vcf_records("chr7", NAMES)


def accumulators(ctx, buf, n_samples=2):
    nh, ta = ctx.n_hap, ctx.total_allele
    return (gtx.download(buf.d_gt_cov, np.uint32, n_samples * ta), gtx.download(buf.d_stat_u64, np.uint64, nh + 2 * ta),
            gtx.download(buf.d_stat_u32, np.uint32, nh + 6 * ta))


def text_of(ctx, buf, n_samples=2):
    import torch
    L = gtx.lib()
    d_phred = torch.zeros(max(n_samples * ctx.total_tri, 1), dtype=torch.uint8, device="cuda:0")
    d_calls = torch.zeros(max(n_samples * ctx.n_hap, 1) * gtx.SAMPLE_CALL.itemsize, dtype=torch.uint8, device="cuda:0")
    gtx.check(L.gtx_calls_batch(ctx.h, C.byref(buf), d_phred.data_ptr(), d_calls.data_ptr(), None))
    torch.cuda.synchronize()
    return ctx.vcf_records("chr7", NAMES, *accumulators(ctx, buf, n_samples), d_phred.cpu().numpy()[:n_samples * ctx.total_tri],
                           d_calls.cpu().numpy().view(gtx.SAMPLE_CALL)[:n_samples * ctx.n_hap])


def pipeline(ctx, paths, threads, chunk, slots):
    """gtx_pipeline_run into a fresh block -> (statistics, VCF text, accumulators)"""
    L = gtx.lib()
    buf = gtx.ScoreBuffers()
    gtx.check(L.gtx_scores_alloc(ctx.h, 2, 1 << 16, C.byref(buf), None))
    try:
        st = gtx.pipeline_run(ctx, paths, threads, buf, harness.REC_WORDS, slots, chunk=chunk, region="chr7")
        return st, text_of(ctx, buf), accumulators(ctx, buf)
    finally:
        L.gtx_scores_free(ctx.h, C.byref(buf))


def resident(ctx, paths, plane_stride, conn_cap=1 << 16):
    """the same files through gtx_stream_push (one stream, plane rows of one pitch) -> gtx_align_batch_planes ->
    gtx_score_batch_flags, every read in one batch on the device -> (accumulators, VCF text)"""
    import torch
    L = gtx.lib()
    chunks, n_rg = stream_chunks(paths, 1 << 16)
    st = gtx.Stream(ctx.params, n_rg)
    st.set_planes(plane_stride)
    parts = [st.push(srec, sseq) for srec, sseq, _ in chunks]
    a_seq, a_meta, items = (np.concatenate([p[k] for p in parts]) for k in range(3))
    n, ni = len(a_meta), len(items)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    d_seq, d_meta, d_items = dev(a_seq), dev(a_meta), dev(items)
    d_rec = torch.zeros(n * 2 * harness.REC_WORDS, dtype=torch.int32, device="cuda:0")
    d_fl = torch.zeros(n * 2, dtype=torch.uint8, device="cuda:0")
    buf = gtx.ScoreBuffers()
    gtx.check(L.gtx_scores_alloc(ctx.h, 2, conn_cap, C.byref(buf), None))
    try:
        gtx.check(L.gtx_align_batch_planes(ctx.h, d_seq.data_ptr(), plane_stride, d_meta.data_ptr(), n, d_rec.data_ptr(), harness.REC_WORDS, d_fl.data_ptr(), None))
        gtx.check(L.gtx_score_batch_flags(ctx.h, d_items.data_ptr(), ni, d_rec.data_ptr(), harness.REC_WORDS, d_fl.data_ptr(), C.byref(buf), None))
        torch.cuda.synchronize()
        acc = accumulators(ctx, buf)
        return acc, text_of(ctx, buf)
    finally:
        L.gtx_scores_free(ctx.h, C.byref(buf))


def test_2x250_pairs_on_a_default_context(tmp_path):
    """two samples of 2 x 250 pairs in two BAM files: gtx_pipeline_run (1 and 2 threads, small and large chunks) == the oracle's text"""
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=12000, n_pairs=600, region_begin=RB, read_len=250, n_samples=2)
    paths = write_bams(tmp_path, rec, list(codes))
    want = oracle_text(ref, recs, paths)
    assert want.count(b"\t0/1:") > 0
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0)
    for threads in (1, 2):
        for chunk in (100, 65536):
            st, text, _ = pipeline(ctx, paths, threads, chunk, len(rec))
            assert st["records"] == len(rec) and st["n_threads"] == threads
            assert st["records_failed"] == 0 and st["score_items_refused"] == 0 and st["connections_dropped"] == 0
            assert text == want, (threads, chunk)
    ctx.close()


def crossings(chunks):
    """(duplicates of a read over 256 bases that are the first record of a batch whose pitch is not that of the batch with the
    original, mates in batches of different pitches) in a stream of chunks"""
    pitches = [pitch_of(s) for s, _, _ in chunks]
    where = {}
    dup_across = mate_across = 0
    for k, (srec, _, cds) in enumerate(chunks):
        if k and pitches[k] != pitches[k - 1]:
            p, c = chunks[k - 1][0][-1], chunks[k - 1][2][-1]
            dup_across += int(srec[0]["pos"] == p["pos"] and len(cds[0]) == len(c) > 256 and np.array_equal(cds[0], c) and (p["flag"] & 256) == 0)
        for r in srec:
            if r["flag"] & 1:
                key = (int(r["sample"]), int(r["name_id"]))
                if key in where and pitches[where[key]] != pitches[k]:
                    mate_across += 1
                where[key] = k
    return dup_across, mate_across


def pitch_change_case(tmp_path):
    """reads of 100, 160, 161, 256, 257, 700 and 1 000 bases whose lengths change from one stretch of the region to the next, so
    that the chunks of 100 records one pipeline thread reads are batches of different pitches -- the first seed whose stream has
    a duplicate of a long read and many mates on the far side of a pitch change (found on the host)"""
    for seed in range(3, 60):
        ref, recs, codes, rec = ragged_case([[100, 160], [161, 256], [257, 700], [257, 700, 1000]], 500, seed=seed, zone=1500, dup_frac=0.6)
        paths = write_bams(tmp_path, rec, codes, tag="s%d" % seed)
        chunks, _ = stream_chunks(paths, 100)
        dup_across, mate_across = crossings(chunks)
        if dup_across and mate_across >= 20 and {80, 128, 512} <= {pitch_of(s) for s, _, _ in chunks}:
            return ref, recs, codes, rec, paths
    raise AssertionError("no seed gives the stream this test needs")


def test_reads_of_up_to_1000_bases_in_batches_of_different_pitches(tmp_path):
    """100 .. 1 000 bases with N bases, pairs and unpaired reads on a max_read_len = 1 000 context: chunks of 100 records are
    batches of different plane pitches, with mates and duplicates of long reads on either side of a pitch change.  The text is
    the oracle's; the accumulators are a resident run's"""
    ref, recs, codes, rec, paths = pitch_change_case(tmp_path)
    want = oracle_text(ref, recs, paths)
    assert want.count(b"\t0/1:") > 0
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0, max_read_len=1000)
    acc_resident, text_resident = resident(ctx, paths, 512)
    assert text_resident == want
    for threads, chunk in ((1, 100), (2, 100), (1, 65536)):
        st, text, acc = pipeline(ctx, paths, threads, chunk, len(rec))
        assert st["records"] == len(rec)
        assert st["records_failed"] == 0 and st["score_items_refused"] == 0 and st["connections_dropped"] == 0
        assert text == want, (threads, chunk)
        for a, b in zip(acc, acc_resident):
            assert np.array_equal(a, b), (threads, chunk)
    assert ctx.long_pass_tasks()[0] > 0
    ctx.close()


@pytest.mark.parametrize("max_read_len,too_long", [(0, 300), (1000, 1200)])
def test_a_read_longer_than_the_context_takes_fails_the_run(tmp_path, max_read_len, too_long):
    """one read over the context's max_read_len among 150-base ones: GTX_ERR_UNSUPPORTED naming its length, every thread ends;
    the same context then runs a valid file to the oracle's text"""
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=12000, n_pairs=300, region_begin=RB, read_len=150, n_samples=2)
    codes = list(codes)
    k = len(codes) // 2
    ext = np.array([1, 2, 4, 8], np.uint8)[synth.make_reference(too_long, seed=5)]
    codes[k] = ext
    rec[k]["l_qseq"] = too_long
    rec[k]["flag"] = 0
    bad = write_bams(tmp_path, rec, codes, tag="bad")
    ref2, recs2, codes2, rec2 = scenarios.paired_case("snp100", n_ref=12000, n_pairs=300, region_begin=RB, read_len=150, n_samples=2)
    good = write_bams(tmp_path, rec2, list(codes2), tag="good")
    assert (ref2, recs2) == (ref, recs)
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0, max_read_len=max_read_len)
    for threads, chunk in ((1, 100), (2, 65536)):
        with pytest.raises(gtx.GtxError) as e:
            pipeline(ctx, bad, threads, chunk, len(rec))
        assert e.value.status == ERR_UNSUPPORTED and ("a read of %d bases" % too_long) in str(e.value), str(e.value)
    _, text, _ = pipeline(ctx, good, 2, 100, len(rec2))
    assert text == oracle_text(ref, recs, good)
    ctx.close()


def _region_jobs(torch, cases, plane_stride, params):
    """per region: the stream's plane rows, metadata and items resident on the device, and the oracle's text"""
    keep, jobs, want = [], [], []
    for rb, (ref, recs, codes, rec) in cases:
        seq, _ = harness.pack_ragged(codes)
        st = gtx.Stream(params, 1)
        st.set_planes(plane_stride)
        a_seq, a_meta, items = st.push(rec, seq)
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in (a_seq, a_meta, items)]
        keep.append(dev)
        jobs.append(dict(reference=ref, region_begin=rb, records=recs, d_planes=dev[0].data_ptr(), plane_stride=plane_stride, d_meta=dev[1].data_ptr(),
                         n_reads=len(a_meta), d_items=dev[2].data_ptr(), n_items=len(items)))
        og = Oracle(ref, recs, region_begin=rb).genotyper(2, 1)
        og.push(list(codes), flags=rec["flag"], tid=rec["tid"], mtid=rec["mtid"], pos=rec["pos"], isize=rec["isize"], mapq=rec["mapq"],
                score_diff=rec["score_diff"], name=rec["name_id"], sample=rec["sample"], rg=rec["rg"])
        want.append(og.vcf_records("chr7", NAMES))
    return gtx.RegionJobs(jobs), keep, want


def test_regions_run_with_long_reads():
    """gtx_regions_run over regions of 2 x 250 pairs (default params), then over reads of up to 1 000 bases with
    params.max_read_len = 1 000 (at most two builders then): every region's text is the oracle's"""
    import torch
    cases = [(RB + 40000 * r, scenarios.paired_case("snp100", n_ref=12000, n_pairs=400, seed=r, region_begin=RB + 40000 * r, read_len=250, n_samples=2))
             for r in range(4)]
    cases = [(rb, (ref, recs, list(codes), rec)) for rb, (ref, recs, codes, rec) in cases]
    jobs, keep, want = _region_jobs(torch, cases, 128, gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 0))
    got, st = jobs.run(NAMES, contig="chr7", rec_words=harness.REC_WORDS)
    assert got == want and all(t.count(b"\t0/1:") > 0 for t in want)
    assert st["n_builders"] == 4
    params = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0, 1000)
    cases = [(RB + 40000 * r, ragged_case([150, 250, 400, 1000], 300, seed=10 + r, region_begin=RB + 40000 * r)) for r in range(4)]
    jobs, keep, want = _region_jobs(torch, cases, 512, params)
    for shape in [(0, 0, 0), (1, 1, 1)]:
        got, st = jobs.run(NAMES, contig="chr7", rec_words=harness.REC_WORDS, builders=shape[0], device_threads=shape[1], text_threads=shape[2], params=params)
        assert got == want, shape
        assert jobs.status == [0] * 4 and st["records_failed"] == 0 and st["score_items_refused"] == 0
        assert st["n_builders"] == (2 if shape[0] == 0 else 1)
    del keep
