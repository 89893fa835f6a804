"""The extra legs of `bench.py --full` (cfg3, clusters, 2 x 250 reads, repeats, genome-like) at their own size, every read
against the CPU oracle.

Each leg is driven through bench.py's own leg function, so that its graph, reads and schedule are the benchmark's: a thin
proxy of graphtyper_amd.lib records the graph_from_records call, and bench.Workload is swapped for a subclass that records
the read set add_reads receives (position-sorted BAM nibble rows and hints, the samples of __init__) and, in close(), while
the context is still open, downloads the last step's accumulators, PL and SampleCalls of EVERY lane and turns them into the
oracle's canonical score and call streams and the VCF records / final texts.  With --read-sets 1 every lane's last step
has worked on the same reads.

Per leg: all reads through oracle_lib.sharded_genotyper (hints as bench gives them, wrong ones included; samples; mapq 60);
lane 0 equals the oracle word for word and byte for byte; every other lane equals lane 0; no record of any lane carries an
overflow status (the repeats and genome-like legs keep six steps in flight in one big-record arena that is never rewound);
the leg did real work.  The captured inputs and the oracle's texts are compared with tests/golden/leg_digests.json
(tests/golden/make_leg_digests.py restates the inputs on the host), unless GTX_LEG_READS overrides the read count
(debugging on a small box).

The last test sends a burst of exact-pass tasks to the light build of that pass (the launch sized behind batches that sent
it nothing) and checks every record against the oracle."""
import importlib.util
import os
import time

import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth
from oracle_lib import Oracle, sharded_genotyper

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_leg_digests", os.path.join(HERE, "golden", "make_leg_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

N_READS = int(os.environ.get("GTX_LEG_READS", "0")) or None
N_BURST = 8000  # reads inside the satellite case's homopolymer (test_exact_pass_burst_behind_batches_that_had_none)
PINS = None


def _pins():
    global PINS
    if PINS is None:
        import json
        PINS = json.load(open(digests.OUT))["legs"]
    return PINS


class _GtxProxy:
    """graphtyper_amd.lib as the leg functions see it: records what graph_from_records builds, delegates the rest"""

    def __init__(self):
        self.graphs = []

    def graph_from_records(self, reference, records, region_begin=0, add_all_variants=False, **kw):
        assert not kw, kw
        self.graphs.append((reference, list(records), region_begin, add_all_variants))
        return gtx.graph_from_records(reference, records, region_begin=region_begin, add_all_variants=add_all_variants)

    def __getattr__(self, name):
        return getattr(gtx, name)


def _lane_results(w, ln, bench):
    """what lane `ln` of Workload `w` holds after its last step, on the host and in the oracle's canonical forms"""
    torch, ctx = w.torch, w.ctx
    torch.cuda.synchronize()
    n, ns = w.n, w.n_samples
    nh, ta, tt = ctx.n_hap, ctx.total_allele, ctx.total_tri
    buf = ln["buf"]
    # records: no overflow status anywhere (the dense array holds the headers of the position-hinted pass' records)
    head = ln["d_rec"].view(n * 2, bench.REC_WORDS)[:, 0].clone()
    if ln["d_compact"] is not None:
        is_compact = (ln["d_flags"][0::2] & gtx.TASK_COMPACT) != 0
        head[0::2] = torch.where(is_compact, ln["d_compact"].view(n, gtx.COMPACT_WORDS)[:, 0], head[0::2])
    errors = int((((head >> 16) & gtx.ST_ERROR_MASK) != 0).sum().item())
    calls = ln["d_calls"].cpu().numpy().view(gtx.SAMPLE_CALL)[:ns * nh].copy()
    phred = ln["d_phred"].cpu().numpy()[:ns * tt].copy()
    acc = harness.Accumulators(ctx, ns, conn_cap=1)
    acc.log_score = gtx.download(buf.d_log_score, np.uint32, ns * tt)
    acc.gt_cov = gtx.download(buf.d_gt_cov, np.uint32, ns * ta)
    acc.hap_u32 = gtx.download(buf.d_hap_u32, np.uint32, ns * nh * 4)
    acc.stat_u64 = gtx.download(buf.d_stat_u64, np.uint64, nh + 2 * ta)
    acc.stat_u32 = gtx.download(buf.d_stat_u32, np.uint32, nh + 6 * ta)
    acc.conn_count = gtx.download(buf.d_conn_count, np.uint32, 2)
    acc.conn_log = gtx.download(buf.d_conn_log, np.uint32, 6 * int(acc.conn_count[0])) if acc.conn_count[0] else np.zeros(6, np.uint32)
    acc.conn_near = gtx.download(buf.d_conn_near, np.uint32, ns * ctx.total_near) if ctx.total_near else np.zeros(0, np.uint32)
    names = w.sample_names()
    text = ctx.vcf_records("chr20", names, acc.gt_cov.copy(), acc.stat_u64, acc.stat_u32, phred, calls)
    final = ctx.vcf_records_final("chr20", names, acc.gt_cov.copy(), acc.stat_u64, acc.stat_u32, phred, calls, no_variant_overlapping=True)
    return dict(errors=errors, scores=harness.canonical_scores(ctx, acc), calls=harness.canonical_calls(ctx, phred, calls, ns),
                text=text, final=final, nonref=int((calls["gt_second"] > 0).sum()))


def _capturing_workload(bench, seen):
    class CapturingWorkload(bench.Workload):
        def __init__(self, torch, gtx_, ctx, device, d_seq, d_pos, n_samples, samples=None, **kw):
            seen.update(n_samples=n_samples, samples=None if samples is None else np.asarray(samples, np.uint32).copy(),
                        read_len=kw.get("read_len", bench.READ_LEN), read_sets=[])
            super().__init__(torch, gtx_, ctx, device, d_seq, d_pos, n_samples, samples=samples, **kw)

        def add_reads(self, d_seq, d_pos):
            seen["read_sets"].append((bench.unpack_nibbles(d_seq.cpu().numpy(), seen["read_len"]), d_pos.cpu().numpy().astype(np.int64)))
            super().add_reads(d_seq, d_pos)

        def close(self):
            ctx = self.ctx
            seen["hap_order"], seen["n_hap"] = np.asarray(ctx.hap_order).copy(), int(ctx.n_hap)
            seen["hap_cnum"] = np.asarray(ctx.hap_cnum).copy()
            seen["lanes"] = [_lane_results(self, ln, bench) for ln in self.lanes]
            super().close()

    return CapturingWorkload


def _site_of_word(hap_cnum, stream, word, n_samples, kind):
    """the site (haplotype index) whose part of a canonical stream (harness.canonical_scores / canonical_calls layout) holds
    `word`, and the word's offset inside that part; walked over the oracle's stream, whose prefix up to `word` both share"""
    i = 0
    for h, cnum in enumerate(int(x) for x in hap_cnum):
        start = i
        tri = cnum * (cnum + 1) // 2
        if kind == "calls":
            i += n_samples * (8 + tri)
        else:
            i += 5 + cnum * 10
            for _s in range(n_samples):
                i += 4 + cnum + tri
                for _a in range(cnum):
                    k = int(stream[i])
                    i += 1
                    for _c in range(k):
                        i += 1 + int(hap_cnum[int(stream[i])])
        if word < i:
            return h, word - start
    return len(hap_cnum), word - i


def _first_line(got, want):
    gl, wl = got.split(b"\n"), want.split(b"\n")
    for k in range(min(len(gl), len(wl))):
        if gl[k] != wl[k]:
            return "line %d (%d vs %d lines):\n  got  %r\n  want %r" % (k, len(gl), len(wl), gl[k][:300], wl[k][:300])
    return "%d vs %d lines" % (len(gl), len(wl))


def _compare(leg, what, seen, got, want, kind, n_samples):
    if kind in ("scores", "calls"):
        if len(got) == len(want) and np.array_equal(got, want):
            return
        m = min(len(got), len(want))
        bad = np.nonzero(got[:m] != want[:m])[0]
        word = int(bad[0]) if len(bad) else m
        h, off = _site_of_word(seen["hap_cnum"], want, word, n_samples, kind)
        where = "site %d (pos %d), word %d of the site" % (h, int(seen["hap_order"][h]), off) if h < len(seen["hap_order"]) else "past the last site"
        raise AssertionError("%s: %s %s differ (%d vs %d words, %d differ) -- first at word %d: %s: got %d, want %d" %
                             (leg, what, kind, len(got), len(want), len(bad), word, where,
                              int(got[word]) if word < len(got) else -1, int(want[word]) if word < len(want) else -1))
    if got != want:
        raise AssertionError("%s: %s %s differs, first at %s" % (leg, what, kind, _first_line(got, want)))


def _run_leg(bench, leg, args, torch, proxy, device, ref):
    if leg in ("cfg3", "clusters"):
        return bench.extra_cfg3(args, torch, proxy, synth, device, ref, leg)
    if leg == "long_reads":
        return bench.extra_long_reads(args, torch, proxy, synth, device, ref)
    if leg == "repeats":
        return bench.extra_repeats(args, torch, proxy, synth, device, ref)
    return bench.extra_genome_like(args, torch, proxy, synth, device)


@pytest.mark.parametrize("leg", digests.LEGS)
def test_leg_every_read_against_the_oracle(leg, monkeypatch):
    import torch
    import bench
    t_start = time.perf_counter()
    assert torch.cuda.is_available() and os.path.exists(gtx.LIB_PATH)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    argv = ["--read-sets", "1", "--no-cpu-baseline"] + (["--extra-reads", str(N_READS)] if N_READS else [])
    args = bench.parse_args(argv)
    n = args.extra_reads
    ref = bench.cfg2_graph_inputs(synth)[0]
    seen = {}
    monkeypatch.setattr(bench, "Workload", _capturing_workload(bench, seen))
    proxy = _GtxProxy()
    out = _run_leg(bench, leg, args, torch, proxy, device, ref)
    t_leg = time.perf_counter() - t_start

    # ---- what bench handed its Workload
    assert len(proxy.graphs) == 1 and len(seen["read_sets"]) == 1, (len(proxy.graphs), len(seen.get("read_sets", ())))
    ref_str, records, region_begin, add_all = proxy.graphs[0]
    codes, pos = seen["read_sets"][0]
    samples, n_samples = seen["samples"], seen["n_samples"]
    assert codes.shape == (n, seen["read_len"]) and np.all(np.diff(pos) >= 0)
    pin = _pins()[leg]
    pinned = n == pin["reads"]
    if pinned:
        assert digests.input_digest(codes, pos, samples) == pin["inputs_sha256"], \
            "%s: the inputs bench.py hands its Workload are not the pinned ones (tests/golden/make_leg_digests.py restates them)" % leg

    # ---- every read through the oracle
    t0 = time.perf_counter()
    oracle = Oracle(ref_str, records, region_begin=region_begin, add_all_variants=add_all)
    og, threads = sharded_genotyper(oracle, codes, pos, n_samples=n_samples, samples=None if samples is None else samples.astype(np.int32),
                                    mapq=np.full(n, 60, np.uint8))
    assert og.counts()["records"] == n
    names = ["SAMP%04d" % i for i in range(n_samples)]
    want_scores, want_calls = og.scores(), og.calls()
    want_text = og.vcf_records("chr20", names)
    want_final = og.vcf_records_final("chr20", names, ref_str, region_begin + 1, no_variant_overlapping=True)
    t_oracle = time.perf_counter() - t0
    if pinned:
        for key, text in (("vcf", want_text), ("final_vcf", want_final)):
            assert digests.text_digest(text) == pin[key], "%s: the oracle's %s text is not the pinned one" % (leg, key)

    # ---- lane 0 against the oracle, every other lane against lane 0
    lanes = seen["lanes"]
    first = lanes[0]
    _compare(leg, "lane 0 vs oracle:", seen, first["scores"], want_scores, "scores", n_samples)
    _compare(leg, "lane 0 vs oracle:", seen, first["calls"], want_calls, "calls", n_samples)
    _compare(leg, "lane 0 vs oracle:", seen, first["text"], want_text, "VCF records", n_samples)
    _compare(leg, "lane 0 vs oracle:", seen, first["final"], want_final, "final VCF records", n_samples)
    for k, ln in enumerate(lanes):
        assert ln["errors"] == 0, "%s: lane %d: %d records carry an overflow status" % (leg, k, ln["errors"])
        if k:
            for kind in ("scores", "calls"):
                _compare(leg, "lane %d vs lane 0:" % k, seen, ln[kind], first[kind], kind, n_samples)
            _compare(leg, "lane %d vs lane 0:" % k, seen, ln["text"], first["text"], "VCF records", n_samples)
            _compare(leg, "lane %d vs lane 0:" % k, seen, ln["final"], first["final"], "final VCF records", n_samples)

    # ---- not vacuous
    records_out = want_text.count(b"\n") - 1
    assert records_out >= 0.9 * seen["n_hap"], (leg, records_out, seen["n_hap"])
    assert want_final.count(b"\n") - 1 > 0.2 * seen["n_hap"], leg
    if pinned:
        assert first["nonref"] > seen["n_hap"] * n_samples // 8, (leg, first["nonref"], seen["n_hap"])
    if leg in ("cfg3", "clusters", "genome_like"):
        assert out["pass_shares"]["handed_to_general"] > 0, (leg, out["pass_shares"])
    if leg == "repeats":
        assert out["exact_pass"]["tasks_with_a_small_part_of_the_slab"] > 0 and out["exact_pass"]["tasks_refused"] == 0, out["exact_pass"]
    print("%s: %d reads, %d lanes, %s; leg %.1f s, oracle %.1f s on %d threads, test %.1f s; %d records, %d non-reference calls" %
          (leg, n, len(lanes), out["schedule"], t_leg, t_oracle, threads, time.perf_counter() - t_start, records_out, first["nonref"]))


def test_exact_pass_burst_behind_batches_that_had_none():
    """More than a thousand exact-pass tasks in the first batch behind two batches that sent the pass nothing, on a fresh
    context: the light build of the pass (gtx_align_exact_light_kernel) does them all, every record is the oracle's, none is
    refused -- and the same batch again, now on the full build, gives the same words.  The batch: the reads of
    scenarios.synthetic_case("satellite") plus N_BURST reads inside its 280-bp homopolymer, the one of its repeats whose reads
    reach the exact pass (a fifth of them; the others' chains fit the general and HBM-table passes)."""
    region_begin = 30000
    ref_str, recs, codes, pos = scenarios.synthetic_case("satellite", n_ref=16000, n_reads=1500, seed=6, region_begin=region_begin)
    ref = np.array(["ACGT".index(c) for c in ref_str], np.uint8)
    inside, ipos = synth.make_reads(ref[2000:2280], [r for r in recs if 2000 < r[0] - region_begin < 2278], N_BURST, read_len=150, seed=13,
                                    region_begin=region_begin + 2000)
    codes, pos = np.concatenate([codes, inside]), np.concatenate([pos, ipos])
    order = np.argsort(pos, kind="stable")
    codes, pos = np.ascontiguousarray(codes[order]), pos[order]
    o = Oracle(ref_str, recs, region_begin=region_begin)
    # (the records of reads in the homopolymer are long: 6 M words of the big-record arena per call of this batch)
    b = harness.GpuBackend(gtx.graph_from_records(ref_str, recs, region_begin=region_begin), big_record_words=1 << 24)
    # easy reads: the stretch between the homopolymer (2000-2280) and the first dinucleotide repeat (5000-5270)
    easy, epos = synth.make_reads(ref[2700:4600], [r for r in recs if 2700 < r[0] - region_begin < 4598], 2000, read_len=150, seed=11,
                                  region_begin=region_begin + 2700)
    eseq, elens = harness.pack_ragged(list(easy))
    for _ in range(2):
        b.align(eseq, harness.read_meta(elens, pos=epos))
        assert b.exact_pass_tasks()[0] == 0
    hseq, hlens = harness.pack_ragged(list(codes))
    hmeta = harness.read_meta(hlens, pos=pos)
    t0 = time.perf_counter()
    first = b.align(hseq, hmeta).copy()
    print("exact-pass burst: %d reads in %.1f ms (light build)" % (len(codes), 1e3 * (time.perf_counter() - t0)))
    tasks = b.exact_pass_tasks()
    assert tasks[0] >= 1000 and tasks[3] == 0, tasks
    big, _ = b.big_records()
    got = gtx.parse_records(first, len(codes), harness.REC_WORDS, b.ctx.hap_order, big)
    want = o.align(list(codes))
    for i, (a, w) in enumerate(zip(got, want)):
        for k in range(2):
            assert a[k]["status"] == 0, "read %d orientation %d: status %d" % (i, k, a[k]["status"])
            ga = dict(longest=a[k]["longest"], paths=a[k]["paths"])
            assert ga == w[k], "read %d orientation %d: kernel %r != oracle %r" % (i, k, ga, w[k])
    # the same batch on the full build: the same words (a record in the big-record arena keeps an offset there that differs
    # from call to call: such records compare by their header words and their parsed contents)
    again = b.align(hseq, hmeta).copy()
    assert b.exact_pass_tasks()[3] == 0
    a1, a2 = first.reshape(2 * len(codes), -1), again.reshape(2 * len(codes), -1)
    external = ((a1[:, 0] >> 16) & gtx.ST_EXTERNAL) != 0
    differ = a1 != a2
    differ[external, 2:] = False
    assert not differ.any(), "records of the light and the full build differ (reads %s)" % (np.nonzero(differ.any(1))[0][:5] // 2)
    big, _ = b.big_records()
    assert gtx.parse_records(again, len(codes), harness.REC_WORDS, b.ctx.hap_order, big) == got
    print("exact-pass burst: %d tasks through the exact pass, %d records in the arena" % (tasks[0], int(external.sum())))
