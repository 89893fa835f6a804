"""Pins the inputs and the oracle's results of the five extra legs of `bench.py --full` (cfg3, clusters, long reads, repeats,
genome-like) into leg_digests.json.  Runs on the host, no GPU:
    python tests/golden/make_leg_digests.py            # writes leg_digests.json
    python tests/golden/make_leg_digests.py --check    # recomputes every entry and compares it with the committed file

Each leg's inputs are RESTATED here from the same synth calls and seeds as bench.py's extra_cfg3 / extra_long_reads /
extra_repeats / extra_genome_like (extra_workload: read set seed 5, position-sorted with a stable sort, samples drawn with
default_rng(3) on the 30-sample legs).  tests/test_gpu_legs_vs_oracle.py captures the inputs bench.py itself hands its
Workload and compares their digest with the pinned one, so that a change of bench.py, synth or this file shows up as a
named failure instead of a silent change of what the leg tests check.  Every read then goes through the CPU oracle
(oracle_lib.sharded_genotyper, mapq 60, the position hints as bench.py gives them, wrong ones included), and the digests of
its VCF records text and of its final (no_variant_overlapping) text are pinned."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from graphtyper_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "leg_digests.json")
REGION_BEGIN = 1000000
REGION_LEN = 1000000
N_READS = 2_000_000   # bench.py --extra-reads (default)
READS_SEED = 5        # extra_workload: make_reads(5) is read set 0
SAMPLES_SEED = 3      # extra_workload: np.random.default_rng(3) draws the reads' samples
LEGS = ("cfg3", "clusters", "long_reads", "repeats", "genome_like")


def sample_names(n_samples):
    return ["SAMP%04d" % i for i in range(n_samples)]


def leg_inputs(leg, n=N_READS):
    """the graph and the read set 0 of one leg, as bench.py makes them: dict(ref_str, records, add_all, n_samples, read_len,
    codes [n, read_len] uint8 BAM codes, pos [n] int64 hints, samples [n] uint32 or None), sorted by position"""
    ref = synth.make_reference(REGION_LEN, seed=42)  # bench.cfg2_graph_inputs
    read_len, n_samples, add_all = 150, 1, False
    if leg == "cfg3":
        recs = synth.make_cfg3_records(ref, 100, seed=17, region_begin=REGION_BEGIN)
        n_samples, add_all = 30, True
    elif leg == "clusters":
        recs = synth.make_cluster_records(ref, 150, seed=8, region_begin=REGION_BEGIN)
        n_samples, add_all = 30, True
    elif leg == "long_reads":
        recs = synth.make_snp_records(ref, 1000, seed=7, region_begin=REGION_BEGIN)
        read_len = 250
    elif leg == "repeats":
        ref = ref.copy()
        synth.plant_repeats(ref, seed=21)
        recs = synth.make_snp_records(ref, 1000, seed=7, region_begin=REGION_BEGIN)
    elif leg == "genome_like":
        ref, _ = synth.make_genome_like_reference(REGION_LEN, seed=1999)
        recs = synth.make_snp_records(ref, 1000, seed=7, region_begin=REGION_BEGIN)
    else:
        raise ValueError(leg)
    if leg == "genome_like":
        codes, pos, _ = synth.make_mapped_reads(ref, recs, n, seed=READS_SEED, region_begin=REGION_BEGIN)
    else:
        codes, pos = synth.make_reads(ref, recs, n, read_len=read_len, seed=READS_SEED, region_begin=REGION_BEGIN)
    order = np.argsort(pos, kind="stable")
    codes, pos = np.ascontiguousarray(codes[order], np.uint8), np.ascontiguousarray(pos[order], np.int64)
    samples = np.random.default_rng(SAMPLES_SEED).integers(0, n_samples, size=n).astype(np.uint32) if n_samples > 1 else None
    return dict(ref_str=synth.bases_to_str(ref), records=recs, add_all=add_all, n_samples=n_samples, read_len=read_len,
                codes=codes, pos=pos, samples=samples)


def input_digest(codes, pos, samples):
    """SHA-256 of the sorted reads: their BAM codes (uint8 rows), then their hints (int64), then their samples (uint32, if any)"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(codes, np.uint8).tobytes())
    h.update(np.ascontiguousarray(pos, np.int64).tobytes())
    if samples is not None:
        h.update(np.ascontiguousarray(samples, np.uint32).tobytes())
    return h.hexdigest()


def text_digest(text):
    """sha256, bytes and records (the column line comes first) of a VCF records text"""
    return {"sha256": hashlib.sha256(text).hexdigest(), "bytes": len(text), "records": text.count(b"\n") - 1}


def oracle_texts(inp, threads=None):
    """every read through the oracle: (genotyper, VCF records text, final text with no_variant_overlapping, threads)"""
    from oracle_lib import Oracle, sharded_genotyper
    n = len(inp["pos"])
    oracle = Oracle(inp["ref_str"], inp["records"], region_begin=REGION_BEGIN, add_all_variants=inp["add_all"])
    og, used = sharded_genotyper(oracle, inp["codes"], inp["pos"], n_samples=inp["n_samples"],
                                 samples=None if inp["samples"] is None else inp["samples"].astype(np.int32),
                                 threads=threads, mapq=np.full(n, 60, np.uint8))
    assert og.counts()["records"] == n, og.counts()
    names = sample_names(inp["n_samples"])
    text = og.vcf_records("chr20", names)
    final = og.vcf_records_final("chr20", names, inp["ref_str"], REGION_BEGIN + 1, no_variant_overlapping=True)
    return og, text, final, used


def entry(leg, n=N_READS, threads=None):
    t0 = time.perf_counter()
    inp = leg_inputs(leg, n)
    t_in = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, text, final, used = oracle_texts(inp, threads)
    t_or = time.perf_counter() - t0
    sys.stderr.write("%-12s inputs %.1f s, oracle %.1f s on %d threads\n" % (leg, t_in, t_or, used))
    return {"reads": n, "reads_seed": READS_SEED, "samples_seed": SAMPLES_SEED if inp["n_samples"] > 1 else None,
            "n_samples": inp["n_samples"], "read_len": inp["read_len"],
            "inputs_sha256": input_digest(inp["codes"], inp["pos"], inp["samples"]),
            "vcf": text_digest(text), "final_vcf": text_digest(final)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed file instead of writing it")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args(argv)
    legs = [x for x in args.legs.split(",") if x]
    got = {leg: entry(leg, threads=args.threads or None) for leg in legs}
    if args.check:
        pin = json.load(open(OUT))["legs"]
        bad = [leg for leg in legs if pin.get(leg) != got[leg]]
        for leg in bad:
            sys.stderr.write("%s: pinned %s\n%s  computed %s\n" % (leg, json.dumps(pin.get(leg)), " " * len(leg), json.dumps(got[leg])))
        print("leg digests: %d of %d legs as pinned" % (len(legs) - len(bad), len(legs)))
        return 1 if bad else 0
    assert legs == list(LEGS), "the file pins every leg"
    doc = {"what": "inputs and oracle results of the extra legs of bench.py --full (read set 0 at --read-sets 1, %d reads each): "
                   "inputs_sha256 = SHA-256 of the position-sorted reads' BAM codes, int64 hints and uint32 samples; vcf / final_vcf = "
                   "the oracle's VCF records text (column line first) and its final text (vcf_records_final, no_variant_overlapping) "
                   "over every read" % N_READS,
           "made_by": "tests/golden/make_leg_digests.py", "checked_by": "tests/test_gpu_legs_vs_oracle.py",
           "legs": got}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=2, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
