"""Reads of 257 .. 1 000 bases (gtx_params::max_read_len): the argument checks of contexts and streams, and the long reads'
passes -- tier 1 (HBM tables, reads taken straight from the batch) and tier 2 (the exact pass) -- run from their kernel source
through the host emulation (tests/emu_long) against the oracle.  The same cases on the device: test_gpu_reads_over_256.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth
from oracle_lib import Oracle
from test_emu_parity import check_align, full_arena_case, run_stream

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_ARG, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


@pytest.fixture(scope="session")
def emu_long_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_long") / "libgtx_emu_long.so")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_long"), "-s", "OUT=" + out])
    return out


class LongEmu(harness.EmuBackend):
    """EmuBackend whose align call runs the long reads' passes behind the others (emu_long_align)"""

    def __init__(self, lib_path, graph, **params):
        old = os.environ.get("GTX_EMU_LIB")
        os.environ["GTX_EMU_LIB"] = lib_path
        try:
            super().__init__(graph, **params)
        finally:
            if old is None:
                del os.environ["GTX_EMU_LIB"]
            else:
                os.environ["GTX_EMU_LIB"] = old
        self.tier_tasks = (0,) * 5

    def align(self, seq, meta, rec_words=harness.REC_WORDS):
        seq = np.ascontiguousarray(seq, np.uint8)
        meta = np.ascontiguousarray(meta, gtx.READ_META)
        n = len(meta)
        rec = np.zeros(n * 2 * rec_words, np.uint32)
        tasks = (C.c_uint64 * 5)()
        rc = self.L.emu_long_align(C.c_void_p(self.h), harness._p(seq), C.c_uint32(seq.shape[1]), harness._p(meta), C.c_uint32(n),
                                   harness._p(rec), C.c_uint32(rec_words), tasks)
        assert rc == 0
        self.tier_tasks = tuple(int(x) for x in tasks)
        return rec


def ragged(codes, seed, lo=257, hi=1000):
    rng = np.random.default_rng(seed)
    return [c[:int(L)] for c, L in zip(codes, rng.integers(lo, hi + 1, size=len(codes)))]


# ---- argument checks ----------------------------------------------------------------------------------------------------

def params(max_read_len):
    p = gtx.Params(75, 0, 0, 0, 0, 3840, 0, 0, 0)
    p.max_read_len = max_read_len
    return p


@pytest.mark.parametrize("value,ok", [(0, True), (257, True), (1000, True), (200, False), (256, False), (1001, False)])
def test_max_read_len_argument(value, ok):
    h = C.c_void_p()
    rc = gtx.lib().gtx_stream_create(C.byref(params(value)), 1, C.byref(h))
    assert (rc == 0) == ok and (ok or rc == ERR_ARG)
    if ok:
        gtx.lib().gtx_stream_destroy(h)
    ref, recs, _, _ = scenarios.synthetic_case("snp100", n_ref=4000, n_reads=1, region_begin=1000)
    g = gtx.graph_from_records(ref, recs, region_begin=1000)
    if ok:
        assert gtx.Context(g, device=-1, max_read_len=value).params.max_read_len == value
    else:
        with pytest.raises(gtx.GtxError) as e:
            gtx.Context(g, device=-1, max_read_len=value)
        assert e.value.status == ERR_ARG


def push(stream, lengths):
    n = len(lengths)
    recs = scenarios.stream_records(n, np.arange(n) * 10 + 100, l_qseq=np.asarray(lengths))
    seq = np.zeros((n, 500), np.uint8)
    return stream.push(recs, seq)


def test_stream_push_limit():
    s = gtx.Stream(params(1000))
    a_seq, a_meta, _ = push(s, [300, 1000, 150])
    assert list(a_meta["l_qseq"][:3]) == [300, 1000, 150]
    with pytest.raises(gtx.GtxError) as e:
        push(s, [1001])
    assert e.value.status == ERR_UNSUPPORTED and "1000" in str(e.value)
    # (a context without the passes behind the general one has none for long reads either: refused, not silently kept back)
    p = params(1000)
    p.no_second_pass = 1
    h = C.c_void_p()
    assert gtx.lib().gtx_stream_create(C.byref(p), 1, C.byref(h)) == ERR_ARG
    ref, recs, _, _ = scenarios.synthetic_case("snp100", n_ref=4000, n_reads=1, region_begin=1000)
    with pytest.raises(gtx.GtxError) as e:
        gtx.Context(gtx.graph_from_records(ref, recs, region_begin=1000), device=-1, max_read_len=1000, no_second_pass=True)
    assert e.value.status == ERR_ARG
    s0 = gtx.Stream(params(0))
    push(s0, [256])
    with pytest.raises(gtx.GtxError) as e:
        push(s0, [257])
    assert e.value.status == ERR_UNSUPPORTED and "256" in str(e.value)


# ---- the tiers' kernel source through the host emulation ---------------------------------------------------------------

def long_case(kind, n_reads, seed=0, err=0.005, n_rate=0.001, n_ref=30000, add_all_variants=False, read_len=1000):
    ref, recs, codes, pos = scenarios.synthetic_case(kind, n_ref=n_ref, n_reads=n_reads, region_begin=2000, read_len=read_len, err=err,
                                                     n_rate=n_rate, seed=seed)
    g = gtx.graph_from_records(ref, recs, region_begin=2000, add_all_variants=add_all_variants)
    o = Oracle(ref, recs, region_begin=2000, add_all_variants=add_all_variants)
    return g, o, codes, pos


@pytest.mark.parametrize("kind,aav", [("snp1k", False), ("snp100", False), ("snp25", False), ("indel", False), ("cfg3", True)])
def test_emu_long_reads(emu_long_lib, kind, aav):
    g, o, codes, pos = long_case(kind, 24, seed=7, add_all_variants=aav)
    b = LongEmu(emu_long_lib, g, max_read_len=1000)
    reads = ragged(codes, seed=11)
    # (hints of the long reads are ignored by every pass: check_align's shifted and foreign hints must change nothing)
    check_align(b, o, reads, pos=pos)
    assert b.tier_tasks[0] >= len(reads)


def test_emu_long_reads_with_errors_and_n(emu_long_lib):
    g, o, codes, pos = long_case("snp100", 24, seed=3, err=0.03, n_rate=0.01)
    b = LongEmu(emu_long_lib, g, max_read_len=1000)
    rng = np.random.default_rng(5)
    flags = rng.choice([0, 1 | 64, 1 | 2 | 32 | 64], size=len(codes)).astype(np.uint16)
    check_align(b, o, ragged(codes, seed=13), flags=flags, isize=rng.integers(-2000, 2000, size=len(codes)))


def test_emu_long_mixed_with_short(emu_long_lib):
    """short reads keep the records a default context gives them; a read over max_read_len keeps the overflow status"""
    g, o, codes, pos = long_case("snp100", 16, seed=9)
    reads = [codes[i][:L] for i, L in enumerate([150, 250, 300, 1000] * 4)]
    b = LongEmu(emu_long_lib, g, max_read_len=1000)
    rec, _ = check_align(b, o, reads)
    d = harness.EmuBackend(g)
    short = [i for i, r in enumerate(reads) if len(r) <= 256]
    seq, lens = harness.pack_ragged(reads)
    r0 = d.align(seq, harness.read_meta(lens)).reshape(len(reads), 2, -1)
    r1 = rec.reshape(len(reads), 2, -1)
    assert (r0[short] == r1[short]).all()
    # a 600-base read under max_read_len = 500
    b5 = LongEmu(emu_long_lib, g, max_read_len=500)
    seq, lens = harness.pack_ragged([codes[0][:600], codes[1][:500]])
    r = b5.align(seq, harness.read_meta(lens)).reshape(2, 2, -1)
    assert r[0, 0, 0] >> 16 == gtx.ST_RECORD_OVERFLOW and r[1, 0, 0] >> 16 == 0


def test_emu_long_reads_reach_tier2(emu_long_lib):
    """reads over low-complexity repeats: the chains exceed tier 1's tables and the exact pass finishes them"""
    g, o, codes, pos = long_case("satellite", 10, seed=1, n_ref=20000, read_len=600)
    b = LongEmu(emu_long_lib, g, max_read_len=1000)
    check_align(b, o, ragged(codes, seed=2, lo=300, hi=600))
    assert b.tier_tasks[1] > 0, b.tier_tasks
    assert b.tier_tasks[4] == 0


def test_emu_long_reads_full_arena(emu_long_lib):
    """tier 1's use of the arena task: 300-base reads on snp100 in slots of 16 words, with room in the arena and without"""
    full_arena_case(lambda g, **p: LongEmu(emu_long_lib, g, max_read_len=300, **p), "snp100", read_len=300)
    assert full_arena_case.external == 4


def wide_long_case(n_reads, seed=0, err=0.004):
    """scenarios.wide_site_case's graph -- site A of 100 alleles (99 insertions), site B of more than 2 000 (a deletion and six
    overlapping SNPs merged) -- with reads of 500 .. 1 000 bases over both sites, drawn from haplotypes that carry allele
    numbers of 64 and more at A.  Returns (graph, oracle, codes)."""
    rb = 20000
    ref, recs, _, _, (pA, pB) = scenarios.wide_site_case(region_begin=rb)
    base = np.array(["ACGT".index(c) for c in ref], np.uint8)
    ins = next(r for r in recs if r[0] == pA + rb)[2]
    snp_at = [pB + k for k in (1, 3, 5, 7, 9, 11)]
    alts = {r[0] - rb: r[2] for r in recs if r[0] - rb in snp_at and len(r[2]) == 3}
    rng = np.random.default_rng(seed + 31)

    def haplotype(ins_k, deletion, snp_choice):
        h = [base[:pA + 1], np.array(["ACGT".index(c) for c in ins[ins_k][1:]], np.uint8), base[pA + 1:pB + 1]]
        if not deletion:
            mid = base[pB + 1:pB + 13].copy()
            for q, k in zip(snp_at, snp_choice):
                if k:
                    mid[q - pB - 1] = "ACGT".index(alts[q][k - 1])
            h.append(mid)
        h.append(base[pB + 13:])
        return np.concatenate(h)
    haps = [haplotype(70, False, (3, 3, 2, 0, 1, 0)), haplotype(98, True, None), haplotype(64, False, (0, 0, 0, 0, 3, 3)),
            haplotype(80, False, (1, 2, 3, 3, 3, 2))]
    codes = []
    for i in range(n_reads):
        h = haps[i % len(haps)]
        start = int(rng.integers(pB + 80 - 1000, pA - 20))
        L = int(rng.integers(pB + 80 - start, 1001))
        r = h[start:start + L].copy()
        e = rng.random(len(r)) < err
        r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()))) % 4
        codes.append(synth._CODE_OF_BASE[r])
    o = Oracle(ref, recs, region_begin=rb, add_all_variants=True)
    g = gtx.graph_from_records(ref, recs, region_begin=rb, add_all_variants=True)
    assert np.sort(g["ref_nvar"])[-1] > 1000
    return g, o, codes


def test_emu_long_reads_wide_sites(emu_long_lib):
    """sites of more than 64 alleles: tier 1 hands the tasks that meet an allele number >= 64 to the wide build of tier 2"""
    g, o, codes = wide_long_case(8)
    b = LongEmu(emu_long_lib, g, max_read_len=1000)
    rec, _ = check_align(b, o, codes)
    assert b.tier_tasks[1] > 0 and b.tier_tasks[4] == 0, b.tier_tasks
    heads = rec.reshape(-1, harness.REC_WORDS)[0::2]
    assert ((heads[:, 1] & gtx.REC_WIDE) != 0).any()


def test_emu_long_pairs_stream_scores_calls_vcf(emu_long_lib):
    """2 x 300 pairs over three samples: stream -> align -> score -> calls -> VCF text == the oracle's (pair selection, the
    clipped-bases and mismatch statistics of reads longer than 256 bases)"""
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=20000, n_pairs=120, region_begin=310000, read_len=300, n_samples=3)
    o = Oracle(ref, recs, region_begin=310000)
    b = LongEmu(emu_long_lib, gtx.graph_from_records(ref, recs, region_begin=310000), max_read_len=1000)
    want = run_stream(b, o, codes, rec, n_samples=3)
    assert want.sum() > 0 and b.tier_tasks[0] > 0
