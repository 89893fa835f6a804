"""The read shapes the position-hinted pass (hinted.hpp) proves since the general pass' share of a cfg2 step was halved:

  A  a k-mer with two or three ambiguous bases that none of hint_kmer_judge's older rules settles.  It is decided once per read
     in hinted_on_path: one half H of the k-mer holds no substitution and at most one ambiguous base; with one, HINT_NEAR_FREE
     has to say that no 16-mer a substitution away from the reference's half is indexed, and no SNP may lie in H (the flag
     speaks of the reference k-mer's halves only, and it is clear wherever a SNP's other allele puts such a 16-mer into the
     index: under a k-mer over a SNP only the cases with a half free of ambiguous bases are proven, whichever allele the read
     carries); the flag of H (HINT_L1 / R1, or the SNP's group) has to say that the judged key alone has H.
  B  a run of k-mers that two parallel chains open behind a label-less k-mer (the walk at the read's start succeeds for both:
     the reference returns the path twice) and one of whose k-mers names ANOTHER allele of its SNP.

Hand-made reads on a reference of 6 kb with a SNP every 1 kb, one read per k-mer position and sub-case, each beside twins that
must stay declined -- with the decline note of their site (tools/decline_notes.py names them): a second SNP 10 bases from the
first (the half is shared with that allele's key), substitutions in both halves, two ambiguous bases in the half without a
substitution, a SNP inside the half HINT_NEAR_FREE is asked about, a substitution or an allele set in the run of twin chains.
Reads of 150 bases have four k-mers (positions 0..3); the fifth k-mer position is looked at with reads of 157 bases.
Every record is held to the oracle (with right, missing, shifted and foreign hints: test_emu_parity.check_align), on the host
emulation for both builds of the pass, and through the C ABI on the device.

Then the bars on the emulation: a random sweep with 2 % N and 3 % substitutions against the oracle, and the share of the
general pass on a cfg2-like sample, which has to be at most half of what it was (761 of 1.2 M reads before these shapes)."""
import ctypes as C

import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from graphtyper_amd import synth
from oracle_lib import Oracle
from test_emu_parity import check_align

RB = 1000000          # region begin
N_REF = 6000
SNP_AT = 2500         # the SNP the reads are laid over (sites at 500, 1500, ...)
CODE = np.array([1, 2, 4, 8], np.uint8)
DONE = 0              # expected: finished by pass 0; any other number: declined with that note
NOTE_SEVERAL, NOTE_TWIN = 72, 107
LEFT_AMB, RIGHT_AMB = (3, 7, 11), (18, 23, 27)  # offsets in the k-mer of its ambiguous bases
LEFT_SUB, RIGHT_SUB, SNP_OFF = 5, 25, 20        # ... of its substitutions, of the SNP (in the last 16 bases)

# shape A: ambiguous bases in the first / last 16 bases of the k-mer, substitutions there; expected without a SNP under the
# k-mer / with one in the last 16 bases (reference allele, then the other allele)
SHAPE_A = [
    # (the older rules: two in one half, one in each)
    ("2+0", 2, 0, 0, 0, DONE, DONE),
    ("1+1", 1, 1, 0, 0, DONE, DONE),
    ("2+0, substitution in the clean half", 2, 0, 0, 1, DONE, DONE),
    # no substitution: all in one half, or one half holds exactly one
    ("3+0", 3, 0, 0, 0, DONE, DONE),
    ("0+3", 0, 3, 0, 0, DONE, DONE),
    ("2+1", 2, 1, 0, 0, DONE, NOTE_SEVERAL),   # (with the SNP: HINT_NEAR_FREE is not asked about a half with a SNP ...
    ("1+2", 1, 2, 0, 0, DONE, NOTE_SEVERAL),   #  ... and is clear at a place whose k-mer lies over one)
    # substitutions in one half, the other half holds no ambiguous base
    ("2+0, substitution beside them", 2, 0, 1, 0, DONE, DONE),
    ("0+2, substitution beside them", 0, 2, 0, 1, DONE, DONE),
    ("3+0, substitution beside them", 3, 0, 1, 0, DONE, DONE),
    # ... the other half holds exactly one
    ("1+1, substitution in the first half", 1, 1, 1, 0, DONE, NOTE_SEVERAL),
    ("1+1, substitution in the last half", 1, 1, 0, 1, DONE, NOTE_SEVERAL),
    ("2+1, substitution beside the two", 2, 1, 1, 0, DONE, NOTE_SEVERAL),
    # twins: the half without a substitution holds two; substitutions in both halves
    ("2+1, substitution beside the one", 2, 1, 0, 1, NOTE_SEVERAL, NOTE_SEVERAL),
    ("1+1, substitutions in both halves", 1, 1, 1, 1, NOTE_SEVERAL, NOTE_SEVERAL),
    ("2+1, substitutions in both halves", 2, 1, 1, 1, NOTE_SEVERAL, NOTE_SEVERAL),
]


def _graphs():
    ref = synth.make_reference(N_REF, seed=5)
    recs = synth.make_snp_records(ref, 1000, seed=6, region_begin=RB, first=500)
    alt = {p - RB: "ACGT".index(a[0]) for p, _, a, _ in recs}
    # the same sites and a second SNP 10 bases behind the one the reads are laid over
    q = SNP_AT + 10
    pair = sorted(recs + [(q + RB, "ACGT"[ref[q]], ["ACGT"[(ref[q] + 2) % 4]], None)])
    return ref, recs, pair, alt


def _read(ref, start, length, alt_base=None):
    codes = CODE[ref[start:start + length]].copy()
    if alt_base is not None:
        codes[SNP_AT - start] = CODE[alt_base]
    return codes


def _ambiguous(codes, at, kind, ref_code):
    others = [c for c in (1, 2, 4, 8) if c != ref_code]
    codes[at] = 15 if kind == "N" else (ref_code | others[0]) if kind == "with" else (others[0] | others[1])


def _substitute(codes, at):
    codes[at] = CODE[(int(np.log2(codes[at])) + 1) % 4]


def _make_reads():
    """(graph, name, codes, position, expected) for every case"""
    ref, recs, pair, alt = _graphs()
    out = []
    for i in range(5):
        length = 150 if i < 4 else 157
        a0 = 31 * i
        for name, al, ar, sl, sr, want_plain, want_snp in SHAPE_A:
            for mode in ("no SNP", "reference allele", "other allele"):
                start = 1600 + 7 * i if mode == "no SNP" else SNP_AT - (a0 + SNP_OFF)
                kinds = ["N"] if (al + ar < 3 or sl + sr) else ["N", "with", "without"]  # (sets that hold / miss the reference base: label / no label)
                for kind in kinds:
                    codes = _read(ref, start, length, alt[SNP_AT] if mode == "other allele" else None)
                    for k, off in enumerate(LEFT_AMB[:al] + RIGHT_AMB[:ar]):
                        _ambiguous(codes, a0 + off, kind if k == 0 else "N", int(CODE[ref[start + a0 + off]]))
                    if sl:
                        _substitute(codes, a0 + LEFT_SUB)
                    if sr:
                        _substitute(codes, a0 + RIGHT_SUB)
                    out.append(("snps", "A k-mer %d, %s, %s, %s" % (i, name, mode, kind), codes, start, want_plain if mode == "no SNP" else want_snp))
        # twin: a second SNP 10 bases from the first, both in the first half of the k-mer -- the key of either one's other allele
        # shares the last 16 bases: the half is not the reference key's alone
        start = SNP_AT - (a0 + 4)
        for name, sl in (("3+0", 0), ("3+0, substitution beside them", 1)):
            codes = _read(ref, start, length)
            for off in LEFT_AMB:
                codes[a0 + off] = 15
            if sl:
                _substitute(codes, a0 + LEFT_SUB)
            out.append(("pair", "A k-mer %d, %s, two SNPs in the half" % (i, name), codes, start, NOTE_SEVERAL))
    # shape B: k-mers 0 .. lo - 1 have no label (an N and a substitution in their first half: one mismatch for the walk at the read's
    # start), k-mer lo lies over the SNP and opens the run with two parallel chains
    for lo in range(1, 5):
        length = 150 if lo < 4 else 157
        for off in (5, 20):
            start = SNP_AT - (31 * lo + off)
            for name, allele, extra, want in (("reference allele", None, None, DONE), ("other allele", alt[SNP_AT], None, DONE),
                                              ("other allele and a substitution in the next k-mer", alt[SNP_AT], "substitution", NOTE_TWIN),
                                              ("both alleles' code on the site", None, "set", NOTE_TWIN)):
                if extra == "substitution" and lo + 1 >= 1 + (length - 32) // 31:
                    continue  # (the run is its last k-mer)
                codes = _read(ref, start, length, allele)
                for k in range(lo):
                    codes[31 * k + 3] = 15
                    _substitute(codes, 31 * k + 6)
                if extra == "substitution":
                    _substitute(codes, 31 * (lo + 1) + 10)  # (its label comes from a Hamming-1 list: the chains' counts differ from the walk's)
                if extra == "set":
                    codes[SNP_AT - start] = CODE[ref[SNP_AT]] | CODE[alt[SNP_AT]]
                out.append(("snps", "B run from k-mer %d, SNP at its base %d, %s" % (lo, off, name), codes, start, want))
    return ref, recs, pair, out


@pytest.fixture(scope="module")
def cases():
    ref, recs, pair, reads = _make_reads()
    graphs = {"snps": recs, "pair": pair}
    made = {}
    for name, rr in graphs.items():
        sel = [r for r in reads if r[0] == name]
        text = synth.bases_to_str(ref)
        made[name] = dict(graph=gtx.graph_from_records(text, rr, region_begin=RB), oracle=Oracle(text, rr, region_begin=RB), names=[r[1] for r in sel],
                          reads=[r[2] for r in sel], pos=np.array([r[3] + RB for r in sel], np.int64), want=np.array([r[4] for r in sel]))
    assert sum(len(m["reads"]) for m in made.values()) < 600
    return made


def _passes(b, n):
    pass_of, why = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    b.L.emu_pass_of(C.c_void_p(b.h), pass_of.ctypes.data_as(C.c_void_p), why.ctypes.data_as(C.c_void_p), C.c_uint32(n))
    return pass_of, why


@pytest.mark.parametrize("build", ["lean", "dense"])
@pytest.mark.parametrize("which", ["snps", "pair"])
def test_hand_made_reads_on_the_emulation(cases, which, build, monkeypatch):
    """every record equals the oracle's; the reads that are to be finished are finished by pass 0, the twins leave it with
    the note of their decline site"""
    monkeypatch.setenv("GTX_HINT_BUILD", build)
    monkeypatch.setenv("GTX_EXPRESS4", "wide" if build == "dense" else "lean")
    c = cases[which]
    b = harness.EmuBackend(c["graph"])
    check_align(b, c["oracle"], c["reads"], pos=c["pos"])
    pass_of, why = _passes(b, len(c["reads"]))
    for k, name in enumerate(c["names"]):
        print("%-90s pass %d note %3d  (want %d)" % (name, pass_of[k], why[k], c["want"][k]))
    done = c["want"] == DONE
    wrong = [c["names"][k] for k in np.nonzero(done & (pass_of != 0))[0]]
    assert not wrong, "not finished by pass 0: %s" % wrong[:8]
    wrong = [(c["names"][k], int(why[k])) for k in np.nonzero(~done & ((pass_of == 0) | (why != c["want"])))[0]]
    assert not wrong, "a twin that was finished, or declined with another note: %s" % wrong[:8]


def test_the_switch_restores_the_declines(cases, monkeypatch):
    """GTX_HINT_MORE=0 (the A/B switch): the new shapes leave pass 0 again, with the notes of their sites; the records stay the oracle's"""
    monkeypatch.setenv("GTX_HINT_BUILD", "lean")
    c = cases["snps"]
    b = harness.EmuBackend(c["graph"])
    seq, lens = harness.pack_ragged(c["reads"])
    b.align(seq, harness.read_meta(lens, pos=c["pos"]))
    with_more, _ = _passes(b, len(c["reads"]))
    monkeypatch.setenv("GTX_HINT_MORE", "0")
    check_align(b, c["oracle"], c["reads"], pos=c["pos"])
    without, why = _passes(b, len(c["reads"]))
    moved = (with_more == 0) & (without != 0)
    assert not ((with_more != 0) & (without == 0)).any()
    assert moved.sum() >= 100 and set(why[moved].tolist()) == {NOTE_SEVERAL, NOTE_TWIN}


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["lean", "dense"])
def test_hand_made_reads_on_the_device(cases, build, monkeypatch):
    """the same reads through the C ABI: the oracle's records, and pass 0 finishes as many reads as the emulation's"""
    import torch
    assert torch.cuda.is_available(), "this test needs the GPU"
    monkeypatch.setenv("GTX_HINT_BUILD", build)
    monkeypatch.setenv("GTX_EXPRESS4", "wide" if build == "dense" else "lean")
    for which in ("snps", "pair"):
        c = cases[which]
        check_align(harness.GpuBackend(c["graph"]), c["oracle"], c["reads"], pos=c["pos"])
        e = harness.EmuBackend(c["graph"])
        seq, lens = harness.pack_ragged(c["reads"])
        e.align(seq, harness.read_meta(lens, pos=c["pos"]))
        assert check_align.hinted_done == e.hinted_done() >= int((c["want"] == DONE).sum())


def test_random_sweep_with_many_ambiguous_bases():
    """snp1k, 20 000 reads, 2 % N and 3 % substitutions: every record equals the oracle's, and the shapes are met by the thousand"""
    ref, recs, codes, pos = scenarios.synthetic_case("snp1k", n_ref=100000, n_reads=20000, region_begin=RB, err=0.03, n_rate=0.02, seed=11)
    b = harness.EmuBackend(gtx.graph_from_records(ref, recs, region_begin=RB))
    check_align(b, Oracle(ref, recs, region_begin=RB), list(codes), pos=pos)
    pass_of, why = _passes(b, len(codes))
    print("finished by pass 0 / express / general:", [int((pass_of == k).sum()) for k in range(3)])
    assert (pass_of == 0).sum() > 0.6 * len(codes)


def test_general_pass_share_is_halved():
    """cfg2-like sample: the general pass finished 761 of these 1.2 M reads before; at most 380 now"""
    n = 1200000
    ref, recs, codes, pos = scenarios.synthetic_case("snp1k", n_ref=400000, n_reads=n, region_begin=RB)
    b = harness.EmuBackend(gtx.graph_from_records(ref, recs, region_begin=RB))
    seq, lens = harness.pack_ragged(list(codes))
    b.align(seq, harness.read_meta(lens, pos=pos))
    pass_of, why = _passes(b, n)
    general = int((pass_of >= 2).sum())
    print("general pass:", general, "of", n, "; by note:", {int(k): int(((why == k) & (pass_of >= 2)).sum()) for k in np.unique(why[pass_of >= 2])})
    assert general <= 380
