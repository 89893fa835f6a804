"""The way out of the position-hinted pass (pass 0) on the device: records built in the lane's LDS row, staged records leaving in as
many rounds as there are, queue appends per wavefront.  Everything goes through the C ABI (harness.GpuBackend); records, side bytes
and compact records are held to the oracle the way test_emu_parity.check_align holds them -- the same words with the right hints,
without hints and with shifted hints, and the oracle's paths -- with the dense records of the pass (HARNESS_COMPACT=1) and without."""
import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

RB = 1000000
N_READS = 6000
PAIRED_BOTH = 1  # (SAM: paired, both mates on the same strand -- align_read aligns both orientations: a reverse task for queue 2)


class Case:
    """a graph, its reads and the oracle's result for them (computed once, then read only)"""

    def __init__(self, kind, n_ref=60000, n_reads=N_READS, seed=0, err=0.005, n_rate=0.001, iupac=0.0):
        aav = kind == "cfg3"
        self.ref, self.recs, codes, self.pos = scenarios.synthetic_case(kind, n_ref=n_ref, n_reads=n_reads, region_begin=RB, seed=seed, err=err,
                                                                        n_rate=n_rate)
        if iupac:
            rng = np.random.default_rng(seed + 77)
            codes = codes.copy()
            amb = rng.random(codes.shape) < iupac
            codes[amb] |= rng.integers(1, 16, size=codes.shape).astype(np.uint8)[amb]  # (the true base widened to a set)
        self.codes = codes
        self.pos = np.asarray(self.pos, np.int64)
        self.graph = gtx.graph_from_records(self.ref, self.recs, region_begin=RB, add_all_variants=aav)
        self.oracle = Oracle(self.ref, self.recs, region_begin=RB, add_all_variants=aav)
        self._want = {}
        self._backend = None

    def backend(self):
        if self._backend is None:
            self._backend = harness.GpuBackend(self.graph)
        return self._backend

    def want(self, which, sam_flags=None):
        """the oracle's paths of reads `which`; all reads of the case are aligned once, reads with SAM flags per batch"""
        if sam_flags is None or not np.any(sam_flags):
            if None not in self._want:
                self._want[None] = self.oracle.align(list(self.codes))
            return [self._want[None][i] for i in which]
        key = (bytes(np.asarray(which, np.int64)), bytes(np.asarray(sam_flags, np.uint16)))
        if key not in self._want:
            self._want[key] = self.oracle.align([self.codes[i] for i in which], flags=sam_flags)
        return self._want[key]


_cases = {}


def case(kind, **kw):
    key = (kind,) + tuple(sorted(kw.items()))
    if key not in _cases:
        _cases[key] = Case(kind, **kw)
    return _cases[key]


def hold(c, which, flags=None, rec_words=harness.REC_WORDS, hint=None, variants=True, overflow_ok=False):
    """reads `which` of the case as one batch: the same record words whatever the hints are, the oracle's paths, and -- dense records --
    side bytes that say what the records say.  flags: gtx_read_meta::flag (SAM bits, GTX_FLAG_FORWARD_ONLY).  Returns the backend
    (its counts are those of the call with `hint`, by default the right hints)."""
    which = np.asarray(which)
    b = c.backend()
    reads = [c.codes[i] for i in which]
    n = len(reads)
    seq, lens = harness.pack_ragged(reads)
    pos = c.pos[which] if hint is None else np.asarray(hint, np.int64)
    fl = None if flags is None else np.asarray(flags, np.uint16)
    others = []
    if variants:
        for v in (None, pos + 1):
            others.append(b.align(seq, harness.read_meta(lens, fl, pos=v), rec_words).copy().reshape(2 * n, rec_words))
    rec = b.align(seq, harness.read_meta(lens, fl, pos=pos), rec_words).copy().reshape(2 * n, rec_words)
    external = ((rec[:, 0] >> 16) & gtx.ST_EXTERNAL) != 0
    for w in others:
        differ = w != rec
        differ[external, 2:] = False  # (an offset into the big-record arena differs from call to call)
        bad = np.nonzero(differ.any(1))[0]
        assert len(bad) == 0, "the records depend on the position hint: tasks %s, words %s" % (bad[:5], np.nonzero(differ[bad[0]])[0])
    if b.compact is not None:
        side = b.compact["fl"]
        has = (rec[:, 1] >> 31).astype(np.uint8)
        npaths = rec[:, 0] & 0xFFFF
        assert np.array_equal(side[0::2] & gtx.TASK_HAS_VARIANTS, has[0::2]), "the forward tasks' side bytes and their records disagree"
        compact = (side[0::2] & gtx.TASK_COMPACT) != 0
        assert not (compact & (has[0::2] != 0)).any() and (npaths[0::2][compact] <= 1).all(), "a compact record with a variant site or two paths"
    big, _ = b.big_records()
    got = gtx.parse_records(rec.reshape(-1), n, rec_words, b.ctx.hap_order, big)
    want = c.want(which, None if fl is None else (fl & 0x0FFF))
    for k, i in enumerate(which):
        for o in range(2):
            g = got[k][o]
            if g["status"] != 0:
                assert overflow_ok and g["paths"] == [] and g["longest"] == 0, "read %d orientation %d: status %d" % (i, o, g["status"])
                continue
            assert dict(longest=g["longest"], paths=g["paths"]) == want[k][o], "read %d orientation %d: %r != oracle %r" % (
                i, o, g, want[k][o])
    b.forward = rec[0::2]  # (the forward records of the batch, compact ones in their slots)
    return b


def queue_fills(b):
    """(entries of queue 1, entries of queue 2) of the backend's last align call, from the counts gtx_ctx_kernel_times reports:
    queue 1 holds what pass 0 neither finished nor sent on itself; queue 2 is what the general and the HBM pass worked off"""
    (_, _, done0), (_, _, done1), (_, _, t2), (_, _, t3) = b.ctx.kernel_times()
    return done0, done1, t2 + t3


@pytest.fixture(params=["slots", "dense_records"])
def compact(request, monkeypatch):
    if request.param == "dense_records":
        monkeypatch.setenv("HARNESS_COMPACT", "1")
    else:
        monkeypatch.delenv("HARNESS_COMPACT", raising=False)
    return request.param == "dense_records"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, N_READS])
def test_batch_sizes(n, compact):
    """a partial wavefront, a workgroup whose second wavefront is empty, an unaligned tail, many workgroups"""
    c = case("snp100")
    b = hold(c, np.arange(n))
    assert (b.compact is not None) == compact
    assert b.hinted_done() > 0 or n == 1


@pytest.mark.parametrize("n", [129, N_READS])
@pytest.mark.parametrize("mix", ["forward", "reverse_beside", "hints"])
def test_every_wavefront_appends(mix, n, compact, monkeypatch):
    """every wavefront has something for the queues.  forward: pass 0 declines every forward task (GTX_HINT=d) -- queue 1 holds every
    read once.  reverse_beside: half of the reads also have a reverse task for queue 2, beside the declined forward ones.  hints: no
    switch; a third of the hints missing or shifted, a third of the reads with a reverse task, the others GTX_FLAG_FORWARD_ONLY."""
    c = case("snp100")
    which = np.arange(n)
    rng = np.random.default_rng(11)
    flags = np.full(n, gtx.FLAG_FORWARD_ONLY, np.uint16)
    hint = c.pos[which].copy()
    if mix != "forward":
        flags[rng.random(n) < (0.5 if mix == "reverse_beside" else 0.33)] = PAIRED_BOTH
    if mix == "hints":
        hint[rng.random(n) < 0.15] = -1
        shifted = rng.random(n) < 0.15
        hint[shifted & (hint >= 0)] += 1
    else:
        monkeypatch.setenv("GTX_HINT", "d")
    n_rev = int((flags == PAIRED_BOTH).sum())
    b = hold(c, which, flags=flags, hint=hint, variants=False)
    done0, done1, queue2 = queue_fills(b)
    # (queue 2's fill count against the forward tasks the general pass counted itself, plus the reverse tasks.  Every task has the
    #  oracle's record, so none is missing from its queue; with the count right none is there twice.)
    assert queue2 == (n - done0 - done1) + n_rev, (done0, done1, queue2, n_rev)
    if mix != "hints":
        assert done0 == 0  # (queue 1 held all n forward tasks)
    else:
        assert 0 < done0 < n


@pytest.mark.parametrize("kind", ["snp1k", "snp100", "snp25", "cfg3"])
def test_sites_per_record(kind, compact):
    """0-1 sites (snp1k), 1-2 with every lane staged (snp100), up to six and the decline of a seventh (snp25), the dense build (cfg3)"""
    c = case(kind)
    b = hold(c, np.arange(N_READS))
    rec = b.forward
    nvar = np.where((rec[:, 0] & 0xFFFF) > 0, rec[:, 5] >> 16, 0)
    most = {"snp1k": 1, "snp100": 2, "snp25": 6, "cfg3": 2}[kind]
    assert nvar.max() >= most, nvar.max()
    assert b.hinted_done() > {"snp1k": 0.8, "snp100": 0.5, "snp25": 0.1, "cfg3": 0.3}[kind] * N_READS, b.hinted_done()


@pytest.mark.parametrize("staged", [0, 1, 16, 17, 64])
def test_staged_round_edges(staged, monkeypatch):
    """a wavefront with exactly 0, 1, 16, 17 and 64 staged records: error-free reads over ONE site of a SNP-per-kilobase graph are
    staged (their records carry the site), error-free reads between two sites leave through the compact block.  Two wavefronts: the
    one under test and one without a staged record."""
    monkeypatch.setenv("HARNESS_COMPACT", "1")
    c = case("snp1k", err=0.0, n_rate=0.0)
    sites = np.array(sorted(r[0] for r in c.recs), np.int64)
    site = sites[len(sites) // 2]
    over = np.nonzero((c.pos + 40 <= site) & (site < c.pos + 110))[0]  # (the site well inside the read)
    nearest = np.abs(c.pos[:, None] + 75 - sites[None, :]).min(1)
    clear = np.nonzero(nearest > 200)[0]  # (no site under the read)
    assert len(over) >= 4 and len(clear) >= 64
    lanes = np.resize(clear, 128)
    # (spread over the wavefront: lane 0, the last lane, and every (64 / staged)-th in between)
    at = np.unique(np.round(np.linspace(0, 63, staged)).astype(int)) if staged else np.array([], int)
    assert len(at) == staged
    lanes[at] = np.resize(over, staged)
    b = hold(c, lanes)
    side = b.compact["fl"][0::2]
    assert b.hinted_done() == 128, "pass 0 did not finish every read of the batch: %d" % b.hinted_done()
    is_staged = (side & gtx.TASK_COMPACT) == 0
    assert np.array_equal(np.nonzero(is_staged)[0], at), (np.nonzero(is_staged)[0], at)
    assert (side[at] & gtx.TASK_HAS_VARIANTS).all()


@pytest.mark.parametrize("kind", ["snp100", "snp25"])
@pytest.mark.parametrize("rec_words", [16, 18, 64])
def test_rec_words(rec_words, kind, compact):
    """slots of 16 words (a staged record fills them), of 64, and of 18 -- no multiple of four: records are not staged, pass 0
    builds them in their slots and takes the entries of a read it declines after all out again"""
    c = case(kind)
    b = hold(c, np.arange(2000), rec_words=rec_words, overflow_ok=rec_words < 64)
    # (a SNP every 25 bases: five sites and more under 150 bases, 21 words -- slots of 16 or 18 words hold none of these records,
    #  pass 0 declines every read for want of room, some of them after it has listed their sites)
    assert b.hinted_done() > 0 or (kind == "snp25" and rec_words < 21)


def test_twin_paths(compact):
    """reads whose first k-mer carries an ambiguity code open two chains, and the reference returns the path twice: pass 0 writes
    the twin as a copy of the words it has just put into the row"""
    c = case("snp1k", iupac=0.01, n_reads=3000)
    b = hold(c, np.arange(3000))
    rec = b.forward
    two, nvar = (rec[:, 0] & 0xFFFF) == 2, rec[:, 5] >> 16
    twins = np.nonzero((two & (nvar == 0) & (rec[:, 2:6] == rec[:, 6:10]).all(1)) | (two & (nvar == 1) & (rec[:, 2:9] == rec[:, 9:16]).all(1)))[0]
    assert len(twins) > 0, "no read of the case has twin paths"
    # the twins alone, with the right hints: pass 0 finishes them itself
    b = hold(c, twins, variants=False)
    assert b.hinted_done() == len(twins), (b.hinted_done(), len(twins))
