"""DEFLATE on the device (gtx_inflate_batch, gtx_inflate_bgzf, the readers' device team) over streams zlib's encoder never writes:
the corpus of test_inflate_made_streams.py -- the members of tests/deflate_maker.py and the recorded libdeflate streams, held to
zlib there and taken cleanly by the emulation of the kernel's source under ASan / UBSan -- in batches of a few thousand members
with canaries around every output, each batch twice on fresh buffers (a fence missing between a match and the match that
feeds it shows as a difference between two runs or against zlib, and only here: the emulation is sequential); the members with
one rule of the format broken, ONCE, as ordinary refusals by status; and a BAM file whose members the maker deflated through
gtx_inflate_bgzf and the readers, where the device may refuse no member."""
import zlib

import numpy as np
import pytest

import inflate_corpus as ic
from graphtyper_amd import lib as gtx
from test_gpu_bgzf_inflate import _drain, _same, run_batch
from test_inflate_made_streams import bam_of_made_members, made_corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


@pytest.fixture(scope="module")
def corpus():
    return made_corpus()


def _twice(inflater, picks, seed):
    """the batch on two fresh output buffers: every member ok, every byte the maker's (which is zlib's), both runs the same"""
    streams, lens, crcs = [s for _, _, s, _ in picks], [len(d) for _, d, _, _ in picks], [zlib.crc32(d) for _, d, _, _ in picks]
    runs = [run_batch(inflater, streams, lens, crcs, seed=seed) for _ in range(2)]
    for st, outs in runs:
        assert (st == ic.OK).all(), "valid members refused: %s" % [(picks[i][0], int(st[i])) for i in np.nonzero(st != ic.OK)[0][:10]]
        wrong = [picks[i][0] for i in range(len(picks)) if outs[i] != picks[i][1]]
        assert wrong == [], "members inflated to other bytes: %s" % wrong[:10]
    assert all(a == b for a, b in zip(runs[0][1], runs[1][1]))


def test_made_members_in_one_batch_twice(corpus):
    valid, _ = corpus
    n = 3000
    assert n > len(valid)
    picks = [valid[i % len(valid)] for i in range(n)]  # every member of the corpus, most of them more than once
    inflater = gtx.Inflater(0)
    _twice(inflater, picks, seed=1)
    st, _ = run_batch(inflater, [s for _, _, s, _ in picks], [len(d) for _, d, _, _ in picks], [zlib.crc32(d) ^ (1 << (i % 32)) for i, (_, d, _, _) in enumerate(picks)], seed=2)
    assert (st == ic.CRC).all()
    inflater.close()


def test_matches_fed_by_matches_on_every_cu(corpus):
    """the members in which a match reads what a match of the same batch of 64 tokens wrote (flush's fence rule), alone and in
    thousands of copies, so that every CU runs them at once"""
    valid, _ = corpus
    fed = sorted((v for v in valid if v[3] is not None and v[3]["match_fed_by_match"]), key=lambda v: -v[3]["match_fed_by_match"])
    assert len(fed) >= 5
    total, picks = 0, []
    while len(picks) < 4096 and total < 160 << 20:  # (at least 16 wavefronts on each of the 256 CUs; the output kept below 160 MB)
        picks.append(fed[len(picks) % len(fed)])
        total += len(picks[-1][1])
    assert len(picks) >= 2048
    inflater = gtx.Inflater(0)
    _twice(inflater, picks, seed=3)
    inflater.close()


def test_invalid_members_are_refused_once(corpus):
    """the members with one rule broken (green in the emulation: test_both_decoders_under_sanitizers), once: the emulation's statuses"""
    _, invalid = corpus
    inflater = gtx.Inflater(0)
    st, _ = run_batch(inflater, [s for _, s, _, _, _ in invalid], [n for _, _, n, _, _ in invalid], [0] * len(invalid), check_crc=False, seed=4)
    for i, (kind, _, _, status, reason) in enumerate(invalid):
        assert st[i] in (ic.BAD_STREAM, ic.SHORT, ic.LONG), reason
        assert status is None or st[i] == status, (reason, int(st[i]))
    inflater.close()


def test_bam_file_of_made_members(tmp_path):
    """records deflated by the maker instead of zlib: gtx_inflate_bgzf gives the file's bytes, the reader with the device's team
    gives the host path's records, and the device refused no member of an encoder that is not zlib"""
    made, plain = str(tmp_path / "made.bam"), str(tmp_path / "plain.bam")
    n, members, text = bam_of_made_members(made, plain)
    assert members > 80
    inflater = gtx.Inflater(0)
    assert inflater.bgzf(open(made, "rb").read()) == text
    inflater.close()
    host = _drain(gtx.Reads([made]), False)
    assert len(host[0]) == n and _same(host, _drain(gtx.Reads([plain]), False))
    before = gtx.reads_inflate_counts()
    assert _same(host, _drain(gtx.Reads([made]), True))
    by_device, fell_back, by_reader = (x - y for x, y in zip(gtx.reads_inflate_counts(), before))
    print("members %d: by the device %d, fell back %d, by the reader %d" % (members, by_device, fell_back, by_reader))
    # (up to 32 members are in flight on the host when the reader is switched over)
    assert fell_back == 0 and by_device >= members - 33 - by_reader and by_device > 0
