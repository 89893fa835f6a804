"""DEFLATE on the device (gtx_inflate_*, gtx_reads_set_inflate_device, GTX_BGZF_DEVICE=1 in gtx_pipeline_run) against zlib and,
for files, against the host path: the corpus of test_inflate_device_emu.py through gtx_inflate_batch in batches of 1, 63, 64,
65 and a few thousand members with canaries around every output; the host convenience call; the readers with the device's
team against the same calls without it; the pipeline in two fresh processes."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bam_writer as bw
import inflate_corpus as ic
import scenarios
from graphtyper_amd import lib as gtx
from test_bam_ingest import _random_files
from test_gpu_pipeline_long_reads import RB, write_bams

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GAP, FILL = 24, 0x5A


@pytest.fixture(scope="module", autouse=True)
def _built():
    gtx.build()


@pytest.fixture(scope="module")
def corpus():
    """[(data, stream)] valid, [(stream, out_len, crc of the undamaged data, data)] damaged"""
    valid, damaged = list(ic.extras()), []
    for seed in range(6):
        for d, s, (bad, want) in ic.seeded(seed):
            valid.append((d, s))
            damaged.append((bad, want, zlib.crc32(d), d))
    valid += [(want, s) for s, _, want in ic.HAND_MADE if want is not None]
    damaged += [(s, n, 0, None) for s, n, want in ic.HAND_MADE if want is None]
    return valid, damaged


def run_batch(inflater, streams, out_lens, crcs, check_crc=True, seed=0):
    """the members through gtx_inflate_batch: streams at odd offsets of one buffer, outputs GAP bytes apart in a buffer of FILL.
    Returns (statuses, [output of member i]); asserts the canaries."""
    import torch
    rng = np.random.default_rng(seed)
    blob, where = ic.pack(streams, rng)
    m = np.zeros(len(streams), gtx.INFLATE_MEMBER)
    at = GAP
    for i, ((off, n), out_len, crc) in enumerate(zip(where, out_lens, crcs)):
        m[i] = (off, at, n, out_len, crc, 0)
        at += out_len + GAP
    out_size = at
    d_in = torch.from_numpy(np.frombuffer(blob + bytes(8), np.uint8).copy()).to("cuda:0")
    d_m = torch.from_numpy(m.view(np.uint8).copy()).to("cuda:0")
    d_out = torch.full((out_size,), FILL, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((len(streams),), 99, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    inflater.batch(d_in.data_ptr(), len(blob), d_m.data_ptr(), len(streams), d_out.data_ptr(), out_size, d_st.data_ptr(), check_crc, s.cuda_stream)
    s.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    canary = np.ones(out_size, bool)
    for r in m:
        canary[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])] = False
    assert (out[canary] == FILL).all(), "a store outside a member's output"
    return st, [out[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])].tobytes() for r in m]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_batches_equal_zlib(corpus, n):
    valid, _ = corpus
    inflater = gtx.Inflater(0)
    if n == 3000:
        picks = [valid[i % len(valid)] for i in range(n)]  # every stream of the corpus, most of them more than once
        assert n > len(valid)
    else:
        picks = [valid[(7 * n + 13 * i) % len(valid)] for i in range(n)]
    st, outs = run_batch(inflater, [s for _, s in picks], [len(d) for d, _ in picks], [zlib.crc32(d) for d, _ in picks], seed=n)
    assert (st == ic.OK).all(), "valid streams refused: %s" % np.nonzero(st != ic.OK)[0][:10]
    assert all(o == d for o, (d, _) in zip(outs, picks))
    # a wrong CRC-32 is a CRC status (the bytes are there all the same), and is not looked at when the caller says so
    crcs = [zlib.crc32(d) ^ (1 << (i % 32)) if i % 2 else zlib.crc32(d) for i, (d, _) in enumerate(picks)]
    st, outs = run_batch(inflater, [s for _, s in picks], [len(d) for d, _ in picks], crcs, seed=n + 1)
    assert list(st) == [ic.CRC if i % 2 else ic.OK for i in range(n)]
    st, outs = run_batch(inflater, [s for _, s in picks], [len(d) for d, _ in picks], crcs, check_crc=False, seed=n + 2)
    assert (st == ic.OK).all() and all(o == d for o, (d, _) in zip(outs, picks))
    inflater.close()


def test_damaged_members_are_refused_once(corpus):
    """the damaged streams of the emulation suite (green there: test_inflate_device_emu.py), once: refused, or zlib's bytes"""
    _, damaged = corpus
    inflater = gtx.Inflater(0)
    st, outs = run_batch(inflater, [b for b, _, _, _ in damaged], [n for _, n, _, _ in damaged], [c for _, _, c, _ in damaged], check_crc=False, seed=3)
    taken = 0
    for i, (bad, want, _, _) in enumerate(damaged):
        verdict = ic.zlib_verdict(bad, want)
        if st[i] == ic.OK:
            assert verdict is not None and outs[i] == verdict, i
            taken += 1
        else:
            assert st[i] in (ic.BAD_STREAM, ic.SHORT, ic.LONG) and verdict is None, i
    assert 0 < taken < len(damaged)
    inflater.close()


def test_bgzf_buffers_come_back(tmp_path):
    rng = np.random.default_rng(11)
    text = b"".join(b"chr20\t%d\t.\tA\tC\t%d\n" % (i, int(rng.integers(0, 1 << 30))) for i in range(150000))
    assert len(text) > 3 << 20
    inflater = gtx.Inflater(0)
    for level in (1, 6):
        assert inflater.bgzf(gtx.bgzf_compress(text, level)) == text
    assert inflater.bgzf(gtx.bgzf_compress(b"")) == b""
    files, paths, headers = _random_files(tmp_path, 4)
    raw = open(paths[0], "rb").read()
    want = b"".join(zlib.decompressobj(31).decompress(raw[at:]) for at in _member_starts(raw))
    assert inflater.bgzf(raw) == want and want[:4] == b"BAM\1"
    # a member the device refuses fails the call and is named
    bad = bytearray(gtx.bgzf_compress(text, 6))
    second = _member_starts(bytes(bad))[1]
    bad[second + 18 + 40] ^= 0x10
    with pytest.raises(gtx.GtxError) as e:
        inflater.bgzf(bytes(bad))
    assert e.value.status == 7 and "number 1 " in str(e.value)
    inflater.close()


def test_members_as_the_one_header_parser_sees_them():
    """gtx_inflate_bgzf parses members with the readers' parser (gtx_bgzf.hpp): a member of 1 byte, one of 300 bytes with another
    extra subfield in front of BC and the end-of-file member come back as zlib's bytes; what is not a member is refused, by name,
    before anything is launched"""
    one, some = b"x", bytes(range(256)) + b"graphtyper " * 4
    assert len(some) == 300
    first, second = bw.bgzf(one, with_eof=False), bw.bgzf(some, with_eof=False, extra=b"XY\0\0")
    buf = first + second + bw.bgzf(b"")
    assert second[10:18] == b"\x0a\0XY\0\0BC"
    want = b"".join(zlib.decompressobj(31).decompress(buf[at:]) for at in (0, len(first), len(first) + len(second)))
    inflater = gtx.Inflater(0)
    assert inflater.bgzf(buf) == want == one + some
    huge = bytearray(first)
    huge[-4:] = (65537).to_bytes(4, "little")
    for data, why in ((first + second[:10], "member 1 at byte %d: not a BGZF member" % len(first)),  # cut in the header: in front of XLEN,
                      (first + second[:20], "member 1 at byte %d: truncated" % len(first)),          # ... and inside the extra field
                      (first + second[:-9], "member 1 at byte %d: truncated" % len(first)),          # cut in the data
                      (first[:12] + b"BX" + first[14:] + second, "member 0 at byte 0: no BC field"),
                      (bytes(huge) + second, "member 0 at byte 0: ISIZE beyond 65536")):
        with pytest.raises(gtx.GtxError) as e:
            inflater.bgzf(data)
        assert e.value.status == 7 and str(e.value).endswith("gtx_inflate_bgzf: " + why), str(e.value)
    inflater.close()


def _member_starts(raw):
    at, out = 0, []
    while at < len(raw):
        out.append(at)
        at += int.from_bytes(raw[at + 16:at + 18], "little") + 1
    return out


def _drain(reads, device):
    if device:
        reads.set_inflate_device(0)
    recs, seqs = [], []
    while True:
        r, s = reads.next(777, seq_stride=160)
        if len(r) == 0:
            break
        recs.append(r.copy()), seqs.append(s.copy())
    reads.close()
    return (np.concatenate(recs), np.concatenate(seqs)) if recs else (np.zeros(0, gtx.STREAM_RECORD), np.zeros((0, 160), np.uint8))


def _same(a, b):
    """the same records (field by field: the padding between them is not written) and packed bases, in the same order"""
    return len(a[0]) == len(b[0]) and all((a[0][f] == b[0][f]).all() for f in gtx.STREAM_RECORD.names) and a[1].tobytes() == b[1].tobytes()


def _big_file(tmp_path, name, seed, n=12000, **index):
    rng = np.random.default_rng(seed)
    refs = [("chrA", 400000), ("chrB", 900000)]
    recs = []
    for tid in (0, 1):
        for p in np.sort(rng.integers(0, refs[tid][1] - 400, size=n)):
            recs.append((tid, int(p), rng.choice([1, 2, 4, 8], size=150).astype(np.uint8)))
    header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    path = str(tmp_path / name)
    blobs = [bw.record("r%d" % i, 0, tid, p, 60, [("M", 150)], -1, -1, 0, c, [("AS", "C", 100)]) for i, (tid, p, c) in enumerate(recs)]
    bw.write_bam(path, refs, header, blobs, index=[(tid, p, p + 150) for tid, p, _ in recs], **index)
    return path


def test_readers_with_the_device_team(tmp_path):
    # a multi-file merge
    files, paths, headers = _random_files(tmp_path, 3)
    host = _drain(gtx.Reads(paths), False)
    assert len(host[0]) > 100 and _same(host, _drain(gtx.Reads(paths), True))
    # files of a hundred members each, two readers open at once: one on the device's team, one on the host's.  The members of
    # the first ARE inflated by the device (gtx_reads_inflate_counts: the host stands behind every member the device does not
    # give "ok" and behind every one the team is late for, so equal records alone would not show it), none falls back, and
    # the reader itself takes a few at most; the members of the second are not counted
    big = [_big_file(tmp_path, "big%d.bam" % k, 20 + k) for k in range(2)]
    n_members = sum(len(_member_starts(open(p, "rb").read())) for p in big)
    assert n_members > 150
    host = _drain(gtx.Reads(big), False)
    before = gtx.reads_inflate_counts()
    a, b = gtx.Reads(big), gtx.Reads(big)
    a.set_inflate_device(0)
    got_b = _drain(b, False)
    assert gtx.reads_inflate_counts()[1:] == before[1:]
    got_a = _drain(a, False)
    assert len(host[0]) == 48000 and _same(host, got_a) and _same(host, got_b)
    by_device, fell_back, by_reader = (x - y for x, y in zip(gtx.reads_inflate_counts(), before))
    print("members %d: by the device %d, fell back %d, by the reader %d" % (n_members, by_device, fell_back, by_reader))
    # (up to 32 members per file are in flight on the host when the reader is switched over)
    assert fell_back == 0 and by_device >= n_members - 2 * 33 - by_reader and by_reader <= 4
    # a region started from a .bai and from a .csi: a seek into the middle of a member
    for name, index in (("bai.bam", dict(poison=True)), ("csi.bam", dict(poison=True, csi=(14, 5)))):
        path = _big_file(tmp_path, name, 31, **index)
        for region in ("chrB:500001-620000", "chrA:1-9000"):
            host = _drain(gtx.Reads([path], region=region), False)
            assert len(host[0]) > 50 and _same(host, _drain(gtx.Reads([path], region=region), True)), (name, region)
    # a bit flipped in one member's payload: the same status and message as the host path
    raw = bytearray(open(big[0], "rb").read())
    starts = _member_starts(bytes(raw))
    raw[starts[len(starts) // 2] + 18 + 100] ^= 0x04
    broken = str(tmp_path / "broken.bam")
    open(broken, "wb").write(bytes(raw))
    errors = []
    for device in (False, True):
        before = gtx.reads_inflate_counts()
        with pytest.raises(gtx.GtxError) as e:
            _drain(gtx.Reads([broken]), device)
        errors.append((e.value.status, str(e.value)))
        by_device, fell_back, by_reader = (x - y for x, y in zip(gtx.reads_inflate_counts(), before))
        # the device refused exactly that member (the whole file is one launch: the ring holds it), and the host's verdict was asked for
        assert (by_device > 0 and fell_back == 1) if device else (by_device, fell_back, by_reader) == (0, 0, 0)
    assert errors[0] == errors[1]


def test_pipeline_with_the_switch(tmp_path):
    """gtx_pipeline_run in two fresh processes, GTX_BGZF_DEVICE unset and =1, over the same files: the same counts and the same
    accumulator block, bit for bit"""
    n_pairs = 8000  # (files of more members than a reader has in flight on the host when it is switched over)
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=12000, n_pairs=n_pairs, region_begin=RB, read_len=250, n_samples=2)
    paths = write_bams(tmp_path, rec, list(codes))
    assert all(len(_member_starts(open(p, "rb").read())) > 45 for p in paths)
    outs = []
    for name, value in (("host", None), ("device", "1")):
        env = dict(os.environ)
        env.pop("GTX_BGZF_DEVICE", None)
        if value:
            env["GTX_BGZF_DEVICE"] = value
        out = str(tmp_path / (name + ".npz"))
        # (the second child is not started when the first did not end with status 0: check=True raises)
        subprocess.run([sys.executable, os.path.join(HERE, "inflate_pipeline_child.py"), out, "2", str(n_pairs)] + paths, env=env, check=True, timeout=300)
        outs.append(np.load(out))
    host, dev = outs
    assert int(host["counts"][0]) == len(rec) and int(host["counts"][3]) == 0
    assert (host["counts"] == dev["counts"]).all()
    for k in ("cov", "s64", "s32"):
        assert host[k].tobytes() == dev[k].tobytes(), k
    assert host["cov"].any()
    # the switch is what sends members to the device, and none of them came back refused
    print("inflate counts: host child %s, device child %s" % (list(host["inflate"]), list(dev["inflate"])))
    assert list(host["inflate"]) == [0, 0, 0]
    assert int(dev["inflate"][0]) > 0 and int(dev["inflate"][1]) == 0
