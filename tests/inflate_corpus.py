"""The DEFLATE streams the device decoder is held to, for its emulation (test_inflate_device_emu.py) and the device
(test_gpu_bgzf_inflate.py): the corpus of test_inflate.py -- the same generator, seeds and draws -- plus sizes and codes that
corpus meets only by chance, the hand-made streams, and the damage test_inflate.py applies.  The yardstick is zlib."""
import struct
import zlib

import numpy as np

import emu_programs
from test_inflate import _data, _deflate

OK, BAD_STREAM, SHORT, LONG, CRC, BAD_MEMBER = range(6)
STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


def _damage(rng, it, comp, n):
    """test_inflate.py's damage: (stream, out_len)"""
    bad, how, want = bytearray(comp), it % 4, n
    if how == 0 and bad:
        bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
    elif how == 1 and bad:
        bad = bad[:int(rng.integers(0, len(bad)))]
    elif how == 2:
        want = want + 1 if it % 8 < 4 or want == 0 else want - 1
    else:
        bad += b"\x00\x01"
    return bytes(bad), want


def seeded(seed):
    """the 120 streams of test_inflate.test_equals_zlib(seed): [(data, stream, (damaged stream, its out_len))]"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(120):
        n = int(rng.integers(0, 40)) if it % 8 == 0 else int(rng.integers(0, 65537))
        data = _data(rng, int(rng.integers(0, 6)), n)
        flushes = sorted((int(rng.integers(0, n + 1)), int(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))) for _ in range(int(rng.integers(0, 4)))) if it % 3 == 0 else []
        comp = _deflate(data, int(rng.integers(0, 10)), int(rng.choice(STRATEGIES)), flushes)
        out.append((data, comp, _damage(rng, it, comp, n)))
    return out


def fibonacci_data():
    """byte k as often as the k-th Fibonacci number: the Huffman code of it is as deep as the alphabet is large, so zlib has to
    cut it at 15 bits -- codes of every length up to 15, in the literal code and in the code-length code's input"""
    f, parts = [1, 1], []
    while sum(f) + f[-1] + f[-2] <= 65536:
        f.append(f[-1] + f[-2])
    for k, c in enumerate(f):
        parts.append(np.full(c, k, np.uint8))
    a = np.concatenate(parts)
    np.random.default_rng(7).shuffle(a)
    return a.tobytes()


def extras():
    """every kind at the sizes that matter (empty, very short, 65 535, 65 536), every level and strategy once more, and the
    skewed alphabets that bring codes of up to 15 bits: [(data, stream)]"""
    rng = np.random.default_rng(99)
    out = []
    for kind in range(6):
        for n in (0, 1, 2, 3, 7, 64, 65, 65535, 65536):
            data = _data(rng, kind, n)
            out.append((data, _deflate(data, 6, zlib.Z_DEFAULT_STRATEGY, [])))
        data = _data(rng, kind, 65536)
        for level in range(10):
            out.append((data, _deflate(data, level, zlib.Z_DEFAULT_STRATEGY, [(30000, zlib.Z_SYNC_FLUSH)] if level % 2 else [])))
        for strategy in STRATEGIES:
            out.append((data, _deflate(data, 9, strategy, [(1, zlib.Z_FULL_FLUSH), (65535, zlib.Z_SYNC_FLUSH)])))
    fib = fibonacci_data()
    for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_HUFFMAN_ONLY):
        out.append((fib, _deflate(fib, 6, strategy, [])))
    for s in (1.05, 1.1, 1.2):
        data = bytes(np.minimum(rng.zipf(s, 65536), 255).astype(np.uint8))
        out.append((data, _deflate(data, 6, zlib.Z_HUFFMAN_ONLY, [])))
    return out


# test_inflate.test_hand_made_streams: (stream, out_len, bytes or None = refused)
HAND_MADE = [(b"\x03\x00", 0, b""), (b"\x01\x00\x00\xff\xff", 0, b""), (b"\x01\x03\x00\xfc\xffabc", 3, b"abc"),
             (b"\x00\x00\x00\xff\xff" + b"\x03\x00", 0, b""),
             (b"", 0, None), (b"\x07\x00", 0, None), (b"\x01\x03\x00\xfc\xfeabc", 3, None), (b"\x01\x03\x00\xfc\xffab", 3, None), (b"\x03", 1, None),
             (bytes([0b00000011, 0b00000010, 0]), 3, None)]


def zlib_verdict(stream, out_len):
    """what zlib inflates the (possibly damaged) stream to when it takes it as a whole stream of out_len bytes, else None"""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(stream)
    except zlib.error:
        return None
    return got if d.eof and len(got) == out_len else None


def max_code_bits(stream):
    """the longest literal / length or distance code any dynamic block's header of the stream declares (a small RFC 1951 header
    parser over zlib's own walk of the blocks would be the decoder again: this only looks at a stream that is ONE dynamic block)"""
    bits = int.from_bytes(stream, "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v
    take(1)
    if take(2) != 2:
        return 0
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = take(3)
    code, codes = 0, {}
    for length in range(1, 8):
        for s in range(19):
            if cl[s] == length:
                codes[(length, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, length = 0, 0
        while (length, c) not in codes:
            c = (c << 1) | take(1)
            length += 1
        s = codes[(length, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    return max(lens)


def run_emu(driver, tmp_path, members, in_blob, mode, check_crc=True, out_size=0, fill=0x5A):
    """members: [(in_off, in_len, out_off, out_len, crc32)].  Returns (statuses, output bytes) of tests/emu_inflate."""
    def write(path):
        with open(path, "wb") as f:
            f.write(struct.pack("<6I", mode, len(members), int(check_crc), len(in_blob), out_size, fill))
            for m in members:
                f.write(struct.pack("<5I", *m))
            f.write(in_blob)
    raw = emu_programs.run(driver, tmp_path, write, lambda path: open(path, "rb").read())
    return np.frombuffer(raw[:4 * len(members)], np.uint32), raw[4 * len(members):]


def pack(streams, rng=None):
    """streams one behind the other (with 0 .. 3 bytes of padding in front of each when rng is given: odd offsets):
    (blob, [(in_off, in_len)])"""
    blob, where = bytearray(), []
    for s in streams:
        if rng is not None:
            blob += bytes(int(rng.integers(0, 4)))
        where.append((len(blob), len(s)))
        blob += s
    return bytes(blob), where


def recorded_inputs():
    """the inputs of tests/golden/libdeflate_streams.bin, from their seeds: {name: bytes} -- test_inflate._data's kinds and the
    records of a BAM file as tests/bam_writer.py writes them"""
    import bam_writer as bw
    rng = np.random.default_rng(1951)
    out = {"acgt": _data(rng, 1, 24000), "text": _data(rng, 2, 65536), "runs": _data(rng, 3, 40000), "zipf": _data(rng, 4, 12000),
           "noise": _data(rng, 0, 600), "empty": b"", "one": b"G"}
    recs, pos = bytearray(), 1000
    for i in range(400):
        pos += int(rng.integers(0, 40))
        if len(recs) > 16000:
            break
        recs += bw.record("read%d" % i, int(rng.choice([0, 16, 99, 147])), 0, pos, int(rng.integers(0, 61)), [("M", 100), ("I", 2), ("M", 49)], 0, pos + 200, 351,
                          rng.choice([1, 2, 4, 8], size=151).astype(np.uint8), [("AS", "C", int(rng.integers(0, 151))), ("XS", "C", 20), ("RG", "Z", "grp1")],
                          qual=rng.choice([11, 25, 37, 40], size=151, p=[0.05, 0.1, 0.25, 0.6]))
    out["bam_records"] = bytes(recs)
    return out


def recorded_libdeflate():
    """the streams libdeflate made of recorded_inputs() at levels 1, 6, 9 and 12 (tests/golden/make_libdeflate_streams.py wrote
    them; only the fixture is read here, never the library): [(name, level, data, stream)].  The file: uint32 n, then per stream
    16 bytes of name, uint32 level, size, crc32, stream length, and the stream."""
    import os
    raw = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libdeflate_streams.bin"), "rb").read()
    inputs, out, at = recorded_inputs(), [], 4
    for _ in range(struct.unpack_from("<I", raw, 0)[0]):
        name, level, size, crc, n = struct.unpack_from("<16s4I", raw, at)
        name, at = name.rstrip(b"\0").decode(), at + 32
        data = inputs[name]
        assert len(data) == size and zlib.crc32(data) == crc, "the input %s is not what the fixture was made of" % name
        out.append((name, level, data, raw[at:at + n]))
        at += n
    assert at == len(raw)
    return out
