"""Records what libdeflate -- the encoder behind htslib, so behind most BAM files -- makes of the inputs of
tests/inflate_corpus.recorded_inputs() at levels 1, 6, 9 and 12, as raw DEFLATE streams, into libdeflate_streams.bin.  Run
where libdeflate.so.0 loads (no headers needed: three calls through ctypes):
    python tests/golden/make_libdeflate_streams.py
The inputs come back from their seeds, so the file holds the streams, the inputs' CRC-32 and sizes, nothing else.  The tests
read the file and never the library (tests/test_inflate_made_streams.py: zlib first, then the decoders)."""
import ctypes as C
import struct
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import inflate_corpus as ic  # noqa: E402

L = C.CDLL("libdeflate.so.0")
L.libdeflate_alloc_compressor.restype = C.c_void_p
L.libdeflate_alloc_compressor.argtypes = [C.c_int]
L.libdeflate_deflate_compress.restype = C.c_size_t
L.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
L.libdeflate_free_compressor.argtypes = [C.c_void_p]

streams = []
for name, data in sorted(ic.recorded_inputs().items()):
    for level in (1, 6, 9, 12):
        c = L.libdeflate_alloc_compressor(level)
        assert c
        out = C.create_string_buffer(len(data) + len(data) // 8 + 512)
        n = L.libdeflate_deflate_compress(c, data, len(data), out, len(out))
        L.libdeflate_free_compressor(c)
        assert n > 0
        comp = out.raw[:n]
        assert zlib.decompressobj(-15).decompress(comp) == data
        streams.append(struct.pack("<16s4I", name.encode(), level, len(data), zlib.crc32(data), n) + comp)
open(os.path.join(HERE, "libdeflate_streams.bin"), "wb").write(struct.pack("<I", len(streams)) + b"".join(streams))
print(len(streams), "streams,", sum(len(s) for s in streams), "bytes")
