// Host emulation of the record walk's three kernels (gtx_disc_bam_walk.hip): a stream through the kernels' source
// (gtx_disc_bam_walk_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_disc_bam_walk case.bin out.bin
// case.bin: uint32 n_bytes, n_lists, waves; the stream's n_bytes bytes; per list uint32 n_cuts and the n_cuts cuts.
// out.bin: per list gtx_bam_walk_out, then n_reads offsets and n_reads gtx_disc_read.
// Per list the three steps as the library launches them: guess over `waves` wavefronts (wavefront w takes the segments w, w + waves,
// ...), resolve on one, the tables sized from resolve's count, emit over `waves` wavefronts.  The stream sits in a heap block of
// exactly n_bytes bytes -- nothing in front, nothing behind --, the cuts, the segment table, `out` and the two tables in heap blocks
// of exactly their sizes (the tables filled with 0xA5 before emit): a load or a store outside of them stops the program.  A list
// that is no list (a cut outside (0, n_bytes), cuts that do not ascend) is refused as the library refuses it (exit status 2).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_disc_bam_walk_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
bool write_exact(std::FILE * f, void const * p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_disc_bam_walk case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[3];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const n_bytes = h[0], n_lists = h[1], waves = h[2];
  if (waves == 0)
    return 2;
  std::unique_ptr<uint8_t[]> stream(new uint8_t[n_bytes]);
  if (!read_exact(f, stream.get(), n_bytes))
    return 2;
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;
  for (uint32_t k = 0; k < n_lists; ++k)
  {
    uint32_t n_cuts = 0;
    if (!read_exact(f, &n_cuts, 4))
      return 2;
    std::unique_ptr<uint32_t[]> cuts(new uint32_t[n_cuts]);
    if (!read_exact(f, cuts.get(), n_cuts * 4ull))
      return 2;
    for (uint32_t i = 0; i < n_cuts; ++i)
      if (cuts[i] == 0 || cuts[i] >= n_bytes || (i && cuts[i] <= cuts[i - 1]))
        return 2;
    std::unique_ptr<gtx_bam_walk_out> out(new gtx_bam_walk_out{});
    std::unique_ptr<uint32_t[]> offsets;
    std::unique_ptr<gtx_disc_read[]> reads;
    if (n_bytes != 0) // (the library launches nothing for an empty stream)
    {
      std::unique_ptr<BamWalkSeg[]> segs(new BamWalkSeg[static_cast<size_t>(n_cuts) + 1]);
      std::memset(segs.get(), 0xA5, (static_cast<size_t>(n_cuts) + 1) * sizeof(BamWalkSeg));
      BamWalkBatch const batch{stream.get(), n_bytes, cuts.get(), n_cuts, segs.get()};
      for (uint32_t w = 0; w < waves; ++w)
        disc_bam_walk_guess_wave<WaveSeq>(batch, w, waves);
      disc_bam_walk_resolve_wave<WaveSeq>(batch, out.get());
      offsets.reset(new uint32_t[out->n_reads]);
      reads.reset(new gtx_disc_read[out->n_reads]);
      std::memset(offsets.get(), 0xA5, out->n_reads * sizeof(uint32_t));
      std::memset(static_cast<void *>(reads.get()), 0xA5, out->n_reads * sizeof(gtx_disc_read));
      if (out->n_reads)
        for (uint32_t w = 0; w < waves; ++w)
          disc_bam_walk_emit_wave<WaveSeq>(batch, offsets.get(), reads.get(), w, waves);
    }
    if (!write_exact(o, out.get(), sizeof(gtx_bam_walk_out)) || !write_exact(o, offsets.get(), out->n_reads * sizeof(uint32_t)) ||
        !write_exact(o, reads.get(), out->n_reads * sizeof(gtx_disc_read)))
      return 2;
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 2;
}
