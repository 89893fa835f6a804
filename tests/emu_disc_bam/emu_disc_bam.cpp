// Host emulation of gtx_disc_bam_unpack_kernel (gtx_disc_bam.hip): the records of a stream through the kernel's source
// (gtx_disc_bam_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_disc_bam case.bin out.bin
// case.bin: uint32 n_reads, n_bytes, n_cigar, plane_stride, qual_stride, waves; the stream's n_bytes bytes; n_reads uint32 offsets;
// n_reads gtx_disc_read.  out.bin: n_reads plane rows, n_reads quality rows, n_cigar cigar words (all filled with 0xA5 before the run).
// Two runs.  Record by record (HeapBatch): every record's bytes sit in a heap block of exactly the size the text may read -- the record
// from its 32 fixed bytes to the end of its block, and DISC_BAM_SLACK bytes, nothing in front --, and every record's plane row, quality
// row and CIGAR words are heap blocks of exactly plane_stride bytes, qual_stride bytes and n_cigar words: a load or a store outside of
// them stops the driver.  Then over the arrays as the launch has them (BamBatch, the addressing of gtx_disc_bam_unpack itself): the
// stream in one heap block of n_bytes + DISC_BAM_SLACK bytes, so that every record lies at its own address residue, and the three
// outputs in blocks of exactly their sizes.  The two runs must leave the same bytes (exit status 3 otherwise); out.bin is the first
// one's.  The records run over `waves` wavefronts as the launch deals them: wavefront w takes records w, w + waves, ...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_disc_bam.hpp"
#include "gtx_disc_bam_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
struct HeapBatch
{
  gtx_disc_read const * reads;
  uint32_t n_reads, plane_stride, qual_stride;
  std::vector<uint8_t const *> const * records;
  std::vector<std::unique_ptr<uint32_t[]>> const * rows;
  std::vector<std::unique_ptr<uint8_t[]>> const * quals;
  std::vector<std::unique_ptr<uint32_t[]>> const * cigars;
  gtx_disc_read read(uint32_t i) const { return reads[i]; }
  uint8_t const * record_of(uint32_t i) const { return (*records)[i]; }
  uint32_t * row_of(uint32_t i) const { return (*rows)[i].get(); }
  uint8_t * qual_of(uint32_t i) const { return (*quals)[i].get(); }
  uint32_t * cigar_of(uint32_t i, gtx_disc_read const &) const { return (*cigars)[i].get(); }
};

bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_disc_bam case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[6];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const n_reads = h[0], n_bytes = h[1], n_cigar = h[2], plane_stride = h[3], qual_stride = h[4], waves = h[5];
  if (plane_stride == 0 || plane_stride % PLANE_GROUP_BYTES || waves == 0)
    return 2;
  std::vector<uint8_t> stream(n_bytes);
  std::vector<uint32_t> offsets(n_reads);
  std::vector<gtx_disc_read> reads(n_reads);
  if (!read_exact(f, stream.data(), n_bytes) || !read_exact(f, offsets.data(), n_reads * 4ull) || !read_exact(f, reads.data(), n_reads * sizeof(gtx_disc_read)))
    return 2;
  std::fclose(f);
  std::vector<std::unique_ptr<uint8_t[]>> blocks(n_reads), quals(n_reads);
  std::vector<uint8_t const *> records(n_reads);
  std::vector<std::unique_ptr<uint32_t[]>> rows(n_reads), cigars(n_reads);
  for (uint32_t i = 0; i < n_reads; ++i)
  {
    gtx_disc_read const & r = reads[i];
    uint32_t block_size = 0;
    if (offsets[i] < 4 || offsets[i] > n_bytes)
      return 2;
    std::memcpy(&block_size, stream.data() + offsets[i] - 4, 4);
    if (block_size < 32 || block_size > n_bytes - offsets[i] || r.l_qseq > qual_stride || r.l_qseq > 2u * plane_stride ||
        static_cast<uint64_t>(r.cigar_off) + r.n_cigar > n_cigar)
      return 2;
    size_t const size = static_cast<size_t>(block_size) + DISC_BAM_SLACK;
    blocks[i].reset(new uint8_t[size]());
    std::memcpy(blocks[i].get(), stream.data() + offsets[i], std::min<size_t>(size, n_bytes - offsets[i]));
    records[i] = blocks[i].get();
    rows[i].reset(new uint32_t[plane_stride / 4u]);
    std::memset(rows[i].get(), 0xA5, plane_stride);
    quals[i].reset(new uint8_t[qual_stride]);
    std::memset(quals[i].get(), 0xA5, qual_stride);
    cigars[i].reset(new uint32_t[r.n_cigar]);
    std::memset(cigars[i].get(), 0xA5, r.n_cigar * 4u);
  }
  HeapBatch const batch{reads.data(), n_reads, plane_stride, qual_stride, &records, &rows, &quals, &cigars};
  for (uint32_t w = 0; w < waves; ++w)
    disc_bam_unpack_wave<WaveSeq>(batch, w, waves);
  std::vector<uint32_t> cigar(n_cigar, 0xA5A5A5A5u);
  for (uint32_t i = 0; i < n_reads; ++i)
    if (reads[i].n_cigar)
      std::memcpy(cigar.data() + reads[i].cigar_off, cigars[i].get(), reads[i].n_cigar * 4u);
  // the same over the launch's own arrays
  std::unique_ptr<uint8_t[]> whole(new uint8_t[static_cast<size_t>(n_bytes) + DISC_BAM_SLACK]());
  std::memcpy(whole.get(), stream.data(), n_bytes);
  std::unique_ptr<uint32_t[]> w_planes(new uint32_t[static_cast<size_t>(n_reads) * plane_stride / 4u]), w_cigar(new uint32_t[n_cigar]);
  std::unique_ptr<uint8_t[]> w_qual(new uint8_t[static_cast<size_t>(n_reads) * qual_stride]);
  std::memset(w_planes.get(), 0xA5, static_cast<size_t>(n_reads) * plane_stride);
  std::memset(w_qual.get(), 0xA5, static_cast<size_t>(n_reads) * qual_stride);
  std::memset(w_cigar.get(), 0xA5, n_cigar * 4ull);
  BamBatch const launch{whole.get(), offsets.data(), reads.data(), n_reads, reinterpret_cast<uint8_t *>(w_planes.get()), plane_stride, w_qual.get(), qual_stride,
                        w_cigar.get()};
  for (uint32_t w = 0; w < waves; ++w)
    disc_bam_unpack_wave<WaveSeq>(launch, w, waves);
  for (uint32_t i = 0; i < n_reads; ++i)
    if (std::memcmp(rows[i].get(), reinterpret_cast<uint8_t *>(w_planes.get()) + static_cast<size_t>(i) * plane_stride, plane_stride) != 0 ||
        std::memcmp(quals[i].get(), w_qual.get() + static_cast<size_t>(i) * qual_stride, qual_stride) != 0)
    {
      std::fprintf(stderr, "record %u: the run over the launch's arrays leaves other rows\n", i);
      return 3;
    }
  if (n_cigar && std::memcmp(cigar.data(), w_cigar.get(), n_cigar * 4ull) != 0)
  {
    std::fprintf(stderr, "the run over the launch's arrays leaves other cigar words\n");
    return 3;
  }
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;
  for (uint32_t i = 0; i < n_reads; ++i)
    if (std::fwrite(rows[i].get(), 1, plane_stride, o) != plane_stride)
      return 2;
  for (uint32_t i = 0; i < n_reads; ++i)
    if (qual_stride && std::fwrite(quals[i].get(), 1, qual_stride, o) != qual_stride)
      return 2;
  if (n_cigar && std::fwrite(cigar.data(), 4, n_cigar, o) != n_cigar)
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
