// Host emulation of gtx_disc_events_kernel (gtx_discover.hip): the reads of a batch, 64 at a time, through the kernel's source
// (gtx_disc_events_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_disc_events case.bin out.bin
// case.bin: uint32 plane_stride, qual_stride, n_reads, n_cigar, reference_len, event_cap, counts[0], counts[1]; int64 region_begin;
// uint32 launches; the region's bytes; n_reads plane rows; n_reads quality rows; n_reads gtx_disc_read; n_cigar cigar words.
// out.bin: the two counters, n_reads gtx_disc_read_out, event_cap gtx_disc_event (both filled with 0xA5 before the first launch).
// Every read runs over heap blocks of exactly its sizes -- the plane groups of its row, l_qseq quality bytes, n_cigar words --, the
// region's planes are sized as gtx_disc_create sizes them, the event buffer has exactly event_cap entries (none: a null pointer)
// and the read states exactly n_reads: a load or a store the kernel's bounds should have prevented stops the driver.
// `launches` > 1 repeats the launch over the same counters and buffers (the counters then accumulate).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_disc_events_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
// the batch as the kernel's text asks for it, a heap block per read and array
struct HeapBatch
{
  uint32_t const * refp;
  uint32_t ref_groups;
  long REF_SIZE, region_begin;
  uint32_t plane_stride;
  gtx_disc_read const * reads;
  uint32_t n_reads;
  gtx_disc_event * events;
  uint32_t event_cap;
  uint32_t * counts;
  gtx_disc_read_out * read_out;
  std::vector<std::unique_ptr<uint32_t[]>> const * rows;
  std::vector<std::unique_ptr<uint8_t[]>> const * quals;
  std::vector<std::unique_ptr<uint32_t[]>> const * cigars;
  gtx_disc_read read(uint32_t i) const { return reads[i]; }
  uint32_t const * row_of(uint32_t i) const { return (*rows)[i].get(); }
  uint8_t const * qual_of(uint32_t i) const { return (*quals)[i].get(); }
  uint32_t const * cigar_of(uint32_t i, gtx_disc_read const &) const { return (*cigars)[i].get(); }
};

bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_disc_events case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[8], launches = 0;
  int64_t region_begin = 0;
  if (!f || !read_exact(f, h, sizeof h) || !read_exact(f, &region_begin, 8) || !read_exact(f, &launches, 4))
    return 2;
  uint32_t const plane_stride = h[0], qual_stride = h[1], n_reads = h[2], n_cigar = h[3], reference_len = h[4], event_cap = h[5];
  if (plane_stride == 0 || plane_stride % PLANE_GROUP_BYTES || reference_len == 0)
    return 2;
  std::vector<char> reference(reference_len);
  std::vector<uint32_t> planes(static_cast<size_t>(n_reads) * plane_stride / 4u), cigar(n_cigar);
  std::vector<uint8_t> qual(static_cast<size_t>(n_reads) * qual_stride);
  std::vector<gtx_disc_read> reads(n_reads);
  if (!read_exact(f, reference.data(), reference_len) || !read_exact(f, planes.data(), planes.size() * 4u) || !read_exact(f, qual.data(), qual.size()) ||
      !read_exact(f, reads.data(), reads.size() * sizeof(gtx_disc_read)) || !read_exact(f, cigar.data(), cigar.size() * 4u))
    return 2;
  std::fclose(f);
  // the region's planes, as gtx_disc_create makes them
  uint32_t const ref_groups = disc_ref_groups(reference_len);
  std::unique_ptr<uint32_t[]> refp(new uint32_t[static_cast<size_t>(ref_groups) * 4u]());
  disc_ref_planes(reference.data(), reference_len, refp.get());
  std::vector<std::unique_ptr<uint32_t[]>> rows(n_reads), cigars(n_reads);
  std::vector<std::unique_ptr<uint8_t[]>> quals(n_reads);
  for (uint32_t i = 0; i < n_reads; ++i)
  {
    gtx_disc_read const & r = reads[i];
    if (r.l_qseq > qual_stride || r.l_qseq > plane_stride * 2u || static_cast<uint64_t>(r.cigar_off) + r.n_cigar > n_cigar)
      return 2;
    rows[i].reset(new uint32_t[plane_stride / 4u]);
    std::memcpy(rows[i].get(), planes.data() + static_cast<size_t>(i) * plane_stride / 4u, plane_stride);
    quals[i].reset(new uint8_t[r.l_qseq]);
    std::memcpy(quals[i].get(), qual.data() + static_cast<size_t>(i) * qual_stride, r.l_qseq);
    cigars[i].reset(new uint32_t[r.n_cigar]);
    std::memcpy(cigars[i].get(), cigar.data() + r.cigar_off, r.n_cigar * 4u);
  }
  std::unique_ptr<gtx_disc_event[]> events(event_cap ? new gtx_disc_event[event_cap] : nullptr);
  std::unique_ptr<gtx_disc_read_out[]> read_out(new gtx_disc_read_out[n_reads]);
  std::unique_ptr<uint32_t[]> counts(new uint32_t[2]);
  if (event_cap)
    std::memset(events.get(), 0xA5, static_cast<size_t>(event_cap) * sizeof(gtx_disc_event));
  std::memset(read_out.get(), 0xA5, static_cast<size_t>(n_reads) * sizeof(gtx_disc_read_out));
  counts[0] = h[6];
  counts[1] = h[7];
  HeapBatch const batch{refp.get(), ref_groups, static_cast<long>(reference_len), static_cast<long>(region_begin), plane_stride, reads.data(), n_reads,
                        events.get(), event_cap, counts.get(), read_out.get(), &rows, &quals, &cigars};
  for (uint32_t launch = 0; launch < launches; ++launch)
    for (uint32_t first = 0; first < n_reads; first += 64)
      disc_events_wave<WaveSeq>(batch, first);
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(counts.get(), 4, 2, o) != 2 || (n_reads && std::fwrite(read_out.get(), sizeof(gtx_disc_read_out), n_reads, o) != n_reads) ||
      (event_cap && std::fwrite(events.get(), sizeof(gtx_disc_event), event_cap, o) != event_cap))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
