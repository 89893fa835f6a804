// Host emulation of gtx_disc_second_intake and gtx_disc_second_candidates (gtx_disc_second.hip): the reads of a file, 64 at a
// time, and the rounds of a list slice, one wave each, through the kernels' source (gtx_disc_second_dev.hpp) over a sequential
// wave, built with AddressSanitizer / UBSan.
//   emu_disc_second case.bin out.bin
// case.bin: uint32 plane_stride, n_reads, n_cigar, reference_len, bucket_size, n_table, n_table_seq, launches, n_list, k0, k1,
// n_events, pair_cap, counts[0], counts[1], given_state; int64 region_begin; the region's bytes; n_reads plane rows; n_reads
// gtx_disc_read; n_cigar cigar words; n_table gtx_disc_indel; n_table_seq letters; n_list list entries; n_events
// gtx_disc_second_event; and, with given_state != 0, n_reads gtx_disc_second_read: the reads' current state for the rounds (else
// the rounds see what the intake left).
// out.bin: n_reads gtx_disc_second_read, n_buckets int32 max_pos_end, n_buckets int32 global_max_pos_end, max_read_size,
// n_reads grouped stream indices, n_buckets + 1 offsets, (n_table + 31) / 32 found words, the two counters, pair_cap pairs.
// Every output is filled with 0xA5 before the first launch.  Every read runs over heap blocks of exactly its sizes -- the plane
// groups of its row, n_cigar words --, the region's planes are sized as gtx_disc_create sizes them, and every other array is a
// heap block of exactly its number of entries (none: a null pointer): a load or a store the kernels' bounds should have
// prevented stops the program.  What rocPRIM does on the device between the kernels -- the running maximum in stream order, the
// stable sort of the stream indices by bucket, the exclusive sum of the rounds' counts -- is done here with the standard library.
// `launches` > 1 repeats the intake and the rounds over the same buffers (the counters then accumulate).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_disc_second_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
// the file as the intake's text asks for it, a heap block per read and array
struct HeapBatch
{
  uint32_t const * ref5;
  uint32_t ref_groups;
  char const * refc;
  long REF_SIZE, region_begin, bucket_size;
  uint32_t n_buckets, plane_stride;
  gtx_disc_read const * reads;
  uint32_t n_reads;
  gtx_disc_indel const * table;
  char const * table_seq;
  uint32_t n_table;
  uint64_t n_table_seq;
  gtx_disc_second_read * out;
  int32_t * bucket_max;
  uint32_t *max_read_size, *found, *key, *index, *end_clip;
  std::vector<std::unique_ptr<uint32_t[]>> const * rows;
  std::vector<std::unique_ptr<uint32_t[]>> const * cigars;
  gtx_disc_read read(uint32_t i) const { return reads[i]; }
  uint32_t const * row_of(uint32_t i) const { return (*rows)[i].get(); }
  uint32_t const * cigar_of(uint32_t i, gtx_disc_read const &) const { return (*cigars)[i].get(); }
};

template <class T>
std::unique_ptr<T[]> block(size_t n)
{
  std::unique_ptr<T[]> p(n ? new T[n] : nullptr);
  if (n)
    std::memset(static_cast<void *>(p.get()), 0xA5, n * sizeof(T));
  return p;
}

bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

template <class T>
bool load(std::FILE * f, std::unique_ptr<T[]> & p, size_t n)
{
  p = block<T>(n);
  return read_exact(f, p.get(), n * sizeof(T));
}

template <class T>
bool store(std::FILE * f, std::unique_ptr<T[]> const & p, size_t n)
{
  return n == 0 || std::fwrite(p.get(), sizeof(T), n, f) == n;
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_disc_second case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[16];
  int64_t region_begin = 0;
  if (!f || !read_exact(f, h, sizeof h) || !read_exact(f, &region_begin, 8))
    return 2;
  uint32_t const plane_stride = h[0], n_reads = h[1], n_cigar = h[2], reference_len = h[3], bucket_size = h[4], n_table = h[5], n_table_seq = h[6], launches = h[7],
                 n_list = h[8], k0 = h[9], k1 = h[10], n_events = h[11], pair_cap = h[12], given_state = h[15];
  if (plane_stride == 0 || plane_stride % PLANE_GROUP_BYTES || reference_len == 0 || bucket_size == 0 || k1 < k0 || k1 > n_list)
    return 2;
  std::unique_ptr<char[]> reference, table_seq;
  std::vector<uint32_t> planes(static_cast<size_t>(n_reads) * plane_stride / 4u), cigar(n_cigar);
  std::unique_ptr<gtx_disc_read[]> reads;
  std::unique_ptr<gtx_disc_indel[]> table;
  std::unique_ptr<uint32_t[]> list;
  std::unique_ptr<gtx_disc_second_event[]> events;
  std::unique_ptr<gtx_disc_second_read[]> state;
  if (!load(f, reference, reference_len) || !read_exact(f, planes.data(), planes.size() * 4u) || !load(f, reads, n_reads) || !read_exact(f, cigar.data(), cigar.size() * 4u) ||
      !load(f, table, n_table) || !load(f, table_seq, n_table_seq) || !load(f, list, n_list) || !load(f, events, n_events) ||
      (given_state && !load(f, state, n_reads)))
    return 2;
  std::fclose(f);
  uint32_t const ref_groups = disc_ref_groups(reference_len);
  std::unique_ptr<uint32_t[]> ref5(new uint32_t[static_cast<size_t>(ref_groups) * disc_second_dev::REF_PLANES]());
  disc_second_ref_planes(reference.get(), reference_len, ref5.get());
  std::vector<std::unique_ptr<uint32_t[]>> rows(n_reads), cigars(n_reads);
  for (uint32_t i = 0; i < n_reads; ++i)
  {
    gtx_disc_read const & r = reads[i];
    if (static_cast<uint64_t>(r.cigar_off) + r.n_cigar > n_cigar)
      return 2;
    rows[i].reset(new uint32_t[plane_stride / 4u]);
    std::memcpy(rows[i].get(), planes.data() + static_cast<size_t>(i) * plane_stride / 4u, plane_stride);
    cigars[i].reset(new uint32_t[r.n_cigar]);
    std::memcpy(cigars[i].get(), cigar.data() + r.cigar_off, r.n_cigar * 4u);
  }
  long const REF_SIZE = reference_len;
  uint32_t const n_buckets = disc_second_buckets(REF_SIZE, bucket_size), found_words = (n_table + 31u) / 32u, m = k1 - k0;
  auto second = block<gtx_disc_second_read>(n_reads);
  auto bucket_max = block<int32_t>(n_buckets), bucket_global_max = block<int32_t>(n_buckets);
  auto max_read_size = block<uint32_t>(1), bucket_reads = block<uint32_t>(n_reads), bucket_off = block<uint32_t>(n_buckets + 1u), found = block<uint32_t>(found_words);
  auto counts = block<uint32_t>(2);
  auto pairs = block<gtx_disc_second_pair>(pair_cap);
  auto key = block<uint32_t>(n_reads), index = block<uint32_t>(n_reads), end_clip = block<uint32_t>(n_reads), run_max = block<uint32_t>(n_reads),
       sorted_key = block<uint32_t>(n_reads);
  auto n_of = block<uint32_t>(m + 1u), off = block<uint32_t>(m + 1u);
  counts[0] = h[13];
  counts[1] = h[14];
  HeapBatch const batch{ref5.get(), ref_groups, reference.get(), REF_SIZE, static_cast<long>(region_begin), static_cast<long>(bucket_size), n_buckets, plane_stride,
                        reads.get(), n_reads, table.get(), table_seq.get(), n_table, n_table_seq, second.get(), bucket_max.get(), max_read_size.get(), found.get(),
                        key.get(), index.get(), end_clip.get(), &rows, &cigars};
  for (uint32_t launch = 0; launch < launches; ++launch)
  {
    if (n_reads) // (gtx_disc_second_intake with no reads writes nothing)
    {
      for (uint32_t i = 0; i < std::max(n_buckets, found_words); ++i)
        disc_second_init(i, bucket_max.get(), n_buckets, found.get(), found_words, max_read_size.get());
      for (uint32_t first = 0; first < n_reads; first += 64)
        disc_second_intake_wave<WaveSeq>(batch, first);
      // rocPRIM's part: the running maximum in stream order, the stable sort by bucket
      uint32_t running = 0;
      for (uint32_t i = 0; i < n_reads; ++i)
        run_max[i] = running = std::max(running, end_clip[i]);
      std::vector<uint32_t> order(n_reads);
      std::iota(order.begin(), order.end(), 0u);
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
      for (uint32_t j = 0; j < n_reads; ++j)
      {
        sorted_key[j] = key[order[j]];
        bucket_reads[j] = index[order[j]];
      }
      for (uint32_t b = 0; b <= n_buckets; ++b)
        disc_second_bucket(b, n_buckets, sorted_key.get(), bucket_reads.get(), n_reads, run_max.get(), bucket_off.get(), bucket_global_max.get());
    }
    if (m)
    {
      SecondRound const round{list.get(), table.get(), n_table, given_state ? state.get() : second.get(), n_reads, events.get(), n_events,
                              static_cast<long>(region_begin), REF_SIZE, static_cast<long>(bucket_size), n_buckets, bucket_max.get(), bucket_global_max.get(),
                              max_read_size.get(), bucket_reads.get(), bucket_off.get(), pairs.get(), pair_cap};
      for (uint32_t w = 0; w < m; ++w)
        n_of[w] = disc_second_round_wave<WaveSeq, false>(round, k0 + w, 0);
      n_of[m] = 0;
      uint32_t sum = 0; // rocPRIM's part: the exclusive sum
      for (uint32_t w = 0; w <= m; ++w)
      {
        off[w] = sum;
        sum += n_of[w];
      }
      for (uint32_t w = 0; w < m; ++w)
        (void)disc_second_round_wave<WaveSeq, true>(round, k0 + w, counts[0] + off[w]);
      disc_second_count(counts.get(), off[m], pair_cap);
    }
  }
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || !store(o, second, n_reads) || !store(o, bucket_max, n_buckets) || !store(o, bucket_global_max, n_buckets) || !store(o, max_read_size, 1) ||
      !store(o, bucket_reads, n_reads) || !store(o, bucket_off, n_buckets + 1u) || !store(o, found, found_words) || !store(o, counts, 2) ||
      !store(o, pairs, pair_cap))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
