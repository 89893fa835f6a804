// Host emulation of gtx_disc_second_rounds (gtx_disc_rounds.hip): the rounds of a list slice through the kernels' source
// (gtx_disc_rounds_dev.hpp, with gtx_disc_second_dev.hpp for a round's pairs and gtx_realign_dev.hpp for the alignments) over a
// sequential wave, built with AddressSanitizer / UBSan.
//   emu_disc_rounds case.bin out.bin
// case.bin: uint32 plane_stride, n_reads, reference_len, bucket_size, n_table, n_table_seq, n_list, k0, k1, event_cap, n_events (in
// use); int64 region_begin; the region's bytes; n_reads plane rows; n_reads gtx_disc_second_read (as the intake left them); n_table
// gtx_disc_indel; n_table_seq letters; n_list list entries; event_cap gtx_disc_second_event; n_buckets int32 max_pos_end; n_buckets
// int32 global_max_pos_end; max_read_size; n_reads grouped stream indices; n_buckets + 1 offsets; n_table gtx_disc_second_support.
// out.bin: uint32 status (0, or 5: the event array is too small), n_events, rounds_done, rounds_skipped, pairs_aligned,
// pairs_refused, windows_built, compactions, events_wanted; n_reads gtx_disc_second_read; event_cap gtx_disc_second_event; n_table
// gtx_disc_second_support; then per window built, in the order of the rounds and the slots: uint32 k, read (0xFFFFFFFF: the plain
// window), n, n_entries, the W::mem_sync() calls of its build (a sequential wave cannot see what they order, it can count them); n letters; n int32 ref_pos values; n_entries applied flags.
// A case.bin whose first word is 0xFFFFFFFF asks for the final decision instead: n_table (the fifth word) gtx_disc_indel and as many
// gtx_disc_second_support follow the header; out.bin: per entry two bytes, disc_second_good_count and disc_second_good of the entry and its
// counters.
// Every array is a heap block of exactly its number of entries, the arena of a round exactly the sum of its slots: a load or a
// store the kernels' bounds should have prevented stops the program.  The host's part -- the exclusive sums, the order of the
// steps, the compaction's copy back -- is restated here with the standard library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_disc_rounds_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
// the sequential wave with the count of W::mem_sync() calls this program writes out per window
struct WaveSeqCounted : WaveSeq
{
  static inline uint64_t syncs = 0;
  static void mem_sync() { ++syncs; }
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
bool store(std::FILE * f, T const * p, size_t n)
{
  return n == 0 || std::fwrite(p, sizeof(T), n, f) == n;
}

void exclusive_sum(uint32_t const * in, uint32_t * out, size_t n)
{
  uint32_t sum = 0;
  for (size_t i = 0; i < n; ++i)
  {
    uint32_t const v = in[i];
    out[i] = sum;
    sum += v;
  }
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_disc_rounds case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[11];
  int64_t region_begin = 0;
  if (!f || !read_exact(f, h, sizeof h) || !read_exact(f, &region_begin, 8))
    return 2;
  if (h[0] == 0xFFFFFFFFu) // the final decision on counters of the caller's
  {
    uint32_t const n = h[4];
    std::unique_ptr<gtx_disc_indel[]> entries;
    std::unique_ptr<gtx_disc_second_support[]> counters;
    if (!load(f, entries, n) || !load(f, counters, n))
      return 2;
    std::fclose(f);
    auto good = block<uint8_t>(2 * static_cast<size_t>(n));
    for (uint32_t t = 0; t < n; ++t)
    {
      good[2 * t] = disc_second_good_count(entries[t], counters[t]) ? 1 : 0;
      good[2 * t + 1] = disc_second_good(entries[t], counters[t]) ? 1 : 0;
    }
    std::FILE * const o = std::fopen(argv[2], "wb");
    if (!o || !store(o, good.get(), 2 * static_cast<size_t>(n)))
      return 2;
    return std::fclose(o) == 0 ? 0 : 2;
  }
  uint32_t const plane_stride = h[0], n_reads = h[1], reference_len = h[2], bucket_size = h[3], n_table = h[4], n_table_seq = h[5], n_list = h[6], k0 = h[7], k1 = h[8],
                 event_cap = h[9];
  uint32_t count = h[10];
  if (plane_stride == 0 || plane_stride % PLANE_GROUP_BYTES || reference_len == 0 || bucket_size == 0 || k1 < k0 || k1 > n_list || count > event_cap || n_reads == 0)
    return 2;
  long const REF_SIZE = reference_len;
  uint32_t const n_buckets = disc_second_buckets(REF_SIZE, bucket_size);
  std::unique_ptr<char[]> reference, table_seq;
  std::unique_ptr<uint8_t[]> planes;
  std::unique_ptr<gtx_disc_second_read[]> second;
  std::unique_ptr<gtx_disc_indel[]> table;
  std::unique_ptr<uint32_t[]> list, max_read_size, bucket_reads, bucket_off;
  std::unique_ptr<gtx_disc_second_event[]> events;
  std::unique_ptr<int32_t[]> bucket_max, bucket_global_max;
  std::unique_ptr<gtx_disc_second_support[]> support;
  if (!load(f, reference, reference_len) || !load(f, planes, static_cast<size_t>(n_reads) * plane_stride) || !load(f, second, n_reads) || !load(f, table, n_table) ||
      !load(f, table_seq, n_table_seq) || !load(f, list, n_list) || !load(f, events, event_cap) || !load(f, bucket_max, n_buckets) ||
      !load(f, bucket_global_max, n_buckets) || !load(f, max_read_size, 1) || !load(f, bucket_reads, n_reads) || !load(f, bucket_off, n_buckets + 1u) ||
      !load(f, support, n_table))
    return 2;
  std::fclose(f);
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;
  std::vector<uint8_t> windows; // the dump behind the arrays

  size_t const slots = static_cast<size_t>(n_reads) + 2;
  auto pairs = block<gtx_disc_second_pair>(n_reads);
  auto counts = block<uint32_t>(2), ctl = block<uint32_t>(ROUNDS_CTL_WORDS + 1u), ub = block<uint32_t>(slots), woff = block<uint32_t>(slots), wlen = block<uint32_t>(slots),
       target_off = block<uint32_t>(2 * slots + 1), newn = block<uint32_t>(slots), noff = block<uint32_t>(slots);
  auto rpairs = block<RealignPair>(n_reads);
  auto results = block<RealignResult>(n_reads);
  auto decisions = block<RoundDecision>(n_reads);
  auto lens = block<uint16_t>(n_reads);
  auto applied = block<uint8_t>(event_cap);
  std::memset(ctl.get(), 0, (ROUNDS_CTL_WORDS + 1u) * 4u);
  for (uint32_t i = 0; i < n_reads; ++i)
    rounds_begin(i, second.get(), n_reads, count, lens.get(), ctl.get());
  if (ctl[ROUNDS_BAD_LIST])
    return 2;

  RoundsIn in{};
  in.refc = reference.get();
  in.REF_SIZE = REF_SIZE;
  in.region_begin = static_cast<long>(region_begin);
  in.table = table.get();
  in.table_seq = table_seq.get();
  in.n_table = n_table;
  in.n_table_seq = n_table_seq;
  in.list = list.get();
  in.max_read_size = max_read_size.get();
  in.reads = second.get();
  in.n_reads = n_reads;
  in.events = events.get();
  in.support = support.get();
  in.pairs = pairs.get();
  in.counts = counts.get();
  in.ub = ub.get();
  in.woff = woff.get();
  in.wlen = wlen.get();
  in.target_off = target_off.get();
  in.rpairs = rpairs.get();
  in.results = results.get();
  in.applied = applied.get();
  in.decisions = decisions.get();
  in.newn = newn.get();
  in.noff = noff.get();
  in.ctl = ctl.get();
  uint32_t status = 0, rounds_done = 0, skipped = 0, aligned = 0, refused = 0, built = 0, compactions = 0, wanted = 0;
  for (uint32_t k = k0; k < k1; ++k)
  {
    in.k = k;
    in.n_events = count;
    counts[0] = counts[1] = 0;
    std::memset(ctl.get(), 0, ROUNDS_CTL_WORDS * 4u);
    SecondRound const round{list.get(), table.get(), n_table, second.get(), n_reads, events.get(), count, static_cast<long>(region_begin), REF_SIZE,
                            static_cast<long>(bucket_size), n_buckets, bucket_max.get(), bucket_global_max.get(), max_read_size.get(), bucket_reads.get(),
                            bucket_off.get(), pairs.get(), n_reads};
    uint32_t const produced = disc_second_round_wave<WaveSeqCounted, true>(round, k, 0);
    disc_second_count(counts.get(), produced, n_reads);
    for (uint32_t i = 0; i < slots; ++i)
      rounds_prepare<WaveSeqCounted>(in, i);
    exclusive_sum(ub.get(), woff.get(), slots);
    uint32_t const n_pairs = ctl[ROUNDS_N_PAIRS];
    uint64_t const letters = (static_cast<uint64_t>(ctl[ROUNDS_LETTERS_HI]) << 32) | ctl[ROUNDS_LETTERS_LO];
    if (letters >= 0x80000000ull)
    {
      status = 5;
      break;
    }
    if (static_cast<uint64_t>(count) + ctl[ROUNDS_NEED_UPPER] > event_cap)
    {
      auto tmp = block<gtx_disc_second_event>(event_cap);
      for (uint32_t i = 0; i <= n_reads; ++i)
        newn[i] = i < n_reads ? second[i].n_events : 0u;
      exclusive_sum(newn.get(), noff.get(), static_cast<size_t>(n_reads) + 1);
      for (uint32_t i = 0; i < n_reads; ++i)
        rounds_compact_copy(i, second.get(), n_reads, events.get(), noff.get(), tmp.get(), event_cap);
      for (uint32_t i = 0; i < n_reads; ++i)
        rounds_compact_place(i, second.get(), n_reads, noff.get());
      uint32_t const live = noff[n_reads];
      if (live > count)
        return 2;
      std::copy(tmp.get(), tmp.get() + live, events.get());
      count = live;
      in.n_events = count;
      ++compactions;
    }
    auto arena_seq = block<uint8_t>(letters);
    auto arena_pos = block<int32_t>(letters);
    in.seq = arena_seq.get();
    in.refpos = arena_pos.get();
    std::vector<uint32_t> syncs(static_cast<size_t>(n_pairs) + 1);
    for (uint32_t slot = 0; slot <= n_pairs; ++slot)
    {
      uint64_t const before = WaveSeqCounted::syncs;
      rounds_window_wave<WaveSeqCounted>(in, slot);
      syncs[slot] = static_cast<uint32_t>(WaveSeqCounted::syncs - before);
    }
    for (uint32_t slot = 0; slot <= n_pairs; ++slot)
    {
      gtx_disc_second_read const * const r = slot ? &second[pairs[slot - 1].read] : nullptr;
      if (slot != 0 && r->n_events == 0) // (a skipped round's windows are dumped too: the aligner is handed them all the same)
        continue;
      uint32_t const head[5] = {k, slot ? pairs[slot - 1].read : 0xFFFFFFFFu, wlen[slot], r ? r->n_events : 0u, syncs[slot]};
      auto put = [&](void const * p, size_t n) { windows.insert(windows.end(), static_cast<uint8_t const *>(p), static_cast<uint8_t const *>(p) + n); };
      put(head, sizeof head);
      put(in.seq + woff[slot], wlen[slot]);
      put(in.refpos + woff[slot], static_cast<size_t>(wlen[slot]) * 4u);
      if (r)
        put(applied.get() + r->first_event, r->n_events);
    }
    for (uint32_t j = 0; j < n_pairs; ++j)
      realign_pair_dev<WaveSeqCounted>(planes.get(), plane_stride, lens.get(), n_reads, in.seq, target_off.get(), 2 * (n_pairs + 1), rpairs[j], &results[j]);
    for (uint32_t j = 0; j <= n_reads; ++j)
      rounds_decide<WaveSeqCounted>(in, j);
    exclusive_sum(newn.get(), noff.get(), static_cast<size_t>(n_reads) + 1);
    uint32_t const total = noff[n_reads];
    if (static_cast<uint64_t>(count) + total > event_cap)
    {
      status = 5;
      wanted = count + total;
      break;
    }
    for (uint32_t j = 0; j < n_pairs; ++j)
      rounds_apply<WaveSeqCounted>(in, j, count, event_cap);
    count += total;
    ++rounds_done;
    built += ctl[ROUNDS_WINDOWS];
    if (ctl[ROUNDS_SKIPPED])
      ++skipped;
    else
    {
      aligned += ctl[ROUNDS_ALIGNED];
      refused += ctl[ROUNDS_REFUSED];
    }
  }
  uint32_t const head[9] = {status, count, rounds_done, skipped, aligned, refused, built, compactions, wanted};
  if (!store(o, head, 9) || !store(o, second.get(), n_reads) || !store(o, events.get(), event_cap) || !store(o, support.get(), n_table) ||
      !store(o, windows.data(), windows.size()))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
