// gtx_disc_second.hip -- discovery's second pass up to the aligner (parallel_second_pass, src/typer/caller.cpp:2633-2751): the
// entry points around the kernel text of gtx_disc_second_dev.hpp.
//
// Host: gtx_disc_indel_table reads the indel table off the words of gtx_disc_merge, gtx_disc_second_plan makes a file's list
// (:2641-2735).  Device: gtx_disc_second_intake -- one read per lane through the intake walk, atomic maxima into the buckets, a
// running maximum in stream order (rocPRIM inclusive scan) and a stable sort of the stream indices by bucket, then one lane per
// bucket for its offset and its global maximum; gtx_disc_second_candidates -- one wavefront per list entry over its bucket range,
// counted first, emitted behind an exclusive scan of the counts, so that the pairs lie in the reference's order of visit
// whatever the scheduling.  The driver that feeds a read's new state into the next round is gtx_disc_rounds.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_devmem.hpp"
#include "gtx_devprim.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_second_dev.hpp"
#include "wave_hip.hpp"

namespace
{
using namespace gtx;

constexpr char const * MSG_PREFIX = "gtx_disc_second: ";
constexpr uint32_t TB = 256;
uint32_t blocks(uint64_t n) { return static_cast<uint32_t>((n + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void gtx_disc_second_init_kernel(int32_t * __restrict__ bucket_max, uint32_t n_buckets, uint32_t * __restrict__ found,
                                                                  uint32_t found_words, uint32_t * __restrict__ max_read_size)
{
  disc_second_init(blockIdx.x * blockDim.x + threadIdx.x, bucket_max, n_buckets, found, found_words, max_read_size);
}

__global__ __launch_bounds__(TB) void gtx_disc_second_intake_kernel(SecondBatch in)
{
  disc_second_intake_wave<WaveHip>(in, blockIdx.x * blockDim.x + (threadIdx.x & ~63u));
}

__global__ __launch_bounds__(TB) void gtx_disc_second_buckets_kernel(uint32_t n_buckets, uint32_t const * __restrict__ sorted_key,
                                                                     uint32_t const * __restrict__ sorted_index, uint32_t n_reads,
                                                                     uint32_t const * __restrict__ run_max, uint32_t * __restrict__ bucket_off,
                                                                     int32_t * __restrict__ bucket_global_max)
{
  uint32_t const b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= n_buckets)
    disc_second_bucket(b, n_buckets, sorted_key, sorted_index, n_reads, run_max, bucket_off, bucket_global_max);
}

// one wavefront per list entry; n_of[m] = 0 closes the array the scan runs over
__global__ __launch_bounds__(TB) void gtx_disc_second_count_kernel(SecondRound in, uint32_t k0, uint32_t m, uint32_t * __restrict__ n_of)
{
  uint32_t const w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w > m)
    return;
  uint32_t const n = w < m ? disc_second_round_wave<WaveHip, false>(in, k0 + w, 0) : 0;
  if (WaveHip::leader())
    n_of[w] = n;
}

__global__ __launch_bounds__(TB) void gtx_disc_second_emit_kernel(SecondRound in, uint32_t k0, uint32_t m, uint32_t const * __restrict__ off,
                                                                  uint32_t const * __restrict__ counts)
{
  uint32_t const w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= m)
    return;
  (void)disc_second_round_wave<WaveHip, true>(in, k0 + w, counts[0] + off[w]);
}

__global__ void gtx_disc_second_count_finish_kernel(uint32_t * counts, uint32_t const * __restrict__ off, uint32_t m, uint32_t pair_cap)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    disc_second_count(counts, off[m], pair_cap);
}

bool launched() { return hip_ok(hipGetLastError(), "kernel launch", MSG_PREFIX); }
bool aligned4(void const * p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int bad(char const * name)
{
  g_last_error = std::string(name) + ": bad argument";
  return GTX_ERR_ARG;
}
} // namespace

// ---- host: the table and the list ---------------------------------------------------------------------------------------------
extern "C" int gtx_disc_indel_table(const uint32_t * words, uint64_t n_words, gtx_disc_indel * entries, uint32_t cap, uint32_t * n, char * seq,
                                    uint64_t seq_cap, uint64_t * n_seq)
{
  if (!n || !n_seq || (n_words && !words) || (cap && !entries) || (seq_cap && !seq))
    return bad("gtx_disc_indel_table");
  *n = 0;
  *n_seq = 0;
  if (n_words == 0)
    return GTX_OK;
  // the words of a file's result (gtx.h: gtx_disc_first_pass_haplotypes): n_indels, per indel pos, type, length, its letters, 15
  // support fields (the 12th the span, the 14th has_indel_good_support), file_index, the phase entries
  std::vector<gtx_disc_indel> table;
  std::string letters;
  uint64_t at = 1;
  uint32_t const n_indels = words[0];
  for (uint32_t i = 0; i < n_indels; ++i)
  {
    if (at + 3 > n_words || words[at + 2] > n_words - at - 3)
      return bad("gtx_disc_indel_table: the words do not parse");
    gtx_disc_indel e{};
    e.pos = words[at];
    e.type = static_cast<uint8_t>(words[at + 1]);
    e.len = words[at + 2];
    e.seq_off = static_cast<uint32_t>(letters.size());
    for (uint32_t k = 0; k < e.len; ++k)
      letters.push_back(static_cast<char>(words[at + 3 + k]));
    at += 3 + e.len;
    if (at + 17 > n_words)
      return bad("gtx_disc_indel_table: the words do not parse");
    e.span = static_cast<uint16_t>(words[at + 11]);
    e.good = words[at + 13] != 0;
    e.file_index = static_cast<int32_t>(words[at + 15]);
    uint32_t const n_phase = words[at + 16];
    at += 17;
    for (uint32_t k = 0; k < n_phase; ++k)
    {
      if (at + 3 > n_words || words[at + 2] > n_words - at - 3 || at + 3 + words[at + 2] + 1 > n_words)
        return bad("gtx_disc_indel_table: the words do not parse");
      at += 3 + words[at + 2] + 1;
    }
    if (letters.size() > 0xFFFFFFFFull)
      return bad("gtx_disc_indel_table: more than 2^32 letters");
    table.push_back(e);
  }
  *n = static_cast<uint32_t>(table.size());
  *n_seq = letters.size();
  if (table.size() > cap || letters.size() > seq_cap)
    return GTX_ERR_CAPACITY;
  std::copy(table.begin(), table.end(), entries);
  std::copy(letters.begin(), letters.end(), seq);
  return GTX_OK;
}

extern "C" int gtx_disc_indel_table_upload(const gtx_disc * d, const gtx_disc_indel * entries, uint32_t n, const char * seq, uint64_t n_seq,
                                           gtx_disc_indel * d_entries, char * d_seq, void * stream)
{
  if (!d || (n && (!entries || !d_entries)) || (n_seq && (!seq || !d_seq)) || !aligned4(d_entries))
    return bad("gtx_disc_indel_table_upload");
  if (int const rc = device_ready(d->device, "gtx_disc_indel_table_upload", ": the object"))
    return rc;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  if ((n && !hip_ok(hipMemcpyAsync(d_entries, entries, static_cast<size_t>(n) * sizeof(gtx_disc_indel), hipMemcpyHostToDevice, s), "copy", MSG_PREFIX)) ||
      (n_seq && !hip_ok(hipMemcpyAsync(d_seq, seq, n_seq, hipMemcpyHostToDevice, s), "copy", MSG_PREFIX)) ||
      !hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX))
    return GTX_ERR_HIP;
  return GTX_OK;
}

extern "C" int gtx_disc_second_plan(const gtx_disc_indel * entries, uint32_t n, const uint32_t * found, int32_t file_index, uint32_t * list, uint32_t cap,
                                    uint32_t * n_list)
{
  if (!n_list || (n && (!entries || !found)) || (cap && !list))
    return bad("gtx_disc_second_plan");
  long constexpr NEARBY_BP = 60; // :2685
  *n_list = 0;
  // :2918-2946 the file's own indels: no good support, and the best support came from this file
  std::vector<uint32_t> own, chosen;
  for (uint32_t t = 0; t < n; ++t)
    if (!entries[t].good && entries[t].file_index == file_index)
      own.push_back(t);
  if (own.empty()) // :2641
    return GTX_OK;
  std::vector<uint8_t> in_list(n, 0);
  for (uint32_t t : own)
    in_list[t] = 1;
  for (uint32_t o : own) // :2687-2718
  {
    long const p = entries[o].pos;
    for (uint32_t t = 0; t < n; ++t)
    {
      if (t == o || !entries[t].good)
        continue;
      long const pos = entries[t].pos;
      bool const near = t < o ? pos + NEARBY_BP >= p : pos - NEARBY_BP <= p; // :2696, :2709
      if (near && ((found[t >> 5] >> (t & 31u)) & 1u) != 0) // :2699, :2712 it also needs to be found in the file
        in_list[t] = 1;
    }
  }
  for (uint32_t t = 0; t < n; ++t)
    if (in_list[t])
      chosen.push_back(t);
  // :2728-2735 good indels first, by position within each class; this library's rule: every indel once, ties in table order
  std::stable_sort(chosen.begin(), chosen.end(), [&](uint32_t a, uint32_t b) {
    if (entries[a].good != entries[b].good)
      return entries[a].good > entries[b].good;
    return entries[a].pos < entries[b].pos;
  });
  *n_list = static_cast<uint32_t>(chosen.size());
  if (chosen.size() > cap)
    return GTX_ERR_CAPACITY;
  std::copy(chosen.begin(), chosen.end(), list);
  return GTX_OK;
}

// ---- device -------------------------------------------------------------------------------------------------------------------
extern "C" int gtx_disc_second_intake(gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads, const uint32_t * d_cigar,
                                      uint32_t n_reads, uint32_t bucket_size, const gtx_disc_indel * d_table, const char * d_table_seq, uint32_t n_table,
                                      uint64_t n_table_seq, gtx_disc_second_read * d_second, int32_t * d_bucket_max, int32_t * d_bucket_global_max,
                                      uint32_t * d_max_read_size, uint32_t * d_bucket_reads, uint32_t * d_bucket_off, uint32_t * d_found, void * stream)
{
  if (!d || bucket_size == 0 || plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0 || !aligned4(d_planes) || !aligned4(d_reads) || !aligned4(d_cigar) ||
      !aligned4(d_table) || !aligned4(d_second) || !aligned4(d_bucket_max) || !aligned4(d_bucket_global_max) || !aligned4(d_max_read_size) ||
      !aligned4(d_bucket_reads) || !aligned4(d_bucket_off) || !aligned4(d_found) || n_reads == 0xFFFFFFFFu || (n_table && (!d_table || !d_found)) ||
      (n_table_seq && !d_table_seq) ||
      (n_reads != 0 && (!d_planes || !d_reads || !d_cigar || !d_second || !d_bucket_max || !d_bucket_global_max || !d_max_read_size || !d_bucket_reads ||
                        !d_bucket_off)))
    return bad("gtx_disc_second_intake");
  if (int const rc = device_ready(d->device, "gtx_disc_second_intake", ": the object"))
    return rc;
  if (n_reads == 0)
    return GTX_OK;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  long const REF_SIZE = static_cast<long>(d->reference.size());
  uint32_t const n_buckets = disc_second_buckets(REF_SIZE, bucket_size), found_words = (n_table + 31u) / 32u;
  TempPool pool(s, MSG_PREFIX);
  uint32_t * key = pool.get<uint32_t>(n_reads, "bucket keys");
  uint32_t * index = pool.get<uint32_t>(n_reads, "stream indices");
  uint32_t * end_clip = pool.get<uint32_t>(n_reads, "ends with clip");
  uint32_t * run_max = pool.get<uint32_t>(n_reads, "running maximum");
  uint32_t * sorted_key = pool.get<uint32_t>(n_reads, "sorted bucket keys");
  if (!pool.fine)
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_second_init_kernel, dim3(blocks(std::max<uint32_t>(std::max(n_buckets, found_words), 1u))), dim3(TB), 0, s, d_bucket_max, n_buckets,
                     d_found, found_words, d_max_read_size);
  SecondBatch const in{d->d_ref5.get(), d->ref_groups, reinterpret_cast<char const *>(d->d_refc.get()), REF_SIZE, static_cast<long>(d->region_begin),
                       static_cast<long>(bucket_size), n_buckets, d_planes, plane_stride, d_reads, d_cigar, n_reads, d_table, d_table_seq, n_table, n_table_seq,
                       d_second, d_bucket_max, d_max_read_size, d_found, key, index, end_clip};
  hipLaunchKernelGGL(gtx_disc_second_intake_kernel, dim3(blocks(n_reads)), dim3(TB), 0, s, in);
  if (!launched())
    return GTX_ERR_HIP;
  // the running maximum in stream order; the stream indices grouped by bucket (a stable sort: stream order within a bucket)
  unsigned bits = 1;
  while ((1ull << bits) <= n_buckets)
    ++bits;
  if (!inclusive_scan(pool, end_clip, run_max, n_reads, rocprim::maximum<uint32_t>(), "scan", "scan temporary") ||
      !sort_pairs(pool, key, sorted_key, index, d_bucket_reads, n_reads, bits, "radix sort", "sort temporary"))
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_second_buckets_kernel, dim3(blocks(static_cast<uint64_t>(n_buckets) + 1)), dim3(TB), 0, s, n_buckets, sorted_key, d_bucket_reads,
                     n_reads, run_max, d_bucket_off, d_bucket_global_max);
  return launched() ? GTX_OK : GTX_ERR_HIP; // (the pool waits for the stream before its blocks go back)
}

extern "C" int gtx_disc_second_candidates(gtx_disc * d, const uint32_t * d_list, uint32_t k0, uint32_t k1, const gtx_disc_indel * d_table, uint32_t n_table,
                                          const gtx_disc_second_read * d_second, uint32_t n_reads, const gtx_disc_second_event * d_events, uint32_t n_events,
                                          uint32_t bucket_size, const int32_t * d_bucket_max, const int32_t * d_bucket_global_max,
                                          const uint32_t * d_max_read_size, const uint32_t * d_bucket_reads, const uint32_t * d_bucket_off,
                                          gtx_disc_second_pair * d_pairs, uint32_t pair_cap, uint32_t * d_counts, void * stream)
{
  bool const work = k1 > k0;
  if (!d || bucket_size == 0 || k1 < k0 || !aligned4(d_list) || !aligned4(d_table) || !aligned4(d_second) || !aligned4(d_events) || !aligned4(d_bucket_max) ||
      !aligned4(d_bucket_global_max) || !aligned4(d_max_read_size) || !aligned4(d_bucket_reads) || !aligned4(d_bucket_off) || !aligned4(d_pairs) ||
      !aligned4(d_counts) || (n_events && !d_events) || (pair_cap && !d_pairs) ||
      (work && (!d_list || !d_table || !d_counts || !d_bucket_max || !d_bucket_global_max || !d_max_read_size || !d_bucket_off ||
                (n_reads && (!d_second || !d_bucket_reads)))))
    return bad("gtx_disc_second_candidates");
  if (int const rc = device_ready(d->device, "gtx_disc_second_candidates", ": the object"))
    return rc;
  if (!work)
    return GTX_OK;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  long const REF_SIZE = static_cast<long>(d->reference.size());
  uint32_t const m = k1 - k0;
  TempPool pool(s, MSG_PREFIX);
  uint32_t * n_of = pool.get<uint32_t>(static_cast<size_t>(m) + 1, "pairs per entry");
  uint32_t * off = pool.get<uint32_t>(static_cast<size_t>(m) + 1, "pair offsets");
  if (!pool.fine)
    return GTX_ERR_HIP;
  SecondRound const in{d_list, d_table, n_table, d_second, n_reads, d_events, n_events, static_cast<long>(d->region_begin), REF_SIZE,
                       static_cast<long>(bucket_size), disc_second_buckets(REF_SIZE, bucket_size), d_bucket_max, d_bucket_global_max, d_max_read_size,
                       d_bucket_reads, d_bucket_off, d_pairs, pair_cap};
  hipLaunchKernelGGL(gtx_disc_second_count_kernel, dim3(blocks((static_cast<uint64_t>(m) + 1) * 64)), dim3(TB), 0, s, in, k0, m, n_of);
  if (!launched() || !exclusive_sum(pool, n_of, off, static_cast<size_t>(m) + 1, "scan", "scan temporary"))
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_second_emit_kernel, dim3(blocks(static_cast<uint64_t>(m) * 64)), dim3(TB), 0, s, in, k0, m, off, d_counts);
  hipLaunchKernelGGL(gtx_disc_second_count_finish_kernel, dim3(1), dim3(64), 0, s, d_counts, off, m, pair_cap);
  return launched() ? GTX_OK : GTX_ERR_HIP;
}
