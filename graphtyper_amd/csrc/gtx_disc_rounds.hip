// gtx_disc_rounds.hip -- discovery's second pass from the aligner on (realign_to_indels, src/typer/caller.cpp:1876-2229): the
// entry points around the kernel text of gtx_disc_rounds_dev.hpp.
//
// gtx_disc_second_rounds runs the rounds of a list slice in order.  A round: gtx_disc_second_candidates for its pairs; one lane per
// slot for the slots' sizes, an exclusive sum for their places; one wavefront per slot for the window; gtx_disc_realign_batch; one
// lane per pair for the decision and the size of the read's new list, an exclusive sum for the lists' places; one lane per pair to
// carry the decision out.  The host waits for the stream where a size comes from a count: behind the sizes (the arena), behind the
// decisions (the event array's room).  gtx_disc_second_decide is the final decision over the downloaded counters, host code over
// the one function the device could run as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_devmem.hpp"
#include "gtx_devprim.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_rounds_dev.hpp"
#include "wave_hip.hpp"

static_assert(sizeof(gtx_disc_second_support) == 24 && sizeof(gtx::RoundDecision) == 20, "layouts");
static_assert(sizeof(gtx_disc_second_pair) == sizeof(gtx::RealignPair), "a round's pairs and the aligner's");

namespace
{
using namespace gtx;

constexpr char const * MSG_PREFIX = "gtx_disc_second_rounds: ";
constexpr uint32_t TB = 256;
uint32_t blocks(uint64_t n) { return static_cast<uint32_t>((n + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void gtx_disc_rounds_begin_kernel(gtx_disc_second_read const * __restrict__ reads, uint32_t n_reads, uint32_t n_events,
                                                                   uint16_t * __restrict__ lens, uint32_t * __restrict__ ctl)
{
  rounds_begin(blockIdx.x * blockDim.x + threadIdx.x, reads, n_reads, n_events, lens, ctl);
}

__global__ __launch_bounds__(TB) void gtx_disc_rounds_prepare_kernel(RoundsIn in) { rounds_prepare<WaveHipMem>(in, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(TB) void gtx_disc_rounds_window_kernel(RoundsIn in)
{
  rounds_window_wave<WaveHipMem>(in, __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
}

__global__ __launch_bounds__(TB) void gtx_disc_rounds_decide_kernel(RoundsIn in) { rounds_decide<WaveHipMem>(in, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(TB) void gtx_disc_rounds_apply_kernel(RoundsIn in, uint32_t base, uint32_t event_cap)
{
  rounds_apply<WaveHipMem>(in, blockIdx.x * blockDim.x + threadIdx.x, base, event_cap);
}

__global__ __launch_bounds__(TB) void gtx_disc_rounds_sizes_kernel(gtx_disc_second_read const * __restrict__ reads, uint32_t n_reads, uint32_t * __restrict__ cnt)
{
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_reads)
    cnt[i] = i < n_reads ? reads[i].n_events : 0u;
}

__global__ __launch_bounds__(TB) void gtx_disc_rounds_compact_copy_kernel(gtx_disc_second_read const * __restrict__ reads, uint32_t n_reads,
                                                                          gtx_disc_second_event const * __restrict__ events, uint32_t const * __restrict__ coff,
                                                                          gtx_disc_second_event * __restrict__ tmp, uint32_t cap)
{
  rounds_compact_copy(blockIdx.x * blockDim.x + threadIdx.x, reads, n_reads, events, coff, tmp, cap);
}

__global__ __launch_bounds__(TB) void gtx_disc_rounds_compact_place_kernel(gtx_disc_second_read * __restrict__ reads, uint32_t n_reads, uint32_t const * __restrict__ coff)
{
  rounds_compact_place(blockIdx.x * blockDim.x + threadIdx.x, reads, n_reads, coff);
}

bool launched() { return hip_ok(hipGetLastError(), "kernel launch", MSG_PREFIX); }
bool aligned4(void const * p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int bad(char const * name, char const * why = "bad argument")
{
  g_last_error = std::string(name) + ": " + why;
  return GTX_ERR_ARG;
}
} // namespace

extern "C" int gtx_disc_second_rounds(gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const uint32_t * d_list, uint32_t k0, uint32_t k1,
                                      const gtx_disc_indel * d_table, const char * d_table_seq, uint32_t n_table, uint64_t n_table_seq,
                                      gtx_disc_second_read * d_second, uint32_t n_reads, gtx_disc_second_event * d_events, uint32_t event_cap, uint32_t * n_events,
                                      uint32_t bucket_size, const int32_t * d_bucket_max, const int32_t * d_bucket_global_max, const uint32_t * d_max_read_size,
                                      const uint32_t * d_bucket_reads, const uint32_t * d_bucket_off, gtx_disc_second_support * d_support,
                                      gtx_disc_second_rounds_stats * stats, void * stream)
{
  bool const work = k1 > k0 && n_reads != 0;
  if (!d || !stats || !n_events || bucket_size == 0 || k1 < k0 || plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0 || n_reads >= 0x7FFFFFF0u ||
      *n_events > event_cap || !aligned4(d_planes) || !aligned4(d_list) || !aligned4(d_table) || !aligned4(d_second) || !aligned4(d_events) ||
      !aligned4(d_bucket_max) || !aligned4(d_bucket_global_max) || !aligned4(d_max_read_size) || !aligned4(d_bucket_reads) || !aligned4(d_bucket_off) ||
      !aligned4(d_support) || (event_cap && !d_events) || (n_table_seq && !d_table_seq) ||
      (work && (!d_planes || !d_list || !d_table || !d_second || !d_bucket_max || !d_bucket_global_max || !d_max_read_size || !d_bucket_reads || !d_bucket_off ||
                !d_support)))
    return bad("gtx_disc_second_rounds");
  if (int const rc = device_ready(d->device, "gtx_disc_second_rounds", ": the object"))
    return rc;
  *stats = gtx_disc_second_rounds_stats{};
  if (!work)
    return GTX_OK;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  long const REF_SIZE = static_cast<long>(d->reference.size());
  size_t const slots = static_cast<size_t>(n_reads) + 2;
  DevPtr<uint8_t> arena_seq; // (declared in front of the pool: the pool waits for the stream before anything goes back)
  DevPtr<int32_t> arena_pos;
  DevPtr<gtx_disc_second_event> compact_tmp;
  TempPool pool(s, MSG_PREFIX);
  auto * pairs = pool.get<gtx_disc_second_pair>(n_reads, "pairs");
  auto * counts = pool.get<uint32_t>(2, "pair counters");
  auto * ctl = pool.get<uint32_t>(ROUNDS_CTL_WORDS, "round counters", 0);
  auto * ub = pool.get<uint32_t>(slots, "slot sizes");
  auto * woff = pool.get<uint32_t>(slots, "slot offsets");
  auto * wlen = pool.get<uint32_t>(slots, "window lengths");
  auto * target_off = pool.get<uint32_t>(2 * slots + 1, "window offsets");
  auto * rpairs = pool.get<RealignPair>(n_reads, "aligner pairs");
  auto * results = pool.get<RealignResult>(n_reads, "aligner results");
  auto * decisions = pool.get<RoundDecision>(n_reads, "decisions");
  auto * newn = pool.get<uint32_t>(slots, "list sizes");
  auto * noff = pool.get<uint32_t>(slots, "list offsets");
  auto * lens = pool.get<uint16_t>(n_reads, "read lengths");
  auto * applied = pool.get<uint8_t>(event_cap, "applied flags");
  // one scan temporary for every round (the largest scan is over the slots)
  size_t scan_bytes = 0;
  if (!pool.ok(rocprim::exclusive_scan(nullptr, scan_bytes, ub, woff, 0u, slots, rocprim::plus<uint32_t>(), s), "scan (size)"))
    return GTX_ERR_HIP;
  void * const scan_tmp = pool.get<uint8_t>(scan_bytes, "scan temporary");
  if (!pool.fine)
    return GTX_ERR_HIP;
  auto scan = [&](uint32_t const * from, uint32_t * to, size_t n) {
    size_t bytes = scan_bytes;
    return pool.ok(rocprim::exclusive_scan(scan_tmp, bytes, from, to, 0u, n, rocprim::plus<uint32_t>(), s), "scan");
  };
  uint64_t arena = 0;
  uint32_t count = *n_events;
  uint32_t h_ctl[ROUNDS_CTL_WORDS];

  hipLaunchKernelGGL(gtx_disc_rounds_begin_kernel, dim3(blocks(n_reads)), dim3(TB), 0, s, d_second, n_reads, count, lens, ctl);
  if (!launched() || !hip_ok(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s), "copy", MSG_PREFIX) ||
      !hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX))
    return GTX_ERR_HIP;
  if (h_ctl[ROUNDS_BAD_LIST])
    return bad("gtx_disc_second_rounds", "a read's list does not lie inside the entries in use");

  RoundsIn in{};
  in.refc = reinterpret_cast<char const *>(d->d_refc.get());
  in.REF_SIZE = REF_SIZE;
  in.region_begin = static_cast<long>(d->region_begin);
  in.table = d_table;
  in.table_seq = d_table_seq;
  in.n_table = n_table;
  in.n_table_seq = n_table_seq;
  in.list = d_list;
  in.max_read_size = d_max_read_size;
  in.reads = d_second;
  in.n_reads = n_reads;
  in.events = d_events;
  in.support = d_support;
  in.pairs = pairs;
  in.counts = counts;
  in.ub = ub;
  in.woff = woff;
  in.wlen = wlen;
  in.target_off = target_off;
  in.rpairs = rpairs;
  in.results = results;
  in.applied = applied;
  in.decisions = decisions;
  in.newn = newn;
  in.noff = noff;
  in.ctl = ctl;

  for (uint32_t k = k0; k < k1; ++k)
  {
    in.k = k;
    in.n_events = count;
    // the pairs, the slots' sizes and places
    if (!hip_ok(hipMemsetAsync(counts, 0, 8, s), "clear", MSG_PREFIX) || !hip_ok(hipMemsetAsync(ctl, 0, sizeof h_ctl, s), "clear", MSG_PREFIX))
      return GTX_ERR_HIP;
    if (int const rc = gtx_disc_second_candidates(d, d_list, k, k + 1, d_table, n_table, d_second, n_reads, d_events, count, bucket_size, d_bucket_max,
                                                  d_bucket_global_max, d_max_read_size, d_bucket_reads, d_bucket_off, pairs, n_reads, counts, stream))
      return rc;
    hipLaunchKernelGGL(gtx_disc_rounds_prepare_kernel, dim3(blocks(slots)), dim3(TB), 0, s, in);
    if (!launched() || !scan(ub, woff, slots) ||
        !hip_ok(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s), "copy", MSG_PREFIX) || !hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX))
      return GTX_ERR_HIP;
    uint32_t const n_pairs = h_ctl[ROUNDS_N_PAIRS];
    uint64_t const letters = (static_cast<uint64_t>(h_ctl[ROUNDS_LETTERS_HI]) << 32) | h_ctl[ROUNDS_LETTERS_LO];
    if (letters >= 0x80000000ull)
    {
      g_last_error = "gtx_disc_second_rounds: the windows of round " + std::to_string(k) + " take " + std::to_string(letters) + " letters";
      *n_events = count;
      return GTX_ERR_CAPACITY;
    }
    // room for the round's new lists, at most old sizes + 1 each: compact in front of the round when that might not fit
    if (static_cast<uint64_t>(count) + h_ctl[ROUNDS_NEED_UPPER] > event_cap)
    {
      if (!compact_tmp && !hip_ok(alloc_e(compact_tmp, std::max<size_t>(event_cap, 1) * sizeof(gtx_disc_second_event)), "compaction buffer", MSG_PREFIX))
        return GTX_ERR_HIP;
      uint32_t live = 0;
      hipLaunchKernelGGL(gtx_disc_rounds_sizes_kernel, dim3(blocks(slots)), dim3(TB), 0, s, d_second, n_reads, newn);
      if (!launched() || !scan(newn, noff, static_cast<size_t>(n_reads) + 1))
        return GTX_ERR_HIP;
      hipLaunchKernelGGL(gtx_disc_rounds_compact_copy_kernel, dim3(blocks(n_reads)), dim3(TB), 0, s, d_second, n_reads, d_events, noff, compact_tmp.get(), event_cap);
      hipLaunchKernelGGL(gtx_disc_rounds_compact_place_kernel, dim3(blocks(n_reads)), dim3(TB), 0, s, d_second, n_reads, noff);
      if (!launched() || !hip_ok(hipMemcpyAsync(&live, noff + n_reads, 4, hipMemcpyDeviceToHost, s), "copy", MSG_PREFIX) ||
          !hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX))
        return GTX_ERR_HIP;
      if (live > count) // (lists that share entries: not a state this call leaves)
        return bad("gtx_disc_second_rounds", "the reads' lists overlap");
      if (live && !hip_ok(hipMemcpyAsync(d_events, compact_tmp.get(), static_cast<size_t>(live) * sizeof(gtx_disc_second_event), hipMemcpyDeviceToDevice, s), "copy",
                          MSG_PREFIX))
        return GTX_ERR_HIP;
      count = live;
      in.n_events = count;
      *n_events = count;
      ++stats->compactions;
    }
    // the windows
    if (letters > arena)
    {
      uint64_t const want = std::max<uint64_t>(letters + letters / 2, 1u << 16);
      if (!hip_ok(alloc_e(arena_seq, want), "window letters", MSG_PREFIX) || !hip_ok(alloc_e(arena_pos, want * sizeof(int32_t)), "window positions", MSG_PREFIX))
        return GTX_ERR_HIP;
      arena = want;
    }
    in.seq = arena_seq.get();
    in.refpos = arena_pos.get();
    hipLaunchKernelGGL(gtx_disc_rounds_window_kernel, dim3(blocks((static_cast<uint64_t>(n_pairs) + 1) * 64)), dim3(TB), 0, s, in);
    if (!launched())
      return GTX_ERR_HIP;
    // the alignments, the decisions, the lists' places
    if (n_pairs)
      if (int const rc = gtx_disc_realign_batch(d, d_planes, plane_stride, lens, n_reads, reinterpret_cast<char const *>(in.seq), target_off, 2 * (n_pairs + 1),
                                                reinterpret_cast<gtx_disc_realign_pair const *>(rpairs), n_pairs, reinterpret_cast<gtx_disc_realign_result *>(results),
                                                stream))
        return rc;
    uint32_t total = 0;
    hipLaunchKernelGGL(gtx_disc_rounds_decide_kernel, dim3(blocks(static_cast<uint64_t>(n_reads) + 1)), dim3(TB), 0, s, in);
    if (!launched() || !scan(newn, noff, static_cast<size_t>(n_reads) + 1) ||
        !hip_ok(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s), "copy", MSG_PREFIX) ||
        !hip_ok(hipMemcpyAsync(&total, noff + n_reads, 4, hipMemcpyDeviceToHost, s), "copy", MSG_PREFIX) || !hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX))
      return GTX_ERR_HIP;
    if (static_cast<uint64_t>(count) + total > event_cap)
    {
      stats->events_wanted = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(count) + total, 0xFFFFFFFFu));
      g_last_error = "gtx_disc_second_rounds: round " + std::to_string(k) + " needs " + std::to_string(static_cast<uint64_t>(count) + total) + " entries";
      *n_events = count;
      return GTX_ERR_CAPACITY;
    }
    if (total)
    {
      hipLaunchKernelGGL(gtx_disc_rounds_apply_kernel, dim3(blocks(n_pairs)), dim3(TB), 0, s, in, count, event_cap);
      if (!launched())
        return GTX_ERR_HIP;
      count += total;
    }
    *n_events = count;
    ++stats->rounds_done;
    stats->windows_built += h_ctl[ROUNDS_WINDOWS];
    if (h_ctl[ROUNDS_SKIPPED])
      ++stats->rounds_skipped;
    else
    {
      stats->pairs += n_pairs;
      stats->pairs_aligned += h_ctl[ROUNDS_ALIGNED];
      stats->pairs_refused += h_ctl[ROUNDS_REFUSED];
    }
  }
  return hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX) ? GTX_OK : GTX_ERR_HIP; // (the arena goes back to the cache behind this)
}

extern "C" int gtx_disc_second_decide(const gtx_disc_indel * entries, uint32_t n, const uint32_t * list, uint32_t n_list, const gtx_disc_second_support * support,
                                      uint32_t * good_bits)
{
  if ((n && (!entries || !support || !good_bits)) || (n_list && !list))
    return bad("gtx_disc_second_decide");
  for (uint32_t w = 0; w < (n + 31u) / 32u; ++w)
    good_bits[w] = 0;
  for (uint32_t k = 0; k < n_list; ++k)
  {
    uint32_t const t = list[k];
    if (t >= n)
      return bad("gtx_disc_second_decide", "a list entry behind the table");
    if (entries[t].good) // :2184
      continue;
    if (disc_second_good(entries[t], support[t]))
      good_bits[t >> 5] |= 1u << (t & 31u);
  }
  return GTX_OK;
}
