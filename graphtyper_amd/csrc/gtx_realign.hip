// gtx_realign.hip -- realignment of reads to indel haplotypes, the pieces of realign_to_indels (src/typer/caller.cpp:1855-2171):
// gtx_realign_kernel (one wavefront per (read, window) pair, gtx_realign_dev.hpp) behind gtx_disc_realign_batch, and the host
// functions around it -- which reads (gtx_disc_realign_wants), the window with the indels applied (gtx_disc_realign_target,
// apply_indel_event src/typer/event.cpp:293-396), what becomes of a read (gtx_disc_realign_decide).  The loop over the indels,
// which carries a read's new state into the next indel's round, is gtx_disc_second_rounds (gtx_disc_rounds.hip).
#include "../../include/gtx.h"
#include "gtx_devmem.hpp"
#include "gtx_disc.hpp"
#include "gtx_realign_dev.hpp"
#include "gtx_realign_long_dev.hpp"
#include "wave_hip.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

static_assert(sizeof(gtx_disc_realign_result) == sizeof(gtx::RealignResult) && sizeof(gtx_disc_realign_result) == 16, "result layout");
static_assert(sizeof(gtx_disc_realign_pair) == sizeof(gtx::RealignPair) && sizeof(gtx_disc_realign_pair) == 8, "pair layout");
static_assert(GTX_REALIGN_OK == gtx::REALIGN_OK && GTX_REALIGN_BAD_PAIR == gtx::REALIGN_BAD_PAIR && GTX_REALIGN_TOO_LONG == gtx::REALIGN_TOO_LONG, "statuses");
static_assert(GTX_REALIGN_MAX_TARGET == gtx::REALIGN_MAX_TARGET && GTX_MAX_READ == gtx::REALIGN_MAX_READ, "limits");
static_assert(GTX_REALIGN_MAX_TARGET_LONG == gtx::REALIGN_MAX_TARGET_LONG && GTX_MAX_READ_LONG == gtx::REALIGN_MAX_READ_LONG, "long limits");

namespace gtx
{
extern thread_local std::string g_last_error;
}

namespace
{
constexpr uint32_t WAVES = 4; // wavefronts (pairs) per workgroup

__global__ __launch_bounds__(64 * WAVES) void gtx_realign_kernel(uint8_t const * __restrict__ planes, uint32_t plane_stride, uint16_t const * __restrict__ lens,
                                                                uint32_t n_reads, uint8_t const * __restrict__ target_seq, uint32_t const * __restrict__ target_off,
                                                                uint32_t n_targets, gtx::RealignPair const * __restrict__ pairs, uint32_t n_pairs,
                                                                gtx::RealignResult * __restrict__ out)
{
  uint32_t const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t const i = blockIdx.x * WAVES + wave;
  if (i >= n_pairs)
    return;
  gtx::RealignPair p;
  p.read = gtx::WaveHip::uni(pairs[i].read);
  p.target = gtx::WaveHip::uni(pairs[i].target);
  gtx::realign_pair_dev<gtx::WaveHip>(planes, plane_stride, lens, n_reads, target_seq, target_off, n_targets, p, out + i);
}

// behind gtx_realign_kernel on the same stream, for a gtx_disc in long mode: the pairs that one refused and the limits in force take
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(3))) void gtx_realign_long_kernel(uint8_t const * __restrict__ planes, uint32_t plane_stride, uint16_t const * __restrict__ lens,
                                                                     uint32_t n_reads, uint8_t const * __restrict__ target_seq,
                                                                     uint32_t const * __restrict__ target_off, uint32_t n_targets, uint32_t max_read,
                                                                     gtx::RealignPair const * __restrict__ pairs, uint32_t n_pairs,
                                                                     gtx::RealignResult * __restrict__ out)
{
  uint32_t const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t const i = blockIdx.x * WAVES + wave;
  if (i >= n_pairs)
    return;
  gtx::RealignPair p;
  p.read = gtx::WaveHip::uni(pairs[i].read);
  p.target = gtx::WaveHip::uni(pairs[i].target);
  gtx::realign_long_pair_dev<gtx::WaveHip>(planes, plane_stride, lens, n_reads, target_seq, target_off, n_targets, max_read, p, out + i);
}
} // namespace

extern "C" int gtx_disc_set_max_read_len(gtx_disc * d, uint32_t max_read_len)
{
  if (!d || !(max_read_len == 0 || (max_read_len >= GTX_MAX_READ && max_read_len <= GTX_MAX_READ_LONG)))
  {
    gtx::g_last_error = "gtx_disc_set_max_read_len: max_read_len must be 0, 256 (GTX_MAX_READ) or 257 .. 1000 (GTX_MAX_READ_LONG)";
    return GTX_ERR_ARG;
  }
  d->max_read_len = max_read_len == GTX_MAX_READ ? 0 : max_read_len;
  return GTX_OK;
}

extern "C" int gtx_disc_realign_batch(gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const uint16_t * d_lens, uint32_t n_reads,
                                      const char * d_target_seq, const uint32_t * d_target_off, uint32_t n_targets, const gtx_disc_realign_pair * d_pairs,
                                      uint32_t n_pairs, gtx_disc_realign_result * d_out, void * stream)
{
  if (!d || plane_stride == 0 || (plane_stride % gtx::PLANE_GROUP_BYTES) != 0 || (reinterpret_cast<uintptr_t>(d_planes) & 3u) != 0 || !d_target_off ||
      (n_pairs != 0 && (!d_pairs || !d_out)) || (n_reads != 0 && (!d_planes || !d_lens)) || (n_targets != 0 && !d_target_seq) || n_targets == 0xFFFFFFFFu)
  {
    gtx::g_last_error = "gtx_disc_realign_batch: bad argument";
    return GTX_ERR_ARG;
  }
  if (int const rc = gtx::device_ready(d->device, "gtx_disc_realign_batch: the object"))
    return rc;
  if (n_pairs == 0)
    return GTX_OK;
  hipLaunchKernelGGL(gtx_realign_kernel, dim3((n_pairs + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream), d_planes, plane_stride, d_lens,
                     n_reads, reinterpret_cast<uint8_t const *>(d_target_seq), d_target_off, n_targets, reinterpret_cast<gtx::RealignPair const *>(d_pairs), n_pairs,
                     reinterpret_cast<gtx::RealignResult *>(d_out));
  if (!gtx::hip_ok(hipGetLastError(), "launch of gtx_realign_kernel", "gtx_disc_realign_batch: "))
    return GTX_ERR_HIP;
  if (d->max_read_len <= GTX_MAX_READ)
    return GTX_OK;
  hipLaunchKernelGGL(gtx_realign_long_kernel, dim3((n_pairs + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream), d_planes, plane_stride,
                     d_lens, n_reads, reinterpret_cast<uint8_t const *>(d_target_seq), d_target_off, n_targets, d->max_read_len,
                     reinterpret_cast<gtx::RealignPair const *>(d_pairs), n_pairs, reinterpret_cast<gtx::RealignResult *>(d_out));
  return gtx::hip_ok(hipGetLastError(), "launch of gtx_realign_long_kernel", "gtx_disc_realign_batch: ") ? GTX_OK : GTX_ERR_HIP;
}

// ---- host: which reads, the window, the decision ----------------------------------------------------------------------------
namespace
{
constexpr long PAD = 50; // caller.cpp:1863

// apply_indel_event (src/typer/event.cpp:293-396); `offset`: contig position of the window's first base
bool apply_indel_event(std::vector<char> & sequence, std::vector<int32_t> & ref_positions, gtx_disc_realign_event const & ev, char const * letters, long offset)
{
  long const ref_pos = static_cast<long>(ev.pos) - offset;
  if (ref_pos <= 0)
    return false;
  long pos = ref_pos; // start the search for the reference position here
  long const event_size = ev.len, seq_size = static_cast<long>(sequence.size());
  if (pos >= seq_size)
    return false;
  if (ref_positions[pos] != ref_pos)
  {
    while (pos + 1 < seq_size && ref_positions[pos] < ref_pos)
      ++pos;
    while (pos > 0 && ref_positions[pos] > ref_pos)
      --pos;
    if (ref_positions[pos] != ref_pos)
      return false;
  }
  { // purity: the positions from three in front to three behind ascend one by one (:330-356)
    long const begin = std::max(0l, pos - 3), end = std::min(seq_size, pos + 3);
    long prev = ref_positions[begin];
    for (long p = begin + 1; p < end; ++p)
    {
      if (ref_positions[p] != prev + 1)
        return false;
      ++prev;
    }
  }
  if (ev.type == 'D')
  {
    if (pos + event_size >= seq_size || ref_positions[pos + event_size] != ref_pos + event_size)
      return false;
    sequence.erase(sequence.begin() + pos, sequence.begin() + pos + event_size);
    ref_positions.erase(ref_positions.begin() + pos, ref_positions.begin() + pos + event_size);
    return true;
  }
  if (ev.type == 'I')
  {
    sequence.insert(sequence.begin() + pos, letters + ev.seq_off, letters + ev.seq_off + event_size);
    ref_positions.insert(ref_positions.begin() + pos + 1, static_cast<size_t>(event_size), static_cast<int32_t>(pos + 1)); // (:385-386: the index, as the text has it)
    return true;
  }
  return false;
}
} // namespace

extern "C" int gtx_disc_realign_wants(int64_t pos, int64_t pos_end, uint32_t num_clipped_begin, uint32_t num_clipped_end, int64_t indel_pos, uint32_t span)
{
  long const cb = num_clipped_begin, ce = num_clipped_end, indel_span = indel_pos + static_cast<long>(span); // caller.cpp:1880
  if (pos < 0) // :1941
    return 0;
  if ((ce == 0 && pos_end < indel_pos) || (pos_end + ce + std::min(ce, PAD) < indel_pos) || (cb == 0 && pos > indel_span) ||
      (pos - cb - std::min(cb, PAD) > indel_span)) // :1948-1955
    return 0;
  return 1;
}

extern "C" int gtx_disc_realign_target(const gtx_disc * d, uint32_t max_read_size, const gtx_disc_realign_event * events, uint32_t n_events,
                                       const char * event_seq, char * seq, int32_t * ref_pos, uint32_t cap, uint32_t * n, int64_t * begin_padded,
                                       uint64_t * applied)
{
  if (!d || !events || n_events == 0 || n_events > 64 || !n || !begin_padded || !applied || (cap && (!seq || !ref_pos)))
  {
    gtx::g_last_error = "gtx_disc_realign_target: bad argument";
    return GTX_ERR_ARG;
  }
  for (uint32_t e = 0; e < n_events; ++e)
    if (events[e].type == 'I' && events[e].len && !event_seq)
    {
      gtx::g_last_error = "gtx_disc_realign_target: an insertion without its letters";
      return GTX_ERR_ARG;
    }
  long const REF_SIZE = static_cast<long>(d->reference.size()), region_begin = d->region_begin, indel_pos = events[0].pos;
  long const begin = std::max(0l, indel_pos - static_cast<long>(max_read_size) - 2 * PAD - region_begin); // caller.cpp:1890
  long const end_padded = indel_pos + static_cast<long>(max_read_size) + 2 * PAD - region_begin;         // :1892
  if (begin >= REF_SIZE || end_padded < begin)
  {
    gtx::g_last_error = "gtx_disc_realign_target: the indel's window lies outside the region";
    return GTX_ERR_ARG;
  }
  long const end = end_padded >= REF_SIZE ? REF_SIZE : end_padded; // :1894
  std::vector<char> new_ref(d->reference.begin() + begin, d->reference.begin() + end);
  std::vector<int32_t> positions(new_ref.size());
  for (size_t i = 0; i < positions.size(); ++i)
    positions[i] = static_cast<int32_t>(i);
  uint64_t bits = 0;
  if (apply_indel_event(new_ref, positions, events[0], event_seq, begin + region_begin)) // :1902-1906
  {
    bits = 1;
    for (uint32_t e = 1; e < n_events; ++e) // :1968-2002
      if (apply_indel_event(new_ref, positions, events[e], event_seq, begin + region_begin))
        bits |= 1ull << e;
  }
  *begin_padded = begin;
  *applied = bits;
  *n = static_cast<uint32_t>(new_ref.size());
  if (new_ref.size() > cap)
  {
    gtx::g_last_error = "gtx_disc_realign_target: the window has " + std::to_string(new_ref.size()) + " letters";
    return GTX_ERR_CAPACITY;
  }
  std::copy(new_ref.begin(), new_ref.end(), seq);
  std::copy(positions.begin(), positions.end(), ref_pos);
  return GTX_OK;
}

extern "C" int gtx_disc_realign_decide(const gtx_disc_realign_result * r, uint32_t read_len, const int32_t * ref_pos, uint32_t n, int64_t begin_padded,
                                       int64_t region_begin, int64_t old_score, int64_t indel_pos, gtx_disc_realign_decision * out)
{
  if (!r || !ref_pos || !out || r->status != GTX_REALIGN_OK || r->target_begin >= r->target_end || r->target_end > n || r->clip_begin >= r->clip_end ||
      r->clip_end > read_len)
  {
    gtx::g_last_error = "gtx_disc_realign_decide: bad argument (a result without GTX_REALIGN_OK, or not of this read and window)";
    return GTX_ERR_ARG;
  }
  *out = gtx_disc_realign_decision{0, 0, GTX_REALIGN_NO_PADDING, 0, 0, 0};
  long const db = r->target_begin, de = r->target_end;
  if (db == 0 || de == static_cast<long>(n)) // caller.cpp:2025
    return GTX_OK;
  if (r->score <= old_score) // :2066
  {
    if (r->score < old_score)
      out->outcome = GTX_REALIGN_WORSE; // READ_ANTI_SUPPORT, :2084
    else if (indel_pos >= ref_pos[db] + begin_padded && indel_pos <= ref_pos[de] + begin_padded) // :2086-2087
      out->outcome = GTX_REALIGN_SAME_OVERLAPPING;                                                  // READ_MULTI_SUPPORT, :2097
    else
      out->outcome = GTX_REALIGN_SAME;
    return GTX_OK;
  }
  out->outcome = GTX_REALIGN_BETTER;
  out->pos = ref_pos[db] + region_begin + begin_padded;     // :2136
  out->pos_end = ref_pos[de] + region_begin + begin_padded; // :2137
  out->num_clipped_begin = r->clip_begin;                   // :2139
  out->num_clipped_end = read_len - r->clip_end;            // :2140
  long num_ins = 0;                                         // :2143-2153
  while (db + num_ins + 1 < static_cast<long>(n) && ref_pos[db + num_ins] == ref_pos[db + num_ins + 1])
    ++num_ins;
  out->num_ins_begin = static_cast<uint32_t>(num_ins);
  return GTX_OK;
}
