// gtx_disc_bam_walk.hip -- the launches of the record walk (gtx_disc_bam_walk_dev.hpp: a BAM record stream in device memory -> where
// its records begin, their counts checked, the two tables of the unpack kernel) and gtx_disc_bam_walk of include/gtx.h.  Three
// kernels in stream order -- guess, resolve, emit --, none of which waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <string>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_devmem.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_bam.hpp"
#include "gtx_disc_bam_walk_dev.hpp"
#include "wave_hip.hpp"

static_assert(sizeof(gtx_bam_walk_out) == 40 && sizeof(gtx_disc_read) == 16, "layouts of the binding");
static_assert(GTX_BAM_WALK_OK == gtx::BAM_WALK_OK && GTX_BAM_WALK_TRUNCATED == gtx::BAM_WALK_TRUNCATED && GTX_BAM_WALK_MALFORMED == gtx::BAM_WALK_MALFORMED &&
                  GTX_BAM_WALK_LONG_READ == gtx::BAM_WALK_LONG_READ,
              "statuses");

namespace
{
using namespace gtx;

constexpr uint32_t WAVES_PER_BLOCK = 4;
constexpr uint32_t MAX_BLOCKS = 1u << 14; // (the wavefronts stride over the segments behind that)

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_disc_bam_walk_guess_kernel(uint8_t const * __restrict__ stream, uint32_t n_bytes,
                                                                                       uint32_t const * __restrict__ cuts, uint32_t n_cuts, BamWalkSeg * __restrict__ segs)
{
  disc_bam_walk_guess_wave<WaveHip>(BamWalkBatch{stream, n_bytes, cuts, n_cuts, segs}, blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6), gridDim.x * WAVES_PER_BLOCK);
}

__global__ __launch_bounds__(64) void gtx_disc_bam_walk_resolve_kernel(uint8_t const * __restrict__ stream, uint32_t n_bytes, uint32_t const * __restrict__ cuts,
                                                                       uint32_t n_cuts, BamWalkSeg * segs, gtx_bam_walk_out * __restrict__ out)
{
  disc_bam_walk_resolve_wave<WaveHip>(BamWalkBatch{stream, n_bytes, cuts, n_cuts, segs}, out);
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_disc_bam_walk_emit_kernel(uint8_t const * __restrict__ stream, uint32_t n_bytes,
                                                                                      uint32_t const * __restrict__ cuts, uint32_t n_cuts, BamWalkSeg * segs,
                                                                                      uint32_t * __restrict__ offsets, gtx_disc_read * __restrict__ reads)
{
  disc_bam_walk_emit_wave<WaveHip>(BamWalkBatch{stream, n_bytes, cuts, n_cuts, segs}, offsets, reads, blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6),
                                   gridDim.x * WAVES_PER_BLOCK);
}

uint32_t blocks_for(uint32_t n_cuts)
{
  return static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(n_cuts) + WAVES_PER_BLOCK) / WAVES_PER_BLOCK, MAX_BLOCKS)); // (n_cuts + 1 segments)
}

int launched(char const * which)
{
  if (hipGetLastError() == hipSuccess)
    return GTX_OK;
  g_last_error = std::string(which) + " launch failed";
  return GTX_ERR_HIP;
}

int bad(char const * why)
{
  g_last_error = std::string("gtx_disc_bam_walk: ") + why;
  return GTX_ERR_ARG;
}

// Declared behind the blocks of a scope: the stream (the null stream too) is waited for before any of them goes back to the cache.
struct WaitBehind
{
  hipStream_t const stream;
  explicit WaitBehind(hipStream_t s) : stream(s) {}
  WaitBehind(WaitBehind const &) = delete;
  WaitBehind & operator=(WaitBehind const &) = delete;
  ~WaitBehind() { (void)hipStreamSynchronize(stream); }
};
} // namespace

int gtx::disc_bam_walk_count(uint8_t const * d_stream, uint32_t n_bytes, uint32_t const * d_cuts, uint32_t n_cuts, BamWalkSeg * d_segs, gtx_bam_walk_out * d_out,
                             void * stream)
{
  hipStream_t const s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gtx_disc_bam_walk_guess_kernel, dim3(blocks_for(n_cuts)), dim3(64 * WAVES_PER_BLOCK), 0, s, d_stream, n_bytes, d_cuts, n_cuts, d_segs);
  if (int const rc = launched("gtx_disc_bam_walk_guess_kernel"))
    return rc;
  hipLaunchKernelGGL(gtx_disc_bam_walk_resolve_kernel, dim3(1), dim3(64), 0, s, d_stream, n_bytes, d_cuts, n_cuts, d_segs, d_out);
  return launched("gtx_disc_bam_walk_resolve_kernel");
}

int gtx::disc_bam_walk_emit(uint8_t const * d_stream, uint32_t n_bytes, uint32_t const * d_cuts, uint32_t n_cuts, BamWalkSeg * d_segs, uint32_t * d_offsets,
                            gtx_disc_read * d_reads, void * stream)
{
  hipLaunchKernelGGL(gtx_disc_bam_walk_emit_kernel, dim3(blocks_for(n_cuts)), dim3(64 * WAVES_PER_BLOCK), 0, static_cast<hipStream_t>(stream), d_stream, n_bytes, d_cuts,
                     n_cuts, d_segs, d_offsets, d_reads);
  return launched("gtx_disc_bam_walk_emit_kernel");
}

extern "C" int gtx_disc_bam_walk(gtx_disc * d, const uint8_t * d_stream, uint64_t n_bytes, const uint32_t * cuts, uint32_t n_cuts, uint32_t * d_offsets,
                                 gtx_disc_read * d_reads, uint32_t cap, gtx_bam_walk_out * out, void * stream)
{
  if (!d || !out || (n_bytes && !d_stream) || (n_cuts && !cuts) || (d_offsets == nullptr) != (d_reads == nullptr) || (!d_offsets && cap != 0) ||
      (reinterpret_cast<uintptr_t>(d_offsets) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_reads) & 3u) != 0)
    return bad("bad argument");
  if (n_bytes >= (1ull << 32))
    return bad("a stream of 2^32 bytes or more");
  for (uint32_t i = 0; i < n_cuts; ++i)
    if (cuts[i] == 0 || cuts[i] >= n_bytes || (i && cuts[i] <= cuts[i - 1]))
      return bad("the cuts do not ascend inside (0, n_bytes)");
  if (int const rc = device_ready(d->device, "gtx_disc_bam_walk: the object"))
    return rc;
  *out = gtx_bam_walk_out{};
  if (n_bytes == 0)
    return GTX_OK;
  try
  {
    char const * const prefix = "gtx_disc_bam_walk: ";
    hipStream_t const s = static_cast<hipStream_t>(stream);
    DevPtr<uint32_t> d_cuts;
    DevPtr<BamWalkSeg> d_segs;
    DevPtr<gtx_bam_walk_out> d_out;
    WaitBehind const behind(s);
    if (!hip_ok(alloc_e(d_cuts, (static_cast<size_t>(n_cuts) + 1) * sizeof(uint32_t)), "cuts", prefix) ||
        !hip_ok(alloc_e(d_segs, (static_cast<size_t>(n_cuts) + 1) * sizeof(BamWalkSeg)), "segment table", prefix) ||
        !hip_ok(alloc_e(d_out, sizeof(gtx_bam_walk_out)), "out", prefix) ||
        (n_cuts && !hip_ok(hipMemcpyAsync(d_cuts.get(), cuts, static_cast<size_t>(n_cuts) * sizeof(uint32_t), hipMemcpyHostToDevice, s), "cuts", prefix)))
      return GTX_ERR_HIP;
    if (int const rc = disc_bam_walk_count(d_stream, static_cast<uint32_t>(n_bytes), d_cuts.get(), n_cuts, d_segs.get(), d_out.get(), stream))
      return rc;
    if (!hip_ok(hipMemcpyAsync(out, d_out.get(), sizeof(gtx_bam_walk_out), hipMemcpyDeviceToHost, s), "out", prefix) ||
        !hip_ok(hipStreamSynchronize(s), "wait", prefix))
      return GTX_ERR_HIP;
    if (!d_offsets)
      return GTX_OK;
    if (out->n_reads > cap)
    {
      g_last_error = "gtx_disc_bam_walk: " + std::to_string(out->n_reads) + " records for tables of " + std::to_string(cap);
      return GTX_ERR_CAPACITY;
    }
    if (out->n_reads == 0)
      return GTX_OK;
    if (int const rc = disc_bam_walk_emit(d_stream, static_cast<uint32_t>(n_bytes), d_cuts.get(), n_cuts, d_segs.get(), d_offsets, d_reads, stream))
      return rc;
    return hip_ok(hipStreamSynchronize(s), "wait", prefix) ? GTX_OK : GTX_ERR_HIP;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_disc_bam_walk: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}
