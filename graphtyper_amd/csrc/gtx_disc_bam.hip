// gtx_disc_bam.hip -- the launch of the unpack kernel (gtx_disc_bam_dev.hpp: a BAM record stream -> plane rows, quality rows, CIGAR
// words) and the checks in front of it: gtx_disc_bam_unpack of include/gtx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_devmem.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_bam.hpp"
#include "gtx_disc_bam_dev.hpp"
#include "wave_hip.hpp"

namespace
{
using namespace gtx;

constexpr uint32_t WAVES_PER_BLOCK = 4;
constexpr uint32_t RECORDS_PER_WAVE = 4; // a wavefront's share where the grid is not at its limit: its start is paid once for them
constexpr uint32_t MAX_BLOCKS = 1u << 16;

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_disc_bam_unpack_kernel(uint8_t const * __restrict__ stream, uint32_t const * __restrict__ offsets,
                                                                                   gtx_disc_read const * __restrict__ reads, uint32_t n_reads,
                                                                                   uint8_t * __restrict__ planes, uint32_t plane_stride,
                                                                                   uint8_t * __restrict__ qual, uint32_t qual_stride,
                                                                                   uint32_t * __restrict__ cigar)
{
  disc_bam_unpack_wave<WaveHip>(BamBatch{stream, offsets, reads, n_reads, planes, plane_stride, qual, qual_stride, cigar},
                                blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6), gridDim.x * WAVES_PER_BLOCK);
}

int bad(char const * why)
{
  g_last_error = std::string("gtx_disc_bam_unpack: ") + why;
  return GTX_ERR_ARG;
}
} // namespace

int gtx::disc_bam_unpack_check(uint64_t n_bytes, uint32_t const * offsets, gtx_disc_read const * reads, uint32_t n_reads, uint32_t plane_stride,
                               uint32_t qual_stride, uint32_t n_cigar)
{
  if (n_reads == 0)
    return GTX_OK;
  if (plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0)
    return bad("plane_stride");
  if (n_bytes >= (1ull << 32) || n_reads > n_bytes / 36u)
    return bad("more records than the stream can hold");
  for (uint32_t i = 0; i < n_reads; ++i)
  {
    gtx_disc_read const & r = reads[i];
    if (r.l_qseq > 2u * plane_stride)
      return bad("a read is longer than its plane row");
    if (r.l_qseq > qual_stride)
      return bad("a read is longer than its quality row");
    if (static_cast<uint64_t>(r.cigar_off) + r.n_cigar > n_cigar)
      return bad("a read's cigar words lie behind n_cigar");
    // (the least a record takes: its fixed bytes, a name of one byte, the words, the codes, the qualities.  The name's length is the
    // stream's own byte, which gtx_disc_bam_read held to the record's block: gtx.h asks for a stream that it made)
    if (offsets[i] + 33ull + 4ull * r.n_cigar + (r.l_qseq + 1u) / 2u + r.l_qseq > n_bytes)
      return bad("a record does not lie in the stream");
  }
  return GTX_OK;
}

int gtx::disc_bam_unpack_launch(uint8_t const * d_stream, uint32_t const * d_offsets, gtx_disc_read const * d_reads, uint32_t n_reads, uint8_t * d_planes,
                                uint32_t plane_stride, uint8_t * d_qual, uint32_t qual_stride, uint32_t * d_cigar, void * stream)
{
  if (n_reads == 0)
    return GTX_OK;
  uint32_t const per_block = WAVES_PER_BLOCK * RECORDS_PER_WAVE;
  uint32_t const blocks = std::min((n_reads + per_block - 1u) / per_block, MAX_BLOCKS);
  hipLaunchKernelGGL(gtx_disc_bam_unpack_kernel, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, static_cast<hipStream_t>(stream), d_stream, d_offsets, d_reads, n_reads,
                     d_planes, plane_stride, d_qual, qual_stride, d_cigar);
  if (hipGetLastError() != hipSuccess)
  {
    g_last_error = "gtx_disc_bam_unpack_kernel launch failed";
    return GTX_ERR_HIP;
  }
  return GTX_OK;
}

extern "C" int gtx_disc_bam_unpack(gtx_disc * d, const uint8_t * d_stream, uint64_t n_bytes, const uint32_t * d_offsets, const gtx_disc_read * d_reads,
                                   uint32_t n_reads, uint8_t * d_planes, uint32_t plane_stride, uint8_t * d_qual, uint32_t qual_stride, uint32_t * d_cigar,
                                   uint32_t n_cigar, void * stream)
{
  if (!d || plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0 || (reinterpret_cast<uintptr_t>(d_planes) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(d_cigar) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_offsets) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_reads) & 3u) != 0 ||
      (n_reads != 0 && (!d_stream || !d_offsets || !d_reads || !d_planes || !d_qual || !d_cigar || qual_stride == 0)))
    return bad("bad argument");
  if (int const rc = device_ready(d->device, "gtx_disc_bam_unpack: the object"))
    return rc;
  if (n_reads == 0)
    return GTX_OK;
  try
  {
    // the two tables back on the host: what the kernel indexes by is looked at before it runs
    hipStream_t const s = static_cast<hipStream_t>(stream);
    std::vector<gtx_disc_read> reads(n_reads);
    std::vector<uint32_t> offsets(n_reads);
    if (!hip_ok(hipMemcpyAsync(reads.data(), d_reads, n_reads * sizeof(gtx_disc_read), hipMemcpyDeviceToHost, s), "reads", "gtx_disc_bam_unpack: ") ||
        !hip_ok(hipMemcpyAsync(offsets.data(), d_offsets, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "offsets", "gtx_disc_bam_unpack: ") ||
        !hip_ok(hipStreamSynchronize(s), "wait", "gtx_disc_bam_unpack: "))
      return GTX_ERR_HIP;
    if (int const rc = disc_bam_unpack_check(n_bytes, offsets.data(), reads.data(), n_reads, plane_stride, qual_stride, n_cigar))
      return rc;
    return disc_bam_unpack_launch(d_stream, d_offsets, d_reads, n_reads, d_planes, plane_stride, d_qual, qual_stride, d_cigar, stream);
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_disc_bam_unpack: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}
