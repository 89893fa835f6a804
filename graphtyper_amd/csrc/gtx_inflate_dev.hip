// gtx_inflate_dev.hip -- DEFLATE on the device: gtx_inflate_kernel (one wavefront per BGZF member, gtx_inflate_dev.hpp) and
// the gtx_inflate_* entry points around it.  The BAM readers' device team (gtx_bgzf.cpp) goes through inflate_host_batch.
#include "../../include/gtx.h"
#include "gtx_bgzf.hpp"
#include "gtx_devmem.hpp"
#include "gtx_host_loops.hpp"
#include "gtx_inflate_dev.hpp"
#include "gtx_inflate_host.hpp"
#include "wave_hip.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gtx
{
extern thread_local std::string g_last_error;
}

static_assert(sizeof(gtx_inflate_member) == sizeof(gtx::InflateMember) && sizeof(gtx_inflate_member) == 32, "descriptor layout");
static_assert(GTX_INFLATE_OK == gtx::INFL_OK && GTX_INFLATE_BAD_STREAM == gtx::INFL_BAD_STREAM && GTX_INFLATE_SHORT == gtx::INFL_SHORT &&
                  GTX_INFLATE_LONG == gtx::INFL_LONG && GTX_INFLATE_CRC == gtx::INFL_CRC && GTX_INFLATE_BAD_MEMBER == gtx::INFL_BAD_MEMBER,
              "statuses");

namespace
{
// the tables are in LDS, the output in global memory: both kinds of hand-over between the lanes of the wavefront
struct WaveInflate : gtx::WaveHip
{
  // (always the wavefront's own hand-over: the wavefronts of a workgroup leave at different times, a workgroup barrier would hang)
  static __device__ inline void lds_sync()
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  static __device__ inline void mem_sync() { gtx::WaveHipMem::mem_sync(); }
};

constexpr uint32_t WAVES = 4; // wavefronts (members) per workgroup

__global__ __launch_bounds__(64 * WAVES) void gtx_inflate_kernel(uint8_t const * __restrict__ in, uint64_t in_size, gtx::InflateMember const * __restrict__ members,
                                                                uint32_t n, uint8_t * out, uint64_t out_size, uint32_t * __restrict__ status, int check_crc)
{
  __shared__ gtx::InflateWs ws[WAVES];
  uint32_t const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t const i = blockIdx.x * WAVES + wave;
  if (i >= n)
    return;
  gtx::InflateMember m;
  m.in_off = WaveInflate::uni(members[i].in_off);
  m.out_off = WaveInflate::uni(members[i].out_off);
  m.in_len = WaveInflate::uni(members[i].in_len);
  m.out_len = WaveInflate::uni(members[i].out_len);
  m.crc32 = WaveInflate::uni(members[i].crc32);
  m.reserved = 0;
  uint32_t const st = gtx::inflate_member_dev<WaveInflate>(ws[wave], in, in_size, m, out, out_size, check_crc != 0);
  if (WaveInflate::leader())
    status[i] = st;
}
} // namespace

struct gtx_inflate
{
  int device = -1;
  // what the host calls stage through (grown on demand, kept)
  gtx::DevPtr<uint8_t> d_in, d_out;
  gtx::DevPtr<gtx_inflate_member> d_members;
  gtx::DevPtr<uint32_t> d_status;
  size_t in_cap = 0, out_cap = 0, n_cap = 0;
  gtx::Stream stream;
};

extern "C" int gtx_inflate_create(int device, gtx_inflate ** out)
{
  if (!out)
  {
    gtx::g_last_error = "gtx_inflate_create: bad argument";
    return GTX_ERR_ARG;
  }
  *out = nullptr;
  int n_dev = 0;
  if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev)
  {
    gtx::g_last_error = "gtx_inflate_create: no such HIP device (no CPU compute path: gtx_inflate_raw is the host's decoder)";
    return GTX_ERR_NO_DEVICE;
  }
  auto h = std::make_unique<gtx_inflate>();
  h->device = device;
  hipStream_t s = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
  {
    gtx::g_last_error = "gtx_inflate_create: could not make a stream on the device";
    return GTX_ERR_HIP;
  }
  h->stream.reset(s);
  *out = h.release();
  return GTX_OK;
}

extern "C" void gtx_inflate_destroy(gtx_inflate * h)
{
  if (!h)
    return;
  (void)hipSetDevice(h->device);
  delete h; // (the stream is waited for before the blocks go back to the cache: members are destroyed in reverse order)
}

extern "C" int gtx_inflate_batch(gtx_inflate * h, const void * d_in, uint64_t in_size, const gtx_inflate_member * d_members, uint32_t n, void * d_out,
                                 uint64_t out_size, uint32_t * d_status, int check_crc, void * stream)
{
  if (!h || (n && (!d_members || !d_status)) || (in_size && !d_in) || (out_size && !d_out))
  {
    gtx::g_last_error = "gtx_inflate_batch: bad argument";
    return GTX_ERR_ARG;
  }
  if (n == 0)
    return GTX_OK;
  if (hipSetDevice(h->device) != hipSuccess)
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_inflate_kernel, dim3((n + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream), static_cast<uint8_t const *>(d_in),
                     in_size, reinterpret_cast<gtx::InflateMember const *>(d_members), n, static_cast<uint8_t *>(d_out), out_size, d_status, check_crc);
  if (hipGetLastError() != hipSuccess)
  {
    gtx::g_last_error = "gtx_inflate_kernel launch failed";
    return GTX_ERR_HIP;
  }
  return GTX_OK;
}

// Host buffers through the inflater's own device blocks and stream: streams and descriptors up, one launch, output and statuses
// down; returns when they are there.  `in` and `out` are best pinned (the readers' team's are).
int gtx::inflate_host_batch(gtx_inflate * h, uint8_t const * in, uint64_t in_size, gtx_inflate_member const * members, uint32_t n, uint8_t * out,
                            uint64_t out_size, uint32_t * status, bool check_crc)
{
  if (n == 0)
    return GTX_OK;
  if (hipSetDevice(h->device) != hipSuccess)
    return GTX_ERR_HIP;
  hipStream_t const s = h->stream.get();
  auto grow = [](auto & p, size_t & cap, size_t want) {
    if (want <= cap)
      return true;
    want += want / 4;
    cap = gtx::alloc(p, want * sizeof(*p.get())) ? want : 0;
    return cap != 0;
  };
  size_t status_cap = h->n_cap;
  if (!grow(h->d_in, h->in_cap, in_size + 8) || !grow(h->d_out, h->out_cap, out_size + 8) || !grow(h->d_members, h->n_cap, n) ||
      !grow(h->d_status, status_cap, n))
  {
    h->in_cap = h->out_cap = h->n_cap = 0;
    gtx::g_last_error = "gtx_inflate: device memory for a batch of " + std::to_string(in_size) + " + " + std::to_string(out_size) + " bytes";
    return GTX_ERR_HIP;
  }
  // (whatever fails: nothing queued on the stream still reads or writes the caller's buffers when this returns)
  gtx::StreamWait const wait(s);
  if ((in_size && hipMemcpyAsync(h->d_in.get(), in, in_size, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(h->d_members.get(), members, static_cast<size_t>(n) * sizeof(gtx_inflate_member), hipMemcpyHostToDevice, s) != hipSuccess)
  {
    gtx::g_last_error = "gtx_inflate: host to device copy";
    return GTX_ERR_HIP;
  }
  int const rc = gtx_inflate_batch(h, h->d_in.get(), in_size, h->d_members.get(), n, h->d_out.get(), out_size, h->d_status.get(), check_crc ? 1 : 0, s);
  if (rc != GTX_OK)
    return rc;
  if ((out_size && hipMemcpyAsync(out, h->d_out.get(), out_size, hipMemcpyDeviceToHost, s) != hipSuccess) ||
      hipMemcpyAsync(status, h->d_status.get(), static_cast<size_t>(n) * 4u, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
  {
    gtx::g_last_error = std::string("gtx_inflate: device to host copy: ") + hipGetErrorString(hipGetLastError());
    return GTX_ERR_HIP;
  }
  return GTX_OK;
}

extern "C" int gtx_inflate_bgzf(gtx_inflate * h, const void * in_v, uint64_t in_len, void * out, uint64_t cap, uint64_t * out_len, int check_crc)
{
  if (!h || (in_len && !in_v) || !out_len || (cap && !out))
  {
    gtx::g_last_error = "gtx_inflate_bgzf: bad argument";
    return GTX_ERR_ARG;
  }
  uint8_t const * in = static_cast<uint8_t const *>(in_v);
  std::vector<gtx_inflate_member> members;
  uint64_t at = 0, total = 0;
  while (at < in_len)
  {
    gtx::BgzfMember head;
    char const * why = gtx::parse_bgzf_member(in + at, in_len - at, head);
    if (!why && !head.whole)
      why = "truncated";
    if (why)
    {
      gtx::g_last_error = "gtx_inflate_bgzf: member " + std::to_string(members.size()) + " at byte " + std::to_string(at) + ": " + why;
      return GTX_ERR_IO;
    }
    gtx_inflate_member m{};
    m.in_off = at + head.hlen;
    m.in_len = static_cast<uint32_t>(head.clen);
    m.crc32 = head.crc32;
    m.out_len = head.isize;
    m.out_off = total;
    total += m.out_len;
    at += head.bsize + 1ull;
    if (m.out_len) // (the end-of-file marker, or an empty member)
      members.push_back(m);
  }
  *out_len = total;
  if (!out && cap == 0)
    return GTX_OK;
  if (total > cap)
  {
    gtx::g_last_error = "gtx_inflate_bgzf: the members inflate to " + std::to_string(total) + " bytes";
    return GTX_ERR_CAPACITY;
  }
  if (members.size() > 0xFFFFFFFFull)
    return GTX_ERR_UNSUPPORTED;
  std::vector<uint32_t> status(members.size());
  int const rc = gtx::inflate_host_batch(h, in, in_len, members.data(), static_cast<uint32_t>(members.size()), static_cast<uint8_t *>(out), total, status.data(),
                                         check_crc != 0);
  if (rc != GTX_OK)
    return rc;
  for (size_t i = 0; i < members.size(); ++i)
    if (status[i] != GTX_INFLATE_OK)
    {
      static char const * const WHAT[] = {"ok", "not a valid DEFLATE stream", "shorter than its ISIZE", "longer than its ISIZE", "CRC32 differs", "bad descriptor"};
      gtx::g_last_error = "gtx_inflate_bgzf: the member at byte " + std::to_string(members[i].in_off) + " (number " + std::to_string(i) + " of those with data): " +
                          (status[i] < 6 ? WHAT[status[i]] : "unknown status");
      return GTX_ERR_IO;
    }
  return GTX_OK;
}

namespace
{
gtx::InflateDeviceOps const OPS = {gtx_inflate_create, gtx_inflate_destroy,
                                   [](gtx_inflate * h, uint64_t bytes) -> void * {
                                     void * p = nullptr;
                                     return hipSetDevice(h->device) == hipSuccess && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
                                   },
                                   [](void * p) { (void)hipHostFree(p); }, gtx::inflate_host_batch};
bool const ops_set = (gtx::inflate_device_ops = &OPS, true);
} // namespace
