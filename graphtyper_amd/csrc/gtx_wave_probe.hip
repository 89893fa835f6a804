// gtx_wave_probe.hip -- the hardware side of the wave policy held to its contract (graph_dev.hpp: the table): wave_probe.hpp's
// text with WaveHip, one wavefront per input set, four to a workgroup so that a wavefront's lanes are threadIdx.x & 63 of a larger
// block the way they are in the kernels.  An inspection call for tests (tests/test_gpu_wave.py); nothing of the library uses it.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "gtx_devmem.hpp"
#include "wave_hip.hpp"
#include "wave_probe.hpp"

namespace
{
using namespace gtx;

constexpr char const * MSG_PREFIX = "gtx_wave_probe: ";
constexpr uint32_t WAVES = 4; // wavefronts (sets) per workgroup

__global__ __launch_bounds__(64 * WAVES) void gtx_wave_probe_kernel(uint32_t const * __restrict__ in, uint32_t n_sets, uint32_t * out)
{
  uint32_t const set = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (set >= n_sets)
    return;
  wave_probe<WaveHip>(in + static_cast<size_t>(set) * WP_IN_WORDS, out + static_cast<size_t>(set) * WP_OUT_WORDS);
}
} // namespace

extern "C" int gtx_wave_probe(int device, const uint32_t * in, uint32_t n_sets, uint32_t * out)
{
  if (n_sets && (!in || !out))
  {
    g_last_error = "gtx_wave_probe: bad argument";
    return GTX_ERR_ARG;
  }
  if (device < 0)
  {
    g_last_error = "gtx_wave_probe: no device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  if (!hip_ok(hipSetDevice(device), "hipSetDevice", MSG_PREFIX))
    return GTX_ERR_HIP;
  if (n_sets == 0)
    return GTX_OK;
  size_t const in_words = static_cast<size_t>(n_sets) * WP_IN_WORDS, out_words = static_cast<size_t>(n_sets) * WP_OUT_WORDS;
  std::vector<uint32_t> start(out_words);
  for (uint32_t s = 0; s < n_sets; ++s)
    wave_probe_start(in + static_cast<size_t>(s) * WP_IN_WORDS, start.data() + static_cast<size_t>(s) * WP_OUT_WORDS);
  DevPtr<uint32_t> d_in, d_out;
  if (!hip_ok(alloc_e(d_in, in_words * 4), "input", MSG_PREFIX) || !hip_ok(alloc_e(d_out, out_words * 4), "output", MSG_PREFIX) ||
      !hip_ok(hipMemcpy(d_in.get(), in, in_words * 4, hipMemcpyHostToDevice), "upload", MSG_PREFIX) ||
      !hip_ok(hipMemcpy(d_out.get(), start.data(), out_words * 4, hipMemcpyHostToDevice), "upload", MSG_PREFIX))
    return GTX_ERR_HIP;
  gtx_wave_probe_kernel<<<(n_sets + WAVES - 1) / WAVES, 64 * WAVES>>>(d_in.get(), n_sets, d_out.get());
  // (the download waits for the kernel: both are on the null stream; the blocks go back to the cache behind it)
  if (!hip_ok(hipGetLastError(), "kernel launch", MSG_PREFIX) || !hip_ok(hipMemcpy(out, d_out.get(), out_words * 4, hipMemcpyDeviceToHost), "download", MSG_PREFIX))
    return GTX_ERR_HIP;
  return GTX_OK;
}
