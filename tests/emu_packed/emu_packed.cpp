// Host emulation of gtx_packed_kernel (gtx_api.hip): every (read, group) thread of the kernel in turn, over the same
// graph_dev.hpp helpers (packed_exc_run, planes_from_packed), built with AddressSanitizer.  Every input lives in a heap block
// of exactly the size the case names, so an access the clamping should have prevented stops the driver.
//   emu_packed case.bin out.bin
// case.bin: uint32 n_reads, packed_stride, plane_stride, n_exc, then n_reads * packed_stride bytes of rows, n_reads + 1 uint32
// exc_start (any values: the offsets may claim more entries than there are), n_exc uint16 entries.
// out.bin: n_reads * plane_stride bytes of plane rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../graphtyper_amd/csrc/graph_dev.hpp"

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// the body of one kernel thread
void packed_thread(uint8_t const * packed, uint32_t packed_stride, uint32_t const * exc_start, uint16_t const * exc, uint32_t n_exc,
                   uint32_t * planes, uint32_t groups, uint64_t t)
{
  uint32_t const read = static_cast<uint32_t>(t / groups), grp = static_cast<uint32_t>(t % groups);
  uint32_t o[4] = {0, 0, 0, 0};
  if (PACKED_GROUP_BYTES * (grp + 1) <= packed_stride)
  {
    uint32_t const * w = reinterpret_cast<uint32_t const *>(packed + static_cast<uint64_t>(read) * packed_stride) + 2u * grp;
    uint32_t b, e;
    packed_exc_run(exc_start, read, n_exc, &b, &e);
    planes_from_packed(w[0], w[1], exc, b, e, grp, o);
  }
  std::memcpy(planes + 4u * t, o, sizeof o);
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_packed case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[4];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const n_reads = h[0], packed_stride = h[1], plane_stride = h[2], n_exc = h[3];
  if (packed_stride % PACKED_GROUP_BYTES || plane_stride % PLANE_GROUP_BYTES)
    return 2;
  // exact-size blocks (an empty list is NULL, as the device entry points allow)
  std::unique_ptr<uint8_t[]> packed(new uint8_t[static_cast<size_t>(n_reads) * packed_stride]);
  std::unique_ptr<uint32_t[]> exc_start(new uint32_t[n_reads + 1u]);
  std::unique_ptr<uint16_t[]> exc(n_exc ? new uint16_t[n_exc] : nullptr);
  std::unique_ptr<uint32_t[]> planes(new uint32_t[static_cast<size_t>(n_reads) * plane_stride / 4u]);
  if (!read_exact(f, packed.get(), static_cast<size_t>(n_reads) * packed_stride) || !read_exact(f, exc_start.get(), (n_reads + 1u) * 4u) ||
      !read_exact(f, exc.get(), n_exc * 2u))
    return 2;
  std::fclose(f);
  uint32_t const groups = plane_stride / PLANE_GROUP_BYTES;
  for (uint64_t t = 0; t < static_cast<uint64_t>(n_reads) * groups; ++t)
    packed_thread(packed.get(), packed_stride, exc_start.get(), exc.get(), n_exc, planes.get(), groups, t);
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(planes.get(), 1, static_cast<size_t>(n_reads) * plane_stride, o) != static_cast<size_t>(n_reads) * plane_stride)
    return 2;
  std::fclose(o);
  return 0;
}
