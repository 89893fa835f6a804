// Host emulation of gtx_inflate_kernel (gtx_inflate_dev.hip): every member of a batch in turn through the kernel's source
// (gtx_inflate_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_inflate case.bin out.bin
// case.bin: uint32 mode, n, check_crc, in_size, out_size, fill; n descriptors of 5 uint32 (in_off, in_len, out_off, out_len, crc32);
// in_size bytes of streams.
//   mode 0: every member alone -- its stream in a heap block of exactly in_len bytes, its output in one of exactly out_len
//           bytes, so a load or store the decoder's bounds should have prevented stops the driver.  out.bin: n uint32 statuses,
//           then the members' outputs one behind the other.
//   mode 1: the batch as the device entry point takes it -- one input block of in_size bytes, one output block of out_size
//           bytes filled with `fill`, the descriptors as given (they may point anywhere).  out.bin: n uint32 statuses, then the
//           output block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../graphtyper_amd/csrc/gtx_inflate_dev.hpp"
#include "../wave_seq.hpp"

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
bool write_exact(std::FILE * f, void const * p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_inflate case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[6];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const mode = h[0], n = h[1], check_crc = h[2], in_size = h[3], out_size = h[4], fill = h[5];
  std::vector<uint32_t> desc(static_cast<size_t>(n) * 5u);
  std::unique_ptr<uint8_t[]> in(new uint8_t[in_size]);
  if (!read_exact(f, desc.data(), desc.size() * 4u) || !read_exact(f, in.get(), in_size))
    return 2;
  std::fclose(f);
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;
  std::vector<uint32_t> status(n);
  std::unique_ptr<InflateWs> ws(new InflateWs);
  if (mode == 1)
  {
    std::unique_ptr<uint8_t[]> out(new uint8_t[out_size]);
    std::memset(out.get(), static_cast<int>(fill), out_size);
    for (uint32_t i = 0; i < n; ++i)
    {
      uint32_t const * d = &desc[i * 5u];
      InflateMember const m{d[0], d[2], d[1], d[3], d[4], 0};
      std::memset(ws.get(), 0xA5, sizeof(InflateWs)); // (what the member before left in LDS is anything)
      status[i] = inflate_member_dev<WaveSeq>(*ws, in.get(), in_size, m, out.get(), out_size, check_crc != 0);
    }
    if (!write_exact(o, status.data(), n * 4u) || !write_exact(o, out.get(), out_size))
      return 2;
  }
  else
  {
    std::vector<uint8_t> all;
    for (uint32_t i = 0; i < n; ++i)
    {
      uint32_t const * d = &desc[i * 5u];
      if (d[0] > in_size || d[1] > in_size - d[0])
        return 2;
      std::unique_ptr<uint8_t[]> mi(new uint8_t[d[1]]), mo(new uint8_t[d[3]]);
      std::memcpy(mi.get(), in.get() + d[0], d[1]);
      std::memset(mo.get(), static_cast<int>(fill), d[3]);
      InflateMember const m{0, 0, d[1], d[3], d[4], 0};
      std::memset(ws.get(), 0xA5, sizeof(InflateWs));
      status[i] = inflate_member_dev<WaveSeq>(*ws, mi.get(), d[1], m, mo.get(), d[3], check_crc != 0);
      all.insert(all.end(), mo.get(), mo.get() + d[3]);
    }
    if (!write_exact(o, status.data(), n * 4u) || !write_exact(o, all.data(), all.size()))
      return 2;
  }
  return std::fclose(o) == 0 ? 0 : 2;
}
