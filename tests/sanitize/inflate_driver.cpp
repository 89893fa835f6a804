// The host DEFLATE decoder (gtx_inflate.hpp: inflate_raw, crc32_of) over the case files of tests/emu_inflate, built with
// AddressSanitizer / UBSan: every member alone, its stream in a heap block of exactly in_len + 8 bytes -- the 8 bytes the
// decoder's header demands behind a stream -- and its output in one of exactly out_len bytes, so a load or store the decoder's
// bounds should have prevented stops the driver.
//   inflate_driver case.bin out.bin
// case.bin: uint32 mode (not looked at), n, check_crc, in_size, out_size, fill; n descriptors of 5 uint32 (in_off, in_len, out_off,
// out_len, crc32); in_size bytes of streams.  out.bin: n uint32 statuses (0 ok, 1 refused, 4 inflated to another CRC-32), then
// the members' outputs one behind the other.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../graphtyper_amd/csrc/gtx_inflate.hpp"

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
bool write_exact(std::FILE * f, void const * p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: inflate_driver case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[6];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const n = h[1], check_crc = h[2], in_size = h[3], fill = h[5];
  std::vector<uint32_t> desc(static_cast<size_t>(n) * 5u);
  std::unique_ptr<uint8_t[]> in(new uint8_t[in_size]);
  if (!read_exact(f, desc.data(), desc.size() * 4u) || !read_exact(f, in.get(), in_size))
    return 2;
  std::fclose(f);
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;
  std::vector<uint32_t> status(n);
  std::vector<uint8_t> all;
  for (uint32_t i = 0; i < n; ++i)
  {
    uint32_t const * d = &desc[i * 5u];
    if (d[0] > in_size || d[1] > in_size - d[0])
      return 2;
    std::unique_ptr<uint8_t[]> mi(new uint8_t[d[1] + 8u]), mo(new uint8_t[d[3]]);
    std::memcpy(mi.get(), in.get() + d[0], d[1]);
    std::memset(mi.get() + d[1], i & 1u ? 0xFF : 0x00, 8); // (a member's CRC-32 and size lie there in a file: anything)
    std::memset(mo.get(), static_cast<int>(fill), d[3]);
    bool const ok = gtx::inflate_raw(mi.get(), d[1], mo.get(), d[3]);
    status[i] = !ok ? 1u : check_crc && gtx::crc32_of(mo.get(), d[3]) != d[4] ? 4u : 0u;
    all.insert(all.end(), mo.get(), mo.get() + d[3]);
  }
  if (!write_exact(o, status.data(), n * 4u) || !write_exact(o, all.data(), all.size()))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
