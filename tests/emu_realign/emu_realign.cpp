// Host emulation of gtx_realign_kernel (gtx_realign.hip): every pair of a batch in turn through the kernel's source
// (gtx_realign_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_realign case.bin out.bin
// case.bin: uint32 plane_stride, n_reads, n_targets, n_pairs, arena; n_reads plane rows; n_reads uint16 lengths (+ one of padding
// when n_reads is odd); n_targets + 1 uint32 offsets; `arena` letters (padded to a multiple of four); n_pairs (read, target).
// out.bin: n_pairs results of 16 bytes (filled with 0xA5 before the pair runs).
// A pair within the limits runs over heap blocks of exactly its sizes -- the read's plane groups that hold its m bases, its n
// letters, one length, two offsets -- so a load the kernel's bounds should have prevented stops the driver; any other pair runs
// over the batch's arrays, of which it may read the lengths and the offsets only (the rows and letters are then not passed).
// Prints the seconds the pairs took (the plain build is the host figure of tools/realign_rate.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_realign_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_realign case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[5];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const plane_stride = h[0], n_reads = h[1], n_targets = h[2], n_pairs = h[3], arena = h[4];
  if (plane_stride == 0 || plane_stride % PLANE_GROUP_BYTES)
    return 2;
  std::vector<uint32_t> planes(static_cast<size_t>(n_reads) * plane_stride / 4u), off(static_cast<size_t>(n_targets) + 1u);
  std::vector<uint16_t> lens((n_reads + 1u) & ~1u);
  std::vector<uint8_t> seq((arena + 3u) & ~3u);
  std::vector<RealignPair> pairs(n_pairs);
  if (!read_exact(f, planes.data(), planes.size() * 4u) || !read_exact(f, lens.data(), lens.size() * 2u) || !read_exact(f, off.data(), off.size() * 4u) ||
      !read_exact(f, seq.data(), seq.size()) || !read_exact(f, pairs.data(), pairs.size() * sizeof(RealignPair)))
    return 2;
  std::fclose(f);
  std::vector<RealignResult> out(n_pairs);
  std::memset(out.data(), 0xA5, out.size() * sizeof(RealignResult));
  auto const t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n_pairs; ++i)
  {
    RealignPair const p = pairs[i];
    bool within = p.read < n_reads && p.target < n_targets;
    uint32_t m = 0, n = 0;
    if (within)
    {
      m = lens[p.read];
      uint32_t const a = off[p.target], b = off[p.target + 1];
      within = a < b && b <= off[n_targets] && b <= arena && m != 0 && m <= REALIGN_MAX_READ && m <= plane_stride / PLANE_GROUP_BYTES * 32u &&
               b - a <= REALIGN_MAX_TARGET;
      n = b - a;
    }
    if (!within)
    {
      realign_pair_dev<WaveSeq>(nullptr, plane_stride, lens.data(), n_reads, nullptr, off.data(), n_targets, p, &out[i]);
      continue;
    }
    uint32_t const groups = (m + 31u) / 32u;
    std::unique_ptr<uint32_t[]> row(new uint32_t[groups * 4u]);
    std::unique_ptr<uint8_t[]> letters(new uint8_t[n]);
    std::unique_ptr<uint16_t[]> len1(new uint16_t[1]);
    std::unique_ptr<uint32_t[]> off2(new uint32_t[2]);
    std::memcpy(row.get(), planes.data() + static_cast<size_t>(p.read) * plane_stride / 4u, groups * 16u);
    std::memcpy(letters.get(), seq.data() + off[p.target], n);
    len1[0] = static_cast<uint16_t>(m);
    off2[0] = 0;
    off2[1] = n;
    // (plane_stride as given: the row's own groups are all the kernel may touch of it)
    realign_pair_dev<WaveSeq>(reinterpret_cast<uint8_t const *>(row.get()), plane_stride, len1.get(), 1, letters.get(), off2.get(), 1, RealignPair{0, 0}, &out[i]);
  }
  double const secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || (n_pairs && std::fwrite(out.data(), sizeof(RealignResult), n_pairs, o) != n_pairs))
    return 2;
  std::printf("%.6f\n", secs);
  return std::fclose(o) == 0 ? 0 : 2;
}
