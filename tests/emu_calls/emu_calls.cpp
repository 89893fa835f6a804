// Host run of gtx_calls_kernel's text (call_cell, graphtyper_amd/csrc/score_core.hpp) over memory of its true size, built with
// AddressSanitizer / UBSan.
//   emu_calls case.bin out.bin
// case.bin: uint32 n_hap, n_samples; uint64 total_tri, total_allele; hap_cnum [n_hap] uint32; tri_off [n_hap], allele_off [n_hap] uint64;
// log_score [n_samples * total_tri], gt_cov [n_samples * total_allele], hap_u32 [n_samples * n_hap * 4] uint32.
// out.bin: phred [n_samples * total_tri] uint8, then calls [n_samples * n_hap] gtx_sample_call (both filled with 0xA5 before the run).
// The graph's three tables, the three accumulators, phred and calls are each a heap block of exactly their size, and the
// accumulators are compared with a copy afterwards: a load or a store outside a cell's rows stops the program, a store into the
// accumulators fails it.  call_cell runs once per cell, as the kernel's threads do.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gtx_flat.hpp"
#include "score_core.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

template <class T>
std::unique_ptr<T[]> block(std::FILE * f, size_t n, bool & ok)
{
  std::unique_ptr<T[]> p(new T[n]); // (n = 0: a block of no bytes, any access is one too many)
  ok = ok && read_exact(f, p.get(), n * sizeof(T));
  return p;
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_calls case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h32[2];
  uint64_t h64[2];
  if (!f || !read_exact(f, h32, sizeof h32) || !read_exact(f, h64, sizeof h64))
    return 2;
  uint32_t const n_hap = h32[0], n_samples = h32[1];
  uint64_t const total_tri = h64[0], total_allele = h64[1], cells = static_cast<uint64_t>(n_samples) * n_hap;
  bool ok = true;
  auto hap_cnum = block<uint32_t>(f, n_hap, ok);
  auto tri_off = block<uint64_t>(f, n_hap, ok);
  auto allele_off = block<uint64_t>(f, n_hap, ok);
  size_t const n_ls = static_cast<size_t>(n_samples) * total_tri, n_cov = static_cast<size_t>(n_samples) * total_allele, n_cu = cells * 4u;
  auto log_score = block<uint32_t>(f, n_ls, ok);
  auto gt_cov = block<uint32_t>(f, n_cov, ok);
  auto hap_u32 = block<uint32_t>(f, n_cu, ok);
  if (!ok || std::fgetc(f) != EOF)
    return 2;
  std::fclose(f);
  // the tables have to tile a sample's rows, or the blocks below are not the sizes the library would allocate
  uint64_t tri = 0, allele = 0;
  for (uint32_t h = 0; h < n_hap; ++h)
  {
    if (tri_off[h] != tri || allele_off[h] != allele || hap_cnum[h] < 2)
      return 2;
    tri += static_cast<uint64_t>(hap_cnum[h]) * (hap_cnum[h] + 1) / 2;
    allele += hap_cnum[h];
  }
  if (tri != total_tri || allele != total_allele)
    return 2;
  std::unique_ptr<uint32_t[]> ls0(new uint32_t[n_ls]), cov0(new uint32_t[n_cov]), cu0(new uint32_t[n_cu]);
  std::memcpy(ls0.get(), log_score.get(), n_ls * 4u);
  std::memcpy(cov0.get(), gt_cov.get(), n_cov * 4u);
  std::memcpy(cu0.get(), hap_u32.get(), n_cu * 4u);
  std::unique_ptr<uint8_t[]> phred(new uint8_t[n_ls]);
  std::unique_ptr<gtx_sample_call[]> calls(new gtx_sample_call[cells]);
  std::memset(phred.get(), 0xA5, n_ls);
  std::memset(static_cast<void *>(calls.get()), 0xA5, cells * sizeof(gtx_sample_call));
  GraphView g{};
  g.ref_nvar = hap_cnum.get();
  g.tri_off = tri_off.get();
  g.allele_off = allele_off.get();
  g.total_tri = total_tri;
  g.total_allele = total_allele;
  g.n_hap = n_hap;
  for (uint64_t cell = 0; cell < cells; ++cell)
    call_cell(g, cell, log_score.get(), gt_cov.get(), hap_u32.get(), phred.get(), calls.get());
  if (std::memcmp(ls0.get(), log_score.get(), n_ls * 4u) || std::memcmp(cov0.get(), gt_cov.get(), n_cov * 4u) || std::memcmp(cu0.get(), hap_u32.get(), n_cu * 4u))
  {
    std::fprintf(stderr, "emu_calls: an accumulator was written\n");
    return 3;
  }
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || (n_ls && std::fwrite(phred.get(), 1, n_ls, o) != n_ls) || (cells && std::fwrite(calls.get(), sizeof(gtx_sample_call), cells, o) != cells))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
