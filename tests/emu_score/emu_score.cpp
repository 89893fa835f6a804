// Host run of the scoring kernels' text (item_is_trivial, score_item and everything under it, graphtyper_amd/csrc/score_core.hpp) over
// memory of its true size, built with AddressSanitizer / UBSan.
//   emu_score case.bin out.bin
// case.bin (tests/score_cases.py: write_case): 16 x uint32 n_ref, n_hap, n_special, n_samples, rec_words, n_reads, n_items, conn_cap, near,
// is_sv_graph, hq_reads, is_segment_calling, compact, n_big, wide (the graph has a site of more than 64 alleles), 1 unused; uint64 total_tri, total_allele, total_near; ref_order, ref_len, ref_nvar
// [n_ref] uint32; tri_off, allele_off [n_hap] uint64; near_last [n_hap] uint32; near_off [n_hap] uint64; special_ref_reach [n_special]
// uint32; records [n_reads * 2 * rec_words] uint32; items [n_items] gtx_score_item; with `compact`: d_compact [max(n_reads, 1) * 8] uint32 and
// the side array [2 * n_reads] uint8; the big-record arena [n_big] uint32 (the path words of records with GTX_ST_EXTERNAL).
// out.bin: log_score, gt_cov, hap_u32, stat_u64, stat_u32, conn_near (with `near`), conn_log [conn_cap * 6], conn_count [2], then the number
// of items both passes refused (uint32).
// The graph's tables, the records, the items, the per-item tables and every accumulator are heap blocks of exactly their size, and the
// records, items, d_compact and the side array are compared with a copy afterwards: a load or a store outside them stops the program, a
// store into the inputs fails it.  The wave policy is sequential: one item after the other, the two passes as the library's scorer runs
// them (the triage, the first pass over tables of SCORE_MAX_HAPS entries, the second over SCORE_MAX_HAPS_BIG -- on a graph with a site
// of more than 64 alleles over SCORE_MAX_HAPS_WIDE entries with wide allele sets -- for what the first gave up).
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
struct WaveSeq
{
  static void atomic_add_u32(uint32_t * p, uint32_t v) { *p += v; }
  static uint32_t atomic_claim_u32(uint32_t * p) { return (*p)++; }
  static void atomic_add_u64(unsigned long long * p, unsigned long long v) { *p += v; }
};

bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

template <class T>
std::unique_ptr<T[]> block(std::FILE * f, size_t n, bool & ok)
{
  std::unique_ptr<T[]> p(new T[n]); // (n = 0: a block of no bytes, any access is one too many)
  ok = ok && read_exact(f, p.get(), n * sizeof(T));
  return p;
}

template <class T>
std::unique_ptr<T[]> zeros(size_t n)
{
  std::unique_ptr<T[]> p(new T[n]);
  if (n)
    std::memset(static_cast<void *>(p.get()), 0, n * sizeof(T));
  return p;
}

template <class T>
std::unique_ptr<T[]> copy_of(std::unique_ptr<T[]> const & a, size_t n)
{
  std::unique_ptr<T[]> p(new T[n]);
  if (n)
    std::memcpy(static_cast<void *>(p.get()), a.get(), n * sizeof(T));
  return p;
}

template <class T>
bool put(std::FILE * o, std::unique_ptr<T[]> const & a, size_t n)
{
  return n == 0 || std::fwrite(a.get(), sizeof(T), n, o) == n;
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_score case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[16];
  uint64_t t[3];
  if (!f || !read_exact(f, h, sizeof h) || !read_exact(f, t, sizeof t))
    return 2;
  uint32_t const n_ref = h[0], n_hap = h[1], n_special = h[2], n_samples = h[3], rec_words = h[4], n_reads = h[5], n_items = h[6], conn_cap = h[7];
  bool const near = h[8] != 0, compact = h[12] != 0, wide = h[14] != 0;
  uint32_t const n_big = h[13];
  ScoreParams const par{h[9], h[10], h[11], 0};
  uint64_t const total_tri = t[0], total_allele = t[1], total_near = t[2];
  bool ok = true;
  auto ref_order = block<uint32_t>(f, n_ref, ok);
  auto ref_len = block<uint32_t>(f, n_ref, ok);
  auto ref_nvar = block<uint32_t>(f, n_ref, ok);
  auto tri_off = block<uint64_t>(f, n_hap, ok);
  auto allele_off = block<uint64_t>(f, n_hap, ok);
  auto near_last = block<uint32_t>(f, n_hap, ok);
  auto near_off = block<uint64_t>(f, n_hap, ok);
  auto special_ref_reach = block<uint32_t>(f, n_special, ok);
  size_t const n_rec = static_cast<size_t>(n_reads) * 2 * rec_words, n_compact = compact ? static_cast<size_t>(n_reads ? n_reads : 1) * GTX_COMPACT_WORDS : 0,
               n_side = compact ? static_cast<size_t>(n_reads) * 2 : 0;
  auto records = block<uint32_t>(f, n_rec, ok);
  auto items = block<gtx_score_item>(f, n_items, ok);
  auto d_compact = block<uint32_t>(f, n_compact, ok);
  auto side = block<uint8_t>(f, n_side, ok);
  auto big_records = block<uint32_t>(f, n_big, ok);
  if (!ok || std::fgetc(f) != EOF || n_hap > n_ref)
    return 2;
  std::fclose(f);
  auto records0 = copy_of(records, n_rec);
  auto items0 = copy_of(items, n_items);
  auto compact0 = copy_of(d_compact, n_compact);
  auto side0 = copy_of(side, n_side);
  auto big0 = copy_of(big_records, n_big);

  GraphView g{};
  g.n_ref = n_ref;
  g.n_special = n_special;
  g.first_order = n_ref ? ref_order[0] : 0;
  g.is_sv_graph = par.is_sv_graph;
  g.ref_order = ref_order.get();
  g.ref_len = ref_len.get();
  g.ref_nvar = ref_nvar.get();
  g.special_ref_reach = special_ref_reach.get();
  g.tri_off = tri_off.get();
  g.allele_off = allele_off.get();
  g.total_tri = total_tri;
  g.total_allele = total_allele;
  g.n_hap = n_hap;
  g.near_last = near_last.get();
  g.near_off = near_off.get();
  g.total_near = total_near;

  size_t const n_ls = static_cast<size_t>(n_samples) * total_tri, n_cov = static_cast<size_t>(n_samples) * total_allele,
               n_cu = static_cast<size_t>(n_samples) * n_hap * 4, n_s64 = n_hap + 2 * total_allele, n_s32 = n_hap + 6 * total_allele,
               n_near = near ? static_cast<size_t>(n_samples) * total_near : 0, n_log = static_cast<size_t>(conn_cap) * 6;
  auto log_score = zeros<uint32_t>(n_ls);
  auto gt_cov = zeros<uint32_t>(n_cov);
  auto hap_u32 = zeros<uint32_t>(n_cu);
  auto stat_u64 = zeros<unsigned long long>(n_s64);
  auto stat_u32 = zeros<uint32_t>(n_s32);
  auto conn_near = zeros<uint32_t>(n_near);
  auto conn_log = zeros<uint32_t>(n_log);
  auto conn_count = zeros<uint32_t>(2);
  ScoreAcc a;
  a.n_samples = n_samples;
  a.conn_cap = conn_cap;
  a.log_score = log_score.get();
  a.gt_cov = gt_cov.get();
  a.hap_u32 = hap_u32.get();
  a.stat_u64 = stat_u64.get();
  a.stat_u32 = stat_u32.get();
  a.conn_log = conn_log.get();
  a.conn_count = conn_count.get();
  a.conn_near = near ? conn_near.get() : nullptr;
  a.big_records = big_records.get();
  if (compact)
  {
    a.compact = d_compact.get();
    a.compact_flags = side.get();
  }
  std::unique_ptr<RecentHap[]> small(new RecentHap[2 * SCORE_MAX_HAPS]), large(new RecentHap[wide ? 0 : 2 * SCORE_MAX_HAPS_BIG]);
  std::unique_ptr<RecentHapWide[]> wide_tables(new RecentHapWide[wide ? 2 * SCORE_MAX_HAPS_WIDE : 0]);
  uint32_t errors = 0;
  for (uint32_t i = 0; i < n_items; ++i)
  {
    if (item_is_trivial(items[i], records.get(), rec_words, false, compact ? side.get() : nullptr)) // stage 1 (gtx_score_triage_kernel)
      continue;
    if (score_item<WaveSeq>(g, par, items[i], records.get(), rec_words, a, small.get(), small.get() + SCORE_MAX_HAPS, SCORE_MAX_HAPS))
      continue;
    if (wide ? !score_item<WaveSeq>(g, par, items[i], records.get(), rec_words, a, wide_tables.get(), wide_tables.get() + SCORE_MAX_HAPS_WIDE, SCORE_MAX_HAPS_WIDE)
             : !score_item<WaveSeq>(g, par, items[i], records.get(), rec_words, a, large.get(), large.get() + SCORE_MAX_HAPS_BIG, SCORE_MAX_HAPS_BIG))
      ++errors;
  }
  if ((n_rec && std::memcmp(records0.get(), records.get(), n_rec * 4u)) || (n_items && std::memcmp(items0.get(), items.get(), n_items * sizeof(gtx_score_item))) ||
      (n_compact && std::memcmp(compact0.get(), d_compact.get(), n_compact * 4u)) || (n_side && std::memcmp(side0.get(), side.get(), n_side)) ||
      (n_big && std::memcmp(big0.get(), big_records.get(), n_big * 4u)))
  {
    std::fprintf(stderr, "emu_score: an input was written\n");
    return 3;
  }
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || !put(o, log_score, n_ls) || !put(o, gt_cov, n_cov) || !put(o, hap_u32, n_cu) || !put(o, stat_u64, n_s64) || !put(o, stat_u32, n_s32) ||
      !put(o, conn_near, n_near) || !put(o, conn_log, n_log) || !put(o, conn_count, 2) || std::fwrite(&errors, 4, 1, o) != 1)
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
