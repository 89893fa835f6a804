// What the stand-alone host runs of the scoring kernels' text share (tests/emu_score, tests/emu_replay): the case file of
// tests/score_cases.py (write_case) loaded into heap blocks of exactly the arrays' sizes, the graph view and the accumulators over them,
// the per-item tables, the scoring pass as the library's scorer runs it, the check that no input was written, and the arrays written out.
// case.bin: 16 x uint32 n_ref, n_hap, n_special, n_samples, rec_words, n_reads, n_items, conn_cap, near, is_sv_graph, hq_reads,
// is_segment_calling, compact, n_big, wide (the graph has a site of more than 64 alleles), log_cap (tests/emu_replay: its first log
// block); uint64 total_tri, total_allele, total_near; ref_order, ref_len, ref_nvar [n_ref] uint32; tri_off, allele_off [n_hap] uint64;
// near_last [n_hap] uint32; near_off [n_hap] uint64; special_ref_reach [n_special] uint32; records [n_reads * 2 * rec_words] uint32; items
// [n_items] gtx_score_item; with `compact`: d_compact [max(n_reads, 1) * 8] uint32 and the side array [2 * n_reads] uint8; the
// big-record arena [n_big] uint32 (the path words of records with GTX_ST_EXTERNAL).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../wave_seq.hpp"
#include "gtx_flat.hpp"
#include "score_core.hpp" // from the Makefile's CSRC

namespace emu_case
{
using namespace gtx;

using WaveSeq = gtx::WaveSeq;

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

struct ScoreCase
{
  uint32_t h[16];
  uint64_t t[3];
  uint32_t n_ref, n_hap, n_special, n_samples, rec_words, n_reads, n_items, conn_cap, n_big;
  bool near, compact, wide;
  ScoreParams par;
  uint64_t total_tri, total_allele, total_near;
  std::unique_ptr<uint32_t[]> ref_order, ref_len, ref_nvar, near_last, special_ref_reach, records, d_compact, big_records, records0, compact0, big0;
  std::unique_ptr<uint64_t[]> tri_off, allele_off, near_off;
  std::unique_ptr<gtx_score_item[]> items, items0;
  std::unique_ptr<uint8_t[]> side, side0;
  size_t n_rec, n_compact, n_side, n_ls, n_cov, n_cu, n_s64, n_s32, n_near, n_log;
  GraphView g;
  std::unique_ptr<uint32_t[]> log_score, gt_cov, hap_u32, stat_u32, conn_near, conn_log, conn_count;
  std::unique_ptr<unsigned long long[]> stat_u64;
  ScoreAcc a;
  std::unique_ptr<RecentHap[]> small, large;
  std::unique_ptr<RecentHapWide[]> wide_tables;

  // false: the file is not a case file
  bool load(char const * path)
  {
    std::FILE * f = std::fopen(path, "rb");
    if (!f || !read_exact(f, h, sizeof h) || !read_exact(f, t, sizeof t))
      return false;
    n_ref = h[0], n_hap = h[1], n_special = h[2], n_samples = h[3], rec_words = h[4], n_reads = h[5], n_items = h[6], conn_cap = h[7];
    near = h[8] != 0, compact = h[12] != 0, wide = h[14] != 0;
    n_big = h[13];
    par = ScoreParams{h[9], h[10], h[11], 0};
    total_tri = t[0], total_allele = t[1], total_near = t[2];
    bool ok = true;
    ref_order = block<uint32_t>(f, n_ref, ok);
    ref_len = block<uint32_t>(f, n_ref, ok);
    ref_nvar = block<uint32_t>(f, n_ref, ok);
    tri_off = block<uint64_t>(f, n_hap, ok);
    allele_off = block<uint64_t>(f, n_hap, ok);
    near_last = block<uint32_t>(f, n_hap, ok);
    near_off = block<uint64_t>(f, n_hap, ok);
    special_ref_reach = block<uint32_t>(f, n_special, ok);
    n_rec = static_cast<size_t>(n_reads) * 2 * rec_words, n_compact = compact ? static_cast<size_t>(n_reads ? n_reads : 1) * GTX_COMPACT_WORDS : 0,
                 n_side = compact ? static_cast<size_t>(n_reads) * 2 : 0;
    records = block<uint32_t>(f, n_rec, ok);
    items = block<gtx_score_item>(f, n_items, ok);
    d_compact = block<uint32_t>(f, n_compact, ok);
    side = block<uint8_t>(f, n_side, ok);
    big_records = block<uint32_t>(f, n_big, ok);
    if (!ok || std::fgetc(f) != EOF || n_hap > n_ref)
      return false;
    std::fclose(f);
    records0 = copy_of(records, n_rec);
    items0 = copy_of(items, n_items);
    compact0 = copy_of(d_compact, n_compact);
    side0 = copy_of(side, n_side);
    big0 = copy_of(big_records, n_big);

    g = GraphView{};
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

    n_ls = static_cast<size_t>(n_samples) * total_tri, n_cov = static_cast<size_t>(n_samples) * total_allele,
                 n_cu = static_cast<size_t>(n_samples) * n_hap * 4, n_s64 = n_hap + 2 * total_allele, n_s32 = n_hap + 6 * total_allele,
                 n_near = near ? static_cast<size_t>(n_samples) * total_near : 0, n_log = static_cast<size_t>(conn_cap) * 6;
    log_score = zeros<uint32_t>(n_ls);
    gt_cov = zeros<uint32_t>(n_cov);
    hap_u32 = zeros<uint32_t>(n_cu);
    stat_u64 = zeros<unsigned long long>(n_s64);
    stat_u32 = zeros<uint32_t>(n_s32);
    conn_near = zeros<uint32_t>(n_near);
    conn_log = zeros<uint32_t>(n_log);
    conn_count = zeros<uint32_t>(2);
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
    small.reset(new RecentHap[2 * SCORE_MAX_HAPS]);
    large.reset(new RecentHap[wide ? 0 : 2 * SCORE_MAX_HAPS_BIG]);
    wide_tables.reset(new RecentHapWide[wide ? 2 * SCORE_MAX_HAPS_WIDE : 0]);

    return true;
  }

  // the triage and the two passes, one item after the other -> the number of items both passes refused
  uint32_t score_all()
  {
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
    return errors;
  }

  bool inputs_untouched() const
  {
    return !((n_rec && std::memcmp(records0.get(), records.get(), n_rec * 4u)) || (n_items && std::memcmp(items0.get(), items.get(), n_items * sizeof(gtx_score_item))) ||
             (n_compact && std::memcmp(compact0.get(), d_compact.get(), n_compact * 4u)) || (n_side && std::memcmp(side0.get(), side.get(), n_side)) ||
             (n_big && std::memcmp(big0.get(), big_records.get(), n_big * 4u)));
  }

  // log_score, gt_cov, hap_u32, stat_u64, stat_u32, conn_near (with `near`), conn_log [conn_cap * 6], conn_count [2], then `errors`
  bool put_arrays(std::FILE * o, uint32_t errors) const
  {
    return put(o, log_score, n_ls) && put(o, gt_cov, n_cov) && put(o, hap_u32, n_cu) && put(o, stat_u64, n_s64) && put(o, stat_u32, n_s32) &&
           put(o, conn_near, n_near) && put(o, conn_log, n_log) && put(o, conn_count, 2) && std::fwrite(&errors, 4, 1, o) == 1;
  }
};
} // namespace emu_case
