// Host run of gtx_scores_replay: the scoring kernels' text (score_item, graphtyper_amd/csrc/score_core.hpp) once to make the sums and once
// more in replay mode, then mark_cells_at_guard and replay_cells of score_replay.hpp as they are, over memory of its true size, built
// with AddressSanitizer / UBSan.
//   emu_replay case.bin out.bin
// case.bin: the case file of tests/emu_score (../emu_score/score_case.hpp: the loader and the scoring pass are shared); its 16th header
// word is the capacity of the first log block in entries (the library's is 2^20).
// out.bin: what emu_score writes -- log_score, gt_cov, hap_u32, stat_u64, stat_u32, conn_near (with `near`), conn_log [conn_cap * 6],
// conn_count [2], the number of items both passes refused (uint32) -- after the replay, then 5 x uint32: cells replayed, cells at the
// guard on a site of more than 64 alleles, log entries, passes over the items that the log took (2: the first block was too small), cells
// that a second replay would mark (0), then the log [entries] ReplayEntry in the order the pass left them.  replay_cells gets the log in three orders -- reversed, and
// shuffled by two seeds (the device's log comes in any order) -- and has to give the same cells each time.
// The replay pass runs as the library's does: over the tables of the second scoring pass (SCORE_MAX_HAPS_BIG entries; on a graph with a
// site of more than 64 alleles SCORE_MAX_HAPS_WIDE entries with wide allele sets), a bitmap of exactly (n_cells + 31) / 32 words and a
// log block of exactly its capacity, all heap blocks of their own: a load or a store outside them stops the program.  The accumulators
// are compared with a copy after the replay pass (it adds nothing), the inputs at the end.
#include <algorithm>
#include <vector>

#include "../emu_score/score_case.hpp"
#include "score_replay.hpp"

using namespace gtx;
using emu_case::WaveSeq;

namespace
{
bool same_cells(std::vector<ReplayedCell> x, std::vector<ReplayedCell> y)
{
  auto by_cell = [](ReplayedCell const & p, ReplayedCell const & q) { return p.cell < q.cell; };
  std::sort(x.begin(), x.end(), by_cell);
  std::sort(y.begin(), y.end(), by_cell);
  if (x.size() != y.size())
    return false;
  for (size_t i = 0; i < x.size(); ++i)
    if (x[i].cell != y[i].cell || x[i].max_log_score != y[i].max_log_score || x[i].log_score != y[i].log_score)
      return false;
  return true;
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_replay case.bin out.bin\n");
    return 2;
  }
  emu_case::ScoreCase c;
  if (!c.load(argv[1]))
    return 2;
  uint32_t const first_cap = c.h[15], n_hap = c.n_hap, n_items = c.n_items;
  uint32_t errors = c.score_all();
  // ---- the replay: which cells, the log, the sequential walk
  HostGraph hg;
  hg.n_hap = n_hap;
  hg.ref_nvar.assign(c.ref_nvar.get(), c.ref_nvar.get() + c.n_ref);
  hg.tri_off.assign(c.tri_off.get(), c.tri_off.get() + n_hap);
  hg.total_tri = c.total_tri;
  uint64_t const n_cells = static_cast<uint64_t>(c.n_samples) * n_hap;
  std::vector<uint32_t> marked_v;
  uint64_t unsupported = 0;
  uint64_t const n_marked = mark_cells_at_guard(hg, c.hap_u32.get(), n_cells, marked_v, unsupported);
  if (marked_v.size() != (n_cells + 31) / 32)
    return 3;
  std::unique_ptr<uint32_t[]> marked(new uint32_t[marked_v.size()]);
  std::copy(marked_v.begin(), marked_v.end(), marked.get());
  using emu_case::copy_of;
  auto ls0 = copy_of(c.log_score, c.n_ls);
  auto cov0 = copy_of(c.gt_cov, c.n_cov);
  auto cu0 = copy_of(c.hap_u32, c.n_cu);
  auto s640 = copy_of(c.stat_u64, c.n_s64);
  auto s320 = copy_of(c.stat_u32, c.n_s32);
  auto near0 = copy_of(c.conn_near, c.n_near);
  auto clog0 = copy_of(c.conn_log, c.n_log);
  uint32_t const count0[2] = {c.conn_count[0], c.conn_count[1]};
  std::vector<ReplayEntry> log;
  uint32_t passes = 0;
  if (n_marked != 0 && n_items != 0)
  {
    uint32_t cap = first_cap;
    for (int attempt = 0; attempt < 2; ++attempt) // (replay_collect: a second launch when the log was too small)
    {
      std::unique_ptr<ReplayEntry[]> block_of_cap(new ReplayEntry[cap]);
      std::unique_ptr<uint32_t[]> count(new uint32_t[1]);
      count[0] = 0;
      ScoreAcc ra = c.a;
      ra.conn_cap = 0;
      ra.replay_cells = marked.get();
      ra.replay_log = block_of_cap.get();
      ra.replay_count = count.get();
      ra.replay_cap = cap;
      ++passes;
      for (uint32_t i = 0; i < n_items; ++i)
      {
        ra.replay_item = i;
        if (c.wide ? !score_item<WaveSeq>(c.g, c.par, c.items[i], c.records.get(), c.rec_words, ra, c.wide_tables.get(), c.wide_tables.get() + SCORE_MAX_HAPS_WIDE, SCORE_MAX_HAPS_WIDE)
                   : !score_item<WaveSeq>(c.g, c.par, c.items[i], c.records.get(), c.rec_words, ra, c.large.get(), c.large.get() + SCORE_MAX_HAPS_BIG, SCORE_MAX_HAPS_BIG))
          ++errors;
      }
      uint32_t const wanted = count[0];
      if (wanted <= cap)
      {
        log.assign(block_of_cap.get(), block_of_cap.get() + wanted);
        break;
      }
      cap = wanted;
      if (attempt == 1)
        return 3;
    }
  }
  if ((c.n_ls && std::memcmp(ls0.get(), c.log_score.get(), c.n_ls * 4u)) || (c.n_cov && std::memcmp(cov0.get(), c.gt_cov.get(), c.n_cov * 4u)) ||
      (c.n_cu && std::memcmp(cu0.get(), c.hap_u32.get(), c.n_cu * 4u)) || (c.n_s64 && std::memcmp(s640.get(), c.stat_u64.get(), c.n_s64 * 8u)) ||
      (c.n_s32 && std::memcmp(s320.get(), c.stat_u32.get(), c.n_s32 * 4u)) || (c.n_near && std::memcmp(near0.get(), c.conn_near.get(), c.n_near * 4u)) ||
      (c.n_log && std::memcmp(clog0.get(), c.conn_log.get(), c.n_log * 4u)) || count0[0] != c.conn_count[0] || count0[1] != c.conn_count[1])
  {
    std::fprintf(stderr, "emu_replay: the replay pass wrote to the accumulators\n");
    return 3;
  }
  std::vector<ReplayEntry> const as_logged = log;
  for (ReplayEntry const & e : log)
    if (e.cell >= n_cells || hg.ref_nvar[e.cell % n_hap] > 64) // (replay_store)
      return 3;
  std::reverse(log.begin(), log.end()); // (the order furthest from the call order)
  std::vector<ReplayedCell> const done = replay_cells(hg, log);
  for (uint64_t seed : {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull}) // ... and two orders of no kind: a shuffle that does not depend on a library
  {
    std::vector<ReplayEntry> other = as_logged;
    uint64_t x = seed;
    for (size_t i = other.size(); i > 1; --i)
    {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(other[i - 1], other[(x >> 33) % i]);
    }
    if (!same_cells(done, replay_cells(hg, other)))
    {
      std::fprintf(stderr, "emu_replay: replay_cells gives another result for another order of the log\n");
      return 3;
    }
  }
  for (ReplayedCell const & rc : done)
  {
    uint32_t const hap = rc.cell % n_hap, sample = rc.cell / n_hap;
    c.hap_u32[4ull * rc.cell] = rc.max_log_score | GTX_CELL_REPLAYED;
    std::copy(rc.log_score.begin(), rc.log_score.end(), c.log_score.get() + static_cast<uint64_t>(sample) * c.total_tri + c.tri_off[hap]);
  }
  if (!c.inputs_untouched())
  {
    std::fprintf(stderr, "emu_replay: an input was written\n");
    return 3;
  }
  // a second gtx_scores_replay finds no cell: what was replayed carries the mark
  std::vector<uint32_t> marked_again;
  uint64_t unsupported_again = 0;
  uint64_t const n_again = mark_cells_at_guard(hg, c.hap_u32.get(), n_cells, marked_again, unsupported_again);
  uint32_t const tail[5] = {static_cast<uint32_t>(done.size()), static_cast<uint32_t>(unsupported), static_cast<uint32_t>(as_logged.size()), passes,
                            static_cast<uint32_t>(n_again)};
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || !c.put_arrays(o, errors) || std::fwrite(tail, 4, 5, o) != 5 ||
      (!as_logged.empty() && std::fwrite(as_logged.data(), sizeof(ReplayEntry), as_logged.size(), o) != as_logged.size()))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
