// Host run of the scoring kernels' text (item_is_trivial, score_item and everything under it, graphtyper_amd/csrc/score_core.hpp) over
// memory of its true size, built with AddressSanitizer / UBSan.
//   emu_score case.bin out.bin
// case.bin: see score_case.hpp (the loader, shared with tests/emu_replay).
// out.bin: log_score, gt_cov, hap_u32, stat_u64, stat_u32, conn_near (with `near`), conn_log [conn_cap * 6], conn_count [2], then the number
// of items both passes refused (uint32).
// The graph's tables, the records, the items, the per-item tables and every accumulator are heap blocks of exactly their size, and the
// records, items, d_compact and the side array are compared with a copy afterwards: a load or a store outside them stops the program, a
// store into the inputs fails it.  The wave policy is sequential: one item after the other, the two passes as the library's scorer runs
// them (the triage, the first pass over tables of SCORE_MAX_HAPS entries, the second over SCORE_MAX_HAPS_BIG -- on a graph with a site
// of more than 64 alleles over SCORE_MAX_HAPS_WIDE entries with wide allele sets -- for what the first gave up).
#include "score_case.hpp"

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_score case.bin out.bin\n");
    return 2;
  }
  emu_case::ScoreCase c;
  if (!c.load(argv[1]))
    return 2;
  uint32_t const errors = c.score_all();
  if (!c.inputs_untouched())
  {
    std::fprintf(stderr, "emu_score: an input was written\n");
    return 3;
  }
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o || !c.put_arrays(o, errors))
    return 2;
  return std::fclose(o) == 0 ? 0 : 2;
}
