// align_long.hpp -- the alignment (align_core.inl) instantiated for reads of GTX_MAX_READ + 1 .. GTX_MAX_READ_LONG bases: the
// two passes a context made with gtx_params::max_read_len > GTX_MAX_READ runs behind the exact pass (gtx_hbm_passes.hip).
// A read of 1 000 bases has 32 k-mers (1 + (1000 - 32) / 31); seed_stage unpacks it in rounds of 256 bases and issues its
// index lookups in rounds of 8 k-mers (the first KC of them with their half-key buckets and staged entries, as in every pass).
#pragma once
#include "align_core.hpp"

namespace gtx
{
// Tier 1: the tables of the HBM-table pass (big::), with room for the variant sites of a long path (a path of 1 000 bases
// crosses about 40 sites of a graph with a SNP every 25 bases).  What exceeds them goes on to tier 2.
namespace longr
{
struct AlignCfg : FixedTablesCfg
{
  static constexpr uint32_t MAX_READ = GTX_MAX_READ_LONG;
  static constexpr uint32_t MAX_KMERS = 32; // get_num_kmers(MAX_READ)
  static constexpr uint32_t MAXP = 512;
  static constexpr uint32_t MAXPP = 512;
  static constexpr uint32_t MAXV = 64;
  static constexpr uint32_t CAND_CAP = 512;
  static constexpr uint32_t MAXIDS = 64;
  static constexpr uint32_t MW = 2;
};
static_assert(1 + (AlignCfg::MAX_READ - 32) / 31 <= AlignCfg::MAX_KMERS, "k-mers of the longest read");
static_assert(AlignCfg::LBL_CAP == 2048 && AlignCfg::MAXV == 64 && !AlignCfg::DYN, "tier 1's tables");
#include "align_core.inl"
} // namespace longr

// Tier 2: the exact pass (align_core.hpp: namespace exact) for long reads -- tables cut out of a slab at run time, the proven
// bounds of a read of MAX_READ bases
namespace exactl
{
struct AlignCfg : RunTimeTablesCfg<GTX_MAX_READ_LONG, 32, 2>
{
};
static_assert(AlignCfg::MAXV == GTX_MAX_READ_LONG && AlignCfg::MAX_KMERS == 32 && AlignCfg::MW == 2 && AlignCfg::DYN, "tier 2's bounds");
#include "align_core.inl"
} // namespace exactl

namespace exactlw // ... for graphs that have a site of more than 64 alleles
{
struct AlignCfg : RunTimeTablesCfg<GTX_MAX_READ_LONG, 32, GTX_WIDE_MASK_WORDS>
{
};
static_assert(AlignCfg::MAXV == GTX_MAX_READ_LONG && AlignCfg::MAX_KMERS == 32 && AlignCfg::MW > 2 && AlignCfg::DYN, "tier 2's bounds");
#include "align_core.inl"
} // namespace exactlw
} // namespace gtx
