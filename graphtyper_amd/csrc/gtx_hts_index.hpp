// gtx_hts_index.hpp -- the binning indexes of htslib's formats (.bai, SAM spec 5.2; .csi; .tbi), as far as they are one thing:
// the numbering of the bins, and the search over the per-reference part of an index held in memory.  Each format's header and
// its own verdicts stay with its reader (gtx_bam.cpp: .bai and the BAM .csi; gtx_tabix.cpp: .tbi and the VCF .csi).
//
// Level l of the bins holds 8^l bins of 2^(min_shift + 3 (depth - l)) positions, numbered from (8^l - 1) / 7; the bin behind
// the last level's, + 1, is the pseudo-bin with the mapped / unmapped counts (37450 in a .bai: min_shift 14, depth 5).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

namespace gtx
{
inline uint32_t bin_first(int level) { return static_cast<uint32_t>(((1ull << (3 * level)) - 1) / 7); }

inline int bin_level(uint32_t bin)
{
  int l = 0;
  while (bin >= bin_first(l + 1))
    ++l;
  return l;
}

// hts_reg2bin: the smallest bin that holds [beg, end)
inline uint32_t reg2bin(int64_t beg, int64_t end, int min_shift, int depth)
{
  --end;
  int s = min_shift;
  for (int l = depth; l > 0; --l, s += 3)
    if ((beg >> s) == (end >> s))
      return bin_first(l) + static_cast<uint32_t>(beg >> s);
  return 0;
}

// little-endian fields off a block of bytes; what lies behind its end is zero and clears `ok`
struct IndexCursor
{
  char const * p;
  size_t n, at = 0;
  bool ok = true;
  template <class T>
  T get()
  {
    T v{};
    if (n - at < sizeof(T))
    {
      ok = false;
      at = n;
      return v;
    }
    std::memcpy(&v, p + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  int32_t count() // (a negative one is no index)
  {
    int32_t const v = get<int32_t>();
    ok = ok && v >= 0;
    return v;
  }
};

struct IndexGeometry
{
  int min_shift, depth;
  bool loffset; // a bin carries the offset of the first record that overlaps it (.csi); else a linear index of 2^min_shift windows follows the bins
};

// Where to start reading for records of reference `tid` that overlap [begin, last]: the smallest chunk start among the bins
// that can hold such a record, not below what the index knows of the region's first window (the linear index' entry, or the
// loffset of the smallest bin around `begin`): no overlapping record of a sorted file starts in front of it.  The cursor
// stands at reference 0's n_bin; references 0 .. tid are walked, so an index cut behind them is as good as a whole one.
// false: the index ends, or a count in it is negative, in front of or inside reference `tid`.  any = false: no record there.
inline bool index_start(IndexCursor & c, IndexGeometry const & g, int32_t tid, int64_t begin, int64_t last, bool & any, uint64_t & voffset)
{
  any = false;
  voffset = UINT64_MAX;
  uint32_t const bins_end = bin_first(g.depth + 1); // (behind it: the pseudo-bin, and numbers no level has)
  for (int32_t r = 0; c.ok && r <= tid; ++r)
  {
    int32_t const n_bin = c.count();
    uint64_t best = UINT64_MAX, lower = 0;
    int lower_level = -1;
    for (int32_t b = 0; c.ok && b < n_bin; ++b)
    {
      uint32_t const bin = c.get<uint32_t>();
      uint64_t const loffset = g.loffset ? c.get<uint64_t>() : 0;
      int32_t const n_chunk = c.count();
      bool overlaps = false;
      if (r == tid && bin < bins_end)
      {
        int const l = bin_level(bin), shift = g.min_shift + 3 * (g.depth - l);
        int64_t const k = static_cast<int64_t>(bin - bin_first(l));
        overlaps = k >= (begin >> shift) && k <= (last >> shift);
        if (g.loffset && k == (begin >> shift) && l > lower_level) // the smallest bin around the region's first base
        {
          lower_level = l;
          lower = loffset;
        }
      }
      for (int32_t k = 0; c.ok && k < n_chunk; ++k)
      {
        uint64_t const chunk_begin = c.get<uint64_t>();
        (void)c.get<uint64_t>();
        if (overlaps && chunk_begin < best)
          best = chunk_begin;
      }
    }
    int32_t const n_intv = g.loffset ? 0 : c.count();
    for (int32_t i = 0; c.ok && i < n_intv; ++i)
    {
      uint64_t const io = c.get<uint64_t>();
      if (r == tid && i == (begin >> g.min_shift))
        lower = io;
    }
    if (c.ok && r == tid && best != UINT64_MAX)
    {
      any = true;
      voffset = std::max(best, lower);
    }
  }
  return c.ok;
}

// The same for a sorted BAM file by the .bai beside it, else its .csi (gtx_bam.cpp): records of reference `tid` that overlap
// [begin, end).  false: no usable index -- the file is scanned from its head.
bool bam_index_start(std::string const & bam_path, int32_t tid, int64_t begin, int64_t end, bool & any, uint64_t & voffset);
} // namespace gtx
