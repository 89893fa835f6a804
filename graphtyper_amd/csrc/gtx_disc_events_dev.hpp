// gtx_disc_events_dev.hpp -- the walk over a read's CIGAR that starts discovery (run_first_pass, src/typer/caller.cpp:517-561,
// 583-793, 824-834), kernel source: one read per lane.  A read's CIGAR is walked against the region's reference held as bit
// planes (the layout of the alignment kernels' reads, graph_dev.hpp): an M block of 32 bases is four XORs and two one-hot tests,
// a mismatch of two unambiguous bases is a set bit, and every set bit is one SNP event; I and D operations give indel events
// when their bases are all A/C/G/T (one-hot over the range).  Events leave in the read's CIGAR order: every lane counts first,
// a wavefront claims one contiguous piece of the output with one atomic, the lanes write behind each other.
//
// Written against the wave policy of graph_dev.hpp (lane lambdas, W::excl_scan, a leader's claim): gtx_discover.hip instantiates
// it with the hardware wave over the arrays of gtx_disc_events_batch (DiscBatch), tests/emu_disc_events with a sequential wave
// under AddressSanitizer over heap blocks of exactly each read's sizes.
//
// A STATED LIMIT THAT DEPARTS FROM THE REFERENCE: gtx_disc_event.len has 16 bits, so a deletion of more than 65 535 bases is no
// event (the reference makes one with all of its bases, make_deletion_event); the reference offset moves over it all the same,
// as over a deletion that covers a base other than A/C/G/T.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"

namespace gtx
{
namespace disc_events_dev
{
// 32 codes from bit offset `o` of a plane array of `groups` groups (zeros behind its end), plane b
GTX_DEV uint32_t plane_bits(uint32_t const * planes, uint32_t groups, uint32_t o, uint32_t b)
{
  uint32_t const g = o >> 5, s = o & 31u;
  uint32_t const lo = g < groups ? planes[4 * g + b] : 0u, hi = g + 1 < groups ? planes[4 * (g + 1) + b] : 0u;
  return s == 0 ? lo : (lo >> s) | (hi << (32 - s));
}

struct Bits32
{
  uint32_t p0, p1, p2, p3;
  GTX_DEV uint32_t onehot() const
  {
    uint32_t const odd = p0 ^ p1 ^ p2 ^ p3, three = (p0 & p1 & (p2 | p3)) | (p2 & p3 & (p0 | p1));
    return odd & ~three;
  }
};

GTX_DEV Bits32 load32(uint32_t const * planes, uint32_t groups, uint32_t o)
{
  return Bits32{plane_bits(planes, groups, o, 0), plane_bits(planes, groups, o, 1), plane_bits(planes, groups, o, 2), plane_bits(planes, groups, o, 3)};
}

// all of the `n` bases from offset o are A / C / G / T
GTX_DEV bool all_acgt(uint32_t const * planes, uint32_t groups, uint32_t o, uint32_t n)
{
  for (uint32_t k = 0; k < n; k += 32)
  {
    uint32_t const m = n - k >= 32 ? 0xFFFFFFFFu : (1u << (n - k)) - 1u;
    if ((load32(planes, groups, o + k).onehot() & m) != m)
      return false;
  }
  return true;
}

// One walk over a read's CIGAR (caller.cpp:583-775).  EMIT = false counts the events, EMIT = true writes them to out[0..).
// Returns the number of events; pos_end = region-relative end of the alignment (min(ref_offset, REF_SIZE - 1)).
template <bool EMIT>
GTX_DEV uint32_t walk(uint32_t const * refp, uint32_t ref_groups, long REF_SIZE, long region_begin, uint32_t const * row, uint32_t row_groups,
                      uint8_t const * qual, gtx_disc_read const & r, uint32_t const * cigar, uint32_t read_index, gtx_disc_event * out, long & pos_end)
{
  uint32_t n = 0;
  long read_offset = 0, ref_offset = static_cast<long>(r.pos) - region_begin;
  long const l_qseq = r.l_qseq;
  auto put = [&](uint32_t pos, uint8_t type, uint16_t len, uint32_t seq, uint8_t hq, uint16_t dist)
  {
    if (EMIT)
      out[n] = gtx_disc_event{read_index, pos, seq, len, type, hq, dist, 0};
    ++n;
  };
  for (uint32_t i = 0; i < r.n_cigar; ++i)
  {
    uint32_t const word = cigar[i];
    long const count = word >> 4;
    uint32_t const op = word & 15u;
    if (ref_offset >= REF_SIZE)
      break;
    if (op == 0 || op == 7 || op == 8) // M = X
    {
      long const span = std::min<long>(count, std::min(REF_SIZE - ref_offset, std::max<long>(l_qseq - read_offset, 0)));
      for (long k = 0; k < span; k += 32)
      {
        uint32_t const m = span - k >= 32 ? 0xFFFFFFFFu : (1u << (span - k)) - 1u;
        Bits32 const a = load32(row, row_groups, static_cast<uint32_t>(read_offset + k)), g = load32(refp, ref_groups, static_cast<uint32_t>(ref_offset + k));
        uint32_t diff = ((a.p0 ^ g.p0) | (a.p1 ^ g.p1) | (a.p2 ^ g.p2) | (a.p3 ^ g.p3)) & a.onehot() & g.onehot() & m;
        while (diff)
        {
          uint32_t const j = static_cast<uint32_t>(__builtin_ctz(diff));
          diff &= diff - 1u;
          long const read_pos = read_offset + k + j;
          uint32_t const code = ((a.p0 >> j) & 1u) | (((a.p1 >> j) & 1u) << 1) | (((a.p2 >> j) & 1u) << 2) | (((a.p3 >> j) & 1u) << 3);
          char const base = code == 1 ? 'A' : code == 2 ? 'C' : code == 4 ? 'G' : 'T';
          long const dist = std::min(read_pos, l_qseq - 1 - read_pos);
          put(static_cast<uint32_t>(ref_offset + k + j + region_begin), 'X', 1, static_cast<uint32_t>(base), EMIT && qual[read_pos] >= 25 ? 1 : 0,
              static_cast<uint16_t>(std::min<long>(dist, 0xFFFF)));
        }
      }
      read_offset += count;
      ref_offset += count;
    }
    else if (op == 1) // I
    {
      long const b = std::min(read_offset, l_qseq), e = std::min(read_offset + count, l_qseq);
      if (b == e)
        continue; // (caller.cpp:698-699: the read offset stays)
      if (all_acgt(row, row_groups, static_cast<uint32_t>(b), static_cast<uint32_t>(e - b)))
        put(static_cast<uint32_t>(region_begin + ref_offset), 'I', static_cast<uint16_t>(e - b), static_cast<uint32_t>(b), 1, 0);
      read_offset += count;
    }
    else if (op == 2) // D
    {
      // (count <= 0xFFFF: the stated limit of this header's first lines)
      if (count <= 0xFFFF && ref_offset + count < REF_SIZE && all_acgt(refp, ref_groups, static_cast<uint32_t>(ref_offset), static_cast<uint32_t>(count)))
        put(static_cast<uint32_t>(region_begin + ref_offset), 'D', static_cast<uint16_t>(count), static_cast<uint32_t>(ref_offset), 1, 0);
      ref_offset += count;
    }
    else if (op == 4) // S
      read_offset += count;
  }
  pos_end = std::min(ref_offset, REF_SIZE - 1);
  return n;
}
} // namespace disc_events_dev

// groups of the region's plane array: its bases and two groups of zeros (a load of 32 codes from any base needs no test of its own)
inline uint32_t disc_ref_groups(uint64_t reference_len) { return static_cast<uint32_t>((reference_len + 31) / 32) + 2; }

// the region as bit planes of BAM codes (anything but A / C / G / T: N); planes: 4 * disc_ref_groups(reference_len) words of zeros
inline void disc_ref_planes(char const * reference, uint64_t reference_len, uint32_t * planes)
{
  for (uint64_t i = 0; i < reference_len; ++i)
  {
    char const c = reference[i];
    uint32_t const code = c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 15u;
    for (uint32_t b = 0; b < 4; ++b)
      planes[4 * (i >> 5) + b] |= ((code >> b) & 1u) << (i & 31u);
  }
}

// the arguments of gtx_disc_events_batch as the kernel sees them (tests/emu_disc_events has a batch of its own: a heap block per
// read and array)
struct DiscBatch
{
  uint32_t const * refp;
  uint32_t ref_groups;
  long REF_SIZE, region_begin;
  uint8_t const * rows;
  uint32_t plane_stride;
  uint8_t const * qual;
  uint32_t qual_stride;
  gtx_disc_read const * reads;
  uint32_t const * cigar;
  uint32_t n_reads;
  gtx_disc_event * events;
  uint32_t event_cap;
  uint32_t * counts;
  gtx_disc_read_out * read_out;
  GTX_DEV gtx_disc_read read(uint32_t i) const { return reads[i]; }
  GTX_DEV uint32_t const * row_of(uint32_t i) const { return reinterpret_cast<uint32_t const *>(rows + static_cast<uint64_t>(i) * plane_stride); }
  GTX_DEV uint8_t const * qual_of(uint32_t i) const { return qual + static_cast<uint64_t>(i) * qual_stride; }
  GTX_DEV uint32_t const * cigar_of(uint32_t, gtx_disc_read const & r) const { return cigar + r.cigar_off; }
};

// The reads first_read .. first_read + 63 of a batch, lane l the read first_read + l: what gtx_disc_events_kernel does per wavefront.
template <class W, class Batch>
GTX_DEV void disc_events_wave(Batch const & in, uint32_t first_read)
{
  using namespace disc_events_dev;
  typename W::template PerLane<gtx_disc_read> r;
  typename W::template PerLane<uint32_t> n, state, excl;
  typename W::template PerLane<long> pos_end;
  uint32_t const row_groups = in.plane_stride / PLANE_GROUP_BYTES;
  W::lanes([&](uint32_t l) {
    uint32_t const i = first_read + l;
    r[l] = gtx_disc_read{};
    n[l] = 0;
    state[l] = GTX_DISC_SKIPPED;
    pos_end[l] = 0;
    if (i < in.n_reads)
    {
      r[l] = in.read(i);
      // caller.cpp:517-561: reads without a cigar or in front of the region are passed over; a read that starts at or behind the
      // region's end ends the pass
      if (r[l].n_cigar != 0 && r[l].pos >= in.region_begin)
      {
        if (static_cast<long>(r[l].pos) - in.region_begin >= in.REF_SIZE)
          state[l] = GTX_DISC_END;
        else
        {
          state[l] = GTX_DISC_COUNTED;
          n[l] = walk<false>(in.refp, in.ref_groups, in.REF_SIZE, in.region_begin, in.row_of(i), row_groups, in.qual_of(i), r[l], in.cigar_of(i, r[l]), i, nullptr,
                             pos_end[l]);
        }
      }
    }
  });
  // one contiguous piece of the output per wavefront
  uint32_t total = 0;
  W::excl_scan(n, excl, total);
  uint32_t base = 0;
  if (total)
    base = W::claim_u32(in.counts, total);
  W::lanes([&](uint32_t l) {
    uint32_t const i = first_read + l;
    uint32_t const first = base + excl[l];
    if (i < in.n_reads)
    {
      bool const fits = static_cast<uint64_t>(first) + n[l] <= in.event_cap;
      if (n[l] && fits)
        (void)walk<true>(in.refp, in.ref_groups, in.REF_SIZE, in.region_begin, in.row_of(i), row_groups, in.qual_of(i), r[l], in.cigar_of(i, r[l]), i,
                         in.events + first, pos_end[l]);
      if (n[l] && !fits)
        W::atomic_add_u32(in.counts + 1, n[l]);
      in.read_out[i] = gtx_disc_read_out{first, n[l], static_cast<int32_t>(pos_end[l]), state[l]};
    }
  });
}
} // namespace gtx
