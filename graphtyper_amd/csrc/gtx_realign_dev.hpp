// gtx_realign_dev.hpp -- affine-gap aligner of a read against an indel haplotype window, kernel source: one wavefront aligns one
// (read, window) pair.  What realign_to_indels (src/typer/caller.cpp:1855-2171) asks of paw::pairwise_alignment: the score, the
// two ends in the window and the two clip points (:2022-2153), under the model the reference's text fixes -- match +1, mismatch
// -4, gap open 7, gap extend 1, clip 5 (include/graphtyper/constants.hpp.in:49-53), both ends of the window free, clipping on
// (caller.cpp:1865-1870), an N on either side a match (:2359).  The recurrence and the outputs are stated in include/gtx.h.
// THE TIE-BREAK AMONG EQUALLY GOOD ALIGNMENTS IS THIS LIBRARY'S OWN (paw's is unknown), AND NOBODY HAS COMPARED THE SCORE WITH
// paw's: paw is absent from the reference's tree and cannot be built.
//
// Written against the wave policy of graph_dev.hpp (wave-uniform state + lane lambdas): gtx_realign.hip instantiates it with the
// hardware wave, tests/emu_realign with a sequential one under AddressSanitizer.
//   * Lane l owns the query rows l*R+1 .. l*R+R (R = ceil(m / 64) <= 4, a template parameter: the rows are registers).
//   * The window's columns pass through the lanes one step apart: at step s lane l works on column j = s - l, so a pair takes
//     n + ceil(m / R) - 1 steps.  Per step one lane shift (W::shift_up) hands H and F of a lane's bottom row to the next lane, a
//     third moves the column's base along; the value shifted in one step earlier is the diagonal of the lane's top row.
//     E and the diagonals of the other rows stay in the lane.
//   * Score and origin are one int32: score * 2^19 + (2047 - db) * 2^8 + (255 - cb).  Adding a score leaves the origin alone, and
//     a signed integer max prefers the higher score, then the smaller db, then the smaller cb -- the rule of the definition.
//     S >= -9 everywhere (start >= -5, one mismatch), so -1000 serves as -inf: it is at most one step away from a real value in
//     E and F, and 13 bits of score never overflow (|score| < 4096).
//   * Each lane keeps its best total (score alone decides; a lane meets its columns in order and its rows top down, so a strict
//     "greater" keeps the smaller j, then the smaller i).  One wave maximum over (score, 2048 - j, 256 - i) names the result.
// No LDS of its own, no memory but the loads of the read's plane words and the window's letters (64 columns at a time, one per
// lane) and the one store of the result.
#pragma once
#include <cstdint>

#include "graph_dev.hpp"

namespace gtx
{
// status of a pair (include/gtx.h: GTX_REALIGN_*)
constexpr uint32_t REALIGN_OK = 0, REALIGN_BAD_PAIR = 1, REALIGN_TOO_LONG = 2;
constexpr uint32_t REALIGN_MAX_READ = 256, REALIGN_MAX_TARGET = 2048, REALIGN_MAX_ROWS = 4;
constexpr int32_t REALIGN_MATCH = 1, REALIGN_MISMATCH = -4, REALIGN_GAP_OPEN = 7, REALIGN_GAP_EXTEND = 1, REALIGN_CLIP = 5;

struct RealignPair // gtx_disc_realign_pair
{
  uint32_t read, target;
};
struct RealignResult // gtx_disc_realign_result
{
  int32_t score;
  uint16_t clip_begin, clip_end, target_begin, target_end;
  uint32_t status;
};

namespace realign_dev
{
constexpr int32_t ONE = 1 << 19, ORIGIN = ONE - 1; // a score of one; the origin's bits
constexpr int32_t NEG = -1000 * ONE;               // -inf
constexpr int32_t NO_ROW = 3500 * ONE;             // what a row behind the read pays: below NONE, above the 13 bits' floor
constexpr int32_t NONE = -3000 * ONE;              // best total of a lane that has met no cell

// htslib's seq_nt16_table over letters (either case) and '='; anything else is N
GTX_DEV uint32_t nt16(uint8_t c)
{
  switch (c & 0xDFu)
  {
  case 'A': return 1;
  case 'C': return 2;
  case 'M': return 3;
  case 'G': return 4;
  case 'R': return 5;
  case 'S': return 6;
  case 'V': return 7;
  case 'T': return 8;
  case 'W': return 9;
  case 'Y': return 10;
  case 'H': return 11;
  case 'K': return 12;
  case 'D': return 13;
  case 'B': return 14;
  default: return c == '=' ? 0u : 15u;
  }
}

GTX_DEV int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

template <uint32_t R>
struct Rows // a lane's part of the table
{
  int32_t H[R], E[R]; // of the column the lane worked on last
  int32_t start[R];   // start(i) with cb = i - 1
  int32_t pay[R];     // what `total` takes off S in this row
  uint32_t match[R];  // bit c: the row's base and code c score as a match
  int32_t diag;       // H of the row above the lane's first, one column back
  int32_t best, best_bar; // best total; the same with every origin bit set (what a better score must exceed)
  uint32_t best_at;   // j << 16 | i of it
};

// one pair whose sizes are within the limits: row = the read's plane row, t = the window's letters
template <class W, uint32_t R>
GTX_DEV void align(uint32_t const * row, uint32_t m, uint8_t const * t, uint32_t n, RealignResult * out)
{
  typename W::template PerLane<Rows<R>> rows;
  typename W::template PerLane<uint32_t> h_bot, f_bot, h_in, f_in, base, letters, key;
  W::lanes([&](uint32_t l) {
    Rows<R> & a = rows[l];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r)
    {
      uint32_t const i = l * R + r + 1;
      uint32_t q = 0;
      if (i <= m)
      {
        uint32_t const * g = row + 4u * ((i - 1) >> 5);
        uint32_t const b = (i - 1) & 31u;
        q = ((g[0] >> b) & 1u) | (((g[1] >> b) & 1u) << 1) | (((g[2] >> b) & 1u) << 2) | (((g[3] >> b) & 1u) << 3);
      }
      a.H[r] = a.E[r] = NEG;
      a.start[r] = (i == 1 ? 0 : -REALIGN_CLIP * ONE) + static_cast<int32_t>(256u - i);
      a.pay[r] = i < m ? REALIGN_CLIP * ONE : i == m ? 0 : NO_ROW;
      a.match[r] = q == 15u ? 0xFFFFu : ((1u << q) | 0x8000u);
    }
    a.diag = NEG;
    a.best = NONE;
    a.best_bar = NONE | ORIGIN;
    a.best_at = (REALIGN_MAX_TARGET << 16) | REALIGN_MAX_READ;
    h_bot[l] = f_bot[l] = static_cast<uint32_t>(NEG);
    base[l] = 0;
    letters[l] = 0;
  });
  uint32_t const n_lanes = (m + R - 1) / R, steps = n + n_lanes - 1;
  for (uint32_t s = 1; s <= steps; ++s)
  {
    if (((s - 1) & 63u) == 0) // the next 64 columns' letters, one per lane
      W::lanes([&](uint32_t l) {
        uint32_t const at = s - 1 + l;
        letters[l] = at < n ? nt16(t[at]) : 0u;
      });
    W::shift_up(base, W::from_lane(letters, (s - 1) & 63u), base);
    W::shift_up(h_bot, static_cast<uint32_t>(NEG), h_in);
    W::shift_up(f_bot, static_cast<uint32_t>(NEG), f_in);
    W::lanes([&](uint32_t l) {
      Rows<R> & a = rows[l];
      int32_t const h_above = static_cast<int32_t>(h_in[l]);
      if (s > l && s - l <= n && l < n_lanes)
      {
        uint32_t const j = s - l, c = base[l];
        int32_t const column = static_cast<int32_t>((REALIGN_MAX_TARGET - j) << 8); // db = j - 1
        int32_t up_h = h_above, up_f = static_cast<int32_t>(f_in[l]), diag = a.diag;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r)
        {
          int32_t const pair = ((a.match[r] >> c) & 1u) ? REALIGN_MATCH * ONE : REALIGN_MISMATCH * ONE;
          int32_t const S = pair + imax(a.start[r] + column, diag);
          int32_t const E = imax(a.H[r] - REALIGN_GAP_OPEN * ONE, a.E[r] - REALIGN_GAP_EXTEND * ONE);
          int32_t const F = imax(up_h - REALIGN_GAP_OPEN * ONE, up_f - REALIGN_GAP_EXTEND * ONE);
          int32_t const H = imax(S, imax(E, F));
          int32_t const total = S - a.pay[r];
          if (total > a.best_bar)
          {
            a.best = total;
            a.best_bar = total | ORIGIN;
            a.best_at = (j << 16) | (l * R + r + 1);
          }
          diag = a.H[r];
          a.H[r] = H;
          a.E[r] = E;
          up_h = H;
          up_f = F;
        }
        h_bot[l] = static_cast<uint32_t>(up_h);
        f_bot[l] = static_cast<uint32_t>(up_f);
      }
      a.diag = h_above;
    });
  }
  // the highest score, then the smallest j, then the smallest i: one cell, so one lane
  W::lanes([&](uint32_t l) {
    Rows<R> const & a = rows[l];
    uint32_t const j = a.best_at >> 16, i = a.best_at & 0xFFFFu;
    key[l] = (static_cast<uint32_t>((a.best >> 19) + 4096) << 19) | ((REALIGN_MAX_TARGET - j) << 8) | (REALIGN_MAX_READ - i);
  });
  uint32_t const top = W::max(key);
  W::lanes([&](uint32_t l) {
    Rows<R> const & a = rows[l];
    if (key[l] != top)
      return;
    uint32_t const origin = static_cast<uint32_t>(a.best) & static_cast<uint32_t>(ORIGIN);
    RealignResult res;
    res.score = a.best >> 19;
    res.clip_begin = static_cast<uint16_t>(255u - (origin & 255u));
    res.clip_end = static_cast<uint16_t>(a.best_at & 0xFFFFu);
    res.target_begin = static_cast<uint16_t>(2047u - (origin >> 8));
    res.target_end = static_cast<uint16_t>(a.best_at >> 16);
    res.status = REALIGN_OK;
    *out = res;
  });
}
} // namespace realign_dev

// Pair `p` of a batch (the arguments of gtx_disc_realign_batch).  A pair that names a read or a window that is not there, an
// empty one, or a window whose offsets are not in order within the arena: REALIGN_BAD_PAIR; sizes beyond the limits (or a read
// longer than its plane row): REALIGN_TOO_LONG.  Of such a pair only lens[] and target_off[] are read.
template <class W>
GTX_DEV void realign_pair_dev(uint8_t const * planes, uint32_t plane_stride, uint16_t const * lens, uint32_t n_reads, uint8_t const * target_seq,
                              uint32_t const * target_off, uint32_t n_targets, RealignPair p, RealignResult * out)
{
  uint32_t status = REALIGN_OK, m = 0, n = 0, t0 = 0;
  if (p.read >= n_reads || p.target >= n_targets)
    status = REALIGN_BAD_PAIR;
  else
  {
    m = W::uni(static_cast<uint32_t>(lens[p.read]));
    t0 = W::uni(target_off[p.target]);
    uint32_t const t1 = W::uni(target_off[p.target + 1]), arena = W::uni(target_off[n_targets]);
    if (t1 < t0 || t1 > arena || m == 0 || t1 == t0)
      status = REALIGN_BAD_PAIR;
    else if (m > REALIGN_MAX_READ || m > plane_stride / PLANE_GROUP_BYTES * 32u || t1 - t0 > REALIGN_MAX_TARGET)
      status = REALIGN_TOO_LONG;
    n = t1 - t0;
  }
  if (status != REALIGN_OK)
  {
    if (W::leader())
      *out = RealignResult{0, 0, 0, 0, 0, status};
    return;
  }
  uint32_t const * row = reinterpret_cast<uint32_t const *>(planes + static_cast<uint64_t>(p.read) * plane_stride);
  uint8_t const * t = target_seq + t0;
  switch ((m + 63u) / 64u)
  {
  case 1: realign_dev::align<W, 1>(row, m, t, n, out); break;
  case 2: realign_dev::align<W, 2>(row, m, t, n, out); break;
  case 3: realign_dev::align<W, 3>(row, m, t, n, out); break;
  default: realign_dev::align<W, 4>(row, m, t, n, out); break;
  }
}
} // namespace gtx
