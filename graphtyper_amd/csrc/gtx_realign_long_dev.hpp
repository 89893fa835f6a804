// gtx_realign_long_dev.hpp -- the affine-gap aligner of gtx_realign_dev.hpp for the pairs that one refuses: reads of up to
// GTX_MAX_READ_LONG (1 000) bases against windows of up to GTX_REALIGN_MAX_TARGET_LONG (4 095) letters, for a gtx_disc on which
// gtx_disc_set_max_read_len turned them on.  Same model, same recurrence, same outputs and the same tie-break (include/gtx.h);
// THE TIE-BREAK IS THIS LIBRARY'S OWN, AND NOBODY HAS COMPARED THE SCORE WITH paw's (gtx_realign_dev.hpp has the reasons).
//
// One wavefront per pair, written against the wave policy of graph_dev.hpp like the short aligner: gtx_realign.hip instantiates
// it with the hardware wave behind gtx_realign_kernel, tests/emu_realign_long with a sequential one under AddressSanitizer.
//   * Lane l owns the query rows l*R+1 .. l*R+R, R = 2 * ceil(m / 128) <= 16, a template parameter: H and E of every row and the
//     row's match mask are registers (5 per row), start(i) is computed from the lane's first row, what `total` takes off S rides
//     in the mask's upper half.  Rows behind the read's last base pay NO_ROW and never name the result.
//   * The columns pass through the lanes one step apart, as in the short aligner: n + ceil(m / R) - 1 steps, per step the lane
//     shifts of H and F of a lane's bottom row (two words each) and of the column's base.
//   * A value is 64 bits, compared as one signed integer: the score in the high word, the origin (4095 - db) * 2^10 + (1023 - cb)
//     in the low one.  12 bits of db hold a window of 4 095 letters, 10 bits of cb a read of 1 000 bases, and neither fits beside
//     a score of -9 .. 1 000 and a -inf in 32 bits.  Adding a score touches the high word alone (one instruction); a max is one
//     64-bit compare and two selects and prefers the higher score, then the smaller db, then the smaller cb.
//     NEG = -2^20 (high word) serves as -inf: E and F stay within 7 of it, no real value (>= -9) comes near it.
//   * Each lane keeps its best total by the score alone (strict "greater": the smaller j, then the smaller i, within the lane).
//     Two wave maxima name the result: the score, then (4096 - j) * 2^10 + (1024 - i) among the lanes that hold it.
// No LDS, no memory but the loads of the read's own plane groups, the window's own letters (64 columns at a time) and one store.
//
// The pairs' sizes are known on the device only, so the long kernel runs behind gtx_realign_kernel over the same pairs: a pair
// within the short limits, a bad pair and a pair beyond the limits in force already have their result, and the wavefront that
// meets one returns without a store.
#pragma once
#include <cstdint>

#include "gtx_realign_dev.hpp"

#if defined(__HIPCC__)
#define GTX_DEV_INLINED __device__ __forceinline__ // (a call from the kernel would save registers to scratch)
#else
#define GTX_DEV_INLINED inline
#endif

namespace gtx
{
constexpr uint32_t REALIGN_MAX_READ_LONG = 1000, REALIGN_MAX_TARGET_LONG = 4095, REALIGN_MAX_ROWS_LONG = 16;

namespace realign_long_dev
{
constexpr int64_t ONE = int64_t(1) << 32;        // a score of one
constexpr uint32_t CB_BITS = 10, CB_TOP = 1023, DB_TOP = 4095; // the origin: (DB_TOP - db) << CB_BITS | (CB_TOP - cb)
constexpr int64_t NEG = -(int64_t(1) << 20) * ONE; // -inf
constexpr uint32_t NO_ROW = 1u << 15;            // what a row behind the read pays: its total stays below NONE
constexpr int32_t NONE = -(1 << 14);             // best score of a lane that has met no cell
constexpr uint32_t KEY_BIAS = 1u << 14;          // makes a lane's best score a non-negative key
constexpr uint32_t PAY_SHIFT = 16;               // Rows::match: the match bits below, what the row pays above

GTX_DEV int64_t lmax(int64_t a, int64_t b) { return a > b ? a : b; }
GTX_DEV int64_t join(uint32_t lo, uint32_t hi) { return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo); }

template <uint32_t R>
struct Rows // a lane's part of the table
{
  int64_t H[R], E[R]; // of the column the lane worked on last
  uint32_t match[R];  // bit c < 16: the row's base and code c score as a match; >> PAY_SHIFT: what `total` takes off the score of S in this row
  int64_t diag;       // H of the row above the lane's first, one column back
  uint32_t best_origin; // the origin of the S behind the best total
  int32_t best_score; // the best total's score
  uint32_t best_at;   // j << 16 | i of it
};

// one pair whose sizes are within the long limits: row = the read's plane row, t = the window's letters
template <class W, uint32_t R>
GTX_DEV_INLINED void align(uint32_t const * row, uint32_t m, uint8_t const * t, uint32_t n, RealignResult * out)
{
  typename W::template PerLane<Rows<R>> rows;
  typename W::template PerLane<uint32_t> h_lo, h_hi, f_lo, f_hi, hin_lo, hin_hi, fin_lo, fin_hi, base, letters, key;
  uint32_t const neg_lo = static_cast<uint32_t>(static_cast<uint64_t>(NEG)), neg_hi = static_cast<uint32_t>(static_cast<uint64_t>(NEG) >> 32);
  W::lanes([&](uint32_t l) {
    Rows<R> & a = rows[l];
    // the lane's R <= 16 bases lie in at most two plane groups of 32: both are loaded when they hold bases of the read, and
    // plane[k] has plane k's bits of the lane's rows from bit 0 up
    uint32_t const first = l * R, g0 = first >> 5;
    uint32_t plane[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
    {
      uint32_t const lo = g0 * 32u < m ? row[4u * g0 + k] : 0u, hi = (g0 + 1u) * 32u < m ? row[4u * (g0 + 1u) + k] : 0u;
      plane[k] = static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (first & 31u));
    }
#pragma unroll
    for (uint32_t r = 0; r < R; ++r)
    {
      uint32_t const i = first + r + 1;
      uint32_t q = 0;
      if (i <= m)
        q = ((plane[0] >> r) & 1u) | (((plane[1] >> r) & 1u) << 1) | (((plane[2] >> r) & 1u) << 2) | (((plane[3] >> r) & 1u) << 3);
      a.H[r] = a.E[r] = NEG;
      a.match[r] = (q == 15u ? 0xFFFFu : ((1u << q) | 0x8000u)) | ((i < m ? static_cast<uint32_t>(REALIGN_CLIP) : i == m ? 0u : NO_ROW) << PAY_SHIFT);
    }
    a.diag = NEG;
    a.best_origin = 0;
    a.best_score = NONE;
    a.best_at = ((REALIGN_MAX_TARGET_LONG + 1u) << 16) | (CB_TOP + 1u);
    h_lo[l] = f_lo[l] = neg_lo;
    h_hi[l] = f_hi[l] = neg_hi;
    base[l] = 0;
    letters[l] = 0;
  });
  uint32_t const n_lanes = (m + R - 1) / R, steps = n + n_lanes - 1;
  for (uint32_t s = 1; s <= steps; ++s)
  {
    if (((s - 1) & 63u) == 0) // the next 64 columns' letters, one per lane
      W::lanes([&](uint32_t l) {
        uint32_t const at = s - 1 + l;
        letters[l] = at < n ? realign_dev::nt16(t[at]) : 0u;
      });
    W::shift_up(base, W::from_lane(letters, (s - 1) & 63u), base);
    W::shift_up(h_lo, neg_lo, hin_lo);
    W::shift_up(h_hi, neg_hi, hin_hi);
    W::shift_up(f_lo, neg_lo, fin_lo);
    W::shift_up(f_hi, neg_hi, fin_hi);
    W::lanes([&](uint32_t l) {
      Rows<R> & a = rows[l];
      int64_t const h_above = join(hin_lo[l], hin_hi[l]);
      if (s > l && s - l <= n && l < n_lanes)
      {
        uint32_t const j = s - l, c = base[l];
        // start(i) of the lane's first row in column j: db = j - 1, cb = l * R
        uint32_t const origin = ((DB_TOP + 1u - j) << CB_BITS) | (CB_TOP - l * R);
        int64_t up_h = h_above, up_f = join(fin_lo[l], fin_hi[l]), diag = a.diag;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r)
        {
          int64_t const start = join(origin - r, r == 0 && l == 0 ? 0u : static_cast<uint32_t>(-REALIGN_CLIP));
          int64_t const pair = ((a.match[r] >> c) & 1u) ? REALIGN_MATCH * ONE : REALIGN_MISMATCH * ONE;
          int64_t const S = pair + lmax(start, diag);
          int64_t const E = lmax(a.H[r] - REALIGN_GAP_OPEN * ONE, a.E[r] - REALIGN_GAP_EXTEND * ONE);
          int64_t const F = lmax(up_h - REALIGN_GAP_OPEN * ONE, up_f - REALIGN_GAP_EXTEND * ONE);
          int64_t const H = lmax(S, lmax(E, F));
          int32_t const total = static_cast<int32_t>(S >> 32) - static_cast<int32_t>(a.match[r] >> PAY_SHIFT);
          if (total > a.best_score)
          {
            a.best_origin = static_cast<uint32_t>(static_cast<uint64_t>(S));
            a.best_score = total;
            a.best_at = (j << 16) | (l * R + r + 1);
          }
          diag = a.H[r];
          a.H[r] = H;
          a.E[r] = E;
          up_h = H;
          up_f = F;
        }
        h_lo[l] = static_cast<uint32_t>(static_cast<uint64_t>(up_h));
        h_hi[l] = static_cast<uint32_t>(static_cast<uint64_t>(up_h) >> 32);
        f_lo[l] = static_cast<uint32_t>(static_cast<uint64_t>(up_f));
        f_hi[l] = static_cast<uint32_t>(static_cast<uint64_t>(up_f) >> 32);
      }
      a.diag = h_above;
    });
  }
  // the highest score, then the smallest j, then the smallest i: one cell, so one lane
  W::lanes([&](uint32_t l) { key[l] = static_cast<uint32_t>(rows[l].best_score + static_cast<int32_t>(KEY_BIAS)); });
  uint32_t const top_score = W::max(key);
  W::lanes([&](uint32_t l) {
    Rows<R> const & a = rows[l];
    uint32_t const j = a.best_at >> 16, i = a.best_at & 0xFFFFu;
    key[l] = key[l] == top_score ? ((REALIGN_MAX_TARGET_LONG + 1u - j) << CB_BITS) | (CB_TOP + 1u - i) : 0u;
  });
  uint32_t const top = W::max(key);
  W::lanes([&](uint32_t l) {
    Rows<R> const & a = rows[l];
    if (key[l] != top)
      return;
    uint32_t const origin = a.best_origin;
    RealignResult res;
    res.score = a.best_score;
    res.clip_begin = static_cast<uint16_t>(CB_TOP - (origin & CB_TOP));
    res.clip_end = static_cast<uint16_t>(a.best_at & 0xFFFFu);
    res.target_begin = static_cast<uint16_t>(DB_TOP - (origin >> CB_BITS));
    res.target_end = static_cast<uint16_t>(a.best_at >> 16);
    res.status = REALIGN_OK;
    *out = res;
  });
}
} // namespace realign_long_dev

// Pair `p` of a batch behind realign_pair_dev (the same arguments, and max_read: the longest read in force, 257 ..
// REALIGN_MAX_READ_LONG).  Aligns the pair when that one refused it and it is within the limits in force; any other pair has its
// result already and nothing is stored.  Of a pair that is not aligned only lens[] and target_off[] are read.
template <class W>
GTX_DEV_INLINED void realign_long_pair_dev(uint8_t const * planes, uint32_t plane_stride, uint16_t const * lens, uint32_t n_reads, uint8_t const * target_seq,
                                   uint32_t const * target_off, uint32_t n_targets, uint32_t max_read, RealignPair p, RealignResult * out)
{
  if (p.read >= n_reads || p.target >= n_targets)
    return;
  uint32_t const m = W::uni(static_cast<uint32_t>(lens[p.read]));
  uint32_t const t0 = W::uni(target_off[p.target]), t1 = W::uni(target_off[p.target + 1]), arena = W::uni(target_off[n_targets]);
  if (t1 < t0 || t1 > arena || m == 0 || t1 == t0)
    return;
  uint32_t const n = t1 - t0;
  if (m <= REALIGN_MAX_READ && n <= REALIGN_MAX_TARGET) // the short aligner's
    return;
  if (m > max_read || m > plane_stride / PLANE_GROUP_BYTES * 32u || n > REALIGN_MAX_TARGET_LONG) // REALIGN_TOO_LONG stays
    return;
  uint32_t const * row = reinterpret_cast<uint32_t const *>(planes + static_cast<uint64_t>(p.read) * plane_stride);
  uint8_t const * t = target_seq + t0;
  switch ((m + 127u) / 128u)
  {
  case 1: realign_long_dev::align<W, 2>(row, m, t, n, out); break;
  case 2: realign_long_dev::align<W, 4>(row, m, t, n, out); break;
  case 3: realign_long_dev::align<W, 6>(row, m, t, n, out); break;
  case 4: realign_long_dev::align<W, 8>(row, m, t, n, out); break;
  case 5: realign_long_dev::align<W, 10>(row, m, t, n, out); break;
  case 6: realign_long_dev::align<W, 12>(row, m, t, n, out); break;
  case 7: realign_long_dev::align<W, 14>(row, m, t, n, out); break;
  default: realign_long_dev::align<W, 16>(row, m, t, n, out); break;
  }
}
} // namespace gtx
