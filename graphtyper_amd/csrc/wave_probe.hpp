// wave_probe.hpp -- the wave policy's primitives (graph_dev.hpp: the table), each called once on one input set and what it returned
// or left in memory written out, per lane where it is per-lane.  Policy-generic text like the kernels': gtx_wave_probe.hip runs it
// with WaveHip, tests/emu_wave with the sequential wave, and tests/wave_probe_cases.py states in plain Python what both must
// write.  Not probed: lds_sync / mem_sync (nothing to read back), clock (any value will do) and note.
#pragma once
#include <cstdint>

#include "graph_dev.hpp"

namespace gtx
{
// a set's input words: per lane two values and a flag, then the wave-uniform ones
constexpr uint32_t WP_IN_A = 0, WP_IN_B = 64, WP_IN_FLAG = 128;
constexpr uint32_t WP_IN_K = 192;       // a lane index (its low six bits are used)
constexpr uint32_t WP_IN_FIRST = 193;   // shift_up's `first`; also what claim_u32 takes
constexpr uint32_t WP_IN_START32 = 194; // where every 32-bit counter starts (atomic_max_i32: as int32)
constexpr uint32_t WP_IN_START64 = 195; // where the 64-bit counters start: low word, high word
constexpr uint32_t WP_IN_WORDS = 200;

// a set's output words.  Per lane:
constexpr uint32_t WP_OUT_SHIFT = 0;    // shift_up(a, first) into another object
constexpr uint32_t WP_OUT_SHIFT2 = 64;  // shift_up(x, first, x) twice on a copy x of a
constexpr uint32_t WP_OUT_SCAN = 128;   // excl_scan(a)
constexpr uint32_t WP_OUT_CLAIM = 192;  // what claim_u32(counter, first) returned
constexpr uint32_t WP_OUT_ACLAIM = 256; // what atomic_claim_u32(counter) returned to a flagged lane; 0xFFFFFFFF for the others
// wave-uniform, written by the leader:
constexpr uint32_t WP_OUT_FROM_LANE = 320; // from_lane(a, k)
constexpr uint32_t WP_OUT_UNI32 = 321;     // uni(first ^ k)
constexpr uint32_t WP_OUT_UNI64 = 322;     // uni(uint64 first << 32 | start32): low word, high word
constexpr uint32_t WP_OUT_BALLOT = 324;    // ballot(flag): low word, high word
constexpr uint32_t WP_OUT_SUM = 326, WP_OUT_MAX = 327, WP_OUT_SCAN_TOTAL = 328; // of a
// the counters: wave_probe_start puts the start values there, the probe's atomics work on them in place.  The flagged lanes
// contribute b (32 bits) or uint64 a << 32 | b (64 bits).
constexpr uint32_t WP_OUT_CLAIM_CTR = 329, WP_OUT_ACLAIM_CTR = 330, WP_OUT_ADD32 = 331;
constexpr uint32_t WP_OUT_ADD64 = 332; // (even, like WP_OUT_WORDS: a 64-bit counter is 8-byte aligned when `out` is)
constexpr uint32_t WP_OUT_SUB32 = 334, WP_OUT_MAXU32 = 335;
constexpr uint32_t WP_OUT_OR64 = 336;
constexpr uint32_t WP_OUT_MAXI32 = 338, WP_OUT_OR32 = 339;
constexpr uint32_t WP_OUT_WORDS = 340;
constexpr uint32_t WP_NO_SLOT = 0xFFFFFFFFu;

// Host, before the probe runs: zeroes a set's output and puts the counters at their start values.  (On the device this is the
// upload in front of the launch: no lane of the probe depends on a store another lane made to global memory.)
inline void wave_probe_start(uint32_t const * in, uint32_t * out)
{
  for (uint32_t i = 0; i < WP_OUT_WORDS; ++i)
    out[i] = 0;
  for (uint32_t c : {WP_OUT_CLAIM_CTR, WP_OUT_ACLAIM_CTR, WP_OUT_ADD32, WP_OUT_SUB32, WP_OUT_MAXU32, WP_OUT_MAXI32, WP_OUT_OR32})
    out[c] = in[WP_IN_START32];
  for (uint32_t c : {WP_OUT_ADD64, WP_OUT_OR64})
  {
    out[c] = in[WP_IN_START64];
    out[c + 1] = in[WP_IN_START64 + 1];
  }
}

// one wave, one set: `in` WP_IN_WORDS words, `out` WP_OUT_WORDS words as wave_probe_start left them, 8-byte aligned
template <class W>
GTX_DEV void wave_probe(uint32_t const * in, uint32_t * out)
{
  typename W::template PerLane<uint32_t> a, b, x, y, scan, slot;
  typename W::template PerLane<bool> flag;
  W::lanes([&](uint32_t l) {
    a[l] = in[WP_IN_A + l];
    b[l] = in[WP_IN_B + l];
    flag[l] = in[WP_IN_FLAG + l] != 0;
    x[l] = a[l];
  });
  uint32_t const k = W::uni(in[WP_IN_K]) & 63u, first = W::uni(in[WP_IN_FIRST]), start32 = W::uni(in[WP_IN_START32]);

  W::shift_up(a, first, y);
  W::shift_up(x, first, x);
  W::shift_up(x, first, x);
  uint32_t total = 0;
  W::excl_scan(a, scan, total);
  uint32_t const picked = W::from_lane(a, k), u32 = W::uni(first ^ k), sum = W::sum(a), max = W::max(a);
  uint64_t const u64 = W::uni((static_cast<uint64_t>(first) << 32) | start32), mask = W::ballot(flag);

  uint32_t const claimed = W::claim_u32(out + WP_OUT_CLAIM_CTR, first);
  W::lanes([&](uint32_t l) {
    slot[l] = WP_NO_SLOT;
    if (flag[l])
    {
      slot[l] = W::atomic_claim_u32(out + WP_OUT_ACLAIM_CTR);
      uint64_t const wide = (static_cast<uint64_t>(a[l]) << 32) | b[l];
      W::atomic_add_u32(out + WP_OUT_ADD32, b[l]);
      W::atomic_add_u64(reinterpret_cast<unsigned long long *>(out + WP_OUT_ADD64), wide);
      W::atomic_sub_u32(out + WP_OUT_SUB32, b[l]);
      W::atomic_max_u32(out + WP_OUT_MAXU32, b[l]);
      W::atomic_max_i32(reinterpret_cast<int32_t *>(out + WP_OUT_MAXI32), static_cast<int32_t>(b[l]));
      W::atomic_or_u32(out + WP_OUT_OR32, b[l]);
      W::atomic_or_u64(reinterpret_cast<uint64_t *>(out + WP_OUT_OR64), wide);
    }
  });

  W::lanes([&](uint32_t l) {
    out[WP_OUT_SHIFT + l] = y[l];
    out[WP_OUT_SHIFT2 + l] = x[l];
    out[WP_OUT_SCAN + l] = scan[l];
    out[WP_OUT_CLAIM + l] = claimed;
    out[WP_OUT_ACLAIM + l] = slot[l];
  });
  if (W::leader())
  {
    out[WP_OUT_FROM_LANE] = picked;
    out[WP_OUT_UNI32] = u32;
    out[WP_OUT_UNI64] = static_cast<uint32_t>(u64);
    out[WP_OUT_UNI64 + 1] = static_cast<uint32_t>(u64 >> 32);
    out[WP_OUT_BALLOT] = static_cast<uint32_t>(mask);
    out[WP_OUT_BALLOT + 1] = static_cast<uint32_t>(mask >> 32);
    out[WP_OUT_SUM] = sum;
    out[WP_OUT_MAX] = max;
    out[WP_OUT_SCAN_TOTAL] = total;
  }
}
} // namespace gtx
