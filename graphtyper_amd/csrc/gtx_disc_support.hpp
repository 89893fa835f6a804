// gtx_disc_support.hpp -- what the first pass of discovery does to ONE event's support, as text that the host stage
// (first_pass_state) and the device walk (gtx_disc_walk_kernel) both compile: the accumulation step of an event of a read
// (caller.cpp:583-775 through add_snp_event_to_bucket / add_indel_event_to_bucket), the correction for reads with 12 and more
// events (caller.cpp:777-822), and the two support filters (event.cpp:226-256, caller.cpp:990-1186).  The counters are 32 bits
// wide and are wrapped to the reference's 16 where they are read.  The filters work in doubles: contraction is off in them,
// so that the device's bits are the host's (no fused multiply-add where the host has a multiply and an add).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gtx
{
struct DiscCounters // the counted part of EventSupport (event.hpp:75-113)
{
  uint32_t hq = 0, lq = 0, proper = 0, first = 0, reversed = 0, clipped = 0;
  uint8_t max_mapq = 0, max_distance = 0;
  int32_t u1 = -1, u2 = -1, u3 = -1;
};

__host__ __device__ inline uint16_t disc_wrap16(uint32_t v) { return static_cast<uint16_t>(v); } // (the reference's counters are uint16_t and wrap)

// one event of a read joins its support; `clipped`: is_clipped of the read (caller.cpp:167-196)
__host__ __device__ inline void disc_accumulate(DiscCounters & s, uint8_t type, uint8_t hq, uint16_t max_distance, int32_t read_pos, uint16_t flag,
                                                uint8_t mapq, bool clipped)
{
  if (type == 'X')
  {
    if (hq)
      ++s.hq;
    else
      ++s.lq;
    s.first += (flag & 64u) != 0;
    if (s.u1 == -1)
      s.u1 = read_pos;
    else if (s.u2 == -1)
    {
      if (s.u1 != read_pos)
        s.u2 = read_pos;
    }
    else if (s.u3 == -1 && s.u2 != read_pos)
      s.u3 = read_pos;
    if (static_cast<long>(max_distance) > static_cast<long>(s.max_distance))
      s.max_distance = static_cast<uint8_t>(max_distance);
  }
  else
    ++s.hq;
  if (mapq != 255 && mapq > s.max_mapq)
    s.max_mapq = mapq;
  s.proper += (flag & 2u) != 0;
  s.reversed += (flag & 16u) != 0;
  s.clipped += clipped;
}

// a read with n_events >= 12 events takes its support back, once per event of its own (caller.cpp:777-822)
__host__ __device__ inline void disc_many_events(DiscCounters & s, uint32_t n_events)
{
  if (n_events >= 18)
  {
    if (disc_wrap16(s.hq) > 0)
      --s.hq;
    else if (disc_wrap16(s.lq) > 0)
      --s.lq;
  }
  else if (disc_wrap16(s.hq) > 0)
  {
    --s.hq;
    ++s.lq;
  }
}

// EventSupport::has_good_support with the default Options (event.cpp:226-256)
__host__ __device__ inline bool disc_good_snp(DiscCounters const & s, long cov)
{
#pragma clang fp contract(off)
  cov = cov > 1 ? cov : 1;
  int const hq = disc_wrap16(s.hq), raw = disc_wrap16(s.hq) + disc_wrap16(s.lq), pp = disc_wrap16(s.proper), fip = disc_wrap16(s.first),
            rev = disc_wrap16(s.reversed), cl = disc_wrap16(s.clipped);
  double const ratio = static_cast<double>(raw) / static_cast<double>(cov);
  bool const very = s.u3 != -1 && ((hq >= 8 && ratio >= 0.35) || (hq >= 7 && ratio >= 0.40)) && pp >= 6;
  bool const prom = s.u3 != -1 && ((hq >= 7 && ratio >= 0.20) || (hq >= 6 && ratio >= 0.30) || (hq >= 5 && ratio >= 0.40)) && pp >= 4;
  return s.u2 != -1 && pp >= 2 && hq >= 3 && (prom || (fip > 0 && fip < raw)) && (very || (prom && rev > 0 && rev < raw) || (rev > 1 && rev < raw - 1)) &&
         (cl <= 1 || cl + 5 <= raw) && (s.max_distance >= 10 || (prom && hq >= 10)) && (hq + (raw - hq) / 2.0) >= 3.9 && (ratio > 0.26 || prom);
}

// the window of an indel's coverage (caller.cpp:1003-1040): region-relative [lo, hi]
__host__ __device__ inline void disc_indel_window(long pos, uint32_t len, uint32_t span, long begin, long REF, long & lo, long & hi)
{
#pragma clang fp contract(off)
  long const pad = static_cast<long>(4.0 + static_cast<double>(len) / 3.0);
  lo = pos - pad - begin;
  lo = lo > 0 ? lo : 0;
  hi = pos + static_cast<long>(span) + pad - begin;
  hi = hi < REF ? hi : REF;
}

// an indel behind its coverage (caller.cpp:1040-1186): 2 good support (and worth a realignment), 1 worth a realignment, 0 dropped;
// log_qual: get_log_qual_double (event.cpp:102-113)
__host__ __device__ inline int disc_indel_class(DiscCounters const & s, bool insertion, uint32_t length, long cov, uint32_t & log_qual)
{
#pragma clang fp contract(off)
  double const len = static_cast<double>(length);
  double const count = (insertion ? (len / 2.0 + 8.0) / 8.0 : (len / 3.0 + 10.0) / 10.0) * (disc_wrap16(s.hq) + disc_wrap16(s.lq));
  double const dcov = static_cast<double>(cov);
  double const corrected = dcov > count ? dcov : count, anti = corrected - count;
  double const gt00 = count * 10.0, both = count + anti, ten = anti * 10.0, gt_alt = ten < both ? ten : both;
  log_qual = gt00 > gt_alt ? static_cast<uint32_t>(gt00 - gt_alt + 0.5) : 0u;
  int const hq = disc_wrap16(s.hq), rev = disc_wrap16(s.reversed), pp = disc_wrap16(s.proper), cl = disc_wrap16(s.clipped);
  if (hq >= 6 && count >= 8.0 && log_qual >= 60 && rev > 0 && rev < hq && pp >= 3 && s.max_mapq >= 20 && (cl == 0 || cl + 3 <= hq))
    return 2;
  if (count >= 3.0 && log_qual > 0 && pp >= 1 && (hq >= 5 || s.max_mapq >= 25) && s.max_mapq >= 10 && cl < hq)
    return 1;
  return 0;
}
} // namespace gtx
