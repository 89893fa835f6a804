// wave_seq.hpp -- TEST HARNESS ONLY: the sequential side of the wave policy the kernel sources are written against (the contract is
// the table at the head of graphtyper_amd/csrc/graph_dev.hpp; the hardware side is wave_hip.hpp).  One wavefront, run by one host
// thread: every `lanes` call runs lane 0..63 to completion in order, the text outside the lambdas runs once, per-lane values are
// arrays of 64.  Every tests/emu* program instantiates the kernels' text with this type (or a type derived from it for what is its
// own), tests/emu_wave holds it to the contract primitive by primitive.  Plain C++: no HIP, nothing of the library includes it.
#pragma once
#include <cstdint>

namespace gtx
{
struct WaveSeq
{
  template <class T>
  struct PerLane
  {
    T v[64];
    T & operator[](uint32_t l) { return v[l]; }
    T const & operator[](uint32_t l) const { return v[l]; }
  };
  template <class F>
  static void lanes(F && f)
  {
    for (uint32_t l = 0; l < 64; ++l)
      f(l);
  }
  static bool leader() { return true; }
  template <class T>
  static T uni(T v)
  {
    return v;
  }
  static uint32_t from_lane(PerLane<uint32_t> const & p, uint32_t lane) { return p.v[lane]; }
  static uint64_t ballot(PerLane<bool> const & p)
  {
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; ++l)
      m |= static_cast<uint64_t>(p.v[l] ? 1u : 0u) << l;
    return m;
  }
  static uint32_t sum(PerLane<uint32_t> const & p)
  {
    uint32_t s = 0;
    for (uint32_t l = 0; l < 64; ++l)
      s += p.v[l];
    return s;
  }
  static uint32_t max(PerLane<uint32_t> const & p)
  {
    uint32_t x = p.v[0];
    for (uint32_t l = 1; l < 64; ++l)
      x = p.v[l] > x ? p.v[l] : x;
    return x;
  }
  static void excl_scan(PerLane<uint32_t> const & in, PerLane<uint32_t> & out, uint32_t & total)
  {
    uint32_t s = 0;
    for (uint32_t l = 0; l < 64; ++l)
    {
      uint32_t const x = in.v[l]; // (read before the write: in and out may be one object)
      out.v[l] = s;
      s += x;
    }
    total = s;
  }
  // from the top down, so that in and out may be one object (the aligners: W::shift_up(base, ..., base))
  static void shift_up(PerLane<uint32_t> const & in, uint32_t first, PerLane<uint32_t> & out)
  {
    for (uint32_t l = 63; l > 0; --l)
      out.v[l] = in.v[l - 1];
    out.v[0] = first;
  }
  // one wavefront's lanes run on one thread, in order: nothing to order
  static void lds_sync() {}
  static void mem_sync() {}
  // relaxed __atomic_*: the threaded library of tests/emu runs a wave per thread over shared counters, the stand-alone programs run one
  static void atomic_add_u32(uint32_t * p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
  static void atomic_add_u64(unsigned long long * p, unsigned long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
  static void atomic_sub_u32(uint32_t * p, uint32_t v) { __atomic_fetch_sub(p, v, __ATOMIC_RELAXED); }
  static void atomic_max_u32(uint32_t * p, uint32_t v)
  {
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
    {
    }
  }
  static void atomic_max_i32(int32_t * p, int32_t v)
  {
    int32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
    {
    }
  }
  static void atomic_or_u32(uint32_t * p, uint32_t v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
  static void atomic_or_u64(uint64_t * p, uint64_t v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
  // outside `lanes`: the wave takes n, the one value is every lane's
  static uint32_t claim_u32(uint32_t * p, uint32_t n) { return __atomic_fetch_add(p, n, __ATOMIC_RELAXED); }
  // inside `lanes`: one slot per calling lane; the lanes run in order, so the slots are consecutive in lane order
  static uint32_t atomic_claim_u32(uint32_t * p) { return __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED); }
  static unsigned long long clock() { return 0; }
};
} // namespace gtx
