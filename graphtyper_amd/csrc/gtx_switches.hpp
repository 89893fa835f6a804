// gtx_switches.hpp -- every switch the library reads from the environment: what it accepts, when it is read, who sets it.
// Plain host C++ (the host emulation of tests/emu and stand-alone host programs include it); the only file of this directory
// that asks the environment.  None is needed for normal use.  README.md's switch paragraph is held to the table
// (tests/test_switches.py), the value rules to tests/emu_switches.
//
// read: call = at every call that uses it, ctx = when a context (or its index) is made, team = when a reader team is made,
// once = the first time in a process.
//
//   name                   values                                                        default         read  set by
//   GTX_EXPRESS4           0 = one read per wavefront in pass 1 (and no pass 0);         by the graph    call  test_emu_parity, test_hint_more_shapes,
//                          l(ean) / w(ide) force that build of the four-read pass                              stress_emu, tools/gpu_check.sh
//   GTX_HINT               0 = no position-hinted pass; d(ecline) = it declines all      on              call  tests/emu, tools/long_reads_rate.py
//   GTX_HINT_BUILD         l(ean) / d(ense) force that build of pass 0                   by the graph    call  test_hint_more_shapes, test_hint_windows,
//                                                                                                              test_gpu_parity, stress_emu, tools/diag_legs.sh
//   GTX_HINT_MORE          0 = pass 0 declines the shapes it learnt to prove last        on              call  test_hint_more_shapes
//   GTX_FORCE_SECOND_PASS  1 = every task through all passes, any other number but 0     0               call  test_emu_parity
//                          (2) = every task done by the general pass
//   GTX_HOST_THREADS       n >= 1 (less: 1) threads of the host teams                    by the host     call  test_vcf_text, tools/ab_ctx.sh, tools/ctx_time.py
//   GTX_HALF_BUCKET_CAP    0 .. HALF_BUCKET_CAP (clamped); 0 = the 96 direct probes      HALF_BUCKET_CAP ctx   test_emu_parity
//   GTX_NB_KNOWN           0 = no index slot gets its neighbours-known bit               on              ctx   test_emu_parity
//   GTX_HINT_WINDOWS       n >= 0 (less: 0) allele windows of the dense build at most    16384           ctx   test_hint_windows, hint_tables_*
//   GTX_EXACT_PASS_MB      n > 0 MB of the exact pass' slab (gtx_params wins)            2048 / 4096     ctx   operational
//   GTX_EXACT_PARTS        n > 0 (at most 1024): always that many parts, no large parts  by the slab     ctx   test_emu_parity
//   GTX_INDEX_RUNS         0 = the host lists every k-mer of the index sweep             on              ctx   operational
//   GTX_BUILD_STREAM       0 = contexts are made on the null stream                      on              ctx   operational
//   GTX_TIMING             set = stage times of context making on stderr                 unset           ctx   tools/ctx_stages.py
//   GTX_DEVICE_CACHE_MB    n MB the device memory cache keeps (negative: 0)              32768           once  operational
//   GTX_BIG_GRID_ADAPTIVE  0 = the HBM-table and exact passes are launched whole         on              once  operational
//   GTX_TIME_EVERY         n >= 1 (less: 1): one align call in n is timed                1               once  bench.py
//   GTX_INFLATE            zlib = the BAM readers inflate with zlib                      own decoder     once  test_bam_ingest
//   GTX_BGZF_CRC           0 = no CRC32 check of BGZF members                            on              once  test_bam_ingest, test_tabix
//   GTX_BGZF_THREADS       n >= 0 (less: 0) threads inflate for the readers; 0 = none    up to 16        team  test_bam_ingest, bench.py, tools/inflate_rate.py,
//                                                                                                              tools/pipe_ab.sh, tools/run_extra_leg.py
//   GTX_BGZF_LINGER_US     n >= 0 us an idle worker of that team looks at the queue      300             team  tools/pipe_ab.sh, tools/run_extra_leg.py
//   GTX_BGZF_DEVICE        anything but nothing and 0 = gtx_pipeline_run's readers       off             call  test_gpu_bgzf_inflate
//                          inflate on the device
//   GTX_BGZF_DEVICE_RING   members such a reader keeps in flight (clamped to the ring    256             call  tools/inflate_rate.py
//                          of a host reader .. 65536)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace gtx
{
namespace sw
{
// ---- the three value rules
// on unless the value starts with 0 (unset and empty: on)
inline bool unless_0(char const * name)
{
  char const * e = std::getenv(name);
  return !(e && e[0] == '0');
}
// set to anything, the empty string too
inline bool is_set(char const * name) { return std::getenv(name) != nullptr; }
// a number clamped to [lo, hi]; unset: the default as it is (a value that is no number counts as 0, like atoll)
inline long long number(char const * name, long long unset, long long lo, long long hi = std::numeric_limits<long long>::max())
{
  char const * e = std::getenv(name);
  return e ? std::min(std::max(std::atoll(e), lo), hi) : unset;
}

// ---- one reader per switch (the table above says what they mean)
inline bool hint_more() { return unless_0("GTX_HINT_MORE"); }
inline bool nb_known() { return unless_0("GTX_NB_KNOWN"); }
inline bool index_runs() { return unless_0("GTX_INDEX_RUNS"); }
inline bool build_stream() { return unless_0("GTX_BUILD_STREAM"); }
inline bool big_grid_adaptive() { return unless_0("GTX_BIG_GRID_ADAPTIVE"); }
inline bool bgzf_crc() { return unless_0("GTX_BGZF_CRC"); }
inline bool timing() { return is_set("GTX_TIMING"); }
inline unsigned host_threads() { return static_cast<unsigned>(number("GTX_HOST_THREADS", 0, 1, std::numeric_limits<int>::max())); } // (0: not given)
inline uint32_t half_bucket_cap(uint32_t cap) { return static_cast<uint32_t>(number("GTX_HALF_BUCKET_CAP", cap, 0, cap)); }
inline uint64_t hint_windows() { return static_cast<uint64_t>(number("GTX_HINT_WINDOWS", 16384, 0)); }
inline size_t device_cache_mb() { return static_cast<size_t>(number("GTX_DEVICE_CACHE_MB", 32768, 0)); }
inline uint32_t time_every() { return static_cast<uint32_t>(number("GTX_TIME_EVERY", 1, 1, std::numeric_limits<int>::max())); }
inline unsigned bgzf_threads(unsigned unset) { return static_cast<unsigned>(number("GTX_BGZF_THREADS", unset, 0, std::numeric_limits<int>::max())); }
inline int bgzf_linger_us(int unset) { return static_cast<int>(number("GTX_BGZF_LINGER_US", unset, 0, std::numeric_limits<int>::max())); }
inline unsigned bgzf_device_ring(unsigned host_ring) { return static_cast<unsigned>(number("GTX_BGZF_DEVICE_RING", 256, host_ring, 65536)); }
inline bool bgzf_device()
{
  char const * e = std::getenv("GTX_BGZF_DEVICE");
  return e && e[0] != '\0' && std::strcmp(e, "0") != 0;
}
inline bool inflate_zlib()
{
  char const * e = std::getenv("GTX_INFLATE");
  return e && std::strcmp(e, "zlib") == 0;
}
// the exact pass: the value, or 0 = not given (the library and the host emulation have defaults of their own)
inline uint64_t exact_pass_mb() { return static_cast<uint64_t>(number("GTX_EXACT_PASS_MB", 0, 0)); }
inline uint32_t exact_parts() { return static_cast<uint32_t>(number("GTX_EXACT_PARTS", 0, 0, 1024)); }

// ---- the align call's schedule (gtx_api.hip: align_front; tests/emu: emu_align): five lookups with a position-hinted pass,
//      three without
struct AlignSwitches
{
  enum Build : uint8_t { BY_GRAPH, LEAN, OTHER }; // (OTHER: the wide build of pass 1, the dense build of pass 0)
  uint32_t force = 0;        // GTX_FORCE_SECOND_PASS: 0, 1, or 2 for every other number
  bool four = true;          // pass 1 takes four reads per wavefront
  bool hinted = true;        // there is a pass 0 (never without `four`)
  bool decline_all = false;  // pass 0 declines every task: GTX_HINT=d, or any force
  Build express4 = BY_GRAPH; // the build of pass 1
  Build hint = BY_GRAPH;     // the build of pass 0
  uint32_t hint_less = 0;    // IndexView::hint_less of pass 0
  static bool pick(Build b, bool by_graph) { return b == BY_GRAPH ? by_graph : b == OTHER; }
  bool wide(bool by_graph) const { return pick(express4, by_graph); }
  bool hint_dense(bool by_graph) const { return pick(hint, by_graph); }
};
inline AlignSwitches align_switches()
{
  AlignSwitches s;
  char const * fb = std::getenv("GTX_FORCE_SECOND_PASS");
  int const f = fb ? std::atoi(fb) : 0;
  s.force = f == 0 ? 0u : f == 1 ? 1u : 2u;
  char const * e4 = std::getenv("GTX_EXPRESS4");
  char const * eh = std::getenv("GTX_HINT");
  s.four = !(e4 && e4[0] == '0');
  s.hinted = s.four && !(eh && eh[0] == '0');
  s.decline_all = s.hinted && (s.force != 0 || (eh && eh[0] == 'd'));
  s.express4 = e4 && e4[0] == 'w' ? AlignSwitches::OTHER : e4 && e4[0] == 'l' ? AlignSwitches::LEAN : AlignSwitches::BY_GRAPH;
  if (s.hinted)
  {
    char const * hb = std::getenv("GTX_HINT_BUILD");
    s.hint = hb && hb[0] == 'd' ? AlignSwitches::OTHER : hb && hb[0] == 'l' ? AlignSwitches::LEAN : AlignSwitches::BY_GRAPH;
    s.hint_less = hint_more() ? 0u : 1u;
  }
  return s;
}
} // namespace sw
} // namespace gtx
