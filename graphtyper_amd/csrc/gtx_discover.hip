// gtx_discover.hip -- first slice of variant discovery: the per-sample first pass over the reads of a
// region, run_first_pass (src/typer/caller.cpp:488-1186).
//
// Device: gtx_disc_events_kernel, one read per lane.  A read's CIGAR is walked against the region's reference held as bit
// planes (the layout of the alignment kernels' reads, graph_dev.hpp): an M block of 32 bases is four XORs and two one-hot
// tests, a mismatch of two unambiguous bases is a set bit, and every set bit is one SNP event; I and D operations give indel
// events when their bases are all A/C/G/T (one-hot over the range).  Events leave in the read's CIGAR order: every lane
// counts first, a wavefront claims one contiguous piece of the output with one atomic, the lanes write behind each other.
// Host: gtx_disc_first_pass keeps what is order-dependent in the reference -- which read sees an event first (span, the
// three distinct start positions), the correction for reads with 12 and more events, the phase counts between the events
// of a read -- by going over the reads in stream order, then applies the two support filters over the coverage arrays.
// gtx_disc_first_pass_haplotypes takes the pass to its end (the sample's haplotype map, :1186-1365), gtx_disc_merge puts the files'
// results together (merge_haplotypes2 :64-165, the union of the indels :2853-2903).
// Device again: gtx_disc_first_pass_device does the host stage's work up to and including the filters over the device arrays
// (sort by event, one lane per distinct event in read order, a second sort for the phase counts; the second half of this file),
// with the accumulation step and the filters of gtx_disc_support.hpp, which the host stage calls too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <map>
#include <set>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_devmem.hpp"
#include "gtx_devprim.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_region.hpp"
#include "gtx_disc_events_dev.hpp"
#include "gtx_disc_second_dev.hpp"
#include "gtx_disc_support.hpp"
#include "wave_hip.hpp"

namespace
{
using namespace gtx;

__global__ __launch_bounds__(256) void gtx_disc_events_kernel(uint32_t const * __restrict__ refp, uint32_t ref_groups, long REF_SIZE, long region_begin,
                                                              uint8_t const * __restrict__ rows, uint32_t plane_stride, uint8_t const * __restrict__ qual,
                                                              uint32_t qual_stride, gtx_disc_read const * __restrict__ reads,
                                                              uint32_t const * __restrict__ cigar, uint32_t n_reads, gtx_disc_event * __restrict__ events,
                                                              uint32_t event_cap, uint32_t * counts, gtx_disc_read_out * __restrict__ read_out)
{
  disc_events_wave<WaveHip>(DiscBatch{refp, ref_groups, REF_SIZE, region_begin, rows, plane_stride, qual, qual_stride, reads, cigar, n_reads, events, event_cap,
                                      counts, read_out},
                            blockIdx.x * blockDim.x + (threadIdx.x & ~63u));
}
} // namespace

extern "C" int gtx_disc_create(const char * reference, uint64_t reference_len, int64_t region_begin, int device, gtx_disc ** out)
{
  if (!reference || !out || reference_len == 0 || reference_len > 0x7FFFFFFFull)
  {
    g_last_error = "gtx_disc_create: bad argument";
    return GTX_ERR_ARG;
  }
  *out = nullptr;
  if (device == -1) // like gtx_ctx_create's -1: an object for the host stages only (the bookkeeping over events a device made elsewhere);
  {                 // gtx_disc_events_batch refuses it -- the library has no CPU path for the walk over the CIGARs (tests/emu_disc_events runs its text)
    auto h = std::make_unique<gtx_disc>();
    h->device = -1;
    h->region_begin = region_begin;
    h->reference.assign(reference, reference_len);
    *out = h.release();
    return GTX_OK;
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
  {
    g_last_error = "gtx_disc_create: no such HIP device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  auto d = std::make_unique<gtx_disc>();
  d->device = device;
  d->region_begin = region_begin;
  d->reference.assign(reference, reference_len);
  d->ref_groups = disc_ref_groups(reference_len);
  std::vector<uint32_t> planes(static_cast<size_t>(d->ref_groups) * 4, 0);
  disc_ref_planes(reference, reference_len, planes.data());
  std::vector<uint32_t> planes5(static_cast<size_t>(d->ref_groups) * disc_second_dev::REF_PLANES, 0);
  disc_second_ref_planes(reference, reference_len, planes5.data());
  if (hipSetDevice(device) != hipSuccess || !alloc(d->d_refp, planes.size() * 4) ||
      hipMemcpy(d->d_refp.get(), planes.data(), planes.size() * 4, hipMemcpyHostToDevice) != hipSuccess || !alloc(d->d_refc, reference_len) ||
      hipMemcpy(d->d_refc.get(), reference, reference_len, hipMemcpyHostToDevice) != hipSuccess || !alloc(d->d_ref5, planes5.size() * 4) ||
      hipMemcpy(d->d_ref5.get(), planes5.data(), planes5.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
  {
    g_last_error = "gtx_disc_create: upload of the reference failed";
    return GTX_ERR_HIP;
  }
  *out = d.release();
  return GTX_OK;
}

void gtx::disc_region(gtx_disc const * d, char const ** reference, uint64_t * reference_len, int64_t * region_begin) // (gtx_disc_region.hpp)
{
  *reference = d->reference.data();
  *reference_len = d->reference.size();
  *region_begin = d->region_begin;
}

extern "C" void gtx_disc_destroy(gtx_disc * d)
{
  if (!d)
    return;
  if (d->d_refp)
  {
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    d->d_refp.reset();
    d->d_refc.reset();
    d->d_ref5.reset();
  }
  delete d;
}

extern "C" int gtx_disc_events_batch(gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const uint8_t * d_qual, uint32_t qual_stride,
                                     const gtx_disc_read * d_reads, const uint32_t * d_cigar, uint32_t n_reads, gtx_disc_event * d_events,
                                     uint32_t event_cap, uint32_t * d_counts, gtx_disc_read_out * d_read_out, void * stream)
{
  if (!d || plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0 || (reinterpret_cast<uintptr_t>(d_planes) & 3u) != 0 ||
      (n_reads != 0 && (!d_planes || !d_qual || !d_reads || !d_cigar || !d_counts || !d_read_out || (event_cap && !d_events))))
  {
    g_last_error = "gtx_disc_events_batch: bad argument";
    return GTX_ERR_ARG;
  }
  if (int const rc = device_ready(d->device, "gtx_disc_events_batch: the object"))
    return rc;
  if (n_reads == 0)
    return GTX_OK;
  hipLaunchKernelGGL(gtx_disc_events_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), d->d_refp.get(), d->ref_groups,
                     static_cast<long>(d->reference.size()), static_cast<long>(d->region_begin), d_planes, plane_stride, d_qual, qual_stride, d_reads,
                     d_cigar, n_reads, d_events, event_cap, d_counts, d_read_out);
  if (hipGetLastError() != hipSuccess)
  {
    g_last_error = "gtx_disc_events_kernel launch failed";
    return GTX_ERR_HIP;
  }
  return GTX_OK;
}

// ---- host: the order-dependent bookkeeping and the filters --------------------------------------------------------------
namespace
{
struct Ev // Event (include/graphtyper/typer/event.hpp:30-73) with its ordering (src/typer/event.cpp:198-207)
{
  uint32_t pos;
  uint8_t type;
  std::string seq;
  bool operator<(Ev const & o) const
  {
    int const a = (type == 'D') + 2 * (type == 'X'), b = (o.type == 'D') + 2 * (o.type == 'X');
    if (pos != o.pos)
      return pos < o.pos;
    if (a != b)
      return a < b;
    return seq < o.seq;
  }
};

struct Support : DiscCounters // EventSupport (event.hpp:75-113): what the first pass fills
{
  uint16_t span = 1;
  bool realign = false, good = false;
  uint32_t max_log_qual = 0;
  int32_t file_i = 0; // max_log_qual_file_i: the file whose reads gave max_log_qual
  std::map<Ev, uint16_t> phase;
};

struct PassState // what run_first_pass has when its two filters are through
{
  std::vector<std::map<Ev, Support>> buckets;
  std::vector<uint32_t> up, down; // cov_up / cov_down
  long REF = 0, B = 0, begin = 0;
};

uint16_t wrap16(uint32_t v) { return disc_wrap16(v); }
} // namespace

// run_first_pass up to and including its two support filters (caller.cpp:488-1186) from the device's events
static int first_pass_state(const gtx_disc * d, const gtx_disc_read * reads, const uint32_t * cigar, const gtx_disc_read_out * read_out, uint32_t n_reads,
                            const gtx_disc_event * events, uint64_t n_events, const uint8_t * seq, uint32_t seq_stride, uint32_t bucket_size,
                            int32_t file_index, PassState & state)
{
  std::string const & ref = d->reference;
  long const REF = static_cast<long>(ref.size()), B = bucket_size, begin = d->region_begin;
  state.REF = REF;
  state.B = B;
  state.begin = begin;
  std::vector<std::map<Ev, Support>> & buckets = state.buckets;
  state.up.assign(REF, 0);
  state.down.assign(REF, 0);
  std::vector<uint32_t> &up = state.up, &down = state.down;
  static char const NT16[] = "=ACMGRSVTWYHKDBN";
  auto bucket_of = [&](uint32_t pos) -> std::map<Ev, Support> &
  {
    size_t const b = static_cast<size_t>((static_cast<long>(pos) - begin) / B);
    if (b >= buckets.size())
      buckets.resize(b + 1);
    return buckets[b];
  };
  std::vector<std::map<Ev, Support>::iterator> mine;
  for (uint32_t i = 0; i < n_reads; ++i)
  {
    gtx_disc_read const & r = reads[i];
    gtx_disc_read_out const & ro = read_out[i];
    if (ro.state == GTX_DISC_SKIPPED)
      continue;
    size_t const start_bucket = static_cast<size_t>((static_cast<long>(r.pos) - begin) / B);
    if (start_bucket >= buckets.size())
      buckets.resize(start_bucket + 1); // (caller.cpp:546-548: before the end-of-region test)
    if (ro.state == GTX_DISC_END)
      break;
    if (static_cast<uint64_t>(ro.first_event) + ro.n_events > n_events)
    {
      g_last_error = "gtx_disc_first_pass: a read's events lie behind the event buffer (it overflowed: event_cap too small)";
      return GTX_ERR_CAPACITY;
    }
    uint32_t const front = cigar[r.cigar_off], back = cigar[r.cigar_off + r.n_cigar - 1];
    bool const clipped = ((front & 15u) == 4 && (front >> 4) >= 1) || ((back & 15u) == 4 && (back >> 4) >= 1); // is_clipped (caller.cpp:167-196)
    mine.clear();
    for (uint32_t k = 0; k < ro.n_events; ++k)
    {
      gtx_disc_event const & e = events[ro.first_event + k];
      Ev ev{e.pos, e.type, {}};
      long const ref_offset = static_cast<long>(e.pos) - begin;
      if (e.type == 'X')
        ev.seq.assign(1, static_cast<char>(e.seq));
      else if (e.type == 'I')
      {
        uint8_t const * row = seq + static_cast<uint64_t>(i) * seq_stride;
        for (uint32_t j = 0; j < e.len; ++j)
        {
          uint32_t const at = e.seq + j;
          ev.seq.push_back(NT16[(row[at >> 1] >> ((~at & 1u) << 2)) & 15u]);
        }
      }
      else
        ev.seq = ref.substr(e.seq, e.len);
      auto ins = bucket_of(e.pos).insert({std::move(ev), Support()});
      Support & s = ins.first->second;
      if (ins.second && e.type != 'X') // span of a new indel (bucket.cpp:100-160)
      {
        std::string const & q = ins.first->first.seq;
        long span = 0, count = static_cast<long>(q.size());
        if (e.type == 'I')
        {
          while (span < count && ref_offset + span < REF && q[span] == ref[ref_offset + span])
            ++span;
          if (span == count)
            while (ref_offset + span < REF && ref[ref_offset + span - count] == ref[ref_offset + span])
              ++span;
        }
        else
          while (ref_offset + span < REF && ref_offset + span + count < REF && ref[ref_offset + span] == ref[ref_offset + span + count])
            ++span;
        s.span = static_cast<uint16_t>(std::min<long>(span, std::numeric_limits<uint16_t>::max() - 1) + 1); // (bucket.cpp:128-131, 156-159)
      }
      disc_accumulate(s, e.type, e.hq, e.max_distance, r.pos, r.flag, r.mapq, clipped); // (shared with the device walk)
      mine.push_back(ins.first);
    }
    // reads with many events (caller.cpp:777-822)
    if (mine.size() >= 12)
      for (auto & it : mine)
        disc_many_events(it->second, static_cast<uint32_t>(mine.size()));
    if (mine.size() < 18)
      for (size_t b2 = 1; b2 < mine.size(); ++b2)
        for (size_t a = 0; a < b2; ++a)
          ++mine[a]->second.phase.insert({mine[b2]->first, 0}).first->second;
    ++up[static_cast<long>(r.pos) - begin];
    ++down[ro.pos_end];
  }
  if ((static_cast<long>(buckets.size()) - 1) * B >= REF)
    buckets.resize((REF - 1) / B + 1);
  long const NB = static_cast<long>(buckets.size());
  auto delta = [&](long o) { return static_cast<long>(up[o]) - static_cast<long>(down[o]); };
  // SNPs with low support (caller.cpp:897-985)
  {
    long depth = 0;
    for (long b = 0; b < NB; ++b)
    {
      for (auto it = buckets[b].begin(); it != buckets[b].end();)
      {
        if (it->first.type != 'X')
        {
          ++it;
          continue;
        }
        long cov = depth;
        long const at = std::max(0l, static_cast<long>(it->first.pos) - begin);
        if (at + 1 > b * B)
          for (long o = b * B; o <= at; ++o)
            cov += delta(o);
        if (disc_good_snp(it->second, cov))
          ++it;
        else
          it = buckets[b].erase(it);
      }
      if (b * B >= REF)
        break;
      for (long o = b * B, e = std::min(REF, (b + 1) * B); o < e; ++o)
        depth += delta(o);
    }
  }
  // indels: good support, worth a realignment, or dropped (caller.cpp:990-1186)
  long depth = 0;
  for (long b = 0; b < NB; ++b)
  {
    for (auto it = buckets[b].begin(); it != buckets[b].end();)
    {
      if (it->first.type == 'X')
      {
        ++it;
        continue;
      }
      Support & s = it->second;
      uint32_t const len = static_cast<uint32_t>(it->first.seq.size());
      long lo = 0, hi = 0;
      disc_indel_window(static_cast<long>(it->first.pos), len, s.span, begin, REF, lo, hi);
      long cov = depth, o = lo;
      if (o <= b * B)
        for (; o < b * B; ++o)
          cov -= delta(o);
      else
        for (o = b * B; o < lo; ++o)
          cov += delta(o);
      for (; o <= hi; ++o)
        cov -= o < REF ? static_cast<long>(down[o]) : 0l;
      uint32_t log_qual = 0;
      int const verdict = disc_indel_class(s, it->first.type == 'I', len, cov, log_qual); // (shared with the device walk)
      if (verdict == 2)
      {
        s.good = s.realign = true;
        s.max_log_qual = log_qual;
        s.file_i = file_index;
        ++it;
      }
      else if (verdict == 1)
      {
        s.realign = true;
        s.max_log_qual = log_qual;
        s.file_i = file_index;
        ++it;
      }
      else
        it = buckets[b].erase(it);
    }
    if (b * B >= REF)
      break;
    for (long o = b * B, e = std::min(REF, (b + 1) * B); o < e; ++o)
      depth += delta(o);
  }
  return GTX_OK;
}

namespace
{
void put_ev(std::vector<uint32_t> & w, Ev const & e)
{
  w.push_back(e.pos);
  w.push_back(e.type);
  w.push_back(static_cast<uint32_t>(e.seq.size()));
  for (char c : e.seq)
    w.push_back(static_cast<uint32_t>(static_cast<unsigned char>(c)));
}

// an event with its support: the fields, (the file of the best support,) the phase entries
void put_support(std::vector<uint32_t> & w, Ev const & e, Support const & s, bool with_file)
{
  put_ev(w, e);
  for (uint32_t v : {uint32_t(wrap16(s.hq)), uint32_t(wrap16(s.lq)), uint32_t(wrap16(s.proper)), uint32_t(wrap16(s.first)), uint32_t(wrap16(s.reversed)),
                     uint32_t(wrap16(s.clipped)), uint32_t(s.max_mapq), uint32_t(s.max_distance), uint32_t(s.u1), uint32_t(s.u2), uint32_t(s.u3),
                     uint32_t(s.span), uint32_t(s.realign), uint32_t(s.good), s.max_log_qual})
    w.push_back(v);
  if (with_file)
    w.push_back(static_cast<uint32_t>(s.file_i));
  w.push_back(static_cast<uint32_t>(s.phase.size()));
  for (auto const & ph : s.phase)
  {
    put_ev(w, ph.first);
    w.push_back(ph.second);
  }
}

int hand_over(std::vector<uint32_t> const & w, uint32_t * out, uint64_t cap, uint64_t * n_words)
{
  *n_words = w.size();
  if (w.size() <= cap && !w.empty())
    std::memcpy(out, w.data(), w.size() * 4);
  return w.size() <= cap ? GTX_OK : GTX_ERR_CAPACITY;
}

// HaplotypeInfo (caller.cpp:45-52): the events an event is seen with -- in some sample, in every sample that has it
struct Together
{
  std::set<Ev> ever, always;
};

struct FileResult // what a file (or several, merged) leaves behind: Tindel_events and the haplotype map
{
  std::map<Ev, Support> indels;
  std::map<Ev, Together> haplotypes;
};

void put_result(std::vector<uint32_t> & w, FileResult const & r)
{
  w.push_back(static_cast<uint32_t>(r.indels.size()));
  for (auto const & kv : r.indels)
    put_support(w, kv.first, kv.second, true);
  w.push_back(static_cast<uint32_t>(r.haplotypes.size()));
  for (auto const & kv : r.haplotypes)
  {
    put_ev(w, kv.first);
    for (std::set<Ev> const * set : {&kv.second.ever, &kv.second.always})
    {
      w.push_back(static_cast<uint32_t>(set->size()));
      for (Ev const & e : *set)
        put_ev(w, e);
    }
  }
}

bool read_result(uint32_t const * w, uint64_t n, FileResult & r)
{
  uint64_t at = 0;
  bool ok = true;
  auto word = [&]() -> uint32_t
  {
    if (at >= n)
    {
      ok = false;
      return 0;
    }
    return w[at++];
  };
  auto event = [&]()
  {
    Ev e;
    e.pos = word();
    e.type = static_cast<uint8_t>(word());
    uint32_t const len = word();
    if (!ok || len > n - at)
    {
      ok = false;
      return e;
    }
    for (uint32_t k = 0; k < len; ++k)
      e.seq.push_back(static_cast<char>(w[at + k]));
    at += len;
    return e;
  };
  if (n == 0)
    return true;
  for (uint32_t i = 0, m = word(); ok && i < m; ++i)
  {
    Ev e = event();
    Support s;
    s.hq = word(); s.lq = word(); s.proper = word(); s.first = word(); s.reversed = word(); s.clipped = word();
    s.max_mapq = static_cast<uint8_t>(word()); s.max_distance = static_cast<uint8_t>(word());
    s.u1 = static_cast<int32_t>(word()); s.u2 = static_cast<int32_t>(word()); s.u3 = static_cast<int32_t>(word());
    s.span = static_cast<uint16_t>(word()); s.realign = word() != 0; s.good = word() != 0; s.max_log_qual = word();
    s.file_i = static_cast<int32_t>(word());
    for (uint32_t k = 0, np = word(); ok && k < np; ++k)
    {
      Ev pe = event();
      s.phase[pe] = static_cast<uint16_t>(word());
    }
    r.indels.insert({std::move(e), std::move(s)});
  }
  for (uint32_t i = 0, m = word(); ok && i < m; ++i)
  {
    Ev e = event();
    Together t;
    for (std::set<Ev> * set : {&t.ever, &t.always})
      for (uint32_t k = 0, ns = word(); ok && k < ns; ++k)
        set->insert(event());
    r.haplotypes.insert({std::move(e), std::move(t)});
  }
  return ok && at == n;
}
} // namespace

extern "C" int gtx_disc_first_pass(const gtx_disc * d, const gtx_disc_read * reads, const uint32_t * cigar, const gtx_disc_read_out * read_out,
                                   uint32_t n_reads, const gtx_disc_event * events, uint64_t n_events, const uint8_t * seq, uint32_t seq_stride,
                                   uint32_t bucket_size, uint32_t * out, uint64_t cap, uint64_t * n_words)
{
  if (!d || !n_words || bucket_size == 0 || (n_reads && (!reads || !cigar || !read_out || !seq)) || (n_events && !events) || (cap && !out))
  {
    g_last_error = "gtx_disc_first_pass: bad argument";
    return GTX_ERR_ARG;
  }
  PassState st;
  int const rc = first_pass_state(d, reads, cigar, read_out, n_reads, events, n_events, seq, seq_stride, bucket_size, 0, st);
  if (rc != GTX_OK)
    return rc;
  // the surviving events as a word stream: pos, type, length, characters, the support fields, the phase entries
  std::vector<uint32_t> w;
  for (auto const & bucket : st.buckets)
    for (auto const & kv : bucket)
      put_support(w, kv.first, kv.second, false);
  return hand_over(w, out, cap, n_words);
}

static int haplotypes_of(PassState & st, uint32_t * out, uint64_t cap, uint64_t * n_words);

// run_first_pass to its end (caller.cpp:1186-1365): for every event that is left, which later events within two buckets it
// travels with -- "ever": in enough of the reads that cover both (by its phase counts and the coverage between the two; any
// shared read when one of them is an indel), "always": those of them at most ten positions on -- the sample's haplotype map;
// the SNPs then leave the buckets.  Output: the file's result (put_result: indels with their support, the haplotype map).
extern "C" int gtx_disc_first_pass_haplotypes(const gtx_disc * d, const gtx_disc_read * reads, const uint32_t * cigar, const gtx_disc_read_out * read_out,
                                              uint32_t n_reads, const gtx_disc_event * events, uint64_t n_events, const uint8_t * seq, uint32_t seq_stride,
                                              uint32_t bucket_size, int32_t file_index, uint32_t * out, uint64_t cap, uint64_t * n_words)
{
  if (!d || !n_words || bucket_size == 0 || (n_reads && (!reads || !cigar || !read_out || !seq)) || (n_events && !events) || (cap && !out))
  {
    g_last_error = "gtx_disc_first_pass_haplotypes: bad argument";
    return GTX_ERR_ARG;
  }
  PassState st;
  int const rc = first_pass_state(d, reads, cigar, read_out, n_reads, events, n_events, seq, seq_stride, bucket_size, file_index, st);
  if (rc != GTX_OK)
    return rc;
  return haplotypes_of(st, out, cap, n_words);
}

// (the state behind the two filters may come from first_pass_state or from the device's survivors: gtx_disc_first_pass_haplotypes_device)
static int haplotypes_of(PassState & st, uint32_t * out, uint64_t cap, uint64_t * n_words)
{
  long const REF = st.REF, B = st.B, begin = st.begin, NB = static_cast<long>(st.buckets.size());
  auto delta = [&](long o) { return static_cast<long>(st.up[o]) - static_cast<long>(st.down[o]); };
  FileResult res;
  long depth = 0;
  for (long b = 0; b < NB; ++b)
  {
    auto & bucket = st.buckets[b];
    for (auto it = bucket.begin(); it != bucket.end();)
    {
      Ev const & ev = it->first;
      Support const & info = it->second;
      long const at = std::max(0l, static_cast<long>(ev.pos) - begin);
      long cov = depth;
      if (at + 1 > b * B)
        for (long o = b * B; o <= at; ++o)
          cov += delta(o);
      Together & tg = res.haplotypes.insert({ev, Together()}).first->second;
      double ratio = static_cast<double>(wrap16(info.hq) + wrap16(info.lq)) / static_cast<double>(cov);
      if (ratio < 0.3)
        ratio = 0.3;
      // 1: seen together, 2: seen apart (caller.cpp:1216-1268; 0: too little coverage to say)
      auto judge = [&](Ev const & other) -> int
      {
        auto const ph = info.phase.find(other);
        if (ev.type != 'X' || other.type != 'X')
          return (ph == info.phase.end() || ph->second == 0) ? 2 : 3;
        long local = cov;
        for (long o = at + 1, last = std::max(0l, static_cast<long>(other.pos) - begin); o <= last; ++o)
          local -= o < REF ? static_cast<long>(st.down[o]) : 0l;
        if (local <= 2)
          return 0;
        double const support = ph == info.phase.end() ? 0.0 : ph->second;
        if ((support / static_cast<double>(local) / ratio) < 0.22)
          return 2;
        if ((support / static_cast<double>(local) / ratio) > 0.78)
          return 1;
        return 3;
      };
      auto look = [&](Ev const & other, bool may_be_always)
      {
        if (judge(other) & 1)
        {
          tg.ever.insert(other);
          if (may_be_always && other.pos <= ev.pos + 10)
            tg.always.insert(other);
        }
      };
      for (auto it2 = std::next(it); it2 != bucket.end(); ++it2)
        if (!(it2->first.pos == ev.pos && it2->first.type == ev.type)) // (alleles of one place exclude each other)
          look(it2->first, true);
      if (b + 1 < NB)
        for (auto const & kv : st.buckets[b + 1])
          look(kv.first, true);
      if (b + 2 < NB)
        for (auto const & kv : st.buckets[b + 2])
        {
          if (kv.first.pos >= ev.pos + 2 * B)
            break;
          look(kv.first, false);
        }
      if (ev.type == 'X')
        it = bucket.erase(it);
      else
        ++it;
    }
    if (b * B >= REF)
      break;
    for (long o = b * B, e = std::min(REF, (b + 1) * B); o < e; ++o)
      depth += delta(o);
  }
  for (auto & bucket : st.buckets)
    for (auto & kv : bucket)
      res.indels.insert(kv);
  std::vector<uint32_t> w;
  put_result(w, res);
  return hand_over(w, out, cap, n_words);
}

// The results of two files (or of files merged before) as one: merge_haplotypes2 (caller.cpp:64-165) -- an event new to `into`
// keeps of its "always" set what `into` has never seen; one known to both has the union of the "ever" sets and the
// intersection of the "always" sets -- and the union of the indels (streamlined_discovery, :2853-2903: good support from any
// file, the best max_log_qual with its file).  `into` may be empty.  Files are merged in their order.
extern "C" int gtx_disc_merge(const uint32_t * into, uint64_t n_into, const uint32_t * from, uint64_t n_from, uint32_t * out, uint64_t cap,
                              uint64_t * n_words)
{
  if (!n_words || (n_into && !into) || (n_from && !from) || (cap && !out))
  {
    g_last_error = "gtx_disc_merge: bad argument";
    return GTX_ERR_ARG;
  }
  FileResult a, b;
  if (!read_result(into, n_into, a) || !read_result(from, n_from, b))
  {
    g_last_error = "gtx_disc_merge: not a result of gtx_disc_first_pass_haplotypes / gtx_disc_merge";
    return GTX_ERR_ARG;
  }
  if (a.haplotypes.empty())
    a.haplotypes = std::move(b.haplotypes);
  else
    for (auto & kv : b.haplotypes)
    {
      auto ins = a.haplotypes.insert(kv);
      Together & mine = ins.first->second;
      if (ins.second)
      {
        for (auto it = mine.always.begin(); it != mine.always.end();)
          it = a.haplotypes.count(*it) ? mine.always.erase(it) : std::next(it);
        continue;
      }
      mine.ever.insert(kv.second.ever.begin(), kv.second.ever.end());
      std::set<Ev> both;
      std::set_intersection(mine.always.begin(), mine.always.end(), kv.second.always.begin(), kv.second.always.end(), std::inserter(both, both.begin()));
      mine.always.swap(both);
    }
  for (auto & kv : b.indels)
  {
    auto ins = a.indels.insert(kv);
    if (ins.second)
      continue;
    Support & old = ins.first->second;
    old.good = old.good || kv.second.good;
    if (kv.second.max_log_qual > old.max_log_qual)
    {
      old.max_log_qual = kv.second.max_log_qual;
      old.file_i = kv.second.file_i;
    }
  }
  std::vector<uint32_t> w;
  put_result(w, a);
  return hand_over(w, out, cap, n_words);
}

// ---- device: the first pass over the events (what first_pass_state does on the host, without a download) -----------------
// The counted reads' events are laid out in stream order (a scan over the reads), keyed by (position, kind, sequence) and
// sorted stably: the events of one Event are then a run in read order.  One lane walks a run with the host's own accumulation
// step, finds the span of an indel and applies the filter of its kind over prefix sums of the coverage arrays.  The phase
// counts are a second sort: every ordered pair of a read's events is a (group, group) key, equal keys are counted.  The
// survivors are written as the words of gtx_disc_first_pass by the device, and only those come down.
namespace
{
constexpr uint32_t DTB = 256;
constexpr uint32_t INS_DIGITS = 13;     // bases of an insertion in the key: 13 digits of base 5 (0: behind its end) fit the key's 31 bits
constexpr uint64_t KEY_DROPPED = ~0ull; // an event in front of the region, of no known kind, or nobody's: sorts last, never leaves
enum : uint32_t
{
  M_END = 0,    // n_reads - index of the first GTX_DISC_END read (0: none)
  M_ERR = 1,    // a read's events lie behind the event buffer
  M_GROUPS = 2, // distinct events
  M_RUNS = 3,   // distinct phase pairs
  M_EVENTS = 4, // events of the counted reads
  M_PAIRS = 5,  // phase pairs of the counted reads
  M_WORDS = 8
};

struct DiscGroup // one distinct event with what the pass knows of it
{
  DiscCounters c;
  uint32_t pos, rep, span, log_qual, phase_first;
  uint16_t len;
  uint8_t type, verdict; // verdict 0: dropped, 1: stays (an indel: worth a realignment), 2: an indel with good support
};

struct DiscInput
{
  gtx_disc_event const * events;
  uint64_t n_events;
  gtx_disc_read const * reads;
  gtx_disc_read_out const * read_out;
  uint32_t const * cigar;
  uint32_t n_reads;
  uint8_t const * rows;
  uint32_t plane_stride;
  uint8_t const * refc;
  long REF, begin, B;
};

inline uint32_t dblocks(uint64_t n) { return static_cast<uint32_t>((n + DTB - 1) / DTB); }

// base k of an insertion event as 0..3 = A C G T (the events kernel lets only such insertions through)
__device__ inline uint32_t ins_base(DiscInput const & in, gtx_disc_event const & e, uint32_t k)
{
  uint32_t const * row = reinterpret_cast<uint32_t const *>(in.rows + static_cast<uint64_t>(e.read) * in.plane_stride);
  uint32_t const at = e.seq + k, g = at >> 5, s = at & 31u;
  if (g >= in.plane_stride / PLANE_GROUP_BYTES)
    return 0;
  uint32_t const code = ((row[4 * g] >> s) & 1u) | (((row[4 * g + 1] >> s) & 1u) << 1) | (((row[4 * g + 2] >> s) & 1u) << 2) | (((row[4 * g + 3] >> s) & 1u) << 3);
  return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : 3u;
}

// std::string order of two insertions that agree in their first INS_DIGITS bases
__device__ inline int ins_compare(DiscInput const & in, gtx_disc_event const & a, gtx_disc_event const & b)
{
  uint32_t const m = a.len < b.len ? a.len : b.len;
  for (uint32_t k = INS_DIGITS; k < m; ++k)
  {
    uint32_t const x = ins_base(in, a, k), y = ins_base(in, b, k);
    if (x != y)
      return x < y ? -1 : 1;
  }
  return a.len < b.len ? -1 : a.len > b.len ? 1 : 0;
}

// a key whose insertion fills all digits: longer strings may hide behind it
__device__ inline bool key_is_long_insertion(uint64_t key) { return key != KEY_DROPPED && ((key >> 31) & 3u) == 0 && (key & 0x7FFFFFFFull) % 5u != 0; }

__global__ __launch_bounds__(DTB) void gtx_disc_end_kernel(gtx_disc_read_out const * __restrict__ read_out, uint32_t n_reads, uint32_t * meta)
{
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_reads && read_out[i].state == GTX_DISC_END)
    atomicMax(meta + M_END, n_reads - i);
}

// per read: how many events and phase pairs it brings, and its two coverage marks
__global__ __launch_bounds__(DTB) void gtx_disc_reads_kernel(DiscInput in, uint32_t * meta, uint32_t * __restrict__ n_ev, uint32_t * __restrict__ n_pairs,
                                                             uint32_t * up, uint32_t * down)
{
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > in.n_reads)
    return;
  uint32_t ne = 0, np = 0;
  if (i < in.n_reads && i < in.n_reads - meta[M_END])
  {
    gtx_disc_read_out const ro = in.read_out[i];
    if (ro.state == GTX_DISC_COUNTED)
    {
      if (static_cast<uint64_t>(ro.first_event) + ro.n_events > in.n_events)
        atomicOr(meta + M_ERR, 1u);
      else
      {
        ne = ro.n_events;
        np = ne >= 2 && ne < 18 ? ne * (ne - 1) / 2 : 0;
      }
      long const rel = static_cast<long>(in.reads[i].pos) - in.begin;
      if (rel >= 0 && rel < in.REF)
        atomicAdd(up + rel, 1u);
      if (ro.pos_end >= 0 && ro.pos_end < in.REF)
        atomicAdd(down + ro.pos_end, 1u);
    }
  }
  n_ev[i] = ne;
  n_pairs[i] = np;
}

__global__ __launch_bounds__(DTB) void gtx_disc_delta_kernel(uint32_t const * __restrict__ up, uint32_t const * __restrict__ down, uint32_t n, uint32_t * __restrict__ delta)
{
  uint32_t const o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o < n)
    delta[o] = up[o] - down[o];
}

// event j -> its place in stream order (its read's offset + its place in the read) with its key
__global__ __launch_bounds__(DTB) void gtx_disc_keys_kernel(DiscInput in, uint32_t const * __restrict__ meta, uint32_t const * __restrict__ ev_off,
                                                            uint64_t * __restrict__ keys, uint32_t * __restrict__ vals)
{
  uint64_t const j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= in.n_events)
    return;
  gtx_disc_event const e = in.events[j];
  uint32_t const i = e.read;
  if (i >= in.n_reads || i >= in.n_reads - meta[M_END])
    return;
  gtx_disc_read_out const ro = in.read_out[i];
  if (ro.state != GTX_DISC_COUNTED || j < ro.first_event || j - ro.first_event >= ro.n_events || ev_off[i + 1] - ev_off[i] != ro.n_events)
    return;
  uint32_t const r = ev_off[i] + static_cast<uint32_t>(j - ro.first_event);
  uint64_t key = KEY_DROPPED;
  long const rel = static_cast<long>(e.pos) - in.begin;
  // (an event at or behind the region's end keeps its key: it sorts behind the region's own, the walk drops it, and as a phase
  // target it is still the event it was)
  if (rel >= 0 && rel < (1l << 31) && (e.type == 'I' || e.type == 'D' || e.type == 'X'))
  {
    uint32_t code = 0;
    if (e.type == 'X')
      code = e.seq & 0xFFu;
    else if (e.type == 'D')
      code = e.len;
    else
      for (uint32_t k = 0; k < INS_DIGITS; ++k)
        code = code * 5u + (k < e.len ? 1u + ins_base(in, e, k) : 0u);
    uint32_t const kind = e.type == 'I' ? 0u : e.type == 'D' ? 1u : 2u; // (event.cpp:198-207: insertions, deletions, SNPs)
    key = (static_cast<uint64_t>(rel) << 33) | (static_cast<uint64_t>(kind) << 31) | code;
  }
  keys[r] = key;
  vals[r] = static_cast<uint32_t>(j);
}

// the exact second step: a run of equal keys of insertions longer than the key holds is put into string order by one lane,
// stably (an insertion sort: a run of one string costs one comparison per event)
__global__ __launch_bounds__(DTB) void gtx_disc_ties_kernel(DiscInput in, uint64_t const * __restrict__ keys, uint32_t * vals, uint32_t n)
{
  uint32_t const t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n || t + 1 >= n)
    return;
  uint64_t const key = keys[t];
  if (!key_is_long_insertion(key) || keys[t + 1] != key || (t != 0 && keys[t - 1] == key))
    return;
  uint32_t end = t + 1;
  while (end < n && keys[end] == key)
    ++end;
  for (uint32_t k = t + 1; k < end; ++k)
  {
    uint32_t const x = vals[k];
    gtx_disc_event const ex = in.events[x];
    uint32_t s = k;
    while (s > t && ins_compare(in, in.events[vals[s - 1]], ex) > 0)
    {
      vals[s] = vals[s - 1];
      --s;
    }
    vals[s] = x;
  }
}

__global__ __launch_bounds__(DTB) void gtx_disc_heads_kernel(DiscInput in, uint64_t const * __restrict__ keys, uint32_t const * __restrict__ vals, uint32_t n,
                                                             uint32_t * __restrict__ head)
{
  uint32_t const t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  bool h = t == 0 || keys[t - 1] != keys[t];
  if (!h && key_is_long_insertion(keys[t]))
    h = ins_compare(in, in.events[vals[t - 1]], in.events[vals[t]]) != 0;
  head[t] = h;
}

// gid1: inclusive scan of the heads (group index + 1)
__global__ __launch_bounds__(DTB) void gtx_disc_groups_kernel(uint32_t const * __restrict__ head, uint32_t const * __restrict__ gid1, uint32_t const * __restrict__ vals,
                                                              uint32_t n, uint32_t * __restrict__ gstart, uint32_t * __restrict__ gid_of, uint32_t * meta)
{
  uint32_t const t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n)
    return;
  uint32_t const g = gid1[t] - 1;
  if (head[t])
    gstart[g] = t;
  gid_of[vals[t]] = g;
  if (t == n - 1)
  {
    gstart[g + 1] = n;
    meta[M_GROUPS] = g + 1;
  }
}

// the ordered pairs of a read's events as (group of the earlier, group of the later)
__global__ __launch_bounds__(DTB) void gtx_disc_pairs_kernel(DiscInput in, uint32_t const * __restrict__ pair_off, uint32_t const * __restrict__ gid_of,
                                                             uint32_t shift, uint64_t * __restrict__ pairs)
{
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n_reads || pair_off[i + 1] == pair_off[i])
    return;
  gtx_disc_read_out const ro = in.read_out[i];
  uint64_t * out = pairs + pair_off[i];
  for (uint32_t b = 1; b < ro.n_events; ++b)
  {
    uint64_t const gb = gid_of[ro.first_event + b];
    for (uint32_t a = 0; a < b; ++a)
      *out++ = (static_cast<uint64_t>(gid_of[ro.first_event + a]) << shift) | gb;
  }
}

__global__ __launch_bounds__(DTB) void gtx_disc_pair_heads_kernel(uint64_t const * __restrict__ pairs, uint32_t n, uint32_t * __restrict__ head)
{
  uint32_t const p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n)
    head[p] = p == 0 || pairs[p - 1] != pairs[p];
}

__global__ __launch_bounds__(DTB) void gtx_disc_runs_kernel(uint64_t const * __restrict__ pairs, uint32_t const * __restrict__ head, uint32_t const * __restrict__ rid1,
                                                            uint32_t n, uint32_t shift, uint64_t * __restrict__ run_key, uint32_t * __restrict__ run_start,
                                                            uint32_t * __restrict__ phase_first, uint32_t * meta)
{
  uint32_t const p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n)
    return;
  uint32_t const r = rid1[p] - 1;
  if (head[p])
  {
    run_key[r] = pairs[p];
    run_start[r] = p;
    if (p == 0 || (pairs[p - 1] >> shift) != (pairs[p] >> shift))
      phase_first[pairs[p] >> shift] = r;
  }
  if (p == n - 1)
  {
    run_start[r + 1] = n;
    meta[M_RUNS] = r + 1;
  }
}

// one lane, one distinct event: its run of events in read order through the host's accumulation step, the span, the filter
__global__ __launch_bounds__(DTB) void gtx_disc_walk_kernel(DiscInput in, uint32_t const * __restrict__ meta, uint64_t const * __restrict__ keys,
                                                            uint32_t const * __restrict__ vals, uint32_t const * __restrict__ gstart,
                                                            uint32_t const * __restrict__ cov_delta, uint32_t const * __restrict__ cov_down,
                                                            uint32_t const * __restrict__ phase_first, DiscGroup * __restrict__ groups)
{
  uint32_t const g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= meta[M_GROUPS])
    return;
  uint32_t const t0 = gstart[g], t1 = gstart[g + 1];
  gtx_disc_event const e0 = in.events[vals[t0]];
  DiscGroup out;
  out.pos = e0.pos;
  out.rep = vals[t0];
  out.len = e0.len;
  out.type = e0.type;
  out.span = 1;
  out.log_qual = 0;
  out.verdict = 0;
  out.phase_first = phase_first[g];
  if (keys[t0] == KEY_DROPPED) // (nothing of it is read again: as a phase target it would be an event without letters)
  {
    out.type = 0;
    out.len = 0;
    groups[g] = out;
    return;
  }
  DiscCounters c;
  for (uint32_t t = t0; t < t1;)
  {
    uint32_t const i = in.events[vals[t]].read; // (a counted read: the keys kernel placed no other's events)
    gtx_disc_read const r = in.reads[i];
    uint32_t const n_of_read = in.read_out[i].n_events;
    bool clipped = false;
    if (r.n_cigar)
    {
      uint32_t const front = in.cigar[r.cigar_off], back = in.cigar[r.cigar_off + r.n_cigar - 1];
      clipped = ((front & 15u) == 4 && (front >> 4) >= 1) || ((back & 15u) == 4 && (back >> 4) >= 1); // is_clipped (caller.cpp:167-196)
    }
    uint32_t u = t;
    for (; u < t1; ++u) // the read's own events of this kind (more than one: two equal insertions at one place)
    {
      gtx_disc_event const e = in.events[vals[u]];
      if (e.read != i)
        break;
      disc_accumulate(c, e.type, e.hq, e.max_distance, r.pos, r.flag, r.mapq, clipped);
    }
    if (n_of_read >= 12) // the correction comes when the read is through, before the next read's events
      for (uint32_t k = t; k < u; ++k)
        disc_many_events(c, n_of_read);
    t = u;
  }
  out.c = c;
  long const REF = in.REF, rel = static_cast<long>(e0.pos) - in.begin;
  if (rel >= REF) // its bucket lies behind the region's last: the reference cuts it off before the filters
  {
    groups[g] = out;
    return;
  }
  if (e0.type == 'X')
    out.verdict = disc_good_snp(c, static_cast<long>(static_cast<int32_t>(cov_delta[rel + 1]))) ? 1 : 0;
  else
  {
    // span of an indel (bucket.cpp:100-160): how far it can be shifted
    long span = 0, count = e0.len;
    uint8_t const * ref = in.refc;
    if (e0.type == 'I')
    {
      while (span < count && rel + span < REF && "ACGT"[ins_base(in, e0, static_cast<uint32_t>(span))] == ref[rel + span])
        ++span;
      if (span == count)
        while (rel + span < REF && ref[rel + span - count] == ref[rel + span])
          ++span;
    }
    else
      while (rel + span < REF && rel + span + count < REF && ref[rel + span] == ref[rel + span + count])
        ++span;
    out.span = static_cast<uint16_t>((span < 0xFFFE ? span : 0xFFFE) + 1);
    // coverage over its window (caller.cpp:1003-1040) from the prefix sums: what lies in front of the window, less the reads that end in it
    // (counted from the event's bucket on, as the reference does)
    long lo = 0, hi = 0;
    disc_indel_window(static_cast<long>(e0.pos), e0.len, out.span, in.begin, REF, lo, hi);
    long const bucket_begin = rel / in.B * in.B, from = lo > bucket_begin ? lo : bucket_begin, to = hi < REF - 1 ? hi : REF - 1;
    long cov = static_cast<long>(static_cast<int32_t>(cov_delta[lo]));
    if (to >= from)
      cov -= static_cast<long>(cov_down[to + 1] - cov_down[from]);
    out.verdict = static_cast<uint8_t>(disc_indel_class(c, e0.type == 'I', e0.len, cov, out.log_qual));
    if (out.verdict == 0)
      out.log_qual = 0;
  }
  groups[g] = out;
}

// words of a surviving event: itself, 16 support words, its phase entries
__global__ __launch_bounds__(DTB) void gtx_disc_sizes_kernel(uint32_t const * __restrict__ meta, DiscGroup const * __restrict__ groups,
                                                             uint64_t const * __restrict__ run_key, uint32_t shift, uint32_t n, uint32_t * __restrict__ words)
{
  uint32_t const g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n)
    return;
  uint32_t w = 0;
  if (g < meta[M_GROUPS] && groups[g].verdict != 0)
  {
    w = 3u + groups[g].len + 16u;
    uint64_t const mask = (1ull << shift) - 1;
    for (uint32_t r = groups[g].phase_first; r < meta[M_RUNS] && (run_key[r] >> shift) == g; ++r)
      w += 4u + groups[run_key[r] & mask].len;
  }
  words[g] = w;
}

__device__ inline uint32_t * emit_event(DiscInput const & in, gtx_disc_event const * events, DiscGroup const & g, uint32_t * w)
{
  *w++ = g.pos;
  *w++ = g.type;
  *w++ = g.len;
  gtx_disc_event const e = events[g.rep];
  if (g.type == 'X')
    *w++ = e.seq & 0xFFu;
  else if (g.type == 'D')
    for (uint32_t k = 0; k < g.len; ++k)
      *w++ = static_cast<long>(e.seq) + k < in.REF ? in.refc[e.seq + k] : static_cast<uint32_t>('N');
  else
    for (uint32_t k = 0; k < g.len; ++k)
      *w++ = static_cast<uint32_t>("ACGT"[ins_base(in, e, k)]);
  return w;
}

__global__ __launch_bounds__(DTB) void gtx_disc_emit_kernel(DiscInput in, uint32_t const * __restrict__ meta, DiscGroup const * __restrict__ groups,
                                                            uint64_t const * __restrict__ run_key, uint32_t const * __restrict__ run_start, uint32_t shift,
                                                            uint32_t const * __restrict__ word_off, uint32_t * __restrict__ out)
{
  uint32_t const g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= meta[M_GROUPS] || groups[g].verdict == 0)
    return;
  DiscGroup const G = groups[g];
  DiscCounters const & s = G.c;
  uint32_t * w = emit_event(in, in.events, G, out + word_off[g]);
  bool const indel = G.type != 'X';
  uint32_t const fields[15] = {disc_wrap16(s.hq), disc_wrap16(s.lq), disc_wrap16(s.proper), disc_wrap16(s.first), disc_wrap16(s.reversed),
                               disc_wrap16(s.clipped), s.max_mapq, s.max_distance, static_cast<uint32_t>(s.u1), static_cast<uint32_t>(s.u2),
                               static_cast<uint32_t>(s.u3), G.span, indel ? 1u : 0u, indel && G.verdict == 2 ? 1u : 0u, G.log_qual};
  for (uint32_t k = 0; k < 15; ++k)
    *w++ = fields[k];
  uint32_t * n_phase = w++;
  uint32_t np = 0;
  uint64_t const mask = (1ull << shift) - 1;
  for (uint32_t r = G.phase_first; r < meta[M_RUNS] && (run_key[r] >> shift) == g; ++r, ++np)
  {
    w = emit_event(in, in.events, groups[run_key[r] & mask], w);
    *w++ = disc_wrap16(run_start[r + 1] - run_start[r]); // (a uint16_t that wraps, event.hpp)
  }
  *n_phase = np;
}

constexpr char const * MSG_PREFIX = "gtx_disc_first_pass_device: "; // of the device pass' HIP error messages (its pool carries it too)

bool disc_download_async(void * to, void const * from, size_t bytes, hipStream_t stream)
{
  return hip_ok(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, stream), "download", MSG_PREFIX);
}

bool disc_wait(hipStream_t stream) { return hip_ok(hipStreamSynchronize(stream), "synchronise", MSG_PREFIX); }

bool disc_download(void * to, void const * from, size_t bytes, hipStream_t stream) { return disc_download_async(to, from, bytes, stream) && disc_wait(stream); }

bool disc_launched() { return hip_ok(hipGetLastError(), "kernel launch", MSG_PREFIX); }

struct DiscDeviceResult
{
  uint32_t * d_words = nullptr; // the words of gtx_disc_first_pass
  uint64_t n_words = 0;
  uint32_t *d_up = nullptr, *d_down = nullptr; // cov_up / cov_down (REF + 1 words each)
};

int disc_device_pass(const gtx_disc * d, TempPool & pool, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads,
                     const uint32_t * d_cigar, const gtx_disc_read_out * d_read_out, uint32_t n_reads, const gtx_disc_event * d_events,
                     const uint32_t * d_counts, uint32_t bucket_size, DiscDeviceResult & res)
{
  hipStream_t const stream = pool.stream;
  long const REF = static_cast<long>(d->reference.size());
  uint32_t counts[2] = {0, 0};
  if (!disc_download(counts, d_counts, sizeof counts, stream))
    return GTX_ERR_HIP;
  if (counts[1] != 0)
  {
    g_last_error = "gtx_disc_first_pass_device: the event buffer overflowed (d_counts[1] != 0: event_cap too small)";
    return GTX_ERR_CAPACITY;
  }
  if (counts[0] > (1u << 28))
  {
    g_last_error = "gtx_disc_first_pass_device: more than 2^28 events in one pass";
    return GTX_ERR_UNSUPPORTED;
  }
  DiscInput in{d_events, counts[0], d_reads, d_read_out, d_cigar, n_reads, d_planes, plane_stride, d->d_refc.get(), REF, static_cast<long>(d->region_begin),
               static_cast<long>(bucket_size)};
  uint32_t * meta = pool.get<uint32_t>(M_WORDS, "counters", 0);
  res.d_up = pool.get<uint32_t>(REF + 1, "cov_up", 0);
  res.d_down = pool.get<uint32_t>(REF + 1, "cov_down", 0);
  uint32_t * n_ev = pool.get<uint32_t>(n_reads + 1, "events per read");
  uint32_t * n_pairs = pool.get<uint32_t>(n_reads + 1, "pairs per read");
  uint32_t * ev_off = pool.get<uint32_t>(n_reads + 1, "event offsets");
  uint32_t * pair_off = pool.get<uint32_t>(n_reads + 1, "pair offsets");
  uint32_t * delta = pool.get<uint32_t>(REF + 1, "coverage differences");
  uint32_t * cov_delta = pool.get<uint32_t>(REF + 1, "coverage prefix");
  uint32_t * cov_down = pool.get<uint32_t>(REF + 1, "cov_down prefix");
  if (!pool.fine)
    return GTX_ERR_HIP;
  res.n_words = 0;
  if (n_reads == 0)
    return GTX_OK;
  hipLaunchKernelGGL(gtx_disc_end_kernel, dim3(dblocks(n_reads)), dim3(DTB), 0, stream, d_read_out, n_reads, meta);
  hipLaunchKernelGGL(gtx_disc_reads_kernel, dim3(dblocks(n_reads + 1)), dim3(DTB), 0, stream, in, meta, n_ev, n_pairs, res.d_up, res.d_down);
  hipLaunchKernelGGL(gtx_disc_delta_kernel, dim3(dblocks(REF + 1)), dim3(DTB), 0, stream, res.d_up, res.d_down, static_cast<uint32_t>(REF + 1), delta);
  if (!exclusive_sum(pool, n_ev, ev_off, n_reads + 1, "scan", "scan temporary") || !exclusive_sum(pool, n_pairs, pair_off, n_reads + 1, "scan", "scan temporary") ||
      !exclusive_sum(pool, delta, cov_delta, REF + 1, "scan", "scan temporary") || !exclusive_sum(pool, res.d_down, cov_down, REF + 1, "scan", "scan temporary"))
    return GTX_ERR_HIP;
  // the two totals join the counters: one copy, one wait
  uint32_t head_words[M_WORDS];
  if (!disc_launched() || !pool.ok(hipMemcpyAsync(meta + M_EVENTS, ev_off + n_reads, 4, hipMemcpyDeviceToDevice, stream), "copy") ||
      !pool.ok(hipMemcpyAsync(meta + M_PAIRS, pair_off + n_reads, 4, hipMemcpyDeviceToDevice, stream), "copy") ||
      !disc_download(head_words, meta, sizeof head_words, stream))
    return GTX_ERR_HIP;
  uint32_t const ne = head_words[M_EVENTS], np = head_words[M_PAIRS];
  if (head_words[M_ERR])
  {
    g_last_error = "gtx_disc_first_pass_device: a read's events lie behind the event buffer (it overflowed: event_cap too small)";
    return GTX_ERR_CAPACITY;
  }
  res.n_words = 0;
  if (ne == 0)
    return GTX_OK;
  // the events in stream order, keyed and sorted
  uint64_t * keys_in = pool.get<uint64_t>(ne, "keys", 0xFF);
  uint64_t * keys = pool.get<uint64_t>(ne, "sorted keys");
  uint32_t * vals_in = pool.get<uint32_t>(ne, "event indices", 0);
  uint32_t * vals = pool.get<uint32_t>(ne, "sorted event indices");
  uint32_t * head = pool.get<uint32_t>(ne, "heads");
  uint32_t * gid1 = pool.get<uint32_t>(ne, "group numbers");
  uint32_t * gstart = pool.get<uint32_t>(ne + 1, "group starts");
  uint32_t * gid_of = pool.get<uint32_t>(counts[0], "group of an event", 0);
  uint32_t * phase_first = pool.get<uint32_t>(ne, "first phase run", 0xFF);
  DiscGroup * groups = pool.get<DiscGroup>(ne, "groups");
  uint32_t * words = pool.get<uint32_t>(ne + 1, "words per group");
  uint32_t * word_off = pool.get<uint32_t>(ne + 1, "word offsets");
  if (!pool.fine)
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_keys_kernel, dim3(dblocks(counts[0])), dim3(DTB), 0, stream, in, meta, ev_off, keys_in, vals_in);
  if (!sort_pairs(pool, keys_in, keys, vals_in, vals, ne, 64u, "radix sort", "sort temporary"))
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_ties_kernel, dim3(dblocks(ne)), dim3(DTB), 0, stream, in, keys, vals, ne);
  hipLaunchKernelGGL(gtx_disc_heads_kernel, dim3(dblocks(ne)), dim3(DTB), 0, stream, in, keys, vals, ne, head);
  if (!inclusive_scan(pool, head, gid1, ne, rocprim::plus<uint32_t>(), "scan", "scan temporary"))
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_groups_kernel, dim3(dblocks(ne)), dim3(DTB), 0, stream, head, gid1, vals, ne, gstart, gid_of, meta);
  // the phase counts: pairs of groups, sorted, run lengths
  uint32_t shift = 1;
  while ((1ull << shift) < ne)
    ++shift;
  uint64_t * run_key = pool.get<uint64_t>(np + 1, "phase keys");
  uint32_t * run_start = pool.get<uint32_t>(np + 1, "phase run starts");
  if (np)
  {
    uint64_t * pairs_in = pool.get<uint64_t>(np, "pairs");
    uint64_t * pairs = pool.get<uint64_t>(np, "sorted pairs");
    uint32_t * phead = pool.get<uint32_t>(np, "pair heads");
    uint32_t * rid1 = pool.get<uint32_t>(np, "run numbers");
    if (!pool.fine)
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_disc_pairs_kernel, dim3(dblocks(n_reads)), dim3(DTB), 0, stream, in, pair_off, gid_of, shift, pairs_in);
    if (!sort_keys(pool, pairs_in, pairs, np, 2 * shift, "radix sort of the pairs", "sort temporary"))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_disc_pair_heads_kernel, dim3(dblocks(np)), dim3(DTB), 0, stream, pairs, np, phead);
    if (!inclusive_scan(pool, phead, rid1, np, rocprim::plus<uint32_t>(), "scan", "scan temporary"))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_disc_runs_kernel, dim3(dblocks(np)), dim3(DTB), 0, stream, pairs, phead, rid1, np, shift, run_key, run_start, phase_first, meta);
  }
  if (!pool.fine)
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_walk_kernel, dim3(dblocks(ne)), dim3(DTB), 0, stream, in, meta, keys, vals, gstart, cov_delta, cov_down, phase_first, groups);
  hipLaunchKernelGGL(gtx_disc_sizes_kernel, dim3(dblocks(ne + 1)), dim3(DTB), 0, stream, meta, groups, run_key, shift, ne, words);
  if (!exclusive_sum(pool, words, word_off, ne + 1, "scan", "scan temporary"))
    return GTX_ERR_HIP;
  uint32_t total = 0;
  if (!disc_launched() || !disc_download(&total, word_off + ne, 4, stream))
    return GTX_ERR_HIP;
  res.n_words = total;
  if (total == 0)
    return GTX_OK;
  res.d_words = pool.get<uint32_t>(total, "result words");
  if (!pool.fine)
    return GTX_ERR_HIP;
  hipLaunchKernelGGL(gtx_disc_emit_kernel, dim3(dblocks(ne)), dim3(DTB), 0, stream, in, meta, groups, run_key, run_start, shift, word_off, res.d_words);
  return disc_launched() ? GTX_OK : GTX_ERR_HIP;
}

int disc_device_args(char const * name, const gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads,
                     const uint32_t * d_cigar, const gtx_disc_read_out * d_read_out, uint32_t n_reads, const gtx_disc_event * d_events,
                     const uint32_t * d_counts, uint32_t bucket_size, uint32_t * out, uint64_t cap, uint64_t * n_words)
{
  if (!d || !n_words || bucket_size == 0 || plane_stride == 0 || (plane_stride % PLANE_GROUP_BYTES) != 0 || (reinterpret_cast<uintptr_t>(d_planes) & 3u) != 0 ||
      !d_counts || (n_reads != 0 && (!d_planes || !d_reads || !d_cigar || !d_read_out)) || (cap && !out) || n_reads == 0xFFFFFFFFu)
  {
    g_last_error = std::string(name) + ": bad argument";
    return GTX_ERR_ARG;
  }
  (void)d_events; // (may be NULL when no event was made)
  return device_ready(d->device, name, ": the object");
}
} // namespace

extern "C" int gtx_disc_first_pass_device(const gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads,
                                          const uint32_t * d_cigar, const gtx_disc_read_out * d_read_out, uint32_t n_reads, const gtx_disc_event * d_events,
                                          const uint32_t * d_counts, uint32_t bucket_size, uint32_t * out, uint64_t cap, uint64_t * n_words, void * stream)
{
  int rc = disc_device_args("gtx_disc_first_pass_device", d, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size, out,
                            cap, n_words);
  if (rc != GTX_OK)
    return rc;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  TempPool pool(s, MSG_PREFIX);
  DiscDeviceResult res;
  rc = disc_device_pass(d, pool, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size, res);
  if (rc != GTX_OK)
    return rc;
  *n_words = res.n_words;
  if (res.n_words > cap)
    return GTX_ERR_CAPACITY;
  if (res.n_words && !disc_download(out, res.d_words, res.n_words * 4, s))
    return GTX_ERR_HIP;
  return GTX_OK;
}

extern "C" int gtx_disc_first_pass_haplotypes_device(const gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads,
                                                     const uint32_t * d_cigar, const gtx_disc_read_out * d_read_out, uint32_t n_reads,
                                                     const gtx_disc_event * d_events, const uint32_t * d_counts, uint32_t bucket_size, int32_t file_index,
                                                     uint32_t * out, uint64_t cap, uint64_t * n_words, void * stream)
{
  int rc = disc_device_args("gtx_disc_first_pass_haplotypes_device", d, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts,
                            bucket_size, out, cap, n_words);
  if (rc != GTX_OK)
    return rc;
  hipStream_t const hs = static_cast<hipStream_t>(stream);
  PassState st;
  st.REF = static_cast<long>(d->reference.size());
  st.B = bucket_size;
  st.begin = d->region_begin;
  std::vector<uint32_t> w;
  {
    TempPool pool(hs, MSG_PREFIX);
    DiscDeviceResult res;
    rc = disc_device_pass(d, pool, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size, res);
    if (rc != GTX_OK)
      return rc;
    w.resize(res.n_words);
    st.up.resize(st.REF);
    st.down.resize(st.REF);
    if ((res.n_words && !disc_download_async(w.data(), res.d_words, res.n_words * 4, hs)) || !disc_download_async(st.up.data(), res.d_up, st.REF * 4, hs) ||
        !disc_download_async(st.down.data(), res.d_down, st.REF * 4, hs) || !disc_wait(hs))
      return GTX_ERR_HIP;
  }
  // the survivors back into the buckets of the host stage
  st.buckets.resize((st.REF - 1) / st.B + 1);
  size_t at = 0;
  bool whole = true; // (the words are the device's own; a cut stream is still not read behind its end)
  auto event = [&]()
  {
    if (at + 3 > w.size() || w[at + 2] > w.size() - at - 3)
    {
      whole = false;
      at = w.size();
      return Ev{};
    }
    Ev e{w[at], static_cast<uint8_t>(w[at + 1]), {}};
    uint32_t const len = w[at + 2];
    for (uint32_t k = 0; k < len; ++k)
      e.seq.push_back(static_cast<char>(w[at + 3 + k]));
    at += 3 + len;
    return e;
  };
  while (at < w.size())
  {
    Ev e = event();
    if (!whole || at + 16 > w.size())
    {
      whole = false;
      break;
    }
    Support s;
    s.hq = w[at]; s.lq = w[at + 1]; s.proper = w[at + 2]; s.first = w[at + 3]; s.reversed = w[at + 4]; s.clipped = w[at + 5];
    s.max_mapq = static_cast<uint8_t>(w[at + 6]); s.max_distance = static_cast<uint8_t>(w[at + 7]);
    s.u1 = static_cast<int32_t>(w[at + 8]); s.u2 = static_cast<int32_t>(w[at + 9]); s.u3 = static_cast<int32_t>(w[at + 10]);
    s.span = static_cast<uint16_t>(w[at + 11]); s.realign = w[at + 12] != 0; s.good = w[at + 13] != 0; s.max_log_qual = w[at + 14];
    s.file_i = e.type != 'X' ? file_index : 0;
    uint32_t const n_phase = w[at + 15];
    at += 16;
    for (uint32_t k = 0; k < n_phase; ++k)
    {
      Ev pe = event();
      if (!whole || at >= w.size())
      {
        whole = false;
        break;
      }
      s.phase[pe] = static_cast<uint16_t>(w[at++]);
    }
    if (!whole)
      break;
    size_t const b = static_cast<size_t>((static_cast<long>(e.pos) - st.begin) / st.B);
    st.buckets[b].insert({std::move(e), std::move(s)});
  }
  if (!whole)
  {
    g_last_error = "gtx_disc_first_pass_haplotypes_device: the device's words do not parse";
    return GTX_ERR_HIP;
  }
  return haplotypes_of(st, out, cap, n_words);
}
