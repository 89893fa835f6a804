// gtx_discover_run.hip -- discovery's host loops inside the library, beside gtx_regions.cpp and gtx_pipeline.cpp: a file's second
// pass as one call (gtx_disc_second_file: what parallel_second_pass, src/typer/caller.cpp:2633-2751, does for one file) and a
// region's discovery to the sites file (streamlined_discovery, :2753-3093, then the writer) from host arrays (gtx_discover_region)
// or from the BAM files themselves (gtx_discover_files: read on the host, gtx_disc_bam.cpp, unpacked on the device, gtx_disc_bam.hip;
// gtx_discover_files_front with front 1: inflated, walked and unpacked on the device, gtx_inflate_dev.hip, gtx_disc_bam_walk.hip);
// the three share one body behind "the file's arrays are on the device".
//
// No kernel lives here: every stage is an entry point that exists, and this file is their caller -- the uploads, the growth
// protocols (the events buffer of the first pass, the event array of the rounds), the downloads, the merge.  A file's arrays are
// uploaded once and stay on the device across both passes.  The files run on worker threads, each with a gtx_disc and a stream of
// its own and nothing else, so that the waits of one file's rounds (launches and waits more than work) overlap the others'.
// Every block, stream and handle has an owner: an error or an exception on any thread frees what was made.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <exception>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gtx.h"
#include "gtx_bam_record.hpp"
#include "gtx_devmem.hpp"
#include "gtx_disc.hpp"
#include "gtx_disc_bam.hpp"
#include "gtx_disc_bam_walk_dev.hpp"
#include "gtx_switches.hpp"

static_assert(sizeof(gtx_disc_variant) == 44 && sizeof(gtx_disc_file) == 48 && sizeof(gtx_discover_params) == 24 && sizeof(gtx_discover_file_stats) == 64 &&
                  sizeof(gtx_discover_front_stats) == 24,
              "layouts of the binding");

struct gtx_discover_result
{
  std::string text;
  std::vector<gtx_disc_variant> variants;
  std::string letters;
  std::vector<uint32_t> ids;
  std::vector<uint32_t> words;
  std::vector<uint8_t> good;
  std::vector<gtx_discover_file_stats> stats;
  std::vector<gtx_discover_front_stats> front;
};

namespace
{
using namespace gtx;

constexpr char const * MSG_PREFIX = "gtx_discover: ";
constexpr size_t PAD = 16; // bytes behind every block: a block of no entries is still a block

using Disc = std::unique_ptr<gtx_disc, Free<gtx_disc_destroy>>;

int bad(char const * name, char const * why = "bad argument")
{
  g_last_error = std::string(name) + ": " + why;
  return GTX_ERR_ARG;
}

// n entries of T on the device, zeroed on the stream
template <class T>
bool zeroed(DevPtr<T> & p, size_t n, hipStream_t s, char const * what)
{
  size_t const bytes = n * sizeof(T) + PAD;
  return hip_ok(alloc_e(p, bytes), what, MSG_PREFIX) && hip_ok(hipMemsetAsync(p.get(), 0, bytes, s), what, MSG_PREFIX);
}

// n entries of T on the device, copied from the host on the stream
template <class T, class H>
bool uploaded(DevPtr<T> & p, H const * from, size_t n, hipStream_t s, char const * what, size_t room_behind = 0)
{
  if (!zeroed(p, n + room_behind, s, what))
    return false;
  return n == 0 || hip_ok(hipMemcpyAsync(p.get(), from, n * sizeof(T), hipMemcpyHostToDevice, s), what, MSG_PREFIX);
}

// n entries of T on the device that the next work on the stream writes, every one of them: only what lies behind them is zeroed
template <class T>
bool made(DevPtr<T> & p, size_t n, hipStream_t s, char const * what, size_t room_behind = 0)
{
  size_t const used = n * sizeof(T), bytes = used + room_behind + PAD;
  return hip_ok(alloc_e(p, bytes), what, MSG_PREFIX) && hip_ok(hipMemsetAsync(reinterpret_cast<uint8_t *>(p.get()) + used, 0, bytes - used, s), what, MSG_PREFIX);
}

template <class T, class H>
bool copied_up(T * to, H const * from, size_t n, hipStream_t s, char const * what)
{
  return n == 0 || hip_ok(hipMemcpyAsync(to, from, n * sizeof(T), hipMemcpyHostToDevice, s), what, MSG_PREFIX);
}

template <class T>
bool downloaded(T * to, void const * from, size_t n, hipStream_t s, char const * what)
{
  return n == 0 || hip_ok(hipMemcpyAsync(to, from, n * sizeof(T), hipMemcpyDeviceToHost, s), what, MSG_PREFIX);
}

bool waited(hipStream_t s) { return hip_ok(hipStreamSynchronize(s), "wait", MSG_PREFIX); }

// Declared behind the blocks of a scope: the stream (the null stream too) is waited for before any of them goes back to the cache,
// on every way out.
struct WaitBehind
{
  hipStream_t const stream;
  explicit WaitBehind(hipStream_t s) : stream(s) {}
  WaitBehind(WaitBehind const &) = delete;
  WaitBehind & operator=(WaitBehind const &) = delete;
  ~WaitBehind() { (void)hipStreamSynchronize(stream); }
};

struct SecondResult // what a file's second pass leaves on the host
{
  std::vector<uint32_t> good_bits, list;
  gtx_disc_second_rounds_stats stats{};
  std::vector<gtx_disc_second_read> second;
  std::vector<gtx_disc_second_event> events;
  std::vector<gtx_disc_second_support> support;
};

// lib.disc_second_file's steps, in C (gtx.h: gtx_disc_second_file); want_state: the reads, their lists and the counters come down too
int second_file(gtx_disc * d, uint8_t const * d_planes, uint32_t plane_stride, gtx_disc_read const * d_reads, uint32_t const * d_cigar, uint32_t n_reads,
                uint32_t const * words, uint64_t n_words, int32_t file_index, uint32_t bucket_size, uint32_t event_cap, bool want_state, hipStream_t s,
                SecondResult & out)
{
  // the table
  uint32_t nt = 0;
  uint64_t n_seq = 0;
  int rc = gtx_disc_indel_table(words, n_words, nullptr, 0, &nt, nullptr, 0, &n_seq);
  if (rc != GTX_OK && rc != GTX_ERR_CAPACITY)
    return rc;
  std::vector<gtx_disc_indel> table(nt);
  std::vector<char> letters(n_seq);
  if ((rc = gtx_disc_indel_table(words, n_words, table.data(), nt, &nt, letters.data(), n_seq, &n_seq)) != GTX_OK)
    return rc;
  if ((rc = device_ready(d->device, "gtx_disc_second_file", ": the object")) != GTX_OK)
    return rc;
  uint32_t const nb = static_cast<uint32_t>((d->reference.size() - 1) / bucket_size + 1), found_words = (nt + 31u) / 32u;
  DevPtr<gtx_disc_indel> d_table;
  DevPtr<char> d_letters;
  DevPtr<gtx_disc_second_read> d_second;
  DevPtr<int32_t> d_bmax, d_gmax;
  DevPtr<uint32_t> d_mrs, d_breads, d_boff, d_found, d_list;
  DevPtr<gtx_disc_second_event> d_events, bigger;
  DevPtr<gtx_disc_second_support> d_support;
  WaitBehind const behind(s);
  if (!zeroed(d_table, nt, s, "table") || !zeroed(d_letters, n_seq, s, "table letters") || !zeroed(d_second, n_reads, s, "reads' state") ||
      !zeroed(d_bmax, nb, s, "bucket maxima") || !zeroed(d_gmax, nb, s, "bucket maxima") || !zeroed(d_mrs, 1, s, "max read size") ||
      !zeroed(d_breads, n_reads, s, "bucket reads") || !zeroed(d_boff, static_cast<size_t>(nb) + 1, s, "bucket offsets") ||
      !zeroed(d_found, found_words, s, "found bits") || !zeroed(d_support, nt, s, "counters"))
    return GTX_ERR_HIP;
  if ((rc = gtx_disc_indel_table_upload(d, table.data(), nt, letters.data(), n_seq, d_table.get(), d_letters.get(), s)) != GTX_OK)
    return rc;
  // the intake, the found-bits down, the plan, the list up
  if ((rc = gtx_disc_second_intake(d, d_planes, plane_stride, d_reads, d_cigar, n_reads, bucket_size, d_table.get(), d_letters.get(), nt, n_seq, d_second.get(),
                                   d_bmax.get(), d_gmax.get(), d_mrs.get(), d_breads.get(), d_boff.get(), d_found.get(), s)) != GTX_OK)
    return rc;
  std::vector<uint32_t> found(found_words);
  if (!downloaded(found.data(), d_found.get(), found_words, s, "found bits") || !waited(s))
    return GTX_ERR_HIP;
  out.list.assign(nt, 0);
  uint32_t n_list = 0;
  if ((rc = gtx_disc_second_plan(table.data(), nt, found.data(), file_index, out.list.data(), nt, &n_list)) != GTX_OK)
    return rc;
  out.list.resize(n_list);
  if (!uploaded(d_list, out.list.data(), n_list, s, "list"))
    return GTX_ERR_HIP;
  // the rounds: the event array grown and the call continued at the round it stopped in front of
  uint64_t cap = event_cap ? event_cap : std::max<uint64_t>(2ull * n_reads, 1024);
  if (!zeroed(d_events, cap, s, "event array") || !waited(s))
    return GTX_ERR_HIP;
  uint32_t k = 0, used = 0;
  out.stats = gtx_disc_second_rounds_stats{};
  for (;;)
  {
    gtx_disc_second_rounds_stats st{};
    rc = gtx_disc_second_rounds(d, d_planes, plane_stride, d_list.get(), k, n_list, d_table.get(), d_letters.get(), nt, n_seq, d_second.get(), n_reads, d_events.get(),
                                static_cast<uint32_t>(cap), &used, bucket_size, d_bmax.get(), d_gmax.get(), d_mrs.get(), d_breads.get(), d_boff.get(),
                                d_support.get(), &st, s);
    if (rc != GTX_OK && rc != GTX_ERR_CAPACITY)
      return rc;
    k += st.rounds_done;
    out.stats.pairs += st.pairs;
    out.stats.pairs_aligned += st.pairs_aligned;
    out.stats.pairs_refused += st.pairs_refused;
    out.stats.windows_built += st.windows_built;
    out.stats.rounds_done += st.rounds_done;
    out.stats.rounds_skipped += st.rounds_skipped;
    out.stats.compactions += st.compactions;
    if (rc == GTX_OK)
      break;
    if (st.events_wanted <= cap) // (GTX_ERR_CAPACITY for another reason: a round whose windows are too large)
      return rc;
    uint64_t const more = std::min<uint64_t>(std::max<uint64_t>(2 * cap, st.events_wanted), 0xFFFFFFFFull);
    if (!waited(s) || !zeroed(bigger, more, s, "event array") ||
        (used && !hip_ok(hipMemcpyAsync(bigger.get(), d_events.get(), static_cast<size_t>(used) * sizeof(gtx_disc_second_event), hipMemcpyDeviceToDevice, s),
                         "event array", MSG_PREFIX)) ||
        !waited(s))
      return GTX_ERR_HIP;
    d_events.swap(bigger);
    bigger.reset();
    cap = more;
  }
  // the counters down, the decision
  out.support.assign(nt, gtx_disc_second_support{});
  if (want_state)
  {
    out.second.assign(n_reads, gtx_disc_second_read{});
    out.events.assign(used, gtx_disc_second_event{});
  }
  if (!downloaded(out.support.data(), d_support.get(), nt, s, "counters") ||
      (want_state && (!downloaded(out.second.data(), d_second.get(), n_reads, s, "reads' state") || !downloaded(out.events.data(), d_events.get(), used, s, "event array"))) ||
      !waited(s))
    return GTX_ERR_HIP;
  out.good_bits.assign(found_words, 0);
  return gtx_disc_second_decide(table.data(), nt, out.list.data(), n_list, out.support.data(), out.good_bits.data());
}

// ---- a region ---------------------------------------------------------------------------------------------------------------------
struct FileState // a file's arrays on the device and what its passes left
{
  DevPtr<uint8_t> planes, qual;
  DevPtr<gtx_disc_read> reads;
  DevPtr<uint32_t> cigar;
  uint32_t plane_stride = 0, qual_stride = 0, n_reads = 0, n_cigar = 0;
  std::vector<uint32_t> words; // of its first pass
  SecondResult second;
  gtx_discover_file_stats stats{};
  gtx_discover_front_stats front{};
  int rc = GTX_OK;
  std::string error;
};

struct Worker
{
  Disc disc;
  Stream stream;
  std::unique_ptr<gtx_inflate, Free<gtx_inflate_destroy>> inflater; // the device front's, made with its first file
};

// gtx_discover_region's way to "the file's arrays are on the device": the host arrays, uploaded
int load_arrays(Worker & w, gtx_disc_file const & f, FileState & st)
{
  hipStream_t const s = w.stream.get();
  if (int const rc = device_ready(w.disc->device, "gtx_discover_region", ": the object"))
    return rc;
  st.plane_stride = f.plane_stride;
  st.qual_stride = f.qual_stride;
  st.n_reads = f.n_reads;
  st.n_cigar = f.n_cigar;
  if (!uploaded(st.planes, f.planes, static_cast<size_t>(f.n_reads) * f.plane_stride, s, "plane rows") ||
      // (the walk reads the quality under any base of a plane row that differs from the region: a row's worth of room behind the last)
      !uploaded(st.qual, f.qual, static_cast<size_t>(f.n_reads) * f.qual_stride, s, "qualities", 2 * static_cast<size_t>(f.plane_stride)) || !uploaded(st.reads, f.reads, f.n_reads, s, "reads") ||
      !uploaded(st.cigar, f.cigar, f.n_cigar, s, "cigar words"))
    return GTX_ERR_HIP;
  return GTX_OK;
}

// gtx_discover_files' way there: the file read on the host and its tables checked, its record stream and the two tables uploaded, the
// host block freed, the unpack kernel.  The stream leaves the device when the kernel has run.
int load_bam(Worker & w, char const * path, FileState & st)
{
  hipStream_t const s = w.stream.get();
  if (int const rc = device_ready(w.disc->device, "gtx_discover_files", ": the object"))
    return rc;
  gtx_disc_bam * raw = nullptr;
  if (int const rc = gtx_disc_bam_read(path, &raw))
    return rc;
  std::unique_ptr<gtx_disc_bam, Free<gtx_disc_bam_destroy>> bam(raw);
  uint32_t const longest = bam->max_l_seq;
  size_t const n_bytes = bam->stream.size() - DISC_BAM_SLACK;
  st.plane_stride = std::max<uint32_t>((longest + 31u) / 32u * 16u, 16u);
  st.qual_stride = std::max<uint32_t>((longest + 3u) & ~3u, 4u);
  st.n_reads = static_cast<uint32_t>(bam->reads.size());
  st.n_cigar = static_cast<uint32_t>(bam->n_cigar);
  if (int const rc = disc_bam_unpack_check(n_bytes, bam->offsets.data(), bam->reads.data(), st.n_reads, st.plane_stride, st.qual_stride, st.n_cigar))
  {
    g_last_error += std::string(" (") + path + ")";
    return rc;
  }
  DevPtr<uint8_t> d_stream;
  DevPtr<uint32_t> d_offsets;
  WaitBehind const behind(s);
  if (!made(d_stream, bam->stream.size(), s, "record stream") || !copied_up(d_stream.get(), bam->stream.data(), bam->stream.size(), s, "record stream") ||
      !made(d_offsets, st.n_reads, s, "record offsets") || !copied_up(d_offsets.get(), bam->offsets.data(), st.n_reads, s, "record offsets") ||
      !made(st.reads, st.n_reads, s, "reads") || !copied_up(st.reads.get(), bam->reads.data(), st.n_reads, s, "reads") || !waited(s))
    return GTX_ERR_HIP;
  bam.reset(); // (the upload is done: the host block goes)
  // the kernel writes every byte of every row and every word; the room behind the last quality row is load_arrays'
  if (!made(st.planes, static_cast<size_t>(st.n_reads) * st.plane_stride, s, "plane rows") ||
      !made(st.qual, static_cast<size_t>(st.n_reads) * st.qual_stride, s, "qualities", 2 * static_cast<size_t>(st.plane_stride)) ||
      !made(st.cigar, st.n_cigar, s, "cigar words"))
    return GTX_ERR_HIP;
  if (int const rc = disc_bam_unpack_launch(d_stream.get(), d_offsets.get(), st.reads.get(), st.n_reads, st.planes.get(), st.plane_stride, st.qual.get(),
                                            st.qual_stride, st.cigar.get(), s))
    return rc;
  return waited(s) ? GTX_OK : GTX_ERR_HIP;
}

// ---- the device front ---------------------------------------------------------------------------------------------------------------
// A file's bytes, whole.  false: it cannot be opened or read (gtx_disc_bam_read then says so in its own words).
bool file_bytes(char const * path, std::vector<uint8_t> & out)
{
  std::unique_ptr<std::FILE, Free<std::fclose>> fp(std::fopen(path, "rb"));
  if (!fp || std::fseek(fp.get(), 0, SEEK_END) != 0)
    return false;
  long const size = std::ftell(fp.get());
  if (size < 0 || std::fseek(fp.get(), 0, SEEK_SET) != 0)
    return false;
  out.assign(static_cast<size_t>(size) + 8, 0); // (8 bytes behind the last member: the host decoder loads 8 at a time)
  return size == 0 || std::fread(out.data(), 1, static_cast<size_t>(size), fp.get()) == static_cast<size_t>(size);
}

// read_bam_header's reader over members that lie in memory: they are inflated on the host one by one, as far as the header reaches
struct MemberBytes
{
  uint8_t const * file;
  std::vector<gtx_inflate_member> const & members;
  size_t next = 0, at = 0;
  std::vector<uint8_t> data;
  long read(void * dst, size_t n)
  {
    while (data.size() - at < n && next < members.size())
    {
      gtx_inflate_member const & m = members[next++];
      size_t const before = data.size();
      data.resize(before + m.out_len);
      if (!inflate_bgzf_member(file + m.in_off, m.in_len, data.data() + before, m.out_len, !sw::inflate_zlib(), sw::bgzf_crc()))
        return -1;
    }
    size_t const got = std::min(n, data.size() - at);
    if (got)
      std::memcpy(dst, data.data() + at, got);
    at += got;
    return static_cast<long>(got);
  }
};

// The device front's way to "the file's arrays are on the device" (gtx.h: gtx_discover_files_front): the inflated bytes never leave
// the device.  GTX_OK with *sound = false: the file is not sound in some way and nothing of it is in `st` -- the caller sends it
// through load_bam, whose status and message are then the file's (the readers' device team's rule: what the device does not take
// the host does, so a damaged file fails exactly as it does there).
int load_bam_device(Worker & w, char const * path, FileState & st, bool * sound)
{
  *sound = false;
  hipStream_t const s = w.stream.get();
  if (int const rc = device_ready(w.disc->device, "gtx_discover_files_front", ": the object"))
    return rc;
  // the file, its members' headers, the BAM header
  std::vector<uint8_t> file;
  if (!file_bytes(path, file))
    return GTX_OK;
  uint64_t const file_len = file.size() - 8;
  std::vector<gtx_inflate_member> members;
  uint64_t total = 0;
  for (uint64_t at = 0; at < file_len;)
  {
    BgzfMember head;
    if (parse_bgzf_member(file.data() + at, file_len - at, head) != nullptr || !head.whole)
      return GTX_OK;
    if (head.isize) // (a member without data -- the end-of-file marker -- gets no descriptor and no cut)
      members.push_back(gtx_inflate_member{at + head.hlen, total, static_cast<uint32_t>(head.clen), head.isize, head.crc32, 0});
    total += head.isize;
    at += head.bsize + 1ull;
  }
  if (total >= (1ull << 32) || members.size() >= (1ull << 32))
    return GTX_OK;
  MemberBytes head_bytes{file.data(), members};
  BamHeader head;
  BamSamples table;
  if (read_bam_header(head_bytes, head) != BAM_HEADER_OK || !read_bam_samples(head.text, path, table) || table.samples.size() != 1) // (caller.cpp:2537-2544)
    return GTX_OK;
  uint64_t const header_len = head_bytes.at, n_bytes = total - header_len;
  st.front.members = static_cast<uint32_t>(members.size());
  if (n_bytes == 0) // a file without records
  {
    st.plane_stride = 16;
    st.qual_stride = 4;
    st.n_reads = st.n_cigar = 0;
    WaitBehind const behind(s);
    if (!made(st.planes, 0, s, "plane rows") || !made(st.qual, 0, s, "qualities", 2 * static_cast<size_t>(st.plane_stride)) || !made(st.reads, 0, s, "reads") ||
        !made(st.cigar, 0, s, "cigar words"))
      return GTX_ERR_HIP;
    st.front.members_device = 0; // (the header's members were the host's)
    *sound = true;
    return GTX_OK;
  }
  std::vector<uint32_t> cuts; // the member ends behind the header
  for (gtx_inflate_member const & m : members)
    if (m.out_off + m.out_len > header_len && m.out_off + m.out_len < total)
      cuts.push_back(static_cast<uint32_t>(m.out_off + m.out_len - header_len));
  if (!w.inflater)
  {
    gtx_inflate * h = nullptr;
    if (int const rc = gtx_inflate_create(w.disc->device, &h))
      return rc;
    w.inflater.reset(h);
  }
  // one upload, the inflate, the walk's count, one small download
  uint32_t const n_members = static_cast<uint32_t>(members.size()), n_cuts = static_cast<uint32_t>(cuts.size());
  DevPtr<uint8_t> d_file, d_out;
  DevPtr<gtx_inflate_member> d_members;
  DevPtr<uint32_t> d_status, d_cuts, d_offsets;
  DevPtr<BamWalkSeg> d_segs;
  DevPtr<gtx_bam_walk_out> d_walk;
  WaitBehind const behind(s);
  if (!made(d_file, file.size(), s, "file bytes") || !copied_up(d_file.get(), file.data(), file.size(), s, "file bytes") ||
      !made(d_members, n_members, s, "members") || !copied_up(d_members.get(), members.data(), n_members, s, "members") ||
      !made(d_cuts, n_cuts, s, "cuts") || !copied_up(d_cuts.get(), cuts.data(), n_cuts, s, "cuts") || !made(d_out, total, s, "inflated bytes") ||
      !made(d_status, n_members, s, "member statuses") || !made(d_segs, static_cast<size_t>(n_cuts) + 1, s, "segment table") || !made(d_walk, 1, s, "walk counts"))
    return GTX_ERR_HIP;
  if (int const rc = gtx_inflate_batch(w.inflater.get(), d_file.get(), file_len, d_members.get(), n_members, d_out.get(), total, d_status.get(), sw::bgzf_crc() ? 1 : 0, s))
    return rc;
  uint8_t const * const d_stream = d_out.get() + header_len;
  if (int const rc = disc_bam_walk_count(d_stream, static_cast<uint32_t>(n_bytes), d_cuts.get(), n_cuts, d_segs.get(), d_walk.get(), s))
    return rc;
  gtx_bam_walk_out walk{};
  std::vector<uint32_t> status(n_members);
  if (!downloaded(&walk, d_walk.get(), 1, s, "walk counts") || !downloaded(status.data(), d_status.get(), n_members, s, "member statuses") || !waited(s))
    return GTX_ERR_HIP;
  file = std::vector<uint8_t>(); // (the upload is done: the host block goes)
  if (std::any_of(status.begin(), status.end(), [](uint32_t m) { return m != GTX_INFLATE_OK; }) || walk.status != GTX_BAM_WALK_OK || walk.n_cigar >= (1ull << 32))
    return GTX_OK;
  // the tables from the count, the arrays with load_bam's strides, the unpack kernel
  st.plane_stride = std::max<uint32_t>((walk.max_l_seq + 31u) / 32u * 16u, 16u);
  st.qual_stride = std::max<uint32_t>((walk.max_l_seq + 3u) & ~3u, 4u);
  st.n_reads = walk.n_reads;
  st.n_cigar = static_cast<uint32_t>(walk.n_cigar);
  if (!made(d_offsets, st.n_reads, s, "record offsets") || !made(st.reads, st.n_reads, s, "reads") ||
      !made(st.planes, static_cast<size_t>(st.n_reads) * st.plane_stride, s, "plane rows") ||
      !made(st.qual, static_cast<size_t>(st.n_reads) * st.qual_stride, s, "qualities", 2 * static_cast<size_t>(st.plane_stride)) ||
      !made(st.cigar, st.n_cigar, s, "cigar words"))
    return GTX_ERR_HIP;
  if (st.n_reads)
    if (int const rc = disc_bam_walk_emit(d_stream, static_cast<uint32_t>(n_bytes), d_cuts.get(), n_cuts, d_segs.get(), d_offsets.get(), st.reads.get(), s))
      return rc;
  // disc_bam_unpack_check wants the two tables on the host; they are not there, and a walk that ended BAM_WALK_OK has held every one of
  // its conditions (gtx_disc_bam_walk_dev.hpp; tests/test_gpu_disc_bam_walk.py and tests/test_gpu_discover_front.py hold each):
  //   the strides            are made above from max_l_seq, the longest l_seq of the records the walk took: l_qseq <= qual_stride and
  //                          l_qseq <= 2 * plane_stride for every one of them, and plane_stride is a multiple of 16;
  //   cigar_off + n_cigar    cigar_off is the exclusive sum of n_cigar over the records in chain order and n_cigar their total (below
  //                          2^32, looked at above): every record's words lie inside the array by construction;
  //   the record             offsets[i] = o + 4 with 32 <= block <= n_bytes - o - 4 (the chain's test) and the counts within the block:
  //                          offsets[i] + 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq <= o + 4 + block <= n_bytes;
  //   the name's byte        is the stream's own, and it is the l_read_name of that same sum: the kernel, which takes it from the
  //                          stream, stays inside the block -- no 254 bytes of doubt as with a stream of another origin.
  if (int const rc = disc_bam_unpack_launch(d_stream, d_offsets.get(), st.reads.get(), st.n_reads, st.planes.get(), st.plane_stride, st.qual.get(), st.qual_stride,
                                            st.cigar.get(), s))
    return rc;
  if (!waited(s))
    return GTX_ERR_HIP;
  st.front.members_device = n_members;
  st.front.segments_hit = walk.segments_hit;
  st.front.segments_rewalked = walk.segments_rewalked;
  *sound = true;
  return GTX_OK;
}

int load_bam_front(Worker & w, char const * path, FileState & st)
{
  bool sound = false;
  if (int const rc = load_bam_device(w, path, st, &sound))
    return rc;
  if (sound)
    return GTX_OK;
  st.front = gtx_discover_front_stats{st.front.members, 0, 0, 0, 1, 0};
  return load_bam(w, path, st);
}

// a file's first pass over its arrays on the device
int first_pass(Worker & w, uint32_t file_index, gtx_discover_params const & p, FileState & st)
{
  hipStream_t const s = w.stream.get();
  gtx_disc * const d = w.disc.get();
  DevPtr<gtx_disc_event> d_events;
  DevPtr<uint32_t> d_counts;
  DevPtr<gtx_disc_read_out> d_read_out;
  WaitBehind const behind(s);
  uint64_t cap = p.first_event_cap ? p.first_event_cap : std::max<uint64_t>(8ull * st.n_reads, 4096);
  uint32_t counts[2] = {0, 0};
  if (!zeroed(d_read_out, st.n_reads, s, "read_out"))
    return GTX_ERR_HIP;
  for (;;) // (a pass whose buffer overflowed names the size it needs: one repeat)
  {
    ++st.stats.events_passes;
    if (!zeroed(d_events, cap, s, "events") || !zeroed(d_counts, 2, s, "event counters"))
      return GTX_ERR_HIP;
    if (int const rc = gtx_disc_events_batch(d, st.planes.get(), st.plane_stride, st.qual.get(), st.qual_stride, st.reads.get(), st.cigar.get(), st.n_reads,
                                             d_events.get(), static_cast<uint32_t>(cap), d_counts.get(), d_read_out.get(), s))
      return rc;
    if (!downloaded(counts, d_counts.get(), 2, s, "event counters") || !waited(s))
      return GTX_ERR_HIP;
    if (counts[1] == 0)
      break;
    if (counts[0] <= cap)
    {
      g_last_error = "gtx_discover: the events pass overflowed a buffer of the size it named";
      return GTX_ERR_HIP;
    }
    cap = counts[0];
  }
  st.stats.events = counts[0];
  uint64_t n_words = 0;
  st.words.assign(1 << 12, 0);
  for (int turn = 0;; ++turn)
  {
    int const rc = gtx_disc_first_pass_haplotypes_device(d, st.planes.get(), st.plane_stride, st.reads.get(), st.cigar.get(), d_read_out.get(), st.n_reads,
                                                         d_events.get(), d_counts.get(), p.bucket_size, static_cast<int32_t>(file_index), st.words.data(),
                                                         st.words.size(), &n_words, s);
    if (rc == GTX_ERR_CAPACITY && turn == 0 && n_words > st.words.size())
    {
      st.words.assign(n_words, 0);
      continue;
    }
    if (rc != GTX_OK)
      return rc;
    break;
  }
  st.words.resize(n_words);
  return GTX_OK;
}

// the files of one pass over the workers: file i on worker i % n_workers, each worker's files in their order.  What a file's run
// returns, with the thread's message, stays with the file; nothing is thrown across a thread's edge.
template <class Run>
void over_files(char const * who, std::vector<Worker> & workers, std::vector<FileState> & files, Run run)
{
  auto work = [&](size_t w)
  {
    for (size_t i = w; i < files.size(); i += workers.size())
    {
      try
      {
        files[i].rc = run(workers[w], i, files[i]);
        if (files[i].rc != GTX_OK)
          files[i].error = g_last_error;
      }
      catch (std::exception const & e)
      {
        files[i].rc = GTX_ERR_CAPACITY;
        files[i].error = std::string(who) + ": " + e.what();
      }
      if (files[i].rc != GTX_OK)
        return;
    }
  };
  if (workers.size() == 1)
  {
    work(0);
    return;
  }
  std::vector<std::thread> threads;
  try
  {
    for (size_t w = 0; w < workers.size(); ++w)
      threads.emplace_back(work, w);
  }
  catch (std::exception const &) // (a thread that could not be started: its files run here, behind the others)
  {
    for (size_t w = threads.size(); w < workers.size(); ++w)
      work(w);
  }
  for (std::thread & t : threads)
    t.join();
}

int first_error(std::vector<FileState> const & files)
{
  for (FileState const & f : files)
    if (f.rc != GTX_OK)
    {
      g_last_error = f.error;
      return f.rc;
    }
  return GTX_OK;
}

// load(worker, i, state): file i's arrays onto the device, their sizes into its state
template <class Load>
int discover(char const * who, char const * reference, uint64_t reference_len, int64_t region_begin, char const * contig, uint32_t n_files, gtx_discover_params const & p,
             gtx_discover_result & res, Load load)
{
  uint32_t const n_workers = std::min(p.n_threads, n_files);
  std::vector<Worker> workers(n_workers);
  for (Worker & w : workers)
  {
    gtx_disc * d = nullptr;
    if (int const rc = gtx_disc_create(reference, reference_len, region_begin, p.device, &d))
      return rc;
    w.disc.reset(d);
    if (int const rc = gtx_disc_set_max_read_len(d, p.max_read_len))
      return rc;
    hipStream_t s = nullptr;
    if (!hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "stream", MSG_PREFIX))
      return GTX_ERR_HIP;
    w.stream.reset(s);
  }
  std::vector<FileState> state(n_files); // (behind the workers: the files' blocks go back before the streams and the objects do)
  over_files(who, workers, state, [&](Worker & w, size_t i, FileState & st) {
    int const rc = load(w, i, st);
    return rc != GTX_OK ? rc : first_pass(w, static_cast<uint32_t>(i), p, st);
  });
  if (int const rc = first_error(state))
    return rc;
  // the merge, in file order
  std::vector<uint32_t> merged, next;
  for (FileState const & st : state)
  {
    uint64_t n = 0;
    next.assign(merged.size() + st.words.size() + 16, 0);
    int rc = gtx_disc_merge(merged.data(), merged.size(), st.words.data(), st.words.size(), next.data(), next.size(), &n);
    if (rc == GTX_ERR_CAPACITY)
    {
      next.assign(n, 0);
      rc = gtx_disc_merge(merged.data(), merged.size(), st.words.data(), st.words.size(), next.data(), next.size(), &n);
    }
    if (rc != GTX_OK)
      return rc;
    next.resize(n);
    merged.swap(next);
  }
  // the second pass of every file, from the arrays still resident
  over_files(who, workers, state, [&](Worker & w, size_t i, FileState & st) {
    return second_file(w.disc.get(), st.planes.get(), st.plane_stride, st.reads.get(), st.cigar.get(), st.n_reads, merged.data(), merged.size(),
                       static_cast<int32_t>(i), p.bucket_size, p.second_event_cap, false, w.stream.get(), st.second);
  });
  if (int const rc = first_error(state))
    return rc;
  // the OR of the good-bits, the records, the text
  uint32_t nt = 0;
  uint64_t n_seq = 0;
  {
    int const rc = gtx_disc_indel_table(merged.data(), merged.size(), nullptr, 0, &nt, nullptr, 0, &n_seq);
    if (rc != GTX_OK && rc != GTX_ERR_CAPACITY)
      return rc;
  }
  std::vector<gtx_disc_indel> table(nt);
  std::vector<char> table_letters(n_seq);
  if (int const rc = gtx_disc_indel_table(merged.data(), merged.size(), table.data(), nt, &nt, table_letters.data(), n_seq, &n_seq))
    return rc;
  std::vector<uint32_t> bits((nt + 31u) / 32u, 0);
  for (FileState & st : state)
  {
    for (size_t w = 0; w < bits.size() && w < st.second.good_bits.size(); ++w)
      bits[w] |= st.second.good_bits[w];
    st.stats.n_list = static_cast<uint32_t>(st.second.list.size());
    st.stats.rounds = st.second.stats;
    res.stats.push_back(st.stats);
    res.front.push_back(st.front);
  }
  res.good.resize(nt);
  for (uint32_t t = 0; t < nt; ++t)
    res.good[t] = table[t].good || ((bits[t >> 5] >> (t & 31u)) & 1u);
  gtx_disc const * const d = workers[0].disc.get();
  uint32_t n = 0;
  uint64_t n_letters = 0, n_ids = 0;
  {
    int const rc = gtx_disc_variants(d, merged.data(), merged.size(), bits.data(), nullptr, 0, &n, nullptr, 0, &n_letters, nullptr, 0, &n_ids);
    if (rc != GTX_OK && rc != GTX_ERR_CAPACITY)
      return rc;
  }
  res.variants.resize(n);
  res.letters.resize(n_letters);
  res.ids.resize(n_ids);
  if (int const rc = gtx_disc_variants(d, merged.data(), merged.size(), bits.data(), res.variants.data(), n, &n, res.letters.data(), n_letters, &n_letters,
                                       res.ids.data(), n_ids, &n_ids))
    return rc;
  uint64_t len = 0;
  {
    int const rc = gtx_disc_vcf_sites(res.variants.data(), n, res.letters.data(), n_letters, res.ids.data(), n_ids, contig, nullptr, 0, &len);
    if (rc != GTX_OK && rc != GTX_ERR_CAPACITY)
      return rc;
  }
  res.text.resize(len);
  if (int const rc = gtx_disc_vcf_sites(res.variants.data(), n, res.letters.data(), n_letters, res.ids.data(), n_ids, contig, &res.text[0], len, &len))
    return rc;
  res.words.swap(merged);
  return GTX_OK;
}
} // namespace

extern "C" int gtx_disc_second_file(gtx_disc * d, const uint8_t * d_planes, uint32_t plane_stride, const gtx_disc_read * d_reads, const uint32_t * d_cigar,
                                    uint32_t n_reads, const uint32_t * words, uint64_t n_words, int32_t file_index, uint32_t bucket_size, uint32_t event_cap,
                                    uint32_t * good_bits, uint32_t * list, uint32_t list_cap, uint32_t * n_list, gtx_disc_second_rounds_stats * stats,
                                    gtx_disc_second_read * second, gtx_disc_second_event * events, uint32_t events_cap, uint32_t * n_events,
                                    gtx_disc_second_support * support, void * stream)
{
  if (!d || !good_bits || !n_list || !stats || bucket_size == 0 || (n_words && !words) || (list_cap && !list) || (events_cap && !events) || (events && !n_events))
    return bad("gtx_disc_second_file");
  *n_list = 0;
  if (n_events)
    *n_events = 0;
  try
  {
    SecondResult r;
    int const rc = second_file(d, d_planes, plane_stride, d_reads, d_cigar, n_reads, words, n_words, file_index, bucket_size, event_cap,
                               second || n_events || support, static_cast<hipStream_t>(stream), r);
    if (rc != GTX_OK)
      return rc;
    *n_list = static_cast<uint32_t>(r.list.size());
    if (n_events)
      *n_events = static_cast<uint32_t>(r.events.size());
    if (r.list.size() > list_cap || (n_events && r.events.size() > events_cap))
    {
      g_last_error = "gtx_disc_second_file: the list or the event array does not fit";
      return GTX_ERR_CAPACITY;
    }
    std::copy(r.good_bits.begin(), r.good_bits.end(), good_bits);
    std::copy(r.list.begin(), r.list.end(), list);
    *stats = r.stats;
    if (second)
      std::copy(r.second.begin(), r.second.end(), second);
    if (n_events)
      std::copy(r.events.begin(), r.events.end(), events);
    if (support)
      std::copy(r.support.begin(), r.support.end(), support);
    return GTX_OK;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_disc_second_file: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" void gtx_discover_params_default(gtx_discover_params * p)
{
  if (p)
    *p = gtx_discover_params{0, 50, 0, 1, 0, 0};
}

extern "C" int gtx_discover_region(const char * reference, uint64_t reference_len, int64_t region_begin, const char * contig, const gtx_disc_file * files,
                                   uint32_t n_files, const gtx_discover_params * params, gtx_discover_result ** out)
{
  if (!out)
    return bad("gtx_discover_region");
  *out = nullptr;
  if (!reference || reference_len == 0 || !contig || !files || n_files == 0 || !params || params->bucket_size == 0 || params->n_threads == 0 ||
      params->n_threads > 8)
    return bad("gtx_discover_region");
  for (uint32_t i = 0; i < n_files; ++i)
  {
    gtx_disc_file const & f = files[i];
    if (f.plane_stride == 0 || (f.n_reads && (!f.planes || !f.qual || !f.reads || f.qual_stride == 0)) || (f.n_cigar && !f.cigar))
      return bad("gtx_discover_region", "a file's arrays");
    for (uint32_t r = 0; r < f.n_reads; ++r) // (the kernels index the cigar words and the quality rows by these)
    {
      if (static_cast<uint64_t>(f.reads[r].cigar_off) + f.reads[r].n_cigar > f.n_cigar)
        return bad("gtx_discover_region", "a read's cigar words lie behind the file's");
      if (f.reads[r].l_qseq > f.qual_stride)
        return bad("gtx_discover_region", "a read is longer than its quality row");
    }
  }
  if (params->device < 0)
  {
    g_last_error = "gtx_discover_region: no device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  try
  {
    auto res = std::make_unique<gtx_discover_result>();
    int const rc = discover("gtx_discover_region", reference, reference_len, region_begin, contig, n_files, *params, *res,
                            [&](Worker & w, size_t i, FileState & st) { return load_arrays(w, files[i], st); });
    if (rc == GTX_OK)
      *out = res.release();
    return rc;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_discover_region: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" int gtx_discover_files(const char * reference, uint64_t reference_len, int64_t region_begin, const char * contig, const char * const * bam_paths,
                                  uint32_t n_files, const gtx_discover_params * params, gtx_discover_result ** out)
{
  if (!out)
    return bad("gtx_discover_files");
  *out = nullptr;
  if (!reference || reference_len == 0 || !contig || !bam_paths || n_files == 0 || !params || params->bucket_size == 0 || params->n_threads == 0 ||
      params->n_threads > 8)
    return bad("gtx_discover_files");
  for (uint32_t i = 0; i < n_files; ++i)
    if (!bam_paths[i])
      return bad("gtx_discover_files", "a path");
  if (params->device < 0) // (before any file is opened)
  {
    g_last_error = "gtx_discover_files: no device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  try
  {
    auto res = std::make_unique<gtx_discover_result>();
    int const rc = discover("gtx_discover_files", reference, reference_len, region_begin, contig, n_files, *params, *res,
                            [&](Worker & w, size_t i, FileState & st) { return load_bam(w, bam_paths[i], st); });
    if (rc == GTX_OK)
      *out = res.release();
    return rc;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_discover_files: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" int gtx_discover_files_front(const char * reference, uint64_t reference_len, int64_t region_begin, const char * contig, const char * const * bam_paths,
                                        uint32_t n_files, const gtx_discover_params * params, uint32_t front, gtx_discover_result ** out)
{
  if (front == 0)
    return gtx_discover_files(reference, reference_len, region_begin, contig, bam_paths, n_files, params, out);
  if (!out)
    return bad("gtx_discover_files_front");
  *out = nullptr;
  if (front != 1)
    return bad("gtx_discover_files_front", "no such front");
  if (!reference || reference_len == 0 || !contig || !bam_paths || n_files == 0 || !params || params->bucket_size == 0 || params->n_threads == 0 ||
      params->n_threads > 8)
    return bad("gtx_discover_files_front");
  for (uint32_t i = 0; i < n_files; ++i)
    if (!bam_paths[i])
      return bad("gtx_discover_files_front", "a path");
  if (params->device < 0) // (before any file is opened)
  {
    g_last_error = "gtx_discover_files_front: no device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  try
  {
    auto res = std::make_unique<gtx_discover_result>();
    int const rc = discover("gtx_discover_files_front", reference, reference_len, region_begin, contig, n_files, *params, *res,
                            [&](Worker & w, size_t i, FileState & st) { return load_bam_front(w, bam_paths[i], st); });
    if (rc == GTX_OK)
      *out = res.release();
    return rc;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string("gtx_discover_files_front: ") + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" const gtx_discover_front_stats * gtx_discover_front(const gtx_discover_result * r, uint32_t * n_files)
{
  if (n_files)
    *n_files = r ? static_cast<uint32_t>(r->front.size()) : 0;
  return r ? r->front.data() : nullptr;
}

extern "C" void gtx_discover_destroy(gtx_discover_result * r) { delete r; }

extern "C" const char * gtx_discover_text(const gtx_discover_result * r, uint64_t * len)
{
  if (len)
    *len = r ? r->text.size() : 0;
  return r ? r->text.data() : nullptr;
}

extern "C" const gtx_disc_variant * gtx_discover_variants(const gtx_discover_result * r, uint32_t * n, const char ** letters, uint64_t * n_letters,
                                                          const uint32_t ** ids, uint64_t * n_ids)
{
  if (n)
    *n = r ? static_cast<uint32_t>(r->variants.size()) : 0;
  if (letters)
    *letters = r ? r->letters.data() : nullptr;
  if (n_letters)
    *n_letters = r ? r->letters.size() : 0;
  if (ids)
    *ids = r ? r->ids.data() : nullptr;
  if (n_ids)
    *n_ids = r ? r->ids.size() : 0;
  return r ? r->variants.data() : nullptr;
}

extern "C" const uint32_t * gtx_discover_words(const gtx_discover_result * r, uint64_t * n_words)
{
  if (n_words)
    *n_words = r ? r->words.size() : 0;
  return r ? r->words.data() : nullptr;
}

extern "C" const uint8_t * gtx_discover_good(const gtx_discover_result * r, uint32_t * n_table)
{
  if (n_table)
    *n_table = r ? static_cast<uint32_t>(r->good.size()) : 0;
  return r ? r->good.data() : nullptr;
}

extern "C" const gtx_discover_file_stats * gtx_discover_stats(const gtx_discover_result * r, uint32_t * n_files)
{
  if (n_files)
    *n_files = r ? static_cast<uint32_t>(r->stats.size()) : 0;
  return r ? r->stats.data() : nullptr;
}
