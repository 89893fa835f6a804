// gtx_pipeline.cpp -- the host loop around the path, inside the library.
//
// gtx_pipeline_run replaces the reference's worker threads over BAM pools (Caller: src/typer/caller.cpp:399-436, each running
// parallel_reader_genotype_only, src/utilities/hts_parallel_reader.cpp:245-338: read a record, filter it, align it, score it):
// T host threads, each with its own group of BAM files, run
//   gtx_reads_next (BGZF members inflated by the library's team, records in the reference's merged order)
//   -> gtx_stream_push (flag filter, duplicate reuse, mate parking; reads leave as plane rows)
//   -> pinned staging -> H2D -> gtx_align_batch_planes -> gtx_score_batch_flags
// on a stream of their own, against ONE context and ONE accumulator block (every per-read effect is an integer addition:
// the block does not depend on which thread scored a read).  Two staging sets per thread: while the device works on one
// batch the thread decodes the next.  What a host language has to add is what follows the loop: gtx_calls_batch,
// gtx_vcf_records.
// Reads of up to the context's max_read_len: the BAM nibbles are decoded into rows that hold the longest of them, and each batch
// is staged as plane rows of the pitch its own longest read needs (80 bytes for reads of up to 160 bases, as before long reads
// were taken).  A staging set is made for 80-byte rows and grows the first time a batch needs more.  What the stream keeps
// across batches (the previous read's bases for duplicate reuse, parked mates) is nibbles and task numbers: the pitch may
// change from one batch to the next.
// What a thread holds (staging sets, record slots, the stream's state, a stream of the context's) is given back by its owners
// (gtx_host_loops.hpp) when the thread's run ends.
#include "gtx_ctx.hpp"
#include "gtx_host_loops.hpp"
#include "gtx_switches.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace
{
using gtx::seconds_since;

constexpr uint32_t MIN_PITCH = 80;   // plane rows of reads of up to 160 bases: every batch gets at least these
constexpr uint32_t GROUP_BYTES = 16; // a plane row's group of 32 bases (gtx.h, gtx_pack_planes)

struct Worker
{
  gtx::Reads reads;
  uint32_t n_samples = 0, n_rg = 0;
  std::vector<uint32_t> sample_of; // the group's sample -> the run's
  bool renumber = false;
  std::vector<std::string> paths;
  double decode = 0, push = 0, enqueue = 0;
  uint64_t records = 0, tasks = 0, items = 0, failed = 0;
  int status = GTX_OK;
  std::string error;
};

// a thread's stream is one of the context's (gtx_ctx::pipeline_streams_all: they live as long as it does): it goes back to the
// idle ones once everything queued on it has run
struct ReturnIdle
{
  gtx_ctx * c = nullptr;
  void operator()(hipStream_t st) const
  {
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lock(c->pipeline_mutex);
    c->pipeline_streams_idle.push_back(st);
  }
};

// one staging set: a batch's plane rows, metas and score items, pinned and on the device, and the event of the work that reads them
struct Staging
{
  gtx::Event done;
  gtx::PinnedPtr<uint8_t> pin_seq;
  gtx::PinnedPtr<gtx_read_meta> pin_meta;
  gtx::PinnedPtr<gtx_score_item> pin_items;
  gtx::DevPtr<uint8_t> dev_seq;
  gtx::DevPtr<gtx_read_meta> dev_meta;
  gtx::DevPtr<gtx_score_item> dev_items;
  size_t rows = 0;                // reads (and score items) it holds
  uint32_t cap_pitch = MIN_PITCH; // the plane rows it holds
  uint32_t pitch = MIN_PITCH;     // the pitch of the batch it holds
  bool used = false;

  bool make(uint32_t chunk)
  {
    rows = chunk;
    hipEvent_t e = nullptr;
    bool const ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    done.reset(e);
    return ok && gtx::alloc(pin_seq, rows * MIN_PITCH) && gtx::alloc(pin_meta, rows * sizeof(gtx_read_meta)) && gtx::alloc(pin_items, rows * sizeof(gtx_score_item)) &&
           gtx::alloc(dev_seq, rows * MIN_PITCH) && gtx::alloc(dev_meta, rows * sizeof(gtx_read_meta)) && gtx::alloc(dev_items, rows * sizeof(gtx_score_item));
  }
  // room for plane rows of p bytes (behind `done`: nothing uses the set)
  bool grow(uint32_t p)
  {
    if (p <= cap_pitch)
      return true;
    pin_seq.reset();
    dev_seq.reset();
    if (!gtx::alloc(pin_seq, rows * p) || !gtx::alloc(dev_seq, rows * p))
      return false;
    cap_pitch = p;
    return true;
  }
};

// one host thread of gtx_pipeline_run: its group of files through gtx_stream_push and the device, on a stream of its own
struct ThreadLoop
{
  gtx_ctx * c;
  gtx_score_buffers const * acc;
  uint32_t chunk, rec_words;
  uint64_t slots; // record_slots_per_thread
  Worker & w;
  // (owners end in the reverse order: the stream goes back to the context after everything that was used on it)
  std::unique_ptr<ihipStream_t, ReturnIdle> st{nullptr, ReturnIdle{c}};
  gtx::DriverPtr<uint32_t> d_rec;
  gtx::DriverPtr<uint8_t> d_fl;
  Staging set[2];
  gtx::ReadStream push;
  uint64_t at = 0; // tasks of this thread so far: the stream numbers them over all its records

  void fail(int status, std::string const & what)
  {
    w.status = status;
    w.error = what;
  }

  // an idle stream of the context, or one made (and kept by the context from now on)
  void lease_stream()
  {
    hipStream_t idle = nullptr, made = nullptr;
    {
      std::lock_guard<std::mutex> lock(c->pipeline_mutex);
      if (!c->pipeline_streams_idle.empty())
      {
        idle = static_cast<hipStream_t>(c->pipeline_streams_idle.back());
        c->pipeline_streams_idle.pop_back();
      }
    }
    if (!idle && hipStreamCreateWithFlags(&made, hipStreamNonBlocking) == hipSuccess)
    {
      std::lock_guard<std::mutex> lock(c->pipeline_mutex);
      c->pipeline_streams_all.emplace_back(made);
    }
    st.reset(idle ? idle : made);
  }

  bool submit(Staging & s, uint32_t na, uint32_t ni)
  {
    if ((na && (hipMemcpyAsync(s.dev_seq.get(), s.pin_seq.get(), static_cast<size_t>(na) * s.pitch, hipMemcpyHostToDevice, st.get()) != hipSuccess ||
                hipMemcpyAsync(s.dev_meta.get(), s.pin_meta.get(), static_cast<size_t>(na) * sizeof(gtx_read_meta), hipMemcpyHostToDevice, st.get()) != hipSuccess)) ||
        (ni && hipMemcpyAsync(s.dev_items.get(), s.pin_items.get(), static_cast<size_t>(ni) * sizeof(gtx_score_item), hipMemcpyHostToDevice, st.get()) != hipSuccess))
    {
      fail(GTX_ERR_HIP, "gtx_pipeline_run: host to device copy");
      return false;
    }
    int rc = GTX_OK;
    if (na)
      rc = gtx_align_batch_planes(c, s.dev_seq.get(), s.pitch, s.dev_meta.get(), na, d_rec.get() + at * 2 * rec_words, rec_words, d_fl.get() + at * 2, st.get());
    if (rc == GTX_OK && ni)
      rc = gtx_score_batch_flags(c, s.dev_items.get(), ni, d_rec.get(), rec_words, d_fl.get(), acc, st.get());
    if (rc != GTX_OK)
    {
      fail(rc, gtx_last_error());
      return false;
    }
    (void)hipEventRecord(s.done.get(), st.get());
    s.used = true;
    at += na;
    w.tasks += na;
    w.items += ni;
    return true;
  }

  // the end of the stream: reads still waiting for their mate (SV calling scores them on their own), through staging set 0
  void flush_parked()
  {
    uint64_t n_rec = 0, n_dup = 0, n_parked = 0;
    gtx_stream_counts(push.get(), &n_rec, &n_dup, &n_parked);
    std::vector<gtx_score_item> left(std::max<uint64_t>(n_parked, 1));
    uint32_t ni = 0;
    int const rc_fin = gtx_stream_finish(push.get(), left.data(), static_cast<uint32_t>(left.size()), &ni);
    if (rc_fin != GTX_OK) // (parked mates left unscored are a wrong result, not a detail)
    {
      w.status = rc_fin;
      return;
    }
    Staging & s = set[0];
    if (ni && s.used && hipEventSynchronize(s.done.get()) != hipSuccess)
      w.status = GTX_ERR_HIP;
    for (uint32_t o = 0; o < ni && w.status == GTX_OK; o += chunk)
    {
      uint32_t const m = std::min(chunk, ni - o);
      std::memcpy(s.pin_items.get(), left.data() + o, static_cast<size_t>(m) * sizeof(gtx_score_item));
      if (submit(s, 0, m) && hipEventSynchronize(s.done.get()) != hipSuccess)
        w.status = GTX_ERR_HIP;
    }
  }

  void run(std::atomic<uint32_t> & ready, std::atomic<uint32_t> const & go)
  {
    if (hipSetDevice(c->device) != hipSuccess)
    {
      fail(GTX_ERR_HIP, "hipSetDevice");
      ready.fetch_add(1); // (the others wait for every thread to be counted)
      return;
    }
    uint32_t const max_len = gtx::max_read_len_of(c->params);
    uint32_t const nibble_stride = (max_len + 1) / 2; // gtx_reads_next's rows: the context's longest read
    uint32_t stream_pitch = MIN_PITCH;                // what gtx_stream_push writes
    lease_stream();
    bool ok = st && set[0].make(chunk) && set[1].make(chunk);
    size_t const rec_bytes = static_cast<size_t>(slots) * 2 * rec_words * 4, fl_bytes = static_cast<size_t>(slots) * 2;
    // (the record slots are large and live for one run: straight from the driver, not through the library's cache of freed blocks --
    //  sixteen of them would fill it and turn every later context's small allocations into driver calls)
    ok = ok && gtx::alloc(d_rec, rec_bytes) && gtx::alloc(d_fl, fl_bytes) && hipMemsetAsync(d_rec.get(), 0, rec_bytes, st.get()) == hipSuccess &&
         hipMemsetAsync(d_fl.get(), 0, fl_bytes, st.get()) == hipSuccess;
    if (!ok)
      fail(GTX_ERR_HIP, "gtx_pipeline_run: could not allocate a thread's staging buffers / record slots");
    gtx_stream * raw = nullptr;
    if (ok && gtx_stream_create(&c->params, std::max(1u, w.n_rg), &raw) != GTX_OK)
    {
      ok = false;
      fail(GTX_ERR_ARG, gtx_last_error());
    }
    push.reset(raw);
    if (ok)
      gtx_stream_set_planes(push.get(), stream_pitch);
    std::vector<gtx_stream_record> recs(chunk);
    std::vector<uint8_t> seq(static_cast<size_t>(chunk) * nibble_stride);
    if (st)
      (void)hipStreamSynchronize(st.get());
    // every thread has its buffers: the loop's clock starts when the last one gets here
    ready.fetch_add(1);
    while (go.load(std::memory_order_acquire) == 0)
      std::this_thread::yield();
    for (int b = 0; ok; b ^= 1)
    {
      Staging & s = set[b];
      auto t0 = std::chrono::steady_clock::now();
      uint32_t n = 0;
      int rc = gtx_reads_next(w.reads.get(), recs.data(), seq.data(), nibble_stride, chunk, &n);
      w.decode += seconds_since(t0);
      uint32_t longest = 0;
      for (uint32_t i = 0; rc == GTX_OK && i < n; ++i)
        longest = std::max<uint32_t>(longest, recs[i].l_qseq);
      if (rc == GTX_ERR_ARG && gtx::reads_refused_len(w.reads.get())) // (a read longer than the nibble rows: longer than the context takes)
        longest = gtx::reads_refused_len(w.reads.get());
      if (longest > max_len)
      {
        fail(GTX_ERR_UNSUPPORTED, "gtx_pipeline_run: a read of " + std::to_string(longest) + " bases (the context's max_read_len is " + std::to_string(max_len) + ")");
        break;
      }
      if (rc != GTX_OK)
      {
        fail(rc, gtx_last_error());
        break;
      }
      if (n == 0)
        break;
      if (w.renumber)
        for (uint32_t i = 0; i < n; ++i)
          recs[i].sample = w.sample_of[recs[i].sample];
      t0 = std::chrono::steady_clock::now();
      if (s.used)
        (void)hipEventSynchronize(s.done.get()); // the staging set is free again
      // the batch's plane rows: as wide as its longest read needs (16 bytes per 32 bases), never narrower than 80 bytes
      uint32_t const pitch = std::max(MIN_PITCH, (longest + 31) / 32 * GROUP_BYTES);
      if (!s.grow(pitch))
      {
        fail(GTX_ERR_HIP, "gtx_pipeline_run: could not grow a thread's staging buffers to plane rows of " + std::to_string(pitch) + " bytes");
        break;
      }
      if (pitch != stream_pitch)
      {
        gtx_stream_set_planes(push.get(), pitch);
        stream_pitch = pitch;
      }
      s.pitch = pitch;
      uint32_t na = 0, ni = 0;
      rc = gtx_stream_push(push.get(), recs.data(), seq.data(), nibble_stride, n, s.pin_seq.get(), s.pin_meta.get(), chunk, &na, s.pin_items.get(), chunk, &ni);
      w.push += seconds_since(t0);
      if (rc != GTX_OK)
      {
        fail(rc, gtx_last_error());
        break;
      }
      if (at + na > slots)
      {
        fail(GTX_ERR_CAPACITY, "gtx_pipeline_run: more reads to align in a thread's files than record_slots_per_thread");
        break;
      }
      t0 = std::chrono::steady_clock::now();
      if (!submit(s, na, ni))
        break;
      w.enqueue += seconds_since(t0);
      w.records += n;
    }
    if (w.status == GTX_OK && push)
      flush_parked();
    if (st && hipStreamSynchronize(st.get()) != hipSuccess && w.status == GTX_OK)
      w.status = GTX_ERR_HIP;
    // (records that are a table-overflow status instead of a result: reads the accumulators lack)
    if (w.status == GTX_OK && at && d_rec)
    {
      uint64_t failed = 0;
      int const rc = gtx_records_failed(c, d_rec.get(), rec_words, at, st.get(), &failed);
      if (rc != GTX_OK)
        fail(rc, gtx_last_error());
      w.failed = failed;
    }
  }
};
} // namespace

extern "C" int gtx_pipeline_run(gtx_ctx * c, const char * const * bam_paths, uint32_t n_paths, uint32_t n_threads, const char * region, uint32_t chunk,
                                uint32_t rec_words, uint64_t record_slots_per_thread, const gtx_score_buffers * acc, gtx_pipeline_stats * stats)
{
  using gtx::g_last_error;
  if (!c || !bam_paths || n_paths == 0 || n_threads == 0 || chunk == 0 || rec_words < 8 || record_slots_per_thread == 0 || !acc)
  {
    g_last_error = "gtx_pipeline_run: bad argument";
    return GTX_ERR_ARG;
  }
  if (int const rc = gtx::device_ready(c->device, "context"))
    return rc;
  auto const t_all = std::chrono::steady_clock::now();
  n_threads = std::min(n_threads, n_paths);
  std::vector<Worker> team(n_threads);
  for (uint32_t f = 0; f < n_paths; ++f)
    team[f % n_threads].paths.push_back(bam_paths[f] ? bam_paths[f] : "");
  // GTX_BGZF_DEVICE=1: the readers' BGZF members are inflated by the context's device (gtx_reads_set_inflate_device)
  bool const bgzf_on_device = gtx::sw::bgzf_device();
  int const device = c->device;
  // the files are opened first (one thread each): the samples' numbers need every group's names
  {
    std::vector<std::thread> openers;
    for (Worker & w : team)
      openers.emplace_back([&w, region, bgzf_on_device, device]
      {
        std::vector<char const *> p;
        for (auto const & s : w.paths)
          p.push_back(s.c_str());
        gtx_reads * raw = nullptr;
        w.status = gtx_reads_open(p.data(), static_cast<uint32_t>(p.size()), region, &raw);
        w.reads.reset(raw);
        if (w.status == GTX_OK && bgzf_on_device)
          w.status = gtx_reads_set_inflate_device(raw, device);
        if (w.status != GTX_OK)
          w.error = gtx_last_error();
        else
          gtx_reads_info(w.reads.get(), &w.n_samples, &w.n_rg);
      });
    for (auto & t : openers)
      t.join();
  }
  int status = GTX_OK;
  uint32_t samples = 0;
  std::vector<std::string> names;
  for (Worker & w : team)
  {
    if (w.status != GTX_OK && status == GTX_OK)
    {
      status = w.status;
      g_last_error = w.error;
    }
    // samples are numbered by name in the order the groups bring them (position-sliced files of one sample are one sample)
    for (uint32_t i = 0; w.reads && i < w.n_samples; ++i)
    {
      char const * nm = gtx_reads_sample_name(w.reads.get(), i);
      std::string const name = nm ? nm : "";
      auto it = std::find(names.begin(), names.end(), name);
      w.sample_of.push_back(static_cast<uint32_t>(it - names.begin()));
      if (it == names.end())
        names.push_back(name);
      w.renumber = w.renumber || w.sample_of.back() != i;
    }
    samples = static_cast<uint32_t>(names.size());
  }
  if (status == GTX_OK && samples > acc->n_samples)
  {
    status = GTX_ERR_ARG;
    g_last_error = "gtx_pipeline_run: the files hold " + std::to_string(samples) + " samples, the accumulator block " + std::to_string(acc->n_samples);
  }
  // (the context's and the block's counters of refused work before the run: what the run adds is the run's)
  uint32_t refused_before = 0, conn_dropped_before = 0;
  if (status == GTX_OK)
  {
    uint32_t conn[2] = {0, 0};
    (void)gtx_ctx_error_count(c, &refused_before);
    if (acc->d_conn_count && hipSetDevice(c->device) == hipSuccess && hipMemcpy(conn, acc->d_conn_count, sizeof conn, hipMemcpyDeviceToHost) == hipSuccess)
      conn_dropped_before = conn[1];
  }
  std::atomic<uint32_t> ready{0}, go{0};
  double t_loop = 0;
  if (status == GTX_OK)
  {
    std::vector<std::thread> threads;
    for (Worker & w : team)
      threads.emplace_back([&, wp = &w] { ThreadLoop{c, acc, chunk, rec_words, record_slots_per_thread, *wp}.run(ready, go); });
    while (ready.load() < n_threads)
      std::this_thread::yield();
    auto const t0 = std::chrono::steady_clock::now();
    go.store(1, std::memory_order_release);
    for (auto & t : threads)
      t.join();
    t_loop = seconds_since(t0);
  }
  gtx_pipeline_stats s{};
  for (Worker & w : team)
  {
    w.reads.reset();
    if (w.status != GTX_OK && status == GTX_OK)
    {
      status = w.status;
      g_last_error = w.error;
    }
    s.records_failed += w.failed;
    s.records += w.records;
    s.tasks += w.tasks;
    s.items += w.items;
    s.decode_s += w.decode;
    s.push_s += w.push;
    s.enqueue_s += w.enqueue;
    s.slowest_thread_s = std::max(s.slowest_thread_s, w.decode + w.push + w.enqueue);
  }
  // What a capacity limit of the library dropped makes the block a wrong result, not a smaller one: records with a table-overflow
  // status, score items over more sites than the scorer's table, far-pair connections beyond the log.  (acc is then undefined.)
  if (status == GTX_OK && c->device >= 0)
  {
    uint32_t refused = 0, conn[2] = {0, 0};
    (void)gtx_ctx_error_count(c, &refused);
    if (acc->d_conn_count)
      (void)hipMemcpy(conn, acc->d_conn_count, sizeof conn, hipMemcpyDeviceToHost);
    s.score_items_refused = refused >= refused_before ? refused - refused_before : refused;
    s.connections_dropped = conn[1] >= conn_dropped_before ? conn[1] - conn_dropped_before : conn[1];
    if (s.records_failed || s.score_items_refused || s.connections_dropped)
    {
      status = GTX_ERR_CAPACITY;
      g_last_error = "gtx_pipeline_run: the result is incomplete -- " + gtx::incomplete_counts(s.records_failed, s.score_items_refused, s.connections_dropped) +
                     " (gtx_params.exact_pass_mb / big_record_words, gtx_scores_alloc's conn_cap)";
    }
  }
  s.n_samples = samples;
  s.n_threads = n_threads;
  s.loop_s = t_loop;
  s.wall_s = seconds_since(t_all);
  if (stats)
    *stats = s;
  return status;
}
