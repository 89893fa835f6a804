// gtx_bgzf.cpp -- the BGZF layer (gtx_bgzf.hpp): reading a member, inflating it on the host, the reader with the host's and
// the device's inflating teams; and the two entry points that are BGZF and nothing else, gtx_bgzf_compress and gtx_inflate_raw.
#include "gtx_bgzf.hpp"
#include "gtx_ctx.hpp"
#include "gtx_inflate.hpp"
#include "gtx_inflate_host.hpp"
#include "gtx_switches.hpp"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>

gtx::InflateDeviceOps const * gtx::inflate_device_ops = nullptr;

namespace gtx
{
namespace
{
std::atomic<uint64_t> g_members_device{0};   // inflated by the device, status ok
std::atomic<uint64_t> g_members_fallback{0}; // taken by the device's team and then inflated on the host: a status but ok, or a launch that failed
std::atomic<uint64_t> g_members_reader{0};   // inflated by their reader before the team had started on them

// the two switches of the BAM readers, read once each (when the first member is inflated)
bool env_own_decoder()
{
  static bool const own = !sw::inflate_zlib();
  return own;
}
bool env_check_crc()
{
  static bool const check = sw::bgzf_crc();
  return check;
}
} // namespace

InflateCounts inflate_counts() { return InflateCounts{g_members_device.load(), g_members_fallback.load(), g_members_reader.load()}; }

MemberRead read_bgzf_member(std::FILE * fp, BgzfMember & m, std::vector<uint8_t> & rest)
{
  uint8_t first[18];
  size_t const got = std::fread(first, 1, 18, fp);
  if (got == 0)
    return MEMBER_END;
  char const * why = parse_bgzf_member(first, got, m);
  if (why && m.hlen > 18) // (an extra field with more than BC in it: the rest of the header, and again)
  {
    std::vector<uint8_t> head(m.hlen);
    std::memcpy(head.data(), first, 18);
    if (std::fread(head.data() + 18, 1, m.hlen - 18u, fp) != m.hlen - 18u)
      return MEMBER_BROKEN;
    why = parse_bgzf_member(head.data(), head.size(), m);
  }
  if (why)
    return MEMBER_BROKEN;
  rest.resize(static_cast<size_t>(m.clen) + 8);
  if (std::fread(rest.data(), 1, rest.size(), fp) != rest.size())
    return MEMBER_BROKEN;
  std::memcpy(&m.crc32, rest.data() + m.clen, 4);
  std::memcpy(&m.isize, rest.data() + m.clen + 4, 4);
  return m.isize > 65536 ? MEMBER_BROKEN : MEMBER_OK;
}

bool inflate_bgzf_member(uint8_t const * rest, size_t clen, uint8_t * out, size_t isize, bool use_own, bool check_crc)
{
  uint32_t want = 0;
  std::memcpy(&want, rest + clen, 4);
  if (use_own && inflate_raw(rest, clen, out, isize) && (!check_crc || crc32_of(out, isize) == want))
    return true;
  z_stream z{}; // (zlib gets the member; a member that is damaged stays damaged)
  if (inflateInit2(&z, -15) != Z_OK)
    return false;
  z.next_in = const_cast<Bytef *>(rest);
  z.avail_in = static_cast<uInt>(clen);
  z.next_out = out;
  z.avail_out = static_cast<uInt>(isize);
  int const rc = inflate(&z, Z_FINISH);
  inflateEnd(&z);
  return rc == Z_STREAM_END && z.avail_out == 0 && (!check_crc || crc32_of(out, isize) == want);
}

struct InflateJob
{
  std::vector<uint8_t> comp, data;
  long clen = 0;
  std::atomic<int> state{2}; // 0 queued, 1 being inflated, 2 done
  bool ok = false;
  std::mutex m;
  std::condition_variable cv;
};

namespace
{
void inflate_member(InflateJob & j)
{
  j.ok = inflate_bgzf_member(j.comp.data(), static_cast<size_t>(j.clen), j.data.data(), j.data.size(), env_own_decoder(), env_check_crc());
  // (notified under the lock: the reader may free the job as soon as it sees it done, and it sees that only after
  // this thread has let go of the mutex -- the last thing it touches)
  std::lock_guard<std::mutex> lock(j.m);
  j.state.store(2);
  j.cv.notify_all();
}

// A team that lives while somebody uses it: the one instance, its users, and the lock of both.
template <class Team>
struct TeamSlot
{
  std::mutex gate;
  int users = 0;
  Team * self = nullptr;
  void release()
  {
    Team * gone = nullptr;
    {
      std::lock_guard<std::mutex> lock(gate);
      if (--users == 0)
      {
        gone = self;
        self = nullptr;
      }
    }
    delete gone;
  }
};

// takes the jobs [first, last) of a reader that goes away out of a team's queue (under the team's lock)
void forget_jobs(std::deque<InflateJob *> & queue, InflateJob const * first, InflateJob const * last)
{
  queue.erase(std::remove_if(queue.begin(), queue.end(), [&](InflateJob * j) { return j >= first && j < last; }), queue.end());
}

class InflateTeam
{
public:
  static void acquire()
  {
    std::lock_guard<std::mutex> lock(slot().gate);
    if (slot().users++ == 0)
    {
      slot().self = new InflateTeam(sw::bgzf_threads(std::min(std::max(std::thread::hardware_concurrency(), 1u), 16u)));
    }
  }
  static void release() { slot().release(); }
  // hands queued jobs to the team (no team: they stay queued and their reader inflates them when it gets there).  The
  // caller wakes at most ONE sleeping worker, and only when nobody is looking at the queue already: waking a thread costs the
  // caller a system call -- a third of a millisecond where the host is a virtual machine and the worker's core is halted,
  // as long as inflating the member takes -- so workers wake each other (run()) and linger a little before they sleep.
  static void submit(InflateJob * const * jobs, size_t n)
  {
    InflateTeam * t = slot().self;
    if (!t || t->workers_.empty() || n == 0)
      return;
    bool wake;
    {
      std::lock_guard<std::mutex> lock(t->m_);
      t->queue_.insert(t->queue_.end(), jobs, jobs + n);
      t->pending_.store(t->queue_.size(), std::memory_order_release);
      wake = t->sleepers_ > 0 && t->lingering_.load(std::memory_order_acquire) == 0;
    }
    if (wake)
      t->cv_.notify_one();
  }
  // forgets the jobs of a reader that goes away (none of them is running any more: the reader has waited for those)
  static void forget(InflateJob const * first, InflateJob const * last)
  {
    InflateTeam * t = slot().self;
    if (!t)
      return;
    std::lock_guard<std::mutex> lock(t->m_);
    forget_jobs(t->queue_, first, last);
    t->pending_.store(t->queue_.size(), std::memory_order_release);
  }

private:
  explicit InflateTeam(unsigned n)
  {
    linger_us_ = sw::bgzf_linger_us(linger_us_);
    for (unsigned i = 0; i < n; ++i)
      workers_.emplace_back([this] { run(); });
  }
  ~InflateTeam()
  {
    {
      std::lock_guard<std::mutex> lock(m_);
      stop_ = true;
      stop_flag_.store(true);
    }
    cv_.notify_all();
    for (auto & w : workers_)
      w.join();
  }
  void run()
  {
    for (;;)
    {
      InflateJob * j = nullptr;
      bool wake_next = false;
      {
        std::unique_lock<std::mutex> lock(m_);
        if (queue_.empty() && !stop_)
        {
          // nothing to do: look at the queue for a little while without sleeping (two workers at most do; a reader hands
          // over its next members within that time when it is reading at all), then sleep
          if (linger_us_ > 0 && lingering_.load(std::memory_order_relaxed) < 2)
          {
            lingering_.fetch_add(1, std::memory_order_acq_rel);
            lock.unlock();
            auto const until = std::chrono::steady_clock::now() + std::chrono::microseconds(linger_us_);
            while (pending_.load(std::memory_order_acquire) == 0 && !stop_flag_.load(std::memory_order_relaxed) &&
                   std::chrono::steady_clock::now() < until)
              std::this_thread::yield();
            lock.lock();
            lingering_.fetch_sub(1, std::memory_order_acq_rel);
          }
          if (queue_.empty() && !stop_)
          {
            ++sleepers_;
            cv_.wait(lock, [this] { return stop_ || !queue_.empty(); });
            --sleepers_;
          }
        }
        if (stop_)
          return;
        j = queue_.front();
        queue_.pop_front();
        pending_.store(queue_.size(), std::memory_order_release);
        wake_next = !queue_.empty() && sleepers_ > 0; // more than this worker can take at once: the next worker is woken from here
        int expect = 0;
        if (!j->state.compare_exchange_strong(expect, 1)) // (its reader got there first)
          j = nullptr;
      }
      if (wake_next)
        cv_.notify_one();
      if (j)
        inflate_member(*j);
    }
  }
  friend struct TeamSlot<InflateTeam>;
  static TeamSlot<InflateTeam> & slot()
  {
    static TeamSlot<InflateTeam> s;
    return s;
  }
  int linger_us_ = 300;                  // GTX_BGZF_LINGER_US
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<InflateJob *> queue_;
  std::vector<std::thread> workers_;
  bool stop_ = false;
  int sleepers_ = 0;                     // workers inside cv_.wait (under m_)
  std::atomic<int> lingering_{0};        // workers polling pending_ before they sleep
  std::atomic<size_t> pending_{0};       // queue_.size() for those
  std::atomic<bool> stop_flag_{false};
};

// The device's team: ONE thread per process that takes what the readers that asked for the device (Bgzf::use_device) have
// queued -- everything that is there, a launch wants thousands of members --, gathers the compressed members into a pinned block,
// has them inflated in one launch (gtx_inflate_dev.hip) and hands the bytes out.  A member the device does not give "ok" goes
// through inflate_member on this thread: the host's verdict is the one that counts, so a damaged file fails as it does without
// the device.  As with the host's team, a reader that needs a member nobody has started on inflates it itself.
class DeviceInflateTeam
{
public:
  static constexpr size_t MAX_BATCH = 16384; // members per launch (1 GB of output at most)
  // 0, or the status and message (gtx_last_error) of what failed; a team on another device is alive: GTX_ERR_UNSUPPORTED
  static int acquire(int device)
  {
    std::lock_guard<std::mutex> lock(slot().gate);
    if (slot().users > 0)
    {
      if (slot().self->device_ != device)
      {
        gtx::g_last_error = "gtx_reads_set_inflate_device: readers of this process inflate on device " + std::to_string(slot().self->device_) + " already";
        return GTX_ERR_UNSUPPORTED;
      }
      ++slot().users;
      return GTX_OK;
    }
    if (!gtx::inflate_device_ops)
    {
      gtx::g_last_error = "gtx_reads_set_inflate_device: this build holds no device inflater";
      return GTX_ERR_NO_DEVICE;
    }
    gtx_inflate * h = nullptr;
    int const rc = gtx::inflate_device_ops->create(device, &h);
    if (rc != GTX_OK)
      return rc;
    slot().self = new DeviceInflateTeam(device, h);
    slot().users = 1;
    return GTX_OK;
  }
  static void release() { slot().release(); }
  static void submit(InflateJob * const * jobs, size_t n)
  {
    DeviceInflateTeam * t = slot().self;
    if (!t || n == 0)
      return;
    {
      std::lock_guard<std::mutex> lock(t->m_);
      t->queue_.insert(t->queue_.end(), jobs, jobs + n);
    }
    t->cv_.notify_one();
  }
  static void forget(InflateJob const * first, InflateJob const * last)
  {
    DeviceInflateTeam * t = slot().self;
    if (!t)
      return;
    std::lock_guard<std::mutex> lock(t->m_);
    forget_jobs(t->queue_, first, last);
  }

private:
  DeviceInflateTeam(int device, gtx_inflate * h) : device_(device), h_(h), worker_([this] { run(); }) {}
  ~DeviceInflateTeam()
  {
    {
      std::lock_guard<std::mutex> lock(m_);
      stop_ = true;
    }
    cv_.notify_all();
    worker_.join();
    gtx::inflate_device_ops->destroy(h_);
  }
  void run()
  {
    gtx::InflateDeviceOps const & ops = *gtx::inflate_device_ops;
    using Pinned = std::unique_ptr<uint8_t, void (*)(void *)>;
    Pinned pin_in(nullptr, ops.pinned_free), pin_out(nullptr, ops.pinned_free);
    auto grow = [&](Pinned & p, size_t & cap, uint64_t want) {
      if (want <= cap)
        return true;
      p.reset();
      p.reset(static_cast<uint8_t *>(ops.pinned_alloc(h_, want + want / 4)));
      cap = p ? want + want / 4 : 0;
      return cap != 0;
    };
    size_t in_cap = 0, out_cap = 0;
    std::vector<InflateJob *> batch;
    std::vector<gtx_inflate_member> members;
    std::vector<uint32_t> status;
    for (;;)
    {
      batch.clear();
      {
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [this] { return stop_ || !queue_.empty(); });
        if (stop_)
          return;
        while (!queue_.empty() && batch.size() < MAX_BATCH)
        {
          InflateJob * j = queue_.front();
          queue_.pop_front();
          int expect = 0;
          if (j->state.compare_exchange_strong(expect, 1)) // (else its reader got there first)
            batch.push_back(j);
        }
      }
      if (batch.empty())
        continue;
      members.resize(batch.size());
      status.assign(batch.size(), GTX_INFLATE_BAD_MEMBER);
      uint64_t in_size = 0, out_size = 0;
      for (size_t i = 0; i < batch.size(); ++i)
      {
        members[i] = gtx_inflate_member{in_size, out_size, static_cast<uint32_t>(batch[i]->clen), static_cast<uint32_t>(batch[i]->data.size()), 0, 0};
        std::memcpy(&members[i].crc32, batch[i]->comp.data() + batch[i]->clen, 4);
        in_size += static_cast<uint64_t>(batch[i]->clen);
        out_size += batch[i]->data.size();
      }
      bool ok = grow(pin_in, in_cap, in_size) && grow(pin_out, out_cap, out_size);
      if (ok)
      {
        for (size_t i = 0; i < batch.size(); ++i)
          std::memcpy(pin_in.get() + members[i].in_off, batch[i]->comp.data(), members[i].in_len);
        ok = ops.batch(h_, pin_in.get(), in_size, members.data(), static_cast<uint32_t>(batch.size()), pin_out.get(), out_size, status.data(),
                       env_check_crc()) == GTX_OK;
      }
      for (size_t i = 0; i < batch.size(); ++i)
      {
        InflateJob & j = *batch[i];
        if (!ok || status[i] != GTX_INFLATE_OK)
        {
          g_members_fallback.fetch_add(1, std::memory_order_relaxed);
          inflate_member(j); // (the host's decoders, and their verdict)
          continue;
        }
        std::memcpy(j.data.data(), pin_out.get() + members[i].out_off, members[i].out_len);
        g_members_device.fetch_add(1, std::memory_order_relaxed);
        j.ok = true;
        std::lock_guard<std::mutex> lock(j.m);
        j.state.store(2);
        j.cv.notify_all();
      }
    }
  }
  friend struct TeamSlot<DeviceInflateTeam>;
  static TeamSlot<DeviceInflateTeam> & slot()
  {
    static TeamSlot<DeviceInflateTeam> s;
    return s;
  }
  int device_;
  gtx_inflate * h_;
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<InflateJob *> queue_;
  bool stop_ = false;
  std::thread worker_; // (last: it runs as soon as it is made)
};
} // namespace

Bgzf::Bgzf() = default;
Bgzf::~Bgzf() { close(); }

bool Bgzf::open(std::string const & path)
{
  fp_ = std::fopen(path.c_str(), "rb");
  if (fp_)
  {
    InflateTeam::acquire();
    ring_n_ = RING;
    ring_.reset(new InflateJob[ring_n_]);
  }
  return fp_ != nullptr;
}

void Bgzf::close()
{
  if (fp_)
  {
    drain();
    ring_.reset();
    InflateTeam::release();
    if (on_device_)
      DeviceInflateTeam::release();
    on_device_ = false;
    std::fclose(fp_);
  }
  fp_ = nullptr;
}

long Bgzf::read(void * dst, size_t n)
{
  size_t done = 0;
  while (done < n)
  {
    if (at_ == data_.size() && !next_block())
      return bad_ ? -1 : static_cast<long>(done);
    size_t const take = std::min(n - done, data_.size() - at_);
    std::memcpy(static_cast<uint8_t *>(dst) + done, data_.data() + at_, take);
    at_ += take;
    done += take;
  }
  return static_cast<long>(done);
}

void Bgzf::read_rest(std::string & out)
{
  while (at_ < data_.size() || next_block())
  {
    out.append(reinterpret_cast<char const *>(data_.data()) + at_, data_.size() - at_);
    at_ = data_.size();
  }
}

bool Bgzf::seek(uint64_t voffset)
{
  drain();
  if (std::fseek(fp_, static_cast<long>(voffset >> 16), SEEK_SET) != 0)
    return false;
  data_.clear();
  at_ = 0;
  if ((voffset & 0xFFFFu) == 0)
    return true;
  if (!next_block() || (voffset & 0xFFFFu) > data_.size())
    return false;
  at_ = voffset & 0xFFFFu;
  return true;
}

int Bgzf::use_device(int device)
{
  if (!fp_ || on_device_)
    return fp_ ? GTX_OK : GTX_ERR_ARG;
  int const rc = DeviceInflateTeam::acquire(device);
  if (rc != GTX_OK)
    return rc;
  unsigned const deep = sw::bgzf_device_ring(RING);
  std::unique_ptr<InflateJob[]> ring(new InflateJob[deep]);
  // the members in flight are finished where they are and move to the front of the deeper ring
  uint64_t n = 0;
  for (uint64_t k = head_; k < tail_ && n < deep; ++k, ++n)
  {
    InflateJob & j = ring_[k % ring_n_];
    finish(j);
    ring[n].comp.swap(j.comp);
    ring[n].data.swap(j.data);
    ring[n].clen = j.clen;
    ring[n].ok = j.ok;
  }
  InflateTeam::forget(ring_.get(), ring_.get() + ring_n_);
  ring_.swap(ring);
  ring_n_ = deep;
  head_ = 0;
  tail_ = n;
  on_device_ = true;
  return GTX_OK;
}

// the next member with data of the file into job j (compressed bytes only)
MemberRead Bgzf::read_member(InflateJob & j)
{
  for (;;)
  {
    BgzfMember m;
    MemberRead const got = read_bgzf_member(fp_, m, j.comp);
    if (got != MEMBER_OK)
      return got;
    if (m.isize == 0)
      continue; // (the end-of-file marker, or an empty member)
    j.clen = m.clen;
    j.data.resize(m.isize);
    return MEMBER_OK;
  }
}

// reads members ahead until the ring is full or the file ends / breaks (which is reported when the caller gets there)
void Bgzf::fill()
{
  if (tail_ - head_ > ring_n_ / 2) // (refilled by halves: the members go to the team in one hand-over)
    return;
  fresh_.resize(ring_n_);
  InflateJob ** const fresh = fresh_.data();
  size_t n = 0;
  while (ahead_ == MEMBER_OK && tail_ - head_ < ring_n_)
  {
    InflateJob & j = ring_[tail_ % ring_n_];
    ahead_ = read_member(j);
    if (ahead_ != MEMBER_OK)
      break;
    j.state.store(0);
    ++tail_;
    fresh[n++] = &j;
  }
  if (on_device_)
    DeviceInflateTeam::submit(fresh, n);
  else
    InflateTeam::submit(fresh, n);
}

bool Bgzf::next_block()
{
  fill();
  if (head_ == tail_)
  {
    bad_ = bad_ || ahead_ == MEMBER_BROKEN;
    return false; // the end of the file, or of what can be read of it
  }
  InflateJob & j = ring_[head_ % ring_n_];
  finish(j);
  ++head_;
  if (!j.ok)
  {
    bad_ = true;
    return false;
  }
  data_.swap(j.data);
  at_ = 0;
  return true;
}

// the member is inflated when this returns: by this thread when nobody has started on it
void Bgzf::finish(InflateJob & j) const
{
  int expect = 0;
  if (j.state.compare_exchange_strong(expect, 1))
  {
    if (on_device_)
      g_members_reader.fetch_add(1, std::memory_order_relaxed);
    inflate_member(j);
  }
  else
  {
    std::unique_lock<std::mutex> lock(j.m);
    j.cv.wait(lock, [&] { return j.state.load() == 2; });
  }
}

// nothing of this reader is in flight or queued afterwards
void Bgzf::drain()
{
  if (!ring_)
    return;
  for (; head_ < tail_; ++head_)
  {
    InflateJob & j = ring_[head_ % ring_n_];
    int expect = 0;
    if (j.state.compare_exchange_strong(expect, 2))
      continue; // (never started)
    std::unique_lock<std::mutex> lock(j.m);
    j.cv.wait(lock, [&] { return j.state.load() == 2; });
  }
  if (on_device_)
    DeviceInflateTeam::forget(ring_.get(), ring_.get() + ring_n_);
  else
    InflateTeam::forget(ring_.get(), ring_.get() + ring_n_);
  head_ = tail_ = 0;
  ahead_ = MEMBER_OK;
}
} // namespace gtx

// ---- BGZF: the members htslib's bgzf_write makes (SAM spec 4.1): gzip members with the BC extra field, at most 0xff00 bytes of
// input each, and the 28-byte empty member at the end of a file (what the reference's bgzf_stream writes its VCF through,
// include/graphtyper/utilities/bgzf_stream.hpp).
extern "C" int gtx_bgzf_compress(const void * in, uint64_t in_len, int level, int with_eof, void * out, uint64_t cap, uint64_t * out_len)
{
  if (!out_len || (in_len && !in) || (cap && !out))
  {
    gtx::g_last_error = "gtx_bgzf_compress: bad argument";
    return GTX_ERR_ARG;
  }
  std::string res;
  uint8_t const * p = static_cast<uint8_t const *>(in);
  auto member = [&](uint8_t const * data, uint32_t n, std::string & res) -> bool
  {
    std::vector<uint8_t> buf(compressBound(n) + 64);
    z_stream zs{};
    if (deflateInit2(&zs, level < 0 ? Z_DEFAULT_COMPRESSION : std::min(level, 9), Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK)
      return false;
    zs.next_in = const_cast<Bytef *>(data);
    zs.avail_in = n;
    zs.next_out = buf.data();
    zs.avail_out = static_cast<uInt>(buf.size());
    int const rc = deflate(&zs, Z_FINISH);
    uint32_t const clen = static_cast<uint32_t>(zs.total_out);
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || clen + 26u > 0x10000u)
      return false;
    uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 0, 0};
    uint16_t const bsize = static_cast<uint16_t>(clen + 25u);
    head[16] = static_cast<uint8_t>(bsize & 255u);
    head[17] = static_cast<uint8_t>(bsize >> 8);
    res.append(reinterpret_cast<char const *>(head), 18);
    res.append(reinterpret_cast<char const *>(buf.data()), clen);
    uint32_t const tail[2] = {static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), data, n)), n};
    res.append(reinterpret_cast<char const *>(tail), 8);
    return true;
  };
  // members are independent: beyond a megabyte of input they are made on a few threads, each a run of consecutive members,
  // and put together in order (the bytes are those of one thread)
  uint64_t const n_members = (in_len + 0xff00u - 1) / 0xff00u;
  unsigned const n_threads = n_members < 16 ? 1u : static_cast<unsigned>(std::min<uint64_t>(std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency() / 2)), n_members / 8));
  std::vector<std::string> parts(std::max(1u, n_threads));
  std::vector<char> failed(parts.size(), 0);
  auto run = [&](unsigned k)
  {
    uint64_t const m0 = n_members * k / parts.size(), m1 = n_members * (k + 1) / parts.size();
    for (uint64_t m = m0; m < m1 && !failed[k]; ++m)
    {
      uint64_t const at = m * 0xff00u;
      if (!member(p + at, static_cast<uint32_t>(std::min<uint64_t>(0xff00u, in_len - at)), parts[k]))
        failed[k] = 1;
    }
  };
  if (parts.size() == 1)
    run(0);
  else
  {
    std::vector<std::thread> team;
    for (unsigned k = 1; k < parts.size(); ++k)
      team.emplace_back(run, k);
    run(0);
    for (auto & t : team)
      t.join();
  }
  for (size_t k = 0; k < parts.size(); ++k)
  {
    if (failed[k])
    {
      gtx::g_last_error = "gtx_bgzf_compress: deflate failed";
      return GTX_ERR_IO;
    }
    res += parts[k];
  }
  if (with_eof)
  {
    // the end-of-file marker is a fixed member (SAM spec 4.1.2), whatever the level: deflating nothing at level 0 gives a stored
    // block and a member of 31 bytes, which htslib's bgzf_check_EOF does not take for the marker
    static unsigned char const EOF_MEMBER[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    res.append(reinterpret_cast<char const *>(EOF_MEMBER), sizeof EOF_MEMBER);
  }
  *out_len = res.size();
  if (res.size() > cap)
    return out ? GTX_ERR_CAPACITY : GTX_OK;
  std::memcpy(out, res.data(), res.size());
  return GTX_OK;
}

extern "C" int gtx_inflate_raw(const void * in, uint64_t in_len, void * out, uint64_t out_len)
{
  if ((in_len && !in) || (out_len && !out))
    return GTX_ERR_ARG;
  std::vector<uint8_t> padded(in_len + 8, 0); // (the decoder loads 8 bytes at a time: a BGZF member has its CRC32 and ISIZE there)
  if (in_len)
    std::memcpy(padded.data(), in, in_len);
  uint8_t nothing = 0;
  if (gtx::inflate_raw(padded.data(), in_len, out_len ? static_cast<uint8_t *>(out) : &nothing, out_len))
    return GTX_OK;
  gtx::g_last_error = "gtx_inflate_raw: not a DEFLATE stream of the given size";
  return GTX_ERR_IO;
}
