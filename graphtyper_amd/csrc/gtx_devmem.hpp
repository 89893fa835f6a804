// gtx_devmem.hpp -- device memory of the library through a process-wide cache, and the owners of what comes from it: scoped
// owners of device / pinned blocks, events and streams, the pool of temporaries, the one HIP error helper.
//
// The reference genotypes a chromosome region by region (50 kb each, src/main.cpp:684): a context -- graph tables, index,
// scratch, the HBM-table workspaces -- lives for milliseconds, and hipMalloc / hipFree (each hipFree also waits for the
// device) of its ~50 allocations were most of what creating one cost.  Freed blocks are kept per device in size classes
// and handed out again; nothing is returned to the driver before the cache holds more than its limit (GTX_DEVICE_CACHE_MB,
// default 32768) or gtx_device_cache_release() is called.  A block goes back to the cache only when no kernel can still use
// it: callers free after the work on it is known to be done (context destruction and the index build synchronise first).
#pragma once
#include "../../include/gtx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <string>
#include <vector>

namespace gtx
{
extern thread_local std::string g_last_error;
hipError_t dev_malloc(void ** p, size_t bytes); // on the current device
hipError_t dev_free(void * p);                  // back to the cache (NULL is fine)
// The stream of the context that is being made on this thread (gtx_ctx_create: uploads, the index build's kernels, the zeroing of
// what it allocates), nullptr outside of one: the work of making a context is ordered on a stream of its own, so that host
// threads that make contexts side by side (gtx_regions_run's builders) neither queue behind each other on the null stream nor
// wait for the regions that are running on other streams.
extern thread_local hipStream_t tls_build_stream;
// Zeroes device memory and returns when it IS zero.  (hipMemset on device memory returns before the fill has run, and the fill
// runs on the null stream: a kernel on a non-blocking stream -- every stream PyTorch makes -- is not ordered behind it, so a
// counter block "zeroed" by a plain hipMemset can be cleared in the middle of the first call that counts in it.)
inline hipError_t dev_zero(void * p, size_t bytes)
{
  hipError_t const e = hipMemsetAsync(p, 0, bytes, tls_build_stream);
  return e != hipSuccess ? e : hipStreamSynchronize(tls_build_stream);
}
// A non-blocking stream of the current device from a process-wide pool becomes this thread's tls_build_stream for the scope's
// life (GTX_BUILD_STREAM=0: the null stream, as before round 5 -- A/B).  The scope's end waits for the stream.
struct BuildStreamScope
{
  hipStream_t stream = nullptr, before = nullptr;
  int device = -1;
  BuildStreamScope();
  ~BuildStreamScope();
  BuildStreamScope(BuildStreamScope const &) = delete;
  BuildStreamScope & operator=(BuildStreamScope const &) = delete;
};
void dev_cache_release();                       // hipFree everything the cache holds
// A 64-byte slot of pinned host memory (a word the device writes and a later call reads, per context): cut from pages that are
// pinned once and kept for the life of the process -- hipHostMalloc / hipHostFree per context were most of what making and
// destroying a small region's context cost its host thread, and the free waits for the device.  nullptr when nothing can be pinned.
void * pinned_slot_get();
void pinned_slot_put(void * p);

// ---- owners: each gives back what it holds when its scope ends ------------------------------------------------------
// a std::unique_ptr deleter that hands the pointer to F (what F returns is not looked at: there is nobody left to tell)
template <auto F>
struct Free
{
  template <class T>
  void operator()(T * p) const { (void)F(p); }
};
struct StreamEnd
{
  void operator()(hipStream_t s) const { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
};

template <class T = void>
using DevPtr = std::unique_ptr<T, Free<dev_free>>; // a device block through the library's cache
template <class T = void>
using PinnedPtr = std::unique_ptr<T, Free<hipHostFree>>; // pinned host memory
template <class T = void>
using PinnedSlot = std::unique_ptr<T, Free<pinned_slot_put>>; // a slot of pinned_slot_get
template <class T = void>
using DriverPtr = std::unique_ptr<T, Free<hipFree>>; // a device block straight from the driver
using Event = std::unique_ptr<ihipEvent_t, Free<hipEventDestroy>>;
using Stream = std::unique_ptr<ihipStream_t, StreamEnd>; // a stream of one's own: waited for, then destroyed
using StreamWait = std::unique_ptr<ihipStream_t, Free<hipStreamSynchronize>>; // a stream it does not own: waited for at the scope's end

// the allocator that goes with each kind of block
inline hipError_t malloc_for(Free<dev_free>, void ** p, size_t bytes) { return dev_malloc(p, bytes); }
inline hipError_t malloc_for(Free<hipHostFree>, void ** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t malloc_for(Free<hipFree>, void ** p, size_t bytes) { return hipMalloc(p, bytes); }
// allocation into an owner: what it held is freed first, and it holds what the allocator returned even when that failed
template <class T, class D>
hipError_t alloc_e(std::unique_ptr<T, D> & p, size_t bytes)
{
  p.reset();
  void * v = nullptr;
  hipError_t const e = malloc_for(D{}, &v, bytes);
  p.reset(static_cast<T *>(v));
  return e;
}
template <class T, class D>
bool alloc(std::unique_ptr<T, D> & p, size_t bytes)
{
  return alloc_e(p, bytes) == hipSuccess;
}

// the library's one way to turn a HIP error into gtx_last_error's text: "<prefix><what>: <the runtime's words>"
inline bool hip_ok(hipError_t e, char const * what, char const * prefix = "")
{
  if (e == hipSuccess)
    return true;
  g_last_error = std::string(prefix) + what + ": " + hipGetErrorString(e);
  return false;
}

// the front of a device entry point: GTX_ERR_NO_DEVICE for an object (`who` and `tail` name it: "context", or "<entry point>" and
// ": the object") that was made without a device, else that device becomes the thread's current one
inline int device_ready(int device, char const * who, char const * tail = "")
{
  if (device < 0)
  {
    g_last_error = std::string(who) + tail + " was created without a device (libgtx has no CPU path)";
    return GTX_ERR_NO_DEVICE;
  }
  return hip_ok(hipSetDevice(device), "hipSetDevice") ? GTX_OK : GTX_ERR_HIP;
}

// Temporary device blocks of one piece of work on one stream: they go back to the cache when the stream is through with
// them.  After the first failure `fine` stays false and get() returns nullptr, so a caller asks for all it needs and
// looks at `fine` once.
struct TempPool
{
  hipStream_t const stream;
  char const * const prefix; // of the messages (hip_ok)
  std::vector<DevPtr<>> temps;
  bool fine = true;
  TempPool(hipStream_t stream_, char const * prefix_) : stream(stream_), prefix(prefix_) {}
  TempPool(TempPool const &) = delete;
  TempPool & operator=(TempPool const &) = delete;
  bool ok(hipError_t e, char const * what) const { return hip_ok(e, what, prefix); }
  // n (at least one) elements; fill >= 0: every byte set to it on the stream (the first user is a later launch there)
  template <class T>
  T * get(size_t n, char const * what, int fill = -1)
  {
    if (!fine)
      return nullptr;
    size_t const bytes = (n ? n : 1) * sizeof(T);
    DevPtr<> p;
    fine = ok(alloc_e(p, bytes), what);
    if (fine && fill >= 0)
      fine = ok(hipMemsetAsync(p.get(), fill, bytes, stream), what);
    T * const raw = static_cast<T *>(p.get());
    if (p)
      temps.push_back(std::move(p));
    return raw;
  }
  // the block outlives the pool: ownership moves to `owner`
  template <class T>
  T * keep(T * p, std::vector<DevPtr<>> & owner)
  {
    auto it = std::find_if(temps.begin(), temps.end(), [p](DevPtr<> const & t) { return t.get() == static_cast<void const *>(p); });
    if (it != temps.end())
    {
      owner.push_back(std::move(*it));
      temps.erase(it);
    }
    return p;
  }
  ~TempPool()
  {
    if (!temps.empty())
      (void)hipStreamSynchronize(stream); // (on an error path kernels may still be writing to them; freed blocks are handed out again)
    temps.clear();
  }
};
} // namespace gtx
