// gtx_host_loops.hpp -- what the library's two host loops (gtx_pipeline.cpp, gtx_regions.cpp) share, host code only: owners of
// their device and pinned blocks, events, streams and handles, each of which gives back what it holds when its scope ends.
#pragma once
#include "../../include/gtx.h"
#include "gtx_devmem.hpp"

#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <string>

namespace gtx
{
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
using DriverPtr = std::unique_ptr<T, Free<hipFree>>; // a device block straight from the driver
using Event = std::unique_ptr<ihipEvent_t, Free<hipEventDestroy>>;
using Stream = std::unique_ptr<ihipStream_t, StreamEnd>; // a stream of one's own: waited for, then destroyed
using StreamWait = std::unique_ptr<ihipStream_t, Free<hipStreamSynchronize>>; // a stream it does not own: waited for at the scope's end
using Ctx = std::unique_ptr<gtx_ctx, Free<gtx_ctx_destroy>>;
using Graph = std::unique_ptr<gtx_graph, Free<gtx_graph_destroy>>;
using ReadStream = std::unique_ptr<gtx_stream, Free<gtx_stream_destroy>>;
using Reads = std::unique_ptr<gtx_reads, Free<gtx_reads_close>>;

// the allocator that goes with each kind of block
inline hipError_t malloc_for(Free<dev_free>, void ** p, size_t bytes) { return dev_malloc(p, bytes); }
inline hipError_t malloc_for(Free<hipHostFree>, void ** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t malloc_for(Free<hipFree>, void ** p, size_t bytes) { return hipMalloc(p, bytes); }
// allocation into an owner: what it held is freed first, and it holds what the allocator returned even when that failed
template <class T, class D>
bool alloc(std::unique_ptr<T, D> & p, size_t bytes)
{
  p.reset();
  void * v = nullptr;
  hipError_t const e = malloc_for(D{}, &v, bytes);
  p.reset(static_cast<T *>(v));
  return e == hipSuccess;
}

inline double seconds_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the middle of the message of a result that a capacity limit of the library left incomplete
inline std::string incomplete_counts(uint64_t records_failed, uint64_t items_refused, uint64_t connections_dropped)
{
  return std::to_string(records_failed) + " records with a table-overflow status, " + std::to_string(items_refused) + " score items refused, " +
         std::to_string(connections_dropped) + " connections beyond the log";
}
} // namespace gtx
