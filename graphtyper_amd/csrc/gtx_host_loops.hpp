// gtx_host_loops.hpp -- what the library's two host loops (gtx_pipeline.cpp, gtx_regions.cpp) share, host code only: owners of
// the library's handles (the owners of blocks, events and streams are gtx_devmem.hpp's) and two small helpers.
#pragma once
#include "../../include/gtx.h"
#include "gtx_devmem.hpp"

#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <string>

namespace gtx
{
using Ctx = std::unique_ptr<gtx_ctx, Free<gtx_ctx_destroy>>;
using Graph = std::unique_ptr<gtx_graph, Free<gtx_graph_destroy>>;
using ReadStream = std::unique_ptr<gtx_stream, Free<gtx_stream_destroy>>;
using Reads = std::unique_ptr<gtx_reads, Free<gtx_reads_close>>;

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
