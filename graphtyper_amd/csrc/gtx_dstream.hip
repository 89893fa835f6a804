// gtx_dstream.hip -- the launches of the record stream's decisions on the device (gtx_dstream_dev.hpp: the definition and the kernel
// text) and gtx_dstream_* of include/gtx.h.  A push is a fixed chain on the caller's stream: the kernels of the header with rocPRIM's
// scans and stable sorts (gtx_devprim.hpp) between them, one download at its end.  All device memory is made at creation: one block
// cut into the arrays, the two slots of the state among them, and one block of temporary storage for the primitives, sized by
// asking rocPRIM what each call wants over a ladder of sizes up to max_batch + parked_cap (PrimStorage hands it out in a TempPool's
// place; a call that wants more fails and nothing is allocated).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <memory>
#include <string>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_ctx.hpp"
#include "gtx_devmem.hpp"
#include "gtx_devprim.hpp"
#include "gtx_dstream_dev.hpp"
#include "wave_hip.hpp"

static_assert(sizeof(gtx_stream_record) == 56 && sizeof(gtx_read_meta) == 20 && sizeof(gtx_rec_meta) == 16 && sizeof(gtx_score_item) == 40, "layouts of the binding");

namespace
{
using namespace gtx;

constexpr uint32_t WAVES_PER_BLOCK = 4;
constexpr uint32_t MAX_BLOCKS = 1u << 10; // (the wavefronts stride over the tiles behind that; finish sums a count per wavefront of classify)
constexpr uint32_t MAX_ELEMENTS = 1u << 28; // max_batch + parked_cap: 4 * record + check fits the `fail` word

#define GTX_DSTREAM_WAVE blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6), gridDim.x * WAVES_PER_BLOCK

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_classify_kernel(DstreamPush a) { dstream_classify_wave<WaveHip>(a, GTX_DSTREAM_WAVE); }
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_compare_kernel(DstreamPush a) { dstream_compare_wave<WaveHip>(a, GTX_DSTREAM_WAVE); }
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_emit_tasks_kernel(DstreamPush a) { dstream_emit_tasks_wave<WaveHip>(a, GTX_DSTREAM_WAVE); }
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_gather_rg_kernel(DstreamPush a, uint32_t const * __restrict__ by_name, uint32_t * __restrict__ keys)
{
  dstream_gather_rg_wave<WaveHip>(a, by_name, keys, GTX_DSTREAM_WAVE);
}
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_walk_kernel(DstreamPush a) { dstream_walk_wave<WaveHip>(a, GTX_DSTREAM_WAVE); }
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gtx_dstream_emit_items_kernel(DstreamPush a) { dstream_emit_items_wave<WaveHip>(a, GTX_DSTREAM_WAVE); }
__global__ __launch_bounds__(64) void gtx_dstream_finish_kernel(DstreamPush a) { dstream_finish_wave<WaveHip>(a); }

// blocks for `count` things, `per_wave` of them a tile
uint32_t blocks_for(uint64_t count, uint32_t per_wave)
{
  uint64_t const tiles = (count + per_wave - 1) / per_wave;
  return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, MAX_BLOCKS)));
}

bool launched(char const * which)
{
  if (hipGetLastError() == hipSuccess)
    return true;
  g_last_error = std::string("gtx_dstream_push: ") + which + " launch failed";
  return false;
}

// The primitives' temporary storage in a TempPool's place.  block == nullptr: nothing runs, `most` is the largest request.
struct PrimStorage
{
  hipStream_t const stream;
  char const * const prefix;
  void * const block;
  size_t const cap;
  size_t most = 0;
  bool fine = true;
  bool ok(hipError_t e, char const * what) const { return hip_ok(e, what, prefix); }
  template <class T>
  T * get(size_t n, char const * what, int = -1)
  {
    most = std::max(most, n * sizeof(T));
    if (!block)
      return nullptr; // (the second call of with_storage asks for the size again)
    if (n * sizeof(T) > cap)
    {
      g_last_error = std::string(prefix) + what + ": " + std::to_string(n * sizeof(T)) + " bytes of temporary storage, the stream was made with " + std::to_string(cap);
      fine = false;
      return nullptr;
    }
    return static_cast<T *>(block);
  }
};

// the primitives of a push, in its order; each is the step's whole call
struct Prims
{
  uint64_t *name, *name_sorted;
  uint32_t *elem, *by_name, *rg_keys, *rg_sorted, *by_key;
  DstreamPush const & a;
  uint32_t rg_bits;
  template <class Pool>
  bool previous_kept(Pool & p, uint32_t n) const
  {
    return inclusive_scan(p, a.kept_in, a.prev_scan, n, rocprim::maximum<uint32_t>(), "previous kept record", "scan storage");
  }
  template <class Pool>
  bool heads(Pool & p, uint32_t n) const
  {
    return exclusive_sum(p, a.head, a.task, n, "task numbers", "scan storage") &&
           inclusive_scan(p, a.head_in, a.head_of, n, rocprim::maximum<uint32_t>(), "heads", "scan storage");
  }
  template <class Pool>
  bool by_names(Pool & p, uint32_t total) const
  {
    return sort_pairs(p, static_cast<uint64_t const *>(name), name_sorted, static_cast<uint32_t const *>(elem), by_name, total, 64u, "sort by name", "sort storage");
  }
  template <class Pool>
  bool by_groups(Pool & p, uint32_t total) const
  {
    return sort_pairs(p, static_cast<uint32_t const *>(rg_keys), rg_sorted, static_cast<uint32_t const *>(by_name), by_key, total, rg_bits, "sort by read group",
                      "sort storage");
  }
  template <class Pool>
  bool slots(Pool & p, uint32_t n, uint32_t total) const
  {
    return exclusive_sum(p, a.emit, a.emit_at, n, "item numbers", "scan storage") && exclusive_sum(p, a.wait, a.wait_at, total, "parked slots", "scan storage");
  }
};

uint32_t bits_for(uint32_t n_values) // to tell 0 .. n_values - 1 apart
{
  uint32_t bits = 1;
  while (bits < 32 && (1ull << bits) < n_values)
    ++bits;
  return bits;
}
} // namespace

struct gtx_dstream
{
  gtx_params params{};
  uint32_t n_read_groups = 0, max_batch = 0, parked_cap = 0, row_cap = 0;
  int device = -1;
  DevPtr<uint8_t> arena, prim;
  size_t prim_cap = 0;
  PinnedSlot<> slot; // the download
  // the arena's arrays
  DstreamCarry * carry[2] = {};
  uint8_t * carry_row[2] = {};
  DstreamParked * parked[2] = {};
  DstreamPush work{}; // the workspace pointers (the rest is set per push)
  uint64_t * name_sorted = nullptr;
  uint32_t *by_name = nullptr, *rg_keys = nullptr, *rg_sorted = nullptr, *by_key = nullptr;
  DstreamOut * d_out = nullptr;
  // the state the host holds
  uint32_t cur = 0, n_parked = 0;
  uint64_t n_records = 0, n_duplicated = 0;
};

extern "C" int gtx_dstream_create(const gtx_params * params, uint32_t n_read_groups, int device, uint32_t max_batch, uint32_t parked_cap, gtx_dstream ** out)
{
  char const * const prefix = "gtx_dstream_create: ";
  if (!params || !out || n_read_groups == 0 || n_read_groups > 65536u || max_batch == 0 || static_cast<uint64_t>(max_batch) + parked_cap >= MAX_ELEMENTS)
  {
    g_last_error = std::string(prefix) + "bad argument (at least one read group and one record a push; max_batch + parked_cap below 2^28)";
    return GTX_ERR_ARG;
  }
  *out = nullptr;
  if (params->is_sv_graph)
  {
    g_last_error = std::string(prefix) + "not for SV graphs: the SV record filter's coverage bins depend on the order of the records, and the leftover items of "
                                         "gtx_stream_finish follow the order of the host's hash map (use gtx_stream_push)";
    return GTX_ERR_UNSUPPORTED;
  }
  if (!max_read_len_ok(*params))
  {
    g_last_error = std::string(prefix) + "max_read_len must be 0 or 257 .. 1000 (GTX_MAX_READ_LONG), and 0 with no_second_pass";
    return GTX_ERR_ARG;
  }
  int n_dev = 0;
  if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev)
  {
    g_last_error = std::string(prefix) + "no such HIP device (libgtx has no CPU path: gtx_stream_push is the host's)";
    return GTX_ERR_NO_DEVICE;
  }
  try
  {
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", prefix))
      return GTX_ERR_HIP;
    auto s = std::make_unique<gtx_dstream>();
    s->params = *params;
    s->n_read_groups = n_read_groups;
    s->max_batch = max_batch;
    s->parked_cap = parked_cap;
    s->device = device;
    s->row_cap = (dstream_dev::nib_bytes(max_read_len_of(*params)) + 15u) / 16u * 16u;
    size_t const N = max_batch, T = static_cast<size_t>(max_batch) + parked_cap;
    // the arena: every array begins at a multiple of 256 bytes
    size_t bytes = 0;
    auto const cut = [&bytes](size_t n) { size_t const at = bytes; bytes += (n + 255) / 256 * 256; return at; };
    size_t const o_carry[2] = {cut(sizeof(DstreamCarry)), cut(sizeof(DstreamCarry))}, o_row[2] = {cut(s->row_cap), cut(s->row_cap)};
    size_t const o_parked[2] = {cut(sizeof(DstreamParked) * std::max<size_t>(parked_cap, 1)), cut(sizeof(DstreamParked) * std::max<size_t>(parked_cap, 1))};
    size_t const o_work = cut(sizeof(DstreamWork)), o_partial = cut(4 * MAX_BLOCKS * WAVES_PER_BLOCK), o_out = cut(sizeof(DstreamOut)), o_name = cut(8 * T), o_name_sorted = cut(8 * T);
    size_t o_t[8], o_n[9];
    for (size_t & o : o_t)
      o = cut(4 * T);
    for (size_t & o : o_n)
      o = cut(4 * N);
    size_t const o_me = cut(sizeof(gtx_rec_meta) * N);
    if (!hip_ok(alloc_e(s->arena, bytes), "the stream's arrays", prefix) || !hip_ok(dev_zero(s->arena.get(), bytes), "the stream's arrays", prefix))
      return GTX_ERR_HIP;
    uint8_t * const base = s->arena.get();
    for (int k = 0; k < 2; ++k)
    {
      s->carry[k] = reinterpret_cast<DstreamCarry *>(base + o_carry[k]);
      s->carry_row[k] = base + o_row[k];
      s->parked[k] = reinterpret_cast<DstreamParked *>(base + o_parked[k]);
    }
    DstreamPush & w = s->work;
    w.work = reinterpret_cast<DstreamWork *>(base + o_work);
    w.kept_partial = reinterpret_cast<uint32_t *>(base + o_partial);
    s->d_out = reinterpret_cast<DstreamOut *>(base + o_out);
    w.name = reinterpret_cast<uint64_t *>(base + o_name);
    s->name_sorted = reinterpret_cast<uint64_t *>(base + o_name_sorted);
    uint32_t ** const per_element[8] = {&w.rg, &w.elem, &w.wait, &w.wait_at, &s->by_name, &s->rg_keys, &s->rg_sorted, &s->by_key};
    for (int k = 0; k < 8; ++k)
      *per_element[k] = reinterpret_cast<uint32_t *>(base + o_t[k]);
    uint32_t ** const per_record[9] = {&w.kept_in, &w.prev_scan, &w.head, &w.head_in, &w.task, &w.head_of, &w.emit, &w.emit_at, &w.partner};
    for (int k = 0; k < 9; ++k)
      *per_record[k] = reinterpret_cast<uint32_t *>(base + o_n[k]);
    w.me = reinterpret_cast<gtx_rec_meta *>(base + o_me);
    // what the primitives want at most: asked over a ladder of sizes (1, 2, 3, 4, 6, 8, 12, ... and the largest)
    PrimStorage sizing{nullptr, prefix, nullptr, 0};
    Prims const prims{w.name, s->name_sorted, w.elem, s->by_name, s->rg_keys, s->rg_sorted, s->by_key, w, bits_for(n_read_groups)};
    auto const ask = [&](size_t total)
    {
      uint32_t const t = static_cast<uint32_t>(std::min(total, T)), n = static_cast<uint32_t>(std::min(total, N));
      return prims.previous_kept(sizing, n) && prims.heads(sizing, n) && prims.by_names(sizing, t) && prims.by_groups(sizing, t) && prims.slots(sizing, n, t);
    };
    for (size_t step = 1; step < T; step *= 2)
      if (!ask(step) || !ask(step + step / 2))
        return GTX_ERR_HIP;
    if (!ask(T))
      return GTX_ERR_HIP;
    s->prim_cap = (sizing.most + 255) / 256 * 256 + 256;
    if (!hip_ok(alloc_e(s->prim, s->prim_cap), "the primitives' storage", prefix))
      return GTX_ERR_HIP;
    s->slot.reset(pinned_slot_get());
    if (!s->slot)
    {
      g_last_error = std::string(prefix) + "no pinned memory for the download";
      return GTX_ERR_HIP;
    }
    static_assert(sizeof(DstreamOut) <= 64, "a pinned slot holds the download");
    *out = s.release();
    return GTX_OK;
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string(prefix) + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" void gtx_dstream_destroy(gtx_dstream * s)
{
  if (!s)
    return;
  if (s->device >= 0 && hipSetDevice(s->device) == hipSuccess)
    (void)hipDeviceSynchronize(); // (the blocks go back to a cache that hands them out again)
  delete s;
}

extern "C" int gtx_dstream_push(gtx_dstream * s, const gtx_stream_record * d_recs, const uint8_t * d_seq, uint32_t seq_stride, uint32_t n, uint8_t * d_planes,
                                uint32_t plane_stride, gtx_read_meta * d_meta, uint32_t align_cap, gtx_score_item * d_items, uint32_t item_cap, uint32_t * n_align,
                                uint32_t * n_items, void * stream)
{
  char const * const prefix = "gtx_dstream_push: ";
  if (!s || !n_align || !n_items || (n != 0 && (!d_recs || !d_seq || !d_planes || !d_meta || !d_items)) || seq_stride == 0 || plane_stride == 0 ||
      (plane_stride % PLANE_GROUP_BYTES) != 0 || (reinterpret_cast<uintptr_t>(d_planes) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_recs) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(d_meta) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_items) & 3u) != 0)
  {
    g_last_error = std::string(prefix) + "bad argument (plane rows: a pitch that is a multiple of 16 bytes, 16-byte aligned)";
    return GTX_ERR_ARG;
  }
  if (n > align_cap || n > item_cap)
  {
    g_last_error = std::string(prefix) + "align_cap and item_cap have to hold one entry per pushed record";
    return GTX_ERR_CAPACITY;
  }
  if (n > s->max_batch)
  {
    g_last_error = std::string(prefix) + std::to_string(n) + " records, the stream was made with max_batch " + std::to_string(s->max_batch);
    return GTX_ERR_CAPACITY;
  }
  *n_align = *n_items = 0;
  if (n == 0)
    return GTX_OK;
  if (int const rc = device_ready(s->device, "gtx_dstream_push", ": the stream"))
    return rc;
  try
  {
    hipStream_t const q = static_cast<hipStream_t>(stream);
    uint32_t const cur = s->cur, total = s->n_parked + n;
    DstreamPush a = s->work;
    a.recs = d_recs;
    a.seq = d_seq;
    a.seq_stride = seq_stride;
    a.n = n;
    a.flag_filter = static_cast<uint32_t>(s->params.sam_flag_filter);
    a.force_both = s->params.force_align_both_orientations ? 1u : 0u;
    a.max_read_len = max_read_len_of(s->params);
    a.n_read_groups = s->n_read_groups;
    a.plane_stride = plane_stride;
    a.parked_cap = s->parked_cap;
    a.n_parked = s->n_parked;
    a.row_cap = s->row_cap;
    a.carry = s->carry[cur];
    a.carry_row = s->carry_row[cur];
    a.parked = s->parked[cur];
    a.next_carry = s->carry[cur ^ 1u];
    a.next_carry_row = s->carry_row[cur ^ 1u];
    a.next_parked = s->parked[cur ^ 1u];
    a.perm = s->n_read_groups > 1 ? s->by_key : s->by_name;
    a.planes = d_planes;
    a.meta = d_meta;
    a.items = d_items;
    a.out = s->d_out;
    PrimStorage pool{q, prefix, s->prim.get(), s->prim_cap};
    Prims const prims{a.name, s->name_sorted, a.elem, s->by_name, s->rg_keys, s->rg_sorted, s->by_key, a, bits_for(s->n_read_groups)};
    dim3 const block(64 * WAVES_PER_BLOCK), per_element(blocks_for(total, 64)), per_record8(blocks_for(n, 8));
    a.n_partial = per_element.x * WAVES_PER_BLOCK;
    // (an error half-way leaves kernels behind that write the workspace and the other slot only: the state is as it was)
    struct WaitOnError
    {
      hipStream_t q;
      bool armed = true;
      ~WaitOnError() { if (armed) (void)hipStreamSynchronize(q); }
    } wait_on_error{q};
    if (!hip_ok(hipMemsetAsync(a.work, 0, sizeof(DstreamWork), q), "counters", prefix))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_dstream_classify_kernel, per_element, block, 0, q, a);
    if (!launched("gtx_dstream_classify_kernel") || !prims.previous_kept(pool, n))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_dstream_compare_kernel, per_record8, block, 0, q, a);
    if (!launched("gtx_dstream_compare_kernel") || !prims.heads(pool, n))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_dstream_emit_tasks_kernel, per_record8, block, 0, q, a);
    if (!launched("gtx_dstream_emit_tasks_kernel") || !prims.by_names(pool, total))
      return GTX_ERR_HIP;
    if (s->n_read_groups > 1)
    {
      hipLaunchKernelGGL(gtx_dstream_gather_rg_kernel, per_element, block, 0, q, a, static_cast<uint32_t const *>(s->by_name), s->rg_keys);
      if (!launched("gtx_dstream_gather_rg_kernel") || !prims.by_groups(pool, total))
        return GTX_ERR_HIP;
    }
    hipLaunchKernelGGL(gtx_dstream_walk_kernel, per_element, block, 0, q, a);
    if (!launched("gtx_dstream_walk_kernel") || !prims.slots(pool, n, total))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_dstream_emit_items_kernel, per_element, block, 0, q, a);
    if (!launched("gtx_dstream_emit_items_kernel"))
      return GTX_ERR_HIP;
    hipLaunchKernelGGL(gtx_dstream_finish_kernel, dim3(1), dim3(64), 0, q, a);
    if (!launched("gtx_dstream_finish_kernel"))
      return GTX_ERR_HIP;
    DstreamOut * const got = static_cast<DstreamOut *>(s->slot.get());
    if (!hip_ok(hipMemcpyAsync(got, s->d_out, sizeof(DstreamOut), hipMemcpyDeviceToHost, q), "download", prefix))
      return GTX_ERR_HIP;
    wait_on_error.armed = false;
    if (!hip_ok(hipStreamSynchronize(q), "wait", prefix))
      return GTX_ERR_HIP;
    DstreamOut const o = *got;
    switch (o.status == GTX_OK ? 0u : o.why)
    {
    case 0:
      s->cur = cur ^ 1u;
      s->n_parked = o.n_parked;
      s->n_records = o.n_records;
      s->n_duplicated = o.n_duplicated;
      *n_align = o.n_align;
      *n_items = o.n_items;
      return GTX_OK;
    case DSTREAM_FAIL_RG:
      g_last_error = std::string(prefix) + "read group index out of range";
      break;
    case DSTREAM_FAIL_LONG:
      g_last_error = std::string(prefix) + "a read of " + std::to_string(o.l_qseq) + " bases (the stream's max_read_len is " + std::to_string(a.max_read_len) + ")";
      break;
    case DSTREAM_FAIL_ROW:
      g_last_error = std::string(prefix) + "a record is longer than seq_stride (or than the plane rows)";
      break;
    case DSTREAM_FAIL_CLASH:
      g_last_error = std::string(prefix) + "two reads with one name have the same IS_FIRST_IN_PAIR";
      break;
    case DSTREAM_FAIL_PARKED:
      g_last_error = std::string(prefix) + std::to_string(o.n_parked) + " mates wait at the end of the push, the stream was made with parked_cap " + std::to_string(s->parked_cap);
      break;
    default:
      g_last_error = std::string(prefix) + "the device left no status";
      return GTX_ERR_HIP;
    }
    return static_cast<int>(o.status);
  }
  catch (std::exception const & e)
  {
    g_last_error = std::string(prefix) + e.what();
    return GTX_ERR_CAPACITY;
  }
}

extern "C" int gtx_dstream_finish(gtx_dstream * s, void *)
{
  if (!s)
    return GTX_ERR_ARG;
  s->n_parked = 0; // (the table's length is the host's: nothing to launch)
  return GTX_OK;
}

extern "C" int gtx_dstream_counts(const gtx_dstream * s, uint64_t * n_records, uint64_t * n_duplicated, uint64_t * n_parked)
{
  if (!s)
    return GTX_ERR_ARG;
  if (n_records)
    *n_records = s->n_records;
  if (n_duplicated)
    *n_duplicated = s->n_duplicated;
  if (n_parked)
    *n_parked = s->n_parked;
  return GTX_OK;
}
