// gtx_hbm_passes.hip -- the alignment passes behind the general one: the same algorithm (align_core.inl) over tables that
// live in HBM.  gtx_align_big_kernel (512 paths, 2 048 labels per k-mer), gtx_align_wide_kernel (allele sets of
// GTX_WIDE_MASK_WORDS words) and the exact pass, gtx_align_exact(_wide)_kernel, whose tables have no fixed size.  Behind
// them, for contexts made with gtx_params::max_read_len > GTX_MAX_READ only, the two passes of the long reads:
// gtx_align_long_kernel and gtx_align_exact_long(_wide)_kernel.
// One text per thing: a task is align_one_arena (align_core.inl, the text the emulations run too) plus the hand-on (hbm_task),
// a pass is a prologue that finds its workspace (hbm_table_pass, exact_pass) and the loop over its queue (hbm_queue_loop), both
// templates over an instantiation of align_core.inl (its `Instance`); the kernels are named builds of one call each.  The queues'
// state words and capacities: gtx_pass_queue.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "gtx_ctx.hpp"
#include "wave_hip.hpp"
#include "align_core.hpp"
#include "align_long.hpp"
#include "gtx_hbm_passes.hpp"

namespace gtx
{
// One (read, orientation) task of a pass: its record (slot or arena), and on to the next pass' queue when it met an allele
// number >= 64 or overflowed a table the next pass has larger.  (The device's arena claim moves the cursor whether the record
// fits or not: the arena stays full for the rest of the batch.)
template <class I>
__device__ __forceinline__ void hbm_task(GraphView const & g, IndexView const & ix, typename I::Workspace & ws, uint8_t const * __restrict__ seq,
                                         uint32_t seq_stride, uint32_t * __restrict__ records, uint32_t rec_words, uint32_t task, uint32_t len,
                                         uint32_t * __restrict__ arena, unsigned long long arena_words, unsigned long long * arena_cursor,
                                         uint32_t * __restrict__ next_tasks, uint32_t next_cap, uint32_t * next_state)
{
  uint32_t const status = I::template task<WaveHipMem>(g, ix, ws, seq + static_cast<uint64_t>(task >> 1) * seq_stride, len, (task & 1u) == 1,
                                                       records + static_cast<uint64_t>(task) * rec_words, rec_words, arena, arena_words,
                                                       [&](uint32_t n) { return wave_claim64(arena_cursor, n); });
  if (status && next_tasks && WaveHip::leader())
    queue_push(next_tasks, next_cap, next_state, task);
}

// The queued tasks of a pass, one claim of the queue's cursor per task
template <class I>
__device__ __forceinline__ void hbm_queue_loop(GraphView const & g, IndexView const & ix, typename I::Workspace & ws, uint8_t const * __restrict__ seq,
                                               uint32_t seq_stride, gtx_read_meta const * __restrict__ meta, uint32_t * __restrict__ records,
                                               uint32_t rec_words, uint32_t const * __restrict__ big_tasks, uint32_t big_task_cap, uint32_t * big_state,
                                               uint32_t * __restrict__ arena, unsigned long long arena_words, unsigned long long * arena_cursor,
                                               uint32_t * __restrict__ next_tasks, uint32_t next_cap, uint32_t * next_state)
{
#ifdef GTX_PROF
  if (threadIdx.x < 16)
    ws.prof_acc[threadIdx.x] = 0; // (second-pass cycles are not added to the report)
  WaveHipMem::mem_sync();
#endif
  uint32_t const queued = big_state[Q_QUEUED] < big_task_cap ? big_state[Q_QUEUED] : big_task_cap;
  for (;;)
  {
    uint32_t const t = wave_claim(big_state + Q_CURSOR, 1u);
    if (t >= queued)
      break;
    uint32_t const task = WaveHip::uni(big_tasks[t]);
    uint32_t const len = WaveHip::uni(static_cast<uint32_t>(meta[task >> 1].l_qseq));
    hbm_task<I>(g, ix, ws, seq, seq_stride, records, rec_words, task, len, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state);
  }
}

// Second pass over the queued (read, orientation) tasks: same algorithm instantiated over tables large enough for what
// the reference's own limits admit; one workspace in HBM per workgroup.  The queue is usually empty or tiny.
// A graph with a site of more than 64 alleles has a further pass of the same shape behind it (wide: allele sets of
// GTX_WIDE_MASK_WORDS words, a larger table of walk candidates: one round of a walk branches into every allele of a site):
// a task that met an allele number >= 64 or overflowed a table is handed on to it (next_tasks / next_state).
// (registers for four wavefronts per SIMD -- 128 instead of the 193 the compiler takes when left alone: the pass has no task on
//  most batches, but every one of its workgroups has to be PLACED before it can see that, and beside another batch's kernels
//  a wavefront of 196 registers waited 0.14 ms for room; what it spills only matters on the rare batch that needs the pass)
#ifndef GTX_HBM_PASS_WAVES
#define GTX_HBM_PASS_WAVES 4
#endif
#define GTX_HBM_PASS_ATTR __attribute__((amdgpu_waves_per_eu(GTX_HBM_PASS_WAVES, GTX_HBM_PASS_WAVES)))
#define GTX_HBM_PASS_ARGS(WS)                                                                                                      \
  GraphView g, IndexView ix, uint8_t const *__restrict__ seq, uint32_t seq_stride, gtx_read_meta const *__restrict__ meta,         \
    uint32_t *__restrict__ records, uint32_t rec_words, uint32_t const *__restrict__ big_tasks, uint32_t big_task_cap,             \
    uint32_t *big_state, WS *workspaces, uint32_t *__restrict__ arena, unsigned long long arena_words,                             \
    unsigned long long *arena_cursor, uint32_t *__restrict__ next_tasks, uint32_t next_cap, uint32_t *next_state

template <class I>
__device__ __forceinline__ void hbm_table_pass(GTX_HBM_PASS_ARGS(typename I::Workspace))
{
  if (big_state[Q_QUEUED] == 0) // (nearly every batch: nothing reached this pass -- leave before the workspace is touched)
    return;
  typename I::Workspace & ws = workspaces[blockIdx.x];
  // the dense start / end tables of the chaining's searches live in LDS (align_core.inl: PpKeyTables)
  __shared__ uint32_t s_pp_keys[2][I::Cfg::MAXPP];
  __shared__ uint64_t s_pp_bits[I::Cfg::MAXPP / 64 + 1];
  ws.pp_start = s_pp_keys[0];
  ws.pp_end = s_pp_keys[1];
  ws.bits_pp = s_pp_bits;
  WaveHipMem::mem_sync();
  hbm_queue_loop<I>(g, ix, ws, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, arena, arena_words, arena_cursor,
                    next_tasks, next_cap, next_state);
}

__global__ __launch_bounds__(64) GTX_HBM_PASS_ATTR void gtx_align_big_kernel(GTX_HBM_PASS_ARGS(big::AlignWorkspace))
{
  hbm_table_pass<big::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, workspaces, arena,
                                arena_words, arena_cursor, next_tasks, next_cap, next_state);
}

__global__ __launch_bounds__(64) GTX_HBM_PASS_ATTR void gtx_align_wide_kernel(GTX_HBM_PASS_ARGS(wide::AlignWorkspace))
{
  hbm_table_pass<wide::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, workspaces, arena,
                                 arena_words, arena_cursor, next_tasks, next_cap, next_state);
}

// The exact pass (align_core.hpp: namespace exact): the same loop over a workspace whose tables are cut out of the
// workgroup's part of a slab of HBM at run time.  Launched three times (exact_launches, below): workgroups with a small part
// each, with a large part each, then one workgroup with the whole slab for what did not fit a part (each launch's queue is
// the next_tasks of the one before).
// (at most one workgroup of this pass per CU, usually none with work: no register diet -- all the registers a wavefront can name)
#define GTX_EXACT_PASS_ATTR __attribute__((amdgpu_waves_per_eu(1, 2)))
#ifndef GTX_EXACT_LDS_KEYS
#define GTX_EXACT_LDS_KEYS 4096
#endif
constexpr uint32_t EXACT_LDS_KEYS = GTX_EXACT_LDS_KEYS; // paths whose dense start / end tables fit the exact pass' 32 KB of LDS
#define GTX_EXACT_PASS_ARGS                                                                                                        \
  GraphView g, IndexView ix, uint8_t const *__restrict__ seq, uint32_t seq_stride, gtx_read_meta const *__restrict__ meta,         \
    uint32_t *__restrict__ records, uint32_t rec_words, uint32_t const *__restrict__ big_tasks, uint32_t big_task_cap,             \
    uint32_t *big_state, uint8_t *slab, unsigned long long part_bytes /* the slab's */, unsigned long long min_part_bytes,         \
    uint32_t fixed_parts, uint32_t cand_cap, uint32_t cap_v, uint32_t *__restrict__ arena, unsigned long long arena_words,         \
    unsigned long long *arena_cursor, uint32_t *__restrict__ next_tasks, uint32_t next_cap, uint32_t *next_state, uint32_t lds_keys

template <class I>
__device__ __forceinline__ void exact_pass(GTX_EXACT_PASS_ARGS)
{
  if (big_state[Q_QUEUED] == 0) // (nearly every batch: nothing reached this pass)
    return;
  // The slab is cut into as many parts as there are tasks, at most one per workgroup of the grid and none smaller than
  // min_part_bytes: a handful of tasks get large parts, thousands -- every read over one long repeat -- get small ones and
  // all of the grid (a task is milliseconds of dependent round trips: the tasks in flight are the pass' throughput).
  {
    unsigned long long const q = big_state[Q_QUEUED] < big_task_cap ? big_state[Q_QUEUED] : big_task_cap;
    unsigned long long parts = (q < gridDim.x && !fixed_parts) ? q : gridDim.x; // (fixed_parts: a test switch, GTX_EXACT_PARTS)
    if (min_part_bytes && parts * min_part_bytes > part_bytes)
      parts = part_bytes / min_part_bytes ? part_bytes / min_part_bytes : 1ull;
    if (blockIdx.x >= parts)
      return;
    part_bytes = (part_bytes / parts) & ~255ull;
  }
  typename I::Workspace & ws = *reinterpret_cast<typename I::Workspace *>(slab + static_cast<unsigned long long>(blockIdx.x) * part_bytes);
  if (!I::template setup<WaveHipMem>(&ws, part_bytes, cand_cap, cap_v))
  {
    // a part that cannot hold one path: everything goes on to the launch that has the whole slab (or keeps its status)
    if (blockIdx.x == 0 && WaveHip::leader() && next_tasks)
    {
      uint32_t const q = big_state[Q_QUEUED] < big_task_cap ? big_state[Q_QUEUED] : big_task_cap;
      for (uint32_t t = 0; t < q; ++t)
        queue_push(next_tasks, next_cap, next_state, big_tasks[t]);
    }
    return;
  }
  // (the dense start / end tables in LDS when the part's paths fit there, else where exact_setup put them in the slab)
  extern __shared__ uint32_t s_pp_keys[]; // 2 x lds_keys words: the launch sizes them
  if (ws.cap_p <= lds_keys)
  {
    ws.pp_start = s_pp_keys;
    ws.pp_end = s_pp_keys + lds_keys;
  }
  WaveHipMem::mem_sync();
  hbm_queue_loop<I>(g, ix, ws, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, arena, arena_words, arena_cursor,
                    next_tasks, next_cap, next_state);
}

__global__ __launch_bounds__(64) GTX_EXACT_PASS_ATTR void gtx_align_exact_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exact::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                            fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}
__global__ __launch_bounds__(64) GTX_EXACT_PASS_ATTR void gtx_align_exact_wide_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exactw::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                             fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}
// ... and a build of it that can be PLACED beside a full chip -- registers for four wavefronts per SIMD (128, what the HBM-table
// pass takes; the pass' own 186 need three wavefronts of the position-hinted pass to retire on one SIMD and nobody to take their
// room), launched with 2 KB of LDS instead of 32 (a CU that holds fourteen workgroups of that pass has 20 KB left) -- for the batch
// whose predecessor sent nothing this way: its four workgroups find the empty queue in 5 us instead of waiting 100-200 us for the
// position-hinted pass of the next batch to end (round 6, kernel trace of the staggered schedule).  A task that does come is done, slowly.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void gtx_align_exact_light_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exact::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                            fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void gtx_align_exact_wide_light_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exactw::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                             fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}
// tier 2 of the long reads: the exact pass over what gtx_align_long_kernel refused
__global__ __launch_bounds__(64) GTX_EXACT_PASS_ATTR void gtx_align_exact_long_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exactl::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                             fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}
__global__ __launch_bounds__(64) GTX_EXACT_PASS_ATTR void gtx_align_exact_long_wide_kernel(GTX_EXACT_PASS_ARGS)
{
  exact_pass<exactlw::Instance>(g, ix, seq, seq_stride, meta, records, rec_words, big_tasks, big_task_cap, big_state, slab, part_bytes, min_part_bytes,
                              fixed_parts, cand_cap, cap_v, arena, arena_words, arena_cursor, next_tasks, next_cap, next_state, lds_keys);
}

// Tier 1 of the long reads (gtx_params::max_read_len > GTX_MAX_READ): the passes in front wrote a header with
// GTX_ST_RECORD_OVERFLOW for every read over GTX_MAX_READ bases and queued nothing for it.  This pass finds those reads
// itself -- a wavefront claims 64 reads of the batch at a time and takes the ones of GTX_MAX_READ + 1 .. max_len bases -- so
// that no queue bounds how many there can be, and writes both slots of each by align_read's rules, as the position-hinted
// pass does for a short read: the reverse orientation when needs_reverse, else an empty header (none under
// GTX_FLAG_FORWARD_ONLY).  A task that exceeds the tables goes on to tier 2 (next_tasks), as from the HBM-table pass.
// long_state: the read cursor and the tasks this pass took (gtx_pass_queue.hpp: LONG_READ_CURSOR, LONG_TASKS).
__global__ __launch_bounds__(64) GTX_HBM_PASS_ATTR void gtx_align_long_kernel(GraphView g, IndexView ix, uint8_t const * __restrict__ seq, uint32_t seq_stride,
                                                                             gtx_read_meta const * __restrict__ meta, uint32_t n_reads, uint32_t max_len,
                                                                             uint32_t force_both, uint32_t * __restrict__ records, uint32_t rec_words,
                                                                             uint32_t * long_state, longr::AlignWorkspace * workspaces,
                                                                             uint32_t * __restrict__ arena, unsigned long long arena_words,
                                                                             unsigned long long * arena_cursor, uint32_t * __restrict__ next_tasks,
                                                                             uint32_t next_cap, uint32_t * next_state)
{
  longr::AlignWorkspace & ws = workspaces[blockIdx.x];
  __shared__ uint32_t s_pp_keys[2][longr::AlignCfg::MAXPP];
  __shared__ uint64_t s_pp_bits[longr::AlignCfg::MAXPP / 64 + 1];
  ws.pp_start = s_pp_keys[0];
  ws.pp_end = s_pp_keys[1];
  ws.bits_pp = s_pp_bits;
  WaveHipMem::mem_sync();
  uint32_t const lane = threadIdx.x & 63u;
  uint32_t n_tasks = 0;
  auto task_of = [&](uint32_t task, uint32_t len)
  {
    hbm_task<longr::Instance>(g, ix, ws, seq, seq_stride, records, rec_words, task, len, arena, arena_words, arena_cursor, next_tasks, next_cap,
                              next_state);
    ++n_tasks;
  };
  for (;;)
  {
    uint32_t const first = wave_claim(long_state + LONG_READ_CURSOR, 64u);
    if (first >= n_reads)
      break;
    uint32_t const len_l = first + lane < n_reads ? static_cast<uint32_t>(meta[first + lane].l_qseq) : 0u;
    unsigned long long todo = __ballot(len_l > GTX_MAX_READ && len_l <= max_len);
    while (todo)
    {
      uint32_t const read = first + static_cast<uint32_t>(__builtin_ctzll(todo));
      todo &= todo - 1ull;
      gtx_read_meta const m = meta[read];
      uint32_t const len = WaveHip::uni(static_cast<uint32_t>(m.l_qseq));
      bool const rev = WaveHip::uni(static_cast<uint32_t>(needs_reverse(m, force_both != 0))) != 0u;
      task_of(2u * read, len);
      if (rev)
        task_of(2u * read + 1u, len);
      else if ((m.flag & GTX_FLAG_FORWARD_ONLY) == 0 && lane == 0)
      {
        uint32_t * rec = records + (2ull * read + 1ull) * rec_words;
        rec[0] = 0;
        rec[1] = len << 16;
      }
    }
  }
  if (n_tasks && lane == 0)
    atomicAdd(long_state + LONG_TASKS, n_tasks);
}

// The side bytes of the long reads (gtx_align_batch_*_flags / _triaged behind the position-hinted pass, which left them as
// for a read it does not align): the final records' GTX_TASK_HAS_VARIANTS bits, and the read's bit of the variant masks
__global__ __launch_bounds__(256) void gtx_long_flags_kernel(gtx_read_meta const * __restrict__ meta, uint32_t n_reads, uint32_t max_len,
                                                            uint32_t force_both, uint32_t const * __restrict__ records, uint32_t rec_words,
                                                            uint8_t * __restrict__ task_flags, unsigned long long * __restrict__ var_mask)
{
  for (uint32_t read = blockIdx.x * blockDim.x + threadIdx.x; read < n_reads; read += gridDim.x * blockDim.x)
  {
    gtx_read_meta const m = meta[read];
    if (m.l_qseq <= GTX_MAX_READ || m.l_qseq > max_len)
      continue;
    uint8_t const f = static_cast<uint8_t>(records[2ull * read * rec_words + 1] >> 31);
    task_flags[2ull * read] = f;
    task_flags[2ull * read + 1] = needs_reverse(m, force_both != 0) ? static_cast<uint8_t>(records[(2ull * read + 1) * rec_words + 1] >> 31) : 0u;
    if (var_mask && f != 0)
      atomicOr(var_mask + (read >> 6), 1ull << (read & 63u));
  }
}


uint64_t big_workspace_bytes() { return sizeof(big::AlignWorkspace); }
uint64_t wide_workspace_bytes() { return sizeof(wide::AlignWorkspace); }

char const * launch_hbm_passes(HbmPassArgs const & a, hipStream_t stream)
{
  unsigned long long const arena_words = a.arena_words;
  bool const wide_pass = a.wide_tasks != nullptr;
  hipLaunchKernelGGL(gtx_align_big_kernel, dim3(a.big_blocks), dim3(64), 0, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, a.records, a.rec_words,
                     a.big_tasks, a.big_task_cap, a.big_state, static_cast<big::AlignWorkspace *>(a.big_ws), a.arena, arena_words, a.arena_cursor,
                     wide_pass ? a.wide_tasks : a.exact_tasks, wide_pass ? WIDE_TASK_CAP : EXACT_TASK_CAP, wide_pass ? a.wide_state : a.exact_state);
  if (hipGetLastError() != hipSuccess)
    return "gtx_align_big_kernel launch";
  if (wide_pass) // graphs with a site of more than 64 alleles: the tasks that met an allele number >= 64
  {
    hipLaunchKernelGGL(gtx_align_wide_kernel, dim3(CallScratch::WIDE_BLOCKS), dim3(64), 0, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, a.records,
                       a.rec_words, a.wide_tasks, WIDE_TASK_CAP, a.wide_state, static_cast<wide::AlignWorkspace *>(a.wide_ws), a.arena,
                       arena_words, a.arena_cursor, a.exact_tasks, EXACT_TASK_CAP, a.exact_state);
    if (hipGetLastError() != hipSuccess)
      return "gtx_align_wide_kernel launch";
  }
  return nullptr;
}

// The three launches of an exact pass over the queues q1, q1 + EXACT_TASK_CAP, q1 + 2 EXACT_TASK_CAP and the EXACT_STATE_WORDS
// state words st1: the short reads' (launch_exact_passes) and the long reads' tier 2 (launch_long_passes)
template <class Kernel>
static char const * exact_launches(HbmPassArgs const & a, Kernel kernel, bool light, uint32_t * q1, uint32_t * st1, uint32_t max_sites, char const * what,
                                   hipStream_t stream)
{
  unsigned long long const arena_words = a.arena_words;
  // the exact pass: what exceeded the tables above, with a small part of the slab per task (up to exact_parts of them side by
  // side), then what did not fit with a large part (up to EXACT_LARGE_PARTS), then -- one workgroup -- with all of it.  Nearly
  // always all three find an empty queue and leave at once.
  // (a small part's paths have room for EXACT_PART_SITES variant sites and its walks for exact_part_cand_cap candidates, a large
  //  part's for EXACT_LARGE_SITES, the whole slab for the proven bounds: a site per read base, 128 live sequences times the alleles
  //  of the graph's widest site)
  static_assert(EXACT_LAUNCHES == 3, "small parts, large parts, the whole slab");
  uint32_t * const q2 = q1 + EXACT_TASK_CAP, * const q3 = q2 + EXACT_TASK_CAP;
  uint32_t * const st2 = st1 + Q_WORDS, * const st3 = st2 + Q_WORDS, * const st4 = st3 + Q_WORDS;
  uint32_t const lds_keys = light ? 256u : EXACT_LDS_KEYS;
  size_t const lds_bytes = 2u * lds_keys * sizeof(uint32_t);
  unsigned long long const slab_bytes = a.exact_slab_bytes, min_part = slab_bytes / a.exact_parts;
  // (the second launch: parts of at least 16 MB -- 32 of them in a 512 MB slab, 128 in the 2 GB slab of a large batch: on a reference
  //  with repeats two hundred tasks come this far, and 32 parts took them in six rounds of a millisecond each)
  // (graphs with sites of more than 64 alleles keep 32: a walk's candidate table alone can be tens of megabytes there)
  uint32_t const large_parts = a.exact_fixed_parts ? 1u
                               : a.wide_sites    ? EXACT_LARGE_PARTS
                                                 : static_cast<uint32_t>(std::min<unsigned long long>(256ull, std::max<unsigned long long>(EXACT_LARGE_PARTS, slab_bytes >> 24)));
  uint32_t const grid1 = a.exact_grid_limit ? std::min<uint32_t>(a.exact_parts, a.exact_grid_limit) : a.exact_parts;
  uint32_t const grid2 = a.exact_grid_limit ? std::min<uint32_t>(large_parts, a.exact_grid_limit) : large_parts;
  hipLaunchKernelGGL(kernel, dim3(grid1), dim3(64), lds_bytes, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, a.records, a.rec_words, q1,
                     EXACT_TASK_CAP, st1, a.exact_slab, slab_bytes, min_part, a.exact_fixed_parts ? 1u : 0u, a.exact_part_cand_cap,
                     EXACT_PART_SITES, a.arena, arena_words, a.arena_cursor, q2, EXACT_TASK_CAP, st2, lds_keys);
  hipLaunchKernelGGL(kernel, dim3(grid2), dim3(64), lds_bytes, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, a.records, a.rec_words, q2,
                     EXACT_TASK_CAP, st2, a.exact_slab, slab_bytes, slab_bytes / large_parts, 0u, a.exact_cand_cap,
                     EXACT_LARGE_SITES, a.arena, arena_words, a.arena_cursor, q3, EXACT_TASK_CAP, st3, lds_keys);
  // (what even the whole slab cannot hold is counted in st4: a queue of capacity 0)
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), lds_bytes, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, a.records, a.rec_words, q3, EXACT_TASK_CAP,
                     st3, a.exact_slab, slab_bytes, 0ull, 0u, a.exact_cand_cap, max_sites, a.arena, arena_words, a.arena_cursor, q3, 0u, st4, lds_keys);
  if (hipGetLastError() != hipSuccess)
    return what;
  return nullptr;
}

char const * launch_exact_passes(HbmPassArgs const & a, hipStream_t stream)
{
  // (nothing expected -- the batch before sent no task here: the build that can be placed beside a full chip, four workgroups a launch)
  bool const light = a.exact_grid_limit != 0 && a.exact_grid_limit <= 4u;
  auto kernel = light ? (a.wide_sites ? gtx_align_exact_wide_light_kernel : gtx_align_exact_light_kernel)
                      : (a.wide_sites ? gtx_align_exact_wide_kernel : gtx_align_exact_kernel);
  return exact_launches(a, kernel, light, a.exact_tasks, a.exact_state, exact::AlignCfg::MAXV, "gtx_align_exact_kernel launch", stream);
}

uint64_t long_workspace_bytes() { return sizeof(longr::AlignWorkspace); }

char const * launch_long_passes(HbmPassArgs const & a, LongPassArgs const & l, hipStream_t stream)
{
  uint32_t * const st1 = l.state + LONG_STATE_EXACT; // (tier 2's state words behind tier 1's)
  HbmPassArgs b = a;
  b.exact_grid_limit = 0; // (the short reads' grid limit says nothing about the long ones)
  hipLaunchKernelGGL(gtx_align_long_kernel, dim3(l.blocks), dim3(64), 0, stream, a.g, a.ix, a.seq, a.seq_stride, a.meta, l.n_reads, l.max_len,
                     l.force_both ? 1u : 0u, a.records, a.rec_words, l.state, static_cast<longr::AlignWorkspace *>(l.ws), a.arena,
                     static_cast<unsigned long long>(a.arena_words), a.arena_cursor, l.tasks, EXACT_TASK_CAP, st1);
  if (hipGetLastError() != hipSuccess)
    return "gtx_align_long_kernel launch";
  // (wide allele sets: a path with room for all 1 000 sites of a long read is 320 KB, and the whole slab would hold too few of
  //  them for the label lists of a site with thousands of alleles -- its paths get room for GTX_MAX_READ sites, as in exactw)
  return a.wide_sites ? exact_launches(b, gtx_align_exact_long_wide_kernel, false, l.tasks, st1, GTX_MAX_READ,
                                       "gtx_align_exact_long_wide_kernel launch", stream)
                      : exact_launches(b, gtx_align_exact_long_kernel, false, l.tasks, st1, exactl::AlignCfg::MAXV,
                                       "gtx_align_exact_long_kernel launch", stream);
}

char const * launch_long_flags(LongPassArgs const & l, uint32_t const * records, uint32_t rec_words, uint8_t * task_flags,
                               unsigned long long * var_mask, hipStream_t stream)
{
  hipLaunchKernelGGL(gtx_long_flags_kernel, dim3(std::min<uint32_t>((l.n_reads + 255u) / 256u, 4096u)), dim3(256), 0, stream, l.meta, l.n_reads,
                     l.max_len, l.force_both ? 1u : 0u, records, rec_words, task_flags, var_mask);
  return hipGetLastError() != hipSuccess ? "gtx_long_flags_kernel launch" : nullptr;
}
} // namespace gtx
