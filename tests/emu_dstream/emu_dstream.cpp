// Host emulation of the record stream's decisions on the device (gtx_dstream.hip): the pushes of a script through the kernels' source
// (gtx_dstream_dev.hpp) over a sequential wave, built with AddressSanitizer / UBSan.
//   emu_dstream case.bin out.bin
// case.bin: 12 uint32 (sam_flag_filter, force_align_both_orientations, max_read_len, n_read_groups, max_batch, parked_cap, seq_stride,
// plane_stride, waves, n_pushes, n_records, 0); the records; their rows; per push 6 uint32 (lo, hi, align_cap, item_cap, and the
// entries its output arrays hold: tasks, items).
// out.bin: per push 8 uint32 (status, n_align, n_items, 0, and the four words of the download that say why a push failed: why, record,
// l_qseq, n_parked -- of a push that runs no kernel 0, 0, 0 and the mates that wait), 3 uint64 (records, duplicated, parked), then the
// three output arrays.
// Per push the steps as the library launches them, each over `waves` wavefronts (wavefront w takes the tiles w, w + waves, ...).  A
// STABLE HOST SORT AND HOST LOOPS STAND IN FOR THE rocPRIM CALLS between the kernels (the scans and the two sorts by key): what is
// emulated is the kernels' text, not rocPRIM.  The push's records and rows are copied into heap blocks of exactly their sizes, the
// outputs are blocks of exactly the entries the case names (filled with 0xA5), the workspace arrays have exactly max_batch or
// max_batch + parked_cap entries and the parked tables parked_cap: a load or a store outside of any of them stops the program.  All
// blocks are 16-byte aligned, as device memory is (the kernels test the alignment themselves before they load 16 bytes at once).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../wave_seq.hpp"
#include "gtx_dstream_dev.hpp" // from the Makefile's CSRC

using namespace gtx;

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
bool write_exact(std::FILE * f, void const * p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }

// a heap block of exactly n elements, 16-byte aligned, every byte `fill`
template <class T>
struct Block
{
  T * p = nullptr;
  size_t n = 0;
  explicit Block(size_t n_, int fill = 0xA5) : n(n_)
  {
    void * v = nullptr;
    size_t const bytes = n * sizeof(T);
    if (posix_memalign(&v, 16, bytes != 0 ? bytes : 1) != 0)
      std::abort();
    p = static_cast<T *>(v);
    std::memset(v, fill, bytes);
  }
  Block(Block const &) = delete;
  Block & operator=(Block const &) = delete;
  ~Block() { std::free(p); }
  T * get() const { return n ? p : nullptr; }
};

void inclusive_max(uint32_t const * in, uint32_t * out, uint32_t n)
{
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; ++i)
    out[i] = m = std::max(m, in[i]);
}

void exclusive_sum(uint32_t const * in, uint32_t * out, uint32_t n)
{
  uint32_t s = 0;
  for (uint32_t i = 0; i < n; ++i)
  {
    out[i] = s;
    s += in[i];
  }
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_dstream case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t h[12];
  if (!f || !read_exact(f, h, sizeof h))
    return 2;
  uint32_t const flag_filter = h[0], force_both = h[1], max_read_len = h[2] ? h[2] : GTX_MAX_READ, n_read_groups = h[3], max_batch = h[4], parked_cap = h[5],
                 seq_stride = h[6], plane_stride = h[7], waves = h[8], n_pushes = h[9], n_records = h[10];
  if (waves == 0 || max_batch == 0 || n_read_groups == 0 || seq_stride == 0 || plane_stride == 0 || plane_stride % 16u != 0)
    return 2;
  std::vector<gtx_stream_record> all_recs(n_records);
  std::vector<uint8_t> all_rows(static_cast<size_t>(n_records) * seq_stride);
  if (!read_exact(f, all_recs.data(), n_records * sizeof(gtx_stream_record)) || !read_exact(f, all_rows.data(), all_rows.size()))
    return 2;
  std::FILE * o = std::fopen(argv[2], "wb");
  if (!o)
    return 2;

  // the stream: what gtx_dstream_create makes
  uint32_t const row_cap = (dstream_dev::nib_bytes(max_read_len) + 15u) / 16u * 16u;
  size_t const N = max_batch, T = static_cast<size_t>(max_batch) + parked_cap;
  Block<DstreamCarry> carry0(1, 0), carry1(1, 0);
  Block<uint8_t> carry_row0(row_cap, 0), carry_row1(row_cap, 0);
  Block<DstreamParked> parked0(parked_cap), parked1(parked_cap);
  DstreamCarry * const carry[2] = {carry0.p, carry1.p};
  uint8_t * const carry_row[2] = {carry_row0.p, carry_row1.p};
  DstreamParked * const parked[2] = {parked0.get(), parked1.get()};
  Block<DstreamWork> work(1);
  Block<uint32_t> kept_partial(waves);
  Block<DstreamOut> out(1);
  Block<uint64_t> name(T);
  Block<uint32_t> rg(T), elem(T), wait(T), wait_at(T), by_name(T), rg_keys(T), by_key(T);
  Block<uint32_t> kept_in(N), prev_scan(N), head(N), head_in(N), task(N), head_of(N), emit(N), emit_at(N), partner(N);
  Block<gtx_rec_meta> me(N);
  uint32_t cur = 0, n_parked = 0;
  uint64_t n_kept_records = 0, n_duplicated = 0;

  for (uint32_t k = 0; k < n_pushes; ++k)
  {
    uint32_t q[6];
    if (!read_exact(f, q, sizeof q))
      return 2;
    uint32_t const lo = q[0], hi = q[1], align_cap = q[2], item_cap = q[3], room_align = q[4], room_items = q[5];
    if (lo > hi || hi > n_records)
      return 2;
    uint32_t const n = hi - lo;
    Block<gtx_stream_record> recs(n);
    Block<uint8_t> rows(static_cast<size_t>(n) * seq_stride), planes(static_cast<size_t>(room_align) * plane_stride);
    Block<gtx_read_meta> meta(room_align);
    Block<gtx_score_item> items(room_items);
    if (n)
    {
      std::memcpy(static_cast<void *>(recs.p), all_recs.data() + lo, n * sizeof(gtx_stream_record));
      std::memcpy(rows.p, all_rows.data() + static_cast<size_t>(lo) * seq_stride, static_cast<size_t>(n) * seq_stride);
    }
    uint32_t status = GTX_OK, n_align = 0, n_items = 0;
    uint32_t reason[4] = {0, 0, 0, n_parked};
    if (n > align_cap || n > item_cap || n > max_batch)
      status = GTX_ERR_CAPACITY;
    else if (n != 0)
    {
      uint32_t const total = n_parked + n;
      DstreamPush a{};
      a.recs = recs.p;
      a.seq = rows.p;
      a.seq_stride = seq_stride;
      a.n = n;
      a.flag_filter = flag_filter;
      a.force_both = force_both;
      a.max_read_len = max_read_len;
      a.n_read_groups = n_read_groups;
      a.plane_stride = plane_stride;
      a.parked_cap = parked_cap;
      a.n_parked = n_parked;
      a.row_cap = row_cap;
      a.carry = carry[cur];
      a.carry_row = carry_row[cur];
      a.parked = parked[cur];
      a.next_carry = carry[cur ^ 1u];
      a.next_carry_row = carry_row[cur ^ 1u];
      a.next_parked = parked[cur ^ 1u];
      a.work = work.p;
      a.kept_partial = kept_partial.p;
      a.n_partial = waves;
      a.name = name.p;
      a.rg = rg.p;
      a.elem = elem.p;
      a.wait = wait.p;
      a.wait_at = wait_at.p;
      a.kept_in = kept_in.p;
      a.prev_scan = prev_scan.p;
      a.head = head.p;
      a.head_in = head_in.p;
      a.task = task.p;
      a.head_of = head_of.p;
      a.emit = emit.p;
      a.emit_at = emit_at.p;
      a.partner = partner.p;
      a.me = me.p;
      a.perm = n_read_groups > 1 ? by_key.p : by_name.p;
      a.planes = planes.get();
      a.meta = meta.get();
      a.items = items.get();
      a.out = out.p;
      std::memset(work.p, 0, sizeof(DstreamWork));
      for (uint32_t w = 0; w < waves; ++w)
        dstream_classify_wave<WaveSeq>(a, w, waves);
      inclusive_max(a.kept_in, a.prev_scan, n);
      for (uint32_t w = 0; w < waves; ++w)
        dstream_compare_wave<WaveSeq>(a, w, waves);
      exclusive_sum(a.head, a.task, n);
      inclusive_max(a.head_in, a.head_of, n);
      for (uint32_t w = 0; w < waves; ++w)
        dstream_emit_tasks_wave<WaveSeq>(a, w, waves);
      // the sort by name: stable, the values are the elements 0 .. total - 1
      std::copy(elem.p, elem.p + total, by_name.p);
      std::stable_sort(by_name.p, by_name.p + total, [&](uint32_t x, uint32_t y) { return name.p[x] < name.p[y]; });
      if (n_read_groups > 1)
      {
        for (uint32_t w = 0; w < waves; ++w)
          dstream_gather_rg_wave<WaveSeq>(a, by_name.p, rg_keys.p, w, waves);
        // the sort by read group: stable, by the keys as they stand beside the values
        std::vector<uint32_t> order(total);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rg_keys.p[x] < rg_keys.p[y]; });
        for (uint32_t s = 0; s < total; ++s)
          by_key.p[s] = by_name.p[order[s]];
      }
      for (uint32_t w = 0; w < waves; ++w)
        dstream_walk_wave<WaveSeq>(a, w, waves);
      exclusive_sum(a.emit, a.emit_at, n);
      exclusive_sum(a.wait, a.wait_at, total);
      for (uint32_t w = 0; w < waves; ++w)
        dstream_emit_items_wave<WaveSeq>(a, w, waves);
      dstream_finish_wave<WaveSeq>(a);
      status = out.p->status;
      reason[0] = out.p->why;
      reason[1] = out.p->record;
      reason[2] = out.p->l_qseq;
      reason[3] = out.p->n_parked;
      if (status == GTX_OK)
      {
        cur ^= 1u;
        n_parked = out.p->n_parked;
        n_kept_records = out.p->n_records;
        n_duplicated = out.p->n_duplicated;
        n_align = out.p->n_align;
        n_items = out.p->n_items;
      }
    }
    uint32_t const head_words[8] = {status, n_align, n_items, 0, reason[0], reason[1], reason[2], reason[3]};
    uint64_t const counts[3] = {n_kept_records, n_duplicated, n_parked};
    if (!write_exact(o, head_words, sizeof head_words) || !write_exact(o, counts, sizeof counts) || !write_exact(o, planes.p, planes.n) ||
        !write_exact(o, meta.p, meta.n * sizeof(gtx_read_meta)) || !write_exact(o, items.p, items.n * sizeof(gtx_score_item)))
      return 2;
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 2;
}
