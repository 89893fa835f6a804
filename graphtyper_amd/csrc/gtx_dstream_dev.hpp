// gtx_dstream_dev.hpp -- the record stream's decisions on the device, kernel source: gtx_stream_push (gtx_capi.cpp: stream_push<> with
// plane rows, is_sv_graph == 0) over records that are in device memory, restated without its loop-carried map.  The launches and the
// primitives between them (scans and stable sorts): gtx_dstream.hip.
//
// The definition -- what a push of n records leaves, given the stream's state (the previous kept record with its head's alignment index
// and forward-only bit, the parked mates in stream order, next_align_index, the counters):
//   checks    over all n records, dropped ones too, before anything is consumed: the first record in record order that fails one, and
//             of its checks the first in the host's order -- rg >= n_read_groups (ARG), l_qseq > max_read_len (UNSUPPORTED),
//             (l_qseq + 1) / 2 > seq_stride or l_qseq > 2 * plane_stride (ARG).  The word `fail` holds the maximum of
//             0xFFFFFFFF - (4 * record + check): the same record and check whatever the grid.
//   kept      (flag & sam_flag_filter) == 0.
//   duplicate a kept record that equals the PREVIOUS KEPT record (of this push, or the one the stream carries) in tid, pos, l_qseq and
//             the first (l_qseq + 1) / 2 bytes of its nibble row, the pad nibble of an odd read included.  Any other kept record is a head.
//             [1] The host compares with the last HEAD.  Equality in (tid, pos, l_qseq, bytes) is an equivalence relation, and by
//             induction over the kept records behind a head h every one of them up to the first non-duplicate equals h: if the previous
//             kept record p equals h (or is h), then r == p iff r == h, by transitivity.  So "equals the previous kept record" and
//             "equals the last head" name the same records, and the head of a duplicate is the last head in front of it.
//   tasks     the heads in record order; head k of the push has align_index = next_align_index + k, the plane row
//             planes_from_nibbles(row, (l_qseq + 1) / 2, plane_stride / 16) -- the whole row, zeros behind the read, the pad nibble
//             kept --, and gtx_read_meta {l_qseq, flag | fo, tid, mtid, isize, pos - clip}: clip the front operation's length when
//             n_cigar != 0 and its code is 4; fo = GTX_FLAG_FORWARD_ONLY when (the read is unpaired, or tid == mtid and -1200 < isize <
//             1200 and bits 16 and 32 of flag differ) and not force_align_both_orientations.
//   rec meta  of every kept record: {align_index of its head, flag | fo OF ITS HEAD, mapq, score_diff, pos, isize}.
//             [2] The host keeps prev_forward_only from the last head and never recomputes it for a duplicate, so a duplicate whose own
//             flags or isize would decide otherwise still carries its head's bit: the bit is a function of the head, found by the same
//             max-scan that finds the head.
//   pairing   per key (rg, name_id), the occurrences in stream order, a mate parked by an earlier push first.  Nothing waiting and
//             flag & 1: the record waits.  Nothing waiting and unpaired: an item {me, {GTX_INVALID_ID, 0 ...}, sample, 0}.  Something
//             waiting: the same flag & 64 on both is the clash (ARG); else an item {the waiting one's meta, me, THIS record's sample,
//             0} and nothing waits.  Items leave in the order of the records that emit them; what still waits at the end goes to the
//             parked table, in stream order.
//             [3] The host's map holds at most one entry per key, and a record looks at and changes the entry of its own key only: the
//             map is a product of independent two-state machines (nothing waits / x waits), one per key, and the stream order matters
//             inside a key alone.  A stable sort by key lays each machine's inputs side by side in stream order; one lane runs it.
//             Which record emits, and with whom, is thereby fixed per record; the order of the items is the record order of the emitters,
//             which an exclusive sum over the emit bits restores.
//   failures  the clash, and more than parked_cap waiting at the end: the next state is written beside the old one (two slots) and the
//             host adopts it only on GTX_OK, so a failing push leaves the stream as it was.
//
// The steps, a kernel each, over wavefronts that take every `step`-th tile; none waits for another workgroup; atomics only for the
// `fail` maximum and the clash bit, both free of order (the kept records are counted per wavefront of classify into kept_partial and
// summed by finish: one add per wavefront on one device word was most of classify's time at a million records).  Every array index is below the array's stated size whatever
// the records hold: the steps behind classify return at once when `fail` is set (a read longer than its row is never loaded).
//   classify    an element per lane (the parked mates, then the records): sort keys, defaults of the pairing arrays; a record's checks
//               and kept bit.
//   (scan)      prev_scan = inclusive max over kept_in (record i: i + 1 if kept, else 0): the previous kept record of i is
//               prev_scan[i - 1] - 1, and 0 stands for the record the stream carries.
//   compare     eight lanes per record: the fields, then the two rows in 16-byte pieces (bytes where a piece is cut by the read's end
//               or the rows are not 16-byte aligned) -> head, head_in.
//   (scans)     task = exclusive sum of head; head_of = inclusive max of head_in.
//   emit_tasks  eight lanes per record: rec meta of every kept record; plane row (whole 16-byte groups) and meta of every head.
//   (sorts)     the elements stably by name_id, then by rg (gather_rg makes the second sort's keys).
//   walk        a lane per sorted position; the lane of a key's first position runs the key's two-state machine.
//   (scans)     emit_at = exclusive sum of emit (records), wait_at = exclusive sum of wait (elements).
//   emit_items  an element per lane: its item, or its entry of the next parked table.
//   finish      one wavefront: the status, the counts, the next carried record.
//
// Written against the wave policy of graph_dev.hpp: gtx_dstream.hip instantiates it with the hardware wave, tests/emu_dstream with a
// sequential wave under AddressSanitizer / UBSan over heap blocks of exactly the sizes.
#pragma once
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"

namespace gtx
{
// the previous kept record and the stream's counters (device memory, two slots)
struct DstreamCarry
{
  uint32_t have; // a record has been kept
  int32_t tid, pos;
  uint32_t l_qseq;
  uint32_t align_index, fo; // of its head
  uint32_t next_align_index;
  uint32_t reserved;
  uint64_t n_records, n_duplicated;
};
static_assert(sizeof(DstreamCarry) == 48, "layout");

// a mate that waits
struct DstreamParked
{
  uint64_t name_id;
  gtx_rec_meta meta;
  uint32_t sample, rg;
};
static_assert(sizeof(DstreamParked) == 32, "layout");

// what the steps of one push count in (zeroed in front of classify)
struct DstreamWork
{
  uint32_t fail;   // 0, or 0xFFFFFFFF - (4 * record + check) of the first failing check
  uint32_t clash;
  uint32_t reserved[2];
};

enum : uint32_t { DSTREAM_FAIL_RG = 1, DSTREAM_FAIL_LONG = 2, DSTREAM_FAIL_ROW = 3, DSTREAM_FAIL_CLASH = 4, DSTREAM_FAIL_PARKED = 5 };

// the one download of a push
struct DstreamOut
{
  uint32_t status; // GTX_*
  uint32_t why;    // DSTREAM_FAIL_*
  uint32_t record; // why <= DSTREAM_FAIL_ROW: the record
  uint32_t l_qseq; // and its length
  uint32_t n_align, n_items, n_parked, reserved;
  uint64_t n_records, n_duplicated;
};
static_assert(sizeof(DstreamOut) == 48, "layout");

// one push: P = n_parked elements in front of the n records, total = P + n
struct DstreamPush
{
  gtx_stream_record const * recs;
  uint8_t const * seq;
  uint32_t seq_stride, n;
  uint32_t flag_filter, force_both, max_read_len, n_read_groups;
  uint32_t plane_stride, parked_cap, n_parked, row_cap; // row_cap: bytes of a carried row (a multiple of 16)
  // the state and the slot beside it
  DstreamCarry const * carry;
  uint8_t const * carry_row;
  DstreamParked const * parked;
  DstreamCarry * next_carry;
  uint8_t * next_carry_row;
  DstreamParked * next_parked; // parked_cap
  // workspace
  DstreamWork * work;
  uint32_t * kept_partial; // [n_partial]: the kept records each wavefront of classify saw
  uint32_t n_partial;      // classify runs on exactly that many wavefronts
  uint64_t * name;                                          // [total]
  uint32_t *rg, *elem, *wait, *wait_at;                     // [total]; elem: 0 .. total - 1
  uint32_t *kept_in, *prev_scan, *head, *head_in, *task, *head_of, *emit, *emit_at, *partner; // [n]
  gtx_rec_meta * me;                                        // [n]
  uint32_t const * perm;                                    // [total]: the elements sorted
  // outputs
  uint8_t * planes;
  gtx_read_meta * meta;
  gtx_score_item * items;
  DstreamOut * out;
};

namespace dstream_dev
{
GTX_HDI uint32_t nib_bytes(uint32_t l_qseq) { return (l_qseq + 1u) / 2u; }

GTX_DEV uint32_t forward_only(gtx_stream_record const & r, uint32_t force_both)
{
  bool const one = (r.flag & 1u) == 0u || (r.tid == r.mtid && r.isize > -1200 && r.isize < 1200 && (((r.flag & 16u) != 0u) != ((r.flag & 32u) != 0u)));
  return one && !force_both ? GTX_FLAG_FORWARD_ONLY : 0u;
}

GTX_DEV bool aligned16(void const * p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the rows may be loaded in 16-byte pieces: every row and the carried one begin at a multiple of 16
GTX_DEV bool rows_vector(DstreamPush const & a) { return aligned16(a.seq) && (a.seq_stride & 15u) == 0 && aligned16(a.carry_row); }

GTX_DEV bool differ16(uint8_t const * x, uint8_t const * y)
{
  uint4_t const u = *reinterpret_cast<uint4_t const *>(x), v = *reinterpret_cast<uint4_t const *>(y);
  return ((u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w)) != 0;
}

GTX_DEV uint64_t key_name(DstreamPush const & a, uint32_t e) { return a.name[e]; }
GTX_DEV bool same_key(DstreamPush const & a, uint32_t x, uint32_t y) { return a.name[x] == a.name[y] && a.rg[x] == a.rg[y]; }
} // namespace dstream_dev

template <class W>
GTX_DEV bool dstream_failed(DstreamPush const & a)
{
  return W::uni(a.work->fail) != 0;
}

// classify.  A wavefront's tiles of 64 elements: `first`, then every `step`-th behind it (in every step below as well).
template <class W>
GTX_DEV void dstream_classify_wave(DstreamPush const & a, uint32_t first, uint32_t step)
{
  uint32_t const total = a.n_parked + a.n;
  uint32_t kept_seen = 0;
  for (uint64_t t = first; t * 64u < total; t += step)
  {
    typename W::template PerLane<uint32_t> k;
    W::lanes([&](uint32_t l)
    {
      k[l] = 0;
      uint64_t const e64 = t * 64u + l;
      if (e64 >= total)
        return;
      uint32_t const e = static_cast<uint32_t>(e64);
      a.elem[e] = e;
      a.wait[e] = 0;
      if (e < a.n_parked)
      {
        a.name[e] = a.parked[e].name_id;
        a.rg[e] = a.parked[e].rg;
        return;
      }
      uint32_t const i = e - a.n_parked;
      gtx_stream_record const & r = a.recs[i];
      a.name[e] = r.name_id;
      a.rg[e] = r.rg;
      a.emit[i] = 0;
      a.partner[i] = GTX_INVALID_ID;
      uint32_t const len = r.l_qseq;
      uint32_t check = 0;
      if (r.rg >= a.n_read_groups)
        check = DSTREAM_FAIL_RG;
      else if (len > a.max_read_len)
        check = DSTREAM_FAIL_LONG;
      else if (dstream_dev::nib_bytes(len) > a.seq_stride || len > 2u * a.plane_stride)
        check = DSTREAM_FAIL_ROW;
      if (check)
        W::atomic_max_u32(&a.work->fail, 0xFFFFFFFFu - (4u * i + check));
      bool const kept = (r.flag & a.flag_filter) == 0;
      a.kept_in[i] = kept ? i + 1u : 0u;
      k[l] = kept ? 1u : 0u;
    });
    kept_seen += W::sum(k);
  }
  if (first < a.n_partial)
    W::lanes([&](uint32_t l)
    {
      if (l == 0)
        a.kept_partial[first] = kept_seen;
    });
}

// compare, behind the scan of kept_in.  Tiles of 8 records, 8 lanes each.
template <class W>
GTX_DEV void dstream_compare_wave(DstreamPush const & a, uint32_t first, uint32_t step)
{
  using namespace dstream_dev;
  if (dstream_failed<W>(a))
    return;
  bool const vector = rows_vector(a);
  for (uint64_t t = first; t * 8u < a.n; t += step)
  {
    // what the rows decide: 0 nothing (not kept, no record; or the fields decided: a head), 1 the rows are compared
    typename W::template PerLane<uint32_t> bytes, is_head;
    typename W::template PerLane<uint8_t const *> mine, other;
    typename W::template PerLane<bool> differ;
    W::lanes([&](uint32_t l)
    {
      bytes[l] = 0;
      is_head[l] = 0;
      mine[l] = other[l] = nullptr;
      differ[l] = false;
      uint64_t const i64 = t * 8u + (l >> 3);
      if (i64 >= a.n || a.kept_in[i64] == 0)
        return;
      uint32_t const i = static_cast<uint32_t>(i64);
      gtx_stream_record const & r = a.recs[i];
      uint32_t const before = i ? a.prev_scan[i - 1u] : 0u;
      bool same;
      uint8_t const * row;
      if (before == 0)
      {
        same = a.carry->have != 0 && r.tid == a.carry->tid && r.pos == a.carry->pos && r.l_qseq == a.carry->l_qseq;
        row = a.carry_row;
      }
      else
      {
        gtx_stream_record const & p = a.recs[before - 1u];
        same = r.tid == p.tid && r.pos == p.pos && r.l_qseq == p.l_qseq;
        row = a.seq + static_cast<uint64_t>(before - 1u) * a.seq_stride;
      }
      if (!same)
      {
        is_head[l] = 1;
        return;
      }
      bytes[l] = nib_bytes(r.l_qseq);
      mine[l] = a.seq + static_cast<uint64_t>(i) * a.seq_stride;
      other[l] = row;
    });
    uint32_t const longest = W::max(bytes);
    for (uint32_t at = 0; at < longest; at += 128u)
      W::lanes([&](uint32_t l)
      {
        uint32_t const o = at + 16u * (l & 7u);
        if (o >= bytes[l] || differ[l])
          return;
        uint32_t const end = o + 16u < bytes[l] ? o + 16u : bytes[l];
        if (vector && end - o == 16u)
          differ[l] = differ16(mine[l] + o, other[l] + o);
        else
          for (uint32_t b = o; b < end; ++b)
            if (mine[l][b] != other[l][b])
              differ[l] = true;
      });
    uint64_t const unequal = W::ballot(differ);
    W::lanes([&](uint32_t l)
    {
      uint64_t const i = t * 8u + (l >> 3);
      if ((l & 7u) != 0 || i >= a.n)
        return;
      bool const head = a.kept_in[i] != 0 && (is_head[l] != 0 || ((unequal >> l) & 0xFFu) != 0);
      a.head[i] = head ? 1u : 0u;
      a.head_in[i] = head ? static_cast<uint32_t>(i) + 1u : 0u;
    });
  }
}

// emit_tasks, behind the scans of head and head_in.  Tiles of 8 records, 8 lanes each.
template <class W>
GTX_DEV void dstream_emit_tasks_wave(DstreamPush const & a, uint32_t first, uint32_t step)
{
  using namespace dstream_dev;
  if (dstream_failed<W>(a))
    return;
  bool const vector = rows_vector(a);
  uint32_t const groups = a.plane_stride / PLANE_GROUP_BYTES;
  for (uint64_t t = first; t * 8u < a.n; t += step)
    W::lanes([&](uint32_t l)
    {
      uint64_t const i64 = t * 8u + (l >> 3);
      if (i64 >= a.n || a.kept_in[i64] == 0)
        return;
      uint32_t const i = static_cast<uint32_t>(i64), sub = l & 7u;
      gtx_stream_record const & r = a.recs[i];
      uint32_t const h = a.head_of[i]; // 0: the head is the one the stream carries
      if (sub == 0)
      {
        uint32_t const align_index = h ? a.carry->next_align_index + a.task[h - 1u] : a.carry->align_index;
        uint32_t const fo = h ? forward_only(a.recs[h - 1u], a.force_both) : a.carry->fo;
        a.me[i] = gtx_rec_meta{align_index, static_cast<uint16_t>(r.flag | fo), r.mapq, r.score_diff, r.pos, r.isize};
      }
      if (a.head[i] == 0)
        return;
      uint32_t const k = a.task[i];
      if (sub == 0)
      {
        int32_t const clip = (r.n_cigar != 0 && (r.cigar_front & 15u) == 4u) ? static_cast<int32_t>(r.cigar_front >> 4) : 0;
        a.meta[k] = gtx_read_meta{r.l_qseq, static_cast<uint16_t>(r.flag | forward_only(r, a.force_both)), r.tid, r.mtid, r.isize, r.pos - clip};
      }
      uint8_t const * const row = a.seq + static_cast<uint64_t>(i) * a.seq_stride;
      uint32_t const bytes = nib_bytes(r.l_qseq);
      for (uint32_t g = sub; g < groups; g += 8u)
      {
        uint32_t w[4] = {0, 0, 0, 0};
        if (vector && 16u * g + 16u <= bytes)
        {
          uint4_t const v = *reinterpret_cast<uint4_t const *>(row + 16u * g);
          w[0] = v.x;
          w[1] = v.y;
          w[2] = v.z;
          w[3] = v.w;
        }
        else
        {
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) // (constant indices: w stays in registers)
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
            {
              uint32_t const at = 16u * g + 4u * k + b;
              w[k] |= (at < bytes ? static_cast<uint32_t>(row[at]) : 0u) << (8u * b);
            }
        }
        uint32_t o[4];
        planes_from_nibble_words(w, o);
        *reinterpret_cast<uint4_t *>(a.planes + static_cast<uint64_t>(k) * a.plane_stride + 16u * g) = uint4_t{o[0], o[1], o[2], o[3]};
      }
    });
}

// the keys of the second sort: the read groups in the order the first sort left (by_name: the elements sorted by name_id)
template <class W>
GTX_DEV void dstream_gather_rg_wave(DstreamPush const & a, uint32_t const * by_name, uint32_t * keys, uint32_t first, uint32_t step)
{
  uint32_t const total = a.n_parked + a.n;
  for (uint64_t t = first; t * 64u < total; t += step)
    W::lanes([&](uint32_t l)
    {
      uint64_t const s = t * 64u + l;
      if (s < total)
      {
        uint32_t const e = by_name[s];
        keys[s] = e < total ? a.rg[e] : 0u;
      }
    });
}

// walk, behind the sorts.  A lane per sorted position.
template <class W>
GTX_DEV void dstream_walk_wave(DstreamPush const & a, uint32_t first, uint32_t step)
{
  using namespace dstream_dev;
  if (dstream_failed<W>(a))
    return;
  uint32_t const total = a.n_parked + a.n, P = a.n_parked;
  for (uint64_t t = first; t * 64u < total; t += step)
    W::lanes([&](uint32_t l)
    {
      uint64_t const s64 = t * 64u + l;
      if (s64 >= total)
        return;
      uint32_t const s = static_cast<uint32_t>(s64), e = a.perm[s];
      if (e >= total || (s != 0 && a.perm[s - 1u] < total && same_key(a, a.perm[s - 1u], e)))
        return;
      // the key's first position: its occurrences in stream order
      uint32_t waiting = GTX_INVALID_ID, waiting_flag = 0;
      for (uint32_t p = s; p < total; ++p)
      {
        uint32_t const x = a.perm[p];
        if (x >= total || (p != s && !same_key(a, e, x)))
          break;
        if (x >= P && a.kept_in[x - P] == 0)
          continue;
        uint32_t const flag = x < P ? a.parked[x].meta.flag : a.recs[x - P].flag;
        if (waiting == GTX_INVALID_ID)
        {
          if (flag & 1u)
          {
            waiting = x;
            waiting_flag = flag;
          }
          else if (x >= P)
            a.emit[x - P] = 1;
          continue;
        }
        if (x < P) // (two parked mates of one key: the table never holds that)
          continue;
        if ((waiting_flag & 64u) == (flag & 64u))
          W::atomic_max_u32(&a.work->clash, 1u);
        a.emit[x - P] = 1;
        a.partner[x - P] = waiting;
        waiting = GTX_INVALID_ID;
      }
      if (waiting != GTX_INVALID_ID)
        a.wait[waiting] = 1;
    });
}

// emit_items, behind the scans of emit and wait.  An element per lane.
template <class W>
GTX_DEV void dstream_emit_items_wave(DstreamPush const & a, uint32_t first, uint32_t step)
{
  if (dstream_failed<W>(a))
    return;
  uint32_t const total = a.n_parked + a.n, P = a.n_parked;
  for (uint64_t t = first; t * 64u < total; t += step)
    W::lanes([&](uint32_t l)
    {
      uint64_t const e64 = t * 64u + l;
      if (e64 >= total)
        return;
      uint32_t const e = static_cast<uint32_t>(e64);
      if (a.wait[e] && a.wait_at[e] < a.parked_cap)
      {
        DstreamParked & to = a.next_parked[a.wait_at[e]]; // (field by field: a local aggregate here is promoted to LDS)
        if (e < P)
          to = a.parked[e];
        else
        {
          to.name_id = a.name[e];
          to.meta = a.me[e - P];
          to.sample = a.recs[e - P].sample;
          to.rg = a.rg[e];
        }
      }
      if (e < P || a.emit[e - P] == 0)
        return;
      uint32_t const i = e - P, w = a.partner[i];
      gtx_score_item & item = a.items[a.emit_at[i]];
      if (w == GTX_INVALID_ID)
      {
        item.first = a.me[i];
        item.second.align_index = GTX_INVALID_ID;
        item.second.flag = 0;
        item.second.mapq = item.second.score_diff = 0;
        item.second.pos = item.second.isize = 0;
      }
      else
      {
        item.first = w < P ? a.parked[w].meta : a.me[w - P];
        item.second = a.me[i];
      }
      item.sample = a.recs[i].sample;
      item.kind = 0;
    });
}

// finish, one wavefront: the status, the download, the next carried record and counters
template <class W>
GTX_DEV void dstream_finish_wave(DstreamPush const & a)
{
  using namespace dstream_dev;
  uint32_t const total = a.n_parked + a.n, fail = W::uni(a.work->fail);
  DstreamOut out{};
  out.n_parked = a.n_parked;
  out.n_records = W::uni(static_cast<uint64_t>(a.carry->n_records));
  out.n_duplicated = W::uni(static_cast<uint64_t>(a.carry->n_duplicated));
  uint32_t last = 0; // the push's last kept record + 1
  if (fail != 0)
  {
    uint32_t const word = 0xFFFFFFFFu - fail;
    out.why = word & 3u;
    out.record = word >> 2;
    out.l_qseq = out.record < a.n ? W::uni(static_cast<uint32_t>(a.recs[out.record].l_qseq)) : 0u;
    out.status = out.why == DSTREAM_FAIL_LONG ? GTX_ERR_UNSUPPORTED : GTX_ERR_ARG;
  }
  else
  {
    uint32_t const n_align = a.n ? W::uni(a.task[a.n - 1u] + a.head[a.n - 1u]) : 0u, n_items = a.n ? W::uni(a.emit_at[a.n - 1u] + a.emit[a.n - 1u]) : 0u;
    uint32_t const n_wait = total ? W::uni(a.wait_at[total - 1u] + a.wait[total - 1u]) : 0u;
    uint32_t n_kept = 0;
    for (uint32_t at = 0; at < a.n_partial; at += 64u)
    {
      typename W::template PerLane<uint32_t> part;
      W::lanes([&](uint32_t l) { part[l] = at + l < a.n_partial ? a.kept_partial[at + l] : 0u; });
      n_kept += W::sum(part);
    }
    if (W::uni(a.work->clash) != 0)
    {
      out.status = GTX_ERR_ARG;
      out.why = DSTREAM_FAIL_CLASH;
    }
    else if (n_wait > a.parked_cap)
    {
      out.status = GTX_ERR_CAPACITY;
      out.why = DSTREAM_FAIL_PARKED;
      out.n_parked = n_wait;
    }
    else
    {
      out.n_align = n_align;
      out.n_items = n_items;
      out.n_parked = n_wait;
      out.n_records += n_kept;
      out.n_duplicated += n_kept - n_align;
      last = a.n ? W::uni(a.prev_scan[a.n - 1u]) : 0u;
    }
  }
  // the carried record: the push's last kept one with its head's index and bit, else the one carried so far
  DstreamCarry next = *a.carry;
  uint8_t const * row = a.carry_row;
  uint32_t bytes = a.row_cap;
  if (last != 0)
  {
    gtx_stream_record const & r = a.recs[last - 1u];
    next.have = 1;
    next.tid = W::uni(r.tid);
    next.pos = W::uni(r.pos);
    next.l_qseq = W::uni(static_cast<uint32_t>(r.l_qseq));
    next.align_index = W::uni(a.me[last - 1u].align_index);
    next.fo = W::uni(static_cast<uint32_t>(a.me[last - 1u].flag)) & GTX_FLAG_FORWARD_ONLY;
    row = a.seq + static_cast<uint64_t>(last - 1u) * a.seq_stride;
    bytes = nib_bytes(next.l_qseq);
    bytes = bytes < a.row_cap ? bytes : a.row_cap;
  }
  next.next_align_index += out.n_align;
  next.n_records = out.n_records;
  next.n_duplicated = out.n_duplicated;
  for (uint32_t at = 0; at < a.row_cap; at += 64u)
    W::lanes([&](uint32_t l)
    {
      uint32_t const b = at + l;
      if (b < a.row_cap)
        a.next_carry_row[b] = b < bytes ? row[b] : 0;
    });
  W::lanes([&](uint32_t l)
  {
    if (l == 0)
    {
      *a.next_carry = next;
      *a.out = out;
    }
  });
}
} // namespace gtx
