// gtx_disc_rounds_dev.hpp -- discovery's second pass from the aligner on (realign_to_indels, src/typer/caller.cpp:1876-2229),
// kernel source: the window of every (read, entry) pair of a round with the indels applied (apply_indel_event,
// src/typer/event.cpp:293-396, as gtx_realign.hip restates it), what becomes of every pair (:2025-2153), the reads' lists and the
// support counters (Alignment::add_indel_event / replace_indel_events, src/typer/read.cpp:29-116), and the good-support decision at
// the end (:2179-2229 with EventSupport::is_good_indel, src/typer/event.cpp:273-291).  The alignments between the windows and the
// decision are gtx_realign_dev.hpp's, untouched.  All values are integers but the two doubles of the final decision.
//
// A round -- one list entry k -- is a fixed number of launches; within it the reads are independent (a read is in a round's pairs
// at most once), rounds run in list order.  Slot 0 of a round is its plain window (entry k applied alone), slot j + 1 is pair j's
// own window when its read has entries; slot s owns `ub[s]` letters of the arena at woff[s] (the plain window's length plus every
// insertion that could be applied -- an upper bound, so that no build can run out of its slot), of which wlen[s] are the window.
// The aligner sees target 2 * s at [woff[s], woff[s] + wlen[s]) (the odd targets are the slots' unused tails and are named by nobody).
//
// THE COUNTERS.  A call is per file and starts from zeros (EventSupport::clear() and the asserts of :2920-2924).  Under that start
// hq_count, sequence_reversed and proper_pairs of an entry equal the number of reads that hold the entry with read_pos >= 0 (and
// have the flag) AT THAT MOMENT: add_indel_event and the second loop of replace_indel_events add one per new holder, the first loop
// of replace_indel_events takes one per holder that lets go, and a holder that lets go was counted when it took hold.  So the floors
// of read.cpp:76,83 never act, no counter is ever below zero, and plain atomic add, subtract and max give the same totals in any
// order.  max_mapq only grows.  (tests/disc_rounds_cases.py checks the holders' equation after every round.)  The counters are 32
// bits wide here; the reference's are uint16_t, and the final decision reads them through that width.
//
// WHERE THE LISTS LIVE.  In the caller's gtx_disc_second_event array: a round's new lists go behind the entries in use, at the
// exclusive sum of their sizes in pair order -- no atomic bump, so the array is a function of the inputs.  The lists a read left
// behind stay where they were until a compaction (in stream order) takes them out.
//
// Written against the wave policy of graph_dev.hpp, as gtx_disc_second_dev.hpp is; gtx_disc_rounds.hip instantiates it with the
// hardware wave, tests/emu_disc_rounds with a sequential wave.  W::mem_sync() orders a wave's stores in front of its later loads.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_disc_second_dev.hpp"
#include "gtx_realign_dev.hpp"

#if defined(__HIPCC__)
#define GTX_HD __host__ __device__ inline
#else
#define GTX_HD inline
#endif

namespace gtx
{
constexpr uint16_t IS_SEQ_REVERSED = 16, IS_PROPER_PAIR = 2; // include/graphtyper/constants.hpp.in
constexpr int32_t READ_MULTI_SUPPORT = -2;                  // read.hpp:16

// ctl[]: what the host reads of a round
enum : uint32_t
{
  ROUNDS_N_PAIRS = 0,   // the round's pairs
  ROUNDS_NEED_UPPER,    // entries the round's new lists hold at most
  ROUNDS_LETTERS_LO,    // the slots' letters, 64 bits
  ROUNDS_LETTERS_HI,
  ROUNDS_SKIPPED,       // 1: entry k did not apply (:1905)
  ROUNDS_ALIGNED,
  ROUNDS_REFUSED,
  ROUNDS_WINDOWS,       // windows built (the plain one included)
  ROUNDS_BAD_LIST,      // a read whose entries lie behind the array's count
  ROUNDS_CTL_WORDS
};

struct RoundDecision
{
  int32_t pos, pos_end, score;
  int16_t num_clipped_begin, num_clipped_end, num_ins_begin;
  uint16_t outcome; // GTX_REALIGN_*; NO_PADDING also for a pair that was not aligned
};

struct RoundsIn
{
  // the file
  char const * refc;
  long REF_SIZE, region_begin;
  gtx_disc_indel const * table;
  char const * table_seq;
  uint32_t n_table;
  uint64_t n_table_seq;
  uint32_t const * list;
  uint32_t k;
  uint32_t const * max_read_size;
  gtx_disc_second_read * reads;
  uint32_t n_reads;
  gtx_disc_second_event * events;
  uint32_t n_events; // entries in use
  gtx_disc_second_support * support;
  // the round
  gtx_disc_second_pair const * pairs;
  uint32_t const * counts; // counts[0]: the pairs
  uint32_t *ub, *woff, *wlen, *target_off; // n_reads + 2, n_reads + 2, n_reads + 1, 2 * (n_reads + 1) + 1
  RealignPair * rpairs;
  RealignResult const * results;
  uint8_t * seq;
  int32_t * refpos;
  uint8_t * applied; // per entry of the event array: the windows kernel applied it
  RoundDecision * decisions;
  uint32_t *newn, *noff; // n_reads + 1
  uint32_t * ctl;
};

namespace disc_rounds_dev
{
using disc_second_dev::PAD;

struct Plain
{
  long begin, end; // offsets in the region; begin == end: the window lies outside the region and entry k cannot apply
};

// :1890-1896
GTX_DEV Plain plain_window(long pos, long max_read_size, long region_begin, long REF_SIZE)
{
  long const begin = std::max(0l, pos - max_read_size - 2 * PAD - region_begin), end_padded = pos + max_read_size + 2 * PAD - region_begin;
  long end = end_padded >= REF_SIZE ? REF_SIZE : end_padded;
  if (end < begin) // (:1891 asserts otherwise; a window that begins at or behind the region's end has end == REF_SIZE <= begin)
    end = begin;
  return Plain{begin, end};
}

GTX_DEV uint32_t n_pairs_of(RoundsIn const & in) { return std::min(in.counts[0], in.n_reads); }

// apply_indel_event (event.cpp:293-396) over a window in global memory, by one wavefront: the tests are wave-uniform, the erase
// and the insert are shifted copies, 64 entries a step, every step's loads in front of its stores.  `room`: the slot's size.
template <class W>
GTX_DEV bool apply_event(uint8_t * seq, int32_t * rp, uint32_t & n, uint32_t room, gtx_disc_indel const & ev, char const * table_seq, uint64_t n_table_seq,
                         long offset)
{
  long const ref_pos = static_cast<long>(ev.pos) - offset;
  if (ref_pos <= 0)
    return false;
  long pos = ref_pos; // start the search for the reference position here
  long const event_size = ev.len, seq_size = n;
  if (pos >= seq_size)
    return false;
  if (rp[pos] != ref_pos)
  {
    while (pos + 1 < seq_size && rp[pos] < ref_pos)
      ++pos;
    while (pos > 0 && rp[pos] > ref_pos)
      --pos;
    if (rp[pos] != ref_pos)
      return false;
  }
  { // purity (:330-356)
    long const begin = std::max(0l, pos - 3), end = std::min(seq_size, pos + 3);
    long prev = rp[begin];
    for (long p = begin + 1; p < end; ++p)
    {
      if (rp[p] != prev + 1)
        return false;
      ++prev;
    }
  }
  if (ev.type == 'D')
  {
    if (pos + event_size >= seq_size || rp[pos + event_size] != ref_pos + event_size)
      return false;
    for (long base = pos; base + event_size < seq_size; base += 64)
    {
      typename W::template PerLane<uint32_t> letter, value;
      W::lanes([&](uint32_t l) {
        long const from = base + l + event_size;
        if (from < seq_size)
        {
          letter[l] = seq[from];
          value[l] = static_cast<uint32_t>(rp[from]);
        }
      });
      W::mem_sync();
      W::lanes([&](uint32_t l) {
        if (base + l + event_size < seq_size)
        {
          seq[base + l] = static_cast<uint8_t>(letter[l]);
          rp[base + l] = static_cast<int32_t>(value[l]);
        }
      });
      W::mem_sync();
    }
    n = static_cast<uint32_t>(seq_size - event_size);
    return true;
  }
  if (ev.type == 'I')
  {
    // (never taken for a slot sized by rounds_prepare and a table whose letters are there: a store may not leave the slot)
    if (seq_size + event_size > static_cast<long>(room) || static_cast<uint64_t>(ev.seq_off) + ev.len > n_table_seq)
      return false;
    // letters [pos, n) and positions [pos + 1, n) move up by event_size, from the top
    for (long top = seq_size; top > pos; top -= 64)
    {
      typename W::template PerLane<uint32_t> letter, value;
      W::lanes([&](uint32_t l) {
        long const from = top - 1 - l;
        if (from >= pos)
        {
          letter[l] = seq[from];
          value[l] = static_cast<uint32_t>(rp[from]);
        }
      });
      W::mem_sync();
      W::lanes([&](uint32_t l) {
        long const from = top - 1 - l;
        if (from >= pos)
          seq[from + event_size] = static_cast<uint8_t>(letter[l]);
        if (from >= pos + 1)
          rp[from + event_size] = static_cast<int32_t>(value[l]);
      });
      W::mem_sync();
    }
    for (long base = 0; base < event_size; base += 64)
      W::lanes([&](uint32_t l) {
        if (base + l < event_size)
        {
          seq[pos + base + l] = static_cast<uint8_t>(table_seq[ev.seq_off + base + l]);
          rp[pos + 1 + base + l] = static_cast<int32_t>(pos + 1); // (:385-386: the index, as the text has it)
        }
      });
    W::mem_sync();
    n = static_cast<uint32_t>(seq_size + event_size);
    return true;
  }
  return false;
}
} // namespace disc_rounds_dev

// at the front of a call, lane i of n_reads: the read's length for the aligner; a list that is not inside the array
GTX_DEV void rounds_begin(uint32_t i, gtx_disc_second_read const * reads, uint32_t n_reads, uint32_t n_events, uint16_t * lens, uint32_t * ctl)
{
  if (i >= n_reads)
    return;
  gtx_disc_second_read const r = reads[i];
  lens[i] = r.l_qseq;
  if (r.n_events != 0 && static_cast<uint64_t>(r.first_event) + r.n_events > n_events)
    ctl[ROUNDS_BAD_LIST] = 1;
}

// Lane i of n_reads + 2: the size of slot i (0: the plain window; j + 1: pair j; behind the pairs: 0) and the round's totals.
// ctl[] is zero at entry but for ROUNDS_BAD_LIST.
template <class W>
GTX_DEV void rounds_prepare(RoundsIn const & in, uint32_t i)
{
  using namespace disc_rounds_dev;
  if (i >= in.n_reads + 2)
    return;
  uint32_t const n_pairs = n_pairs_of(in), entry = in.list[in.k];
  uint64_t size = 0;
  if (entry < in.n_table && i <= n_pairs)
  {
    gtx_disc_indel const indel = in.table[entry];
    Plain const w = plain_window(indel.pos, *in.max_read_size, in.region_begin, in.REF_SIZE);
    uint64_t const plain = static_cast<uint64_t>(w.end - w.begin) + (indel.type == 'I' ? indel.len : 0u);
    if (i == 0)
      size = plain;
    else
    {
      gtx_disc_second_read const r = in.reads[in.pairs[i - 1].read];
      if (r.n_events != 0)
      {
        size = plain;
        for (uint32_t e = 0; e < r.n_events; ++e)
        {
          uint32_t const t = in.events[r.first_event + e].indel;
          if (t < in.n_table && in.table[t].type == 'I')
            size += in.table[t].len;
        }
      }
      W::atomic_add_u32(in.ctl + ROUNDS_NEED_UPPER, r.n_events + 1u);
    }
  }
  in.ub[i] = static_cast<uint32_t>(std::min<uint64_t>(size, 0x7FFFFFFFu)); // (the host refuses a round of 2^31 letters and more: the sum below says so)
  if (size)
    W::atomic_add_u64(reinterpret_cast<unsigned long long *>(in.ctl + ROUNDS_LETTERS_LO), size);
  if (i == 0)
    in.ctl[ROUNDS_N_PAIRS] = n_pairs;
}

// One wavefront per slot: the window, its ref_pos values, the applied flag of every entry of the read, what the aligner takes.
template <class W>
GTX_DEV void rounds_window_wave(RoundsIn const & in, uint32_t slot)
{
  using namespace disc_rounds_dev;
  uint32_t const n_pairs = n_pairs_of(in), entry = in.list[in.k];
  if (slot > n_pairs)
    return;
  uint32_t const at = in.woff[slot], room = in.ub[slot];
  uint32_t n = 0;
  gtx_disc_second_read r{};
  if (slot != 0)
    r = in.reads[in.pairs[slot - 1].read];
  bool const build = slot == 0 || r.n_events != 0;
  bool k_applied = false;
  if (build && entry < in.n_table)
  {
    gtx_disc_indel const indel = in.table[entry];
    Plain const w = plain_window(indel.pos, *in.max_read_size, in.region_begin, in.REF_SIZE);
    uint8_t * const seq = in.seq + at;
    int32_t * const rp = in.refpos + at;
    n = static_cast<uint32_t>(std::min<long>(w.end - w.begin, room));
    for (uint32_t base = 0; base < n; base += 64)
      W::lanes([&](uint32_t l) {
        if (base + l < n)
        {
          seq[base + l] = static_cast<uint8_t>(in.refc[w.begin + base + l]);
          rp[base + l] = static_cast<int32_t>(base + l);
        }
      });
    W::mem_sync();
    long const offset = w.begin + in.region_begin;
    k_applied = apply_event<W>(seq, rp, n, room, indel, in.table_seq, in.n_table_seq, offset); // :1902-1906
    for (uint32_t e = 0; e < r.n_events; ++e) // :1968-2002: every entry of the read in list order, whatever its read_pos
    {
      uint32_t const t = in.events[r.first_event + e].indel;
      bool const ok = k_applied && t < in.n_table && apply_event<W>(seq, rp, n, room, in.table[t], in.table_seq, in.n_table_seq, offset);
      if (W::leader())
        in.applied[r.first_event + e] = ok ? 1 : 0;
    }
  }
  if (W::leader())
  {
    in.wlen[slot] = n;
    in.target_off[2 * slot] = at;
    in.target_off[2 * slot + 1] = at + n;
    if (slot == 0)
    {
      in.target_off[2 * (n_pairs + 1)] = in.woff[n_pairs + 1];
      in.ctl[ROUNDS_SKIPPED] = k_applied ? 0 : 1;
    }
    else
      in.rpairs[slot - 1] = RealignPair{in.pairs[slot - 1].read, build ? 2 * slot : 0u};
    if (build && (slot == 0 || k_applied)) // (a skipped round counts its plain window alone)
      W::atomic_add_u32(in.ctl + ROUNDS_WINDOWS, 1u);
  }
}

// Lane j of n_reads + 1: what becomes of pair j (:2025-2153, as gtx_disc_realign_decide has it) and the size of its read's new
// list; nothing is changed yet.  Behind the pairs: newn = 0.
template <class W>
GTX_DEV void rounds_decide(RoundsIn const & in, uint32_t j)
{
  if (j > in.n_reads)
    return;
  uint32_t const n_pairs = disc_rounds_dev::n_pairs_of(in);
  uint32_t newn = 0;
  if (j < n_pairs && in.ctl[ROUNDS_SKIPPED] == 0)
  {
    gtx_disc_second_read const r = in.reads[in.pairs[j].read];
    RealignResult const res = in.results[j];
    RoundDecision d{0, 0, 0, 0, 0, 0, static_cast<uint16_t>(GTX_REALIGN_NO_PADDING)};
    if (res.status != REALIGN_OK)
      W::atomic_add_u32(in.ctl + ROUNDS_REFUSED, 1u); // the stated limit: such a pair is not aligned in this round
    else
    {
      W::atomic_add_u32(in.ctl + ROUNDS_ALIGNED, 1u);
      uint32_t const slot = r.n_events != 0 ? j + 1 : 0;
      int32_t const * const rp = in.refpos + in.woff[slot];
      long const n = in.wlen[slot], db = res.target_begin, de = res.target_end;
      gtx_disc_indel const indel = in.table[in.list[in.k]];
      disc_rounds_dev::Plain const w = disc_rounds_dev::plain_window(indel.pos, *in.max_read_size, in.region_begin, in.REF_SIZE);
      long const begin_padded = w.begin, indel_pos = indel.pos, old_score = r.score;
      if (db == 0 || de >= n) // :2025
        ;
      else if (res.score <= old_score) // :2066
      {
        if (res.score < old_score)
          d.outcome = GTX_REALIGN_WORSE; // :2084
        else if (indel_pos >= rp[db] + begin_padded && indel_pos <= rp[de] + begin_padded) // :2086-2087
          d.outcome = GTX_REALIGN_SAME_OVERLAPPING;
        else
          d.outcome = GTX_REALIGN_SAME;
      }
      else
      {
        d.outcome = GTX_REALIGN_BETTER;
        d.pos = static_cast<int32_t>(static_cast<uint32_t>(rp[db] + in.region_begin + begin_padded));     // :2136
        d.pos_end = static_cast<int32_t>(static_cast<uint32_t>(rp[de] + in.region_begin + begin_padded)); // :2137
        d.score = res.score;                                                                               // :2138
        d.num_clipped_begin = static_cast<int16_t>(res.clip_begin);                                        // :2139
        d.num_clipped_end = static_cast<int16_t>(static_cast<uint16_t>(static_cast<long>(r.l_qseq) - res.clip_end)); // :2140
        long num_ins = 0; // :2143-2153
        while (db + num_ins + 1 < n && rp[db + num_ins] == rp[db + num_ins + 1])
          ++num_ins;
        d.num_ins_begin = static_cast<int16_t>(static_cast<uint16_t>(num_ins));
      }
    }
    in.decisions[j] = d;
    if (d.outcome == GTX_REALIGN_BETTER || d.outcome == GTX_REALIGN_WORSE || d.outcome == GTX_REALIGN_SAME_OVERLAPPING)
      newn = r.n_events + 1u;
  }
  in.newn[j] = newn;
}

namespace disc_rounds_dev
{
// one entry of a list enters (+1) or leaves (-1) the counters (read.cpp:31-52, :62-86, :92-112)
template <class W>
GTX_DEV void count_entry(gtx_disc_second_support * support, uint32_t n_table, gtx_disc_second_event const & ev, uint16_t flags, uint8_t mapq, bool enters)
{
  if (ev.indel >= n_table)
    return;
  gtx_disc_second_support & s = support[ev.indel];
  auto move = [&](uint32_t * p) { enters ? W::atomic_add_u32(p, 1u) : W::atomic_sub_u32(p, 1u); };
  if (ev.read_pos == disc_second_dev::READ_ANTI_SUPPORT)
    move(&s.anti_count);
  else if (ev.read_pos == READ_MULTI_SUPPORT)
    move(&s.multi_count);
  else
  {
    move(&s.hq_count);
    if ((flags & IS_SEQ_REVERSED) != 0u)
      move(&s.sequence_reversed);
    if ((flags & IS_PROPER_PAIR) != 0u)
      move(&s.proper_pairs);
    if (enters && mapq < 255)
      W::atomic_max_u32(&s.max_mapq, mapq);
  }
}
} // namespace disc_rounds_dev

// Lane j of the pairs: pair j's outcome is carried out.  The read's new list goes to events[base + noff[j]].
template <class W>
GTX_DEV void rounds_apply(RoundsIn const & in, uint32_t j, uint32_t base, uint32_t event_cap)
{
  using namespace disc_rounds_dev;
  if (j >= n_pairs_of(in) || in.newn[j] == 0)
    return;
  uint32_t const read = in.pairs[j].read, entry = in.list[in.k];
  gtx_disc_second_read r = in.reads[read];
  RoundDecision const d = in.decisions[j];
  uint64_t const first = static_cast<uint64_t>(base) + in.noff[j];
  if (first + in.newn[j] > event_cap) // (the host has checked the round's total)
    return;
  gtx_disc_second_event * const to = in.events + first;
  gtx_disc_second_event const * const old = in.events + r.first_event;
  if (d.outcome == GTX_REALIGN_BETTER) // replace_indel_events (read.cpp:57-116) with the applied_events of :1965-2002
  {
    for (uint32_t e = 0; e < r.n_events; ++e)
      count_entry<W>(in.support, in.n_table, old[e], r.flags, r.mapq, false);
    to[0] = gtx_disc_second_event{entry, 0};
    for (uint32_t e = 0; e < r.n_events; ++e)
      to[1 + e] = gtx_disc_second_event{old[e].indel, in.applied[r.first_event + e] ? 0 : disc_second_dev::READ_ANTI_SUPPORT};
    for (uint32_t e = 0; e <= r.n_events; ++e)
      count_entry<W>(in.support, in.n_table, to[e], r.flags, r.mapq, true);
    r.pos = d.pos;
    r.pos_end = d.pos_end;
    r.score = d.score;
    r.num_clipped_begin = d.num_clipped_begin;
    r.num_clipped_end = d.num_clipped_end;
    r.num_ins_begin = d.num_ins_begin;
  }
  else // add_indel_event (read.cpp:29-55): anti-support (:2084) or multi-support (:2097)
  {
    for (uint32_t e = 0; e < r.n_events; ++e)
      to[e] = old[e];
    to[r.n_events] = gtx_disc_second_event{entry, d.outcome == GTX_REALIGN_WORSE ? disc_second_dev::READ_ANTI_SUPPORT : READ_MULTI_SUPPORT};
    count_entry<W>(in.support, in.n_table, to[r.n_events], r.flags, r.mapq, true);
  }
  r.first_event = static_cast<uint32_t>(first);
  r.n_events = in.newn[j];
  in.reads[read] = r;
}

// The compaction, in stream order: lane i of n_reads copies read i's list to tmp[coff[i]..] (first), then takes its new place (second)
GTX_DEV void rounds_compact_copy(uint32_t i, gtx_disc_second_read const * reads, uint32_t n_reads, gtx_disc_second_event const * events, uint32_t const * coff,
                                 gtx_disc_second_event * tmp, uint32_t cap)
{
  if (i >= n_reads)
    return;
  gtx_disc_second_read const r = reads[i];
  for (uint32_t e = 0; e < r.n_events; ++e)
    if (static_cast<uint64_t>(coff[i]) + e < cap) // (lists that share entries add up to more than the array: the host refuses them behind this)
      tmp[coff[i] + e] = events[r.first_event + e];
}

GTX_DEV void rounds_compact_place(uint32_t i, gtx_disc_second_read * reads, uint32_t n_reads, uint32_t const * coff)
{
  if (i < n_reads)
    reads[i].first_event = reads[i].n_events != 0 ? coff[i] : 0u;
}

// ---- the final decision (:2179-2229) ------------------------------------------------------------------------------------------
// get_log_qual (event.cpp:95-106)
GTX_HD uint32_t disc_log_qual(uint32_t count, uint32_t anti_count, uint32_t eps)
{
  uint32_t const gt00 = count * eps, gt01 = count + anti_count, gt11 = anti_count * eps;
  uint32_t const gt_alt = gt01 < gt11 ? gt01 : gt11;
  return gt00 > gt_alt ? gt00 - gt_alt : 0u;
}

// is_good_count (:2187-2194) of a list entry and its counters.  With hq_count above 6 -- which is_good_indel asks for -- the first
// arm always holds, so disc_second_good never shows the two others; they are a function of their own so that they can be held to
// the text all the same (tests/emu_disc_rounds).
GTX_HD bool disc_second_good_count(gtx_disc_indel const & indel, gtx_disc_second_support const & s)
{
  uint16_t const hq_count = static_cast<uint16_t>(s.hq_count), span = indel.span; // (lq_count is 0 in this pass and left out)
  double const size = static_cast<double>(indel.len);
  double const correction = indel.type == 'I' ? static_cast<double>(size / 2.0 + 8.0) / 8.0 : static_cast<double>(size / 3.0 + 10.0) / 10.0; // :2187-2188
  double const count = correction * hq_count;                                                                                                // :2190
  return (hq_count >= 5 && count >= 5.5) || (span >= 5 && hq_count >= 4 && count >= 5.0) || (span >= 15 && hq_count >= 3 && count >= 4.5);
}

// Does a list entry without good support have it after the file's rounds?  lq_count is 0 in this pass.  The counters are read
// through the reference's uint16_t (max_mapq: uint8_t); the doubles are one operation each, as the text has them.
GTX_HD bool disc_second_good(gtx_disc_indel const & indel, gtx_disc_second_support const & s)
{
  if (!disc_second_good_count(indel, s))
    return false;
  uint16_t const hq_count = static_cast<uint16_t>(s.hq_count), anti_count = static_cast<uint16_t>(s.anti_count),
                 multi_count = static_cast<uint16_t>(s.multi_count), sequence_reversed = static_cast<uint16_t>(s.sequence_reversed),
                 proper_pairs = static_cast<uint16_t>(s.proper_pairs);
  uint8_t const max_mapq = static_cast<uint8_t>(s.max_mapq);
  // EventSupport::is_good_indel(eps = 7)
  long const depth = hq_count + anti_count + multi_count;
  if (hq_count <= 6 || sequence_reversed <= 0 || sequence_reversed >= depth || proper_pairs <= 4 || (hq_count < 10 && max_mapq <= 10))
    return false;
  long const qual = 3l * disc_log_qual(hq_count, anti_count, 7u);
  if (qual < 50)
    return false;
  double const qd = static_cast<double>(qual) / static_cast<double>(depth);
  return qd >= 3.5;
}
} // namespace gtx
