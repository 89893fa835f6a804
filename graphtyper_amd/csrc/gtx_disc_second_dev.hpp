// gtx_disc_second_dev.hpp -- discovery's second pass up to the aligner (parallel_second_pass, src/typer/caller.cpp:2633-2751),
// kernel source: the intake of a file's reads (read_hts_and_return_realignment_indels, :2232-2509), the buckets (:2490-2500,
// include/graphtyper/typer/bucket.hpp:33-43) and which reads the round of one indel looks at (realign_to_indels, :1890-1958).
// Nothing here calls an aligner; all values are integers.
//
// What the intake keeps of the reference's text (the text, not its comments):
//   * the file's buckets are made new (:2649-2650), so add_indel_event_to_bucket inserts a fresh EventSupport whose
//     has_realignment_support is false (event.hpp:101): every I and D that reaches the score pays 7 + (count - 1) * 1, and the
//     branch of :2404 is never taken.  The CIGAR indels live in the bucket's map, never in the global table: all that survives of
//     them is whether the file holds a given event at all (is_indel_in_bucket, src/typer/bucket.cpp:66-79) -- one found-bit per
//     table entry, set by a lookup of (position, type, length, letters).  No CIGAR event is written anywhere.
//   * score, pos_end and the sums they enter are int32_t in the reference (read.hpp:43-47) and are kept modulo 2^32 here; the
//     clip counts go through int16_t.
// The M compare is letter against letter: the read's letter is seq_nt16_str of its 4-bit code, the region's letter is the byte
// given to gtx_disc_create.  REPRESENTATION: the region is held as five bit planes per group of 32 bases -- the four planes of the
// letter's index in "=ACMGRSVTWYHKDBN" and a fifth that marks a byte outside that alphabet (such a byte differs from every read
// letter and is not N).  A block of 32 bases is then four XORs, the fifth plane and the two N tests.  (disc_ref_planes, which
// turns every letter but A/C/G/T into N, would score read A on region R as a match.)
//
// STATED LIMITS THAT DEPART FROM THE REFERENCE, which is undefined there: an M that runs behind the region's end or behind the
// read's last base -- such bases are not compared and add nothing, the offsets advance by `count` all the same; a read that
// starts at or behind the region's end (the reference ends the process, :2283-2287) is passed over like one in front of it.  The
// 16-bit deletion length of the first pass (gtx_disc_events_dev.hpp) does NOT apply here: a deletion of any length pays its
// penalty and is looked up by its length.
//
// The number of buckets is (REF_SIZE - 1) / BUCKET_SIZE + 1: every read that is not passed over lies below it.  The reference's
// NUM_BUCKETS and its resizes (bucket.cpp:95-96) differ from this only in empty buckets, which change nothing (an empty bucket
// has no reads to visit, and the descent of :1919 never starts above the last bucket a read lies in: begin_padded < REF_SIZE).
//
// Written against the wave policy of graph_dev.hpp (lane lambdas, W::excl_scan), as gtx_disc_events_dev.hpp is:
// gtx_disc_second.hip instantiates it with the hardware wave, tests/emu_disc_second with a sequential wave under
// AddressSanitizer / UBSan over heap blocks of exactly each array's size.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"
#include "gtx_disc_events_dev.hpp"

namespace gtx
{
namespace disc_second_dev
{
// include/graphtyper/constants.hpp.in:49-53, :94; realign_to_indels' PAD (:1863); read.hpp:15
constexpr uint32_t SCORE_MATCH = 1, SCORE_MISMATCH = 4, SCORE_GAP_OPEN = 7, SCORE_GAP_EXTEND = 1, SCORE_CLIP = 5;
constexpr uint16_t IS_CLIPPED = 8192;
constexpr long PAD = 50, MIN_READ_SIZE = 100;
constexpr int32_t READ_ANTI_SUPPORT = -1;
constexpr uint32_t REF_PLANES = 5;

// 32 bits from bit offset `o` of plane b of the region's five-plane array (zeros behind its end)
GTX_DEV uint32_t ref_bits(uint32_t const * planes, uint32_t groups, uint32_t o, uint32_t b)
{
  uint32_t const g = o >> 5, s = o & 31u;
  uint32_t const lo = g < groups ? planes[REF_PLANES * g + b] : 0u, hi = g + 1 < groups ? planes[REF_PLANES * (g + 1) + b] : 0u;
  return s == 0 ? lo : (lo >> s) | (hi << (32 - s));
}

// the letter of a read's base (seq_nt16_str of its code, :2311)
GTX_DEV char read_letter(uint32_t const * row, uint32_t row_groups, uint32_t o)
{
  uint32_t const g = o >> 5, s = o & 31u;
  uint32_t code = 0;
  if (g < row_groups)
    code = ((row[4 * g] >> s) & 1u) | (((row[4 * g + 1] >> s) & 1u) << 1) | (((row[4 * g + 2] >> s) & 1u) << 2) | (((row[4 * g + 3] >> s) & 1u) << 3);
  return "=ACMGRSVTWYHKDBN"[code];
}

// is_indel_in_bucket (bucket.cpp:66-79) turned round: the table entry that equals the event (pos, type, the `len` letters
// letter(0..len)) gets its found-bit.  The table is in Event order (src/typer/event.cpp:173-181): position first.
template <class W, class Batch, class Letter>
GTX_DEV void lookup(Batch const & in, uint32_t pos, uint8_t type, uint32_t len, Letter letter)
{
  uint32_t lo = 0, hi = in.n_table;
  while (lo < hi)
  {
    uint32_t const mid = lo + (hi - lo) / 2;
    if (in.table[mid].pos < pos)
      lo = mid + 1;
    else
      hi = mid;
  }
  for (uint32_t t = lo; t < in.n_table; ++t)
  {
    gtx_disc_indel const e = in.table[t];
    if (e.pos != pos)
      break;
    if (e.type != type)
      continue;
    if (e.len != len)
      continue;
    if (static_cast<uint64_t>(e.seq_off) + e.len > in.n_table_seq) // (an entry whose letters are not there equals nothing)
      continue;
    bool same = true;
    for (uint32_t k = 0; k < len && same; ++k)
      same = in.table_seq[e.seq_off + k] == letter(k);
    if (same)
    {
      W::atomic_or_u32(in.found + (t >> 5), 1u << (t & 31u));
      return;
    }
  }
}

// The intake of one read (:2261-2491): `o` receives pos_end, score, the clips and IS_CLIPPED; -> end_with_clip (:2491).
template <class W, class Batch>
GTX_DEV int32_t intake_walk(Batch const & in, uint32_t const * row, uint32_t row_groups, gtx_disc_read const & r, uint32_t const * cigar,
                            gtx_disc_second_read & o)
{
  long read_offset = 0, ref_offset = static_cast<long>(r.pos) - in.region_begin; // :2267-2270
  long const l_qseq = r.l_qseq, REF_SIZE = in.REF_SIZE;
  uint32_t score = 0; // (:2322; int32_t modulo 2^32)
  for (uint32_t i = 0; i < r.n_cigar; ++i)
  {
    if (ref_offset >= REF_SIZE) // :2326
      break;
    uint32_t const word = cigar[i];
    uint32_t const count = word >> 4, op = word & 15u;
    if (op == 0 || op == 7 || op == 8) // M = X (:2348-2372)
    {
      // (the stated limit: bases behind the region's end or the read's last base are not compared)
      long const span = std::min<long>(count, std::min(REF_SIZE - ref_offset, std::max<long>(l_qseq - read_offset, 0)));
      for (long k = 0; k < span; k += 32)
      {
        uint32_t const m = span - k >= 32 ? 0xFFFFFFFFu : (1u << (span - k)) - 1u;
        disc_events_dev::Bits32 const a = disc_events_dev::load32(row, row_groups, static_cast<uint32_t>(read_offset + k));
        uint32_t const q = static_cast<uint32_t>(ref_offset + k);
        uint32_t const g0 = ref_bits(in.ref5, in.ref_groups, q, 0), g1 = ref_bits(in.ref5, in.ref_groups, q, 1), g2 = ref_bits(in.ref5, in.ref_groups, q, 2),
                       g3 = ref_bits(in.ref5, in.ref_groups, q, 3), outside = ref_bits(in.ref5, in.ref_groups, q, 4);
        uint32_t const differ = (a.p0 ^ g0) | (a.p1 ^ g1) | (a.p2 ^ g2) | (a.p3 ^ g3) | outside;
        uint32_t const read_n = a.p0 & a.p1 & a.p2 & a.p3, ref_n = g0 & g1 & g2 & g3; // (a byte outside the alphabet has no code bits: never N)
        uint32_t const mismatch = differ & ~read_n & ~ref_n & m; // :2359
        uint32_t const bases = static_cast<uint32_t>(std::min<long>(span - k, 32)), bad = static_cast<uint32_t>(__builtin_popcount(mismatch));
        score += (bases - bad) * SCORE_MATCH;
        score -= bad * SCORE_MISMATCH;
      }
      read_offset += count;
      ref_offset += count;
    }
    else if (op == 1) // I (:2374-2409)
    {
      long const b = std::min(read_offset, l_qseq), e = std::min(read_offset + static_cast<long>(count), l_qseq);
      if (b == e)
        continue; // (:2385-2388: the read offset stays)
      lookup<W>(in, static_cast<uint32_t>(in.region_begin + ref_offset), 'I', static_cast<uint32_t>(e - b),
                [&](uint32_t k) { return read_letter(row, row_groups, static_cast<uint32_t>(b) + k); });
      score -= SCORE_GAP_OPEN + (count - 1u) * SCORE_GAP_EXTEND; // :2402
      read_offset += count;
    }
    else if (op == 2) // D (:2411-2442)
    {
      if (ref_offset + static_cast<long>(count) >= REF_SIZE) // :2415-2425: nothing happens, the loop goes on
        continue;
      lookup<W>(in, static_cast<uint32_t>(in.region_begin + ref_offset), 'D', count, [&](uint32_t k) { return in.refc[ref_offset + k]; });
      score -= SCORE_GAP_OPEN + (count - 1u) * SCORE_GAP_EXTEND; // :2437
      ref_offset += count;
    }
    else if (op == 4) // S (:2444-2484)
    {
      read_offset += count;
      o.flags |= IS_CLIPPED;
      score -= SCORE_CLIP;
      if (i == 0)
        o.num_clipped_begin = static_cast<int16_t>(static_cast<uint16_t>(count)); // (read.hpp:46-47: int16_t)
      else
        o.num_clipped_end = static_cast<int16_t>(static_cast<uint16_t>(count));
    }
    // (anything else, N included, moves neither the reference nor the read)
  }
  o.score = static_cast<int32_t>(score);
  o.pos_end = static_cast<int32_t>(static_cast<uint32_t>(in.region_begin + ref_offset)); // :2489
  return static_cast<int32_t>(static_cast<uint32_t>(o.pos_end) + static_cast<uint32_t>(static_cast<int32_t>(o.num_clipped_end))); // :2491
}

// The four-part test of :1948-1958 on the read's current fields (what gtx_disc_realign_wants states for clip counts that are not negative)
GTX_DEV bool wants(gtx_disc_second_read const & r, long indel_pos, long indel_span)
{
  long const pos = r.pos, pos_end = r.pos_end, cb = r.num_clipped_begin, ce = r.num_clipped_end;
  if (ce == 0 && pos_end < indel_pos)
    return false;
  if (pos_end + ce + std::min(ce, PAD) < indel_pos)
    return false;
  if (cb == 0 && pos > indel_span)
    return false;
  if (pos - cb - std::min(cb, PAD) > indel_span)
    return false;
  return true;
}
} // namespace disc_second_dev

// the region as five bit planes (the header's REPRESENTATION); planes: 5 * disc_ref_groups(reference_len) words of zeros
inline void disc_second_ref_planes(char const * reference, uint64_t reference_len, uint32_t * planes)
{
  char const * const nt16 = "=ACMGRSVTWYHKDBN";
  for (uint64_t i = 0; i < reference_len; ++i)
  {
    uint32_t code = 16;
    for (uint32_t c = 0; c < 16; ++c)
      if (nt16[c] == reference[i])
        code = c;
    uint32_t const bits = code < 16 ? code : 16u; // bit 4: outside the alphabet (its code planes stay 0)
    for (uint32_t b = 0; b < disc_second_dev::REF_PLANES; ++b)
      planes[disc_second_dev::REF_PLANES * (i >> 5) + b] |= ((bits >> b) & 1u) << (i & 31u);
  }
}

inline uint32_t disc_second_buckets(long REF_SIZE, long bucket_size) { return static_cast<uint32_t>((REF_SIZE - 1) / bucket_size + 1); }

constexpr uint32_t DISC_SECOND_NO_BUCKET = 0xFFFFFFFFu;

// the arguments of gtx_disc_second_intake as the kernel sees them (tests/emu_disc_second has a batch of its own)
struct SecondBatch
{
  uint32_t const * ref5;
  uint32_t ref_groups;
  char const * refc;
  long REF_SIZE, region_begin, bucket_size;
  uint32_t n_buckets;
  uint8_t const * rows;
  uint32_t plane_stride;
  gtx_disc_read const * reads;
  uint32_t const * cigar;
  uint32_t n_reads;
  gtx_disc_indel const * table;
  char const * table_seq;
  uint32_t n_table;
  uint64_t n_table_seq;
  gtx_disc_second_read * out;
  int32_t * bucket_max;
  uint32_t * max_read_size;
  uint32_t * found;
  uint32_t *key, *index, *end_clip; // per read: its bucket (n_buckets: none), its stream index, max(0, end_with_clip)
  GTX_DEV gtx_disc_read read(uint32_t i) const { return reads[i]; }
  GTX_DEV uint32_t const * row_of(uint32_t i) const { return reinterpret_cast<uint32_t const *>(rows + static_cast<uint64_t>(i) * plane_stride); }
  GTX_DEV uint32_t const * cigar_of(uint32_t, gtx_disc_read const & r) const { return cigar + r.cigar_off; }
};

// what the call sets before the reads are taken in (lane i of as many as there are buckets or found-words)
GTX_DEV void disc_second_init(uint32_t i, int32_t * bucket_max, uint32_t n_buckets, uint32_t * found, uint32_t found_words, uint32_t * max_read_size)
{
  if (i < n_buckets)
    bucket_max[i] = -1; // bucket.hpp:37
  if (i < found_words)
    found[i] = 0;
  if (i == 0)
    *max_read_size = static_cast<uint32_t>(disc_second_dev::MIN_READ_SIZE); // :2651
}

// The reads first_read .. first_read + 63 of a file, lane l the read first_read + l.  What a read leaves in the bucket arrays
// goes through atomic maxima, so no launch order shows in them.
template <class W, class Batch>
GTX_DEV void disc_second_intake_wave(Batch const & in, uint32_t first_read)
{
  using namespace disc_second_dev;
  uint32_t const row_groups = in.plane_stride / PLANE_GROUP_BYTES;
  W::lanes([&](uint32_t l) {
    uint32_t const i = first_read + l;
    if (i >= in.n_reads)
      return;
    gtx_disc_read const r = in.read(i);
    gtx_disc_second_read o{};
    o.pos = -1;
    o.pos_end = -1;
    o.flags = r.flag; // :2305-2306
    o.mapq = r.mapq;
    o.l_qseq = r.l_qseq;
    o.bucket = DISC_SECOND_NO_BUCKET;
    uint32_t key = in.n_buckets, end_clip = 0;
    long const ref_offset = static_cast<long>(r.pos) - in.region_begin;
    // :2247 a read without a cigar or in front of the region is passed over (and, the stated limit, one behind the region's end)
    if (r.n_cigar != 0 && r.pos >= in.region_begin && ref_offset < in.REF_SIZE)
    {
      key = static_cast<uint32_t>(ref_offset / in.bucket_size); // :2273
      W::atomic_max_u32(in.max_read_size, r.l_qseq); // :2276-2277
      int32_t const end_with_clip = intake_walk<W>(in, in.row_of(i), row_groups, r, in.cigar_of(i, r), o);
      o.pos = r.pos; // :2488
      o.bucket = key;
      W::atomic_max_i32(in.bucket_max + key, end_with_clip); // :2493-2495 (max_pos_end begins at -1, bucket.hpp:37)
      end_clip = static_cast<uint32_t>(std::max<int32_t>(end_with_clip, 0)); // :2241, :2496 (global_max_pos_end begins at 0)
    }
    in.out[i] = o;
    in.key[i] = key;
    in.index[i] = i;
    in.end_clip[i] = end_clip;
  });
}

// Bucket b once the reads' indices are grouped by bucket, stably (sorted_key / sorted_index: n_reads entries, the reads that
// were passed over last), and run_max[i] = max(end_clip[0..i]) in STREAM order.
// global_max_pos_end, derived from the text: :2499 gives every read's bucket the running maximum as it stands after that
// read, so a bucket keeps the value of its LAST read in stream order, whatever the bucket's number; the running value grows
// only inside `if (end_with_clip > bucket.max_pos_end)` (:2493-2497), but a read that fails that test is not above an earlier
// read of its bucket, which did enter: the running value is max(0, end_with_clip of every read so far).  A bucket without
// reads keeps -1 (bucket.hpp:36).  Nothing updates it after the intake.
GTX_DEV void disc_second_bucket(uint32_t b, uint32_t n_buckets, uint32_t const * sorted_key, uint32_t const * sorted_index, uint32_t n_reads,
                                uint32_t const * run_max, uint32_t * bucket_off, int32_t * bucket_global_max)
{
  auto lower = [&](uint32_t v)
  {
    uint32_t lo = 0, hi = n_reads;
    while (lo < hi)
    {
      uint32_t const mid = lo + (hi - lo) / 2;
      if (sorted_key[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo;
  };
  uint32_t const lo = lower(b);
  bucket_off[b] = lo;
  if (b < n_buckets)
  {
    uint32_t const hi = lower(b + 1);
    bucket_global_max[b] = hi > lo ? static_cast<int32_t>(run_max[sorted_index[hi - 1]]) : -1;
  }
}

// the arguments of gtx_disc_second_candidates as the kernels see them
struct SecondRound
{
  uint32_t const * list;
  gtx_disc_indel const * table;
  uint32_t n_table;
  gtx_disc_second_read const * reads;
  uint32_t n_reads;
  gtx_disc_second_event const * events;
  uint32_t n_events;
  long region_begin, REF_SIZE, bucket_size;
  uint32_t n_buckets;
  int32_t const *bucket_max, *bucket_global_max;
  uint32_t const * max_read_size;
  uint32_t const *bucket_reads, *bucket_off;
  gtx_disc_second_pair * pairs;
  uint32_t pair_cap;
};

// One read of one indel's round (:1941-1958): does realign_to_indels align it?
template <class In>
GTX_DEV bool disc_second_takes(In const & in, uint32_t read, uint32_t entry, long indel_pos, long indel_span)
{
  using namespace disc_second_dev;
  gtx_disc_second_read const r = in.reads[read];
  if (r.pos < 0 || r.l_qseq == 0) // :1941
    return false;
  if (r.bucket >= in.n_buckets || in.bucket_max[r.bucket] <= indel_pos - PAD) // :1929 (the intake's maximum of the read's bucket)
    return false;
  // has_indel_event (src/typer/read.cpp:13-22): the first entry that names the indel decides
  for (uint32_t e = 0; e < r.n_events; ++e)
  {
    if (static_cast<uint64_t>(r.first_event) + e >= in.n_events)
      break;
    gtx_disc_second_event const ev = in.events[r.first_event + e];
    if (ev.indel == entry)
    {
      if (ev.read_pos != READ_ANTI_SUPPORT)
        return false;
      break;
    }
  }
  return wants(r, indel_pos, indel_span);
}

// The round of list entry k (:1876-1958): the reads it looks at, in the reference's order of visit -- bucket, then stream
// order.  EMIT = false counts them; EMIT = true writes pair j to pairs[first + j] where that lies below pair_cap.  -> their number.
// One wavefront; 64 reads of the bucket range per step.
template <class W, bool EMIT, class In>
GTX_DEV uint32_t disc_second_round_wave(In const & in, uint32_t k, uint32_t first)
{
  using namespace disc_second_dev;
  uint32_t const entry = in.list[k];
  if (entry >= in.n_table)
    return 0;
  gtx_disc_indel const indel = in.table[entry];
  long const pos = indel.pos, indel_span = pos + indel.span; // :1880
  long const max_read_size = *in.max_read_size;
  long const begin_padded = std::max(0l, pos - max_read_size - 2 * PAD - in.region_begin); // :1890
  long const end_padded = pos + max_read_size + 2 * PAD - in.region_begin;                  // :1892
  long b = begin_padded / in.bucket_size;                                                   // :1911
  long const b_end = std::min(static_cast<long>(in.n_buckets) - 1, end_padded / in.bucket_size); // :1912
  if (b >= static_cast<long>(in.n_buckets) || end_padded < 0) // (:1891, :1913 assert otherwise: an indel behind or in front of the region has no round)
    return 0;
  while (b > 0 && in.bucket_global_max[b] > pos - PAD) // :1919 (an empty bucket, -1, stops the descent)
    --b;
  if (b_end < b)
    return 0;
  // the buckets b .. b_end are one stretch of the grouped reads
  uint32_t const lo = in.bucket_off[b], hi = in.bucket_off[b_end + 1];
  uint32_t produced = 0;
  for (uint32_t at = lo; at < hi; at += 64)
  {
    typename W::template PerLane<uint32_t> take, excl, read;
    W::lanes([&](uint32_t l) {
      take[l] = 0;
      read[l] = 0;
      if (at + l < hi)
      {
        read[l] = in.bucket_reads[at + l];
        take[l] = read[l] < in.n_reads && disc_second_takes(in, read[l], entry, pos, indel_span) ? 1u : 0u;
      }
    });
    uint32_t total = 0;
    W::excl_scan(take, excl, total);
    if (EMIT)
      W::lanes([&](uint32_t l) {
        uint64_t const slot = static_cast<uint64_t>(first) + produced + excl[l];
        if (take[l] && slot < in.pair_cap)
          in.pairs[slot] = gtx_disc_second_pair{read[l], k};
      });
    produced += total;
  }
  return produced;
}

// the counters behind a call (the d_counts convention of gtx_disc_events_batch): counts[0] += pairs produced, counts[1] += those
// of them that lie at or behind pair_cap
GTX_DEV void disc_second_count(uint32_t * counts, uint32_t total, uint32_t pair_cap)
{
  uint64_t const base = counts[0], end = base + total;
  uint64_t const fit = end <= pair_cap ? total : (base < pair_cap ? pair_cap - base : 0);
  counts[0] = static_cast<uint32_t>(end);
  counts[1] += static_cast<uint32_t>(total - fit);
}
} // namespace gtx
