// gtx_disc_bam_walk_dev.hpp -- the record walk of a BAM record stream on the device, kernel source: where the records begin, each
// record's counts held to its block, and the two tables the unpack kernel (gtx_disc_bam_dev.hpp) indexes by -- `offsets` and the
// gtx_disc_read table.  It is the host walk of gtx_disc_bam.cpp (append_bam_block + parse_bam_core) over bytes that stay on the device.
//
// The definition.  o = 0; a record begins with its block_size word at o.  o == n_bytes: the stream ends, BAM_WALK_OK.  Fewer than 4
// bytes left, block < 32 as a signed word, o + 4 + block > n_bytes: BAM_WALK_TRUNCATED at o.  l_seq < 0 or 32 + l_read_name +
// 4 n_cigar + (l_seq + 1) / 2 + l_seq > block: BAM_WALK_MALFORMED at o; else l_seq > 65 535: BAM_WALK_LONG_READ at o.  A sound record
// is offsets[i] = o + 4 and reads[i] = {pos, flag, mapq, 0, l_seq, n_cigar, the sum of n_cigar in front of it}; the next o is
// o + 4 + block.  Nothing behind the first bad record is reported; the records in front of it are.
//
// The chain is sequential, the segments between the caller's cuts need not be: three steps in stream order over one function
// walk(entry, limit), none of which waits for another workgroup.
//   guess    a wavefront per segment walks from "a record begins at the segment's start" (htslib's layout: bgzf_flush_try puts a
//            record that does not fit into the next member) over the records that BEGIN in the segment, and leaves its entry, its
//            exit (the first o at or behind the segment's end), its counts and its status;
//   resolve  one wavefront goes through the segments in order (disc_bam_walk_resolve_wave: the argument stands there);
//   emit     a wavefront per segment writes the tables from the segment's true entry.
//
// Inside a walk the lanes share the work in turns of up to 64 records.  Only the block_size words are a chain: the turn's first part
// follows them, wave-uniform, one load per record behind its two tests (4 bytes left; 32 <= block <= what is left), and hands record
// k's start to lane k.  Then the lanes parse their records' fixed bytes side by side -- those 32 bytes lie inside the block, which
// lies inside the stream --, a ballot finds the first record whose counts fail, an exclusive scan numbers the CIGAR words, and the
// lanes store their table entries next to each other.
//
// Every load lies in [0, n_bytes), whatever a guessed walk meets: the word at o is loaded when n_bytes - o >= 4, the fixed bytes
// behind 32 <= block <= n_bytes - o - 4.  The arithmetic cannot wrap: o <= n_bytes < 2^32 and block <= n_bytes - o - 4, so
// o + 4 + block <= n_bytes; the counts are summed in 64 bits (l_seq up to 2^31 - 1).  Every step advances o by at least 36: a walk ends.
// Bytes are loaded one by one (a record lies at any residue).
//
// Written against the wave policy of graph_dev.hpp: gtx_disc_bam_walk.hip instantiates it with the hardware wave,
// tests/emu_disc_bam_walk with a sequential wave under AddressSanitizer / UBSan over heap blocks of exactly the sizes.
#pragma once
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"

namespace gtx
{
enum : uint32_t { BAM_WALK_OK = 0, BAM_WALK_TRUNCATED = 1, BAM_WALK_MALFORMED = 2, BAM_WALK_LONG_READ = 3 };

// what a walk leaves; every field is wave-uniform
struct BamWalkRun
{
  uint32_t exit;      // the first o the walk did not take (status OK: at or behind its limit)
  uint32_t n_reads;   // sound records, in front of the first bad one
  uint32_t max_l_seq; // of those
  uint32_t status;    // BAM_WALK_*
  uint32_t bad_at;    // status != OK: the o of the bad record
  uint64_t n_cigar;   // the sum of n_cigar of the sound records
};

// a segment between two steps (device memory, n_cuts + 1 of them)
struct BamWalkSeg
{
  uint32_t entry;     // guess: the segment's start; resolve: the true entry (at or behind the segment's end: no record begins here)
  uint32_t exit;
  uint32_t n_reads;   // resolve: 0 behind the first bad record and in a segment a record spans
  uint32_t max_l_seq;
  uint32_t status, bad_at;
  uint32_t base;      // resolve: the records in front of the segment's
  uint32_t reserved;
  uint64_t n_cigar, cigar_base; // cigar_base: resolve, the CIGAR words in front of the segment's
};
static_assert(sizeof(BamWalkSeg) == 48, "the segment table's layout");

namespace disc_bam_walk_dev
{
GTX_DEV uint32_t load_u16(uint8_t const * p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8); }
GTX_DEV uint32_t load_u32(uint8_t const * p) { return load_u16(p) | (load_u16(p + 2) << 16); }

// The records that begin in [entry, limit) (entry <= limit <= n_bytes), at most `want` of them.  offsets != nullptr: their table
// entries go to offsets[base + i], reads[base + i] with cigar_off = cigar_base + the words in front (modulo 2^32, as the host walk
// casts it).  All arguments are wave-uniform.
template <class W>
GTX_DEV BamWalkRun walk(uint8_t const * stream, uint32_t n_bytes, uint32_t entry, uint32_t limit, uint32_t want, uint32_t * offsets, gtx_disc_read * reads,
                        uint32_t base, uint64_t cigar_base)
{
  BamWalkRun run{entry, 0, 0, BAM_WALK_OK, 0, 0};
  uint32_t o = entry;
  while (o < limit && run.n_reads < want)
  {
    // the chain: up to 64 starts, lane k gets the k-th
    typename W::template PerLane<uint32_t> start, block;
    uint32_t k = 0, chain_status = BAM_WALK_OK;
    while (k < 64u && o < limit)
    {
      if (n_bytes - o < 4u)
      {
        chain_status = BAM_WALK_TRUNCATED;
        break;
      }
      uint32_t const b = W::uni(load_u32(stream + o));
      if (static_cast<int32_t>(b) < 32 || b > n_bytes - o - 4u)
      {
        chain_status = BAM_WALK_TRUNCATED;
        break;
      }
      W::lanes([&](uint32_t l)
      {
        if (l == k)
        {
          start[l] = o;
          block[l] = b;
        }
      });
      ++k;
      o += 4u + b;
    }
    // the counts, a record per lane
    typename W::template PerLane<uint32_t> verdict, words, len;
    typename W::template PerLane<bool> bad;
    W::lanes([&](uint32_t l)
    {
      verdict[l] = BAM_WALK_OK;
      words[l] = 0;
      len[l] = 0;
      if (l < k)
      {
        uint8_t const * const p = stream + start[l] + 4u;
        uint32_t const l_read_name = p[8], n_cigar = load_u16(p + 12), l_seq = load_u32(p + 16);
        if (static_cast<int32_t>(l_seq) < 0 || 32ull + l_read_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1u) / 2u + l_seq > block[l])
          verdict[l] = BAM_WALK_MALFORMED;
        else if (l_seq > 0xFFFFu)
          verdict[l] = BAM_WALK_LONG_READ;
        words[l] = n_cigar;
        len[l] = l_seq;
      }
      bad[l] = verdict[l] != BAM_WALK_OK;
    });
    uint64_t const bad_lanes = W::ballot(bad);
    uint32_t const first_bad = bad_lanes ? static_cast<uint32_t>(__builtin_ctzll(bad_lanes)) : 64u;
    uint32_t const sound = first_bad < k ? first_bad : k, room = want - run.n_reads, take = sound < room ? sound : room;
    W::lanes([&](uint32_t l)
    {
      if (l >= take)
      {
        words[l] = 0;
        len[l] = 0;
      }
    });
    typename W::template PerLane<uint32_t> before;
    uint32_t turn_words = 0;
    W::excl_scan(words, before, turn_words);
    uint32_t const longest = W::max(len);
    if (offsets)
      W::lanes([&](uint32_t l)
      {
        if (l < take)
        {
          uint8_t const * const p = stream + start[l] + 4u;
          uint32_t const i = base + run.n_reads + l;
          offsets[i] = start[l] + 4u;
          reads[i] = gtx_disc_read{static_cast<int32_t>(load_u32(p + 4)), static_cast<uint16_t>(load_u16(p + 14)), p[9], 0, static_cast<uint16_t>(len[l]),
                                   static_cast<uint16_t>(words[l]), static_cast<uint32_t>(cigar_base + run.n_cigar + before[l])};
        }
      });
    run.n_reads += take;
    run.n_cigar += turn_words;
    run.max_l_seq = longest > run.max_l_seq ? longest : run.max_l_seq;
    if (take < sound) // (`want` records are there)
      break;
    if (first_bad < k) // a record whose counts fail lies in front of whatever ended the chain
    {
      run.status = W::from_lane(verdict, first_bad);
      run.bad_at = W::from_lane(start, first_bad);
      break;
    }
    if (chain_status != BAM_WALK_OK)
    {
      run.status = chain_status;
      run.bad_at = o;
      break;
    }
  }
  run.exit = o;
  return run;
}

GTX_DEV uint32_t seg_begin(uint32_t const * cuts, uint32_t s) { return s == 0 ? 0u : cuts[s - 1u]; }
GTX_DEV uint32_t seg_end(uint32_t const * cuts, uint32_t n_cuts, uint32_t n_bytes, uint32_t s) { return s < n_cuts ? cuts[s] : n_bytes; }
} // namespace disc_bam_walk_dev

// the arrays of the three steps: the stream, the cuts (strictly ascending, in (0, n_bytes)), the segment table
struct BamWalkBatch
{
  uint8_t const * stream;
  uint32_t n_bytes;
  uint32_t const * cuts;
  uint32_t n_cuts;
  BamWalkSeg * segs; // n_cuts + 1
};

// guess.  A wavefront's segments: `first`, then every `step`-th behind it.
template <class W>
GTX_DEV void disc_bam_walk_guess_wave(BamWalkBatch const & b, uint32_t first, uint32_t step)
{
  using namespace disc_bam_walk_dev;
  for (uint64_t s = first; s <= b.n_cuts; s += step) // (64 bits: n_cuts + step may pass 2^32)
  {
    uint32_t const begin = W::uni(seg_begin(b.cuts, static_cast<uint32_t>(s))), end = W::uni(seg_end(b.cuts, b.n_cuts, b.n_bytes, static_cast<uint32_t>(s)));
    BamWalkRun const r = walk<W>(b.stream, b.n_bytes, begin, end, 0xFFFFFFFFu, nullptr, nullptr, 0, 0);
    W::lanes([&](uint32_t l)
    {
      if (l == 0)
        b.segs[s] = BamWalkSeg{begin, r.exit, r.n_reads, r.max_l_seq, r.status, r.bad_at, 0, 0, r.n_cigar, 0};
    });
  }
}

// resolve, one wavefront, behind every guess.  Segment 0's true entry is 0; a segment's true entry is its predecessor's true exit.
// Why the adopted chain is the true chain, by induction over the segments: let e be segment s's true entry -- the first record start
// of the true chain at or behind the end of segment s - 1 (s = 0: e = 0).  If e lies at or behind the end of s, a record spans s, no
// record begins in it, and e is the true entry of s + 1 as well.  Else the records that begin in s are those walk(e, end of s) takes,
// for walk is a function of its entry alone; where e is the segment's start, that is the walk the guess made, whose result is
// adopted unread; where it is not, the guess walked something else (a record's inside), its result is dropped and the segment is
// walked from e.  Either way the segment's exit is the true chain's first start at or behind its end: the true entry of s + 1.
// A guess is never looked at but for its entry being the true one, so what it met -- quality bytes that read as records, damage
// that is none -- decides nothing.  Behind the first bad record of the true chain no segment reports anything.
// Leaves per segment the true entry, the counts and their exclusive sums, and in *out the totals, the first status in chain order
// with its offset, the segments whose guess held (hit) and those walked again (rewalked).
template <class W>
GTX_DEV void disc_bam_walk_resolve_wave(BamWalkBatch const & b, gtx_bam_walk_out * out)
{
  using namespace disc_bam_walk_dev;
  uint32_t e = 0, n_reads = 0, longest = 0, status = BAM_WALK_OK, bad_at = 0, hit = 0, rewalked = 0;
  uint64_t n_cigar = 0;
  for (uint32_t s = 0; s <= b.n_cuts; ++s)
  {
    uint32_t const begin = W::uni(seg_begin(b.cuts, s)), end = W::uni(seg_end(b.cuts, b.n_cuts, b.n_bytes, s));
    BamWalkSeg seg{e, e, 0, 0, BAM_WALK_OK, 0, n_reads, 0, 0, n_cigar};
    if (status == BAM_WALK_OK && e < end)
    {
      if (e == begin)
      {
        ++hit;
        seg.exit = W::uni(b.segs[s].exit);
        seg.n_reads = W::uni(b.segs[s].n_reads);
        seg.max_l_seq = W::uni(b.segs[s].max_l_seq);
        seg.status = W::uni(b.segs[s].status);
        seg.bad_at = W::uni(b.segs[s].bad_at);
        seg.n_cigar = W::uni(static_cast<uint64_t>(b.segs[s].n_cigar));
      }
      else
      {
        ++rewalked;
        BamWalkRun const r = walk<W>(b.stream, b.n_bytes, e, end, 0xFFFFFFFFu, nullptr, nullptr, 0, 0);
        seg.exit = r.exit;
        seg.n_reads = r.n_reads;
        seg.max_l_seq = r.max_l_seq;
        seg.status = r.status;
        seg.bad_at = r.bad_at;
        seg.n_cigar = r.n_cigar;
      }
      n_reads += seg.n_reads;
      n_cigar += seg.n_cigar;
      longest = seg.max_l_seq > longest ? seg.max_l_seq : longest;
      status = seg.status;
      bad_at = seg.bad_at;
      e = seg.exit;
    }
    else if (status != BAM_WALK_OK)
      seg.entry = seg.exit = end; // behind the first bad record
    W::lanes([&](uint32_t l)
    {
      if (l == 0)
        b.segs[s] = seg;
    });
  }
  W::lanes([&](uint32_t l)
  {
    if (l == 0)
      *out = gtx_bam_walk_out{status, longest, bad_at, n_cigar, n_reads, hit, rewalked, 0};
  });
}

// emit, behind resolve.  A wavefront's segments as in guess; a segment writes its n_reads entries from `base` on and nothing else.
template <class W>
GTX_DEV void disc_bam_walk_emit_wave(BamWalkBatch const & b, uint32_t * offsets, gtx_disc_read * reads, uint32_t first, uint32_t step)
{
  using namespace disc_bam_walk_dev;
  for (uint64_t s = first; s <= b.n_cuts; s += step) // (64 bits: n_cuts + step may pass 2^32)
  {
    uint32_t const n = W::uni(b.segs[s].n_reads);
    if (n == 0)
      continue;
    uint32_t const end = W::uni(seg_end(b.cuts, b.n_cuts, b.n_bytes, static_cast<uint32_t>(s)));
    (void)walk<W>(b.stream, b.n_bytes, W::uni(b.segs[s].entry), end, n, offsets, reads, W::uni(b.segs[s].base), W::uni(static_cast<uint64_t>(b.segs[s].cigar_base)));
  }
}
} // namespace gtx
