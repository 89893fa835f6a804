// gtx_disc_bam_dev.hpp -- the split of a BAM file's record stream into the arrays discovery's kernels take, kernel source: one
// record per wavefront, one base per lane.  A record (SAM spec 4.2) is 32 fixed bytes, the name (l_read_name bytes), n_cigar words,
// (l_seq + 1) / 2 bytes of 4-bit codes -- the even base in the high nibble --, l_seq qualities, aux data.  Out of it come
//   the plane row   (gtx.h: the layout of gtx_pack_planes) -- lane l takes base 64k + l and its nibble; four ballots are 64 bases of
//                   each plane, that is the words 4g + b of the two groups g = 2k, 2k + 1, which lane 0 stores.  The whole row of
//                   plane_stride bytes is written: bits and groups behind l_qseq are zero;
//   the quality row -- l_qseq bytes as they lie in the record (0xFF as any other: the reference compares the raw byte), zero up to
//                   qual_stride;
//   the CIGAR words -- n_cigar of them at cigar_off, a word per lane and turn.
// The name shifts the words, the codes and the qualities to every residue mod 4: everything is read from the stream byte by byte.
// Only bytes of the record itself are read -- the low nibble of an odd read's last byte is masked out by its base index, not by its
// value --, and only the three outputs are written.  What the text indexes by (l_qseq, n_cigar, cigar_off, the offsets) is the host
// walk's, checked there against each record's block (gtx_disc_bam.cpp) and against the strides at the launch (gtx_disc_bam.hip).
//
// Written against the wave policy of graph_dev.hpp (lane lambdas, W::ballot): gtx_disc_bam.hip instantiates it with the hardware
// wave over the arrays of gtx_disc_bam_unpack (BamBatch), tests/emu_disc_bam with a sequential wave under AddressSanitizer / UBSan
// over heap blocks of exactly each record's bytes and each output's size.
#pragma once
#include <cstdint>

#include "../../include/gtx.h"
#include "graph_dev.hpp"

namespace gtx
{
namespace disc_bam_dev
{
constexpr uint32_t O_L_READ_NAME = 8, O_NAME = 32; // in a record, from its 32 fixed bytes on

// one record of `len` bases and `n_cigar` operations -> its three outputs.  rec: the record's 32 fixed bytes; row: plane_stride bytes,
// 4-byte aligned; qrow: qual_stride bytes; cigar: the record's own n_cigar words.  All arguments are wave-uniform.
template <class W>
GTX_DEV void unpack_record(uint8_t const * rec, uint32_t len, uint32_t n_cigar, uint32_t * row, uint32_t plane_stride, uint8_t * qrow, uint32_t qual_stride,
                           uint32_t * cigar)
{
  uint32_t const o_cigar = O_NAME + W::uni(static_cast<uint32_t>(rec[O_L_READ_NAME]));
  uint32_t const o_seq = o_cigar + 4u * n_cigar, o_qual = o_seq + (len + 1u) / 2u;
  uint32_t const groups = plane_stride / PLANE_GROUP_BYTES;
  for (uint32_t k = 0; 2u * k < groups; ++k) // 64 bases: two groups
  {
    typename W::template PerLane<bool> b0, b1, b2, b3;
    W::lanes([&](uint32_t l)
    {
      uint32_t const base = 64u * k + l;
      uint32_t code = 0;
      if (base < len)
      {
        uint32_t const byte = rec[o_seq + base / 2u];
        code = (base & 1u) ? (byte & 15u) : (byte >> 4);
      }
      b0[l] = (code & 1u) != 0;
      b1[l] = (code & 2u) != 0;
      b2[l] = (code & 4u) != 0;
      b3[l] = (code & 8u) != 0;
    });
    uint64_t const m0 = W::ballot(b0), m1 = W::ballot(b1), m2 = W::ballot(b2), m3 = W::ballot(b3);
    W::lanes([&](uint32_t l) // (the ballots are the wavefront's: one lane stores the eight words)
    {
      if (l != 0)
        return;
      uint32_t * const g = row + 8u * k;
      g[0] = static_cast<uint32_t>(m0);
      g[1] = static_cast<uint32_t>(m1);
      g[2] = static_cast<uint32_t>(m2);
      g[3] = static_cast<uint32_t>(m3);
      if (2u * k + 1u < groups)
      {
        g[4] = static_cast<uint32_t>(m0 >> 32);
        g[5] = static_cast<uint32_t>(m1 >> 32);
        g[6] = static_cast<uint32_t>(m2 >> 32);
        g[7] = static_cast<uint32_t>(m3 >> 32);
      }
    });
  }
  W::lanes([&](uint32_t l)
  {
    for (uint32_t j = l; j < qual_stride; j += 64u)
      qrow[j] = j < len ? rec[o_qual + j] : static_cast<uint8_t>(0);
    for (uint32_t j = l; j < n_cigar; j += 64u)
    {
      uint8_t const * const p = rec + o_cigar + 4u * j;
      cigar[j] = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
    }
  });
}
} // namespace disc_bam_dev

// the arrays of gtx_disc_bam_unpack
struct BamBatch
{
  uint8_t const * stream;
  uint32_t const * offsets;
  gtx_disc_read const * reads;
  uint32_t n_reads;
  uint8_t * planes;
  uint32_t plane_stride;
  uint8_t * qual;
  uint32_t qual_stride;
  uint32_t * cigar;
  GTX_DEV gtx_disc_read read(uint32_t i) const { return reads[i]; }
  GTX_DEV uint8_t const * record_of(uint32_t i) const { return stream + offsets[i]; }
  GTX_DEV uint32_t * row_of(uint32_t i) const { return reinterpret_cast<uint32_t *>(planes + static_cast<size_t>(i) * plane_stride); }
  GTX_DEV uint8_t * qual_of(uint32_t i) const { return qual + static_cast<size_t>(i) * qual_stride; }
  GTX_DEV uint32_t * cigar_of(uint32_t, gtx_disc_read const & r) const { return cigar + r.cigar_off; }
};

// A wavefront's records: `first`, then every `step`-th behind it (the launch: first = the wavefront's number, step = their count).
template <class W, class Batch>
GTX_DEV void disc_bam_unpack_wave(Batch const & b, uint32_t first, uint32_t step)
{
  for (uint32_t i = first; i < b.n_reads; i += step)
  {
    gtx_disc_read r = b.read(i);
    r.cigar_off = W::uni(r.cigar_off);
    disc_bam_dev::unpack_record<W>(b.record_of(i), W::uni(static_cast<uint32_t>(r.l_qseq)), W::uni(static_cast<uint32_t>(r.n_cigar)), b.row_of(i), b.plane_stride,
                                   b.qual_of(i), b.qual_stride, b.cigar_of(i, r));
  }
}
} // namespace gtx
