// gtx_disc_bam.hpp -- what the two halves of discovery's BAM front end share: the file read on the host (gtx_disc_bam.cpp, no HIP) and
// the unpack of its record stream on the device (gtx_disc_bam.hip, kernel text: gtx_disc_bam_dev.hpp).  No HIP header here.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gtx.h"

namespace gtx
{
extern thread_local std::string g_last_error;

// Bytes behind a record that the kernel's text may read: it loads bytes and never past a record's qualities, so none.  The host block
// and the device block are sized with it all the same, and tests/emu_disc_bam gives every record exactly this much.
constexpr uint32_t DISC_BAM_SLACK = 0;

// gtx_disc_bam_unpack in its two halves, for a caller that has the two tables on the host (gtx_discover_files).  The check, host
// code over the host copies: what the kernel indexes by -- the strides against every l_qseq, the CIGAR words against n_cigar, the
// offsets against n_bytes -- or GTX_ERR_ARG with a message.  The launch: the kernel over device arrays that passed the check.
int disc_bam_unpack_check(uint64_t n_bytes, uint32_t const * offsets, gtx_disc_read const * reads, uint32_t n_reads, uint32_t plane_stride,
                          uint32_t qual_stride, uint32_t n_cigar);
int disc_bam_unpack_launch(uint8_t const * d_stream, uint32_t const * d_offsets, gtx_disc_read const * d_reads, uint32_t n_reads, uint8_t * d_planes,
                           uint32_t plane_stride, uint8_t * d_qual, uint32_t qual_stride, uint32_t * d_cigar, void * stream);

// gtx_disc_bam_walk in its two halves (gtx_disc_bam_walk.hip), for a caller that sizes the tables from the count (gtx_discover_files_front):
// guess and resolve, which leave *d_out and the segment table (n_cuts + 1 entries of BamWalkSeg, gtx_disc_bam_walk_dev.hpp); then emit
// over the same cuts and segment table into tables of at least d_out->n_reads entries.  Launches on `stream`, nothing is waited for.
// d_cuts: device, strictly ascending in (0, n_bytes); n_bytes > 0.
struct BamWalkSeg;
int disc_bam_walk_count(uint8_t const * d_stream, uint32_t n_bytes, uint32_t const * d_cuts, uint32_t n_cuts, BamWalkSeg * d_segs, gtx_bam_walk_out * d_out,
                        void * stream);
int disc_bam_walk_emit(uint8_t const * d_stream, uint32_t n_bytes, uint32_t const * d_cuts, uint32_t n_cuts, BamWalkSeg * d_segs, uint32_t * d_offsets,
                       gtx_disc_read * d_reads, void * stream);
} // namespace gtx

struct gtx_disc_bam
{
  std::vector<uint8_t> stream; // the records as they lie in the file, DISC_BAM_SLACK zero bytes behind them
  std::vector<gtx_disc_read> reads;
  std::vector<uint32_t> offsets; // of each record's 32 fixed bytes
  uint32_t max_l_seq = 0;
  uint64_t n_cigar = 0;
  std::string sample;
};
