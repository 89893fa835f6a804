// gtx_disc_bam.cpp -- a BAM file of discovery read once on the host, as parallel_first_pass / parallel_second_pass read it
// (src/typer/caller.cpp:2511-2571, :2633-2682: region ".", every record in file order with get_next_read): the record stream as it
// lies in the file and, per record, the gtx_disc_read and the offset the unpack kernel (gtx_disc_bam_dev.hpp) starts from.  Built on
// the one BAM parser (gtx_bam_record.hpp) and the BGZF reader with its inflate team (gtx_bgzf.hpp); host code, no HIP.
//
// Each record's block is read where it stays, behind the stream (append_bam_block), and the walk looks at its block_size word and
// its 32 fixed bytes: parse_bam_core holds the counts to the block, so the device never follows a length that nobody checked.
#include "gtx_bam_record.hpp"
#include "gtx_disc_bam.hpp"

#include <exception>
#include <memory>

#include <sys/stat.h>

namespace
{
int fail(std::string const & msg, int status)
{
  gtx::g_last_error = "gtx_disc_bam_read: " + msg;
  return status;
}

int read_file(std::string const & path, gtx_disc_bam & out)
{
  gtx::Bgzf fp;
  if (!fp.open(path))
    return fail("could not open " + path, GTX_ERR_IO);
  gtx::BamHeader head;
  gtx::BamHeaderRead const got = gtx::read_bam_header(fp, head);
  if (got == gtx::BAM_NOT_BAM)
    return fail(path + " is not a BAM file (CRAM is not read)", GTX_ERR_UNSUPPORTED);
  if (got == gtx::BAM_TRUNCATED)
    return fail(path + ": truncated header", GTX_ERR_IO);
  gtx::BamSamples table;
  if (!gtx::read_bam_samples(head.text, path, table))
    return fail(path + ": an @RG line without ID or SM", GTX_ERR_ARG);
  if (table.samples.size() != 1) // caller.cpp:2537-2544
    return fail(path + ": more than one sample in a file of discovery", GTX_ERR_UNSUPPORTED);
  out.sample = table.samples[0];
  // (room for the whole stream at once, from the file's size: short reads inflate to some 2.4 times their BGZF; a file that
  // inflates to more grows the block as a vector does)
  struct stat info;
  if (::stat(path.c_str(), &info) == 0 && info.st_size > 0)
    out.stream.reserve(static_cast<size_t>(std::min<uint64_t>(3ull * static_cast<uint64_t>(info.st_size), (1ull << 32) - 1)));
  for (;;)
  {
    size_t at = 0;
    gtx::BamBlockRead const next = gtx::append_bam_block(fp, out.stream, &at);
    if (next == gtx::BAM_BLOCK_END)
      break;
    if (next != gtx::BAM_BLOCK_OK)
      return fail(path + ": truncated BAM record", GTX_ERR_IO);
    gtx::BamCore c;
    if (!gtx::parse_bam_core(out.stream.data() + at, out.stream.size() - at, c))
      return fail(path + ": malformed BAM record", GTX_ERR_IO);
    if (c.l_seq > 0xFFFF)
      return fail(path + ": a read of more than 65535 bases", GTX_ERR_UNSUPPORTED);
    if (out.stream.size() + gtx::DISC_BAM_SLACK >= (1ull << 32))
      return fail(path + ": a record stream of 2^32 bytes or more", GTX_ERR_CAPACITY);
    out.offsets.push_back(static_cast<uint32_t>(at));
    out.reads.push_back(gtx_disc_read{c.pos, c.flag, c.mapq, 0, static_cast<uint16_t>(c.l_seq), c.n_cigar, static_cast<uint32_t>(out.n_cigar)});
    out.n_cigar += c.n_cigar;
    out.max_l_seq = std::max(out.max_l_seq, static_cast<uint32_t>(c.l_seq));
  }
  out.stream.insert(out.stream.end(), gtx::DISC_BAM_SLACK, 0);
  return GTX_OK;
}
} // namespace

extern "C" int gtx_disc_bam_read(const char * path, gtx_disc_bam ** out)
{
  if (!out)
  {
    gtx::g_last_error = "gtx_disc_bam_read: bad argument";
    return GTX_ERR_ARG;
  }
  *out = nullptr;
  if (!path)
  {
    gtx::g_last_error = "gtx_disc_bam_read: bad argument";
    return GTX_ERR_ARG;
  }
  try
  {
    auto h = std::make_unique<gtx_disc_bam>();
    int const rc = read_file(path, *h);
    if (rc == GTX_OK)
      *out = h.release();
    return rc;
  }
  catch (std::exception const & e)
  {
    return fail(std::string(path) + ": " + e.what(), GTX_ERR_CAPACITY);
  }
}

extern "C" void gtx_disc_bam_destroy(gtx_disc_bam * b) { delete b; }

extern "C" const uint8_t * gtx_disc_bam_stream(const gtx_disc_bam * b, uint64_t * n_bytes, uint32_t * slack)
{
  if (n_bytes)
    *n_bytes = b ? b->stream.size() - gtx::DISC_BAM_SLACK : 0;
  if (slack)
    *slack = gtx::DISC_BAM_SLACK;
  return b ? b->stream.data() : nullptr;
}

extern "C" const gtx_disc_read * gtx_disc_bam_reads(const gtx_disc_bam * b, uint32_t * n_reads, const uint32_t ** offsets)
{
  if (n_reads)
    *n_reads = b ? static_cast<uint32_t>(b->reads.size()) : 0;
  if (offsets)
    *offsets = b ? b->offsets.data() : nullptr;
  return b ? b->reads.data() : nullptr;
}

extern "C" const char * gtx_disc_bam_info(const gtx_disc_bam * b, uint32_t * max_l_seq, uint64_t * n_cigar)
{
  if (max_l_seq)
    *max_l_seq = b ? b->max_l_seq : 0;
  if (n_cigar)
    *n_cigar = b ? b->n_cigar : 0;
  return b ? b->sample.c_str() : nullptr;
}
