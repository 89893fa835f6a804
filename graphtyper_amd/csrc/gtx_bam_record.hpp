// gtx_bam_record.hpp -- the BAM format as all of its readers see it (gtx_bam.cpp: gtx_reads_*; gtx_shrink.cpp: the pre-filter;
// gtx_disc_bam.cpp: discovery's files): the header, its samples, the next record's block, the fixed 32 bytes of a record with the
// offsets of what follows them, the reference span of a CIGAR.  (SAM spec 4.2)
#pragma once
#include "gtx_bgzf.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace gtx
{
struct BamHeader
{
  std::string text; // as in the file: l_text bytes
  std::vector<std::pair<std::string, int32_t>> refs; // name, length
};

// BAM_NOT_BAM: no magic, or no text length behind it; BAM_TRUNCATED: the file ends inside the text or the reference list (or a
// name's length is none: not positive, or beyond 1 MiB -- no contig is called that, and the field must not size an allocation)
// Reader: a Bgzf, or anything with its read(dst, n) -> bytes read (gtx_discover_run.hip reads a header out of members it holds)
enum BamHeaderRead { BAM_HEADER_OK, BAM_NOT_BAM, BAM_TRUNCATED };
template <class Reader>
inline BamHeaderRead read_bam_header(Reader & fp, BamHeader & h)
{
  auto rd = [&](void * d, size_t n) { return fp.read(d, n) == static_cast<long>(n); };
  char magic[4];
  int32_t l_text = 0, n_ref = 0;
  if (!rd(magic, 4) || std::memcmp(magic, "BAM\1", 4) != 0 || !rd(&l_text, 4) || l_text < 0)
    return BAM_NOT_BAM;
  h.text.assign(static_cast<size_t>(l_text), '\0');
  if ((l_text && !rd(&h.text[0], static_cast<size_t>(l_text))) || !rd(&n_ref, 4) || n_ref < 0)
    return BAM_TRUNCATED;
  h.refs.clear();
  for (int32_t i = 0; i < n_ref; ++i)
  {
    int32_t l_name = 0, l_ref = 0;
    std::string name;
    if (!rd(&l_name, 4) || l_name <= 0 || l_name > (1 << 20) || (name.resize(static_cast<size_t>(l_name)), !rd(&name[0], static_cast<size_t>(l_name))) ||
        !rd(&l_ref, 4))
      return BAM_TRUNCATED;
    name.resize(std::strlen(name.c_str()));
    h.refs.emplace_back(name, l_ref);
  }
  return BAM_HEADER_OK;
}

// the read groups and samples of a header's @RG lines (hts_reader.cpp:31-80: first "\tID:", last "\tSM:"); without an @RG line the
// one sample is the file name up to its first '.' (hts_reader.cpp:83-91)
struct BamSamples
{
  std::vector<std::string> samples;         // in header order
  std::map<std::string, uint32_t> rg2index; // read group id -> its index
  std::vector<uint32_t> rg2sample;          // -> index into samples
};

// false: an @RG line without ID or SM
inline bool read_bam_samples(std::string const & text, std::string const & path, BamSamples & s)
{
  size_t at = 0;
  while (at < text.size())
  {
    size_t const nl = std::min(text.find('\n', at), text.size());
    std::string const line = text.substr(at, nl - at);
    at = nl + 1;
    if (line.rfind("@RG", 0) != 0)
      continue;
    size_t const pid = line.find("\tID:"), psm = line.rfind("\tSM:");
    if (pid == std::string::npos || psm == std::string::npos)
      return false;
    size_t const eid = std::min(line.find('\t', pid + 1), line.size()), esm = std::min(line.find('\t', psm + 1), line.size());
    std::string const id = line.substr(pid + 4, eid - pid - 4), sm = line.substr(psm + 4, esm - psm - 4);
    s.rg2index[id] = static_cast<uint32_t>(s.rg2sample.size());
    auto it = std::find(s.samples.begin(), s.samples.end(), sm);
    s.rg2sample.push_back(static_cast<uint32_t>(it - s.samples.begin()));
    if (it == s.samples.end())
      s.samples.push_back(sm);
  }
  if (s.samples.empty())
  {
    std::string name = path.substr(path.rfind('/') + 1);
    if (name.find('.') != std::string::npos)
      name = name.substr(0, name.find('.'));
    s.samples.push_back(name);
  }
  return true;
}

// the next record's block (what follows its block_size) into buf
enum BamBlockRead { BAM_BLOCK_OK, BAM_BLOCK_END, BAM_BLOCK_DAMAGED };
inline BamBlockRead read_bam_block(Bgzf & fp, std::vector<uint8_t> & buf)
{
  int32_t block = 0;
  long const got = fp.read(&block, 4);
  if (got == 0)
    return BAM_BLOCK_END;
  if (got != 4 || block < 32)
    return BAM_BLOCK_DAMAGED;
  buf.resize(static_cast<size_t>(block));
  return fp.read(buf.data(), buf.size()) == static_cast<long>(buf.size()) ? BAM_BLOCK_OK : BAM_BLOCK_DAMAGED;
}

// the same behind what `stream` holds already, as the bytes lie in the file: the block_size word, then the block, read where it
// stays (gtx_disc_bam.cpp keeps a file's records so).  *at: where the block begins.  Not BAM_BLOCK_OK: `stream` is as it was.
inline BamBlockRead append_bam_block(Bgzf & fp, std::vector<uint8_t> & stream, size_t * at)
{
  size_t const before = stream.size();
  int32_t block = 0;
  long const got = fp.read(&block, 4);
  if (got == 0)
    return BAM_BLOCK_END;
  if (got != 4 || block < 32)
    return BAM_BLOCK_DAMAGED;
  stream.resize(before + 4 + static_cast<size_t>(block));
  std::memcpy(stream.data() + before, &block, 4);
  *at = before + 4;
  if (fp.read(stream.data() + *at, static_cast<size_t>(block)) == static_cast<long>(block))
    return BAM_BLOCK_OK;
  stream.resize(before);
  return BAM_BLOCK_DAMAGED;
}

struct BamCore
{
  int32_t tid, pos, l_seq, mtid, mpos, tlen;
  uint8_t l_read_name, mapq;
  uint16_t n_cigar, flag;
  size_t o_cigar, o_seq, o_qual, o_aux; // offsets in the block; the name is at 32
};

// false: the block is shorter than its own counts say (or l_seq is negative)
inline bool parse_bam_core(uint8_t const * p, size_t size, BamCore & c) // a block of `size` bytes (at least 32) at p
{
  std::memcpy(&c.tid, p, 4);
  std::memcpy(&c.pos, p + 4, 4);
  c.l_read_name = p[8];
  c.mapq = p[9];
  std::memcpy(&c.n_cigar, p + 12, 2);
  std::memcpy(&c.flag, p + 14, 2);
  std::memcpy(&c.l_seq, p + 16, 4);
  std::memcpy(&c.mtid, p + 20, 4);
  std::memcpy(&c.mpos, p + 24, 4);
  std::memcpy(&c.tlen, p + 28, 4);
  if (c.l_seq < 0)
    return false;
  c.o_cigar = 32 + static_cast<size_t>(c.l_read_name);
  c.o_seq = c.o_cigar + 4ull * c.n_cigar;
  c.o_qual = c.o_seq + (static_cast<size_t>(c.l_seq) + 1) / 2;
  c.o_aux = c.o_qual + static_cast<size_t>(c.l_seq);
  return c.o_aux <= size;
}
inline bool parse_bam_core(std::vector<uint8_t> const & buf, BamCore & c) { return parse_bam_core(buf.data(), buf.size(), c); }

// reference positions an alignment covers (bam_endpos: M, D, N, =, X consume the reference); cigar: n words of len << 4 | op,
// at any alignment.  What a span of zero or an unmapped read counts as is the caller's rule.
inline int64_t ref_span(void const * cigar, size_t n)
{
  int64_t span = 0;
  for (size_t c = 0; c < n; ++c)
  {
    uint32_t w;
    std::memcpy(&w, static_cast<uint8_t const *>(cigar) + 4 * c, 4);
    uint32_t const op = w & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8)
      span += w >> 4;
  }
  return span;
}
} // namespace gtx
