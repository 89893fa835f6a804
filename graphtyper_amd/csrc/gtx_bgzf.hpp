// gtx_bgzf.hpp -- the BGZF layer of the file readers and writers (host): the one parser of a member's header, the one host
// inflate of a member, the reader with its inflating teams (gtx_bgzf.cpp).  BGZF: a series of gzip members of at most 64 KB,
// each with its compressed size in a "BC" extra subfield (SAM spec 4.1); a virtual offset = (file offset of a member) << 16 |
// offset in its data.
#pragma once
#include "../../include/gtx.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gtx
{
struct BgzfMember
{
  uint32_t hlen = 0, xlen = 0; // the header's length (12 + XLEN) and XLEN
  uint32_t bsize = 0;          // BSIZE: the whole member's length - 1
  long clen = 0;               // compressed bytes between the header and CRC32 / ISIZE
  bool bc_first = false;       // BC is the first extra subfield, as in every writer there is
  bool whole = false;          // the range held the whole member: crc32 and isize are those of its last 8 bytes
  uint32_t crc32 = 0, isize = 0;
};

// The member that begins at h, of which n bytes are there (at least its header: 12 + XLEN bytes).  nullptr, or why the bytes
// are not a member.  The extra subfields are walked: BC need not be the first.  "truncated" (the extra field ends behind the
// range) leaves hlen and xlen set: a reader that has the first 18 bytes learns from them how many more the header needs.
inline char const * parse_bgzf_member(uint8_t const * h, uint64_t n, BgzfMember & m)
{
  m = BgzfMember{};
  if (n < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4))
    return "not a BGZF member";
  m.xlen = h[10] | (h[11] << 8);
  m.hlen = 12 + m.xlen;
  if (n < m.hlen)
    return "truncated";
  long bsize = -1;
  for (uint32_t i = 0; i + 4 <= m.xlen;)
  {
    uint8_t const * x = h + 12 + i;
    uint32_t const slen = x[2] | (x[3] << 8);
    if (x[0] == 'B' && x[1] == 'C' && slen == 2 && i + 6 <= m.xlen)
    {
      bsize = x[4] | (x[5] << 8);
      m.bc_first = i == 0;
    }
    i += 4 + slen;
  }
  m.clen = bsize + 1 - static_cast<long>(m.hlen) - 8;
  if (bsize < 0 || m.clen < 0)
    return "no BC field";
  m.bsize = static_cast<uint32_t>(bsize);
  if (n < m.bsize + 1ull)
    return nullptr;
  m.whole = true;
  std::memcpy(&m.crc32, h + m.hlen + m.clen, 4);
  std::memcpy(&m.isize, h + m.hlen + m.clen + 4, 4);
  return m.isize > 65536 ? "ISIZE beyond 65536" : nullptr; // (a damaged ISIZE must not size an allocation)
}

// The next member of a file: its header into m, and what follows the header -- m.clen compressed bytes, CRC32, ISIZE -- into
// `rest`.  MEMBER_END: the file ends in front of it; MEMBER_BROKEN: it is malformed or cut.
enum MemberRead { MEMBER_OK, MEMBER_END, MEMBER_BROKEN };
MemberRead read_bgzf_member(std::FILE * fp, BgzfMember & m, std::vector<uint8_t> & rest);

// One member inflated on the host: the library's own decoder (gtx_inflate.hpp: built for whole members of known size, 1.5-1.9 x
// zlib's rate; use_own), the member's CRC32 (check_crc: htslib compares it, and it is what holds the decoder here to the
// file), and zlib's verdict on what those two refuse -- a damaged member, or a code whose tables do not fit the decoder's fixed
// ones.  `rest` as read_bgzf_member leaves it (the own decoder loads 8 bytes at a time: CRC32 and ISIZE are there); out: isize bytes.
bool inflate_bgzf_member(uint8_t const * rest, size_t clen, uint8_t * out, size_t isize, bool use_own, bool check_crc);

struct InflateJob;

// what became of the members of readers that asked for the device (process-wide, gtx_reads_inflate_counts)
struct InflateCounts
{
  uint64_t by_device, fell_back, by_reader;
};
InflateCounts inflate_counts();

// The reader.  Members are inflated one at a time (raw deflate), which is what makes seeking by virtual offset possible -- and
// what makes them independent: inflating is nine tenths of the time of reading a BAM file, so a reader keeps up to RING members
// in flight (refilled by halves).  The calling thread reads the compressed members ahead (sequential file reads), a small team
// of worker threads shared by all open readers inflates them, and the caller takes them in file order; a member nobody has
// started on when the caller needs it is inflated by the caller itself, so a reader is never slower than without the team (many
// readers on many host threads each still get their own core).  The team lives while a reader is open (GTX_BGZF_THREADS sizes
// it, 0 = none).  GTX_INFLATE=zlib: zlib only; GTX_BGZF_CRC=0: the members' CRC32 is not compared.
class Bgzf
{
public:
  Bgzf();
  ~Bgzf();
  bool open(std::string const & path);
  void close();
  bool is_open() const { return fp_ != nullptr; }
  // reads n bytes; returns the number read (short at the end of the file), -1 on a malformed member
  long read(void * dst, size_t n);
  // appends everything from here to the end of the file, or to the first malformed member
  void read_rest(std::string & out);
  bool seek(uint64_t voffset);
  // From here on the members go to the device's team, and the reader keeps more of them in flight: a launch wants thousands of
  // members from all readers together, not 32 from each.  What has been read ahead stays, in order.  0 or a gtx status.
  int use_device(int device);

private:
  static constexpr unsigned RING = 32; // members in flight per reader (2 MB of data at most)
  MemberRead read_member(InflateJob & j);
  void fill();
  bool next_block();
  void finish(InflateJob & j) const;
  void drain();
  std::FILE * fp_ = nullptr;
  std::unique_ptr<InflateJob[]> ring_;
  uint64_t ring_n_ = RING;       // RING, or what use_device chose
  bool on_device_ = false;       // the members go to the device's team
  std::vector<InflateJob *> fresh_;
  uint64_t head_ = 0, tail_ = 0; // members taken / read ahead
  MemberRead ahead_ = MEMBER_OK; // what the last look ahead found
  std::vector<uint8_t> data_;
  size_t at_ = 0;
  bool bad_ = false;
};
} // namespace gtx
