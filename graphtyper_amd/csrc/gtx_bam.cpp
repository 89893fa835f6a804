// gtx_bam.cpp -- BAM ingest in front of gtx_stream_push, host side, zlib only.
//
// What the reference does with htslib before a record reaches genotype_only():
//   HtsReader::open                      src/utilities/hts_reader.cpp:17-124   header, @RG -> (read group, sample) tables, region
//   HtsReader::get_next_read_in_order    hts_reader.cpp:166-303                records of one position sorted by (l_qseq, packed bases)
//   HtsParallelReader::open/read_record  src/utilities/hts_parallel_reader.cpp:66-136   k-way merge of the files by
//                                        (tid, pos, l_qseq, packed bases)       include/graphtyper/utilities/hts_utils.hpp:48-108
//   HtsReader::get_sample_and_rg_index   hts_reader.cpp:354-387                RG tag -> read group / sample index
//   get_score_diff                       src/typer/alignment.cpp:140-325       AS - XS from the aux fields, with its parsing quirks
// Here: BGZF members are inflated member by member (raw deflate; ahead of the reader by a team of worker threads,
// see Bgzf in gtx_bgzf.hpp); a BAM record is parsed in place into a
// gtx_stream_record + its packed bases (copied verbatim: the kernels read BAM nibbles).  Equal keys keep file order, then
// position in the file (the reference's std::sort / heap leave the order of exact duplicates unspecified; their results do
// not depend on it).  A region starts from the .bai or .csi when there is one (else the file is scanned from its head).  Not read:
// CRAM (needs htslib's codecs).
#include "gtx_bam_record.hpp"
#include "gtx_ctx.hpp"
#include "gtx_hts_index.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace gtx
{
namespace
{
// the .bai (SAM spec 5.2): bins of min_shift 14, depth 5 -- positions up to 2^29 -- and a linear index of 16 kb windows
bool bai_start(std::string const & bam_path, int32_t tid, int64_t begin, int64_t end, bool & any, uint64_t & voffset)
{
  std::FILE * fp = std::fopen((bam_path + ".bai").c_str(), "rb");
  if (!fp && bam_path.size() > 4)
    fp = std::fopen((bam_path.substr(0, bam_path.size() - 4) + ".bai").c_str(), "rb");
  if (!fp)
    return false;
  std::string raw;
  char block[1 << 16];
  for (size_t n; (n = std::fread(block, 1, sizeof block, fp)) > 0;)
    raw.append(block, n);
  std::fclose(fp);
  IndexCursor c{raw.data(), raw.size()};
  uint32_t const magic = c.get<uint32_t>();
  int32_t const n_ref = c.get<int32_t>();
  if (!c.ok || std::memcmp(&magic, "BAI\1", 4) != 0 || tid < 0 || tid >= n_ref)
    return false;
  return index_start(c, IndexGeometry{14, 5, false}, tid, begin, std::min<int64_t>(end, 1ll << 29) - 1, any, voffset);
}

// the .csi: htslib's coordinate-sorted index with a free bin geometry (min_shift, depth) and an offset per bin in place of
// the linear index; the file is BGZF-compressed.  Any l_aux is taken (a BAM file's index has none).
bool csi_start(std::string const & bam_path, int32_t tid, int64_t begin, int64_t end, bool & any, uint64_t & voffset)
{
  Bgzf z;
  if (!z.open(bam_path + ".csi") && !(bam_path.size() > 4 && z.open(bam_path.substr(0, bam_path.size() - 4) + ".csi")))
    return false;
  std::string raw;
  z.read_rest(raw);
  IndexCursor c{raw.data(), raw.size()};
  uint32_t const magic = c.get<uint32_t>();
  int32_t const min_shift = c.get<int32_t>(), depth = c.get<int32_t>(), l_aux = c.get<int32_t>();
  if (!c.ok || std::memcmp(&magic, "CSI\1", 4) != 0 || min_shift < 0 || min_shift > 32 || depth < 0 || depth > 10 || l_aux < 0 || l_aux >= (1 << 24) ||
      c.n - c.at < static_cast<size_t>(l_aux))
    return false;
  c.at += static_cast<size_t>(l_aux);
  int32_t const n_ref = c.get<int32_t>();
  if (!c.ok || tid < 0 || tid >= n_ref)
    return false;
  int64_t const max_pos = 1ll << std::min(62, min_shift + 3 * depth);
  return index_start(c, IndexGeometry{min_shift, depth, true}, tid, begin, std::min<int64_t>(end, max_pos) - 1, any, voffset);
}
} // namespace

bool bam_index_start(std::string const & bam_path, int32_t tid, int64_t begin, int64_t end, bool & any, uint64_t & voffset)
{
  return bai_start(bam_path, tid, begin, end, any, voffset) || csi_start(bam_path, tid, begin, end, any, voffset);
}
} // namespace gtx

namespace
{
using gtx::Bgzf;

struct Rec // one BAM record as the merge needs it
{
  gtx_stream_record r{};
  std::vector<uint8_t> seq; // (l_qseq + 1) / 2 bytes
  int64_t end_pos = 0;      // first reference position behind the alignment
};

// gt_pos_seq_same_pos / gt_pos_seq (hts_utils.hpp:48-108) as "a comes before b"
bool seq_before(Rec const & a, Rec const & b)
{
  if (a.r.l_qseq != b.r.l_qseq)
    return a.r.l_qseq < b.r.l_qseq;
  return a.seq < b.seq; // bytewise, equal lengths
}

bool record_before(Rec const & a, Rec const & b)
{
  if (a.r.tid != b.r.tid)
    return a.r.tid < b.r.tid;
  if (a.r.pos != b.r.pos)
    return a.r.pos < b.r.pos;
  return seq_before(a, b);
}

uint64_t name_hash(char const * s, size_t n) // identity of a read name: 64-bit FNV-1a
{
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i)
    h = (h ^ static_cast<uint8_t>(s[i])) * 1099511628211ull;
  return h;
}

struct File
{
  Bgzf fp;
  std::string path;
  std::vector<std::string> ref_names;
  std::vector<std::string> samples;          // of this file, in header order
  std::map<std::string, uint32_t> rg2index;  // read group id -> index in this file
  std::vector<uint32_t> rg2sample;           // -> sample index in this file
  uint32_t sample_offset = 0, rg_offset = 0;
  // region (by scanning): records of contig `want_tid` that overlap [begin, end)
  int32_t want_tid = -2;
  int64_t begin = 0, end = INT64_MAX;
  bool eof = false;
  bool indexed = false;        // the scan started from the .bai
  Rec ahead;                   // the first record of the next position
  bool have_ahead = false;
  std::deque<Rec> same_pos;    // the records of the current position, in order
  std::vector<uint8_t> buf;

  bool read_exact(void * dst, unsigned n)
  {
    return fp.read(dst, n) == static_cast<long>(n);
  }

  uint32_t num_rg() const { return std::max<uint32_t>(1, static_cast<uint32_t>(rg2sample.size())); }

  // alignment.cpp:140-325
  static uint8_t score_diff(uint8_t const * it, uint32_t l_aux)
  {
    uint32_t i = 0;
    int64_t as = -1, xs = -1;
    auto load = [&](auto tag, bool is_as, bool is_xs)
    {
      decltype(tag) num = 0;
      if (i + sizeof(num) > l_aux) // (a truncated aux area: the reference reads on into htslib's padding; here the field is not there)
      {
        i = l_aux;
        return;
      }
      std::memcpy(&num, it + i, sizeof(num));
      if (is_as)
        as = num;
      else if (is_xs)
        xs = num;
      i += sizeof(num);
    };
    while (i < l_aux)
    {
      i += 3;
      if (i > l_aux)
        break;
      char const type = static_cast<char>(it[i - 1]);
      bool const is_s = it[i - 2] == 'S', is_as = is_s && it[i - 3] == 'A', is_xs = is_s && it[i - 3] == 'X';
      switch (type)
      {
      case 'A': ++i; break;
      case 'Z':
        while (i < l_aux && it[i] != '\0' && it[i] != '\n')
          ++i;
        ++i;
        break;
      case 'c': load(int8_t(), is_as, is_xs); break;
      case 'C': load(uint8_t(), is_as, is_xs); break;
      case 's': load(int16_t(), is_as, is_xs); break;
      case 'S': load(uint16_t(), is_as, is_xs); break;
      case 'i': load(int32_t(), is_as, is_xs); break;
      case 'I': load(uint32_t(), is_as, is_xs); break;
      case 'f': i += 4; break;
      default: i = l_aux; break; // unknown tag type: the reference stops here
      }
    }
    if (as == -1 || as < xs)
      return 0;
    if (xs == -1)
      xs = 0;
    int64_t const diff = as - xs;
    return diff < 255 ? static_cast<uint8_t>(diff) : 255;
  }

  // bam_aux_get(rec, "RG"): htslib walks the fields by their types
  static bool find_rg(uint8_t const * aux, uint32_t l_aux, std::string & out)
  {
    uint64_t i = 0; // (64 bits: a hostile 'B' count must not wrap the cursor back into the area)
    while (i + 3 <= l_aux)
    {
      char const t0 = static_cast<char>(aux[i]), t1 = static_cast<char>(aux[i + 1]), type = static_cast<char>(aux[i + 2]);
      i += 3;
      uint64_t size = 0;
      switch (type)
      {
      case 'A': case 'c': case 'C': size = 1; break;
      case 's': case 'S': size = 2; break;
      case 'i': case 'I': case 'f': size = 4; break;
      case 'd': size = 8; break;
      case 'Z': case 'H':
      {
        uint64_t j = i;
        while (j < l_aux && aux[j] != '\0')
          ++j;
        if (t0 == 'R' && t1 == 'G' && type == 'Z')
        {
          out.assign(reinterpret_cast<char const *>(aux + i), j - i);
          return true;
        }
        size = j - i + 1;
        break;
      }
      case 'B':
      {
        if (i + 5 > l_aux)
          return false;
        char const sub = static_cast<char>(aux[i]);
        uint32_t n;
        std::memcpy(&n, aux + i + 1, 4);
        uint64_t const w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
        size = 5 + static_cast<uint64_t>(n) * w;
        break;
      }
      default: return false;
      }
      if (i + size > l_aux) // a field that runs past the aux area: malformed record, no read group
        return false;
      i += size;
    }
    return false;
  }

  // next record of the file that lies in the region; false at the end of the file (or behind the region)
  bool read_one(Rec & out, std::string & err)
  {
    auto stop = [&](char const * what) // (false: nothing more comes from this file)
    {
      if (what)
        err = path + what;
      eof = true;
      return false;
    };
    for (;;)
    {
      if (eof)
        return false;
      gtx::BamBlockRead const got = gtx::read_bam_block(fp, buf);
      if (got != gtx::BAM_BLOCK_OK)
        return stop(got == gtx::BAM_BLOCK_END ? nullptr : ": truncated BAM record");
      gtx::BamCore c;
      if (!gtx::parse_bam_core(buf, c))
        return stop(": malformed BAM record");
      uint8_t const * p = buf.data();
      // the first reference position behind the alignment (bam_endpos: at least one position)
      int64_t const span = gtx::ref_span(p + c.o_cigar, c.n_cigar);
      int64_t const end_pos = static_cast<int64_t>(c.pos) + (span > 0 ? span : 1);
      if (want_tid != -2)
      {
        if (c.tid != want_tid || end_pos <= begin)
        {
          if (c.tid > want_tid && c.tid >= 0 && want_tid >= 0)
            return stop(nullptr); // sorted file: behind the contig
          continue;
        }
        if (c.pos >= end)
          return stop(nullptr);
      }
      if (c.l_seq > 0xFFFF)
        return stop(": a read of more than 65535 bases");
      out.r = gtx_stream_record{};
      out.r.flag = c.flag;
      out.r.mapq = c.mapq;
      out.r.tid = c.tid;
      out.r.mtid = c.mtid;
      out.r.pos = c.pos;
      out.r.isize = c.tlen;
      out.r.l_qseq = static_cast<uint16_t>(c.l_seq);
      out.r.mpos = c.mpos;
      out.r.n_cigar = c.n_cigar;
      if (c.n_cigar)
      {
        std::memcpy(&out.r.cigar_front, p + c.o_cigar, 4);
        std::memcpy(&out.r.cigar_back, p + c.o_seq - 4, 4);
      }
      out.r.name_id = name_hash(reinterpret_cast<char const *>(p + 32), c.l_read_name ? c.l_read_name - 1u : 0u);
      uint32_t const l_aux = static_cast<uint32_t>(buf.size() - c.o_aux);
      out.r.score_diff = score_diff(p + c.o_aux, l_aux);
      uint32_t rg = 0, sample = 0;
      if (rg2sample.size() > 1) // hts_reader.cpp:354-387
      {
        std::string id;
        if (!find_rg(p + c.o_aux, l_aux, id))
          return stop(": a record without RG tag in a file with several read groups");
        auto it = rg2index.find(id);
        if (it == rg2index.end())
          return stop((": unknown read group " + id).c_str());
        rg = it->second;
        sample = rg2sample[rg];
      }
      out.r.rg = static_cast<uint16_t>(rg + rg_offset);
      out.r.sample = sample + sample_offset;
      out.seq.assign(p + c.o_seq, p + c.o_qual);
      out.end_pos = end_pos;
      return true;
    }
  }

  // HtsReader::get_next_read_in_order: the records of one position (the reference compares core.pos only), sorted
  bool next(Rec & out, std::string & err)
  {
    if (same_pos.empty())
    {
      if (!have_ahead)
        have_ahead = read_one(ahead, err);
      if (!have_ahead)
        return false;
      int32_t const pos = ahead.r.pos;
      std::vector<Rec> group;
      group.push_back(std::move(ahead));
      have_ahead = false;
      Rec r;
      while (read_one(r, err))
      {
        if (r.r.pos != pos)
        {
          ahead = std::move(r);
          have_ahead = true;
          break;
        }
        group.push_back(std::move(r));
        r = Rec();
      }
      std::stable_sort(group.begin(), group.end(), seq_before);
      for (auto & g : group)
        same_pos.push_back(std::move(g));
    }
    out = std::move(same_pos.front());
    same_pos.pop_front();
    return true;
  }
};
} // namespace

struct gtx_reads
{
  std::vector<std::unique_ptr<File>> files;
  std::vector<std::string> samples;
  uint32_t n_rg = 0;
  // merge front: one record per file that still has some
  std::vector<std::pair<Rec, uint32_t>> front;
  std::string error;
  uint32_t refused_len = 0; // bases of the read the last gtx_reads_next stopped at for want of seq_stride (0: none)
};

namespace
{
int fail(gtx_reads * r, std::string const & msg, int status)
{
  gtx::g_last_error = msg;
  delete r;
  return status;
}
} // namespace

extern "C" int gtx_reads_open(const char * const * bam_paths, uint32_t n_paths, const char * region, gtx_reads ** out)
{
  if (!bam_paths || n_paths == 0 || !out)
    return GTX_ERR_ARG;
  *out = nullptr;
  auto * r = new gtx_reads();
  // "chr", "chr:begin", "chr:begin-end" (1-based, inclusive like a samtools region); "" / "." / NULL: everything
  std::string contig;
  int64_t begin = 0, end = INT64_MAX;
  bool const whole = !region || std::strlen(region) <= 1;
  if (!whole)
  {
    std::string const s(region);
    size_t const colon = s.rfind(':');
    contig = s.substr(0, colon);
    if (colon != std::string::npos)
    {
      std::string rest = s.substr(colon + 1);
      rest.erase(std::remove(rest.begin(), rest.end(), ','), rest.end());
      size_t const dash = rest.find('-');
      begin = std::max<int64_t>(0, std::atoll(rest.substr(0, dash).c_str()) - 1);
      if (dash != std::string::npos && dash + 1 < rest.size())
        end = std::atoll(rest.substr(dash + 1).c_str());
    }
  }
  for (uint32_t f = 0; f < n_paths; ++f)
  {
    auto file = std::make_unique<File>();
    file->path = bam_paths[f] ? bam_paths[f] : "";
    if (!file->fp.open(file->path))
      return fail(r, "could not open " + file->path, GTX_ERR_IO);
    gtx::BamHeader head;
    gtx::BamHeaderRead const got = gtx::read_bam_header(file->fp, head);
    if (got == gtx::BAM_NOT_BAM)
      return fail(r, file->path + " is not a BAM file (CRAM is not read)", GTX_ERR_UNSUPPORTED);
    if (got == gtx::BAM_TRUNCATED)
      return fail(r, file->path + ": truncated header", GTX_ERR_IO);
    for (auto const & ref : head.refs)
      file->ref_names.push_back(ref.first);
    // @RG lines -> read groups and samples
    gtx::BamSamples table;
    if (!gtx::read_bam_samples(head.text, file->path, table))
      return fail(r, file->path + ": an @RG line without ID or SM", GTX_ERR_ARG);
    file->samples.swap(table.samples);
    file->rg2index.swap(table.rg2index);
    file->rg2sample.swap(table.rg2sample);
    if (!whole)
    {
      auto it = std::find(file->ref_names.begin(), file->ref_names.end(), contig);
      if (it == file->ref_names.end())
      {
        return fail(r, file->path + ": no contig " + contig, GTX_ERR_ARG);
      }
      file->want_tid = static_cast<int32_t>(it - file->ref_names.begin());
      file->begin = begin;
      file->end = end;
      // with a .bai the scan starts at the first place an overlapping record can be, else behind the header
      bool any = false;
      uint64_t voffset = 0;
      if (gtx::bam_index_start(file->path, file->want_tid, begin, end, any, voffset))
      {
        file->indexed = true;
        if (!any)
          file->eof = true; // the index knows of no record there
        else if (!file->fp.seek(voffset))
          return fail(r, file->path + ": the index points outside the file", GTX_ERR_IO);
      }
    }
    file->sample_offset = static_cast<uint32_t>(r->samples.size());
    file->rg_offset = r->n_rg;
    r->samples.insert(r->samples.end(), file->samples.begin(), file->samples.end());
    r->n_rg += file->num_rg();
    r->files.push_back(std::move(file));
  }
  for (uint32_t f = 0; f < r->files.size(); ++f)
  {
    Rec rec;
    if (r->files[f]->next(rec, r->error))
      r->front.emplace_back(std::move(rec), f);
    if (!r->error.empty())
    {
      std::string const e = r->error;
      return fail(r, e, GTX_ERR_IO);
    }
  }
  *out = r;
  return GTX_OK;
}

extern "C" int gtx_reads_set_inflate_device(gtx_reads * r, int device)
{
  if (!r)
  {
    gtx::g_last_error = "gtx_reads_set_inflate_device: bad argument";
    return GTX_ERR_ARG;
  }
  for (auto & f : r->files)
  {
    int const rc = f->fp.use_device(device);
    if (rc != GTX_OK)
      return rc; // (the files before this one stay with the device, the others with the host: every one of them reads on)
  }
  return GTX_OK;
}

extern "C" int gtx_reads_inflate_counts(uint64_t * by_device, uint64_t * fell_back, uint64_t * by_reader)
{
  gtx::InflateCounts const n = gtx::inflate_counts();
  if (by_device)
    *by_device = n.by_device;
  if (fell_back)
    *fell_back = n.fell_back;
  if (by_reader)
    *by_reader = n.by_reader;
  return GTX_OK;
}

extern "C" int gtx_reads_info(const gtx_reads * r, uint32_t * n_samples, uint32_t * n_read_groups)
{
  if (!r)
    return GTX_ERR_ARG;
  if (n_samples)
    *n_samples = static_cast<uint32_t>(r->samples.size());
  if (n_read_groups)
    *n_read_groups = r->n_rg;
  return GTX_OK;
}

extern "C" const char * gtx_reads_sample_name(const gtx_reads * r, uint32_t i)
{
  return r && i < r->samples.size() ? r->samples[i].c_str() : nullptr;
}

extern "C" int gtx_reads_next(gtx_reads * r, gtx_stream_record * recs, uint8_t * seq, uint32_t seq_stride, uint32_t cap, uint32_t * n)
{
  if (!r || !recs || !seq || !n)
    return GTX_ERR_ARG;
  *n = 0;
  r->refused_len = 0;
  while (*n < cap && !r->front.empty())
  {
    // the smallest record; equal keys: the file that was opened first
    size_t best = 0;
    for (size_t i = 1; i < r->front.size(); ++i)
      if (record_before(r->front[i].first, r->front[best].first))
        best = i;
    Rec & rec = r->front[best].first;
    if (rec.seq.size() > seq_stride)
    {
      r->refused_len = rec.r.l_qseq;
      gtx::g_last_error = "gtx_reads_next: a read does not fit in seq_stride";
      return GTX_ERR_ARG;
    }
    recs[*n] = rec.r;
    uint8_t * row = seq + static_cast<size_t>(*n) * seq_stride;
    std::memcpy(row, rec.seq.data(), rec.seq.size());
    std::memset(row + rec.seq.size(), 0, seq_stride - rec.seq.size());
    ++*n;
    uint32_t const f = r->front[best].second;
    Rec next;
    if (r->files[f]->next(next, r->error))
      r->front[best].first = std::move(next);
    else
      r->front.erase(r->front.begin() + static_cast<long>(best));
    if (!r->error.empty())
    {
      gtx::g_last_error = r->error;
      return GTX_ERR_IO;
    }
  }
  return GTX_OK;
}

uint32_t gtx::reads_refused_len(gtx_reads const * r) { return r ? r->refused_len : 0; }

extern "C" void gtx_reads_close(gtx_reads * r)
{
  if (!r)
    return;
  delete r;
}
