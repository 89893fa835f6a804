// gtx_disc_variants.cpp -- discovery behind its second pass: the variant records (streamlined_discovery, src/typer/caller.cpp:2985-3092,
// through Variant::add_base_in_front, src/typer/variant.cpp:1135-1167, over Graph::get_generated_reference_genome,
// src/graph/graph.cpp:409-435) and the text of iteration 1's sites file (Vcf::write_records, src/typer/vcf.cpp:1161-1275, and
// Vcf::write_record for a file without samples, :767-1015).  Host code: a region of 50 kb has a few hundred events, and the loop
// over the map is sequential in its event index.  Plain C++ with no HIP header (tests/emu_disc_variants compiles this file alone,
// with the sanitizers); the region's letters come through gtx_disc_region.hpp.
#include "../../include/gtx.h"
#include "gtx_disc_region.hpp"
#include "gtx_vcf_text.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace
{
using namespace gtx;

using Key = std::tuple<uint32_t, uint8_t, std::string>; // an Event: only equality and a lookup are needed here, the words carry the map's order

struct Hap // one entry of the haplotype map
{
  Key ev;
  std::set<Key> ever, always;
};

struct Merged
{
  std::map<Key, bool> indels; // -> has_indel_good_support, good_bits applied
  std::vector<Hap> haplotypes;
};

int bad(char const * what)
{
  g_last_error = what;
  return GTX_ERR_ARG;
}

// the words of gtx_disc_merge (gtx.h: n_indels, per indel the event, 15 support fields, file_index, its phase entries; n_events, per
// event its "ever" and "always" sets)
bool read_words(uint32_t const * w, uint64_t n, uint32_t const * good_bits, Merged & r)
{
  uint64_t at = 0;
  bool ok = true;
  auto word = [&]() -> uint32_t
  {
    if (at >= n)
    {
      ok = false;
      return 0;
    }
    return w[at++];
  };
  auto event = [&]() -> Key
  {
    uint32_t const pos = word();
    uint32_t const type = word();
    uint32_t const len = word();
    std::string seq;
    if (!ok || len > n - at || (type != 'X' && type != 'I' && type != 'D'))
    {
      ok = false;
      return Key();
    }
    for (uint32_t k = 0; k < len; ++k)
      seq.push_back(static_cast<char>(w[at + k]));
    at += len;
    return Key(pos, static_cast<uint8_t>(type), std::move(seq));
  };
  if (n == 0)
    return true;
  for (uint32_t t = 0, m = word(); ok && t < m; ++t)
  {
    Key e = event();
    if (!ok || at + 17 > n || std::get<1>(e) == 'X')
      return false;
    bool const good = w[at + 13] != 0 || (good_bits && ((good_bits[t >> 5] >> (t & 31u)) & 1u) != 0);
    at += 16;
    for (uint32_t k = 0, np = word(); ok && k < np; ++k)
    {
      (void)event();
      (void)word();
    }
    r.indels.insert({std::move(e), good});
  }
  for (uint32_t i = 0, m = word(); ok && i < m; ++i)
  {
    Hap h;
    h.ev = event();
    for (std::set<Key> * set : {&h.ever, &h.always})
      for (uint32_t k = 0, ns = word(); ok && k < ns; ++k)
        set->insert(event());
    if (ok && std::get<1>(h.ev) == 'X' && std::get<2>(h.ev).size() != 1)
      ok = false;
    r.haplotypes.push_back(std::move(h));
  }
  return ok && at == n;
}

struct Alleles
{
  std::pair<char const *, uint32_t> ref, alt;
};

Alleles alleles_of(gtx_disc_variant const & v, char const * letters) { return {{letters + v.ref_off, v.ref_len}, {letters + v.alt_off, v.alt_len}}; }

int compare_letters(std::pair<char const *, uint32_t> const & a, std::pair<char const *, uint32_t> const & b) // std::vector<char>'s order
{
  uint32_t const m = std::min(a.second, b.second);
  for (uint32_t k = 0; k < m; ++k)
    if (a.first[k] != b.first[k])
      return a.first[k] < b.first[k] ? -1 : 1;
  return a.second < b.second ? -1 : a.second > b.second ? 1 : 0;
}

void put_ids(std::string & text, char const * key, uint32_t const * ids, uint32_t n)
{
  if (n == 0)
    return;
  text += key;
  for (uint32_t k = 0; k < n; ++k)
  {
    text += k ? ',' : '=';
    put_u(text, ids[k]);
  }
  text += ';';
}
} // namespace

extern "C" int gtx_disc_variants(const gtx_disc * d, const uint32_t * words, uint64_t n_words, const uint32_t * good_bits, gtx_disc_variant * out, uint32_t cap,
                                 uint32_t * n, char * letters, uint64_t letters_cap, uint64_t * n_letters, uint32_t * ids, uint64_t ids_cap, uint64_t * n_ids)
{
  if (!d || !n || !n_letters || !n_ids || (n_words && !words) || (cap && !out) || (letters_cap && !letters) || (ids_cap && !ids))
    return bad("gtx_disc_variants: bad argument");
  *n = 0;
  *n_letters = 0;
  *n_ids = 0;
  Merged m;
  if (!read_words(words, n_words, good_bits, m))
    return bad("gtx_disc_variants: not a result of gtx_disc_merge");
  char const * reference = nullptr;
  uint64_t reference_len = 0;
  int64_t region_begin = 0;
  disc_region(d, &reference, &reference_len, &region_begin);
  long constexpr BUCKET_SIZE = 50; // caller.cpp:2764; the window of :3046 does not follow the bucket size of the passes
  // :2992-3000 and :3050-3058: an indel the table does not hold, or holds without good support, is no event and no next event
  std::vector<uint8_t> kept(m.haplotypes.size());
  for (size_t i = 0; i < m.haplotypes.size(); ++i)
  {
    Key const & e = m.haplotypes[i].ev;
    auto const it = std::get<1>(e) == 'X' ? m.indels.end() : m.indels.find(e);
    kept[i] = std::get<1>(e) == 'X' || (it != m.indels.end() && it->second);
  }
  std::vector<gtx_disc_variant> recs;
  std::string all_letters;
  std::vector<uint32_t> all_ids;
  for (size_t i = 0; i < m.haplotypes.size(); ++i) // event_index = i + 1: every event of the map counts, skipped ones included (:2987)
  {
    if (!kept[i])
      continue;
    Hap const & h = m.haplotypes[i];
    int64_t const pos = std::get<0>(h.ev);
    uint8_t const type = std::get<1>(h.ev);
    std::string const & seq = std::get<2>(h.ev);
    gtx_disc_variant v{};
    v.type = type;
    v.gt_id = static_cast<uint32_t>(i + 1);
    v.pos = static_cast<uint32_t>(pos);
    std::string ref_allele, alt_allele;
    if (type == 'X')
    {
      if (pos < region_begin || static_cast<uint64_t>(pos - region_begin) >= reference_len) // (the asserts of :3006-3007)
        return bad("gtx_disc_variants: an SNP outside the region");
      ref_allele.assign(1, reference[pos - region_begin]);
      alt_allele = seq;
    }
    else
    {
      (type == 'I' ? alt_allele : ref_allele) = seq;
      // add_base_in_front(true) over the reference-only graph of the region, in 1-based contig positions (variant.cpp:1137-1143,
      // graph.cpp:412-434): the base [pos, pos + 1) clamped to [region_begin + 1, region_begin + 1 + size); anything but one base left
      // -- the indel at the region's first base, or behind its end -- and the function returns false: no base, the position stays
      int64_t const first = region_begin + 1, from = std::max<int64_t>(first, pos), to = std::min<int64_t>(first + static_cast<int64_t>(reference_len), pos + 1);
      if (to - from == 1 && from == pos && to == pos + 1)
      {
        char base = reference[from - first];
        if (base != 'A' && base != 'C' && base != 'G' && base != 'T')
          base = 'N';
        ref_allele.insert(ref_allele.begin(), base);
        alt_allele.insert(alt_allele.begin(), base);
        v.pos = static_cast<uint32_t>(pos - 1);
      }
    }
    v.ref_off = static_cast<uint32_t>(all_letters.size());
    v.ref_len = static_cast<uint32_t>(ref_allele.size());
    all_letters += ref_allele;
    v.alt_off = static_cast<uint32_t>(all_letters.size());
    v.alt_len = static_cast<uint32_t>(alt_allele.size());
    all_letters += alt_allele;
    std::vector<uint32_t> hap, anti;
    for (size_t j = i + 1; j < m.haplotypes.size(); ++j) // :3042-3080
    {
      Key const & next = m.haplotypes[j].ev;
      if (static_cast<int64_t>(std::get<0>(next)) >= pos + 2 * BUCKET_SIZE)
        break;
      if (!kept[j])
        continue;
      if (h.always.count(next))
        hap.push_back(static_cast<uint32_t>(j + 1));
      else if (!h.ever.count(next))
        anti.push_back(static_cast<uint32_t>(j + 1));
    }
    v.hap_off = static_cast<uint32_t>(all_ids.size());
    v.n_hap = static_cast<uint32_t>(hap.size());
    all_ids.insert(all_ids.end(), hap.begin(), hap.end());
    v.anti_off = static_cast<uint32_t>(all_ids.size());
    v.n_anti = static_cast<uint32_t>(anti.size());
    all_ids.insert(all_ids.end(), anti.begin(), anti.end());
    if (all_letters.size() > 0xFFFFFFFFull || all_ids.size() > 0xFFFFFFFFull)
      return bad("gtx_disc_variants: more than 2^32 letters or ids");
    recs.push_back(v);
  }
  *n = static_cast<uint32_t>(recs.size());
  *n_letters = all_letters.size();
  *n_ids = all_ids.size();
  if (recs.size() > cap || all_letters.size() > letters_cap || all_ids.size() > ids_cap)
    return GTX_ERR_CAPACITY;
  std::copy(recs.begin(), recs.end(), out);
  std::copy(all_letters.begin(), all_letters.end(), letters);
  std::copy(all_ids.begin(), all_ids.end(), ids);
  return GTX_OK;
}

extern "C" int gtx_disc_vcf_sites(const gtx_disc_variant * v, uint32_t n, const char * letters, uint64_t n_letters, const uint32_t * ids, uint64_t n_ids,
                                  const char * contig, char * out, uint64_t cap, uint64_t * len)
{
  if (!len || !contig || (n && !v) || (n_letters && !letters) || (n_ids && !ids) || (cap && !out))
    return bad("gtx_disc_vcf_sites: bad argument");
  *len = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (v[i].ref_off > n_letters || v[i].ref_len > n_letters - v[i].ref_off || v[i].alt_off > n_letters || v[i].alt_len > n_letters - v[i].alt_off ||
        v[i].hap_off > n_ids || v[i].n_hap > n_ids - v[i].hap_off || v[i].anti_off > n_ids || v[i].n_anti > n_ids - v[i].anti_off)
      return bad("gtx_disc_vcf_sites: a record reaches behind the letters or the ids");
  auto n_infos = [&](uint32_t i) { return 1u + (v[i].n_hap != 0) + (v[i].n_anti != 0); };
  // compare_variants (vcf.cpp:1174-1214): position; SNP, insertion, deletion; REF shorter, REF longer, equal lengths; the alleles; the
  // record with more INFO keys first.  (std::sort there: no two records of one region are equal in all of these; stable here)
  auto less = [&](uint32_t i, uint32_t j)
  {
    gtx_disc_variant const & a = v[i];
    gtx_disc_variant const & b = v[j];
    if (a.pos != b.pos)
      return a.pos < b.pos;
    int const order_a = (a.type == 'I') + 2 * (a.type == 'D'), order_b = (b.type == 'I') + 2 * (b.type == 'D');
    if (order_a != order_b)
      return order_a < order_b;
    int const a_vt = (a.ref_len > a.alt_len) + 2 * (a.ref_len == a.alt_len), b_vt = (b.ref_len > b.alt_len) + 2 * (b.ref_len == b.alt_len);
    if (a_vt != b_vt)
      return a_vt < b_vt;
    Alleles const x = alleles_of(a, letters), y = alleles_of(b, letters);
    int c = compare_letters(x.ref, y.ref);
    if (c == 0)
      c = compare_letters(x.alt, y.alt);
    return c < 0 || (c == 0 && n_infos(i) > n_infos(j));
  };
  std::vector<uint32_t> index(n);
  for (uint32_t i = 0; i < n; ++i)
    index[i] = i;
  std::stable_sort(index.begin(), index.end(), less);
  std::string text = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  std::string const name = contig;
  std::vector<std::pair<const char *, uint32_t>> seqs(2);
  auto type_of = [&](gtx_disc_variant const & r)
  {
    Alleles const a = alleles_of(r, letters);
    seqs[0] = a.ref;
    seqs[1] = a.alt;
    return variant_type(seqs);
  };
  auto write_record = [&](gtx_disc_variant const & r, long dup) // vcf.cpp:767-1015 for a record without calls
  {
    if (static_cast<uint64_t>(r.ref_len) + r.alt_len > 16000) // :791-807
      return;
    text += name;
    text += '\t';
    put_u(text, static_cast<uint64_t>(r.pos) + 1);
    text += '\t';
    text += name;
    text += ':';
    put_u(text, static_cast<uint64_t>(r.pos) + 1);
    text += ':';
    text += type_of(r);
    if (dup >= 0)
    {
      text += '.';
      put_u(text, static_cast<uint64_t>(dup));
    }
    text += '\t';
    text.append(letters + r.ref_off, r.ref_len);
    text += '\t';
    text.append(letters + r.alt_off, r.alt_len);
    text += "\t0\t.\t";
    put_ids(text, "GT_ANTI_HAPLOTYPE", ids + r.anti_off, r.n_anti); // (the keys in std::map's order)
    put_ids(text, "GT_HAPLOTYPE", ids + r.hap_off, r.n_hap);
    text += "GT_ID=";
    put_u(text, r.gt_id);
    text += '\n';
  };
  if (n)
    write_record(v[index[0]], -1);
  long dup = -1;
  for (uint32_t i = 1; i < n; ++i) // :1241-1274 (the region is the whole contig: Vcf::write("."))
  {
    gtx_disc_variant const & prev = v[index[i - 1]];
    gtx_disc_variant const & cur = v[index[i]];
    Alleles const x = alleles_of(prev, letters), y = alleles_of(cur, letters);
    if (cur.pos == prev.pos && compare_letters(x.ref, y.ref) == 0 && compare_letters(x.alt, y.alt) == 0) // Variant::operator== (variant.cpp:2242-2245)
      continue;
    if (cur.pos == prev.pos && std::strcmp(type_of(cur), type_of(prev)) == 0)
      write_record(cur, ++dup);
    else
    {
      write_record(cur, -1);
      dup = -1;
    }
  }
  *len = text.size();
  if (text.size() > cap)
    return GTX_ERR_CAPACITY;
  std::memcpy(out, text.data(), text.size());
  return GTX_OK;
}
