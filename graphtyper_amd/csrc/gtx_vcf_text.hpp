// gtx_vcf_text.hpp -- the two pieces of a VCF line that every writer of the library shares (gtx_vcf.cpp: the records and sites of a
// genotyped region; gtx_disc_variants.cpp: the sites of discovery): the number writer and the type code of a record's ID.
// Plain C++, no HIP header: tests/emu_disc_variants compiles it on its own.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace gtx
{
inline void put_u(std::string & s, uint64_t v) // (most of a VCF line is small integers: digits by hand, not through printf)
{
  char b[24];
  int n = 24;
  do
  {
    b[--n] = static_cast<char>('0' + v % 10);
    v /= 10;
  } while (v != 0);
  s.append(b + n, static_cast<size_t>(24 - n));
}

// Variant::determine_variant_type (variant.cpp:1430-1520) for the alleles of a graph without SV alleles
inline const char * variant_type(std::vector<std::pair<const char *, uint32_t>> const & seqs)
{
  size_t longer = 0;
  for (auto const & s : seqs)
    longer += s.second > 1;
  if (longer == 0)
    return "SG";
  if (seqs.size() - longer == 1)
    return "IG";
  if (seqs.size() - longer == 2 && seqs.back().second == 1 && seqs.back().first[0] == '*')
    return "IG";
  return "XG";
}
} // namespace gtx
