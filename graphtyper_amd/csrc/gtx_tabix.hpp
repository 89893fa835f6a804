// gtx_tabix.hpp -- what gtx_graph_from_files (gtx_files.cpp) takes from the index of a bgzip VCF (gtx_tabix.cpp)
#pragma once
#include <zlib.h>

#include <cstdint>
#include <string>

namespace gtx
{
// Where to start reading `vcf_path` for records of `chrom` that overlap [begin, end).  false: no usable index beside the file
// (<vcf>.tbi, <vcf>.csi).  any = false: the index knows of no record there.
bool tabix_start(std::string const & vcf_path, std::string const & chrom, int64_t begin, int64_t end, bool & any, uint64_t & voffset);
// A gzFile positioned at a virtual offset of a BGZF file (NULL: could not)
gzFile gz_open_at(std::string const & path, uint64_t voffset);
} // namespace gtx
