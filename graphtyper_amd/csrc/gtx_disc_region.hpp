// gtx_disc_region.hpp -- what the host stage behind the second pass (gtx_disc_variants.cpp) needs of a gtx_disc: the region's
// letters and where they begin.  No HIP header: the object itself (gtx_disc.hpp) owns device blocks, and gtx_disc_variants.cpp is
// also compiled on its own (tests/emu_disc_variants, which brings an object and this function of its own).
#pragma once
#include <cstdint>
#include <string>

struct gtx_disc;

namespace gtx
{
extern thread_local std::string g_last_error;
// defined beside gtx_disc_create (gtx_discover.hip); the letters live as long as the object
void disc_region(gtx_disc const * d, char const ** reference, uint64_t * reference_len, int64_t * region_begin);
} // namespace gtx
