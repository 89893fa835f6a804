// gtx_disc.hpp -- the discovery object of include/gtx.h, for the translation units that hold its entry points (gtx_discover.hip:
// the first pass; gtx_realign.hip: the realignment to the indels; gtx_disc_second.hip: the second pass up to the aligner;
// gtx_disc_rounds.hip: from the aligner on; gtx_discover_run.hip: the host loops).  Host code without HIP: gtx_disc_region.hpp.
#pragma once
#include <cstdint>
#include <string>

#include "gtx_devmem.hpp"

struct gtx_disc
{
  int device = -1;
  int64_t region_begin = 0;
  std::string reference; // region's bases as given (upper case letters)
  gtx::DevPtr<uint32_t> d_refp; // (gtx_disc_destroy waits for the device before the two blocks go back to the cache)
  uint32_t ref_groups = 0;
  gtx::DevPtr<uint8_t> d_refc; // the letters themselves (the span of an indel compares them as the host does)
  uint32_t max_read_len = 0; // gtx_disc_set_max_read_len: 0 = GTX_MAX_READ; above it, gtx_disc_realign_batch runs the long aligner behind the short one
  gtx::DevPtr<uint32_t> d_ref5; // the letters as five planes per group (gtx_disc_second_dev.hpp: the second pass compares letter against letter)
};
