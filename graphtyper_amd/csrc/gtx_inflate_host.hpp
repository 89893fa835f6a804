// gtx_inflate_host.hpp -- the device inflater as the library's own host code uses it (gtx_inflate_dev.hip; the BAM readers' device
// team in gtx_bgzf.cpp).
#pragma once
#include "../../include/gtx.h"

#include <cstdint>

namespace gtx
{
// n members from host buffers through the inflater's device blocks and stream: `in` (in_size bytes of streams) and the
// descriptors up, one launch, out_size bytes of output and the n statuses down; returns when they have arrived.
int inflate_host_batch(gtx_inflate * h, uint8_t const * in, uint64_t in_size, gtx_inflate_member const * members, uint32_t n, uint8_t * out, uint64_t out_size,
                       uint32_t * status, bool check_crc);

// The BAM readers (gtx_bgzf.cpp) are also built without the HIP runtime (the sanitizer drivers of tests/sanitize link the parsers
// alone), so they reach the device inflater through this table: gtx_inflate_dev.hip sets it when the library is loaded, and
// where it is not linked in the readers answer GTX_ERR_NO_DEVICE.
struct InflateDeviceOps
{
  int (*create)(int device, gtx_inflate ** out);
  void (*destroy)(gtx_inflate *);
  void * (*pinned_alloc)(gtx_inflate *, uint64_t bytes); // nullptr: none to be had
  void (*pinned_free)(void *);
  int (*batch)(gtx_inflate *, uint8_t const *, uint64_t, gtx_inflate_member const *, uint32_t, uint8_t *, uint64_t, uint32_t *, bool); // inflate_host_batch
};
extern InflateDeviceOps const * inflate_device_ops; // (gtx_bgzf.cpp)
} // namespace gtx
