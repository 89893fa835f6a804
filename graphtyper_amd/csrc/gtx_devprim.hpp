// gtx_devprim.hpp -- the rocPRIM primitives the library's host code runs (gtx_index_dev.hip, gtx_discover.hip; nothing else
// includes this, so that rocPRIM stays out of the other translation units), each over a TempPool: rocPRIM is called once for the
// size of its temporary storage, the storage comes from the pool, and the second call runs on the pool's stream.  The
// sorts take the caller's own iterator types (one caller sorts from pointers to const, one does not), so that every call
// instantiates the kernels it did when it was written out by hand.  Pool is a TempPool, or whatever hands out the storage in its
// place through the same members (get<uint8_t>, ok, fine, stream): gtx_dstream.hip has a block made once, so that a push allocates nothing.
#pragma once
#include <cstring> // (rocPRIM's texture iterator calls memset on the host)

#include <rocprim/rocprim.hpp>

#include <string>

#include "gtx_devmem.hpp"

namespace gtx
{
// run(storage, bytes) is one rocPRIM call: with storage == nullptr it only sets `bytes` (and launches nothing).  `what` and
// `storage` name the primitive and its temporary in the messages.
template <class Pool, class Run>
bool with_storage(Pool & pool, char const * what, char const * storage, Run run)
{
  size_t bytes = 0;
  hipError_t const e = run(nullptr, bytes);
  if (e != hipSuccess)
    return pool.ok(e, (std::string(what) + " (size)").c_str());
  void * const tmp = pool.template get<uint8_t>(bytes, storage);
  return pool.fine && pool.ok(run(tmp, bytes), what);
}

template <class Pool>
bool exclusive_sum(Pool & pool, uint32_t const * in, uint32_t * out, size_t n, char const * what, char const * storage)
{
  return with_storage(pool, what, storage,
                      [&](void * tmp, size_t & bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), pool.stream); });
}

template <class Pool, class Op>
bool inclusive_scan(Pool & pool, uint32_t const * in, uint32_t * out, size_t n, Op op, char const * what, char const * storage)
{
  return with_storage(pool, what, storage, [&](void * tmp, size_t & bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, n, op, pool.stream); });
}

// stable, bits [0, bits) of the keys (rocPRIM makes the type of the size a template argument of its sort kernels: both callers count in 32 bits)
template <class Pool, class KeysIn, class KeysOut, class ValuesIn, class ValuesOut>
bool sort_pairs(Pool & pool, KeysIn kin, KeysOut kout, ValuesIn vin, ValuesOut vout, uint32_t n, unsigned bits, char const * what, char const * storage)
{
  return with_storage(pool, what, storage,
                      [&](void * tmp, size_t & bytes) { return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0u, bits, pool.stream); });
}

template <class Pool, class KeysIn, class KeysOut>
bool sort_keys(Pool & pool, KeysIn kin, KeysOut kout, uint32_t n, unsigned bits, char const * what, char const * storage)
{
  return with_storage(pool, what, storage, [&](void * tmp, size_t & bytes) { return rocprim::radix_sort_keys(tmp, bytes, kin, kout, n, 0u, bits, pool.stream); });
}
} // namespace gtx
