// Mailbox granules shared by the persistent rollout (mdr_persist.hip) and the one-step mailbox exchange (mdr_mailbox.hip).
// A granule is 8 bytes {tag, 32 data bits} written by ONE write-through atomic store, so it is its own flag; the layout of a
// mailbox is [PERSIST_HDR header | SLOTS x E x world x stride x PERSIST_G records | SLOTS x E x PERSIST_TOT totals] (mdr_kernels.h)
// and, when a halo region was allocated behind it, [HALO_SLOTS x world x count] message granules (mdr_mailbox.hip).
#pragma once

#include "mdr_device.h"
#include "mdr_kernels.h"

namespace mdr {

typedef __attribute__((address_space(1))) unsigned long long gu64;

template <bool SYS>
__device__ __forceinline__ void granule_store(gu64* p, uint32_t tag, uint32_t value) {
  const unsigned long long x = ((unsigned long long)tag << 32) | value;
  if (SYS) __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool SYS>
__device__ __forceinline__ unsigned long long granule_load(const gu64* p) {
  if (SYS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t rec_offset(const PersistArgs& m, int E, int slot, int e, int r, int b) {
  return PERSIST_HDR + ((((int64_t)slot * E + e) * m.world + r) * m.stride + b) * PERSIST_G;
}
__device__ __forceinline__ int64_t tot_offset(const PersistArgs& m, int E, int slot, int e) {
  return PERSIST_HDR + (int64_t)PERSIST_SLOTS * E * m.world * m.stride * PERSIST_G + ((int64_t)slot * E + e) * PERSIST_TOT;
}

// Kinds of the error word.  1, 2: the persistent rollout; 3, 4: the one-step exchange; 5: the halo exchange.
enum : uint32_t {
  PERSIST_FAIL_TOTALS = 1, PERSIST_FAIL_RECORDS = 2,
  MAILBOX_FAIL_TOTALS = 3, MAILBOX_FAIL_RECORDS = 4, MAILBOX_FAIL_HALO = 5,
};

// error word (granule 0 of every rank's header): {tag | kind << 28 | workgroup}; a spinner that finds it set leaves as well.
// Lane r < world keeps rank r's header address (`abort_ptr`): the eight mailbox pointers then need not stay live in scalar
// registers across the step loops for the sake of this cold path (they were spilled to vector lanes and reloaded every step).
template <bool SYS>
__device__ __forceinline__ void raise_abort(gu64* abort_ptr, uint32_t tag, uint32_t kind) {
  if (abort_ptr != nullptr) granule_store<SYS>(abort_ptr, tag, (kind << 28) | (blockIdx.x & 0x0FFFFFFFu));
}
template <bool SYS>
__device__ __forceinline__ bool abort_raised(const gu64* own) {
  return granule_load<SYS>(own) != 0ull;
}

}  // namespace mdr
