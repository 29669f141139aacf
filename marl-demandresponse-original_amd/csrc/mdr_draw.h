// The draw behind a sampled action, shared by every kernel that samples one (mdr_policy.hip, mdr_tarmac.hip, mdr_tarmac_mlp.hip): gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdr_device.h"

namespace mdr {

constexpr uint32_t TAG_ACTION = 0x41435431u;

// The Philox key of a draw, hidden from loop-invariant code motion: hipcc otherwise keeps the ten round keys (k + n W) of both
// words in 20 scalar registers for the whole kernel - beyond the scalar file, so they are parked in the lanes of a vector
// register and fetched back one v_readlane at a time.  Re-deriving them where a draw is made is 20 scalar adds.
__device__ __forceinline__ uint32_t loop_local(uint32_t x) {
  asm volatile("" : "+s"(x));
  return x;
}

// Word 0 of Philox4x32-10 with key = (k0, k1) = seed and counter = (agent lo, agent hi, step lo + *step_dev, TAG_ACTION ^ step hi)
// (include/mdr_policy.h).  `agent` is the index in the whole batch.  The device-side step is added to the low word only (mod 2^32,
// no carry into the high word).
__device__ __forceinline__ uint32_t action_word(int64_t agent, uint32_t step_lo, uint32_t step_hi, const int32_t* step_dev, uint32_t k0,
                                                uint32_t k1) {
  return philox4x32_10((uint32_t)agent, (uint32_t)((uint64_t)agent >> 32), step_lo + (step_dev ? (uint32_t)*step_dev : 0u),
                       TAG_ACTION ^ step_hi, loop_local(k0), loop_local(k1)).x;
}

// ... and its uniform in (0,1): the centre of one of 2^24 cells.  The top cell's centre, 16777215.5, is no fp32 number and ties to
// 2^24, i.e. u = 1.0f, which `u < p0` fails even for p0 == 1.0f (an action of probability 0); the clamp maps that one cell to the
// largest float below 1 and changes no other draw.
__device__ __forceinline__ float action_uniform(uint32_t bits) {
  return fminf(((float)(bits >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
}

}  // namespace mdr
