// The bf16 head + tail split behind every bf16x3 kernel form (mdr_policy.hip, mdr_tarmac_mlp_bf16.hip): x = xh + xl with xh = bf16(x),
// xl = bf16(x - xh), round to nearest even - 16 significand bits per operand; w x ~ wh xh + wl xh + wh xl on v_mfma_f32_16x16x32_bf16.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// (bf16(hi) << 16) | bf16(lo), round to nearest even.  Inline assembly is opaque to hipcc's hazard recogniser: a VGPR written here and
// read as an MFMA operand by the very next instruction needs two wait states that nobody else inserts (round 1 shipped this
// statement without them; the stale-operand reads surfaced when a new kernel variant changed the instruction schedule:
// half the agents of the second column block came out with garbage logits).  Hence the `s_nop 1` INSIDE the string.  The
// plain vector conversion (__builtin_convertvector to bf16x2) is hazard-safe too and selects the same instruction, but lets the
// scheduler hoist the conversions until k_actor_sample_bf16 spills (1.1 KB of scratch per lane, 6x slower).
// four packed conversions in ONE statement: the last write is two wait states away from whatever follows the statement, the
// earlier ones further - one `s_nop 1` instead of four
__device__ __forceinline__ void cvt_pk_bf16_x4(const float* v, uint32_t* out) {
  asm("v_cvt_pk_bf16_f32 %0, %4, %5\n\tv_cvt_pk_bf16_f32 %1, %6, %7\n\tv_cvt_pk_bf16_f32 %2, %8, %9\n\tv_cvt_pk_bf16_f32 %3, %10, %11\n\ts_nop 1"
      : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3])
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
}

// eight fp32 values -> their bf16 head and tail fragments
__device__ __forceinline__ void split8(const float* v, uint4& hi, uint4& lo) {
  uint32_t h[4], l[4];
  cvt_pk_bf16_x4(v, h);
  float res[8];
#pragma unroll
  for (int p = 0; p < 4; ++p) {   // x - float(bf16(x)); scalar subtractions: packed f32 VALU issues slowly beside MFMAs (MI355X_MICROARCH.md)
    res[2 * p] = v[2 * p] - __uint_as_float(h[p] << 16);
    res[2 * p + 1] = v[2 * p + 1] - __uint_as_float(h[p] & 0xFFFF0000u);
  }
  cvt_pk_bf16_x4(res, l);
  hi = uint4{h[0], h[1], h[2], h[3]};
  lo = uint4{l[0], l[1], l[2], l[3]};
}
