// The device helpers of the kernel families that stream an MLP's weights from L2 (mdr_maddpg_grad.hip, mdr_tarmac_critic_grad.hip):
// one wave per 16-unit block of a layer, the weights - torch's [out][in] layout - as the MFMA A operand straight from global memory,
// the tile's activations transposed [unit][row] with row stride LT in LDS as the B operand.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 (A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: col = l & 15, row = 4 (l >> 4) +
// reg).  Throughout: c = lane & 15 (the tile row the lane's MFMA column belongs to), g = lane >> 4.  A contraction runs over k in
// ascending steps of four on one accumulator, whatever the chunking of its input: the bits do not depend on where a chunk ends.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mdr_stream {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LT = 20;                // row stride of the transposed tile images
constexpr int KC = 128;               // joint-input columns staged at a time
constexpr int LIB_MAX_WG = 512;       // the library's own grid: min(work items, CUs, this)

__host__ __device__ inline int blocks16(int n) { return (n + 15) / 16; }

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc[unit u0 + 4 g + i][row c] += sum_{k < kn} W[u0 + m][k0 + k] inT[k][row]; inT zero from kn up to the next multiple of 4
template <int UNR>
__device__ __forceinline__ void fwd_accum(f32x4& acc, const float* __restrict__ W, int ldw, int H, int u0, int k0, int kn, const float* inT,
                                          int c, int g) {
  const int u = u0 + c;
  const bool uok = u < H;
  const float* wr = W + (int64_t)(uok ? u : 0) * ldw + k0;
  const int ks = (kn + 3) >> 2;
  for (int q0 = 0; q0 < ks; q0 += UNR) {      // UNR k-steps' weights asked for together
    float av[UNR];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int kk = 4 * (q0 + i) + g;
      av[i] = (uok && kk < kn) ? wr[kk] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
      if (q0 + i < ks) acc = mfma(av[i], inT[(4 * (q0 + i) + g) * LT + c], acc);
  }
}

__device__ __forceinline__ f32x4 bias_block(const float* __restrict__ b, int H, int u0, int g) {
  f32x4 acc;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (u0 + 4 * g + i < H) ? b[u0 + 4 * g + i] : 0.0f;
  return acc;
}

// the block's values into the LDS image and, where asked, the workspace [row][Hp]
__device__ __forceinline__ void store_block(const f32x4& v, float* imgT, float* ws, int Hp, int64_t row, int u0, int c, int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) imgT[(u0 + 4 * g + i) * LT + c] = v[i];
  if (ws) *reinterpret_cast<f32x4*>(ws + row * Hp + u0 + 4 * g) = v;
}

// dzin[k0 + 4 g + i][row c] = relu'(hin) sum_{u < Hout} W[u][k0 + m] dzout[u][row], in place of hin's image
template <int UNR>
__device__ __forceinline__ void bwd_block(const float* __restrict__ W, int Hout, int Hin, int k0, const float* dzoutT, float* hinT, float* ws, int Hp,
                                          int64_t row, int c, int g) {
  f32x4 acc = {0, 0, 0, 0};
  const int kc = k0 + c;
  const bool kok = kc < Hin;
  const float* wc = W + (kok ? kc : 0);
  const int ks = 4 * blocks16(Hout);
  for (int q0 = 0; q0 < ks; q0 += UNR) {
    float av[UNR];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int u = 4 * (q0 + i) + g;
      av[i] = (kok && u < Hout) ? wc[(int64_t)u * Hin] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
      if (q0 + i < ks) acc = mfma(av[i], dzoutT[(4 * (q0 + i) + g) * LT + c], acc);      // ks is a multiple of 4, not of UNR
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = hinT[(k0 + 4 * g + i) * LT + c] > 0.0f ? acc[i] : 0.0f;
  store_block(acc, hinT, ws, Hp, row, k0, c, g);
}

inline int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }

inline int lib_cap(int32_t max_workgroups) {
  if (max_workgroups > 0) return max_workgroups;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  return cus < LIB_MAX_WG ? cus : LIB_MAX_WG;
}

}  // namespace mdr_stream
