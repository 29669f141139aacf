// The reduction both gradient chains end with (mdr_ppo_grad.hip, mdr_tarmac_ppo_grad.hip): one partial gradient per workgroup, added
// in workgroup order by one thread per element - no floating-point atomics, the same partials give the same bits.
#ifndef MDR_GRAD_REDUCE_H
#define MDR_GRAD_REDUCE_H

#include <hip/hip_runtime.h>

#include <cstdint>

// grad[i] = (sum over the partials in workgroup order) / denom, the loss (element G of every partial) behind it; no partials: zeros
// (eight loads in flight at a time; the additions stay in workgroup order)
static __global__ void k_ppo_grad_reduce(const float* __restrict__ part, int nparts, int stride, int G, float denom, float* __restrict__ grad,
                                         float* __restrict__ loss) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > G) return;
  float sum = 0.0f;
  int p = 0;
  for (; p + 8 <= nparts; p += 8) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = part[(int64_t)(p + j) * stride + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += x[j];
  }
  for (; p < nparts; ++p) sum += part[(int64_t)p * stride + i];
  const float v = nparts > 0 ? sum / denom : 0.0f;
  if (i < G) grad[i] = v;
  else *loss = v;
}

#endif
