// The reduction the gradient chains end with (mdr_ppo_grad.hip - PPO and DQN -, mdr_tarmac_ppo_grad.hip): one partial gradient per workgroup, added
// in workgroup order by one thread per element - no floating-point atomics, the same partials give the same bits.
#ifndef MDR_GRAD_REDUCE_H
#define MDR_GRAD_REDUCE_H

#include <hip/hip_runtime.h>

#include <cstdint>

// the sum over the partials of element i in workgroup order (eight loads in flight at a time; the additions stay in that order)
static __device__ __forceinline__ float grad_reduce_sum(const float* __restrict__ part, int nparts, int stride, int i) {
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
  return sum;
}

// grad[i] = (sum over the partials in workgroup order) / denom, the loss (element G of every partial) behind it; no partials: zeros
static __global__ void k_ppo_grad_reduce(const float* __restrict__ part, int nparts, int stride, int G, float denom, float* __restrict__ grad,
                                         float* __restrict__ loss) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > G) return;
  const float sum = grad_reduce_sum(part, nparts, stride, i);
  const float v = nparts > 0 ? sum / denom : 0.0f;
  if (i < G) grad[i] = v;
  else *loss = v;
}

// the same with every gradient element clamped to [-c, c] behind the division (agents/dqn.py:108-109, param.grad.data.clamp_(-1, 1)),
// the loss never: comparisons, not fminf / fmaxf, so that a NaN stays a NaN as under clamp_; c = inf clamps nothing
static __global__ void k_grad_reduce_clamped(const float* __restrict__ part, int nparts, int stride, int G, float denom, float c,
                                             float* __restrict__ grad, float* __restrict__ loss) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > G) return;
  const float sum = grad_reduce_sum(part, nparts, stride, i);
  const float v = nparts > 0 ? sum / denom : 0.0f;
  if (i < G) grad[i] = v < -c ? -c : (v > c ? c : v);
  else *loss = v;
}

#endif
