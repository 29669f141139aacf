// The actor of up to 256 hidden units per layer (include/mdr_policy.h: mdr_mlp_actor_sample): observation rows -> Linear - ReLU - Linear -
// ReLU - Linear(2) -> softmax -> draw or argmax in ONE launch, the weights read from torch's own [out][in] layout on every call.
//
// Reference: MADDPG's actor (agents/ddpg.py, DDPG_Network of agents/network.py:80-100, config.py DDPG_prop.actor_hidden_dim = 256) acts on
// every agent's observation at every step of train_ddpg.py:95-116.  W2 alone is 256 KB - more than the 160 KB of LDS k_actor_sample16
// keeps its fragments in - and mdr_stream_mlp.h's kernels re-read a layer from L2 for every 16 rows, which is right for a 64-row
// minibatch and wrong for millions of agents.  The register file of a compute unit is 512 KB, so the weights live there:
//
//   a persistent workgroup of NW = 16 / UB waves; wave w owns the UB 16-unit blocks w UB .. w UB + UB - 1 of BOTH hidden layers (H <= 256:
//   at most 16 blocks) and loads their rows of W1 and W2 ONCE, as MFMA A operands: lane l holds W[16 blk + (l & 15)][4 s + (l >> 4)] for
//   every k-step s - S1 = 16 or 32 registers of W1 (F <= 64 / <= 128) and 64 of W2 per block, zero beyond the net's sizes.
//   F <= 64: UB = 1 - 16 waves, four per SIMD, 80 weight registers under the 128 of that occupancy.  F <= 128: UB = 2 - 8 waves, two per
//   SIMD, 192 weight registers under 256 (with UB = 1 its 96 + the tile's working set spilled 27 registers).  Neither form uses scratch.
//
//   per tile of R = 32 consecutive agents (two 16-agent column blocks, so that one A register feeds two MFMAs):
//     stage    the rows (prefetched into registers during the previous tile) transposed into LDS, xT[feature][agent]       | barrier
//     layer 1  B = xT, C starts as the bias; relu; the h1 tile goes to LDS as hT[unit][agent]                              | barrier
//     layer 2  B = hT; relu; per-wave partial of the head's dot product with W3[0] - W3[1] -> part[wave][agent]            | barrier
//     finish   32 threads add the NW partials in wave order and b3[0] - b3[1], softmax, draw (mdr_draw.h), guarded stores
//   LDS images interleave the two column blocks - [k][2 r + cb] - so a lane's B operands of both blocks are one 8-byte read.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 (A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: col = l & 15, row = 4 (l >> 4) +
// reg).  An agent's arithmetic does not depend on where in a tile, a batch or a grid it sits: a column of an MFMA is a chain over k
// whatever the column, the partials are added in wave order, there are no atomics.  Rows past the batch are staged as zeros and never
// stored.  Groups of four k-steps and waves beyond the net's sizes are skipped by uniform branches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_draw.h"

namespace {

using mdr::action_uniform;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MAX_F = 128, MAX_H = 256;
constexpr int R = 32;                 // agents per tile: two column blocks
constexpr int S2 = MAX_H / 4;         // k-steps of layer 2

struct MlpActorArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float* obs;
  int64_t ld, A, ntiles;
  int F, H1, H2, greedy;
  uint32_t k0, k1, step_lo, step_hi;
  const int32_t* step_dev;
  uint8_t* action;
  float *a_prob, *probs;
};

__device__ __forceinline__ float relu(float x) {      // mdr_policy.hip: max on the bit pattern, one instruction
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__host__ __device__ constexpr int lds_floats(int s1, int ub) { return 4 * s1 * R + MAX_H * R + (16 / ub) * R + 3 * MAX_H; }

// S1: k-steps of layer 1 the form holds registers for (4 S1 >= F); UB: 16-unit blocks per wave
template <int S1, int UB>
__global__ __launch_bounds__(64 * (16 / UB)) void k_mlp_actor(MlpActorArgs a) {
  constexpr int NW = 16 / UB, NT = 64 * NW, KX = 4 * S1;
  constexpr int NLD = KX * R / NT;      // floats of a tile a thread stages
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                      // [KX][2 r + cb]
  float* hT = xT + KX * R;              // [256][2 r + cb]
  float* part = hT + MAX_H * R;         // [NW][16 cb + r]
  float* vb1 = part + NW * R;           // b1, b2, W3[0] - W3[1]: zero beyond the net's sizes
  float* vb2 = vb1 + MAX_H;
  float* vwd = vb2 + MAX_H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4, w = tid >> 6;
  const int F = a.F, H1 = a.H1, H2 = a.H2;

  // ---- once per workgroup: this wave's rows of W1 and W2 into registers
  float w1[UB][S1], w2[UB][S2];
#pragma unroll
  for (int ub = 0; ub < UB; ++ub) {
    const int u = 16 * (w * UB + ub) + r;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      const int k = 4 * s + g;
      const float v = a.w1[min(u, H1 - 1) * F + min(k, F - 1)];      // clamped address, then a select: no branch per register
      w1[ub][s] = (u < H1 && k < F) ? v : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      const int k = 4 * s + g;
      const float v = a.w2[min(u, H2 - 1) * H1 + min(k, H1 - 1)];
      w2[ub][s] = (u < H2 && k < H1) ? v : 0.0f;
    }
  }
  for (int i = tid; i < MAX_H; i += NT) {
    vb1[i] = i < H1 ? a.b1[i] : 0.0f;
    vb2[i] = i < H2 ? a.b2[i] : 0.0f;
    vwd[i] = i < H2 ? a.w3[i] - a.w3[H2 + i] : 0.0f;
  }
  for (int i = F * R + tid; i < KX * R; i += NT) xT[i] = 0.0f;      // features F .. KX - 1: never staged, met by zero weights
  const float bias3 = a.b3[0] - a.b3[1];

  // staging: thread -> agent tid & 31 of the tile, features tid >> 5 + j NT / 32.  Agent-fastest, so that the transposed LDS writes of
  // a wave fall on 32 banks; the rows' cache lines are shared by the waves of the workgroup.  No division, one address per thread.
  constexpr int KQ = NT / R;
  const int srow = tid & (R - 1), kq = tid >> 5;
  float* const xdst = xT + kq * R + 2 * (srow & 15) + (srow >> 4);
  float xr[NLD];
  auto fetch = [&](int64_t t) {
    const int64_t agent = t * R + srow;
    const bool ok = agent < a.A;
    const float* src = a.obs + (ok ? agent : 0) * a.ld + kq;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const bool kok = ok && kq + KQ * j < F;
      const float v = src[kok ? KQ * j : -kq];      // a refused element reads the row's first float instead
      xr[j] = kok ? v : 0.0f;
    }
  };
  if ((int64_t)blockIdx.x < a.ntiles) fetch(blockIdx.x);

  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
#pragma unroll
    for (int j = 0; j < NLD; ++j)
      if (kq + KQ * j < F) xdst[KQ * j * R] = xr[j];
    __syncthreads();
    if (t + gridDim.x < a.ntiles) fetch(t + gridDim.x);      // in flight during both layers

    // the sizes as this tile's own values (mdr_draw.h says why): the compiler otherwise computes the skip conditions of all 24 groups
    // of k-steps once, ahead of the loop, and keeps them in scalar registers it does not have
    const int Fk = (int)mdr::loop_local((uint32_t)F), H1k = (int)mdr::loop_local((uint32_t)H1);

    // ---- layer 1
    f32x4 acc[UB][2];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) acc[ub][0] = acc[ub][1] = *reinterpret_cast<const f32x4*>(vb1 + 16 * (w * UB + ub) + 4 * g);
    if (16 * w * UB < H1) {
#pragma unroll
      for (int q = 0; q < S1 / 4; ++q)
        if (16 * q < Fk) {
#pragma unroll
          for (int s = 4 * q; s < 4 * q + 4; ++s) {
            const float2 b = *reinterpret_cast<const float2*>(xT + (4 * s + g) * R + 2 * r);
#pragma unroll
            for (int ub = 0; ub < UB; ++ub) {
              acc[ub][0] = mma(w1[ub][s], b.x, acc[ub][0]);
              acc[ub][1] = mma(w1[ub][s], b.y, acc[ub][1]);
            }
          }
        }
    }
#pragma unroll
    for (int ub = 0; ub < UB; ++ub)
#pragma unroll
      for (int i = 0; i < 4; ++i)      // every unit up to 255 is written: layer 2 reads zeros, not stale LDS, beyond H1
        *reinterpret_cast<float2*>(hT + (16 * (w * UB + ub) + 4 * g + i) * R + 2 * r) = make_float2(relu(acc[ub][0][i]), relu(acc[ub][1][i]));
    __syncthreads();

    // ---- layer 2 and this wave's share of the head
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) acc[ub][0] = acc[ub][1] = *reinterpret_cast<const f32x4*>(vb2 + 16 * (w * UB + ub) + 4 * g);
    if (16 * w * UB < H2) {
#pragma unroll
      for (int q = 0; q < S2 / 4; ++q)
        if (16 * q < H1k) {
#pragma unroll
          for (int s = 4 * q; s < 4 * q + 4; ++s) {
            const float2 b = *reinterpret_cast<const float2*>(hT + (4 * s + g) * R + 2 * r);
#pragma unroll
            for (int ub = 0; ub < UB; ++ub) {
              acc[ub][0] = mma(w2[ub][s], b.x, acc[ub][0]);
              acc[ub][1] = mma(w2[ub][s], b.y, acc[ub][1]);
            }
          }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float d = 0.0f;
#pragma unroll
      for (int ub = 0; ub < UB; ++ub) {
        const f32x4 wd = *reinterpret_cast<const f32x4*>(vwd + 16 * (w * UB + ub) + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) d = fmaf(wd[i], relu(acc[ub][cb][i]), d);
      }
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (g == 0) part[w * R + 16 * cb + r] = d;
    }
    __syncthreads();

    // ---- finish: the partials in wave order, the two-logit softmax and the draw of mdr_logits_sample
    if (tid < R) {
      float d = part[tid];
#pragma unroll
      for (int v = 1; v < NW; ++v) d += part[v * R + tid];
      d += bias3;
      const int64_t agent = t * R + tid;
      if (agent < a.A) {
        const float p0 = 1.0f / (1.0f + expf(-d));
        const float p1 = 1.0f / (1.0f + expf(d));
        int act;
        if (a.greedy) {
          act = d >= 0.0f ? 0 : 1;      // argmax keeps the first maximum, as torch.argmax
        } else {
          const float u = action_uniform(mdr::action_word(agent, a.step_lo, a.step_hi, a.step_dev, a.k0, a.k1));
          act = u < p0 ? 0 : 1;
        }
        a.action[agent] = (uint8_t)act;
        if (a.a_prob) a.a_prob[agent] = act ? p1 : p0;
        if (a.probs) {
          a.probs[agent * 2] = p0;
          a.probs[agent * 2 + 1] = p1;
        }
      }
    }
  }
}

template <int S1, int UB>
int launch(const MlpActorArgs& a, int64_t grid, hipStream_t st) {
  constexpr size_t bytes = (size_t)lds_floats(S1, UB) * sizeof(float);
  static_assert(bytes <= 64 * 1024, "beyond 64 KB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL((k_mlp_actor<S1, UB>), dim3((unsigned)grid), dim3(64 * (16 / UB)), bytes, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int mdr_mlp_actor_sample(const mdr_mlp_t* actor, const float* obs, int64_t ld_obs, int64_t nb_agents, uint64_t seed, uint64_t step,
                         const int32_t* step_dev, int32_t greedy, int32_t max_workgroups, uint8_t* action, float* a_prob, float* probs,
                         void* stream) {
  if (!actor || actor->struct_size != sizeof(mdr_mlp_t) || !obs || !action || nb_agents < 0 || max_workgroups < 0) return MDR_ERR_INVALID;
  if (!actor->w1 || !actor->b1 || !actor->w2 || !actor->b2 || !actor->w3 || !actor->b3) return MDR_ERR_INVALID;
  const int F = actor->num_state, H1 = actor->hidden1, H2 = actor->hidden2;
  if (F < 1 || F > MAX_F || H1 < 1 || H1 > MAX_H || H2 < 1 || H2 > MAX_H || actor->num_out != 2) return MDR_ERR_UNSUPPORTED;
  if (ld_obs < F) return MDR_ERR_INVALID;
  if (nb_agents == 0) return MDR_OK;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  MlpActorArgs a{};
  a.w1 = actor->w1, a.b1 = actor->b1, a.w2 = actor->w2, a.b2 = actor->b2, a.w3 = actor->w3, a.b3 = actor->b3;
  a.obs = obs, a.ld = ld_obs, a.A = nb_agents, a.ntiles = (nb_agents + R - 1) / R;
  a.F = F, a.H1 = H1, a.H2 = H2, a.greedy = greedy != 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.step_dev = step_dev;
  a.action = action, a.a_prob = a_prob, a.probs = probs;
  // the weight registers allow one workgroup per compute unit: a larger grid would only load the weights more often.  The form
  // depends on F alone, never on the batch: an agent's bits must not
  int64_t grid = a.ntiles < cus ? a.ntiles : cus;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  hipStream_t st = (hipStream_t)stream;
  return F <= 64 ? launch<16, 1>(a, grid, st) : launch<32, 2>(a, grid, st);
}

}  // extern "C"
