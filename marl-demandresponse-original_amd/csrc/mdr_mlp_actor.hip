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
//
// One net per agent (mdr_mlp_actors_sample; MADDPG's unshared networks, ddpg.py:200-213): the PER_NET instantiations of the same kernel.
// Row e K + k goes through net k; a unit of work is (net k, tile of 32 ENVS), whose rows lie K ld floats apart; a workgroup walks a
// contiguous run of units, net by net, and reloads its slabs when the run changes net.  Both per-net forms have 8 waves (UB = 2): the
// 16-wave form has two registers to spare, the run's bookkeeping needs more.  The F <= 64 one keeps one head partial per 16-unit block,
// added in block order, so that it gives the 16-wave shared form's bits; the F > 64 one has no register for a tile in flight and
// fetches a tile when it stages it.  Neither uses scratch; the two shared forms compile to the registers they had before.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

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

// one net per agent (mdr_mlp_actors_sample): row e K + k goes through net k.  The pointers travel in the kernel argument block - 32 x
// 48 bytes - so there is no device table to own.  A unit of work is (net k, tile t of 32 envs), numbered k T + t; workgroup b of G
// walks the units [b U / G, (b + 1) U / G): consecutive tiles of one net, then the next net's
struct NetPtrs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};
struct MlpActorsArgs {
  MlpActorArgs s;             // w1 .. b3 unused; A = E K rows in all
  int64_t E, T, U;            // envs, tiles of 32 envs per net, units = K T
  int K;
  NetPtrs net[MDR_MAX_AGENT_NETS];
};
__device__ __forceinline__ int64_t uniform64(int64_t x) {      // a wave-uniform value into scalar registers
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int clamp30(int64_t d) {      // min(d, 2^30) of a d >= 0
  const uint32_t hi = (uint32_t)((uint64_t)d >> 32), lo = (uint32_t)d;
  return (hi != 0u || lo > (1u << 30)) ? (1 << 30) : (int)lo;
}
__device__ __forceinline__ const MlpActorArgs& shared_args(const MlpActorArgs& a) { return a; }
__device__ __forceinline__ const MlpActorArgs& shared_args(const MlpActorsArgs& a) { return a.s; }

__device__ __forceinline__ float relu(float x) {      // mdr_policy.hip: max on the bit pattern, one instruction
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__host__ __device__ constexpr int lds_floats(int s1, int np) { return 4 * s1 * R + MAX_H * R + np * R + 3 * MAX_H; }      // np: partials per agent

// S1: k-steps of layer 1 the form holds registers for (4 S1 >= F); UB: 16-unit blocks per wave
// PER_NET: one net per agent (MlpActorsArgs above) - an instantiation of its own, so that the shared forms keep their code and registers
template <int S1, int UB, bool PER_NET = false>
__global__ __launch_bounds__(64 * (16 / UB)) void k_mlp_actor(std::conditional_t<PER_NET, MlpActorsArgs, MlpActorArgs> args) {
  const MlpActorArgs& a = shared_args(args);
  constexpr int NW = 16 / UB, NT = 64 * NW, KX = 4 * S1;
  constexpr int NLD = KX * R / NT;      // floats of a tile a thread stages
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                      // [KX][2 r + cb]
  float* hT = xT + KX * R;              // [256][2 r + cb]
  float* part = hT + MAX_H * R;         // [NW][16 cb + r]
  // the per-net form of F <= 64 runs the 8-wave layout (the 16-wave one has no register to spare for the run's bookkeeping) and must
  // still give the bits of the shared 16-wave form: its head keeps one partial per 16-unit BLOCK, added in block order
  constexpr int GB = (PER_NET && S1 <= 16) ? 1 : UB;      // blocks per partial
  constexpr int NP = 16 / GB;                             // partials per agent
  float* vb1 = part + NP * R;           // b1, b2, W3[0] - W3[1]: zero beyond the net's sizes
  float* vb2 = vb1 + MAX_H;
  float* vwd = vb2 + MAX_H;

  // PER_NET: this workgroup's run of units [q, q1), net by net - `net` is the net of unit q, [t0, tend) its tiles in the run.  The shared
  // forms make one pass: the net of the call, tiles blockIdx.x, + gridDim.x, ... of all
  NetPtrs net{a.w1, a.b1, a.w2, a.b2, a.w3, a.b3};
  int64_t t0 = blockIdx.x, tstep = gridDim.x, tend = a.ntiles;
  [[maybe_unused]] int64_t q = 0, q1 = 0;
  [[maybe_unused]] int kn = 0, knl = 0, pass = 0, left = 0;      // the net's index; the pass's tiles, those still to do
  if constexpr (PER_NET) {
    // 64-bit quotients come out of the vector unit: back into scalar registers, or the run's bounds live in vector ones all the way
    q = uniform64((int64_t)blockIdx.x * args.U / gridDim.x), q1 = uniform64(((int64_t)blockIdx.x + 1) * args.U / gridDim.x);
    kn = __builtin_amdgcn_readfirstlane((int)(q / args.T));
    t0 = q - kn * args.T, tstep = 1;
  }
  do {
  if constexpr (PER_NET) {
    // the table sits in the kernel argument block, which a kernel cannot index by a variable through its by-value parameter without a
    // private copy of all of it: read the entry through the segment's own address (the first argument starts the segment)
    const char* seg = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    net = reinterpret_cast<const NetPtrs*>(seg + offsetof(MlpActorsArgs, net))[kn];
    knl = (int)mdr::loop_local((uint32_t)__builtin_amdgcn_readfirstlane(kn));    // the rows' addresses from this pass's own copy: no pointers carried from net to net
    // the pass's tiles as a 32-bit count, from 32-bit halves (there is no scalar 64-bit `<`: bounds compared in 64 bits would live in
    // vector registers); a net with more than 2^30 tiles in the run takes another pass
    left = pass = min(clamp30(args.T - t0), clamp30(q1 - q));
    q += pass;
    // the net before was last read ahead of the barrier that precedes the finish of its last tile; the first barrier of the next tile
    // publishes the LDS writes below
  }

  // PER_NET: the thread's index and the sizes as this pass's own values (mdr_draw.h says why), or the compiler computes every weight
  // address, every select mask and what the tile loop keeps per thread once, ahead of the loop over the nets, and holds them through
  // the weight load in registers it does not have
  int tid = threadIdx.x, F = a.F, H1 = a.H1, H2 = a.H2;
  if constexpr (PER_NET) {
    asm volatile("" : "+v"(tid));
    F = (int)mdr::loop_local((uint32_t)F), H1 = (int)mdr::loop_local((uint32_t)H1), H2 = (int)mdr::loop_local((uint32_t)H2);
  }
  int w = tid >> 6;
  if constexpr (PER_NET) w = __builtin_amdgcn_readfirstlane(w);      // the hidden tid is no longer known to be uniform in its high bits
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;

  // ---- once per workgroup (PER_NET: once per net of its run): this wave's rows of W1 and W2 into registers
  float w1[UB][S1], w2[UB][S2];
#pragma unroll
  for (int ub = 0; ub < UB; ++ub) {
    const int u = 16 * (w * UB + ub) + r;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      const int k = 4 * s + g;
      const float v = net.w1[min(u, H1 - 1) * F + min(k, F - 1)];      // clamped address, then a select: no branch per register
      w1[ub][s] = (u < H1 && k < F) ? v : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      const int k = 4 * s + g;
      const float v = net.w2[min(u, H2 - 1) * H1 + min(k, H1 - 1)];
      w2[ub][s] = (u < H2 && k < H1) ? v : 0.0f;
    }
  }
  for (int i = tid; i < MAX_H; i += NT) {
    vb1[i] = i < H1 ? net.b1[i] : 0.0f;
    vb2[i] = i < H2 ? net.b2[i] : 0.0f;
    vwd[i] = i < H2 ? net.w3[i] - net.w3[H2 + i] : 0.0f;
  }
  for (int i = F * R + tid; i < KX * R; i += NT) xT[i] = 0.0f;      // features F .. KX - 1: never staged, met by zero weights
  const float bias3 = net.b3[0] - net.b3[1];

  // staging: thread -> agent tid & 31 of the tile, features tid >> 5 + j NT / 32.  Agent-fastest, so that the transposed LDS writes of
  // a wave fall on 32 banks; the rows' cache lines are shared by the waves of the workgroup.  No division, one address per thread.
  constexpr int KQ = NT / R;
  const int srow = tid & (R - 1), kq = tid >> 5;
  float* const xdst = xT + kq * R + 2 * (srow & 15) + (srow >> 4);
  float xr[NLD];
  auto fetch = [&](int64_t t) {
    int64_t agent = t * R + srow;
    bool ok;
    if constexpr (PER_NET) {      // env 32 t + srow of net kn is row env K + kn
      ok = agent < args.E;
      agent = agent * args.K + knl;
    } else {
      ok = agent < a.A;
    }
    const float* src = a.obs + (ok ? agent : 0) * a.ld + kq;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const bool kok = ok && kq + KQ * j < F;
      const float v = src[kok ? KQ * j : -kq];      // a refused element reads the row's first float instead
      xr[j] = kok ? v : 0.0f;
    }
  };
  // the per-net form of F > 64 has no registers for a tile in flight (192 of weights, and the run's bookkeeping on top of what the
  // shared form fits into 256 exactly): it fetches a tile when it stages it
  constexpr bool AHEAD = !(PER_NET && S1 > 16);
  if constexpr (AHEAD)
    if (PER_NET ? left > 0 : t0 < tend) fetch(t0);

  for (int64_t t = t0; PER_NET ? left > 0 : t < tend; t += tstep) {
    if constexpr (!AHEAD) fetch(t);
#pragma unroll
    for (int j = 0; j < NLD; ++j)
      if (kq + KQ * j < F) xdst[KQ * j * R] = xr[j];
    __syncthreads();
    if constexpr (PER_NET) --left;
    if constexpr (AHEAD)
      if (PER_NET ? left > 0 : t + tstep < tend) fetch(t + tstep);      // in flight during both layers

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
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int pb = 0; pb < UB; pb += GB) {
        float d = 0.0f;
#pragma unroll
        for (int ub = pb; ub < pb + GB; ++ub) {
          const f32x4 wd = *reinterpret_cast<const f32x4*>(vwd + 16 * (w * UB + ub) + 4 * g);
#pragma unroll
          for (int i = 0; i < 4; ++i) d = fmaf(wd[i], relu(acc[ub][cb][i]), d);
        }
        d += __shfl_xor(d, 16);
        d += __shfl_xor(d, 32);
        if (g == 0) part[((w * UB + pb) / GB) * R + 16 * cb + r] = d;
      }
    __syncthreads();

    // ---- finish: the partials in wave order, the two-logit softmax and the draw of mdr_logits_sample
    if (tid < R) {
      float d = part[tid];
#pragma unroll
      for (int v = 1; v < NP; ++v) d += part[v * R + tid];
      d += bias3;
      // what the finish reads of the arguments.  PER_NET: read here, through an address the compiler cannot follow back to the
      // argument block, or all of it sits in scalar registers through both layers - registers that form does not have
      MlpActorArgs f = a;
      [[maybe_unused]] int64_t E = 0;
      [[maybe_unused]] int K = 0;
      if constexpr (PER_NET) {
        typedef const __attribute__((address_space(4))) MlpActorsArgs* Block;
        Block kp = (Block)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        f.greedy = kp->s.greedy, f.step_lo = kp->s.step_lo, f.step_hi = kp->s.step_hi, f.step_dev = kp->s.step_dev, f.k0 = kp->s.k0, f.k1 = kp->s.k1;
        f.action = kp->s.action, f.a_prob = kp->s.a_prob, f.probs = kp->s.probs;
        E = kp->E, K = kp->K;
      }
      int64_t agent = t * R + tid;
      bool ok;
      if constexpr (PER_NET) {
        ok = agent < E;
        agent = agent * K + knl;      // the GLOBAL row: the draw's counter, as in the shared forms
      } else {
        ok = agent < a.A;
      }
      if (ok) {
        const float p0 = 1.0f / (1.0f + expf(-d));
        const float p1 = 1.0f / (1.0f + expf(d));
        int act;
        if (f.greedy) {
          act = d >= 0.0f ? 0 : 1;      // argmax keeps the first maximum, as torch.argmax
        } else {
          const float u = action_uniform(mdr::action_word(agent, f.step_lo, f.step_hi, f.step_dev, f.k0, f.k1));
          act = u < p0 ? 0 : 1;
        }
        f.action[agent] = (uint8_t)act;
        if (f.a_prob) f.a_prob[agent] = act ? p1 : p0;
        if (f.probs) {
          f.probs[agent * 2] = p0;
          f.probs[agent * 2 + 1] = p1;
        }
      }
    }
  }
  if constexpr (PER_NET) {      // the run goes on at the next net's first tile
    const bool wrap = t0 + pass == args.T;
    t0 = uniform64(wrap ? 0 : t0 + pass);
    kn = __builtin_amdgcn_readfirstlane(kn + (wrap ? 1 : 0));
  }
  } while (PER_NET && q != q1);
}

template <int S1, int UB>
int launch(const MlpActorArgs& a, int64_t grid, hipStream_t st) {
  constexpr size_t bytes = (size_t)lds_floats(S1, 16 / UB) * sizeof(float);
  static_assert(bytes <= 64 * 1024, "beyond 64 KB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL((k_mlp_actor<S1, UB>), dim3((unsigned)grid), dim3(64 * (16 / UB)), bytes, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

template <int S1, int UB>
int launch_per_net(const MlpActorsArgs& a, int64_t grid, hipStream_t st) {
  constexpr size_t bytes = (size_t)lds_floats(S1, S1 <= 16 ? 16 : 16 / UB) * sizeof(float);
  static_assert(bytes <= 64 * 1024, "beyond 64 KB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  static_assert(sizeof(MlpActorsArgs) <= 4096, "the kernel argument block");
  hipLaunchKernelGGL((k_mlp_actor<S1, UB, true>), dim3((unsigned)grid), dim3(64 * (16 / UB)), bytes, st, a);
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

int mdr_mlp_actors_sample(const mdr_mlp_t* actors, int32_t nb_nets, const float* obs, int64_t ld_obs, int64_t nb_rows, uint64_t seed,
                          uint64_t step, const int32_t* step_dev, int32_t greedy, int32_t max_workgroups, uint8_t* action, float* a_prob,
                          float* probs, void* stream) {
  if (!actors || !obs || !action || nb_nets < 1 || nb_rows < 0 || max_workgroups < 0) return MDR_ERR_INVALID;
  if (nb_nets > MDR_MAX_AGENT_NETS) return MDR_ERR_UNSUPPORTED;
  for (int k = 0; k < nb_nets; ++k) {
    const mdr_mlp_t& n = actors[k];
    if (n.struct_size != sizeof(mdr_mlp_t) || !n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3) return MDR_ERR_INVALID;
  }
  const int F = actors[0].num_state, H1 = actors[0].hidden1, H2 = actors[0].hidden2;
  for (int k = 0; k < nb_nets; ++k) {
    const mdr_mlp_t& n = actors[k];
    if (n.num_state != F || n.hidden1 != H1 || n.hidden2 != H2 || n.num_out != 2) return MDR_ERR_UNSUPPORTED;
  }
  if (F < 1 || F > MAX_F || H1 < 1 || H1 > MAX_H || H2 < 1 || H2 > MAX_H) return MDR_ERR_UNSUPPORTED;
  if (ld_obs < F || nb_rows % nb_nets != 0) return MDR_ERR_INVALID;
  if (nb_rows == 0) return MDR_OK;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  MlpActorsArgs aa{};
  MlpActorArgs& a = aa.s;
  a.obs = obs, a.ld = ld_obs, a.A = nb_rows;
  a.F = F, a.H1 = H1, a.H2 = H2, a.greedy = greedy != 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.step_dev = step_dev;
  a.action = action, a.a_prob = a_prob, a.probs = probs;
  aa.K = nb_nets, aa.E = nb_rows / nb_nets, aa.T = (aa.E + R - 1) / R, aa.U = aa.T * nb_nets;
  a.ntiles = aa.U;
  for (int k = 0; k < nb_nets; ++k) aa.net[k] = NetPtrs{actors[k].w1, actors[k].b1, actors[k].w2, actors[k].b2, actors[k].w3, actors[k].b3};
  // one workgroup per compute unit, each a contiguous run of units: with at least as many workgroups as nets a workgroup loads one
  // net's weights, two where its run crosses into the next net; with max_workgroups = 1 one workgroup walks every net.  The form
  // depends on F alone, as in mdr_mlp_actor_sample
  int64_t grid = aa.U < cus ? aa.U : cus;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  hipStream_t st = (hipStream_t)stream;
  return F <= 64 ? launch_per_net<16, 2>(aa, grid, st) : launch_per_net<32, 2>(aa, grid, st);
}

}  // extern "C"
