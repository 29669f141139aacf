// The actor of up to 256 hidden units per layer in bf16x3 (include/mdr_policy.h: mdr_mlp_actor_sample_bf16x3): k_mlp_actor of
// mdr_mlp_actor.hip with both hidden layers on v_mfma_f32_16x16x32_bf16.  Every operand is split into a bf16 head and tail
// (mdr_bf16_split.h: xh = bf16(x), xl = bf16(x - xh), round to nearest even) and every product is wh xh + wl xh + wh xl, accumulated in
// fp32 from the fp32 bias.  The head's dot product, the softmax and the draw are the fp32 form's, statement for statement.
//
// The scheme is the fp32 form's: a persistent workgroup of NW = 16 / UB waves; wave w owns the UB 16-unit blocks w UB .. w UB + UB - 1
// of BOTH hidden layers and loads their rows of W1 and W2 ONCE per launch, from torch's own [out][in] tensors, splits them and keeps them
// as A fragments: lane l holds W[16 blk + (l & 15)][32 s + 8 (l >> 4) + j], j < 8, for every k-step s of 32 - four registers of heads
// and four of tails per k-step, zero beyond the net's sizes.  Per block: 8 k-steps of W2 = 64 registers, and S1 = 2 (F <= 64) or 4
// (F <= 128) k-steps of W1 = 16 or 32 - the fp32 form's budget, so its two layouts carry over: F <= 64: UB = 1, 16 waves, four per SIMD,
// 80 weight registers under 128; F <= 128: UB = 2, 8 waves, two per SIMD, 192 under 256.  Neither form uses scratch.
//
// Activations are split ONCE, by the thread that produces them: the staging thread splits the observation floats it fetched during
// the previous tile, the layer-1 epilogue splits relu(h1).  The LDS images are [agent][k] with k contiguous - one image of heads, one
// of tails, per layer - so a B fragment (B[k = 8 g + j][col = agent]) is one 16-byte read per image and k-step, and the C/D layout
// (col = agent, row = 4 g + reg: four consecutive units of one agent) is one 8-byte write per image.  A ds_read_b128 is served in
// four groups of 16 lanes - rows {0-3, 12-15} of one 16-byte k-chunk with rows {4-11} of the next, and the reverse - which must fall on
// 16 distinct 16-byte slots of the 64 banks.  The row images (64 or 128 bf16 per row) are padded by 16 bf16: with the row stride = 8
// dwords mod 64 they do, and the staging writes (ds_write_b32, one row per 32 lanes) are conflict-free too.  The h1 images (256 bf16 =
// 32 chunks per row) are not padded but swizzled: chunk q of row a lies at chunk q ^ (a & 15), which serves every read group from 16
// distinct slots AND spreads the 8-byte epilogue writes of 16 rows over 16 slots (2-way on the 32 banks a write sees; padded rows
// would make them 4-way).
//
//   per tile of R = 32 consecutive agents (two 16-agent column blocks: one A fragment feeds two MFMAs per product):
//     stage    split the prefetched floats -> xh, xl [agent][k]; k in [F, KX) written as zeros                        | barrier
//     finish   of the tile BEFORE: the last wave's first 32 threads add the NW partials in wave order and b3[0] - b3[1], softmax,
//              draw (mdr_draw.h), guarded stores - beside the other waves' layer 1, not between two barriers of its own
//     layer 1  B = xh / xl, C starts as the bias; relu; split; -> hh, hl [agent][unit], all 256 units                 | barrier
//     layer 2  B = hh / hl; relu; per-wave partial of the head's dot with W3[0] - W3[1] -> part[wave][agent]
//   and after the last tile one barrier and its finish.  part is written after a tile's second barrier and read after the next
//   tile's first, by a wave that reaches that tile's second barrier only when it has read it.
//
// An agent's arithmetic does not depend on where in a tile, a batch or a grid it sits: a column of an MFMA is the same sum whatever the
// column, the partials are added in wave order, there are no atomics.  Rows past the batch are staged as zeros and never stored.
// k-steps beyond F / H1 and waves beyond the net's sizes are skipped by wave-uniform branches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_bf16_split.h"
#include "mdr_draw.h"

namespace {

using mdr::action_uniform;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int MAX_F = 128, MAX_H = 256;
constexpr int R = 32;                 // agents per tile: two column blocks
constexpr int S2 = MAX_H / 32;        // k-steps of layer 2
constexpr int PAD = 16;               // bf16 of padding per row of the row images (see above)
constexpr int SH = MAX_H;             // row stride of the h1 images, in bf16: swizzled, not padded

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

// two floats -> the packed heads and the packed tails (a in the low half).  The plain conversion, not split8's assembly: these words
// go to LDS, never straight into an MFMA
__device__ __forceinline__ uint32_t pack2(float a, float b) { return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{a, b}), bf16x2)); }
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u));
}

// acc += wh bh + wl bh + wh bl
__device__ __forceinline__ f32x4 mma3(const uint4& wh, const uint4& wl, const bf16x8& bh, const bf16x8& bl, f32x4 acc) {
  const bf16x8 ah = __builtin_bit_cast(bf16x8, wh), al = __builtin_bit_cast(bf16x8, wl);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
}

__host__ __device__ constexpr int lds_bytes(int kx, int nw) { return 2 * R * (kx + PAD) * 2 + 2 * R * SH * 2 + (nw * R + 3 * MAX_H) * 4; }

// S1: k-steps of layer 1 the form holds registers for (32 S1 >= F); UB: 16-unit blocks per wave
template <int S1, int UB>
__global__ __launch_bounds__(64 * (16 / UB)) void k_mlp_actor_bf16(MlpActorArgs a) {
  constexpr int NW = 16 / UB, NT = 64 * NW, KX = 32 * S1, SX = KX + PAD;
  constexpr int KP = KX / 2;            // pairs of features per row
  constexpr int NPR = R * KP / NT;      // pairs of a tile a thread stages
  constexpr int RSTEP = NT / KP;        // ... which lie this many rows apart
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint16_t* xh = reinterpret_cast<uint16_t*>(lds);      // [R][SX] heads of the rows
  uint16_t* xl = xh + R * SX;                           // ... and their tails
  uint16_t* hh = xl + R * SX;                           // [R][SH] heads of relu(h1)
  uint16_t* hl = hh + R * SH;
  float* part = reinterpret_cast<float*>(hl + R * SH);  // [NW][16 cb + r]
  float* vb1 = part + NW * R;           // b1, b2, W3[0] - W3[1]: zero beyond the net's sizes
  float* vb2 = vb1 + MAX_H;
  float* vwd = vb2 + MAX_H;

  const int tid = threadIdx.x, F = a.F, H1 = a.H1, H2 = a.H2;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;

  // ---- once per workgroup: this wave's rows of W1 and W2, split, into registers
  uint4 w1h[UB][S1], w1l[UB][S1], w2h[UB][S2], w2l[UB][S2];
#pragma unroll
  for (int ub = 0; ub < UB; ++ub) {
    const int u = 16 * (w * UB + ub) + r;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w1[min(u, H1 - 1) * F + min(k, F - 1)];      // clamped address, then a select: no branch per register
        v[j] = (u < H1 && k < F) ? x : 0.0f;
      }
      split8(v, w1h[ub][s], w1l[ub][s]);
    }
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w2[min(u, H2 - 1) * H1 + min(k, H1 - 1)];
        v[j] = (u < H2 && k < H1) ? x : 0.0f;
      }
      split8(v, w2h[ub][s], w2l[ub][s]);
    }
  }
  for (int i = tid; i < MAX_H; i += NT) {
    vb1[i] = i < H1 ? a.b1[i] : 0.0f;
    vb2[i] = i < H2 ? a.b2[i] : 0.0f;
    vwd[i] = i < H2 ? a.w3[i] - a.w3[H2 + i] : 0.0f;
  }
  const float bias3 = a.b3[0] - a.b3[1];

  // staging: thread -> features 2 kp, 2 kp + 1 of the rows srow0 + j RSTEP of the tile.  Feature-fastest: a wave reads one or two whole
  // rows and writes one dword per lane to 32 consecutive banks
  const int kp = tid & (KP - 1), srow0 = tid / KP;
  float xr[NPR][2];
  auto fetch = [&](int64_t t) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) {
      const int64_t agent = t * R + srow0 + j * RSTEP;
      const bool ok = agent < a.A;
      const float* src = a.obs + (ok ? agent : 0) * a.ld;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool kok = ok && 2 * kp + e < F;
        const float v = src[kok ? 2 * kp + e : 0];      // a refused element reads the row's first float instead
        xr[j][e] = kok ? v : 0.0f;
      }
    }
  };
  if (blockIdx.x < a.ntiles) fetch(blockIdx.x);

  // the partials in wave order, the two-logit softmax and the draw of mdr_logits_sample: agent `i` of tile `t`
  auto finish = [&](int64_t t, int i) {
    float d = part[i];
#pragma unroll
    for (int v = 1; v < NW; ++v) d += part[v * R + i];
    d += bias3;
    const int64_t agent = t * R + i;
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
  };
  const bool finisher = w == NW - 1 && lane < R;
  const int hx = (g ^ r) * 8;      // h1 images: chunk 4 s + g of row 16 cb + r lies at chunk (4 s) ^ (g ^ r)

  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) {      // every feature up to KX - 1 is written: layer 1 reads zeros, not stale LDS, beyond F
      uint32_t h, l;
      split2(xr[j][0], xr[j][1], h, l);
      const int at = (srow0 + j * RSTEP) * (SX / 2) + kp;
      reinterpret_cast<uint32_t*>(xh)[at] = h;
      reinterpret_cast<uint32_t*>(xl)[at] = l;
    }
    __syncthreads();
    if (finisher && t != blockIdx.x) finish(t - gridDim.x, lane);      // ahead of the fetch: no tile in flight across the draw's registers
    if (t + gridDim.x < a.ntiles) fetch(t + gridDim.x);      // in flight during both layers

    // the sizes as this tile's own values (mdr_draw.h says why): the compiler otherwise computes the skip conditions of every k-step
    // once, ahead of the loop, and keeps them in scalar registers
    const int Fk = (int)mdr::loop_local((uint32_t)F), H1k = (int)mdr::loop_local((uint32_t)H1);

    // ---- layer 1
    f32x4 acc[UB][2];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) acc[ub][0] = acc[ub][1] = *reinterpret_cast<const f32x4*>(vb1 + 16 * (w * UB + ub) + 4 * g);
    if (16 * w * UB < H1) {
#pragma unroll
      for (int s = 0; s < S1; ++s)
        if (32 * s < Fk) {
          bf16x8 bh[2], bl[2];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            bh[cb] = *reinterpret_cast<const bf16x8*>(xh + (16 * cb + r) * SX + 32 * s + 8 * g);
            bl[cb] = *reinterpret_cast<const bf16x8*>(xl + (16 * cb + r) * SX + 32 * s + 8 * g);
          }
#pragma unroll
          for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[ub][cb] = mma3(w1h[ub][s], w1l[ub][s], bh[cb], bl[cb], acc[ub][cb]);
        }
    }
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {      // every unit up to 255 is written: layer 2 reads zeros, not stale LDS, beyond H1
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = relu(acc[ub][0][i]), v[4 + i] = relu(acc[ub][1][i]);
      uint4 h, l;
      split8(v, h, l);
      const int at = r * SH + (((2 * (w * UB + ub) + (g >> 1)) ^ r) * 8) + 4 * (g & 1);      // units 16 blk + 4 g ..: half a chunk
      *reinterpret_cast<uint2*>(hh + at) = uint2{h.x, h.y};
      *reinterpret_cast<uint2*>(hl + at) = uint2{l.x, l.y};
      *reinterpret_cast<uint2*>(hh + at + 16 * SH) = uint2{h.z, h.w};
      *reinterpret_cast<uint2*>(hl + at + 16 * SH) = uint2{l.z, l.w};
    }
    __syncthreads();

    // ---- layer 2 and this wave's share of the head
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) acc[ub][0] = acc[ub][1] = *reinterpret_cast<const f32x4*>(vb2 + 16 * (w * UB + ub) + 4 * g);
    if (16 * w * UB < H2) {
#pragma unroll
      for (int s = 0; s < S2; ++s)
        if (32 * s < H1k) {
          bf16x8 bh[2], bl[2];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            bh[cb] = *reinterpret_cast<const bf16x8*>(hh + (16 * cb + r) * SH + ((32 * s) ^ hx));
            bl[cb] = *reinterpret_cast<const bf16x8*>(hl + (16 * cb + r) * SH + ((32 * s) ^ hx));
          }
#pragma unroll
          for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[ub][cb] = mma3(w2h[ub][s], w2l[ub][s], bh[cb], bl[cb], acc[ub][cb]);
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
  }
  __syncthreads();
  if (finisher && blockIdx.x < a.ntiles) {      // the last tile of this workgroup: blockIdx.x + gridDim.x floor((ntiles - 1 - blockIdx.x) / gridDim.x)
    const int64_t last = a.ntiles - 1 - (a.ntiles - 1 - blockIdx.x) % gridDim.x;
    finish(last, lane);
  }
}

template <int S1, int UB>
int launch(const MlpActorArgs& a, int64_t grid, hipStream_t st) {
  constexpr size_t bytes = (size_t)lds_bytes(32 * S1, 16 / UB);
  static_assert(bytes <= 64 * 1024, "beyond 64 KB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL((k_mlp_actor_bf16<S1, UB>), dim3((unsigned)grid), dim3(64 * (16 / UB)), bytes, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int mdr_mlp_actor_sample_bf16x3(const mdr_mlp_t* actor, const float* obs, int64_t ld_obs, int64_t nb_agents, uint64_t seed, uint64_t step,
                                const int32_t* step_dev, int32_t greedy, int32_t max_workgroups, uint8_t* action, float* a_prob,
                                float* probs, void* stream) {
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
  // one workgroup per compute unit, as mdr_mlp_actor_sample; the form depends on F alone, never on the batch: an agent's bits must not
  int64_t grid = a.ntiles < cus ? a.ntiles : cus;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  hipStream_t st = (hipStream_t)stream;
  return F <= 64 ? launch<2, 1>(a, grid, st) : launch<4, 2>(a, grid, st);
}

}  // extern "C"
