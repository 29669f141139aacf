// Observe -> act for the actor of up to 256 hidden units per layer (include/mdr_policy.h: mdr_env_mlp_actor_sample,
// mdr_env_mlp_actor_sample_bf16x3): the 16-wave forms of k_mlp_actor (mdr_mlp_actor.hip) and k_mlp_actor_bf16 (mdr_mlp_actor_bf16.hip)
// fed from the env's compact state instead of observation rows.  A file of its own: the six kernels of those two files keep their
// code, their names and their registers (126 and 122 of the 128 a 16-wave workgroup has), whatever is tried here.
//
// Per tile of R = 32 consecutive agents ONE wavefront - the observer - builds the default observation (51 features) in an LDS window
// from about 33 bytes of state per house, with the staging of mdr_observe.h exactly as the TarMAC bf16x3 encode kernel drives it
// (ObserveWindow<32, STORE, GEN>: observe_load / observe_stage for tiles inside one env, the _gen forms with TileCursor and SegSlot
// for tiles that leave theirs, then the lockout quotients).  The window's float order is not normStateDict order and these kernels
// read W1 in place in torch's order, so the workgroup's staging step copies window float ObserveWindow::at(n) of agent a to feature n
// of the LDS image the rows form stages - xT[n][2 (a & 15) + (a >> 4)] in fp32, the split xh / xl at [a][n] in bf16x3; features 51
// .. 63 and agents past the batch are zeros.  From there on both layers, the head, the softmax, the draw (keyed by the agent's global
// index) and the stores are the rows kernels', statement for statement: the staged floats are the rows' bits and every MFMA chain takes
// them in the same order, so action, a_prob and probs are those of mdr_mlp_actor_sample[_bf16x3] on mdr_env_obs_vector's rows, bit for bit.
// STORE: the window is also written to rows_out through observe_build_table's offsets - bit for bit those rows - by observe_store_rows'
// stores spread over the whole workgroup (Observer::store_tile) when the tile is staged.
//
// Overlap, with ONE window.  The matrix pipe bounds these kernels and four waves share it, so what one wave adds on the memory,
// vector and LDS side is hidden as long as it comes early in a phase and no other wave waits for it alone:
//     stage    window -> xT | xh, xl, and -> rows_out (all threads)                                                    | barrier A
//     layer 1                                                                                                          | barrier B
//              the observer loads the compact state of the workgroup's NEXT tile, stages it into the window (free since A) and runs
//              the quotients - beside the other waves' layer 2, the long phase - and only then runs its own
//     layer 2  and the head's partials                                                                                 | barrier C
//     finish   (fp32: here, wave 0; bf16x3: after the next tile's barrier A, the last wave, as in the rows form)
// The bf16x3 rows form has no barrier C (its next tile is staged from registers); here the window must be complete before any wave
// reads it, so this form has one.  Issuing the loads behind barrier A already, so that they are in flight during layer 1, was tried
// and dropped: the 11 registers of compact state and the segment slot live across layer 1 on top of 80 of weights made six of the
// eight forms spill (8 - 36 bytes of scratch per lane).  As it is no form uses scratch (117 - 127 VGPRs).  A second window would not
// help: what it allows, staging during layer 1, puts the work into the short phase.
// The observer is a wave that does not also finish: the last one in fp32, the first in bf16x3.
// Measured (profiles/mlp_actor_observe_README.md): in fp32 the observer's work disappears beside a 12 us tile and the kernel is
// faster than the rows kernel alone; in bf16x3 a tile takes 3.7 us, the other waves wait for the observer and the kernel is slower
// than rows kernel + row kernel together.  Opt-in for that reason.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_bf16_split.h"
#include "mdr_draw.h"
#include "mdr_kernels.h"
#include "mdr_observe.h"

namespace {

using mdr::action_uniform;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int F = 51;                 // the default observation
constexpr int MAX_H = 256;
constexpr int R = 32;                 // agents per tile: two column blocks
constexpr int NW = 16, NT = 64 * NW;  // waves, threads: one 16-unit block of both hidden layers per wave
constexpr int KX = 64;                // features the LDS images hold

struct ObsActorArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int64_t A, ntiles;
  int H1, H2, greedy;
  uint32_t k0, k1, step_lo, step_hi;
  const int32_t* step_dev;
  uint8_t* action;
  float *a_prob, *probs;
  float* rows_out;
};

__device__ __forceinline__ float relu(float x) {      // mdr_policy.hip: max on the bit pattern, one instruction
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// ---- the observer's side, alike in both precisions
template <bool STORE, bool GEN>
struct Observer : ObserveWindow<R, STORE, GEN> {
  using W = ObserveWindow<R, STORE, GEN>;
  static constexpr size_t BYTES = W::WIN * sizeof(float) + (STORE ? R * F * sizeof(uint16_t) : 0);
  bool mine;      // this wave is the observer

  __device__ __forceinline__ Observer(const mdr::ObserveArgs& o, const ObsActorArgs& a) : W{o, a.rows_out, a.A, a.ntiles} {}

  // before the workgroup's first barrier: where the window lies, and the row table
  __device__ __forceinline__ void carve(float* behind, int tid, bool observer) {
    this->rows = behind;
    this->table = reinterpret_cast<uint16_t*>(behind + W::WIN);
    this->lane0 = tid & 63;
    mine = observer;
    if (STORE) observe_build_table<R, W::ROW>(this->table, tid, NT);
  }
  __device__ __forceinline__ void gather() {
    const int g = this->lane0 >> 4, r = this->lane0 & 15;
    this->lockout_quotients(r, g);
    this->lockout_quotients(16 + r, g);
  }
  // STORE: the complete window of tile t -> rows_out, by the whole workgroup beside its staging step - the tile's 32 x 51 contiguous
  // floats are at most 408 16-byte stores, one per thread (observe_store_rows, which one wave runs in seven rounds, spread out:
  // on the observer alone it cost more than the row kernel it replaces)
  __device__ __forceinline__ void store_tile(int64_t t, int tid) {
    if (!STORE) return;
    const int64_t first = t * R;
    const int n = (int)((this->A - first) < (int64_t)R ? (this->A - first) : (int64_t)R) * F;
    float* out = this->rows_out + first * F;
    const float* rows = this->rows;
    const uint16_t* table = this->table;
    if (((uintptr_t)out & 15u) != 0) {      // a buffer whose tiles are not 16-byte aligned: 4-byte stores
      for (int i = tid; i < n; i += NT) __builtin_nontemporal_store(rows[table[i]], out + i);
      return;
    }
    const int quads = n / 4, i = tid - quads;      // quads <= 408 < NT; the last tile of a batch may end in up to three single floats
    if (tid < quads) {
      const uint2 src = *reinterpret_cast<const uint2*>(table + 4 * tid);      // four 16-bit window offsets
      v4f_nt v = {rows[src.x & 0xFFFFu], rows[src.x >> 16], rows[src.y & 0xFFFFu], rows[src.y >> 16]};
      __builtin_nontemporal_store(v, reinterpret_cast<v4f_nt*>(out) + tid);
    } else if (i < n - 4 * quads) {
      out[4 * quads + i] = rows[table[4 * quads + i]];
    }
  }
  // behind that barrier: the workgroup's first tile, complete before the barrier that follows
  __device__ __forceinline__ void prime() {
    this->start(blockIdx.x, gridDim.x);
    if (!mine) return;
    for (int i = this->lane0; i < W::WIN; i += 64) this->rows[i] = 0.0f;
    observe_window_fence();
    if ((int64_t)blockIdx.x < this->ntiles) {
      this->load((int64_t)blockIdx.x * R);
      this->stage_rows();
      observe_window_fence();
      gather();
    }
  }
  // behind barrier B of tile t (the window was last read before barrier A): the workgroup's next tile into the window, before
  // this wave's layer 2
  __device__ __forceinline__ void restage(int64_t t) {
    this->advance(t);
    if (mine && this->more) {
      this->load(this->next_tile * R);
      this->stage_rows();
      observe_window_fence();
      gather();
    }
  }
};

// the finish of both forms: the partials in wave order, the two-logit softmax and the draw of mdr_logits_sample
__device__ __forceinline__ void finish(const ObsActorArgs& a, const float* part, float bias3, int64_t t, int i) {
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
}

// ================================================================ exact fp32: k_mlp_actor<16, 1> on the window

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int S1 = KX / 4, S2 = MAX_H / 4;      // k-steps of the two layers
constexpr int FP32_FLOATS = KX * R + MAX_H * R + NW * R + 3 * MAX_H;      // lds_floats(16, 16) of mdr_mlp_actor.hip

template <bool STORE, bool GEN>
__global__ __launch_bounds__(NT) void k_mlp_actor_observe(ObsActorArgs a, mdr::ObserveArgs o) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xT = lds;                      // [KX][2 r + cb]
  float* hT = xT + KX * R;              // [256][2 r + cb]
  float* part = hT + MAX_H * R;         // [NW][16 cb + r]
  float* vb1 = part + NW * R;           // b1, b2, W3[0] - W3[1]: zero beyond the net's sizes
  float* vb2 = vb1 + MAX_H;
  float* vwd = vb2 + MAX_H;

  const int tid = threadIdx.x, H1 = a.H1, H2 = a.H2;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;
  Observer<STORE, GEN> obs(o, a);
  obs.carve(vwd + MAX_H, tid, w == NW - 1);

  // ---- once per workgroup: this wave's rows of W1 and W2 into registers
  float w1[S1], w2[S2];
  {
    const int u = 16 * w + r;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      const int k = 4 * s + g;
      const float v = a.w1[min(u, H1 - 1) * F + min(k, F - 1)];      // clamped address, then a select: no branch per register
      w1[s] = (u < H1 && k < F) ? v : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < S2; ++s) {
      const int k = 4 * s + g;
      const float v = a.w2[min(u, H2 - 1) * H1 + min(k, H1 - 1)];
      w2[s] = (u < H2 && k < H1) ? v : 0.0f;
    }
  }
  for (int i = tid; i < MAX_H; i += NT) {
    vb1[i] = i < H1 ? a.b1[i] : 0.0f;
    vb2[i] = i < H2 ? a.b2[i] : 0.0f;
    vwd[i] = i < H2 ? a.w3[i] - a.w3[H2 + i] : 0.0f;
  }
  for (int i = F * R + tid; i < KX * R; i += NT) xT[i] = 0.0f;      // features F .. KX - 1: never staged, met by zero weights
  const float bias3 = a.b3[0] - a.b3[1];
  __syncthreads();      // the row table
  obs.prime();
  __syncthreads();      // the first window

  // staging: thread -> agent tid & 31 of the tile, features tid >> 5 and + 32, as the rows form
  const int srow = tid & (R - 1), kq = tid >> 5;
  float* const xdst = xT + kq * R + 2 * (srow & 15) + (srow >> 4);
  const float* const xsrc = obs.rows + srow * obs.ROW;

  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    obs.store_tile(t, tid);
    const bool ok = t * R + srow < a.A;      // agents past the batch: zeros
#pragma unroll
    for (int j = 0; j < KX / (NT / R); ++j) {
      const int n = kq + (NT / R) * j;
      if (n < F) {
        const float v = xsrc[obs.at(n)];
        xdst[(NT / R) * j * R] = ok ? v : 0.0f;
      }
    }
    __syncthreads();

    // the size as this tile's own value (mdr_draw.h says why)
    const int H1k = (int)mdr::loop_local((uint32_t)H1);

    // ---- layer 1
    f32x4 acc[2];
    acc[0] = acc[1] = *reinterpret_cast<const f32x4*>(vb1 + 16 * w + 4 * g);
    if (16 * w < H1) {
#pragma unroll
      for (int s = 0; s < S1; ++s) {      // F = 51: all four groups of k-steps
        const float2 b = *reinterpret_cast<const float2*>(xT + (4 * s + g) * R + 2 * r);
        acc[0] = mma(w1[s], b.x, acc[0]);
        acc[1] = mma(w1[s], b.y, acc[1]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)      // every unit up to 255 is written: layer 2 reads zeros, not stale LDS, beyond H1
      *reinterpret_cast<float2*>(hT + (16 * w + 4 * g + i) * R + 2 * r) = make_float2(relu(acc[0][i]), relu(acc[1][i]));
    __syncthreads();
    obs.restage(t);

    // ---- layer 2 and this wave's share of the head
    acc[0] = acc[1] = *reinterpret_cast<const f32x4*>(vb2 + 16 * w + 4 * g);
    if (16 * w < H2) {
#pragma unroll
      for (int q = 0; q < S2 / 4; ++q)
        if (16 * q < H1k) {
#pragma unroll
          for (int s = 4 * q; s < 4 * q + 4; ++s) {
            const float2 b = *reinterpret_cast<const float2*>(hT + (4 * s + g) * R + 2 * r);
            acc[0] = mma(w2[s], b.x, acc[0]);
            acc[1] = mma(w2[s], b.y, acc[1]);
          }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float d = 0.0f;
      const f32x4 wd = *reinterpret_cast<const f32x4*>(vwd + 16 * w + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) d = fmaf(wd[i], relu(acc[cb][i]), d);
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (g == 0) part[w * R + 16 * cb + r] = d;
    }
    __syncthreads();

    if (tid < R) finish(a, part, bias3, t, tid);
  }
}

// ================================================================ bf16x3: k_mlp_actor_bf16<2, 1> on the window

constexpr int B1 = KX / 32, B2 = MAX_H / 32;      // k-steps of the two layers
constexpr int PAD = 16;                           // bf16 of padding per row of the row images
constexpr int SX = KX + PAD, SH = MAX_H;          // row strides of the row images and of the (swizzled) h1 images, in bf16
constexpr int BF16_BYTES = 2 * R * SX * 2 + 2 * R * SH * 2 + (NW * R + 3 * MAX_H) * 4;      // lds_bytes(64, 16) of mdr_mlp_actor_bf16.hip

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

template <bool STORE, bool GEN>
__global__ __launch_bounds__(NT) void k_mlp_actor_observe_bf16(ObsActorArgs a, mdr::ObserveArgs o) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint16_t* xh = reinterpret_cast<uint16_t*>(lds);      // [R][SX] heads of the rows
  uint16_t* xl = xh + R * SX;                           // ... and their tails
  uint16_t* hh = xl + R * SX;                           // [R][SH] heads of relu(h1)
  uint16_t* hl = hh + R * SH;
  float* part = reinterpret_cast<float*>(hl + R * SH);  // [NW][16 cb + r]
  float* vb1 = part + NW * R;           // b1, b2, W3[0] - W3[1]: zero beyond the net's sizes
  float* vb2 = vb1 + MAX_H;
  float* vwd = vb2 + MAX_H;

  const int tid = threadIdx.x, H1 = a.H1, H2 = a.H2;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;
  Observer<STORE, GEN> obs(o, a);
  obs.carve(vwd + MAX_H, tid, w == 0);

  // ---- once per workgroup: this wave's rows of W1 and W2, split, into registers
  uint4 w1h[B1], w1l[B1], w2h[B2], w2l[B2];
  {
    const int u = 16 * w + r;
#pragma unroll
    for (int s = 0; s < B1; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w1[min(u, H1 - 1) * F + min(k, F - 1)];      // clamped address, then a select: no branch per register
        v[j] = (u < H1 && k < F) ? x : 0.0f;
      }
      split8(v, w1h[s], w1l[s]);
    }
#pragma unroll
    for (int s = 0; s < B2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w2[min(u, H2 - 1) * H1 + min(k, H1 - 1)];
        v[j] = (u < H2 && k < H1) ? x : 0.0f;
      }
      split8(v, w2h[s], w2l[s]);
    }
  }
  for (int i = tid; i < MAX_H; i += NT) {
    vb1[i] = i < H1 ? a.b1[i] : 0.0f;
    vb2[i] = i < H2 ? a.b2[i] : 0.0f;
    vwd[i] = i < H2 ? a.w3[i] - a.w3[H2 + i] : 0.0f;
  }
  const float bias3 = a.b3[0] - a.b3[1];
  __syncthreads();      // the row table
  obs.prime();
  __syncthreads();      // the first window

  // staging: thread -> features 2 kp, 2 kp + 1 of tile row tid / 32, as the rows form
  const int kp = tid & (KX / 2 - 1), srow = tid / (KX / 2);
  const float* const xsrc = obs.rows + srow * obs.ROW;
  const int n0 = 2 * kp, n1 = 2 * kp + 1;
  const bool finisher = w == NW - 1 && lane < R;
  const int hx = (g ^ r) * 8;      // h1 images: chunk 4 s + g of row 16 cb + r lies at chunk (4 s) ^ (g ^ r)

  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    obs.store_tile(t, tid);
    {      // every feature up to KX - 1 is written: zeros from F on and for agents past the batch
      const bool ok = t * R + srow < a.A;
      const float v0 = xsrc[obs.at(min(n0, F - 1))], v1 = xsrc[obs.at(min(n1, F - 1))];
      uint32_t h, l;
      split2(ok && n0 < F ? v0 : 0.0f, ok && n1 < F ? v1 : 0.0f, h, l);
      const int at = srow * (SX / 2) + kp;
      reinterpret_cast<uint32_t*>(xh)[at] = h;
      reinterpret_cast<uint32_t*>(xl)[at] = l;
    }
    __syncthreads();
    if (finisher && t != blockIdx.x) finish(a, part, bias3, t - gridDim.x, lane);

    // the size as this tile's own value (mdr_draw.h says why)
    const int H1k = (int)mdr::loop_local((uint32_t)H1);

    // ---- layer 1
    f32x4 acc[2];
    acc[0] = acc[1] = *reinterpret_cast<const f32x4*>(vb1 + 16 * w + 4 * g);
    if (16 * w < H1) {
#pragma unroll
      for (int s = 0; s < B1; ++s) {      // F = 51: both k-steps
        bf16x8 bh[2], bl[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          bh[cb] = *reinterpret_cast<const bf16x8*>(xh + (16 * cb + r) * SX + 32 * s + 8 * g);
          bl[cb] = *reinterpret_cast<const bf16x8*>(xl + (16 * cb + r) * SX + 32 * s + 8 * g);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[cb] = mma3(w1h[s], w1l[s], bh[cb], bl[cb], acc[cb]);
      }
    }
    {      // every unit up to 255 is written: layer 2 reads zeros, not stale LDS, beyond H1
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = relu(acc[0][i]), v[4 + i] = relu(acc[1][i]);
      uint4 h, l;
      split8(v, h, l);
      const int at = r * SH + (((2 * w + (g >> 1)) ^ r) * 8) + 4 * (g & 1);      // units 16 blk + 4 g ..: half a chunk
      *reinterpret_cast<uint2*>(hh + at) = uint2{h.x, h.y};
      *reinterpret_cast<uint2*>(hl + at) = uint2{l.x, l.y};
      *reinterpret_cast<uint2*>(hh + at + 16 * SH) = uint2{h.z, h.w};
      *reinterpret_cast<uint2*>(hl + at + 16 * SH) = uint2{l.z, l.w};
    }
    __syncthreads();
    obs.restage(t);

    // ---- layer 2 and this wave's share of the head
    acc[0] = acc[1] = *reinterpret_cast<const f32x4*>(vb2 + 16 * w + 4 * g);
    if (16 * w < H2) {
#pragma unroll
      for (int s = 0; s < B2; ++s)
        if (32 * s < H1k) {
          bf16x8 bh[2], bl[2];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            bh[cb] = *reinterpret_cast<const bf16x8*>(hh + (16 * cb + r) * SH + ((32 * s) ^ hx));
            bl[cb] = *reinterpret_cast<const bf16x8*>(hl + (16 * cb + r) * SH + ((32 * s) ^ hx));
          }
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) acc[cb] = mma3(w2h[s], w2l[s], bh[cb], bl[cb], acc[cb]);
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float d = 0.0f;
      const f32x4 wd = *reinterpret_cast<const f32x4*>(vwd + 16 * w + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) d = fmaf(wd[i], relu(acc[cb][i]), d);
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      if (g == 0) part[w * R + 16 * cb + r] = d;
    }
    __syncthreads();      // the window of the next tile is complete (and the partials of this one)
  }
  if (finisher && (int64_t)blockIdx.x < a.ntiles) {      // the last tile of this workgroup
    const int64_t last = a.ntiles - 1 - (a.ntiles - 1 - blockIdx.x) % gridDim.x;
    finish(a, part, bias3, last, lane);
  }
}

using ObserveKernel = void (*)(ObsActorArgs, mdr::ObserveArgs);

template <bool BF16>
ObserveKernel form(bool store, bool gen) {
  if constexpr (BF16)
    return store ? (gen ? k_mlp_actor_observe_bf16<true, true> : k_mlp_actor_observe_bf16<true, false>)
                 : (gen ? k_mlp_actor_observe_bf16<false, true> : k_mlp_actor_observe_bf16<false, false>);
  else
    return store ? (gen ? k_mlp_actor_observe<true, true> : k_mlp_actor_observe<true, false>)
                 : (gen ? k_mlp_actor_observe<false, true> : k_mlp_actor_observe<false, false>);
}

}  // namespace

namespace mdr {

int mlp_actor_observe_status(const mdr_mlp_t* actor, int32_t nb_houses) {
  if (!actor || actor->struct_size != sizeof(mdr_mlp_t)) return MDR_ERR_INVALID;
  if (!actor->w1 || !actor->b1 || !actor->w2 || !actor->b2 || !actor->w3 || !actor->b3) return MDR_ERR_INVALID;
  if (actor->hidden1 < 1 || actor->hidden1 > MAX_H || actor->hidden2 < 1 || actor->hidden2 > MAX_H || actor->num_out != 2) return MDR_ERR_UNSUPPORTED;
  if (actor->num_state != F || nb_houses < 2 * OBS_HALO + 1) return MDR_ERR_UNSUPPORTED;
  if (nb_houses % R != 0 && observe_window_lanes(nb_houses, 2 * OBS_HALO, R) > 64) return MDR_ERR_UNSUPPORTED;
  return MDR_OK;
}

int launch_mlp_actor_observe(const mdr_mlp_t* actor, const ObserveArgs& o, bool bf16x3, uint64_t seed, uint64_t step, const int32_t* step_dev,
                             int32_t greedy, int32_t max_workgroups, uint8_t* action, float* a_prob, float* probs, float* rows_out,
                             hipStream_t st) {
  if (!action || max_workgroups < 0 || o.E < 0) return MDR_ERR_INVALID;
  if (o.ext) return MDR_ERR_UNSUPPORTED;
  const int rc = mlp_actor_observe_status(actor, o.N);
  if (rc != MDR_OK) return rc;
  ObsActorArgs a{};
  a.w1 = actor->w1, a.b1 = actor->b1, a.w2 = actor->w2, a.b2 = actor->b2, a.w3 = actor->w3, a.b3 = actor->b3;
  a.A = (int64_t)o.E * o.N, a.ntiles = (a.A + R - 1) / R;
  a.H1 = actor->hidden1, a.H2 = actor->hidden2, a.greedy = greedy != 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.step_dev = step_dev;
  a.action = action, a.a_prob = a_prob, a.probs = probs, a.rows_out = rows_out;
  if (a.A == 0) return MDR_OK;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  // one workgroup per compute unit, as mdr_mlp_actor_sample: the weight registers allow no more
  int64_t grid = a.ntiles < cus ? a.ntiles : cus;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  const bool store = rows_out != nullptr, gen = o.N % R != 0;
  const size_t window = (size_t)R * TARMAC_OBS_ROW * sizeof(float) + (store ? (size_t)R * F * sizeof(uint16_t) : 0);
  const size_t bytes = (bf16x3 ? (size_t)BF16_BYTES : (size_t)FP32_FLOATS * sizeof(float)) + window;
  static_assert((size_t)BF16_BYTES + Observer<true, true>::BYTES <= 64 * 1024 && FP32_FLOATS * sizeof(float) + Observer<true, true>::BYTES <= 64 * 1024,
                "beyond 64 KB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  static_assert(BF16_BYTES % 16 == 0 && (FP32_FLOATS * sizeof(float)) % 16 == 0, "the window's rows are stored 16 bytes at a time");
  hipLaunchKernelGGL(bf16x3 ? form<true>(store, gen) : form<false>(store, gen), dim3((unsigned)grid), dim3(NT), bytes, st, a, o);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace mdr
