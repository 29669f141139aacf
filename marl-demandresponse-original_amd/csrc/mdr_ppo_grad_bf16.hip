// PPO's update step for the MLP actor and critic in the bf16x3 precision (include/mdr_policy.h: mdr_ppo_actor_grad_bf16x3,
// mdr_ppo_critic_grad_bf16x3): the chain of mdr_ppo_grad.hip - forward, loss, backward of one network for a minibatch in one launch,
// one partial gradient per workgroup, the reduction of mdr_grad_reduce.h behind it - with its five matrix products on
// v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_16x16x4_f32.  Two heads (HEAD_ACTOR, HEAD_CRITIC), the narrow limits (F <= 64,
// hidden <= 128, O = 2 / 1).
//
// Arithmetic.  Every operand of F1 (z1 = W1 x), F2 (z2 = W2 h1), B2 (dh1 = W2^T dz2), dW2 = dz2^T h1 and dW1 = dz1^T x is split
// a = ah + al, ah = bf16(a), al = bf16(a - ah), round to nearest even (mdr_bf16_split.h), and every product is ah bh + al bh + ah bl,
// accumulated in fp32.  Everything else is the fp32 kernel's, in fp32: biases (the accumulators start from them), ReLU, the logits
// and dW3 / db3 on the vector unit from the fp32 h2, the head's loss and dlogits, relu'(z) = [z > 0] on the kernel's own z, the
// bias gradients (per-lane fp32 sums of the unsplit dz, added across lanes once per launch), rows past the minibatch as zero states
// with zero dlogits: exact zeros.
//
// Design points.
//   weights   Wave w owns the 16-unit block w of both hidden layers for the whole launch, as in the fp32 kernel, so the A operands it
//             ever needs are three fixed fragments: rows of block w of W1 (F1), of W2 (F2) and of W2^T (B2).  They are read in
//             place in torch's layout at the start of every launch (the next call sees an optimiser step; nothing is packed on the
//             host), split once by split8 and kept in 80 registers: no weight image in LDS at all, no operand read per MFMA for A,
//             and W2^T costs a strided global read once per workgroup instead of a transposed LDS read per tile.  LDS is therefore
//             not the binding constraint here: 78,352 bytes for every covered shape, (64,128,128) included; no shape inside the
//             limits is refused.
//   images    Each activation image is split once, when it is written to LDS, into a head and a tail image of bf16 (together the 4
//             bytes per element of the fp32 image).  The forward products and B2 contract over units and read [row][unit]
//             images; the weight-gradient products contract over minibatch rows and read [unit][row] images.  x, h1 and dz2 are
//             needed both ways and are WRITTEN both ways (a second image: at 16 rows a [128][16] bf16 image is 6 KB), dz1 only
//             [unit][row], h2 stays fp32 (only the vector unit reads it).  ds_read_b64_tr_b16 was not tried.
//   tile      16 minibatch rows, as the fp32 kernel, so the grid, the workspace and mdr_mlp_grad_floats /
//             mdr_mlp_grad_workspace_bytes serve both precisions.  The weight-gradient products contract over 32 k-slots per
//             instruction; with 16 rows the upper half is not left zero but takes a cross term: slots 0..15 hold (dz_h, in_h) of the
//             tile's rows and slots 16..31 (dz_l, in_h), so A = [dz_h | dz_l], B = [in_h | in_h] is two of the three products and a
//             second instruction with B = [in_l | 0] the third - two MFMAs per output block and tile, not three.  A 32-row tile was
//             not built or measured.
//   barriers  The fp32 kernel's five per tile, for the same reasons; dz1 has an image of its own (no aliasing).
//   determinism  The accumulators of dW2, dW1, db2, db1, dW3 / db3 and the loss stay in registers for the whole launch, each workgroup
//             writes one partial, k_ppo_grad_reduce adds them in slot order.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_bf16_split.h"
#include "mdr_grad_reduce.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int NW = 8;                 // waves per workgroup = the most 16-unit blocks of a hidden layer
constexpr int TILE = 16;              // minibatch rows per tile
constexpr int MAX_F = 64, MAX_H = 128;
constexpr int S1 = MAX_F / 32, S2 = MAX_H / 32;      // k-steps of 32 the register fragments hold
constexpr int LIB_MAX_WG = 512;       // the library's own grid: min(tiles, CUs, this), as mdr_ppo_grad.hip
constexpr int SXR = MAX_F + 8;        // bf16 per row of the [row][feature] images (144 bytes: the 16-byte reads of 16 rows spread over the banks)
constexpr int SHR = MAX_H + 8;        // ... of the [row][unit] images
constexpr int SR = TILE + 8;          // ... of the [unit][row] images (48 bytes: 16-byte aligned halves)
constexpr int LT = 20;                // floats per row of the fp32 h2 image, as mdr_ppo_grad.hip

// LDS: bf16 images (offsets in uint16_t), then fp32 (offsets in floats behind them)
constexpr int O_XR = 0;                              // x     [16][SXR]   head, tail
constexpr int O_XC = O_XR + 2 * TILE * SXR;          // x     [64][SR]
constexpr int O_H1R = O_XC + 2 * MAX_F * SR;         // h1    [16][SHR]
constexpr int O_H1C = O_H1R + 2 * TILE * SHR;        // h1    [128][SR]
constexpr int O_D2R = O_H1C + 2 * MAX_H * SR;        // dz2   [16][SHR]
constexpr int O_D2C = O_D2R + 2 * TILE * SHR;        // dz2   [128][SR]
constexpr int O_D1C = O_D2C + 2 * MAX_H * SR;        // dz1   [128][SR]
constexpr int N_U16 = O_D1C + 2 * MAX_H * SR;
static_assert(N_U16 % 8 == 0, "the fp32 part starts 16-byte aligned");
constexpr int F_H2 = 0;                              // h2T   [128][LT]
constexpr int F_DL = F_H2 + MAX_H * LT;              // dlogits [wave][row][2]
constexpr int F_LP = F_DL + NW * TILE * 2;           // the logits' partial sums [wave][row][2]
constexpr int F_W3 = F_LP + NW * TILE * 2;           // W3 [2][128]
constexpr int F_B3 = F_W3 + 2 * MAX_H;
constexpr int N_F32 = F_B3 + 4;
constexpr size_t LDS_BYTES = (size_t)N_U16 * 2 + (size_t)N_F32 * 4;
static_assert(LDS_BYTES == 78352 && LDS_BYTES <= 160 * 1024, "one layout for every covered shape");

__host__ __device__ constexpr int blocks16(int n) { return (n + 15) / 16; }

struct Args {
  int F, H1, H2;
  int oW1, ob1, oW2, ob2, oW3, ob3, G, stride;      // the flat gradient's offsets and a partial's floats, as mdr_ppo_grad.hip's Shape
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float* state;
  int64_t ld_state;
  const int64_t* index;
  int64_t B, ntiles;
  const int64_t* action;      // actor
  const float* old_prob;      // actor
  const float* adv_in;        // actor: the advantage, minibatch order
  const float* target;        // critic: Gt, read through index
  float clip_lo, clip_hi;
  float* part;                // [gridDim.x][stride]
  float* out0;                // actor: ratio; critic: value (minibatch order, may be null)
  float* out1;                // critic: advantage (may be null)
};

enum Head : int { HEAD_CRITIC = 0, HEAD_ACTOR = 1 };

__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// two floats -> the packed heads and the packed tails (a in the low half), as mdr_mlp_actor_bf16.hip: the plain conversion, not
// split8's assembly - these words go to LDS, never straight into an MFMA
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

// the four values (units 4 g .. 4 g + 3 of a block, row c) a lane holds behind an MFMA: split, into the [row][unit] image `rows`
// (may be null) at rows + c * SHR + unit and into the [unit][row] image `cols` at cols + unit * SR + c; the tails `tail` uint16_t
// behind the heads in both
__device__ __forceinline__ void store_split(const f32x4& v, uint16_t* rows, int tail_r, uint16_t* cols, int tail_c, int unit, int c) {
  uint32_t h01, l01, h23, l23;
  split2(v[0], v[1], h01, l01);
  split2(v[2], v[3], h23, l23);
  if (rows) {
    *reinterpret_cast<uint2*>(rows + c * SHR + unit) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(rows + tail_r + c * SHR + unit) = uint2{l01, l23};
  }
  uint16_t* ch = cols + unit * SR + c;
  ch[0] = (uint16_t)h01, ch[SR] = (uint16_t)(h01 >> 16), ch[2 * SR] = (uint16_t)h23, ch[3 * SR] = (uint16_t)(h23 >> 16);
  uint16_t* cl = ch + tail_c;
  cl[0] = (uint16_t)l01, cl[SR] = (uint16_t)(l01 >> 16), cl[2 * SR] = (uint16_t)l23, cl[3 * SR] = (uint16_t)(l23 >> 16);
}

// the sum over the 16 lanes of a lane group (c = 0..15), in one fixed order
__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

template <Head HEAD>
__global__ __launch_bounds__(64 * NW) void k_ppo_grad_bf16(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int O = HEAD == HEAD_CRITIC ? 1 : 2;
  constexpr bool TWO = O == 2;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = a.F, H1 = a.H1, H2 = a.H2;
  const int nb1 = blocks16(H1), nb2 = blocks16(H2), nbf = blocks16(F);
  const int nkf = (F + 31) >> 5, nk1 = (nb1 + 1) >> 1, nk2 = (nb2 + 1) >> 1;      // k-steps of 32 over F, H1, H2
  uint16_t* img = reinterpret_cast<uint16_t*>(lds);
  uint16_t* xr = img + O_XR;
  uint16_t* xc = img + O_XC;
  uint16_t* h1r = img + O_H1R;
  uint16_t* h1c = img + O_H1C;
  uint16_t* d2r = img + O_D2R;
  uint16_t* d2c = img + O_D2C;
  uint16_t* d1c = img + O_D1C;
  constexpr int TXR = TILE * SXR, TXC = MAX_F * SR, THR = TILE * SHR, THC = MAX_H * SR;      // head -> tail
  float* fl = reinterpret_cast<float*>(img + N_U16);
  float* h2T = fl + F_H2;
  float* dl = fl + F_DL + w * (TILE * 2);      // the wave's own copy of the tile's dlogits [row][2]
  float* lp = fl + F_LP;
  float* W3s = fl + F_W3;
  float* b3s = fl + F_B3;

  // ---- once per workgroup.  Every image starts as zeros: the blocks no wave owns (w >= nb) are read by the k-steps of 32 that
  // reach past them and are never written
  for (int i = tid; i < N_U16 / 2; i += 64 * NW) reinterpret_cast<uint32_t*>(img)[i] = 0u;
  for (int i = tid; i < 2 * MAX_H; i += 64 * NW) {
    const int o = i / MAX_H, u = i - o * MAX_H;
    W3s[i] = (o < O && u < H2) ? a.w3[o * H2 + u] : 0.0f;
  }
  if (tid < 4) b3s[tid] = tid < O ? a.b3[tid] : 0.0f;

  // this wave's A fragments, split: lane (c, g) holds row 16 w + c, columns 32 s + 8 g .. + 7 (clamped address, then a select)
  uint4 w1h[S1], w1l[S1], w2h[S2], w2l[S2], wth[S2], wtl[S2];
  {
    const int u = 16 * w + c;
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w1[min(u, H1 - 1) * F + min(k, F - 1)];
        v[j] = (u < H1 && k < F) ? x : 0.0f;
      }
      split8(v, w1h[s], w1l[s]);
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
      split8(v, w2h[s], w2l[s]);
    }
#pragma unroll
    for (int s = 0; s < S2; ++s) {      // W2^T: row u of the fragment is column u of W2
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * s + 8 * g + j;
        const float x = a.w2[min(k, H2 - 1) * H1 + min(u, H1 - 1)];
        v[j] = (u < H1 && k < H2) ? x : 0.0f;
      }
      split8(v, wth[s], wtl[s]);
    }
  }
  // the biases of the lane's four accumulator rows (units 16 w + 4 g + i)
  f32x4 b1r, b2r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = 16 * w + 4 * g + i;
    b1r[i] = u < H1 ? a.b1[min(u, H1 - 1)] : 0.0f;
    b2r[i] = u < H2 ? a.b2[min(u, H2 - 1)] : 0.0f;
  }

  // the tile's states: thread -> row tid / 32, features 2 (tid % 32) and the next
  const int xrow = tid >> 5, xf = 2 * (tid & 31);
  float xn[2];
  auto load_x = [&](int64_t t) {
    const int64_t row = t * TILE + xrow;
    xn[0] = xn[1] = 0.0f;
    if (row < a.B) {
      const int64_t j = a.index ? a.index[row] : row;
      const float* p = a.state + j * a.ld_state;
      if (xf < F) xn[0] = p[xf];
      if (xf + 1 < F) xn[1] = p[xf + 1];
    }
  };
  auto store_x = [&]() {
    uint32_t h, l;
    split2(xn[0], xn[1], h, l);
    *reinterpret_cast<uint32_t*>(xr + xrow * SXR + xf) = h;
    *reinterpret_cast<uint32_t*>(xr + TXR + xrow * SXR + xf) = l;
    xc[xf * SR + xrow] = (uint16_t)h, xc[(xf + 1) * SR + xrow] = (uint16_t)(h >> 16);
    xc[TXC + xf * SR + xrow] = (uint16_t)l, xc[TXC + (xf + 1) * SR + xrow] = (uint16_t)(l >> 16);
  };

  f32x4 dW2[NW], dW1[MAX_F / 16], db2 = {0, 0, 0, 0}, db1 = {0, 0, 0, 0};      // db: the lane's rows (= c mod 16) only, summed at the end
#pragma unroll
  for (int i = 0; i < NW; ++i) dW2[i] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < MAX_F / 16; ++i) dW1[i] = f32x4{0, 0, 0, 0};
  float acc3 = 0.0f;      // lane (g < O, c): dW3[g][16 w + c];  lane (g == 2, c < O): db3[c]
  float loss = 0.0f;      // wave 0, lanes g == 0: the terms of the rows = c (mod 16) of this workgroup's tiles

  __syncthreads();        // the zeros are in place before the first image is written
  const int64_t first = blockIdx.x;
  if (first < a.ntiles) load_x(first);
  else xn[0] = xn[1] = 0.0f;
  store_x();
  __syncthreads();

  // where the lane reads its halves of the [unit][row] images: k-slots 0..15 (g < 2) take rows 8 g .. of the first image, k-slots
  // 16..31 rows 8 (g - 2) .. of the second
  const bool lower = g < 2;
  const int rsel = 8 * (g & 1);
  const bf16x8 zero8 = __builtin_bit_cast(bf16x8, uint4{0u, 0u, 0u, 0u});

  for (int64_t t = first; t < a.ntiles; t += gridDim.x) {
    const bool more = t + gridDim.x < a.ntiles;
    if (more) load_x(t + gridDim.x);      // lands during the tile's matrix work
    const int64_t row = t * TILE + c;
    const bool valid = row < a.B;

    // ---- F1
    f32x4 z1 = {0, 0, 0, 0};
    if (w < nb1) {
      z1 = b1r;
#pragma unroll
      for (int s = 0; s < S1; ++s)
        if (s < nkf) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(xr + c * SXR + 32 * s + 8 * g);
          const bf16x8 bl = *reinterpret_cast<const bf16x8*>(xr + TXR + c * SXR + 32 * s + 8 * g);
          z1 = mma3(w1h[s], w1l[s], bh, bl, z1);
        }
      f32x4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = fmaxf(z1[i], 0.0f);
      store_split(h, h1r, THR, h1c, THC, 16 * w + 4 * g, c);
    }
    __syncthreads();

    // ---- F2
    f32x4 z2 = {0, 0, 0, 0};
    if (w < nb2) {
      z2 = b2r;
#pragma unroll
      for (int s = 0; s < S2; ++s)
        if (s < nk1) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(h1r + c * SHR + 32 * s + 8 * g);
          const bf16x8 bl = *reinterpret_cast<const bf16x8*>(h1r + THR + c * SHR + 32 * s + 8 * g);
          z2 = mma3(w2h[s], w2l[s], bh, bl, z2);
        }
      // the block's share of the logits from the lane's own registers: four units per lane, the four lane groups by two shuffles
      const f32x4 w30 = *reinterpret_cast<const f32x4*>(W3s + 16 * w + 4 * g);
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + MAX_H + 16 * w + 4 * g);
      float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float h = fmaxf(z2[i], 0.0f);
        h2T[(16 * w + 4 * g + i) * LT + c] = h;
        p0 = fmaf(w30[i], h, p0);
        if (TWO) p1 = fmaf(w31[i], h, p1);
      }
      p0 += __shfl_xor(p0, 16);
      p0 += __shfl_xor(p0, 32);
      if (TWO) {
        p1 += __shfl_xor(p1, 16);
        p1 += __shfl_xor(p1, 32);
      }
      if (g == 0) {
        lp[(w * TILE + c) * 2] = p0;
        lp[(w * TILE + c) * 2 + 1] = p1;
      }
    }
    __syncthreads();

    // ---- head: logits of row c, every wave for itself (the same bits in all of them)
    float l0 = 0.0f, l1 = 0.0f;
#pragma unroll
    for (int b = 0; b < NW; ++b)      // the blocks' partial sums in block order
      if (b < nb2) {
        l0 += lp[(b * TILE + c) * 2];
        if (TWO) l1 += lp[(b * TILE + c) * 2 + 1];
      }
    l0 += b3s[0];
    if (TWO) l1 += b3s[1];
    float d0 = 0.0f, d1 = 0.0f, term = 0.0f;      // dlogits (before the 1 / B of the reduction) and the row's loss term
    if (valid) {
      const int64_t j = a.index ? a.index[row] : row;
      if constexpr (HEAD == HEAD_ACTOR) {
        // agents/ppo.py:153-166, statement for statement as mdr_ppo_grad.hip has it
        const bool act = a.action[j] != 0;
        const float d = act ? l1 - l0 : l0 - l1;
        const float pa = 1.0f / (1.0f + expf(-d)), pb = 1.0f / (1.0f + expf(d));
        const float ratio = pa / a.old_prob[j];
        const float adv = a.adv_in[row];
        const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi) * adv;
        term = -fminf(s1, s2);
        const bool active = (ratio >= a.clip_lo && ratio <= a.clip_hi) || s1 < s2;
        const float da = active ? (-adv * ratio) * pb : 0.0f;      // d term / d logit[a]; the other logit takes the negative
        d0 = act ? -da : da;
        d1 = act ? da : -da;
        if (w == 0 && g == 0 && a.out0) a.out0[row] = ratio;
      } else {
        // agents/ppo.py:149-150, 173: delta = Gt - V, value loss = mean(delta^2)
        const float adv = a.target[j] - l0;
        term = adv * adv;
        d0 = -2.0f * adv;
        if (w == 0 && g == 0) {
          if (a.out0) a.out0[row] = l0;
          if (a.out1) a.out1[row] = adv;
        }
      }
    }
    if (w == 0 && g == 0) loss += term;
    if (g == 0) {
      dl[2 * c] = d0;
      dl[2 * c + 1] = d1;
    }
    if (w < nb2) {
      const f32x4 w30 = *reinterpret_cast<const f32x4*>(W3s + 16 * w + 4 * g);
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + MAX_H + 16 * w + 4 * g);
      f32x4 dz;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dh = TWO ? fmaf(d0, w30[i], d1 * w31[i]) : d0 * w30[i];
        dz[i] = z2[i] > 0.0f ? dh : 0.0f;
      }
      db2 += dz;
      store_split(dz, d2r, THR, d2c, THC, 16 * w + 4 * g, c);
    }
    wave_lds_fence();
    if (w < nb2) {
      // dW2[16 w + m][16 ib + n] += sum_r dz2[r][16 w + m] h1[r][16 ib + n]: A = [dz2_h | dz2_l] over the 32 k-slots
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(d2c + (lower ? 0 : THC) + (16 * w + c) * SR + rsel);
#pragma unroll
      for (int ib = 0; ib < NW; ++ib)
        if (ib < nb1) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(h1c + (16 * ib + c) * SR + rsel);
          const bf16x8 bt = *reinterpret_cast<const bf16x8*>(h1c + THC + (16 * ib + c) * SR + rsel);
          dW2[ib] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bh, dW2[ib], 0, 0, 0);                       // dz_h h_h + dz_l h_h
          dW2[ib] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, lower ? bt : zero8, dW2[ib], 0, 0, 0);       // dz_h h_l
        }
      // the head's gradient, columns of block w: a chain over the tile's rows
      if (g < O) {
        const float* hr = h2T + (16 * w + c) * LT;
#pragma unroll
        for (int r = 0; r < TILE; ++r) acc3 = fmaf(dl[2 * r + g], hr[r], acc3);
      } else if (g == 2 && c < O) {
#pragma unroll
        for (int r = 0; r < TILE; ++r) acc3 += dl[2 * r + c];
      }
    }
    __syncthreads();

    // ---- B2
    if (w < nb1) {
      f32x4 dh = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < S2; ++s)
        if (s < nk2) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(d2r + c * SHR + 32 * s + 8 * g);
          const bf16x8 bl = *reinterpret_cast<const bf16x8*>(d2r + THR + c * SHR + 32 * s + 8 * g);
          dh = mma3(wth[s], wtl[s], bh, bl, dh);
        }
      f32x4 dz;
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[i] = z1[i] > 0.0f ? dh[i] : 0.0f;
      db1 += dz;
      store_split(dz, nullptr, 0, d1c, THC, 16 * w + 4 * g, c);
      wave_lds_fence();
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(d1c + (lower ? 0 : THC) + (16 * w + c) * SR + rsel);
#pragma unroll
      for (int ib = 0; ib < MAX_F / 16; ++ib)
        if (ib < nbf) {
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(xc + (16 * ib + c) * SR + rsel);
          const bf16x8 bt = *reinterpret_cast<const bf16x8*>(xc + TXC + (16 * ib + c) * SR + rsel);
          dW1[ib] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bh, dW1[ib], 0, 0, 0);
          dW1[ib] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, lower ? bt : zero8, dW1[ib], 0, 0, 0);
        }
    }
    __syncthreads();
    if (more) {
      store_x();
      __syncthreads();
    }
  }

  // ---- the workgroup's partial: every float of [0, G] exactly once
  float* part = a.part + (int64_t)blockIdx.x * a.stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    db1[i] = sum16(db1[i]);
    db2[i] = sum16(db2[i]);
  }
  if (w < nb1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = 16 * w + 4 * g + i;
      if (u < H1) {
#pragma unroll
        for (int ib = 0; ib < MAX_F / 16; ++ib)
          if (ib < nbf && 16 * ib + c < F) part[a.oW1 + u * F + 16 * ib + c] = dW1[ib][i];
        if (c == 0) part[a.ob1 + u] = db1[i];
      }
    }
  }
  if (w < nb2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = 16 * w + 4 * g + i;
      if (u < H2) {
#pragma unroll
        for (int ib = 0; ib < NW; ++ib)
          if (ib < nb1 && 16 * ib + c < H1) part[a.oW2 + u * H1 + 16 * ib + c] = dW2[ib][i];
        if (c == 0) part[a.ob2 + u] = db2[i];
      }
    }
    if (g < O && 16 * w + c < H2) part[a.oW3 + g * H2 + 16 * w + c] = acc3;
  }
  if (w == 0) {
    if (g == 2 && c < O) part[a.ob3 + c] = acc3;
    // the loss: the 16 lanes' sums in lane order
    if (g == 0) dl[c] = loss;
    wave_lds_fence();
    if (lane == 0) {
      float sum = 0.0f;
      for (int i = 0; i < TILE; ++i) sum += dl[i];
      part[a.G] = sum;
    }
  }
}

bool net_fields_ok(const mdr_mlp_t* n) {
  return n && n->struct_size == sizeof(mdr_mlp_t) && n->num_state > 0 && n->hidden1 > 0 && n->hidden2 > 0 && n->num_out > 0;
}

// the fp32 entry points' grid (mdr_ppo_grad.hip: launch_grid; the stride in run() is its Shape's), so that mdr_mlp_grad_workspace_bytes
// sizes the workspace of both.  That file stays as it is; tests/test_gpu_ppo_grad_bf16.py holds the two to each other: both entry
// points must write the same floats of a canaried workspace
int launch_grid(int64_t nb_rows, int32_t max_workgroups) {
  int dev = 0, cus = 256;
  if (max_workgroups == 0 &&
      (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess))
    cus = 256;
  const int64_t ntiles = (nb_rows + TILE - 1) / TILE;
  const int64_t cap = max_workgroups > 0 ? max_workgroups : (cus < LIB_MAX_WG ? cus : LIB_MAX_WG);
  const int64_t grid = ntiles < cap ? ntiles : cap;
  return (int)(grid > 0 ? grid : 1);
}

int run(Head head, const mdr_mlp_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows, const int64_t* action,
        const float* old_prob, const float* adv_in, const float* target, float clip, int32_t max_workgroups, void* workspace, float* grad,
        float* loss, float* out0, float* out1, void* stream) {
  if (!net_fields_ok(net) || !state || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  if (!(net->w1 && net->b1 && net->w2 && net->b2 && net->w3 && net->b3)) return MDR_ERR_INVALID;
  if (head == HEAD_ACTOR ? (!action || !old_prob || !adv_in || !(clip >= 0.0f && clip < 1.0f)) : !target) return MDR_ERR_INVALID;
  if (nb_rows < 0 || ld_state < net->num_state || max_workgroups < 0) return MDR_ERR_INVALID;
  if (net->num_state > MAX_F || net->hidden1 > MAX_H || net->hidden2 > MAX_H || net->num_out != (head == HEAD_CRITIC ? 1 : 2))
    return MDR_ERR_UNSUPPORTED;
  Args a{};
  const int F = net->num_state, H1 = net->hidden1, H2 = net->hidden2, O = net->num_out;
  a.F = F, a.H1 = H1, a.H2 = H2;
  a.oW1 = 0, a.ob1 = H1 * F, a.oW2 = a.ob1 + H1, a.ob2 = a.oW2 + H2 * H1, a.oW3 = a.ob2 + H2, a.ob3 = a.oW3 + O * H2, a.G = a.ob3 + O;
  a.stride = (a.G + 1 + 3) & ~3;
  hipStream_t st = (hipStream_t)stream;
  int grid = 0;
  if (nb_rows > 0) {
    grid = launch_grid(nb_rows, max_workgroups);
    a.w1 = net->w1, a.b1 = net->b1, a.w2 = net->w2, a.b2 = net->b2, a.w3 = net->w3, a.b3 = net->b3;
    a.state = state, a.ld_state = ld_state, a.index = index, a.B = nb_rows, a.ntiles = (nb_rows + TILE - 1) / TILE;
    a.action = action, a.old_prob = old_prob, a.adv_in = adv_in, a.target = target;
    a.clip_lo = (float)(1.0 - (double)clip), a.clip_hi = (float)(1.0 + (double)clip);
    a.part = static_cast<float*>(workspace), a.out0 = out0, a.out1 = out1;
    auto kernel = head == HEAD_ACTOR ? k_ppo_grad_bf16<HEAD_ACTOR> : k_ppo_grad_bf16<HEAD_CRITIC>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES) != hipSuccess)
      return MDR_ERR_HIP;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * NW), LDS_BYTES, st, a);
    if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
  }
  const int n = a.G + 1;
  hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(workspace), grid,
                     a.stride, a.G, (float)nb_rows, grad, loss);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int mdr_ppo_actor_grad_bf16x3(const mdr_mlp_t* actor, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                              const int64_t* action, const float* old_prob, const float* advantage, float clip_param, int32_t max_workgroups,
                              void* workspace, float* grad, float* loss, float* ratio, void* stream) {
  return run(HEAD_ACTOR, actor, state, ld_state, index, nb_rows, action, old_prob, advantage, nullptr, clip_param, max_workgroups, workspace, grad,
             loss, ratio, nullptr, stream);
}

int mdr_ppo_critic_grad_bf16x3(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                               const float* target, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* value,
                               float* advantage, void* stream) {
  return run(HEAD_CRITIC, critic, state, ld_state, index, nb_rows, nullptr, nullptr, nullptr, target, 0.0f, max_workgroups, workspace, grad, loss,
             value, advantage, stream);
}

}  // extern "C"
