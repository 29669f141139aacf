// PPO's update step for the MLP actor and critic (include/mdr_policy.h: mdr_mlp_t, mdr_ppo_actor_grad, mdr_ppo_critic_grad), DQN's /
// DDQN's on the same network (mdr_dqn_target, mdr_dqn_grad) and MAPPO's centralised critic (mdr_mappo_critic_grad): one kernel body,
// five heads.
//
// Reference: PPO.update (agents/ppo.py:139-188) evaluates, per minibatch, Actor / Critic (agents/network.py:14-57: Linear(F,H1) - ReLU -
// Linear(H1,H2) - ReLU - Linear(H2,O)), forms the clipped surrogate (ppo.py:157-166) or F.mse_loss(Gt, V) (ppo.py:173) and calls
// backward().  Here one launch does forward, loss and backward of one network for a minibatch and leaves the loss and the flat gradient
// dW1 | db1 | dW2 | db2 | dW3 | db3 in torch's [out][in] layout; a second small launch sums the workgroups' partials in one fixed order
// and scales by 1 / B.  No floating-point atomics: the same inputs and the same grid give the same bits.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 (A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: col = l & 15, row = 4 (l >> 4) +
// reg).  At 32 cycles per instruction and SIMD the matrix pipe leaves room for two LDS operand reads per MFMA, so every operand comes
// from LDS and the work of a tile of 16 minibatch rows is split over the 8 waves of a persistent workgroup by 16-unit OUTPUT block:
// wave w owns block w of both hidden layers (H <= 128: at most 8 blocks) through the whole launch.
//
//   stage    W1 [H1p][ld1], W2 [H2p][ld2] in torch's layout, zero-padded to whole blocks, ld = 4 (mod 32): the 64 lanes of an A read
//            (W[16 w + m][4 q + g], forward) fall two on each bank; the transposed read of the backward (W2[4 q + g][16 w + m]) at
//            most four.  Biases and W3 behind them.  Once per workgroup.
//   x        the tile's state rows, gathered through `index`, transposed into xT [feature][row] (row stride LT = 20: the reads
//            [16 b + n][4 s + g] of the weight-gradient products fall two on each bank, the forward's [4 q + g][r] at most three)
//   F1       z1 block w = b1 + W1 x (units on the MFMA row index, the tile's rows on the column index)      -> h1T = relu(z1)
//   F2       z2 block w = b2 + W2 h1                                                                       -> h2T
//            and the block's share of the O logits from the same registers (four fmas per lane, two shuffles)      -> lp
//   head     every wave: the logits of the 16 rows = the blocks' shares in block order + b3, the loss term and dlogits of its
//            row on the vector unit; dz2 block w = relu'(z2) (dlogits . W3)                                -> dz2T
//            and, from the block it has just written: dW2 rows of block w += dz2^T h1 (k = the tile's rows), db2 (the same
//            product against ones), dW3 / db3 columns of block w on the vector unit
//   B2       dh1 block w = W2^T dz2 (A = W2 read transposed), dz1 = relu'(z1) dh1                           -> dz1T
//            and dW1 rows of block w += dz1^T x, db1
// Five barriers per tile.  The accumulators of the three weight gradients stay in registers for the whole launch (dW2 8 blocks, dW1
// 4 blocks - 8 in the wide instantiations below -, two bias blocks, one head register: 57 or 73 registers); each workgroup writes its partial once.  relu'(z) = 1 iff z > 0.
// Rows past the minibatch are forwarded as zero states and given zero dlogits: they add exact zeros.
//
// DQN.update / DDQN.update (agents/dqn.py:84-146) take two more heads of the same body.  HEAD_TARGET is forward only - staging, F1, F2
// and the logits as above, then wave 0 writes next_q = max(Q0, Q1) (or Q[pick], DDQN's gather), y = reward + gamma next_q and the
// argmax; no h2T / dz images, no accumulators, no partials, three barriers per tile.  HEAD_HUBER is the actor's chain with
// nn.SmoothL1Loss (beta = 1) on the taken action's Q-value against y.  Its reduction clamps every gradient element (dqn.py:108-109).
//
// MAPPO.update (agents/mappo.py:85-89, 113-116) evaluates Critic(num_state + nb_agents - 1) on torch.cat((state, others_actions)).
// HEAD_JOINT is HEAD_CRITIC's chain on that joint input of J = F + (N - 1) <= 128 features; only the tile image differs: rows 0..F-1
// of xT are the state's, row F + k of transition j is the action of the k-th OTHER agent of j's env (train_mappo.py:79-84: the step's
// action dict without agent a = j % N, in agent order), read from the `action` buffer while the tile is staged - the env-mates of
// row j are the N entries from j - a on (collect_ppo_rollout's flat layout: the agent index runs fastest).  No others_actions
// tensor is read or needed.
//
// The input width is a compile-time property of the instantiation, independent of the head: MAXF = 64 (4 dW1 blocks per wave, 2 tile
// elements per thread) or MAXF = 128 (8 and 4).  HEAD_JOINT has the wide form only; the other four heads have both, the narrow one
// behind the entry points of up to 64 features, the wide one behind the mdr_*_wide entry points for 65..128 (the optional message
// columns: 81, 91, 121 features).  The wide entry points lay LDS out with dz1T in h2T's storage (make_shape: `alias`), which is
// what a 100-100 network needs at 101..128 inputs; the layout is a property of the Shape, not of the code.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_grad_reduce.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NW = 8;                 // waves per workgroup = the most 16-unit blocks of a hidden layer
constexpr int TILE = 16;              // minibatch rows per tile
constexpr int LT = 20;                // row stride of the transposed tile images
constexpr int MAX_F = 64, MAX_H = 128;
constexpr int MAX_J = 128;           // HEAD_JOINT: state + others' actions
constexpr int MAX_WIDE = 128;        // the wide instantiations of the other heads
constexpr int LIB_MAX_WG = 512;       // the library's own grid: min(tiles, CUs, this)
constexpr size_t LDS_LIMIT = 160 * 1024;

__host__ __device__ constexpr int blocks16(int n) { return (n + 15) / 16; }
// smallest stride >= n that is 4 (mod 32)
__host__ __device__ constexpr int ld_for(int n) { return ((n + 27) / 32) * 32 + 4; }

struct Shape {
  int F, H1, H2, O;
  int nbf, nb1, nb2;            // 16-blocks of F, H1, H2
  int ld1, ld2;
  int oW1, ob1, oW2, ob2, oW3, ob3, G;      // offsets into the flat gradient; G floats
  int stride;                   // floats per workgroup partial: G + 1 (the loss), rounded up to 4
  // LDS offsets (floats)
  int sW1, sW2, sb1, sb2, sW3, sb3, sx, sh1, sh2, sdz2, sdz1, sdl, slp, lds;
};

// backward == false (HEAD_TARGET): no h2T, dz2T, dz1T and dlogits images
//
// alias == true (the wide entry points): dz1T lies in h2T's storage, one image of max(H1p, H2p) rows.  The two never hold live data
// at once, and every access of either is to the wave's own block w:
//   h2T   written in F2 (wave w, rows 16 w .. 16 w + 15), last read by the dW3 chain of the head section (wave w, the same rows),
//         which lies before the barrier that opens B2;
//   dz1T  written in B2 (wave w, rows of block w) and read only there (dW1 / db1 of block w, behind the wave's fence); B2 ends in a
//         barrier;
//   h2T's next write is in the next tile's F2, behind that tile's F1 barrier (and the barrier after store_x).
// So every read of h2T is separated by a barrier from the dz1T writes that follow it, and every read of dz1T by two barriers from the
// h2T writes that follow.  HEAD_TARGET has neither image.
__host__ __device__ constexpr Shape make_shape(int F, int H1, int H2, int O, bool backward = true, bool alias = false) {
  Shape s{};
  s.F = F, s.H1 = H1, s.H2 = H2, s.O = O;
  s.nbf = blocks16(F), s.nb1 = blocks16(H1), s.nb2 = blocks16(H2);
  s.ld1 = ld_for(4 * ((F + 3) / 4)), s.ld2 = ld_for(16 * s.nb1);
  s.oW1 = 0, s.ob1 = H1 * F, s.oW2 = s.ob1 + H1, s.ob2 = s.oW2 + H2 * H1, s.oW3 = s.ob2 + H2, s.ob3 = s.oW3 + O * H2, s.G = s.ob3 + O;
  s.stride = (s.G + 1 + 3) & ~3;
  const int H1p = 16 * s.nb1, H2p = 16 * s.nb2;
  s.sW1 = 0;
  s.sW2 = s.sW1 + H1p * s.ld1;
  s.sb1 = s.sW2 + H2p * s.ld2;
  s.sb2 = s.sb1 + H1p;
  s.sW3 = s.sb2 + H2p;
  s.sb3 = s.sW3 + 2 * H2p;
  s.sx = s.sb3 + 4;
  s.sh1 = s.sx + 16 * s.nbf * LT;
  s.sh2 = s.sh1 + H1p * LT;
  if (alias) {
    s.sdz1 = s.sh2;
    s.sdz2 = s.sh2 + (backward ? (H1p > H2p ? H1p : H2p) * LT : 0);
    s.sdl = s.sdz2 + (backward ? H2p * LT : 0);
  } else {
    s.sdz2 = s.sh2 + (backward ? H2p * LT : 0);
    s.sdz1 = s.sdz2 + (backward ? H2p * LT : 0);
    s.sdl = s.sdz1 + (backward ? H1p * LT : 0);
  }
  s.slp = s.sdl + (backward ? NW * TILE * 2 : 0);
  s.lds = s.slp + NW * TILE * 2;
  return s;
}

// What the aliased layout buys, by make_shape's own arithmetic (bytes of LDS against the 160 KiB of a workgroup)
constexpr size_t lds_bytes_of(int F, int H1, int H2, bool alias) { return (size_t)make_shape(F, H1, H2, 2, true, alias).lds * sizeof(float); }
static_assert(lds_bytes_of(121, 100, 100, true) == 159248 && lds_bytes_of(128, 100, 100, true) == 159248, "100-100: every F <= 128 fits aliased");
static_assert(lds_bytes_of(121, 100, 100, false) == 168208 && lds_bytes_of(121, 100, 100, false) > LDS_LIMIT, "100-100 at F = 121 needs the alias");
static_assert(lds_bytes_of(100, 128, 128, true) == 162576 && lds_bytes_of(100, 128, 128, true) <= LDS_LIMIT, "128-128: up to F = 100");
static_assert(lds_bytes_of(101, 128, 128, true) > LDS_LIMIT, "128-128 at F = 101 (ld1 steps from 100 to 132): refused by the LDS-fit check");
static_assert(lds_bytes_of(64, 128, 128, false) <= LDS_LIMIT, "every shape of the narrow entry points fits un-aliased");

struct GradArgs {
  Shape s;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float* state;
  int64_t ld_state;
  const int64_t* index;
  int64_t B, ntiles;
  const int64_t* action;      // actor, Huber
  const float* old_prob;      // actor
  const float* adv_in;        // actor: the advantage; Huber: y.  Minibatch order
  const float* target;        // critic: Gt; TD target: reward.  Read through index
  float clip_lo, clip_hi;
  float* part;                // [gridDim.x][stride]
  float* out0;                // actor: ratio; critic: value; TD target: y; Huber: q      (minibatch order, may be null)
  float* out1;                // critic: advantage; TD target: next_q                     (may be null)
  // behind the fields of the PPO heads, which keep their offsets
  const uint8_t* pick;        // TD target: the action whose Q-value is taken (minibatch order); null: the larger one
  uint8_t* amax;              // TD target: Q1 > Q0 (minibatch order, may be null)
  float gamma;                // TD target
  int32_t Fs, N;              // joint critic: the state's features (s.F = Fs + N - 1) and the agents per env; `action` the whole buffer
};

enum Head : int { HEAD_CRITIC = 0, HEAD_ACTOR = 1, HEAD_TARGET = 2, HEAD_HUBER = 3, HEAD_JOINT = 4 };

__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// dst [rows_p][ld] <- src [rows][cols] (torch layout), zeros in the padding
__device__ __forceinline__ void stage_matrix(float* dst, const float* src, int rows, int cols, int rows_p, int ld, int tid) {
  for (int i = tid; i < rows_p * ld; i += 64 * NW) {
    const int r = i / ld, c = i - r * ld;
    dst[i] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0.0f;
  }
}

template <Head HEAD, int MAXF>
__global__ __launch_bounds__(64 * NW) void k_ppo_grad(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Shape& s = a.s;
  constexpr bool JOINT = HEAD == HEAD_JOINT;
  constexpr int O = (HEAD == HEAD_CRITIC || JOINT) ? 1 : 2;
  static_assert(MAXF == MAX_F || MAXF == MAX_WIDE, "input features of this instantiation: 64 or 128");
  static_assert(!JOINT || MAXF == MAX_J, "the joint head has the wide form only");
  constexpr int NX = MAXF * TILE / (64 * NW);         // tile elements per thread
  constexpr bool TWO = O == 2;                        // a second logit
  constexpr bool BACKWARD = HEAD != HEAD_TARGET;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nb1 = s.nb1, nb2 = s.nb2, nbf = s.nbf;
  const int H1p = 16 * nb1, H2p = 16 * nb2, Fp = 16 * nbf;
  float* W1s = lds + s.sW1;
  float* W2s = lds + s.sW2;
  float* b1s = lds + s.sb1;
  float* b2s = lds + s.sb2;
  float* W3s = lds + s.sW3;      // [2][H2p]
  float* b3s = lds + s.sb3;
  float* xT = lds + s.sx;
  float* h1T = lds + s.sh1;
  float* h2T = lds + s.sh2;
  float* dz2T = lds + s.sdz2;
  float* dz1T = lds + s.sdz1;
  float* dl = lds + s.sdl + w * (TILE * 2);      // the wave's own copy of the tile's dlogits [row][2]
  float* lp = lds + s.slp;                       // [wave][row][2]: the logits' partial sums over the wave's block of h2

  stage_matrix(W1s, a.w1, s.H1, s.F, H1p, s.ld1, tid);
  stage_matrix(W2s, a.w2, s.H2, s.H1, H2p, s.ld2, tid);
  for (int i = tid; i < H1p; i += 64 * NW) b1s[i] = i < s.H1 ? a.b1[i] : 0.0f;
  for (int i = tid; i < H2p; i += 64 * NW) b2s[i] = i < s.H2 ? a.b2[i] : 0.0f;
  for (int i = tid; i < 2 * H2p; i += 64 * NW) {
    const int o = i / H2p, u = i - o * H2p;
    W3s[i] = (o < O && u < s.H2) ? a.w3[o * s.H2 + u] : 0.0f;
  }
  if (tid < 4) b3s[tid] = tid < O ? a.b3[tid] : 0.0f;

  // the tile's states: element e = tid + 512 i of the [row][Fp] image, NX per thread at most (16 x 64 / 512 = 2; wide: 16 x 128 / 512 = 4)
  float xn[NX];
  auto load_x = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + 64 * NW * i;
      const int r = e / Fp, f = e - r * Fp;
      const int64_t row = t * TILE + r;
      xn[i] = 0.0f;
      if (r < TILE && f < s.F && row < a.B) {
        const int64_t j = a.index ? a.index[row] : row;
        if constexpr (JOINT) {
          if (f < a.Fs) {
            xn[i] = a.state[j * a.ld_state + f];
          } else {
            // train_mappo.py:79-84: the k-th other agent of agent ag is agent k (k < ag) or k + 1 (k >= ag) of the same env
            const int k = f - a.Fs;
            const int64_t ag = j % a.N;
            xn[i] = a.action[j - ag + k + (k >= ag ? 1 : 0)] != 0 ? 1.0f : 0.0f;
          }
        } else {
          xn[i] = a.state[j * a.ld_state + f];
        }
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + 64 * NW * i;
      const int r = e / Fp, f = e - r * Fp;
      if (r < TILE) xT[f * LT + r] = xn[i];
    }
  };

  f32x4 dW2[NW], dW1[MAXF / 16], db2 = {0, 0, 0, 0}, db1 = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < NW; ++i) dW2[i] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < MAXF / 16; ++i) dW1[i] = f32x4{0, 0, 0, 0};
  float acc3 = 0.0f;      // lane (g < O, c): dW3[g][16 w + c];  lane (g == 2, c < O): db3[c]
  float loss = 0.0f;      // wave 0, lanes g == 0: the terms of the rows = c (mod 16) of this workgroup's tiles

  const int64_t first = blockIdx.x;
  if (first < a.ntiles) {
    load_x(first);
  } else {
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = 0.0f;
  }
  store_x();
  __syncthreads();

  for (int64_t t = first; t < a.ntiles; t += gridDim.x) {
    const bool more = t + gridDim.x < a.ntiles;
    if (more) load_x(t + gridDim.x);      // lands during the tile's matrix work
    const int64_t row = t * TILE + c;
    const bool valid = row < a.B;

    // ---- F1
    f32x4 z1 = {0, 0, 0, 0};
    if (w < nb1) {
      z1 = *reinterpret_cast<const f32x4*>(b1s + 16 * w + 4 * g);
      const float* wa = W1s + (16 * w + c) * s.ld1 + g;
      const float* xb = xT + g * LT + c;
      const int ks = (s.F + 3) >> 2;
      f32x4 odd = {0, 0, 0, 0};      // two chains (even / odd k-steps): 40 cycles of dependent latency against 32 of issue; measured no gain at two waves per SIMD
      for (int q0 = 0; q0 < ks; q0 += 4) {      // four k-steps' operands in flight
#pragma unroll
        for (int q = q0; q < q0 + 4; q += 2) {
          if (q < ks) z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[4 * q], xb[4 * q * LT], z1, 0, 0, 0);
          if (q + 1 < ks) odd = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[4 * q + 4], xb[(4 * q + 4) * LT], odd, 0, 0, 0);
        }
      }
      z1 += odd;
#pragma unroll
      for (int i = 0; i < 4; ++i) h1T[(16 * w + 4 * g + i) * LT + c] = fmaxf(z1[i], 0.0f);
    }
    __syncthreads();

    // ---- F2
    f32x4 z2 = {0, 0, 0, 0};
    if (w < nb2) {
      z2 = *reinterpret_cast<const f32x4*>(b2s + 16 * w + 4 * g);
      const float* wa = W2s + (16 * w + c) * s.ld2 + g;
      const float* hb = h1T + g * LT + c;
      const int ks = 4 * nb1;
      f32x4 odd = {0, 0, 0, 0};
      for (int q0 = 0; q0 < ks; q0 += 4) {
#pragma unroll
        for (int q = q0; q < q0 + 4; q += 2) {
          z2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[4 * q], hb[4 * q * LT], z2, 0, 0, 0);
          odd = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[4 * q + 4], hb[(4 * q + 4) * LT], odd, 0, 0, 0);
        }
      }
      z2 += odd;
      // the block's share of the logits from the lane's own registers: four units per lane, the four lane groups by two shuffles
      const f32x4 w30 = *reinterpret_cast<const f32x4*>(W3s + 16 * w + 4 * g);
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + H2p + 16 * w + 4 * g);
      float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float h = fmaxf(z2[i], 0.0f);
        if (BACKWARD) h2T[(16 * w + 4 * g + i) * LT + c] = h;
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
    if constexpr (HEAD == HEAD_TARGET) {
      // agents/dqn.py:96-99 (DQN), 129-135 (DDQN): next_q = max_a Q(s', a) or Q(s', pick), y = reward + gamma next_q.  A tie takes
      // action 0 (torch.argmax: the first maximal index); a NaN Q1 is the maximum, as torch.max has it.  The product and the sum
      // are two statements: each rounds on its own (-ffp-contract=on fuses inside one expression only).
      if (valid && w == 0 && g == 0) {
        const bool top = l1 > l0;
        const bool take = a.pick ? a.pick[row] != 0 : (top || l1 != l1);
        const float nq = take ? l1 : l0;
        if (a.amax) a.amax[row] = top ? 1 : 0;
        if (a.out1) a.out1[row] = nq;
        if (a.out0) {
          const int64_t j = a.index ? a.index[row] : row;
          const float discounted = a.gamma * nq;
          a.out0[row] = a.target[j] + discounted;
        }
      }
      // xT was last read in F1, two barriers ago; lp is next written after the next tile's first barrier
      if (more) {
        store_x();
        __syncthreads();
      }
      continue;
    }
    float d0 = 0.0f, d1 = 0.0f, term = 0.0f;      // dlogits (before the 1 / B of the reduction) and the row's loss term
    if (valid) {
      const int64_t j = a.index ? a.index[row] : row;
      if constexpr (HEAD == HEAD_HUBER) {
        // agents/dqn.py:93, 102-103: nn.SmoothL1Loss() (beta = 1) of Q(s, action) against y; the gradient as torch's
        // smooth_l1_loss_backward takes it (delta itself on [-1, 1], a NaN included), the other logit's is 0
        const bool act = a.action[j] != 0;
        const float q = act ? l1 : l0;
        const float delta = q - a.adv_in[row];
        const float ad = fabsf(delta);
        term = ad < 1.0f ? 0.5f * delta * delta : ad - 0.5f;
        const float dq = delta < -1.0f ? -1.0f : (delta > 1.0f ? 1.0f : delta);
        d0 = act ? 0.0f : dq;
        d1 = act ? dq : 0.0f;
        if (w == 0 && g == 0 && a.out0) a.out0[row] = q;
      } else if constexpr (HEAD == HEAD_ACTOR) {
        // agents/ppo.py:153-166: ratio = pi(a) / old_prob, L = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A); torch passes the
        // gradient through min to the first argument unless the second is smaller, and through clamp inside the closed range
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
        // agents/ppo.py:149-150, 173 (agents/mappo.py:85-88, 113): delta = Gt - V, value loss = mean(delta^2)
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
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + H2p + 16 * w + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dh = TWO ? fmaf(d0, w30[i], d1 * w31[i]) : d0 * w30[i];
        dz2T[(16 * w + 4 * g + i) * LT + c] = z2[i] > 0.0f ? dh : 0.0f;
      }
    }
    wave_lds_fence();
    if (w < nb2) {
      // dW2[16 w + m][16 ib + n] += sum_r dz2[r][16 w + m] h1[r][16 ib + n]
      const float* da = dz2T + (16 * w + c) * LT + g;
      const float* hb = h1T + c * LT + g;
#pragma unroll
      for (int q = 0; q < TILE / 4; ++q) {
        const float av = da[4 * q];
        db2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.0f, db2, 0, 0, 0);
#pragma unroll
        for (int ib = 0; ib < NW; ++ib)
          if (ib < nb1) dW2[ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hb[16 * ib * LT + 4 * q], dW2[ib], 0, 0, 0);
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
      const float* wa = W2s + g * s.ld2 + 16 * w + c;
      const float* db = dz2T + g * LT + c;
      const int ks = 4 * nb2;
      f32x4 odd = {0, 0, 0, 0};
      for (int q0 = 0; q0 < ks; q0 += 4) {
#pragma unroll
        for (int q = q0; q < q0 + 4; q += 2) {
          dh = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[4 * q * s.ld2], db[4 * q * LT], dh, 0, 0, 0);
          odd = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[(4 * q + 4) * s.ld2], db[(4 * q + 4) * LT], odd, 0, 0, 0);
        }
      }
      dh += odd;
#pragma unroll
      for (int i = 0; i < 4; ++i) dz1T[(16 * w + 4 * g + i) * LT + c] = z1[i] > 0.0f ? dh[i] : 0.0f;
      wave_lds_fence();
      const float* da = dz1T + (16 * w + c) * LT + g;
      const float* xb = xT + c * LT + g;
#pragma unroll
      for (int q = 0; q < TILE / 4; ++q) {
        const float av = da[4 * q];
        db1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.0f, db1, 0, 0, 0);
#pragma unroll
        for (int ib = 0; ib < MAXF / 16; ++ib)
          if (ib < nbf) dW1[ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[16 * ib * LT + 4 * q], dW1[ib], 0, 0, 0);
      }
    }
    __syncthreads();
    if (more) {
      store_x();
      __syncthreads();
    }
  }

  if constexpr (!BACKWARD) return;
  // ---- the workgroup's partial: every float of [0, G] exactly once
  float* part = a.part + (int64_t)blockIdx.x * s.stride;
  if (w < nb1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = 16 * w + 4 * g + i;
      if (u < s.H1) {
#pragma unroll
        for (int ib = 0; ib < MAXF / 16; ++ib)
          if (ib < nbf && 16 * ib + c < s.F) part[s.oW1 + u * s.F + 16 * ib + c] = dW1[ib][i];
        if (c == 0) part[s.ob1 + u] = db1[i];
      }
    }
  }
  if (w < nb2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = 16 * w + 4 * g + i;
      if (u < s.H2) {
#pragma unroll
        for (int ib = 0; ib < NW; ++ib)
          if (ib < nb1 && 16 * ib + c < s.H1) part[s.oW2 + u * s.H1 + 16 * ib + c] = dW2[ib][i];
        if (c == 0) part[s.ob2 + u] = db2[i];
      }
    }
    if (g < O && 16 * w + c < s.H2) part[s.oW3 + g * s.H2 + 16 * w + c] = acc3;
  }
  if (w == 0) {
    if (g == 2 && c < O) part[s.ob3 + c] = acc3;
    // the loss: the 16 lanes' sums in lane order
    if (g == 0) dl[c] = loss;
    wave_lds_fence();
    if (lane == 0) {
      float sum = 0.0f;
      for (int i = 0; i < TILE; ++i) sum += dl[i];
      part[s.G] = sum;
    }
  }
}

// k_ppo_grad_reduce (mdr_grad_reduce.h): grad = (sum over the partials in workgroup order) / B, the loss behind it; B == 0: zeros

bool net_fields_ok(const mdr_mlp_t* n) {
  return n && n->struct_size == sizeof(mdr_mlp_t) && n->num_state > 0 && n->hidden1 > 0 && n->hidden2 > 0 && n->num_out > 0;
}
// wide: the mdr_*_wide entry points (up to MAX_WIDE features)
bool net_covered(const mdr_mlp_t* n, bool wide = false) {
  return n->num_state <= (wide ? MAX_WIDE : MAX_F) && n->hidden1 <= MAX_H && n->hidden2 <= MAX_H && (n->num_out == 1 || n->num_out == 2);
}
// A wide entry point takes the wide instantiation and the aliased layout from the first width the narrow one does not cover; up to
// MAX_F features it is its narrow sibling (every such shape fits un-aliased), so it returns that one's bits at that one's cost.
bool wide_form(const mdr_mlp_t* n, bool wide) { return wide && n->num_state > MAX_F; }

int64_t grid_for(int64_t nb_rows, int32_t max_workgroups, int cus) {
  const int64_t ntiles = (nb_rows + TILE - 1) / TILE;
  int64_t cap = max_workgroups > 0 ? max_workgroups : (cus < LIB_MAX_WG ? cus : LIB_MAX_WG);
  const int64_t grid = ntiles < cap ? ntiles : cap;
  return grid > 0 ? grid : 1;
}

// the library's grid for nb_rows > 0 (max_workgroups == 0: one workgroup per compute unit, LIB_MAX_WG at most)
int launch_grid(int64_t nb_rows, int32_t max_workgroups) {
  int dev = 0, cus = 256;
  if (max_workgroups == 0 &&
      (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess))
    cus = 256;
  return (int)grid_for(nb_rows, max_workgroups, cus);
}

void fill_rows(GradArgs& a, const mdr_mlp_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows) {
  a.w1 = net->w1, a.b1 = net->b1, a.w2 = net->w2, a.b2 = net->b2, a.w3 = net->w3, a.b3 = net->b3;
  a.state = state, a.ld_state = ld_state, a.index = index, a.B = nb_rows, a.ntiles = (nb_rows + TILE - 1) / TILE;
}

// wide: the MAXF = 128 instantiation (HEAD_JOINT has no other)
int launch(Head head, bool wide, const GradArgs& a, int grid, hipStream_t st) {
  auto kernel = head == HEAD_JOINT ? k_ppo_grad<HEAD_JOINT, MAX_J>
              : wide ? (head == HEAD_ACTOR    ? k_ppo_grad<HEAD_ACTOR, MAX_WIDE>
                        : head == HEAD_CRITIC ? k_ppo_grad<HEAD_CRITIC, MAX_WIDE>
                        : head == HEAD_TARGET ? k_ppo_grad<HEAD_TARGET, MAX_WIDE>
                                              : k_ppo_grad<HEAD_HUBER, MAX_WIDE>)
                     : (head == HEAD_ACTOR    ? k_ppo_grad<HEAD_ACTOR, MAX_F>
                        : head == HEAD_CRITIC ? k_ppo_grad<HEAD_CRITIC, MAX_F>
                        : head == HEAD_TARGET ? k_ppo_grad<HEAD_TARGET, MAX_F>
                                              : k_ppo_grad<HEAD_HUBER, MAX_F>);
  const size_t lds_bytes = (size_t)a.s.lds * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * NW), lds_bytes, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

bool net_pointers_ok(const mdr_mlp_t* n) { return n->w1 && n->b1 && n->w2 && n->b2 && n->w3 && n->b3; }

// the three heads with a backward: HEAD_ACTOR, HEAD_CRITIC, HEAD_HUBER (adv_in = y, grad_clamp > 0; 0 for the PPO heads: no clamp)
int run(Head head, const mdr_mlp_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
        const int64_t* action, const float* old_prob, const float* adv_in, const float* target, float clip, float grad_clamp,
        int32_t max_workgroups, void* workspace, float* grad, float* loss, float* out0, float* out1, void* stream, bool wide = false) {
  if (!net_fields_ok(net) || !state || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  if (!net_pointers_ok(net)) return MDR_ERR_INVALID;
  if (head == HEAD_ACTOR ? (!action || !old_prob || !adv_in || !(clip >= 0.0f && clip < 1.0f))
      : head == HEAD_HUBER ? (!action || !adv_in || !(grad_clamp > 0.0f))
                           : !target)
    return MDR_ERR_INVALID;
  if (nb_rows < 0 || ld_state < net->num_state || max_workgroups < 0) return MDR_ERR_INVALID;
  if (!net_covered(net, wide) || net->num_out != (head == HEAD_CRITIC ? 1 : 2)) return MDR_ERR_UNSUPPORTED;
  const bool wf = wide_form(net, wide);
  GradArgs a{};
  a.s = make_shape(net->num_state, net->hidden1, net->hidden2, net->num_out, true, wf);
  if ((size_t)a.s.lds * sizeof(float) > LDS_LIMIT) return MDR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  int grid = 0;
  if (nb_rows > 0) {
    grid = launch_grid(nb_rows, max_workgroups);
    fill_rows(a, net, state, ld_state, index, nb_rows);
    a.action = action, a.old_prob = old_prob, a.adv_in = adv_in, a.target = target;
    a.clip_lo = (float)(1.0 - (double)clip), a.clip_hi = (float)(1.0 + (double)clip);
    a.part = static_cast<float*>(workspace), a.out0 = out0, a.out1 = out1;
    if (launch(head, wf, a, grid, st) != MDR_OK) return MDR_ERR_HIP;
  }
  const int n = a.s.G + 1;
  if (head == HEAD_HUBER)
    hipLaunchKernelGGL(k_grad_reduce_clamped, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(workspace), grid,
                       a.s.stride, a.s.G, (float)nb_rows, grad_clamp, grad, loss);
  else
    hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(workspace), grid,
                       a.s.stride, a.s.G, (float)nb_rows, grad, loss);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// the wide entry points' size queries: the net is covered and its backward layout fits
bool wide_shape(const mdr_mlp_t* net, Shape* out) {
  if (!net_fields_ok(net) || !net_covered(net, true)) return false;
  *out = make_shape(net->num_state, net->hidden1, net->hidden2, net->num_out, true, wide_form(net, true));
  return (size_t)out->lds * sizeof(float) <= LDS_LIMIT;
}

// the joint critic's argument checks that need no device: MDR_OK, MDR_ERR_INVALID or MDR_ERR_UNSUPPORTED (the LDS fit included)
// (alias: mdr_mappo_critic_grad_wide's layout, the same kernel)
int joint_shape(const mdr_mlp_t* critic, int32_t nb_agents, Shape* out, bool alias = false) {
  if (!net_fields_ok(critic) || nb_agents < 1 || (int64_t)critic->num_state - (nb_agents - 1) < 1) return MDR_ERR_INVALID;
  if (critic->num_out != 1 || critic->num_state > MAX_J || critic->hidden1 > MAX_H || critic->hidden2 > MAX_H) return MDR_ERR_UNSUPPORTED;
  const Shape s = make_shape(critic->num_state, critic->hidden1, critic->hidden2, 1, true, alias);
  if ((size_t)s.lds * sizeof(float) > LDS_LIMIT) return MDR_ERR_UNSUPPORTED;
  if (out) *out = s;
  return MDR_OK;
}

// the joint head behind both entry points; alias: the wide one's LDS layout
int run_joint(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* action, int64_t nb_transitions,
                     int32_t nb_agents, const int64_t* index, int64_t nb_rows, const float* target, int32_t max_workgroups, void* workspace,
                     float* grad, float* loss, float* value, float* advantage, void* stream, bool alias) {
  if (!net_fields_ok(critic) || !net_pointers_ok(critic) || !state || !action || !target || !grad || !loss || !workspace ||
      ((uintptr_t)workspace & 15u))
    return MDR_ERR_INVALID;
  GradArgs a{};
  const int rc = joint_shape(critic, nb_agents, &a.s, alias);
  if (rc == MDR_ERR_INVALID) return rc;
  const int F = critic->num_state - (nb_agents - 1);
  if (ld_state < F || nb_transitions < 0 || nb_transitions % nb_agents != 0 || nb_rows < 0 || max_workgroups < 0) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  int grid = 0;
  if (nb_rows > 0) {
    grid = launch_grid(nb_rows, max_workgroups);
    fill_rows(a, critic, state, ld_state, index, nb_rows);
    a.action = action, a.target = target, a.Fs = F, a.N = nb_agents;
    a.part = static_cast<float*>(workspace), a.out0 = value, a.out1 = advantage;
    if (launch(HEAD_JOINT, true, a, grid, st) != MDR_OK) return MDR_ERR_HIP;
  }
  const int n = a.s.G + 1;
  hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(workspace), grid,
                     a.s.stride, a.s.G, (float)nb_rows, grad, loss);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// the TD target behind both entry points
int run_target(const mdr_mlp_t* target_net, const mdr_mlp_t* policy_net, const float* next_state, int64_t ld_state,
                      const int64_t* index, int64_t nb_rows, const float* reward, float gamma, int32_t max_workgroups, float* y,
                      float* next_q, uint8_t* next_action, void* stream, bool wide) {
  if (!net_fields_ok(target_net) || !net_pointers_ok(target_net) || !next_state || !reward || !y) return MDR_ERR_INVALID;
  if (policy_net && (!net_fields_ok(policy_net) || !net_pointers_ok(policy_net) || !next_action)) return MDR_ERR_INVALID;
  if (nb_rows < 0 || ld_state < target_net->num_state || max_workgroups < 0 || !(fabsf(gamma) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (!net_covered(target_net, wide) || target_net->num_out != 2) return MDR_ERR_UNSUPPORTED;
  const bool wf = wide_form(target_net, wide);
  if (policy_net && (policy_net->num_state != target_net->num_state || policy_net->hidden1 != target_net->hidden1 ||
                     policy_net->hidden2 != target_net->hidden2 || policy_net->num_out != 2))
    return MDR_ERR_UNSUPPORTED;
  GradArgs a{};
  a.s = make_shape(target_net->num_state, target_net->hidden1, target_net->hidden2, 2, false);
  if ((size_t)a.s.lds * sizeof(float) > LDS_LIMIT) return MDR_ERR_UNSUPPORTED;
  // the wide pair is accepted or refused together: a target for a network whose gradient call does not fit LDS serves no update
  Shape fit;
  if (wide && !wide_shape(target_net, &fit)) return MDR_ERR_UNSUPPORTED;
  if (nb_rows == 0) return MDR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int grid = launch_grid(nb_rows, max_workgroups);
  if (policy_net) {      // DDQN (agents/dqn.py:129): the policy net's argmax on the next states first - the two weight sets do not share LDS
    fill_rows(a, policy_net, next_state, ld_state, index, nb_rows);
    a.amax = next_action;
    if (launch(HEAD_TARGET, wf, a, grid, st) != MDR_OK) return MDR_ERR_HIP;
  }
  fill_rows(a, target_net, next_state, ld_state, index, nb_rows);
  a.target = reward, a.gamma = gamma, a.out0 = y, a.out1 = next_q;
  a.pick = policy_net ? next_action : nullptr;
  a.amax = policy_net ? nullptr : next_action;
  return launch(HEAD_TARGET, wf, a, grid, st);
}

}  // namespace

extern "C" {

int64_t mdr_mlp_grad_floats(const mdr_mlp_t* net) {
  if (!net_fields_ok(net) || !net_covered(net)) return -1;
  return make_shape(net->num_state, net->hidden1, net->hidden2, net->num_out).G;
}

int64_t mdr_mlp_grad_workspace_bytes(const mdr_mlp_t* net, int64_t nb_rows, int32_t max_workgroups) {
  if (!net_fields_ok(net) || !net_covered(net) || nb_rows < 0 || max_workgroups < 0) return -1;
  const Shape s = make_shape(net->num_state, net->hidden1, net->hidden2, net->num_out);
  // max_workgroups == 0: room for the library's grid on any device (no device call here)
  return grid_for(nb_rows, max_workgroups, LIB_MAX_WG) * s.stride * (int64_t)sizeof(float);
}

// the wide entry points' sizes: the limits and the LDS fit of the calls with a backward (the TD target's image is smaller)
int64_t mdr_mlp_wide_grad_floats(const mdr_mlp_t* net) {
  Shape s;
  return wide_shape(net, &s) ? s.G : -1;
}

int64_t mdr_mlp_wide_grad_workspace_bytes(const mdr_mlp_t* net, int64_t nb_rows, int32_t max_workgroups) {
  Shape s;
  if (!wide_shape(net, &s) || nb_rows < 0 || max_workgroups < 0) return -1;
  return grid_for(nb_rows, max_workgroups, LIB_MAX_WG) * s.stride * (int64_t)sizeof(float);
}

int mdr_ppo_actor_grad_wide(const mdr_mlp_t* actor, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                            const int64_t* action, const float* old_prob, const float* advantage, float clip_param, int32_t max_workgroups,
                            void* workspace, float* grad, float* loss, float* ratio, void* stream) {
  return run(HEAD_ACTOR, actor, state, ld_state, index, nb_rows, action, old_prob, advantage, nullptr, clip_param, 0.0f, max_workgroups,
             workspace, grad, loss, ratio, nullptr, stream, true);
}

int mdr_ppo_critic_grad_wide(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                             const float* target, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* value,
                             float* advantage, void* stream) {
  return run(HEAD_CRITIC, critic, state, ld_state, index, nb_rows, nullptr, nullptr, nullptr, target, 0.0f, 0.0f, max_workgroups, workspace,
             grad, loss, value, advantage, stream, true);
}

int mdr_dqn_grad_wide(const mdr_mlp_t* policy_net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                      const int64_t* action, const float* y, float grad_clamp, int32_t max_workgroups, void* workspace, float* grad,
                      float* loss, float* q, void* stream) {
  return run(HEAD_HUBER, policy_net, state, ld_state, index, nb_rows, action, nullptr, y, nullptr, 0.0f, grad_clamp, max_workgroups, workspace,
             grad, loss, q, nullptr, stream, true);
}

int mdr_ppo_actor_grad(const mdr_mlp_t* actor, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                       const int64_t* action, const float* old_prob, const float* advantage, float clip_param, int32_t max_workgroups,
                       void* workspace, float* grad, float* loss, float* ratio, void* stream) {
  return run(HEAD_ACTOR, actor, state, ld_state, index, nb_rows, action, old_prob, advantage, nullptr, clip_param, 0.0f, max_workgroups,
             workspace, grad, loss, ratio, nullptr, stream);
}

int mdr_ppo_critic_grad(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                        const float* target, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* value,
                        float* advantage, void* stream) {
  return run(HEAD_CRITIC, critic, state, ld_state, index, nb_rows, nullptr, nullptr, nullptr, target, 0.0f, 0.0f, max_workgroups, workspace,
             grad, loss, value, advantage, stream);
}

int64_t mdr_mappo_critic_grad_floats(const mdr_mlp_t* critic, int32_t nb_agents) {
  Shape s;
  return joint_shape(critic, nb_agents, &s) == MDR_OK ? s.G : -1;
}

int64_t mdr_mappo_critic_workspace_bytes(const mdr_mlp_t* critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups) {
  Shape s;
  if (joint_shape(critic, nb_agents, &s) != MDR_OK || nb_rows < 0 || max_workgroups < 0) return -1;
  return grid_for(nb_rows, max_workgroups, LIB_MAX_WG) * s.stride * (int64_t)sizeof(float);
}

int64_t mdr_mappo_critic_wide_grad_floats(const mdr_mlp_t* critic, int32_t nb_agents) {
  Shape s;
  return joint_shape(critic, nb_agents, &s, true) == MDR_OK ? s.G : -1;
}

int64_t mdr_mappo_critic_wide_workspace_bytes(const mdr_mlp_t* critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups) {
  Shape s;
  if (joint_shape(critic, nb_agents, &s, true) != MDR_OK || nb_rows < 0 || max_workgroups < 0) return -1;
  return grid_for(nb_rows, max_workgroups, LIB_MAX_WG) * s.stride * (int64_t)sizeof(float);
}

int mdr_mappo_critic_grad(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* action, int64_t nb_transitions,
                          int32_t nb_agents, const int64_t* index, int64_t nb_rows, const float* target, int32_t max_workgroups,
                          void* workspace, float* grad, float* loss, float* value, float* advantage, void* stream) {
  return run_joint(critic, state, ld_state, action, nb_transitions, nb_agents, index, nb_rows, target, max_workgroups, workspace, grad, loss,
                   value, advantage, stream, false);
}

int mdr_mappo_critic_grad_wide(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* action, int64_t nb_transitions,
                               int32_t nb_agents, const int64_t* index, int64_t nb_rows, const float* target, int32_t max_workgroups,
                               void* workspace, float* grad, float* loss, float* value, float* advantage, void* stream) {
  return run_joint(critic, state, ld_state, action, nb_transitions, nb_agents, index, nb_rows, target, max_workgroups, workspace, grad, loss,
                   value, advantage, stream, true);
}

int mdr_dqn_target(const mdr_mlp_t* target_net, const mdr_mlp_t* policy_net, const float* next_state, int64_t ld_state,
                   const int64_t* index, int64_t nb_rows, const float* reward, float gamma, int32_t max_workgroups, float* y, float* next_q,
                   uint8_t* next_action, void* stream) {
  return run_target(target_net, policy_net, next_state, ld_state, index, nb_rows, reward, gamma, max_workgroups, y, next_q, next_action, stream,
                    false);
}

int mdr_dqn_target_wide(const mdr_mlp_t* target_net, const mdr_mlp_t* policy_net, const float* next_state, int64_t ld_state,
                        const int64_t* index, int64_t nb_rows, const float* reward, float gamma, int32_t max_workgroups, float* y,
                        float* next_q, uint8_t* next_action, void* stream) {
  return run_target(target_net, policy_net, next_state, ld_state, index, nb_rows, reward, gamma, max_workgroups, y, next_q, next_action, stream,
                    true);
}

int mdr_dqn_grad(const mdr_mlp_t* policy_net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                 const int64_t* action, const float* y, float grad_clamp, int32_t max_workgroups, void* workspace, float* grad, float* loss,
                 float* q, void* stream) {
  return run(HEAD_HUBER, policy_net, state, ld_state, index, nb_rows, action, nullptr, y, nullptr, 0.0f, grad_clamp, max_workgroups, workspace,
             grad, loss, q, nullptr, stream);
}

}  // extern "C"
