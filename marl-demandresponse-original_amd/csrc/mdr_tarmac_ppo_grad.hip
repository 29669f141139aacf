// TarMAC-PPO's update step for the actor (include/mdr_policy.h: mdr_tarmac_net_t, mdr_tarmac_ppo_actor_grad).
//
// Reference: TarmacPPO.update (agents/tarmac_ppo.py:168-186) evaluates TarMAC_Actor (agents/network.py:201-238) on a minibatch of
// stored env-steps, forms the clipped surrogate and calls backward().  Here the actor's ten Linear layers run, forward and backward,
// as three kinds of kernels around the two attention kernels (mdr_tarmac.hip, mdr_tarmac_grad.hip):
//
//   k_tppo_o2h<false>    obs rows (gathered through `index`) -> relu(obs2hidden.0) -> obs2hidden.2 = x        -> cat[:, :H]
//   k_tppo_proj<false>   x -> tanh(hidden2{query,key,value}.0) -> .2                                          -> qkv [A][2K + V]
//   mdr_tarmac_comm      qkv -> comm                                                                         -> cat[:, H:]
//   k_tppo_head          cat = [x | comm] -> relu(head.0) -> logits -> p, ratio, loss term, dlogits -> dz -> d[x | comm] -> dcat;
//                        the head's weight gradients
//   mdr_tarmac_comm_backward   dcat[:, H:] -> dq | dk | dv                                                   -> dqkv
//   k_tppo_proj<true>    t = tanh(..) recomputed from x; the projections' weight gradients; dx = dcat[:, :H] + sum W0^T dt, in place
//   k_tppo_o2h<true>     t1 = relu(..) recomputed from the obs rows; obs2hidden's weight gradients
//   k_ppo_grad_reduce    the partials in slot order, divided by A
// Nothing but x, comm, q | k | v and their gradients passes through memory; the hidden activations (5 H floats per agent) are
// recomputed.  The encode side is split in two kernels in both directions because its weights (o2h 2 x 64 x 68, projections
// 4 x 64 x 68 floats) do not fit the 160 KB of a workgroup beside the tile images of the backward.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32, every operand from LDS, as k_ppo_grad (mdr_ppo_grad.hip): weights staged once per workgroup
// in torch's layout with a row stride of 4 (mod 32), tile images transposed [unit][agent] with row stride 20, a wave owns one 16-unit
// OUTPUT block of every layer and keeps that block's weight-gradient accumulators in registers for the whole launch.  H <= 64 is
// four blocks, so a workgroup of 8 waves works on TWO tiles of 16 agents at a time (waves 0-3 / 4-7) that share the staged weights;
// each half leaves its own partial gradient.  relu'(z) = 1 iff z > 0, tanh' = 1 - t^2.  Agents past the batch are forwarded as zero
// rows and given zero dlogits / dqkv / dx: they add exact zeros.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_grad_reduce.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SUB = 2;                // tiles a workgroup works on at a time
constexpr int WPS = 4;                // waves per tile = the most 16-unit blocks of a layer's output
constexpr int ST = 64 * WPS;          // threads per tile
constexpr int NT = ST * SUB;          // threads per workgroup
constexpr int TILE = 16;              // agents per tile
constexpr int LT = 20;                // row stride of the transposed tile images
constexpr int MAX_F = 64, MAX_H = 64, MAX_K = 16, MAX_V = 32, MAX_C = 64;
constexpr int LIB_MAX_WG = 512;       // the library's own grid: min(tile pairs, CUs, this)
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int64_t MAX_AGENTS = 0x7FFFFFFF - 16;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__host__ __device__ inline int blocks16(int n) { return (n + 15) / 16; }
// smallest stride >= n that is 4 (mod 32)
__host__ __device__ inline int ld_for(int n) { return ((n + 27) / 32) * 32 + 4; }

struct Net {
  int F, H, K, V, M, Q, comm;      // M = H + V (H without communication): the head's input; Q = 2 K + V
  int nbF, nbH, nbV, nbM, nb2;     // 16-blocks; nb2 = 2 + nbV: the blocks of the three projections' last layers side by side
  int Hp, ldF, ldH, ldM;
  int oE0w, oE0b, oE2w, oE2b, oH0w, oH0b, oH2w, oH2b;      // offsets into the flat gradient
  int oP0w[3], oP0b[3], oP2w[3], oP2b[3];                  // projection 0 query, 1 key, 2 value (the order of q | k | v)
  int G, stride;                   // G floats; floats per partial: G + 1 (the loss), rounded up to 4
};

__host__ __device__ inline Net make_net(int F, int H, int K, int V, int comm) {
  Net n;
  n.F = F, n.H = H, n.K = K, n.V = V, n.comm = comm;
  n.M = comm ? H + V : H, n.Q = 2 * K + V;
  n.nbF = blocks16(F), n.nbH = blocks16(H), n.nbV = blocks16(V), n.nbM = blocks16(n.M), n.nb2 = 2 + n.nbV;
  n.Hp = 16 * n.nbH;
  n.ldF = ld_for(4 * ((F + 3) / 4)), n.ldH = ld_for(n.Hp), n.ldM = ld_for(16 * n.nbM);
  int o = 0;
  n.oE0w = o, o += H * F, n.oE0b = o, o += H, n.oE2w = o, o += H * H, n.oE2b = o, o += H;
  n.oH0w = o, o += H * n.M, n.oH0b = o, o += H, n.oH2w = o, o += 2 * H, n.oH2b = o, o += 2;
  const int order[3] = {1, 2, 0};      // parameters(): hidden2key, hidden2value, hidden2query
  for (int i = 0; i < 3; ++i) {
    const int s = order[i], out = s == 2 ? V : K;
    n.oP0w[s] = n.oP0b[s] = n.oP2w[s] = n.oP2b[s] = 0;
    if (!comm) continue;
    n.oP0w[s] = o, o += H * H, n.oP0b[s] = o, o += H, n.oP2w[s] = o, o += out * H, n.oP2b[s] = o, o += out;
  }
  n.G = o;
  n.stride = (n.G + 1 + 3) & ~3;
  return n;
}

// LDS floats of the three kernels
__host__ __device__ inline int lds_o2h(const Net& n) { return n.Hp * n.ldF + n.Hp * n.ldH + 2 * n.Hp + SUB * (16 * n.nbF + 3 * n.Hp) * LT; }
__host__ __device__ inline int lds_proj(const Net& n) {
  return 3 * n.Hp * n.ldH + 16 * n.nb2 * n.ldH + 3 * n.Hp + 16 * n.nb2 + SUB * (7 * n.Hp + 16 * n.nb2) * LT;
}
__host__ __device__ inline int lds_head(const Net& n) {
  return n.Hp * n.ldM + 3 * n.Hp + 4 + SUB * ((16 * n.nbM + 2 * n.Hp) * LT + 2 * WPS * TILE * 2);
}

struct Args {
  Net n;
  const float *e_w0, *e_b0, *e_w2, *e_b2, *h_w0, *h_b0, *h_w2, *h_b2;
  const float *p_w0[3], *p_b0[3], *p_w2[3], *p_b2[3];      // 0 query, 1 key, 2 value
  const float* state;
  int64_t ld_state;
  const int64_t* index;
  int N;                       // agents per env-step
  int64_t A, npairs;           // agents; pairs of tiles
  const int64_t* action;
  const float* old_prob;
  const float* adv;            // [A], minibatch order
  float clip_lo, clip_hi;
  float *cat, *dcat;           // [A][M]
  float *qkv, *dqkv;           // [A][Q]
  float* part;                 // [SUB * gridDim.x][stride]
  float* ratio;                // [A], minibatch order (may be null)
};

__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// dst [rows_p][ld] <- src [rows][cols] (torch layout), zeros in the padding
__device__ __forceinline__ void stage_matrix(float* dst, const float* src, int rows, int cols, int rows_p, int ld, int tid) {
  for (int i = tid; i < rows_p * ld; i += NT) {
    const int r = i / ld, c = i - r * ld;
    dst[i] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0.0f;
  }
}
__device__ __forceinline__ void stage_vector(float* dst, const float* src, int n, int n_p, int tid) {
  for (int i = tid; i < n_p; i += NT) dst[i] = i < n ? src[i] : 0.0f;
}

// the buffer row agent `ag` of the minibatch reads its state, action and old_prob from
__device__ __forceinline__ int64_t source_row(const Args& a, int64_t ag) {
  const uint32_t i = (uint32_t)ag / (uint32_t)a.N, h = (uint32_t)ag - i * (uint32_t)a.N;
  const int64_t j = a.index ? a.index[i] : (int64_t)i;
  return j * a.N + h;
}

// dstT [width_p][LT] <- the tile's 16 rows of `width` floats (transposed), zeros past `width` and past the batch
template <bool GATHER>
__device__ __forceinline__ void load_tile(float* dstT, int width_p, int width, const float* src, int64_t ld, const Args& a, int64_t tile, int stid) {
  for (int e = stid; e < TILE * width_p; e += ST) {
    const int r = e / width_p, f = e - r * width_p;
    const int64_t ag = tile * TILE + r;
    float x = 0.0f;
    if (f < width && ag < a.A) x = src[(GATHER ? source_row(a, ag) : ag) * ld + f];
    dstT[f * LT + r] = x;
  }
}

// acc += sum over ks k-steps of A(k-step q at pa + q sa) x B(pb + q sb); two chains (even / odd k-steps) against the 40 cycles of
// dependent latency
__device__ __forceinline__ f32x4 mm(const float* pa, int sa, const float* pb, int sb, int ks, f32x4 acc) {
  f32x4 odd = {0, 0, 0, 0};
  int q = 0;
  for (; q + 1 < ks; q += 2) {
    acc = MFMA(pa[q * sa], pb[q * sb], acc);
    odd = MFMA(pa[(q + 1) * sa], pb[(q + 1) * sb], odd);
  }
  if (q < ks) acc = MFMA(pa[q * sa], pb[q * sb], acc);
  return acc + odd;
}

// z block ob = bias + W[16 ob ..][:] in  (W [..][ld] row-major, inT [unit][agent]); lane (c, g) gets units 16 ob + 4 g + i of agent c
__device__ __forceinline__ f32x4 layer_fwd(const float* W, int ld, const float* bias, int ob, const float* inT, int ks, int c, int g) {
  const f32x4 z = *reinterpret_cast<const f32x4*>(bias + 16 * ob + 4 * g);
  return mm(W + (16 * ob + c) * ld + g, 4, inT + g * LT + c, 4 * LT, ks, z);
}
// d in block ib = W^T d out  (W read transposed; ks = output units / 4)
__device__ __forceinline__ f32x4 layer_bwd(const float* W, int ld, int ib, const float* doutT, int ks, int c, int g, f32x4 acc) {
  return mm(W + g * ld + 16 * ib + c, 4 * ld, doutT + g * LT + c, 4 * LT, ks, acc);
}
// dW[16 ob + m][16 ib + n] += sum over the tile's agents of d out[agent][16 ob + m] in[agent][16 ib + n]; db likewise against ones.
// doutT_ob = doutT + 16 ob LT
template <int NB>
__device__ __forceinline__ void wgrad(f32x4 (&dW)[NB], f32x4& db, const float* doutT_ob, const float* inT, int nb_in, int c, int g) {
  const float* da = doutT_ob + c * LT + g;
  const float* hb = inT + c * LT + g;
#pragma unroll
  for (int q = 0; q < TILE / 4; ++q) {
    const float av = da[4 * q];
    db = MFMA(av, 1.0f, db);
#pragma unroll
    for (int ib = 0; ib < NB; ++ib)
      if (ib < nb_in) dW[ib] = MFMA(av, hb[16 * ib * LT + 4 * q], dW[ib]);
  }
}
__device__ __forceinline__ void store_T(float* outT, int ob, const f32x4& x, int c, int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) outT[(16 * ob + 4 * g + i) * LT + c] = x[i];
}
// the accumulators of output block ob (rows `row0 + 4 g + i` of a [rows][cols] matrix) into the partial
template <int NB>
__device__ __forceinline__ void store_wgrad(float* pw, float* pb, int rows, int cols, int row0, const f32x4 (&dW)[NB], const f32x4& db, int nb_in,
                                            int c, int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = row0 + 4 * g + i;
    if (u < rows) {
#pragma unroll
      for (int ib = 0; ib < NB; ++ib)
        if (ib < nb_in && 16 * ib + c < cols) pw[u * cols + 16 * ib + c] = dW[ib][i];
      if (c == 0) pb[u] = db[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- obs2hidden
template <bool BWD>
__global__ __launch_bounds__(NT) void k_tppo_o2h(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Net& n = a.n;
  const int tid = threadIdx.x, sub = tid / ST, stid = tid - sub * ST, v = stid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nbH = n.nbH, nbF = n.nbF, Hp = n.Hp;
  float* W0s = lds;
  float* W2s = W0s + Hp * n.ldF;
  float* b0s = W2s + Hp * n.ldH;
  float* b2s = b0s + Hp;
  float* obsT = b2s + Hp + sub * (16 * nbF + 3 * Hp) * LT;
  float* t1T = obsT + 16 * nbF * LT;
  float* dxT = t1T + Hp * LT;
  float* dz1T = dxT + Hp * LT;
  stage_matrix(W0s, a.e_w0, n.H, n.F, Hp, n.ldF, tid);
  stage_matrix(W2s, a.e_w2, n.H, n.H, Hp, n.ldH, tid);
  stage_vector(b0s, a.e_b0, n.H, Hp, tid);
  stage_vector(b2s, a.e_b2, n.H, Hp, tid);

  f32x4 dW0[MAX_F / 16], dW2[MAX_H / 16], db0 = {0, 0, 0, 0}, db2 = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < MAX_F / 16; ++i) dW0[i] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < MAX_H / 16; ++i) dW2[i] = f32x4{0, 0, 0, 0};

  for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
    const int64_t tile = p * SUB + sub;
    load_tile<true>(obsT, 16 * nbF, n.F, a.state, a.ld_state, a, tile, stid);
    if (BWD) load_tile<false>(dxT, Hp, n.H, a.dcat, n.M, a, tile, stid);
    __syncthreads();
    f32x4 z1 = {0, 0, 0, 0};
    if (v < nbH) {
      z1 = layer_fwd(W0s, n.ldF, b0s, v, obsT, (n.F + 3) >> 2, c, g);
      f32x4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = fmaxf(z1[i], 0.0f);
      store_T(t1T, v, h, c, g);
    }
    __syncthreads();
    if (v < nbH) {
      if (!BWD) {
        const f32x4 x = layer_fwd(W2s, n.ldH, b2s, v, t1T, 4 * nbH, c, g);
        const int64_t ag = tile * TILE + c;
        if (ag < a.A && 16 * v + 4 * g < n.H) *reinterpret_cast<f32x4*>(a.cat + ag * n.M + 16 * v + 4 * g) = x;
      } else {
        wgrad(dW2, db2, dxT + 16 * v * LT, t1T, nbH, c, g);
        const f32x4 dh = layer_bwd(W2s, n.ldH, v, dxT, 4 * nbH, c, g, f32x4{0, 0, 0, 0});
        f32x4 dz;
#pragma unroll
        for (int i = 0; i < 4; ++i) dz[i] = z1[i] > 0.0f ? dh[i] : 0.0f;
        store_T(dz1T, v, dz, c, g);
        wave_lds_fence();
        wgrad(dW0, db0, dz1T + 16 * v * LT, obsT, nbF, c, g);
      }
    }
    if (BWD) __syncthreads();      // the next tile's load overwrites obsT and dxT
  }
  if (BWD && v < nbH) {
    float* part = a.part + ((int64_t)blockIdx.x * SUB + sub) * n.stride;
    store_wgrad(part + n.oE0w, part + n.oE0b, n.H, n.F, 16 * v, dW0, db0, nbF, c, g);
    store_wgrad(part + n.oE2w, part + n.oE2b, n.H, n.H, 16 * v, dW2, db2, nbH, c, g);
  }
}

// ---------------------------------------------------------------------------------------------------------------- projections
// Segments 0 query, 1 key, 2 value.  First layers W0s[seg] [Hp][ldH]; the last layers side by side in W2s [16 nb2][ldH]: block 0
// hidden2query.2 (K rows), block 1 hidden2key.2, blocks 2.. hidden2value.2 - block b reads the tanh units of segment min(b, 2).
template <bool BWD>
__global__ __launch_bounds__(NT) void k_tppo_proj(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Net& n = a.n;
  const int tid = threadIdx.x, sub = tid / ST, stid = tid - sub * ST, v = stid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nbH = n.nbH, nb2 = n.nb2, Hp = n.Hp, ldH = n.ldH;
  float* W0s = lds;
  float* W2s = W0s + 3 * Hp * ldH;
  float* b0s = W2s + 16 * nb2 * ldH;
  float* b2s = b0s + 3 * Hp;
  float* xT = b2s + 16 * nb2 + sub * (7 * Hp + 16 * nb2) * LT;
  float* tT = xT + Hp * LT;              // [3][Hp]
  float* dtT = tT + 3 * Hp * LT;         // [3][Hp]
  float* dqT = dtT + 3 * Hp * LT;        // [16 nb2]: dq | dk | dv, each padded to whole blocks
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int out = s == 2 ? n.V : n.K, rows_p = s == 2 ? 16 * n.nbV : 16;
    stage_matrix(W0s + s * Hp * ldH, a.p_w0[s], n.H, n.H, Hp, ldH, tid);
    stage_vector(b0s + s * Hp, a.p_b0[s], n.H, Hp, tid);
    stage_matrix(W2s + 16 * s * ldH, a.p_w2[s], out, n.H, rows_p, ldH, tid);
    stage_vector(b2s + 16 * s, a.p_b2[s], out, rows_p, tid);
  }
  const int seg2 = v < 2 ? v : 2;                                 // the segment of last-layer block v
  const int out2 = seg2 == 2 ? n.V : n.K;
  const int col2 = v == 0 ? 0 : v == 1 ? n.K : 2 * n.K + 16 * (v - 2);      // the block's first column of q | k | v

  f32x4 dP0[3][MAX_H / 16], dP2[MAX_H / 16], dbP0[3], dbP2 = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    dbP0[s] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < MAX_H / 16; ++i) dP0[s][i] = f32x4{0, 0, 0, 0};
  }
#pragma unroll
  for (int i = 0; i < MAX_H / 16; ++i) dP2[i] = f32x4{0, 0, 0, 0};

  for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
    const int64_t tile = p * SUB + sub;
    const int64_t ag = tile * TILE + c;
    load_tile<false>(xT, Hp, n.H, a.cat, n.M, a, tile, stid);
    if (BWD) {
      load_tile<false>(dqT, 16, n.K, a.dqkv, n.Q, a, tile, stid);
      load_tile<false>(dqT + 16 * LT, 16, n.K, a.dqkv + n.K, n.Q, a, tile, stid);
      load_tile<false>(dqT + 32 * LT, 16 * n.nbV, n.V, a.dqkv + 2 * n.K, n.Q, a, tile, stid);
    }
    __syncthreads();
    f32x4 t[3];
    if (v < nbH) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const f32x4 z = layer_fwd(W0s + s * Hp * ldH, ldH, b0s + s * Hp, v, xT, 4 * nbH, c, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) t[s][i] = tanhf(z[i]);
        store_T(tT + s * Hp * LT, v, t[s], c, g);
      }
    }
    __syncthreads();
    if (!BWD) {
      if (v < nb2) {
        const f32x4 y = layer_fwd(W2s, ldH, b2s, v, tT + seg2 * Hp * LT, 4 * nbH, c, g);
        const int u = (v < 2 ? 0 : 16 * (v - 2)) + 4 * g;
        if (ag < a.A && u < out2) *reinterpret_cast<f32x4*>(a.qkv + ag * n.Q + col2 + 4 * g) = y;
      }
      continue;      // the next tile's images are written behind its first barrier, the tanh units behind this one
    }
    if (v < nb2) wgrad(dP2, dbP2, dqT + 16 * v * LT, tT + seg2 * Hp * LT, nbH, c, g);
    if (v < nbH) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int ks = (s == 2 ? n.V : n.K) >> 2;
        const f32x4 d = layer_bwd(W2s + 16 * s * ldH, ldH, v, dqT + 16 * s * LT, ks, c, g, f32x4{0, 0, 0, 0});
        f32x4 dt;
#pragma unroll
        for (int i = 0; i < 4; ++i) dt[i] = d[i] * (1.0f - t[s][i] * t[s][i]);
        store_T(dtT + s * Hp * LT, v, dt, c, g);
      }
    }
    __syncthreads();
    if (v < nbH) {
      f32x4 dx = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        wgrad(dP0[s], dbP0[s], dtT + (s * Hp + 16 * v) * LT, xT, nbH, c, g);
        dx = layer_bwd(W0s + s * Hp * ldH, ldH, v, dtT + s * Hp * LT, 4 * nbH, c, g, dx);
      }
      if (ag < a.A && 16 * v + 4 * g < n.H) {
        f32x4* px = reinterpret_cast<f32x4*>(a.dcat + ag * n.M + 16 * v + 4 * g);
        *px = *px + dx;      // the head's dx plus the three projections'
      }
    }
    __syncthreads();      // the next tile's load overwrites xT and dqT
  }
  if (BWD) {
    float* part = a.part + ((int64_t)blockIdx.x * SUB + sub) * n.stride;
    if (v < nbH) {
#pragma unroll
      for (int s = 0; s < 3; ++s) store_wgrad(part + n.oP0w[s], part + n.oP0b[s], n.H, n.H, 16 * v, dP0[s], dbP0[s], nbH, c, g);
    }
    if (v < nb2) {
      const int ow = v == 0 ? n.oP2w[0] : v == 1 ? n.oP2w[1] : n.oP2w[2], ob = v == 0 ? n.oP2b[0] : v == 1 ? n.oP2b[1] : n.oP2b[2];
      store_wgrad(part + ow, part + ob, out2, n.H, v < 2 ? 0 : 16 * (v - 2), dP2, dbP2, nbH, c, g);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------- head
__global__ __launch_bounds__(NT) void k_tppo_head(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Net& n = a.n;
  const int tid = threadIdx.x, sub = tid / ST, stid = tid - sub * ST, v = stid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nbH = n.nbH, nbM = n.nbM, Hp = n.Hp, ldM = n.ldM;
  float* W0s = lds;
  float* b0s = W0s + Hp * ldM;
  float* W3s = b0s + Hp;      // [2][Hp]
  float* b3s = W3s + 2 * Hp;
  float* inT = b3s + 4 + sub * ((16 * nbM + 2 * Hp) * LT + 2 * WPS * TILE * 2);
  float* hT = inT + 16 * nbM * LT;
  float* dzT = hT + Hp * LT;
  float* lp = dzT + Hp * LT;                          // [wave][agent][2]: the logits' partial sums over the wave's block of h
  float* dl = lp + WPS * TILE * 2 + v * TILE * 2;      // the wave's own copy of the tile's dlogits [agent][2]
  stage_matrix(W0s, a.h_w0, n.H, n.M, Hp, ldM, tid);
  stage_vector(b0s, a.h_b0, n.H, Hp, tid);
  for (int i = tid; i < 2 * Hp; i += NT) {
    const int o = i / Hp, u = i - o * Hp;
    W3s[i] = u < n.H ? a.h_w2[o * n.H + u] : 0.0f;
  }
  if (tid < 4) b3s[tid] = tid < 2 ? a.h_b2[tid] : 0.0f;

  f32x4 dW0[(MAX_H + MAX_V) / 16], db0 = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < (MAX_H + MAX_V) / 16; ++i) dW0[i] = f32x4{0, 0, 0, 0};
  float acc3 = 0.0f;      // lane (g < 2, c): dW3[g][16 v + c];  lane (g == 2, c < 2): db3[c]
  float loss = 0.0f;      // wave 0 of the tile, lanes g == 0: the terms of the agents = c (mod 16)

  for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
    const int64_t tile = p * SUB + sub;
    const int64_t ag = tile * TILE + c;
    const bool valid = ag < a.A;
    load_tile<false>(inT, 16 * nbM, n.M, a.cat, n.M, a, tile, stid);
    __syncthreads();
    f32x4 z = {0, 0, 0, 0};
    if (v < nbH) {
      z = layer_fwd(W0s, ldM, b0s, v, inT, n.M >> 2, c, g);
      // the block's share of the two logits from the lane's own registers
      const f32x4 w30 = *reinterpret_cast<const f32x4*>(W3s + 16 * v + 4 * g);
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + Hp + 16 * v + 4 * g);
      float p0 = 0.0f, p1 = 0.0f;
      f32x4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        h[i] = fmaxf(z[i], 0.0f);
        p0 = fmaf(w30[i], h[i], p0);
        p1 = fmaf(w31[i], h[i], p1);
      }
      store_T(hT, v, h, c, g);
      p0 += __shfl_xor(p0, 16);
      p0 += __shfl_xor(p0, 32);
      p1 += __shfl_xor(p1, 16);
      p1 += __shfl_xor(p1, 32);
      if (g == 0) {
        lp[(v * TILE + c) * 2] = p0;
        lp[(v * TILE + c) * 2 + 1] = p1;
      }
    }
    __syncthreads();
    // the logits of agent c, every wave for itself (the same bits in all of them): the blocks' shares in block order
    float l0 = 0.0f, l1 = 0.0f;
#pragma unroll
    for (int b = 0; b < WPS; ++b)
      if (b < nbH) {
        l0 += lp[(b * TILE + c) * 2];
        l1 += lp[(b * TILE + c) * 2 + 1];
      }
    l0 += b3s[0];
    l1 += b3s[1];
    float d0 = 0.0f, d1 = 0.0f, term = 0.0f;      // dlogits (before the 1 / A of the reduction) and the agent's loss term
    if (valid) {
      // agents/tarmac_ppo.py:168-182: ratio = pi(a) / old_prob, L = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A); torch passes
      // the gradient through min to the first argument unless the second is smaller, and through clamp inside the closed range
      const int64_t j = source_row(a, ag);
      const bool act = a.action[j] != 0;
      const float d = act ? l1 - l0 : l0 - l1;
      const float pa = 1.0f / (1.0f + expf(-d)), pb = 1.0f / (1.0f + expf(d));
      const float ratio = pa / a.old_prob[j];
      const float adv = a.adv[ag];
      const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi) * adv;
      term = -fminf(s1, s2);
      const bool active = (ratio >= a.clip_lo && ratio <= a.clip_hi) || s1 < s2;
      const float da = active ? (-adv * ratio) * pb : 0.0f;      // d term / d logit[a]; the other logit takes the negative
      d0 = act ? -da : da;
      d1 = act ? da : -da;
      if (v == 0 && g == 0 && a.ratio) a.ratio[ag] = ratio;
    }
    if (v == 0 && g == 0) loss += term;
    if (g == 0) {
      dl[2 * c] = d0;
      dl[2 * c + 1] = d1;
    }
    if (v < nbH) {
      const f32x4 w30 = *reinterpret_cast<const f32x4*>(W3s + 16 * v + 4 * g);
      const f32x4 w31 = *reinterpret_cast<const f32x4*>(W3s + Hp + 16 * v + 4 * g);
      f32x4 dz;
#pragma unroll
      for (int i = 0; i < 4; ++i) dz[i] = z[i] > 0.0f ? fmaf(d0, w30[i], d1 * w31[i]) : 0.0f;
      store_T(dzT, v, dz, c, g);
    }
    wave_lds_fence();
    if (v < nbH) {
      wgrad(dW0, db0, dzT + 16 * v * LT, inT, nbM, c, g);
      // the last layer's gradient, columns of block v: a chain over the tile's agents
      if (g < 2) {
        const float* hr = hT + (16 * v + c) * LT;
#pragma unroll
        for (int r = 0; r < TILE; ++r) acc3 = fmaf(dl[2 * r + g], hr[r], acc3);
      } else if (g == 2 && c < 2) {
#pragma unroll
        for (int r = 0; r < TILE; ++r) acc3 += dl[2 * r + c];
      }
    }
    __syncthreads();
    // d[x | comm]: input block ib by wave ib mod 4
    for (int ib = v; ib < nbM; ib += WPS) {
      const f32x4 din = layer_bwd(W0s, ldM, ib, dzT, 4 * nbH, c, g, f32x4{0, 0, 0, 0});
      if (valid && 16 * ib + 4 * g < n.M) *reinterpret_cast<f32x4*>(a.dcat + ag * n.M + 16 * ib + 4 * g) = din;
    }
    // no barrier here: the next tile's load writes inT, last read before the barrier above; dzT and lp are rewritten behind two more
  }

  float* part = a.part + ((int64_t)blockIdx.x * SUB + sub) * n.stride;
  if (v < nbH) {
    store_wgrad(part + n.oH0w, part + n.oH0b, n.H, n.M, 16 * v, dW0, db0, nbM, c, g);
    if (g < 2 && 16 * v + c < n.H) part[n.oH2w + g * n.H + 16 * v + c] = acc3;
  }
  if (v == 0) {
    if (g == 2 && c < 2) part[n.oH2b + c] = acc3;
    // the loss: the 16 lanes' sums in lane order
    wave_lds_fence();
    if (g == 0) dl[c] = loss;
    wave_lds_fence();
    if (lane == 0) {
      float sum = 0.0f;
      for (int i = 0; i < TILE; ++i) sum += dl[i];
      part[n.G] = sum;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------- host
bool net_fields_ok(const mdr_tarmac_net_t* n) {
  return n && n->struct_size == sizeof(mdr_tarmac_net_t) && n->num_state > 0 && n->hidden > 0 && (n->with_comm == 0 || n->with_comm == 1) &&
         (!n->with_comm || (n->num_key > 0 && n->num_value > 0));
}
bool net_covered(const mdr_tarmac_net_t* n) {
  if (n->num_state > MAX_F || n->hidden % 4 || n->hidden > MAX_H || n->num_hops != 1) return false;
  if (!n->with_comm) return true;
  if (n->mode != MDR_TARMAC_NEIGHBOURS && n->mode != MDR_TARMAC_NONE) return false;
  return n->num_key % 4 == 0 && n->num_key <= MAX_K && n->num_value % 4 == 0 && n->num_value <= MAX_V;
}
Net net_of(const mdr_tarmac_net_t* n) {
  return make_net(n->num_state, n->hidden, n->with_comm ? n->num_key : 4, n->with_comm ? n->num_value : 4, n->with_comm);
}

int64_t grid_for(int64_t agents, int32_t max_workgroups, int cus) {
  const int64_t ntiles = (agents + TILE - 1) / TILE, npairs = (ntiles + SUB - 1) / SUB;
  const int64_t cap = max_workgroups > 0 ? max_workgroups : (cus < LIB_MAX_WG ? cus : LIB_MAX_WG);
  const int64_t grid = npairs < cap ? npairs : cap;
  return grid > 0 ? grid : 1;
}

int64_t align16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }

struct Layout {
  int64_t part, cat, dcat, qkv, dqkv, stats, total;      // byte offsets
};
Layout layout_of(const Net& n, int64_t agents, int64_t grid) {
  Layout l;
  int64_t o = 0;
  l.part = o, o += align16(SUB * grid * n.stride * (int64_t)sizeof(float));
  l.cat = o, o += align16(agents * n.M * (int64_t)sizeof(float));
  l.dcat = o, o += align16(agents * n.M * (int64_t)sizeof(float));
  l.qkv = l.dqkv = l.stats = o;
  if (n.comm) {
    l.qkv = o, o += align16(agents * n.Q * (int64_t)sizeof(float));
    l.dqkv = o, o += align16(agents * n.Q * (int64_t)sizeof(float));
    l.stats = o, o += align16(mdr_tarmac_comm_backward_workspace_bytes(agents, n.K, n.V));
  }
  l.total = o;
  return l;
}

template <typename K>
int prepare(K kernel, int lds_floats) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             lds_floats * (int)sizeof(float)) == hipSuccess
             ? MDR_OK
             : MDR_ERR_HIP;
}

// the by-value entry point (key_dev and step_dev NULL: the defects' key is `seed`) and the keyed one
int actor_grad(const mdr_tarmac_net_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows, int32_t nb_houses,
               const int64_t* action, const float* old_prob, const float* advantage, float clip_param, const int32_t* key_dev, uint64_t seed,
               uint64_t step, const int32_t* step_dev, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* ratio,
               void* stream) {
  if (!net_fields_ok(net) || !state || !action || !old_prob || !advantage || !grad || !loss) return MDR_ERR_INVALID;
  if (!workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  if (!net->encode_w0 || !net->encode_b0 || !net->encode_w2 || !net->encode_b2 || !net->head_w0 || !net->head_b0 || !net->head_w2 || !net->head_b2)
    return MDR_ERR_INVALID;
  if (net->with_comm && (!net->key_w0 || !net->key_b0 || !net->key_w2 || !net->key_b2 || !net->value_w0 || !net->value_b0 || !net->value_w2 ||
                         !net->value_b2 || !net->query_w0 || !net->query_b0 || !net->query_w2 || !net->query_b2))
    return MDR_ERR_INVALID;
  if (nb_rows < 0 || nb_houses <= 0 || ld_state < net->num_state || max_workgroups < 0 || !(clip_param >= 0.0f && clip_param < 1.0f))
    return MDR_ERR_INVALID;
  if (net->with_comm && (net->nb_comm < 0 || !(net->defect_prob >= 0.0f && net->defect_prob <= 1.0f))) return MDR_ERR_INVALID;
  if (!net_covered(net)) return MDR_ERR_UNSUPPORTED;
  if (nb_rows > MAX_AGENTS / nb_houses) return MDR_ERR_UNSUPPORTED;
  const int cc = net->nb_comm < nb_houses - 1 ? net->nb_comm : nb_houses - 1;
  if (net->with_comm && net->mode == MDR_TARMAC_NEIGHBOURS && cc > MAX_C) return MDR_ERR_UNSUPPORTED;
  Args a{};
  a.n = net_of(net);
  const Net& n = a.n;
  const int l_o2h = lds_o2h(n), l_proj = lds_proj(n), l_head = lds_head(n);
  if ((size_t)l_o2h * sizeof(float) > LDS_LIMIT || (size_t)l_proj * sizeof(float) > LDS_LIMIT || (size_t)l_head * sizeof(float) > LDS_LIMIT)
    return MDR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t agents = nb_rows * nb_houses;
  int grid = 0;
  if (nb_rows > 0) {
    int dev = 0, cus = 256;
    if (max_workgroups == 0 &&
        (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess))
      cus = 256;
    grid = (int)grid_for(agents, max_workgroups, cus);
    const Layout l = layout_of(n, agents, grid);
    char* ws = static_cast<char*>(workspace);
    a.e_w0 = net->encode_w0, a.e_b0 = net->encode_b0, a.e_w2 = net->encode_w2, a.e_b2 = net->encode_b2;
    a.h_w0 = net->head_w0, a.h_b0 = net->head_b0, a.h_w2 = net->head_w2, a.h_b2 = net->head_b2;
    a.p_w0[0] = net->query_w0, a.p_b0[0] = net->query_b0, a.p_w2[0] = net->query_w2, a.p_b2[0] = net->query_b2;
    a.p_w0[1] = net->key_w0, a.p_b0[1] = net->key_b0, a.p_w2[1] = net->key_w2, a.p_b2[1] = net->key_b2;
    a.p_w0[2] = net->value_w0, a.p_b0[2] = net->value_b0, a.p_w2[2] = net->value_w2, a.p_b2[2] = net->value_b2;
    a.state = state, a.ld_state = ld_state, a.index = index, a.N = nb_houses, a.A = agents;
    a.npairs = ((agents + TILE - 1) / TILE + SUB - 1) / SUB;
    a.action = action, a.old_prob = old_prob, a.adv = advantage;
    a.clip_lo = (float)(1.0 - (double)clip_param), a.clip_hi = (float)(1.0 + (double)clip_param);
    a.part = reinterpret_cast<float*>(ws + l.part);
    a.cat = reinterpret_cast<float*>(ws + l.cat), a.dcat = reinterpret_cast<float*>(ws + l.dcat);
    a.qkv = reinterpret_cast<float*>(ws + l.qkv), a.dqkv = reinterpret_cast<float*>(ws + l.dqkv);
    a.ratio = ratio;
    // nothing is launched unless every kernel of the chain can be
    if (prepare(k_tppo_o2h<false>, l_o2h) != MDR_OK || prepare(k_tppo_o2h<true>, l_o2h) != MDR_OK || prepare(k_tppo_head, l_head) != MDR_OK ||
        (n.comm && (prepare(k_tppo_proj<false>, l_proj) != MDR_OK || prepare(k_tppo_proj<true>, l_proj) != MDR_OK)))
      return MDR_ERR_HIP;
    const dim3 g3((unsigned)grid), b3(NT);
    const size_t b_o2h = (size_t)l_o2h * sizeof(float), b_proj = (size_t)l_proj * sizeof(float), b_head = (size_t)l_head * sizeof(float);
    hipLaunchKernelGGL(k_tppo_o2h<false>, g3, b3, b_o2h, st, a);
    if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
    float *q = a.qkv, *k = a.qkv + n.K, *v = a.qkv + 2 * n.K, *comm = a.cat + n.H;
    if (n.comm) {
      hipLaunchKernelGGL(k_tppo_proj<false>, g3, b3, b_proj, st, a);
      if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
      const int rc = key_dev ? mdr_tarmac_comm_keyed(q, n.Q, k, n.Q, v, n.Q, (int32_t)nb_rows, nb_houses, n.K, n.V, net->nb_comm, net->mode,
                                                     net->defect_prob, key_dev, step, step_dev, 0, comm, n.M, stream)
                             : mdr_tarmac_comm(q, n.Q, k, n.Q, v, n.Q, (int32_t)nb_rows, nb_houses, n.K, n.V, net->nb_comm, net->mode,
                                               net->defect_prob, seed, step, step_dev, 0, comm, n.M, stream);
      if (rc != MDR_OK) return MDR_ERR_HIP;
    }
    hipLaunchKernelGGL(k_tppo_head, g3, b3, b_head, st, a);
    if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
    if (n.comm) {
      float *dq = a.dqkv, *dk = a.dqkv + n.K, *dv = a.dqkv + 2 * n.K, *dcomm = a.dcat + n.H;
      const int rc =
          key_dev ? mdr_tarmac_comm_backward_keyed(q, n.Q, k, n.Q, v, n.Q, (int32_t)nb_rows, nb_houses, n.K, n.V, net->nb_comm, net->mode,
                                                   net->defect_prob, key_dev, step, step_dev, 0, comm, n.M, dcomm, n.M, dq, n.Q, dk, n.Q, dv, n.Q,
                                                   ws + l.stats, stream)
                  : mdr_tarmac_comm_backward(q, n.Q, k, n.Q, v, n.Q, (int32_t)nb_rows, nb_houses, n.K, n.V, net->nb_comm, net->mode,
                                             net->defect_prob, seed, step, step_dev, 0, comm, n.M, dcomm, n.M, dq, n.Q, dk, n.Q, dv, n.Q,
                                             ws + l.stats, stream);
      if (rc != MDR_OK) return MDR_ERR_HIP;
      hipLaunchKernelGGL(k_tppo_proj<true>, g3, b3, b_proj, st, a);
      if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
    }
    hipLaunchKernelGGL(k_tppo_o2h<true>, g3, b3, b_o2h, st, a);
    if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
  }
  const int cnt = n.G + 1;
  hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(workspace), SUB * grid,
                     n.stride, n.G, (float)agents, grad, loss);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int64_t mdr_tarmac_net_grad_floats(const mdr_tarmac_net_t* net) {
  if (!net_fields_ok(net) || !net_covered(net)) return -1;
  return net_of(net).G;
}

int64_t mdr_tarmac_ppo_workspace_bytes(const mdr_tarmac_net_t* net, int64_t nb_rows, int32_t nb_houses, int32_t max_workgroups) {
  if (!net_fields_ok(net) || !net_covered(net) || nb_rows < 0 || nb_houses <= 0 || max_workgroups < 0) return -1;
  if (nb_rows > MAX_AGENTS / nb_houses) return -1;
  const Net n = net_of(net);
  const int64_t agents = nb_rows * nb_houses;
  // max_workgroups == 0: room for the library's grid on any device (no device call here)
  return layout_of(n, agents, grid_for(agents, max_workgroups, LIB_MAX_WG)).total;
}

int mdr_tarmac_ppo_actor_grad(const mdr_tarmac_net_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                              int32_t nb_houses, const int64_t* action, const float* old_prob, const float* advantage, float clip_param,
                              uint64_t seed, uint64_t step, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* ratio,
                              void* stream) {
  return actor_grad(net, state, ld_state, index, nb_rows, nb_houses, action, old_prob, advantage, clip_param, nullptr, seed, step, nullptr,
                    max_workgroups, workspace, grad, loss, ratio, stream);
}

int mdr_tarmac_ppo_actor_grad_keyed(const mdr_tarmac_net_t* net, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                                    int32_t nb_houses, const int64_t* action, const float* old_prob, const float* advantage, float clip_param,
                                    const int32_t* key_dev, uint64_t step, const int32_t* step_dev, int32_t max_workgroups, void* workspace,
                                    float* grad, float* loss, float* ratio, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return actor_grad(net, state, ld_state, index, nb_rows, nb_houses, action, old_prob, advantage, clip_param, key_dev, 0, step, step_dev,
                    max_workgroups, workspace, grad, loss, ratio, stream);
}

}  // extern "C"
