// TarMAC-PPO actor, the two non-banded masks of make_masks (agents/network.py:138-177): tarmac_comm_mode "all" and "random_sample"
// (include/mdr_policy.h, mdr_tarmac_gather / mdr_tarmac_gather_backward).  The attention itself is mdr_tarmac.hip's - score =
// query . key / sqrt(K), softmax over the receiver's senders with the maximum over those senders, out = sum attn value - only the
// sender set S(r) differs: every agent of the env ("all"), or the receiver and c distinct others drawn per (seed, step, hop, agent)
// with Floyd's algorithm on Philox words ("random_sample").
//
//   k_tarmac_gather            one workgroup = floor(256 / N) whole envs (N <= 256) or 256 consecutive receivers of one env, whose N
//                              key | value rows are ALL staged in LDS (any agent may be a sender), 16-byte accesses, row stride an odd
//                              multiple of 4 floats.  One lane per receiver.  "all": the lanes of an env walk the rows 0 .. N - 1
//                              together (an LDS broadcast).  "random_sample": the lane first builds its c <= 64 house indices in
//                              LDS (uint16, [slot][lane], read back by the same lane only), then gathers.  Two passes over the senders
//                              as k_tarmac_comm: the maximum, then exp(score - max), the sum and the weighted values.
//   k_tarmac_gather_grad_recv  receiver-major pass of the backward (N <= 256: whole envs only): the forward's staging, delta, the
//                              statistics (max, 1 / sum, delta, 0) and grad_query; "random_sample" also leaves the receiver's
//                              index list in the workspace.
//   k_tarmac_gather_grad_send  sender-major pass: stages query | grad_out | statistics rows (and the index lists) of its envs, one
//                              lane per sender walks the receivers of its env in ascending order, keeps those that hear it (all;
//                              or itself and the lists that name it), recomputes p_rs from the statistics and accumulates grad_key
//                              and grad_value.  A fixed order and no floating-point atomics: the same operands give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_device.h"
#include "mdr_draw.h"

namespace {

using mdr::loop_local;
using mdr::philox4x32_10;
using mdr::u32x4;

constexpr uint32_t TAG_GATHER = 0x544D4732u;
constexpr int TILE = 256;
constexpr int MAX_C = 64;
constexpr size_t MAX_LDS = 160 * 1024;

struct GatherArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* out;      // backward: the forward's result
  const float* g;
  float* dst;            // forward: out
  float* dq;
  float* dk;
  float* dv;
  float4* stats;         // backward workspace: per receiver max score, 1 / sum, delta, 0
  uint16_t* ws_idx;      // ... and, random_sample, [agent][c] house indices
  int64_t ldq, ldk, ldv, ldo, ldg, lddq, lddk, lddv;
  int E, N;
  int kq, vq;            // float4 per key / value row
  int c;                 // drawn senders besides the receiver itself
  int epw;               // whole envs per workgroup (N <= 256), 0: slices of an env
  int slices;            // ceil(N / 256) when epw == 0
  int stride;            // floats per LDS row: K + V (sender-major pass: K + V + 4) rounded up to an odd multiple of 4
  int idx_off;           // float index of the index lists behind the rows
  float inv_sqrt_k;
  uint32_t k0, k1, step_lo, step_hi;
  int hop;
  const int32_t* step_dev;
};

template <int Q>
__device__ __forceinline__ float dot_row(const float4 (&x)[Q], const float* y, int n) {
  float d = 0.0f;
#pragma unroll
  for (int j = 0; j < Q; ++j)
    if (j < n) {
      const float4 yy = *reinterpret_cast<const float4*>(y + 4 * j);
      d = fmaf(x[j].x, yy.x, d);
      d = fmaf(x[j].y, yy.y, d);
      d = fmaf(x[j].z, yy.z, d);
      d = fmaf(x[j].w, yy.w, d);
    }
  return d;
}

// the same with the row as the first factor: q_r . k_s with the key in registers rounds as with the query in registers
template <int Q>
__device__ __forceinline__ float row_dot(const float* x, const float4 (&y)[Q], int n) {
  float d = 0.0f;
#pragma unroll
  for (int j = 0; j < Q; ++j)
    if (j < n) {
      const float4 xx = *reinterpret_cast<const float4*>(x + 4 * j);
      d = fmaf(xx.x, y[j].x, d);
      d = fmaf(xx.y, y[j].y, d);
      d = fmaf(xx.z, y[j].z, d);
      d = fmaf(xx.w, y[j].w, d);
    }
  return d;
}

// The score as a value of its own: under -ffp-contract=on a product written inside `d * inv - m` would fuse into fma(d, inv, -m),
// which differs from the rounded product the maximum was taken of - the sender holding the maximum must give exp(0) exactly.
__device__ __forceinline__ float scaled(float d, float inv) { return d * inv; }

template <int Q>
__device__ __forceinline__ void axpy_row(float w, const float* x, float4 (&acc)[Q], int n) {
#pragma unroll
  for (int j = 0; j < Q; ++j)
    if (j < n) {
      const float4 xx = *reinterpret_cast<const float4*>(x + 4 * j);
      acc[j].x = fmaf(w, xx.x, acc[j].x);
      acc[j].y = fmaf(w, xx.y, acc[j].y);
      acc[j].z = fmaf(w, xx.z, acc[j].z);
      acc[j].w = fmaf(w, xx.w, acc[j].w);
    }
}

// Floyd's algorithm over the M = N - 1 others of the receiver at house h, agent `ag` of the whole batch: for j = M - c .. M - 1
// t = (word_j (j + 1)) >> 32, taken unless already taken, then j; other index o stands for house o (o < h) or o + 1.  word_j = word
// j & 3 of Philox4x32-10, key = seed, counter (ag lo, ag hi | (j >> 2) << 16 | hop << 29 | 1 << 31, step lo + *step_dev,
// TAG_GATHER ^ step hi).  The c houses go to list[0], list[TILE], ... in insertion order; only this lane reads them back.
__device__ __forceinline__ void draw_senders(uint16_t* list, int64_t ag, int h, int N, int c, const GatherArgs& a) {
  const int M = N - 1;
  const uint32_t c0 = (uint32_t)ag;
  const uint32_t c1 = (uint32_t)((uint64_t)ag >> 32) | ((uint32_t)a.hop << 29) | 0x80000000u;
  const uint32_t c2 = a.step_lo + (a.step_dev ? (uint32_t)*a.step_dev : 0u), c3 = TAG_GATHER ^ a.step_hi;
  u32x4 r{0u, 0u, 0u, 0u};
  int n = 0;
  for (int j = M - c; j < M; ++j, ++n) {
    if (n == 0 || (j & 3) == 0) r = philox4x32_10(c0, c1 | ((uint32_t)(j >> 2) << 16), c2, c3, loop_local(a.k0), loop_local(a.k1));
    const int w = j & 3;
    const uint32_t word = w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
    const int o = (int)__umulhi(word, (uint32_t)(j + 1));
    int s = o < h ? o : o + 1;
    bool taken = false;
    for (int i = 0; i < n; ++i) taken |= list[i * TILE] == (uint16_t)s;
    if (taken) s = j < h ? j : j + 1;
    list[n * TILE] = (uint16_t)s;
  }
}

// the tile of a workgroup: whole envs or (forward only) 256 receivers of one env whose rows are all staged
struct Tile {
  int64_t agent0;      // agent of LDS row 0
  int nrows, nlane;
  int start;           // slice: house of lane 0
};

__device__ __forceinline__ Tile tile_of(const GatherArgs& a) {
  Tile w;
  w.start = 0;
  if (a.epw > 0) {
    const int64_t env0 = (int64_t)blockIdx.x * a.epw;
    const int ne = (int)(a.E - env0 < a.epw ? a.E - env0 : a.epw);
    w.agent0 = env0 * a.N;
    w.nrows = w.nlane = ne * a.N;
  } else {
    const int env = (int)(blockIdx.x / (unsigned)a.slices);
    w.start = (int)(blockIdx.x - (unsigned)env * (unsigned)a.slices) * TILE;
    w.agent0 = (int64_t)env * a.N;
    w.nrows = a.N;
    w.nlane = a.N - w.start < TILE ? a.N - w.start : TILE;
  }
  return w;
}

__device__ __forceinline__ void stage_kv(const GatherArgs& a, const Tile& w, float* rows, int kq, int vq) {
  const int cpr = kq + vq;
  for (int idx = (int)threadIdx.x; idx < w.nrows * cpr; idx += TILE) {
    const int row = idx / cpr, j = idx - row * cpr;
    const int64_t ag = w.agent0 + row;
    const float* src = j < kq ? a.k + ag * a.ldk + 4 * j : a.v + ag * a.ldv + 4 * (j - kq);
    *reinterpret_cast<float4*>(rows + row * a.stride + 4 * j) = *reinterpret_cast<const float4*>(src);
  }
}

// KQ / VQ: float4 per key / value row the lane has registers for; EXACT: the rows have exactly that many (else a.kq / a.vq of them)
template <int KQ, int VQ, bool EXACT, int MODE>
__global__ __launch_bounds__(TILE) void k_tarmac_gather(GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  uint16_t* lists = reinterpret_cast<uint16_t*>(rows + a.idx_off);
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int t = (int)threadIdx.x;
  const int N = a.N;
  const Tile w = tile_of(a);
  stage_kv(a, w, rows, kq, vq);
  const bool active = t < w.nlane;
  int base = 0, h = w.start + t;      // LDS row of house 0 of the receiver's env; the receiver's house
  if (a.epw > 0) {
    base = (t / N) * N;
    h = t - base;
  }
  const int64_t ag = w.agent0 + base + h;
  if (MODE == MDR_TARMAC_RANDOM_SAMPLE && active) draw_senders(lists + t, ag, h, N, a.c, a);
  __syncthreads();
  if (!active) return;
  float4 qr[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) qr[j] = *reinterpret_cast<const float4*>(a.q + ag * a.ldq + 4 * j);
  // sender number i: "all" house i; "random_sample" the receiver, then its list in insertion order
  const int L = MODE == MDR_TARMAC_ALL ? N : a.c + 1;
  auto sender_row = [&](int i) { return MODE == MDR_TARMAC_ALL ? base + i : i == 0 ? base + h : base + (int)lists[(i - 1) * TILE + t]; };
  float m = dot_row<KQ>(qr, rows + sender_row(0) * a.stride, kq) * a.inv_sqrt_k;
  for (int i = 1; i < L; ++i) m = fmaxf(m, dot_row<KQ>(qr, rows + sender_row(i) * a.stride, kq) * a.inv_sqrt_k);
  float4 acc[VQ];
#pragma unroll
  for (int j = 0; j < VQ; ++j) acc[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float l = 0.0f;
  for (int i = 0; i < L; ++i) {
    const float* row = rows + sender_row(i) * a.stride;
    const float p = __expf(scaled(dot_row<KQ>(qr, row, kq), a.inv_sqrt_k) - m);
    l += p;
    axpy_row<VQ>(p, row + 4 * kq, acc, vq);
  }
  const float inv = 1.0f / l;      // l >= 1: the sender holding the maximum contributes exp(0)
  float* dst = a.dst + ag * a.ldo;
#pragma unroll
  for (int j = 0; j < VQ; ++j)
    if (j < vq) *reinterpret_cast<float4*>(dst + 4 * j) = make_float4(acc[j].x * inv, acc[j].y * inv, acc[j].z * inv, acc[j].w * inv);
}

template <int KQ, int VQ, bool EXACT, int MODE>
__global__ __launch_bounds__(TILE) void k_tarmac_gather_grad_recv(GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  uint16_t* lists = reinterpret_cast<uint16_t*>(rows + a.idx_off);
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int t = (int)threadIdx.x;
  const int N = a.N;
  const Tile w = tile_of(a);      // whole envs
  stage_kv(a, w, rows, kq, vq);
  const bool active = t < w.nlane;
  const int base = (t / N) * N, h = t - base;
  const int64_t ag = w.agent0 + t;
  if (MODE == MDR_TARMAC_RANDOM_SAMPLE && active) {
    draw_senders(lists + t, ag, h, N, a.c, a);
    for (int i = 0; i < a.c; ++i) a.ws_idx[ag * a.c + i] = lists[i * TILE + t];
  }
  __syncthreads();
  if (!active) return;
  float4 qr[KQ], gr[VQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) qr[j] = *reinterpret_cast<const float4*>(a.q + ag * a.ldq + 4 * j);
#pragma unroll
  for (int j = 0; j < VQ; ++j)
    if (j < vq) gr[j] = *reinterpret_cast<const float4*>(a.g + ag * a.ldg + 4 * j);
  const float delta = dot_row<VQ>(gr, a.out + ag * a.ldo, vq);
  const int L = MODE == MDR_TARMAC_ALL ? N : a.c + 1;
  auto sender_row = [&](int i) { return MODE == MDR_TARMAC_ALL ? base + i : i == 0 ? base + h : base + (int)lists[(i - 1) * TILE + t]; };
  float m = dot_row<KQ>(qr, rows + sender_row(0) * a.stride, kq) * a.inv_sqrt_k;
  for (int i = 1; i < L; ++i) m = fmaxf(m, dot_row<KQ>(qr, rows + sender_row(i) * a.stride, kq) * a.inv_sqrt_k);
  float4 acc[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j) acc[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float l = 0.0f;
  for (int i = 0; i < L; ++i) {
    const float* row = rows + sender_row(i) * a.stride;
    const float e = __expf(scaled(dot_row<KQ>(qr, row, kq), a.inv_sqrt_k) - m);
    l += e;
    axpy_row<KQ>(e * (dot_row<VQ>(gr, row + 4 * kq, vq) - delta), row, acc, kq);
  }
  const float inv = 1.0f / l;
  const float scale = inv * a.inv_sqrt_k;
  float* dst = a.dq + ag * a.lddq;
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) *reinterpret_cast<float4*>(dst + 4 * j) = make_float4(acc[j].x * scale, acc[j].y * scale, acc[j].z * scale, acc[j].w * scale);
  a.stats[ag] = make_float4(m, inv, delta, 0.0f);
}

template <int KQ, int VQ, bool EXACT, int MODE>
__global__ __launch_bounds__(TILE) void k_tarmac_gather_grad_send(GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  uint16_t* lists = reinterpret_cast<uint16_t*>(rows + a.idx_off);      // [row][c]
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int cpr = kq + vq + 1;
  const int t = (int)threadIdx.x;
  const int N = a.N, c = a.c;
  const Tile w = tile_of(a);      // whole envs
  for (int idx = t; idx < w.nrows * cpr; idx += TILE) {
    const int row = idx / cpr, j = idx - row * cpr;
    const int64_t ag = w.agent0 + row;
    const float* src = j < kq ? a.q + ag * a.ldq + 4 * j : j < kq + vq ? a.g + ag * a.ldg + 4 * (j - kq) : reinterpret_cast<const float*>(a.stats + ag);
    *reinterpret_cast<float4*>(rows + row * a.stride + 4 * j) = *reinterpret_cast<const float4*>(src);
  }
  if (MODE == MDR_TARMAC_RANDOM_SAMPLE)
    for (int idx = t; idx < w.nrows * c; idx += TILE) lists[idx] = a.ws_idx[w.agent0 * c + idx];
  __syncthreads();
  if (t >= w.nlane) return;
  const int base = (t / N) * N, h = t - base;
  const int64_t ag = w.agent0 + t;
  float4 kr[KQ], vr[VQ], dk[KQ], dv[VQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j) {
    if (j < kq) kr[j] = *reinterpret_cast<const float4*>(a.k + ag * a.ldk + 4 * j);
    dk[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
#pragma unroll
  for (int j = 0; j < VQ; ++j) {
    if (j < vq) vr[j] = *reinterpret_cast<const float4*>(a.v + ag * a.ldv + 4 * j);
    dv[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  for (int r = 0; r < N; ++r) {      // the receivers of the env in ascending order
    if (MODE == MDR_TARMAC_RANDOM_SAMPLE && r != h) {
      const uint16_t* list = lists + (base + r) * c;
      bool hears = false;
      for (int i = 0; i < c; ++i) hears |= list[i] == (uint16_t)h;
      if (!hears) continue;
    }
    const float* row = rows + (base + r) * a.stride;
    const float4 st = *reinterpret_cast<const float4*>(row + 4 * (kq + vq));
    const float p = __expf(scaled(row_dot<KQ>(row, kr, kq), a.inv_sqrt_k) - st.x) * st.y;
    const float ds = p * (row_dot<VQ>(row + 4 * kq, vr, vq) - st.z);
    axpy_row<KQ>(ds, row, dk, kq);
    axpy_row<VQ>(p, row + 4 * kq, dv, vq);
  }
  const float sc = a.inv_sqrt_k;
  float* dst = a.dk + ag * a.lddk;
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) *reinterpret_cast<float4*>(dst + 4 * j) = make_float4(dk[j].x * sc, dk[j].y * sc, dk[j].z * sc, dk[j].w * sc);
  dst = a.dv + ag * a.lddv;
#pragma unroll
  for (int j = 0; j < VQ; ++j)
    if (j < vq) *reinterpret_cast<float4*>(dst + 4 * j) = dv[j];
}

template <typename K>
int prepare(K kernel, size_t lds_bytes) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  return MDR_OK;
}

template <int KQ, int VQ, bool EXACT, int MODE>
int launch_forward(unsigned grid, size_t lds, hipStream_t s, const GatherArgs& a) {
  if (prepare(k_tarmac_gather<KQ, VQ, EXACT, MODE>, lds) != MDR_OK) return MDR_ERR_HIP;
  hipLaunchKernelGGL((k_tarmac_gather<KQ, VQ, EXACT, MODE>), dim3(grid), dim3(TILE), lds, s, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// both kernels of one instantiation; nothing is launched unless both can be.  `a` holds the receiver pass's LDS layout.
template <int KQ, int VQ, bool EXACT, int MODE>
int launch_backward(unsigned grid, size_t lds_recv, size_t lds_send, int stride_send, int idx_off_send, hipStream_t s, GatherArgs a) {
  if (prepare(k_tarmac_gather_grad_recv<KQ, VQ, EXACT, MODE>, lds_recv) != MDR_OK ||
      prepare(k_tarmac_gather_grad_send<KQ, VQ, EXACT, MODE>, lds_send) != MDR_OK)
    return MDR_ERR_HIP;
  hipLaunchKernelGGL((k_tarmac_gather_grad_recv<KQ, VQ, EXACT, MODE>), dim3(grid), dim3(TILE), lds_recv, s, a);
  if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
  a.stride = stride_send, a.idx_off = idx_off_send;
  hipLaunchKernelGGL((k_tarmac_gather_grad_send<KQ, VQ, EXACT, MODE>), dim3(grid), dim3(TILE), lds_send, s, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 3) == 0; }

size_t list_bytes(int mode, int entries, int c) {      // uint16 lists, rounded up to 16 bytes
  return mode == MDR_TARMAC_RANDOM_SAMPLE ? (((size_t)entries * c * sizeof(uint16_t) + 15) & ~(size_t)15) : 0;
}

// the checks both entry points share; c is set on success
int check_common(int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, int32_t hop, int* c) {
  if (nb_envs < 0 || nb_houses <= 0 || nb_comm < 0) return MDR_ERR_INVALID;
  if (mode != MDR_TARMAC_ALL && mode != MDR_TARMAC_RANDOM_SAMPLE) return MDR_ERR_INVALID;
  if (hop < 0 || hop > 3) return MDR_ERR_INVALID;
  if (num_key <= 0 || num_value <= 0) return MDR_ERR_INVALID;
  if (num_key % 4 || num_key > 32 || num_value % 4 || num_value > 64) return MDR_ERR_UNSUPPORTED;
  *c = mode == MDR_TARMAC_ALL ? 0 : nb_comm < nb_houses - 1 ? nb_comm : nb_houses - 1;      // make_masks 140-141
  return MDR_OK;
}

void fill_common(GatherArgs& a, int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int c, uint64_t seed, uint64_t step,
                 const int32_t* step_dev, int32_t hop) {
  a.E = nb_envs, a.N = nb_houses;
  a.kq = num_key / 4, a.vq = num_value / 4;
  a.c = c;
  a.epw = nb_houses <= TILE ? TILE / nb_houses : 0;
  a.slices = a.epw ? 0 : (nb_houses + TILE - 1) / TILE;
  a.inv_sqrt_k = 1.0f / sqrtf((float)num_key);
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.hop = hop;
  a.step_dev = step_dev;
}

template <int MODE>
int dispatch_forward(unsigned grid, size_t lds, hipStream_t s, const GatherArgs& a) {
  if (a.kq == 2 && a.vq == 4) return launch_forward<2, 4, true, MODE>(grid, lds, s, a);      // the reference's sizes
  if (a.kq <= 4 && a.vq <= 8) return launch_forward<4, 8, false, MODE>(grid, lds, s, a);
  return launch_forward<8, 16, false, MODE>(grid, lds, s, a);
}

template <int MODE>
int dispatch_backward(unsigned grid, size_t lds_recv, size_t lds_send, int stride_send, int idx_off_send, hipStream_t s, const GatherArgs& a) {
  if (a.kq == 2 && a.vq == 4) return launch_backward<2, 4, true, MODE>(grid, lds_recv, lds_send, stride_send, idx_off_send, s, a);
  if (a.kq <= 4 && a.vq <= 8) return launch_backward<4, 8, false, MODE>(grid, lds_recv, lds_send, stride_send, idx_off_send, s, a);
  return launch_backward<8, 16, false, MODE>(grid, lds_recv, lds_send, stride_send, idx_off_send, s, a);
}

}  // namespace

extern "C" {

int mdr_tarmac_gather(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                      int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, uint64_t seed, uint64_t step,
                      const int32_t* step_dev, int32_t hop, float* out, int64_t ldo, void* stream) {
  if (!query || !key || !value || !out) return MDR_ERR_INVALID;
  int c = 0;
  const int rc = check_common(nb_envs, nb_houses, num_key, num_value, nb_comm, mode, hop, &c);
  if (rc != MDR_OK) return rc;
  if (!aligned16(query, ldq) || !aligned16(key, ldk) || !aligned16(value, ldv) || !aligned16(out, ldo)) return MDR_ERR_INVALID;
  if (ldq < num_key || ldk < num_key || ldv < num_value || ldo < num_value) return MDR_ERR_INVALID;
  if (c > MAX_C) return MDR_ERR_UNSUPPORTED;
  if (nb_envs == 0) return MDR_OK;
  if ((int64_t)nb_envs * nb_houses >= ((int64_t)1 << 48)) return MDR_ERR_UNSUPPORTED;      // the counter holds 48 bits of the agent index
  GatherArgs a{};
  a.q = query, a.k = key, a.v = value, a.dst = out;
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo;
  fill_common(a, nb_envs, nb_houses, num_key, num_value, c, seed, step, step_dev, hop);
  a.stride = 4 * ((a.kq + a.vq) | 1);      // an odd multiple of 4 floats: no two lanes of a ds_read_b128 group on one bank
  const int64_t max_rows = a.epw ? (int64_t)a.epw * nb_houses : nb_houses;      // every row of the env is staged
  const size_t lds = (size_t)max_rows * a.stride * sizeof(float) + list_bytes(mode, TILE, c);
  if (lds > MAX_LDS) return MDR_ERR_UNSUPPORTED;
  a.idx_off = (int)(max_rows * a.stride);
  const int64_t grid = a.epw ? ((int64_t)nb_envs + a.epw - 1) / a.epw : (int64_t)nb_envs * a.slices;
  if (grid > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return mode == MDR_TARMAC_ALL ? dispatch_forward<MDR_TARMAC_ALL>((unsigned)grid, lds, s, a)
                                : dispatch_forward<MDR_TARMAC_RANDOM_SAMPLE>((unsigned)grid, lds, s, a);
}

int64_t mdr_tarmac_gather_backward_workspace_bytes(int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm,
                                                   int32_t mode) {
  int c = 0;
  if (check_common(nb_envs, nb_houses, num_key, num_value, nb_comm, mode, 0, &c) != MDR_OK) return -1;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  return A * (int64_t)sizeof(float4) + (mode == MDR_TARMAC_RANDOM_SAMPLE ? ((A * c * (int64_t)sizeof(uint16_t) + 15) & ~(int64_t)15) : 0);
}

int mdr_tarmac_gather_backward(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                               int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, uint64_t seed,
                               uint64_t step, const int32_t* step_dev, int32_t hop, const float* out, int64_t ldo, const float* grad_out,
                               int64_t ldg, float* grad_query, int64_t ldgq, float* grad_key, int64_t ldgk, float* grad_value, int64_t ldgv,
                               void* workspace, void* stream) {
  if (!query || !key || !value || !out || !grad_out || !grad_query || !grad_key || !grad_value) return MDR_ERR_INVALID;
  int c = 0;
  const int rc = check_common(nb_envs, nb_houses, num_key, num_value, nb_comm, mode, hop, &c);
  if (rc != MDR_OK) return rc;
  if (!aligned16(query, ldq) || !aligned16(key, ldk) || !aligned16(value, ldv) || !aligned16(out, ldo) || !aligned16(grad_out, ldg) ||
      !aligned16(grad_query, ldgq) || !aligned16(grad_key, ldgk) || !aligned16(grad_value, ldgv))
    return MDR_ERR_INVALID;
  if (ldq < num_key || ldk < num_key || ldgq < num_key || ldgk < num_key) return MDR_ERR_INVALID;
  if (ldv < num_value || ldo < num_value || ldg < num_value || ldgv < num_value) return MDR_ERR_INVALID;
  if (!workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  if (c > MAX_C || nb_houses > TILE) return MDR_ERR_UNSUPPORTED;      // the backward covers whole envs per workgroup
  if (nb_envs == 0) return MDR_OK;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  GatherArgs a{};
  a.q = query, a.k = key, a.v = value, a.out = out, a.g = grad_out;
  a.dq = grad_query, a.dk = grad_key, a.dv = grad_value;
  a.stats = reinterpret_cast<float4*>(workspace);
  a.ws_idx = reinterpret_cast<uint16_t*>(a.stats + A);
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.ldg = ldg, a.lddq = ldgq, a.lddk = ldgk, a.lddv = ldgv;
  fill_common(a, nb_envs, nb_houses, num_key, num_value, c, seed, step, step_dev, hop);
  const int max_rows = a.epw * nb_houses;
  a.stride = 4 * ((a.kq + a.vq) | 1);
  a.idx_off = max_rows * a.stride;
  const int stride_send = 4 * ((a.kq + a.vq + 1) | 1);
  // at most 256 rows of 100 floats and 256 lists of 64 uint16: 135,168 bytes, inside the 160 KB of a workgroup
  const size_t lds_recv = (size_t)max_rows * a.stride * sizeof(float) + list_bytes(mode, TILE, c);
  const size_t lds_send = (size_t)max_rows * stride_send * sizeof(float) + list_bytes(mode, max_rows, c);
  if (lds_recv > MAX_LDS || lds_send > MAX_LDS) return MDR_ERR_UNSUPPORTED;
  const int64_t grid = ((int64_t)nb_envs + a.epw - 1) / a.epw;
  if (grid > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return mode == MDR_TARMAC_ALL
             ? dispatch_backward<MDR_TARMAC_ALL>((unsigned)grid, lds_recv, lds_send, stride_send, max_rows * stride_send, s, a)
             : dispatch_backward<MDR_TARMAC_RANDOM_SAMPLE>((unsigned)grid, lds_recv, lds_send, stride_send, max_rows * stride_send, s, a);
}

}  // extern "C"
