// Backward of the banded masked attention of csrc/mdr_tarmac.hip (include/mdr_policy.h, mdr_tarmac_comm_backward): the gradient
// of out_r = sum_s p_rs v_s with respect to query, key and value, O(E N c) like the forward.
//
//   delta_r = g_r . out_r          ds_rs = p_rs (g_r . v_s - delta_r)
//   dq_r = (1 / sqrt K) sum_{s in S(r)} ds_rs k_s      dk_s = (1 / sqrt K) sum_{r: s in S(r)} ds_rs q_r      dv_s = sum_{r: s in S(r)} p_rs g_r
//
// Two kernels on the forward's tiling (256 consecutive agents of one env, or floor(256 / N) whole envs, rows staged once in LDS
// with 16-byte accesses at a stride that is an odd multiple of 4 floats), NO floating-point atomics - dk and dv are gathered per
// sender, so two calls on the same operands give the same bits:
//
//   k_tarmac_grad_recv   receiver-major, k_tarmac_comm's staging of key | value rows and dead flags.  One lane per receiver keeps
//                        query and grad_out in registers, forms delta from the forward's out, walks its live senders twice (the
//                        maximum; then exp(score - max), the sum and sum_s e_s (g . v_s - delta) k_s), writes dq and the
//                        receiver's statistics (max, 1 / sum, delta, 0) as one float4 into the workspace.
//   k_tarmac_grad_send   sender-major.  Stages query | grad_out | statistics rows of the tile's receivers plus the MIRRORED halo:
//                        sender s is heard by the receivers s - o, so the halo has ceil(c / 2) rows on the - side and floor(c / 2) on
//                        the + side.  One lane per sender keeps its key and value in registers, draws its own dead flag (a dead
//                        sender is heard by itself only), walks its c + 1 receivers, recomputes p_rs from the stored statistics -
//                        the score is the forward's fma chain on the same operands, hence the same bits - and accumulates dk, dv.
//   k_tarmac_grad_zero   mode "none": the output is the constant 0, so are the three gradients.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_device.h"
#include "mdr_draw.h"

namespace {

using mdr::action_uniform;
using mdr::loop_local;
using mdr::philox4x32_10;
using mdr::u32x4;

constexpr uint32_t TAG_TARMAC = 0x544D4331u;
constexpr int TILE = 256;
constexpr int MAX_C = 64;

struct GradArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* out;
  const float* g;
  float* dq;
  float* dk;
  float* dv;
  float4* stats;      // per receiver: max score, 1 / sum, delta, 0
  int64_t ldq, ldk, ldv, ldo, ldg, lddq, lddk, lddv;
  int E, N;
  int kq, vq;        // float4 per key / value row
  int c, hm;         // senders besides the receiver itself; floor(c / 2)
  int epw;           // whole envs per workgroup (N <= 256), 0: slices of an env
  int slices;        // ceil(N / 256) when epw == 0
  int stride_kv;     // floats per LDS row of the receiver-major kernel: K + V rounded up to an odd multiple of 4
  int stride_qg;     // ... of the sender-major kernel: K + V + 4
  int dead_off;      // receiver-major: float index of the dead-sender flags behind the rows
  float inv_sqrt_k;
  float defect_prob;
  uint32_t k0, k1, step_lo, step_hi;
  int hop;
  const int32_t* step_dev;
  const int32_t* key;      // may be NULL: k0, k1 above
};

__device__ __forceinline__ int wrap(int h, int n) {      // h in [-n, 2 n)
  h = h < 0 ? h + n : h;
  return h >= n ? h - n : h;
}

// offset number i >= 1 of make_masks: +1, -1, +2, -2, ...
__device__ __forceinline__ int band_offset(int i) { return (i & 1) ? (i + 1) >> 1 : -(i >> 1); }

__device__ __forceinline__ bool sender_dead(const GradArgs& a, int64_t ag) {
  const uint32_t c2 = a.step_lo + (a.step_dev ? (uint32_t)*a.step_dev : 0u), c3 = TAG_TARMAC ^ a.step_hi;
  // the key from device memory is the same word in every lane: readfirstlane hands loop_local the scalar it asks for
  const uint32_t k0 = a.key ? (uint32_t)__builtin_amdgcn_readfirstlane(a.key[0]) : a.k0;
  const uint32_t k1 = a.key ? (uint32_t)__builtin_amdgcn_readfirstlane(a.key[1]) : a.k1;
  const u32x4 r = philox4x32_10((uint32_t)ag, (uint32_t)((uint64_t)ag >> 32), c2, c3, loop_local(k0), loop_local(k1));
  const uint32_t word = a.hop == 0 ? r.x : a.hop == 1 ? r.y : a.hop == 2 ? r.z : r.w;
  return action_uniform(word) < a.defect_prob;
}

// sum_j x_j y_j over n float4 of registers `x` and of the row `y`, the forward's chain: x first, ascending
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

// the tile of a workgroup: whole envs (agent0 = agent of LDS row 0) or a slice of one env (agent0 = its first agent, `start` the
// house of lane 0); `nlane` agents get a lane
struct Tile {
  int64_t agent0;
  int start, nlane;
  bool whole;
};

__device__ __forceinline__ Tile tile_of(const GradArgs& a) {
  Tile w;
  w.whole = a.epw > 0;
  w.start = 0;
  if (w.whole) {
    const int64_t env0 = (int64_t)blockIdx.x * a.epw;
    const int ne = (int)(a.E - env0 < a.epw ? a.E - env0 : a.epw);
    w.agent0 = env0 * a.N;
    w.nlane = ne * a.N;
  } else {
    const int env = (int)(blockIdx.x / (unsigned)a.slices);
    w.start = (int)(blockIdx.x - (unsigned)env * (unsigned)a.slices) * TILE;
    w.agent0 = (int64_t)env * a.N;
    w.nlane = a.N - w.start < TILE ? a.N - w.start : TILE;
  }
  return w;
}

// KQ / VQ: float4 per key / value row the lane has registers for; EXACT: the rows have exactly that many (else a.kq / a.vq of them)
template <int KQ, int VQ, bool EXACT>
__global__ __launch_bounds__(TILE) void k_tarmac_grad_recv(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  uint32_t* dead = reinterpret_cast<uint32_t*>(smem) + a.dead_off;
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int cpr = kq + vq;
  const int t = (int)threadIdx.x;
  const int N = a.N;
  const Tile w = tile_of(a);
  const bool whole = w.whole;
  const int nrows = whole ? w.nlane : w.nlane + a.c;      // slice: row j is house start - hm + j
  // ---- stage keys and values (and the halo) once, as k_tarmac_comm
  for (int idx = t; idx < nrows * cpr; idx += TILE) {
    const int row = idx / cpr, j = idx - row * cpr;
    const int64_t ag = w.agent0 + (whole ? row : wrap(w.start - a.hm + row, N));
    const float* src = j < kq ? a.k + ag * a.ldk + 4 * j : a.v + ag * a.ldv + 4 * (j - kq);
    *reinterpret_cast<float4*>(rows + row * a.stride_kv + 4 * j) = *reinterpret_cast<const float4*>(src);
  }
  const bool defects = a.defect_prob > 0.0f;
  if (defects)
    for (int row = t; row < nrows; row += TILE)
      dead[row] = sender_dead(a, w.agent0 + (whole ? row : wrap(w.start - a.hm + row, N))) ? 1u : 0u;
  __syncthreads();
  if (t >= w.nlane) return;
  // ---- one lane per receiver
  int base = 0, h = t, own = a.hm + t;      // slice: sender at offset o is row own + o
  if (whole) {
    const int e = t / N;
    base = e * N;
    h = t - base;
    own = t;
  }
  const int64_t ag = w.agent0 + (whole ? t : w.start + t);
  float4 qr[KQ], gr[VQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) qr[j] = *reinterpret_cast<const float4*>(a.q + ag * a.ldq + 4 * j);
#pragma unroll
  for (int j = 0; j < VQ; ++j)
    if (j < vq) gr[j] = *reinterpret_cast<const float4*>(a.g + ag * a.ldg + 4 * j);
  const float delta = dot_row<VQ>(gr, a.out + ag * a.ldo, vq);
  auto sender_row = [&](int i) { return whole ? base + wrap(h + band_offset(i), N) : own + band_offset(i); };
  float m = dot_row<KQ>(qr, rows + own * a.stride_kv, kq) * a.inv_sqrt_k;
  for (int i = 1; i <= a.c; ++i) {
    const int s = sender_row(i);
    if (defects && dead[s]) continue;
    m = fmaxf(m, dot_row<KQ>(qr, rows + s * a.stride_kv, kq) * a.inv_sqrt_k);
  }
  float4 acc[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j) acc[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float l = 0.0f;
  for (int i = 0; i <= a.c; ++i) {
    const int s = i == 0 ? own : sender_row(i);
    if (i > 0 && defects && dead[s]) continue;
    const float* row = rows + s * a.stride_kv;
    const float e = __expf(dot_row<KQ>(qr, row, kq) * a.inv_sqrt_k - m);
    l += e;
    axpy_row<KQ>(e * (dot_row<VQ>(gr, row + 4 * kq, vq) - delta), row, acc, kq);
  }
  const float inv = 1.0f / l;      // l >= 1: the sender holding the maximum contributes exp(0)
  const float scale = inv * a.inv_sqrt_k;
  float* dst = a.dq + ag * a.lddq;
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) *reinterpret_cast<float4*>(dst + 4 * j) = make_float4(acc[j].x * scale, acc[j].y * scale, acc[j].z * scale, acc[j].w * scale);
  a.stats[ag] = make_float4(m, inv, delta, 0.0f);
}

template <int KQ, int VQ, bool EXACT>
__global__ __launch_bounds__(TILE) void k_tarmac_grad_send(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int cpr = kq + vq + 1;
  const int t = (int)threadIdx.x;
  const int N = a.N;
  const Tile w = tile_of(a);
  const bool whole = w.whole;
  const int hp = a.c - a.hm;      // ceil(c / 2): the receivers s - o of the + offsets lie on the - side
  const int nrows = whole ? w.nlane : w.nlane + a.c;      // slice: row j is house start - hp + j
  // ---- stage query | grad_out | statistics of the tile's receivers (and the mirrored halo) once
  for (int idx = t; idx < nrows * cpr; idx += TILE) {
    const int row = idx / cpr, j = idx - row * cpr;
    const int64_t ag = w.agent0 + (whole ? row : wrap(w.start - hp + row, N));
    const float* src = j < kq ? a.q + ag * a.ldq + 4 * j : j < kq + vq ? a.g + ag * a.ldg + 4 * (j - kq) : reinterpret_cast<const float*>(a.stats + ag);
    *reinterpret_cast<float4*>(rows + row * a.stride_qg + 4 * j) = *reinterpret_cast<const float4*>(src);
  }
  __syncthreads();
  if (t >= w.nlane) return;
  // ---- one lane per sender
  int base = 0, h = t, own = hp + t;      // slice: the receiver hearing this sender at offset o is row own - o
  if (whole) {
    const int e = t / N;
    base = e * N;
    h = t - base;
    own = t;
  }
  const int64_t ag = w.agent0 + (whole ? t : w.start + t);
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
  // a silenced sender is heard by itself only
  const int heard = (a.defect_prob > 0.0f && sender_dead(a, ag)) ? 0 : a.c;
  for (int i = 0; i <= heard; ++i) {
    const int r = i == 0 ? own : whole ? base + wrap(h - band_offset(i), N) : own - band_offset(i);
    const float* row = rows + r * a.stride_qg;
    const float4 st = *reinterpret_cast<const float4*>(row + 4 * (kq + vq));
    const float p = __expf(row_dot<KQ>(row, kr, kq) * a.inv_sqrt_k - st.x) * st.y;
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

__global__ __launch_bounds__(TILE) void k_tarmac_grad_zero(float* out, int64_t ld, int quads, int64_t chunks) {
  const int64_t idx = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (idx >= chunks) return;
  const int64_t ag = idx / quads;
  const int j = (int)(idx - ag * quads);
  *reinterpret_cast<float4*>(out + ag * ld + 4 * j) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <typename K>
int prepare(K kernel, size_t lds_bytes) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  return MDR_OK;
}

// both kernels of one instantiation; nothing is launched unless both can be
template <int KQ, int VQ, bool EXACT>
int launch_grad(unsigned grid, size_t lds_recv, size_t lds_send, hipStream_t s, const GradArgs& a) {
  if (prepare(k_tarmac_grad_recv<KQ, VQ, EXACT>, lds_recv) != MDR_OK || prepare(k_tarmac_grad_send<KQ, VQ, EXACT>, lds_send) != MDR_OK)
    return MDR_ERR_HIP;
  hipLaunchKernelGGL((k_tarmac_grad_recv<KQ, VQ, EXACT>), dim3(grid), dim3(TILE), lds_recv, s, a);
  if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
  hipLaunchKernelGGL((k_tarmac_grad_send<KQ, VQ, EXACT>), dim3(grid), dim3(TILE), lds_send, s, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 3) == 0; }

// the by-value entry point (key_dev NULL: the key is `seed`) and the keyed one
int comm_backward(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                  int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob,
                  const int32_t* key_dev, uint64_t seed, uint64_t step, const int32_t* step_dev, int32_t hop, const float* out, int64_t ldo,
                  const float* grad_out, int64_t ldg, float* grad_query, int64_t ldgq, float* grad_key, int64_t ldgk, float* grad_value,
                  int64_t ldgv, void* workspace, void* stream) {
  if (!query || !key || !value || !out || !grad_out || !grad_query || !grad_key || !grad_value) return MDR_ERR_INVALID;
  if (nb_envs < 0 || nb_houses <= 0 || nb_comm < 0) return MDR_ERR_INVALID;
  if (mode != MDR_TARMAC_NEIGHBOURS && mode != MDR_TARMAC_NONE) return MDR_ERR_INVALID;
  if (hop < 0 || hop > 3 || !(defect_prob >= 0.0f && defect_prob <= 1.0f)) return MDR_ERR_INVALID;
  if (num_key <= 0 || num_value <= 0) return MDR_ERR_INVALID;
  if (num_key % 4 || num_key > 32 || num_value % 4 || num_value > 64) return MDR_ERR_UNSUPPORTED;
  if (!aligned16(query, ldq) || !aligned16(key, ldk) || !aligned16(value, ldv) || !aligned16(out, ldo) || !aligned16(grad_out, ldg) ||
      !aligned16(grad_query, ldgq) || !aligned16(grad_key, ldgk) || !aligned16(grad_value, ldgv))
    return MDR_ERR_INVALID;
  if (ldq < num_key || ldk < num_key || ldgq < num_key || ldgk < num_key) return MDR_ERR_INVALID;
  if (ldv < num_value || ldo < num_value || ldg < num_value || ldgv < num_value) return MDR_ERR_INVALID;
  const int c = nb_comm < nb_houses - 1 ? nb_comm : nb_houses - 1;      // make_masks 140-141
  if (mode == MDR_TARMAC_NEIGHBOURS && c > MAX_C) return MDR_ERR_UNSUPPORTED;
  if (nb_envs == 0) return MDR_OK;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  hipStream_t s = (hipStream_t)stream;
  const int kq = num_key / 4, vq = num_value / 4;
  if (mode == MDR_TARMAC_NONE) {
    const int64_t most = A * (kq > vq ? kq : vq);
    if ((most + TILE - 1) / TILE > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
    float* dst[3] = {grad_query, grad_key, grad_value};
    const int64_t ld[3] = {ldgq, ldgk, ldgv};
    const int quads[3] = {kq, kq, vq};
    for (int i = 0; i < 3; ++i) {
      const int64_t chunks = A * quads[i];
      hipLaunchKernelGGL(k_tarmac_grad_zero, dim3((unsigned)((chunks + TILE - 1) / TILE)), dim3(TILE), 0, s, dst[i], ld[i], quads[i], chunks);
      if (hipGetLastError() != hipSuccess) return MDR_ERR_HIP;
    }
    return MDR_OK;
  }
  if (!workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  GradArgs a{};
  a.q = query, a.k = key, a.v = value, a.out = out, a.g = grad_out;
  a.dq = grad_query, a.dk = grad_key, a.dv = grad_value;
  a.stats = reinterpret_cast<float4*>(workspace);
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.ldg = ldg, a.lddq = ldgq, a.lddk = ldgk, a.lddv = ldgv;
  a.E = nb_envs, a.N = nb_houses;
  a.kq = kq, a.vq = vq;
  a.c = c, a.hm = c / 2;
  a.epw = nb_houses <= TILE ? TILE / nb_houses : 0;
  a.slices = a.epw ? 0 : (nb_houses + TILE - 1) / TILE;
  a.stride_kv = 4 * ((kq + vq) | 1);      // odd multiples of 4 floats: no two lanes of a ds_read_b128 group on one bank
  a.stride_qg = 4 * ((kq + vq + 1) | 1);
  const int max_rows = a.epw ? a.epw * nb_houses : TILE + c;
  a.dead_off = max_rows * a.stride_kv;
  a.inv_sqrt_k = 1.0f / sqrtf((float)num_key);
  a.defect_prob = defect_prob;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.hop = hop;
  a.step_dev = step_dev;
  a.key = key_dev;
  const int64_t grid = a.epw ? ((int64_t)nb_envs + a.epw - 1) / a.epw : (int64_t)nb_envs * a.slices;
  if (grid > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
  // at most 320 rows of 100 floats: 128,000 bytes (+ 1,280 of flags), inside the 160 KB of a workgroup for every served shape
  const size_t lds_recv = ((size_t)max_rows * a.stride_kv + (defect_prob > 0.0f ? max_rows : 0)) * sizeof(float);
  const size_t lds_send = (size_t)max_rows * a.stride_qg * sizeof(float);
  if (lds_recv > 160 * 1024 || lds_send > 160 * 1024) return MDR_ERR_UNSUPPORTED;
  if (kq == 2 && vq == 4) return launch_grad<2, 4, true>((unsigned)grid, lds_recv, lds_send, s, a);      // the reference's sizes
  if (kq <= 4 && vq <= 8) return launch_grad<4, 8, false>((unsigned)grid, lds_recv, lds_send, s, a);
  return launch_grad<8, 16, false>((unsigned)grid, lds_recv, lds_send, s, a);
}

}  // namespace

extern "C" {

int64_t mdr_tarmac_comm_backward_workspace_bytes(int64_t nb_agents, int32_t num_key, int32_t num_value) {
  if (nb_agents < 0 || num_key <= 0 || num_value <= 0) return -1;
  return nb_agents * (int64_t)sizeof(float4);
}

int mdr_tarmac_comm_backward(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                             int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob,
                             uint64_t seed, uint64_t step, const int32_t* step_dev, int32_t hop, const float* out, int64_t ldo,
                             const float* grad_out, int64_t ldg, float* grad_query, int64_t ldgq, float* grad_key, int64_t ldgk,
                             float* grad_value, int64_t ldgv, void* workspace, void* stream) {
  return comm_backward(query, ldq, key, ldk, value, ldv, nb_envs, nb_houses, num_key, num_value, nb_comm, mode, defect_prob, nullptr, seed, step,
                       step_dev, hop, out, ldo, grad_out, ldg, grad_query, ldgq, grad_key, ldgk, grad_value, ldgv, workspace, stream);
}

int mdr_tarmac_comm_backward_keyed(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv,
                                   int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode,
                                   float defect_prob, const int32_t* key_dev, uint64_t step, const int32_t* step_dev, int32_t hop,
                                   const float* out, int64_t ldo, const float* grad_out, int64_t ldg, float* grad_query, int64_t ldgq,
                                   float* grad_key, int64_t ldgk, float* grad_value, int64_t ldgv, void* workspace, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return comm_backward(query, ldq, key, ldk, value, ldv, nb_envs, nb_houses, num_key, num_value, nb_comm, mode, defect_prob, key_dev, 0, step,
                       step_dev, hop, out, ldo, grad_out, ldg, grad_query, ldgq, grad_key, ldgk, grad_value, ldgv, workspace, stream);
}

}  // extern "C"
