// TarMAC-PPO actor (include/mdr_policy.h): the banded masked attention of TarMAC_Comm.forward and the policy head's last step.
//
// Reference: agents/network.py:180-199 builds, per env, the dense agents x agents score matrix query . key^T / sqrt(K), masks it
// (make_masks 138-177: in mode "neighbours" a circular band of c + 1 non-zeros per row) and multiplies the masked softmax into the
// values.  Here the band is walked directly, O(E N c):
//
//   k_tarmac_comm   one workgroup = 256 consecutive agents of one env (N > 256) or floor(256 / N) whole envs.  The key and value rows
//                   of those agents - plus, for a slice of an env, the circular halo of ceil(c / 2) rows on the + side and
//                   floor(c / 2) on the - side - are staged ONCE in LDS with 16-byte accesses, one row of K + V floats per agent at a
//                   stride that is an odd multiple of 4 floats (the 16 lanes of a ds_read_b128 group then start on 16 different
//                   4-bank groups).  One lane per receiver keeps its query in registers and walks its c + 1 senders twice: the
//                   maximum of the scores first, then exp(score - max), the sum and the weighted values.  The scores of the
//                   second pass are the same fma chains on the same operands, hence the same bits; nothing is rescaled.
//   k_tarmac_zero   mode "none": the reference's all-zero mask gives 0 / 0 -> NaN -> 0, i.e. comm = 0 exactly.
//   k_logits_sample softmax over two logits, the project's action draw (mdr_draw.h), a_prob.
//
// Communication defects (make_masks 159-165: a sender is silenced for every receiver but itself): one Philox draw per STAGED row,
// kept as a flag beside the rows in LDS - word `hop` of Philox4x32-10, counter (sender's agent index lo, hi, step lo + *step_dev,
// TAG_TARMAC ^ step hi), dead iff action_uniform(word) < defect_prob.
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

struct CommArgs {
  const float* q;
  const float* k;
  const float* v;
  float* out;
  int64_t ldq, ldk, ldv, ldo;
  int E, N;
  int kq, vq;        // float4 per key / value row
  int c, hm;         // senders besides the receiver itself; halo rows on the - side (floor(c / 2))
  int epw;           // whole envs per workgroup (N <= 256), 0: slices of an env
  int slices;        // ceil(N / 256) when epw == 0
  int stride;        // floats per LDS row: K + V rounded up to an odd multiple of 4
  int dead_off;      // float index of the dead-sender flags behind the rows
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

template <int KQ>
__device__ __forceinline__ float score(const float4 (&qr)[KQ], const float* row, int kq, float inv_sqrt_k) {
  float d = 0.0f;
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) {
      const float4 kk = *reinterpret_cast<const float4*>(row + 4 * j);
      d = fmaf(qr[j].x, kk.x, d);
      d = fmaf(qr[j].y, kk.y, d);
      d = fmaf(qr[j].z, kk.z, d);
      d = fmaf(qr[j].w, kk.w, d);
    }
  return d * inv_sqrt_k;
}

// KQ / VQ: float4 per key / value row the lane has registers for; EXACT: the rows have exactly that many (else a.kq / a.vq of them)
template <int KQ, int VQ, bool EXACT>
__global__ __launch_bounds__(TILE) void k_tarmac_comm(CommArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  uint32_t* dead = reinterpret_cast<uint32_t*>(smem) + a.dead_off;
  const int kq = EXACT ? KQ : a.kq, vq = EXACT ? VQ : a.vq;
  const int cpr = kq + vq;
  const int t = (int)threadIdx.x;
  const int N = a.N;
  const bool whole = a.epw > 0;
  int64_t agent0;      // whole envs: agent of LDS row 0; slice: first agent of the env
  int start = 0;       // slice: house of receiver 0
  int nrows, nrecv;
  if (whole) {
    const int64_t env0 = (int64_t)blockIdx.x * a.epw;
    const int ne = (int)(a.E - env0 < a.epw ? a.E - env0 : a.epw);
    agent0 = env0 * N;
    nrows = nrecv = ne * N;
  } else {
    const int env = (int)(blockIdx.x / (unsigned)a.slices);
    start = (int)(blockIdx.x - (unsigned)env * (unsigned)a.slices) * TILE;
    agent0 = (int64_t)env * N;
    nrecv = N - start < TILE ? N - start : TILE;
    nrows = nrecv + a.c;
  }
  // ---- stage keys and values (and the halo) once: thread -> one float4 of one row, consecutive threads consecutive chunks
  for (int idx = t; idx < nrows * cpr; idx += TILE) {
    const int row = idx / cpr, j = idx - row * cpr;
    const int64_t ag = agent0 + (whole ? row : wrap(start - a.hm + row, N));
    const float* src = j < kq ? a.k + ag * a.ldk + 4 * j : a.v + ag * a.ldv + 4 * (j - kq);
    *reinterpret_cast<float4*>(rows + row * a.stride + 4 * j) = *reinterpret_cast<const float4*>(src);
  }
  const bool defects = a.defect_prob > 0.0f;
  if (defects) {
    const uint32_t c2 = a.step_lo + (a.step_dev ? (uint32_t)*a.step_dev : 0u), c3 = TAG_TARMAC ^ a.step_hi;
    // the key from device memory is the same word in every lane: readfirstlane hands loop_local the scalar it asks for
    const uint32_t k0 = a.key ? (uint32_t)__builtin_amdgcn_readfirstlane(a.key[0]) : a.k0;
    const uint32_t k1 = a.key ? (uint32_t)__builtin_amdgcn_readfirstlane(a.key[1]) : a.k1;
    for (int row = t; row < nrows; row += TILE) {
      const int64_t ag = agent0 + (whole ? row : wrap(start - a.hm + row, N));
      const u32x4 r = philox4x32_10((uint32_t)ag, (uint32_t)((uint64_t)ag >> 32), c2, c3, loop_local(k0), loop_local(k1));
      const uint32_t word = a.hop == 0 ? r.x : a.hop == 1 ? r.y : a.hop == 2 ? r.z : r.w;
      dead[row] = action_uniform(word) < a.defect_prob ? 1u : 0u;
    }
  }
  __syncthreads();
  if (t >= nrecv) return;
  // ---- one lane per receiver
  int base = 0, h = t, own = a.hm + t;      // slice: sender at offset o is row own + o
  if (whole) {
    const int e = t / N;
    base = e * N;
    h = t - base;
    own = t;
  }
  const int64_t ag = agent0 + (whole ? t : start + t);
  float4 qr[KQ];
#pragma unroll
  for (int j = 0; j < KQ; ++j)
    if (j < kq) qr[j] = *reinterpret_cast<const float4*>(a.q + ag * a.ldq + 4 * j);
  auto sender_row = [&](int i) { return whole ? base + wrap(h + band_offset(i), N) : own + band_offset(i); };
  float m = score<KQ>(qr, rows + own * a.stride, kq, a.inv_sqrt_k);
  for (int i = 1; i <= a.c; ++i) {
    const int s = sender_row(i);
    if (defects && dead[s]) continue;
    m = fmaxf(m, score<KQ>(qr, rows + s * a.stride, kq, a.inv_sqrt_k));
  }
  float4 acc[VQ];
#pragma unroll
  for (int j = 0; j < VQ; ++j) acc[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float l = 0.0f;
  for (int i = 0; i <= a.c; ++i) {
    const int s = i == 0 ? own : sender_row(i);
    if (i > 0 && defects && dead[s]) continue;
    const float* row = rows + s * a.stride;
    const float p = __expf(score<KQ>(qr, row, kq, a.inv_sqrt_k) - m);
    l += p;
#pragma unroll
    for (int j = 0; j < VQ; ++j)
      if (j < vq) {
        const float4 vv = *reinterpret_cast<const float4*>(row + 4 * (kq + j));
        acc[j].x = fmaf(p, vv.x, acc[j].x);
        acc[j].y = fmaf(p, vv.y, acc[j].y);
        acc[j].z = fmaf(p, vv.z, acc[j].z);
        acc[j].w = fmaf(p, vv.w, acc[j].w);
      }
  }
  const float inv = 1.0f / l;      // l >= 1: the sender holding the maximum contributes exp(0)
  float* dst = a.out + ag * a.ldo;
#pragma unroll
  for (int j = 0; j < VQ; ++j)
    if (j < vq) *reinterpret_cast<float4*>(dst + 4 * j) = make_float4(acc[j].x * inv, acc[j].y * inv, acc[j].z * inv, acc[j].w * inv);
}

__global__ __launch_bounds__(TILE) void k_tarmac_zero(float* out, int64_t ldo, int vq, int64_t chunks) {
  const int64_t idx = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (idx >= chunks) return;
  const int64_t ag = idx / vq;
  const int j = (int)(idx - ag * vq);
  *reinterpret_cast<float4*>(out + ag * ldo + 4 * j) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(TILE) void k_logits_sample(const float* logits, int64_t ld, int64_t A, uint32_t k0, uint32_t k1, uint32_t step_lo,
                                                        uint32_t step_hi, const int32_t* step_dev, int greedy, uint8_t* action, float* a_prob,
                                                        float* probs) {
  const int64_t ag = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (ag >= A) return;
  const float d = logits[ag * ld] - logits[ag * ld + 1];
  const float p0 = 1.0f / (1.0f + expf(-d));
  const float p1 = 1.0f / (1.0f + expf(d));
  int act;
  if (greedy) {
    act = d >= 0.0f ? 0 : 1;      // argmax keeps the first maximum, as torch.argmax
  } else {
    const float u = action_uniform(mdr::action_word(ag, step_lo, step_hi, step_dev, k0, k1));
    act = u < p0 ? 0 : 1;
  }
  action[ag] = (uint8_t)act;
  if (a_prob) a_prob[ag] = act ? p1 : p0;
  if (probs) {
    probs[ag * 2] = p0;
    probs[ag * 2 + 1] = p1;
  }
}

template <typename K>
int launch_comm(K kernel, unsigned grid, size_t lds_bytes, hipStream_t s, const CommArgs& a) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(TILE), lds_bytes, s, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 3) == 0; }

// the by-value entry point (key_dev NULL: the key is `seed`) and the keyed one
int comm(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs, int32_t nb_houses,
         int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob, const int32_t* key_dev, uint64_t seed,
         uint64_t step, const int32_t* step_dev, int32_t hop, float* out, int64_t ldo, void* stream) {
  if (!query || !key || !value || !out || nb_envs < 0 || nb_houses <= 0 || nb_comm < 0) return MDR_ERR_INVALID;
  if (mode != MDR_TARMAC_NEIGHBOURS && mode != MDR_TARMAC_NONE) return MDR_ERR_INVALID;
  if (hop < 0 || hop > 3 || !(defect_prob >= 0.0f && defect_prob <= 1.0f)) return MDR_ERR_INVALID;
  if (num_key <= 0 || num_value <= 0) return MDR_ERR_INVALID;
  if (num_key % 4 || num_key > 32 || num_value % 4 || num_value > 64) return MDR_ERR_UNSUPPORTED;
  if (!aligned16(query, ldq) || !aligned16(key, ldk) || !aligned16(value, ldv) || !aligned16(out, ldo)) return MDR_ERR_INVALID;
  if (ldq < num_key || ldk < num_key || ldv < num_value || ldo < num_value) return MDR_ERR_INVALID;
  const int c = nb_comm < nb_houses - 1 ? nb_comm : nb_houses - 1;      // make_masks 140-141
  if (mode == MDR_TARMAC_NEIGHBOURS && c > MAX_C) return MDR_ERR_UNSUPPORTED;
  if (nb_envs == 0) return MDR_OK;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  hipStream_t s = (hipStream_t)stream;
  if (mode == MDR_TARMAC_NONE) {
    const int64_t chunks = A * (num_value / 4);
    if ((chunks + TILE - 1) / TILE > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_tarmac_zero, dim3((unsigned)((chunks + TILE - 1) / TILE)), dim3(TILE), 0, s, out, ldo, num_value / 4, chunks);
    return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
  }
  CommArgs a{};
  a.q = query, a.k = key, a.v = value, a.out = out;
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo;
  a.E = nb_envs, a.N = nb_houses;
  a.kq = num_key / 4, a.vq = num_value / 4;
  a.c = c, a.hm = c / 2;
  a.epw = nb_houses <= TILE ? TILE / nb_houses : 0;
  a.slices = a.epw ? 0 : (nb_houses + TILE - 1) / TILE;
  const int quads = a.kq + a.vq;
  a.stride = 4 * (quads | 1);      // an odd multiple of 4 floats: no two lanes of a ds_read_b128 group on one bank
  const int max_rows = a.epw ? a.epw * nb_houses : TILE + c;
  a.dead_off = max_rows * a.stride;
  a.inv_sqrt_k = 1.0f / sqrtf((float)num_key);
  a.defect_prob = defect_prob;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.hop = hop;
  a.step_dev = step_dev;
  a.key = key_dev;
  const int64_t grid = a.epw ? ((int64_t)nb_envs + a.epw - 1) / a.epw : (int64_t)nb_envs * a.slices;
  if (grid > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
  const size_t lds_bytes = ((size_t)max_rows * a.stride + (defect_prob > 0.0f ? max_rows : 0)) * sizeof(float);
  if (lds_bytes > 160 * 1024) return MDR_ERR_UNSUPPORTED;
  if (a.kq == 2 && a.vq == 4) return launch_comm(k_tarmac_comm<2, 4, true>, (unsigned)grid, lds_bytes, s, a);      // the reference's sizes
  if (a.kq <= 4 && a.vq <= 8) return launch_comm(k_tarmac_comm<4, 8, false>, (unsigned)grid, lds_bytes, s, a);
  return launch_comm(k_tarmac_comm<8, 16, false>, (unsigned)grid, lds_bytes, s, a);
}

}  // namespace

extern "C" {

int mdr_tarmac_comm(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                    int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob, uint64_t seed,
                    uint64_t step, const int32_t* step_dev, int32_t hop, float* out, int64_t ldo, void* stream) {
  return comm(query, ldq, key, ldk, value, ldv, nb_envs, nb_houses, num_key, num_value, nb_comm, mode, defect_prob, nullptr, seed, step, step_dev,
              hop, out, ldo, stream);
}

int mdr_tarmac_comm_keyed(const float* query, int64_t ldq, const float* key, int64_t ldk, const float* value, int64_t ldv, int32_t nb_envs,
                          int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob,
                          const int32_t* key_dev, uint64_t step, const int32_t* step_dev, int32_t hop, float* out, int64_t ldo, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return comm(query, ldq, key, ldk, value, ldv, nb_envs, nb_houses, num_key, num_value, nb_comm, mode, defect_prob, key_dev, 0, step, step_dev,
              hop, out, ldo, stream);
}

int mdr_logits_sample(const float* logits, int64_t ld, int64_t nb_agents, uint64_t seed, uint64_t step, const int32_t* step_dev,
                      int32_t greedy, uint8_t* action, float* a_prob, float* probs, void* stream) {
  if (!logits || !action || nb_agents < 0 || ld < 2) return MDR_ERR_INVALID;
  if (nb_agents == 0) return MDR_OK;
  if ((nb_agents + TILE - 1) / TILE > 0x7FFFFFFF) return MDR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_logits_sample, dim3((unsigned)((nb_agents + TILE - 1) / TILE)), dim3(TILE), 0, (hipStream_t)stream, logits, ld, nb_agents,
                     (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), step_dev, (int)greedy, action, a_prob, probs);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // extern "C"
