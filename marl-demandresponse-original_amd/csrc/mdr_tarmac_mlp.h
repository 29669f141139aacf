// What the TarMAC actor's matrix-core kernels share between the exact-fp32 forms (mdr_tarmac_mlp.hip) and the bf16x3 forms
// (mdr_tarmac_mlp_bf16.hip): the limits, the layout of mdr_tarmac_actor_t.vec, the kernel arguments, the activations, the LDS staging
// and the persistent-grid launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_device.h"
#include "mdr_draw.h"
#include "mdr_observe.h"

namespace {

using mdr::action_uniform;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVES = 16;        // per workgroup, the forms of the reference's sizes: four per SIMD in 128 registers
constexpr int WAVES_GEN = 8;     // the general forms: two per SIMD in 256 registers
constexpr int MAX_F = 64, MAX_H = 64, MAX_K = 16, MAX_V = 32, MAX_HOPS = 4, MAX_C = 64;

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

__host__ __device__ inline int blocks(int n) { return (n + 15) / 16; }

// Offsets (floats) into mdr_tarmac_actor_t.vec: every bias zero-padded to whole 16-unit blocks, in unit order - lane group g reads
// the four units 16 mb + 4 g + reg of block mb as one float4.
struct VecLayout {
  int o1, o2, p1, q2, k2, v2, m1, m2, h1, wd, b3, total;
};

__host__ __device__ inline VecLayout vec_layout(int mbh, int mbv, int mbm) {
  VecLayout L;
  const int nH = 16 * mbh;
  L.o1 = 0;
  L.o2 = nH;
  L.p1 = 2 * nH;             // query | key | value, first layers
  L.q2 = 5 * nH;
  L.k2 = L.q2 + 16;
  L.v2 = L.k2 + 16;
  L.m1 = L.v2 + 16 * mbv;
  L.m2 = L.m1 + 16 * mbm;
  L.h1 = L.m2 + nH;
  L.wd = L.h1 + nH;          // W3[0] - W3[1]
  L.b3 = L.wd + nH;          // b3[0] - b3[1], 0, 0, 0
  L.total = L.b3 + 4;
  return L;
}

struct MlpArgs {
  const float* fa;        // encode: frag_encode; rehop: frag_msg; head: frag_head
  const float* fp;        // frag_proj
  const float* vec;
  const float* in0;       // encode: obs rows; rehop: the comm columns of cat; head: cat
  const float* in1;       // rehop: h (cat's x columns for the first re-hop, state afterwards)
  int64_t ld0, ld1;
  float* cat;
  float* qkv;
  float* state;
  int64_t ldcat, ldqkv;
  uint8_t* action;
  float* a_prob;
  float* probs;
  int64_t A, ntiles;
  int D0, S0, S1;         // floats per in0 row that are features; k-steps fed from in0 / in1 (lane group g holds features [g S, g S + S))
  int vec0, vec1;         // the group's S features are whole aligned float4s
  int H, K, V;
  int mbh, mbv, mbm;
  int with_comm, greedy;
  int na, np, nvec;       // floats staged from fa / fp / vec
  uint32_t k0, k1, step_lo, step_hi;
  const int32_t* step_dev;
};

__device__ __forceinline__ float relu(float x) {      // mdr_policy.hip: max on the bit pattern, one instruction
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// tanh to a few ulp at every magnitude: 1 - 2 / (exp(2 |x|) + 1) has an ABSOLUTE error of ~1e-7 (the fast exponential's relative
// error |2 x| 2^-24 is damped by 2 e / (e + 1)^2 <= 1 / 2), which near 0 would be a large relative one - there the odd series
// x (1 - x^2 / 3 + 2 x^4 / 15) is used, whose first dropped term 17 x^6 / 315 is below 2^-24 for |x| < 0.1.
__device__ __forceinline__ float tanh_f(float x) {
  const float ax = fabsf(x);
  const float x2 = x * x;
  const float small = x * fmaf(x2, fmaf(x2, 2.0f / 15.0f, -1.0f / 3.0f), 1.0f);
  const float e = __expf(2.0f * ax);                        // inf beyond ~44: 2 / inf = 0, tanh = 1
  const float big = copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f), x);
  return ax < 0.1f ? small : big;
}

template <int ACT>
__device__ __forceinline__ float activate(float x) {
  return ACT == ACT_RELU ? relu(x) : (ACT == ACT_TANH ? tanh_f(x) : x);
}

__device__ __forceinline__ void stage(float* dst, const float* src, int n, int tid) {
  const int stride = (int)blockDim.x * 4;      // n a multiple of 4, both 16-byte aligned
  for (int i = tid * 4; i < n; i += stride) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename K>
int launch(K kernel, int waves, const MlpArgs& a, int lds_floats, int cus, hipStream_t s) {
  const size_t lds_bytes = (size_t)lds_floats * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  const int64_t want = (a.ntiles + waves - 1) / waves;
  const unsigned grid = (unsigned)(want < cus ? want : cus);      // persistent: the weights are staged once per workgroup
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds_bytes, s, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// ---- observe -> act (mdr_env_tarmac_actor_sample): the encode kernels' forms that build their features in LDS (mdr_observe.h)
constexpr int TARMAC_OBS_ROW = 60;      // floats per staged row (k_tarmac_encode_obs says why)
constexpr size_t LDS_PER_CU = 160 * 1024;

// LDS: the staged weights, then one window of `tile` rows per wave and, with rows_out, the row table of observe_store_rows.  A form
// whose windows do not fit beside its weights runs with fewer waves per workgroup, whole waves per SIMD.
template <typename K>
int launch_observe(K kernel, int waves, int tile, const MlpArgs& a, const mdr::ObserveArgs& o, float* rows_out, int cus, hipStream_t s) {
  const size_t fixed = (size_t)(a.na + a.np + a.nvec) * sizeof(float) + (rows_out ? (size_t)tile * 51 * sizeof(uint16_t) : 0);
  const size_t window = (size_t)tile * TARMAC_OBS_ROW * sizeof(float);
  while (waves > 4 && fixed + waves * window > LDS_PER_CU) waves -= 4;
  const size_t lds_bytes = fixed + waves * window;
  if (lds_bytes > LDS_PER_CU) return MDR_ERR_UNSUPPORTED;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  const int64_t want = (a.ntiles + waves - 1) / waves;
  const unsigned grid = (unsigned)(want < cus ? want : cus);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds_bytes, s, a, o, rows_out);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// ---- the bf16x3 fragments (include/mdr_policy.h): 512 4-byte words per (k-step, output block) pair - head and tail, 64 lanes, 8 bf16
constexpr int PAIR_WORDS = 512;
__host__ __device__ inline int ksteps_rows(int n) { return (n + 31) / 32; }      // 32 floats of a row per k-step
__host__ __device__ inline int ksteps_regs(int mbi) { return (mbi + 1) / 2; }     // two blocks of the previous layer per k-step
inline int64_t encode_words(int F, int H) { return (int64_t)PAIR_WORDS * (ksteps_rows(F) + ksteps_regs(blocks(H))) * blocks(H); }
inline int64_t proj_words(int H, int V) { return (int64_t)PAIR_WORDS * ksteps_regs(blocks(H)) * (3 * blocks(H) + 2 + blocks(V)); }
inline int64_t msg_words(int H, int V) {
  return (int64_t)PAIR_WORDS * ((ksteps_rows(V) + ksteps_rows(H)) * blocks(H + V) + ksteps_regs(blocks(H + V)) * blocks(H));
}
inline int64_t head_words(int H, int V, int with_comm) { return (int64_t)PAIR_WORDS * ksteps_rows(H + (with_comm ? V : 0)) * blocks(H); }

}  // namespace

namespace mdr {
// The launch chain of mdr_tarmac_actor_sample for MDR_TARMAC_BF16X3, after that entry point's argument checks (mdr_tarmac_mlp_bf16.hip)
// (`o` != nullptr: the observe form of the encode kernel on the env's compact state instead of `obs`, `rows_out` optional)
int tarmac_sample_bf16(const mdr_tarmac_actor_t* actor, const float* obs, const ObserveArgs* o, float* rows_out, int32_t nb_envs, int32_t nb_houses,
                       uint64_t seed, uint64_t step, const int32_t* step_dev, void* workspace, uint8_t* action, float* a_prob, float* probs, int cus,
                       void* stream);

// What the observe forms cover: the default observation (51 features: ten circular neighbours, no optional column, no link defect)
// of unsharded envs of at least 11 houses whose tiles of `tile` agents fit the staging lanes of a wave
inline bool tarmac_observe_covered(const ObserveArgs& o, int num_state, int tile) {
  if (o.ext || num_state != 51 || o.N < 11 || o.E < 0) return false;
  return o.N % tile == 0 || observe_window_lanes(o.N, 10, tile) <= 64;
}
}  // namespace mdr
