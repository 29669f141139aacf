// What the TarMAC actor's matrix-core kernels share between the exact-fp32 forms (mdr_tarmac_mlp.hip) and the bf16x3 forms
// (mdr_tarmac_mlp_bf16.hip): the limits, the layout of mdr_tarmac_actor_t.vec, the kernel arguments, the activations, the kernels'
// prologue (stage_weights), the head's tail (head_finish), the fragment sizes, the
// persistent-grid launch and the launch chain of a sample (run_chain<Forms>).
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
  // n a multiple of 4, both 16-byte aligned.  The builtin, not blockDim.x: read inside a helper of a helper, the library call behind
  // blockDim is no longer folded to the uniform workgroup size and the stride ends up in a vector register
  const int stride = (int)__builtin_amdgcn_workgroup_size_x() * 4;
  for (int i = tid * 4; i < n; i += stride) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---- what every kernel opens with: the staged weights in LDS, fa | fp | vec, and which tiles the wavefront takes.  The helpers take
// what they need of MlpArgs as values the kernel has read: handed the argument block by reference, the kernel's registers move.
struct Fragments {      // fp == nullptr: no frag_proj in LDS (head)
  const float *fa, *fp, *vec;
  int na, np, nvec;
};

struct Staged {
  float *fa, *fp, *vec;
  int lane0, r;
  int64_t wave, nwaves;
};

struct NoHooks {      // of a kernel or feature source with nothing to do there: no windows before the barrier, no staging between layers
  __device__ __forceinline__ void operator()() const {}
  __device__ __forceinline__ void carve(float*, int) {}
  __device__ __forceinline__ void prime(int64_t, int64_t) {}
  __device__ __forceinline__ void after_layer1() {}
  __device__ __forceinline__ void end() {}
};

// `nw` waves per workgroup; `before_sync()`: what else a kernel leaves in LDS before the barrier (the observe forms' windows)
template <class F = NoHooks>
__device__ __forceinline__ Staged stage_weights(float* lds, const Fragments w, bool stage_fp, int nw, F&& before_sync = F{}) {
  Staged S;
  S.fa = lds;
  S.fp = S.fa + w.na;
  S.vec = S.fp + w.np;
  const int tid = threadIdx.x;
  S.lane0 = tid & 63, S.r = S.lane0 & 15;
  S.wave = (int64_t)blockIdx.x * nw + (tid >> 6), S.nwaves = (int64_t)gridDim.x * nw;      // read ahead of the barrier, not behind it
  stage(S.fa, w.fa, w.na, tid);
  if (stage_fp) stage(S.fp, w.fp, w.np, tid);
  stage(S.vec, w.vec, w.nvec, tid);
  before_sync();
  __syncthreads();
  return S;
}

// ---- the head's tail, on the accumulators acc of comm_hidden2action's first layer that lane group g holds for `agent`: the last
// layer as one dot product with W3[0] - W3[1], the two-logit softmax, the action draw of mdr_logits_sample (mdr_draw.h), the writes
struct DrawArgs {
  uint8_t* action;
  float *a_prob, *probs;
  int greedy;
  uint32_t k0, k1, step_lo, step_hi;
  const int32_t* step_dev;
};

template <int MBH, bool EXACT>
__device__ __forceinline__ void head_finish(const f32x4 (&acc)[MBH], const float* vec, const VecLayout& L, int mbh, int g, float bias3,
                                            const DrawArgs a, int64_t agent, bool valid) {
  float d = 0.0f;
#pragma unroll
  for (int mb = 0; mb < MBH; ++mb)
    if (EXACT || mb < mbh) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(vec + L.wd + 16 * mb + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) d = fmaf(w[i], relu(acc[mb][i]), d);
    }
  d += __shfl_xor(d, 16);
  d += __shfl_xor(d, 32);
  d += bias3;
  const float p0 = 1.0f / (1.0f + expf(-d));      // mdr_logits_sample's softmax over two logits
  const float p1 = 1.0f / (1.0f + expf(d));
  if (g == 0 && valid) {
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

// ---- what the observe source of an encode kernel takes beside MlpArgs, as a second kernel argument (the rows source: none)
struct WindowArgs {
  mdr::ObserveArgs o;
  float* rows_out;
};

// ---- observe -> act (mdr_env_tarmac_actor_sample): the encode kernels' forms that build their features in LDS (mdr_observe.h)
// (the window itself: ObserveWindow and its row stride TARMAC_OBS_ROW, mdr_observe.h)
constexpr size_t LDS_PER_CU = 160 * 1024;

// ---- host: the launches.  Each kernel is a persistent grid: the weights are staged once per workgroup
template <typename K, typename... Extra>
int launch(K kernel, int waves, size_t lds_bytes, const MlpArgs& a, int cus, hipStream_t s, const Extra&... extra) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return MDR_ERR_HIP;
  const int64_t want = (a.ntiles + waves - 1) / waves;
  const unsigned grid = (unsigned)(want < cus ? want : cus);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds_bytes, s, a, extra...);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

inline size_t weights_bytes(const MlpArgs& a, bool proj) { return (size_t)(a.na + (proj ? a.np : 0) + a.nvec) * sizeof(float); }

// LDS: the staged weights, then one window of `tile` rows per wave and, with rows_out, the row table of observe_store_rows.  A form
// whose windows do not fit beside its weights runs with fewer waves per workgroup, whole waves per SIMD.
template <typename K>
int launch_observe(K kernel, int waves, int tile, const MlpArgs& a, const mdr::ObserveArgs& o, float* rows_out, int cus, hipStream_t s) {
  const size_t fixed = weights_bytes(a, true) + (rows_out ? (size_t)tile * 51 * sizeof(uint16_t) : 0);
  const size_t window = (size_t)tile * TARMAC_OBS_ROW * sizeof(float);
  while (waves > 4 && fixed + waves * window > LDS_PER_CU) waves -= 4;
  if (fixed + waves * window > LDS_PER_CU) return MDR_ERR_UNSUPPORTED;
  return launch(kernel, waves, fixed + waves * window, a, cus, s, WindowArgs{o, rows_out});
}

// ---- the fragment sizes (include/mdr_policy.h), in 4-byte words.  fp32: a k-step is 4 inputs, 64 lanes x one float per output block
struct FragFloats {
  static int64_t encode(int F, int H) { return ((int64_t)(F + 3) / 4 + 4 * blocks(H)) * 64 * blocks(H); }
  static int64_t proj(int H, int V) { return (int64_t)4 * blocks(H) * 64 * (3 * blocks(H) + 2 + blocks(V)); }
  static int64_t msg(int H, int V) { return (int64_t)((V + H) / 4) * 64 * blocks(H + V) + (int64_t)4 * blocks(H + V) * 64 * blocks(H); }
  static int64_t head(int H, int V, int with_comm) { return (int64_t)((H + (with_comm ? V : 0)) / 4) * 64 * blocks(H); }
};

// bf16x3: 512 words per (k-step, output block) pair - head and tail, 64 lanes, 8 bf16
constexpr int PAIR_WORDS = 512;
__host__ __device__ inline int ksteps_rows(int n) { return (n + 31) / 32; }      // 32 floats of a row per k-step
__host__ __device__ inline int ksteps_regs(int mbi) { return (mbi + 1) / 2; }     // two blocks of the previous layer per k-step
struct FragWords {
  static int64_t encode(int F, int H) { return (int64_t)PAIR_WORDS * (ksteps_rows(F) + ksteps_regs(blocks(H))) * blocks(H); }
  static int64_t proj(int H, int V) { return (int64_t)PAIR_WORDS * ksteps_regs(blocks(H)) * (3 * blocks(H) + 2 + blocks(V)); }
  static int64_t msg(int H, int V) {
    return (int64_t)PAIR_WORDS * ((ksteps_rows(V) + ksteps_rows(H)) * blocks(H + V) + ksteps_regs(blocks(H + V)) * blocks(H));
  }
  static int64_t head(int H, int V, int with_comm) { return (int64_t)PAIR_WORDS * ksteps_rows(H + (with_comm ? V : 0)) * blocks(H); }
};

using MlpKernel = void (*)(MlpArgs);
using MlpObserveKernel = void (*)(MlpArgs, WindowArgs);

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

namespace {

// The launch chain of a sample, after the argument checks of mdr_tarmac_actor_sample (mdr_tarmac_mlp.hip): 1 + hops + (hops - 1) + 1
// launches.  `o` == nullptr: from the observation rows `obs`; else from the env's compact state (`obs` unused), `rows_out` optional.
// Forms is what a precision brings: TILE agents per wavefront and tile, waves(exact) per workgroup, the fragment sizes encode / proj /
// msg / head in 4-byte words, row_steps(n) k-steps fed from a row of n floats (lane group g holds the features [g S, g S + S) of
// fp32's k-steps), whole_vectors(S, D) - such a row is read as aligned float4s - head_exact(mbh, S), and its kernels.
template <class Forms>
int run_chain(const mdr_tarmac_actor_t* actor, const float* obs, const mdr::ObserveArgs* o, float* rows_out, int32_t nb_envs, int32_t nb_houses,
              uint64_t seed, uint64_t step, const int32_t* step_dev, void* workspace, uint8_t* action, float* a_prob, float* probs, int cus,
              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int F = actor->num_state, H = actor->hidden, K = actor->num_key, V = actor->num_value;
  const int hops = actor->num_hops, wc = actor->with_comm != 0;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  const int mbh = blocks(H), mbv = blocks(V), mbm = blocks(H + V);
  const VecLayout L = vec_layout(mbh, mbv, mbm);
  const bool exact = mbh == 4 && mbv == 1 && (!wc || hops == 1 || mbm == 5);
  const int waves = Forms::waves(exact);
  const int64_t ldcat = wc ? H + V : H, ldqkv = K + K + V;
  float* cat = static_cast<float*>(workspace);
  float* qkv = cat + A * ldcat;
  float* state = qkv + A * ldqkv;

  MlpArgs a{};
  a.vec = actor->vec, a.nvec = L.total;
  a.cat = cat, a.qkv = qkv, a.state = state, a.ldcat = ldcat, a.ldqkv = ldqkv;
  a.action = action, a.a_prob = a_prob, a.probs = probs;
  a.A = A, a.ntiles = (A + Forms::TILE - 1) / Forms::TILE;
  a.H = H, a.K = K, a.V = V, a.mbh = mbh, a.mbv = mbv, a.mbm = mbm;
  a.with_comm = wc, a.greedy = actor->greedy != 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.step_dev = step_dev;
  a.np = wc ? (int)Forms::proj(H, V) : 0;

  // ---- obs -> x (-> qkv)
  a.fa = actor->frag_encode, a.fp = actor->frag_proj, a.na = (int)Forms::encode(F, H);
  a.in0 = obs, a.ld0 = F, a.D0 = F, a.S0 = Forms::row_steps(F);
  a.vec0 = Forms::whole_vectors(a.S0, F) && aligned16(obs);
  int rc;
  if (o)      // the same layers on features built in LDS: whole-tile staging where no tile leaves its env
    rc = launch_observe(Forms::encode_observe_kernel(exact, rows_out != nullptr, o->N % Forms::TILE != 0), waves, Forms::TILE, a, *o,
                        rows_out, cus, s);
  else
    rc = launch(Forms::encode_kernel(exact), waves, weights_bytes(a, true), a, cus, s);
  if (rc != MDR_OK) return rc;
  if (wc) {
    for (int hop = 0; hop < hops; ++hop) {
      if (hop > 0) {      // [comm, h] -> h' -> qkv
        a.fa = actor->frag_msg, a.na = (int)Forms::msg(H, V);
        a.in0 = cat + H, a.ld0 = ldcat, a.D0 = V, a.S0 = Forms::row_steps(V);
        a.in1 = hop == 1 ? cat : state, a.ld1 = hop == 1 ? ldcat : H, a.S1 = Forms::row_steps(H);
        // H, V and both leading dimensions are multiples of 4 floats, the workspace is 16-byte aligned
        a.vec0 = Forms::whole_vectors(a.S0, V), a.vec1 = Forms::whole_vectors(a.S1, H);
        rc = launch(Forms::rehop_kernel(exact), waves, weights_bytes(a, true), a, cus, s);
        if (rc != MDR_OK) return rc;
      }
      rc = mdr_tarmac_comm(qkv, ldqkv, qkv + K, ldqkv, qkv + 2 * K, ldqkv, nb_envs, nb_houses, K, V, actor->nb_comm, actor->mode, actor->defect_prob,
                           seed, step, step_dev, hop, cat + H, ldcat, stream);
      if (rc != MDR_OK) return rc;
    }
  }
  // ---- [x, comm] -> logits -> action
  a.fa = actor->frag_head, a.na = (int)Forms::head(H, V, wc);
  a.in0 = cat, a.ld0 = ldcat, a.D0 = (int)ldcat, a.S0 = Forms::row_steps((int)ldcat);
  a.vec0 = Forms::whole_vectors(a.S0, (int)ldcat);
  const bool head_exact = Forms::head_exact(mbh, a.S0);
  return launch(Forms::head_kernel(head_exact), Forms::waves(head_exact), weights_bytes(a, false), a, cus, s);
}

}  // namespace
