// Minibatch indices drawn on the device (include/mdr_policy.h: mdr_minibatch_permutation, mdr_minibatch_sample) and the cursor block a
// captured update reads them through (mdr_update_cursor_set / _add).  What keeps PPO's, MAPPO's and DQN's update on the host is
// torch.randperm / torch.randint under a generator seeded per epoch; with the indices a function of (seed, epoch + *cursor, element)
// alone a whole update is a fixed chain of launches, and a replayed graph draws new indices by bumping one device word.
//
// The permutation is a four-round balanced Feistel network over the 2h-bit integers (h = ceil(ceil(log2 n) / 2)) with cycle walking:
// one thread per element, no sort, no scratch.  A thread walks its own cycle of the 2h-bit bijection until it lands below n: the
// domain holds fewer than 4 n values, so the walk is 4 rounds x under 4 visits on average.  The round function is word .x of the
// project's Philox4x32-10; its key may come from the device (the _keyed forms), so the seed need not be baked into a captured node.
// Plain loads and vector stores only; every kernel checks its element index against n before it stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_device.h"

namespace {

using mdr::philox4x32_10;

constexpr int THREADS = 256;

struct DrawArgs {
  int64_t n;                    // elements to write
  int64_t* out;
  const int32_t* cursor_dev;    // may be NULL
  const int32_t* key_dev;       // may be NULL: k0, k1 below
  const int64_t* len_dev;       // sample only; may be NULL: len below
  uint32_t k0, k1, c2, c3;      // key, counter word 2 (epoch / step lo), counter word 3 (tag ^ epoch / step hi)
  uint32_t len;                 // sample only
  int32_t h;                    // permutation only: bits of one half
};

__device__ __forceinline__ void resolve(const DrawArgs& a, uint32_t& k0, uint32_t& k1, uint32_t& c2) {
  k0 = a.key_dev ? (uint32_t)a.key_dev[0] : a.k0;
  k1 = a.key_dev ? (uint32_t)a.key_dev[1] : a.k1;
  c2 = a.c2 + (a.cursor_dev ? (uint32_t)*a.cursor_dev : 0u);
}

__global__ __launch_bounds__(THREADS) void k_minibatch_permutation(const DrawArgs a) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.n) return;
  uint32_t k0, k1, c2;
  resolve(a, k0, k1, c2);
  const int h = a.h;
  const uint32_t mask = (uint32_t)((1ull << h) - 1ull);      // h <= 31
  uint64_t x = (uint64_t)i;
  do {
    uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t f = philox4x32_10(R, r, c2, a.c3, k0, k1).x & mask;
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
    }
    x = ((uint64_t)L << h) | (uint64_t)R;
  } while (x >= (uint64_t)a.n);
  a.out[i] = (int64_t)x;
}

__global__ __launch_bounds__(THREADS) void k_minibatch_sample(const DrawArgs a) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.n) return;
  uint32_t k0, k1, c2;
  resolve(a, k0, k1, c2);
  uint32_t len = a.len;
  if (a.len_dev) {
    const int64_t l = *a.len_dev;
    len = l < 1 ? 1u : (l > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)l);
  }
  const uint32_t word = philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), c2, a.c3, k0, k1).x;
  a.out[i] = mdr::mulhi_pick(word, len);      // < len
}

// Everything MADDPGLearner.draws() returns, in one launch (include/mdr_policy.h: mdr_maddpg_draws).  Thread t < N B (N + 1) draws the
// two gumbel values of noise counter q = t; the first N B threads also walk position t % B of agent t / B's Feistel permutation.
struct MaddpgDrawArgs {
  int64_t batch;                // B
  int64_t rows;                 // N B
  int64_t draws;                // N B (N + 1)
  int64_t* index;               // [N][B]
  float* noise_t;               // [N][B][N][2]
  float* noise_a;               // [N][B][2]
  const int32_t* cursor_dev;    // may be NULL
  const int32_t* key_dev;       // may be NULL: k0, k1 below
  const int64_t* len_dev;       // may be NULL: len below
  int64_t len;
  uint32_t k0, k1, c2, c3_index, c3_noise;
  int32_t nb_agents;            // N
};

__device__ __forceinline__ float gumbel(uint32_t word) {
  return (float)(-log(-log(mdr::u01(word))));      // in double: -log(u) stays in [1.2e-10, 22.9], the value is finite for every word
}

__global__ __launch_bounds__(THREADS) void k_maddpg_draws(const MaddpgDrawArgs a) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= a.draws) return;
  const uint32_t k0 = a.key_dev ? (uint32_t)a.key_dev[0] : a.k0;
  const uint32_t k1 = a.key_dev ? (uint32_t)a.key_dev[1] : a.k1;
  const uint32_t c2 = a.c2 + (a.cursor_dev ? (uint32_t)*a.cursor_dev : 0u);
  const int64_t N = a.nb_agents;
  {
    const mdr::u32x4 w = philox4x32_10((uint32_t)t, (uint32_t)((uint64_t)t >> 32), c2, a.c3_noise, k0, k1);
    const int64_t row = t / (N + 1), k = t - row * (N + 1);      // row = a B + b < N B
    float* dst = k < N ? a.noise_t + (row * N + k) * 2 : a.noise_a + row * 2;
    dst[0] = gumbel(w.x);
    dst[1] = gumbel(w.y);
  }
  if (t >= a.rows) return;
  int64_t len = a.len;
  if (a.len_dev) {
    len = *a.len_dev;
    len = len < 1 ? 1 : (len > (1ll << 62) - 1 ? (1ll << 62) - 1 : len);
  }
  const int b = len > 1 ? 64 - __clzll((unsigned long long)(len - 1)) : 1;      // max(1, ceil(log2 len)) <= 62
  const int h = (b + 1) / 2;                                                     // <= 31
  const uint32_t mask = (uint32_t)((1ull << h) - 1ull);
  const uint32_t agent = (uint32_t)(t / a.batch);
  // a walk that starts below len comes back to its start, so it ends; a start at or beyond len (a device len below the batch) is
  // reduced first - such rows repeat positions, none leaves [0, len)
  uint64_t x = (uint64_t)(t - (int64_t)agent * a.batch);
  if (x >= (uint64_t)len) x %= (uint64_t)len;
  do {
    uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t f = philox4x32_10(R, (agent << 8) | r, c2, a.c3_index, k0, k1).x & mask;
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
    }
    x = ((uint64_t)L << h) | (uint64_t)R;
  } while (x >= (uint64_t)len);
  a.index[t] = (int64_t)x;
}

struct CursorArgs {
  int32_t* dst;
  int32_t count, index;
  int32_t v[4];
};

__global__ void k_cursor_set(const CursorArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int k = 0; k < a.count && k < 4; ++k) a.dst[k] = a.v[k];
}

__global__ void k_cursor_add(const CursorArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  a.dst[a.index] += a.v[0];
}

int permutation(int64_t n, const int32_t* key_dev, uint64_t seed, uint64_t epoch, const int32_t* cursor_dev, int64_t* out, void* stream) {
  if (n < 0 || (n > 0 && !out)) return MDR_ERR_INVALID;
  if (n >= (1ll << 62)) return MDR_ERR_UNSUPPORTED;
  if (n == 0) return MDR_OK;
  int b = 1;
  while (b < 62 && (1ll << b) < n) ++b;      // max(1, ceil(log2 n))
  DrawArgs a{};
  a.n = n, a.out = out, a.cursor_dev = cursor_dev, a.key_dev = key_dev;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFull), a.k1 = (uint32_t)(seed >> 32);
  a.c2 = (uint32_t)(epoch & 0xFFFFFFFFull), a.c3 = MDR_TAG_MINIBATCH ^ (uint32_t)(epoch >> 32);
  a.h = (b + 1) / 2;
  const int64_t blocks = (n + THREADS - 1) / THREADS;
  if (blocks > 0x7FFFFFFFll) return MDR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_minibatch_permutation, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int sample(int64_t nb, const int64_t* len_dev, int64_t len, const int32_t* key_dev, uint64_t seed, uint64_t step, const int32_t* cursor_dev,
           int64_t* out, void* stream) {
  if (nb < 0 || (nb > 0 && !out)) return MDR_ERR_INVALID;
  if (!len_dev && (len < 1 || len > 0xFFFFFFFFll)) return MDR_ERR_INVALID;
  if (nb == 0) return MDR_OK;
  DrawArgs a{};
  a.n = nb, a.out = out, a.cursor_dev = cursor_dev, a.key_dev = key_dev, a.len_dev = len_dev;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFull), a.k1 = (uint32_t)(seed >> 32);
  a.c2 = (uint32_t)(step & 0xFFFFFFFFull), a.c3 = MDR_TAG_REPLAY ^ (uint32_t)(step >> 32);
  a.len = len_dev ? 1u : (uint32_t)len;
  const int64_t blocks = (nb + THREADS - 1) / THREADS;
  if (blocks > 0x7FFFFFFFll) return MDR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_minibatch_sample, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int maddpg_draws(int32_t nb_agents, int64_t batch, const int64_t* len_dev, int64_t len, const int32_t* key_dev, uint64_t seed, uint64_t step,
                 const int32_t* cursor_dev, int64_t* index, float* noise_t, float* noise_a, void* stream) {
  if (nb_agents < 1 || batch < 0) return MDR_ERR_INVALID;
  if (batch > 0 && (!index || !noise_t || !noise_a)) return MDR_ERR_INVALID;
  if (!len_dev && len < 1) return MDR_ERR_INVALID;
  if (nb_agents > MDR_MADDPG_DRAWS_MAX_AGENTS) return MDR_ERR_UNSUPPORTED;
  if (!len_dev && len >= (1ll << 62)) return MDR_ERR_UNSUPPORTED;
  if (!len_dev && batch > len) return MDR_ERR_INVALID;      // no batch distinct positions among len
  if (batch == 0) return MDR_OK;
  const int64_t per_agent = (int64_t)nb_agents * (nb_agents + 1);      // <= 426 x 427
  if (batch > (0x7FFFFFFFll * THREADS) / per_agent) return MDR_ERR_UNSUPPORTED;
  MaddpgDrawArgs a{};
  a.batch = batch, a.rows = batch * nb_agents, a.draws = batch * per_agent;
  a.index = index, a.noise_t = noise_t, a.noise_a = noise_a;
  a.cursor_dev = cursor_dev, a.key_dev = key_dev, a.len_dev = len_dev, a.len = len_dev ? 1 : len;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFull), a.k1 = (uint32_t)(seed >> 32);
  a.c2 = (uint32_t)(step & 0xFFFFFFFFull);
  a.c3_index = MDR_TAG_MADDPG_INDEX ^ (uint32_t)(step >> 32), a.c3_noise = MDR_TAG_MADDPG_NOISE ^ (uint32_t)(step >> 32);
  a.nb_agents = nb_agents;
  const int64_t blocks = (a.draws + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(k_maddpg_draws, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int mdr_maddpg_draws(int32_t nb_agents, int64_t batch, const int64_t* len_dev, int64_t len, uint64_t seed, uint64_t step,
                     const int32_t* cursor_dev, int64_t* index, float* noise_t, float* noise_a, void* stream) {
  return maddpg_draws(nb_agents, batch, len_dev, len, nullptr, seed, step, cursor_dev, index, noise_t, noise_a, stream);
}

int mdr_maddpg_draws_keyed(int32_t nb_agents, int64_t batch, const int64_t* len_dev, int64_t len, const int32_t* key_dev, uint64_t step,
                           const int32_t* cursor_dev, int64_t* index, float* noise_t, float* noise_a, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return maddpg_draws(nb_agents, batch, len_dev, len, key_dev, 0, step, cursor_dev, index, noise_t, noise_a, stream);
}

int mdr_minibatch_permutation(int64_t n, uint64_t seed, uint64_t epoch, const int32_t* cursor_dev, int64_t* out, void* stream) {
  return permutation(n, nullptr, seed, epoch, cursor_dev, out, stream);
}

int mdr_minibatch_permutation_keyed(int64_t n, const int32_t* key_dev, uint64_t epoch, const int32_t* cursor_dev, int64_t* out, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return permutation(n, key_dev, 0, epoch, cursor_dev, out, stream);
}

int mdr_minibatch_sample(int64_t nb, const int64_t* len_dev, int64_t len, uint64_t seed, uint64_t step, const int32_t* cursor_dev, int64_t* out,
                         void* stream) {
  return sample(nb, len_dev, len, nullptr, seed, step, cursor_dev, out, stream);
}

int mdr_minibatch_sample_keyed(int64_t nb, const int64_t* len_dev, int64_t len, const int32_t* key_dev, uint64_t step, const int32_t* cursor_dev,
                               int64_t* out, void* stream) {
  if (!key_dev) return MDR_ERR_INVALID;
  return sample(nb, len_dev, len, key_dev, 0, step, cursor_dev, out, stream);
}

int mdr_update_cursor_set(int32_t* dst, int32_t count, int32_t v0, int32_t v1, int32_t v2, int32_t v3, void* stream) {
  if (!dst || count < 1 || count > 4) return MDR_ERR_INVALID;
  CursorArgs a{};
  a.dst = dst, a.count = count, a.v[0] = v0, a.v[1] = v1, a.v[2] = v2, a.v[3] = v3;
  hipLaunchKernelGGL(k_cursor_set, dim3(1), dim3(1), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int mdr_update_cursor_add(int32_t* dst, int32_t index, int32_t delta, void* stream) {
  if (!dst || index < 0) return MDR_ERR_INVALID;
  CursorArgs a{};
  a.dst = dst, a.index = index, a.v[0] = delta;
  hipLaunchKernelGGL(k_cursor_add, dim3(1), dim3(1), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // extern "C"
