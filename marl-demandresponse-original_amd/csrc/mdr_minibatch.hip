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

}  // namespace

extern "C" {

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
