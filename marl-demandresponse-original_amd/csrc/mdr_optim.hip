// The optimiser tail of every learner's update (include/mdr_policy.h: mdr_adam_segments_t, mdr_adam_step): elementwise clamp, norm clip
// (nn.utils.clip_grad_norm_, error_if_nonfinite=False), torch.optim.Adam's step and the target blend of agents/dqn.py:77-82 in ONE launch
// on the flat gradient the gradient kernels leave - or on autograd's own tensors: the kernel works on a table of up to 32 segments
// {param, grad, target, count} passed by value in the kernel arguments, so that parameters, gradients and targets stay where torch holds
// them.  exp_avg / exp_avg_sq are two flat buffers in segment order.
//
// The norm is defined over CHUNKS: 1024 consecutive elements of one live segment (the last chunk of a segment ragged, padded with
// zeros), numbered through the live segments in segment order.  One wave sums one chunk: lane l takes the elements 256 i + 4 l + j
// (i, j = 0..3) in that order as s = fma(g, g, s) from s = 0, the 64 lane sums meet in the xor butterfly 32, 16, .., 1 (every lane
// ends with the same bits: each level adds the same two values in either order), and the chunk sums are added one after the other
// in chunk order from 0.  No floating-point atomics, and nothing in that definition knows the grid or the form:
//
//   one launch    (total floats <= max_fused_floats) every workgroup recomputes all chunk sums from L2 into LDS - wave w the chunks
//                 c = w (mod 4) -, adds them in order and then steps its own chunks.  A network of the reference is 15-33 k floats:
//                 re-reading 60-130 KB per workgroup is cheaper than a second launch.
//   two launches  k_adam_sumsq writes the chunk sums to the workspace (one wave per chunk), k_adam_step<false> adds them in the
//                 same order and steps.
//
// No clip and no norm asked for: the norm pass is skipped, one launch whatever the size.  Stepping is elementwise: workgroup b takes
// the chunks c = b (mod grid), thread t the four elements 4 t .. 4 t + 3 of a chunk - as one 16-byte access per array where the bases
// of param, grad, target and the segment's moments are all 16-byte aligned and the four elements are inside the segment (slices of a
// flat gradient start at arbitrary float offsets: F = 5, H = 7 puts the first bias at float 35), scalar otherwise; both paths run
// the same expression (adam_elem) and give the same bits.  7 floats move per element; what this kernel saves is launches.
// No spin-waits, no signalling between workgroups; the gradient is read, never written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"

namespace {

constexpr int CHUNK = 1024;              // elements per chunk of the norm = elements one workgroup steps at a time
constexpr int THREADS = 256;             // 4 waves
constexpr int MAX_FUSED_CHUNKS = 1024;   // LDS image of the chunk sums in the one-launch form (4 KB)
constexpr int MAX_GRID = 1024;
constexpr int64_t DEFAULT_MAX_FUSED_FLOATS = 70804;      // profiles/optim_step_README.md: the largest measured size at which one launch still won

struct Seg {
  float* p;
  const float* g;      // NULL: a dead segment (no chunks)
  float* t;            // NULL without blend
  int64_t n;
  int64_t moff;        // of the segment's moments in exp_avg / exp_avg_sq
};

struct StepArgs {
  Seg seg[MDR_ADAM_MAX_SEGMENTS];
  int32_t chunk0[MDR_ADAM_MAX_SEGMENTS + 1];      // first chunk of every segment; chunk0[nseg] = nchunks
  int32_t nseg, nchunks;
  float* m;
  float* v;
  const float* partial;      // the chunk sums of k_adam_sumsq (two launches)
  float* norm_out;           // may be NULL
  float b1, omb1, b2, omb2, step_size, bc2_sqrt, eps, max_norm, clamp, tau, omtau;
  int32_t do_norm, do_clip, do_blend;
};

// mdr_adam_step_table (k_adam_step<.., true>): the pair {step_size, bc2_sqrt} number slot + *base_dev of corrections.  A type of its
// own, so that the kernels of mdr_adam_step take the arguments - and compile to the instructions - they always did.
struct TableStepArgs : StepArgs {
  const float* corrections;
  const int32_t* base_dev;      // may be NULL
  int32_t slot;
};

template <bool TABLE>
struct ArgsOf {
  using type = StepArgs;
};
template <>
struct ArgsOf<true> {
  using type = TableStepArgs;
};

// comparisons, not fminf / fmaxf: a NaN stays a NaN (k_grad_reduce_clamped); c = inf clamps nothing
__device__ __forceinline__ float clampf(float g, float c) { return g < -c ? -c : (g > c ? c : g); }

// the sum of the clamped squares of one chunk (n > 0 elements left in the segment from g on), by one wave; every lane returns it
__device__ __forceinline__ float chunk_sumsq(const float* __restrict__ g, int64_t n, float c, int lane, bool vec) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + 4 * lane;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec && idx + 4 <= n) {
      const float4 q = *reinterpret_cast<const float4*>(g + idx);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (idx + j < n) x[j] = g[idx + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y = clampf(x[j], c);
      s = fmaf(y, y, s);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// x[0] + x[1] + ... in that order from 0 (eight loads in flight at a time; the additions stay in order)
__device__ __forceinline__ float ordered_sum(const float* x, int n) {
  float sum = 0.0f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = x[i + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += y[j];
  }
  for (; i < n; ++i) sum += x[i];
  return sum;
}

// one element: clamp -> coef g -> the moments -> the parameter -> the target, as torch.optim.Adam's defaults (no weight decay, no amsgrad)
// TABLE: the two bias corrections are `ss` and `bc` (read from the table), otherwise the kernel arguments'
template <bool TABLE, class Args = StepArgs>
__device__ __forceinline__ void adam_elem(const Args& a, float ss, float bc, float coef, float g, float& p, float& m, float& v, float& t) {
  g = coef * clampf(g, a.clamp);      // coef == 1 without a clip: exact
  m = a.b1 * m + a.omb1 * g;
  v = a.b2 * v + a.omb2 * (g * g);
  if constexpr (TABLE) {
    const float denom = sqrtf(v) / bc + a.eps;
    p = p - ss * (m / denom);
  } else {
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
  }
  t = a.omtau * t + a.tau * p;      // stored only with a blend
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// two launches, the first: chunk c = 4 blockIdx.x + wave -> partial[c]
__global__ __launch_bounds__(THREADS) void k_adam_sumsq(const StepArgs a, float* __restrict__ partial) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + wave;
  if (c >= a.nchunks) return;
  for (int s = 0; s < a.nseg; ++s) {
    const int c0 = a.chunk0[s], c1 = a.chunk0[s + 1];
    if (c < c0 || c >= c1) continue;
    const float* g = a.seg[s].g;
    const int64_t off = (int64_t)(c - c0) * CHUNK;
    const float sum = chunk_sumsq(g + off, a.seg[s].n - off, a.clamp, lane, aligned16(g));
    if (lane == 0) partial[c] = sum;
  }
}

// TABLE: the two bias corrections come from device memory (mdr_adam_step_table) instead of the kernel arguments; nothing else differs
template <bool FUSED, bool TABLE>
__global__ __launch_bounds__(THREADS) void k_adam_step(const typename ArgsOf<TABLE>::type a) {
  __shared__ float csum[FUSED ? MAX_FUSED_CHUNKS : 1];
  const int tid = threadIdx.x;
  float coef = 1.0f;
  if (a.do_norm) {
    float ss;
    if (FUSED) {
      const int wave = tid >> 6, lane = tid & 63;
      for (int s = 0; s < a.nseg; ++s) {
        const int c0 = a.chunk0[s], nck = a.chunk0[s + 1] - c0;
        if (nck == 0) continue;
        const float* g = a.seg[s].g;
        const int64_t n = a.seg[s].n;
        const bool vec = aligned16(g);
        for (int k = (wave - c0) & 3; k < nck; k += 4) {      // the chunks c0 + k = wave (mod 4)
          const int64_t off = (int64_t)k * CHUNK;
          const float sum = chunk_sumsq(g + off, n - off, a.clamp, lane, vec);
          if (lane == 0) csum[c0 + k] = sum;
        }
      }
      __syncthreads();
      ss = ordered_sum(csum, a.nchunks);
    } else {
      ss = ordered_sum(a.partial, a.nchunks);
    }
    const float norm = sqrtf(ss);
    if (a.norm_out && blockIdx.x == 0 && tid == 0) *a.norm_out = norm;
    if (a.do_clip) {
      const float c = a.max_norm / (norm + 1e-6f);
      coef = c > 1.0f ? 1.0f : c;      // a NaN norm gives a NaN coef
    }
  }
  float step_size = 0.0f, bc2_sqrt = 1.0f;      // read below with TABLE only
  if constexpr (TABLE) {
    const int64_t pair = (int64_t)a.slot + (a.base_dev ? (int64_t)*a.base_dev : 0);
    step_size = a.corrections[2 * pair], bc2_sqrt = a.corrections[2 * pair + 1];
  }
  const int grid = (int)gridDim.x, b = (int)blockIdx.x;
  for (int s = 0; s < a.nseg; ++s) {
    const int c0 = a.chunk0[s], nck = a.chunk0[s + 1] - c0;
    if (nck == 0) continue;
    const Seg sg = a.seg[s];
    float* m = a.m + sg.moff;
    float* v = a.v + sg.moff;
    const bool vec = aligned16(sg.p) && aligned16(sg.g) && aligned16(m) && aligned16(v) && (!a.do_blend || aligned16(sg.t));
    int k = (b - c0) % grid;
    if (k < 0) k += grid;
    for (; k < nck; k += grid) {      // the chunks c0 + k = b (mod grid)
      const int64_t i = (int64_t)k * CHUNK + 4 * tid;
      if (i >= sg.n) continue;
      if (vec && i + 4 <= sg.n) {
        const float4 g4 = *reinterpret_cast<const float4*>(sg.g + i);
        float4 p4 = *reinterpret_cast<float4*>(sg.p + i), m4 = *reinterpret_cast<float4*>(m + i), v4 = *reinterpret_cast<float4*>(v + i);
        float4 t4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.do_blend) t4 = *reinterpret_cast<float4*>(sg.t + i);
        adam_elem<TABLE>(a, step_size, bc2_sqrt, coef, g4.x, p4.x, m4.x, v4.x, t4.x);
        adam_elem<TABLE>(a, step_size, bc2_sqrt, coef, g4.y, p4.y, m4.y, v4.y, t4.y);
        adam_elem<TABLE>(a, step_size, bc2_sqrt, coef, g4.z, p4.z, m4.z, v4.z, t4.z);
        adam_elem<TABLE>(a, step_size, bc2_sqrt, coef, g4.w, p4.w, m4.w, v4.w, t4.w);
        *reinterpret_cast<float4*>(sg.p + i) = p4;
        *reinterpret_cast<float4*>(m + i) = m4;
        *reinterpret_cast<float4*>(v + i) = v4;
        if (a.do_blend) *reinterpret_cast<float4*>(sg.t + i) = t4;
      } else {
        for (int j = 0; j < 4 && i + j < sg.n; ++j) {
          float p1 = sg.p[i + j], m1 = m[i + j], v1 = v[i + j], t1 = a.do_blend ? sg.t[i + j] : 0.0f;
          adam_elem<TABLE>(a, step_size, bc2_sqrt, coef, sg.g[i + j], p1, m1, v1, t1);
          sg.p[i + j] = p1, m[i + j] = m1, v[i + j] = v1;
          if (a.do_blend) sg.t[i + j] = t1;
        }
      }
    }
  }
}

// ---- N nets in one step (mdr_adam_nets_bind, mdr_adam_step_nets).  One net's segment records are what StepArgs carries by value -
// 1.5 KB -, so those of N nets live in a device table the caller owns: record `net` is written by k_adam_bind from its kernel
// arguments and read by every later step until an address changes.  The step is the two-launch form with the net as the grid's y:
// chunk sums of all nets into the workspace (net y's at y * stride), then every net adds ITS chunk sums in chunk order, takes its
// own norm and clip and steps its own chunks - chunk_sumsq, ordered_sum and adam_elem as above, hence mdr_adam_step's bits per net.
struct NetRec {
  Seg seg[MDR_ADAM_MAX_SEGMENTS];
  int32_t chunk0[MDR_ADAM_MAX_SEGMENTS + 1];
  int32_t nseg, nchunks;
  float* m;
  float* v;
};
static_assert(sizeof(NetRec) % 8 == 0 && sizeof(NetRec) + 8 <= 4096, "a record travels in the kernel argument block, in 8-byte words");

struct NetsArgs {
  const NetRec* table;
  const float* partial;      // [nets][stride] chunk sums; NULL without a norm
  float* norm_out;           // [nets]; may be NULL
  int32_t stride;            // chunk sums per net the workspace has room for: a net bound with more chunks is left alone
  float b1, omb1, b2, omb2, step_size, bc2_sqrt, eps, max_norm, clamp, tau, omtau;
  int32_t do_norm, do_clip, do_blend;
};

// the record is copied word by word from the argument block's own address (indexing the by-value struct would copy it to private memory)
__global__ __launch_bounds__(THREADS) void k_adam_bind(const NetRec rec, NetRec* dst) {
  const uint64_t* src = (const uint64_t*)__builtin_amdgcn_kernarg_segment_ptr();
  uint64_t* out = reinterpret_cast<uint64_t*>(dst);
  for (int i = threadIdx.x; i < (int)(sizeof(NetRec) / 8); i += THREADS) out[i] = src[i];
}

// chunk c = 4 blockIdx.x + wave, + 4 gridDim.x, ... of net blockIdx.y -> partial[y * stride + c]
__global__ __launch_bounds__(THREADS) void k_adam_sumsq_nets(const NetRec* __restrict__ table, float clamp, float* __restrict__ partial, int32_t stride) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const NetRec& r = table[blockIdx.y];
  const int nchunks = r.nchunks;
  if (nchunks > stride) return;
  for (int c = blockIdx.x * 4 + wave; c < nchunks; c += gridDim.x * 4) {
    for (int s = 0; s < r.nseg; ++s) {
      const int c0 = r.chunk0[s], c1 = r.chunk0[s + 1];
      if (c < c0 || c >= c1) continue;
      const float* g = r.seg[s].g;
      const int64_t off = (int64_t)(c - c0) * CHUNK;
      const float sum = chunk_sumsq(g + off, r.seg[s].n - off, clamp, lane, aligned16(g));
      if (lane == 0) partial[(int64_t)blockIdx.y * stride + c] = sum;
    }
  }
}

__global__ __launch_bounds__(THREADS) void k_adam_step_nets(const NetsArgs a) {
  const int tid = threadIdx.x;
  const NetRec& r = a.table[blockIdx.y];
  const int nchunks = r.nchunks;
  if (nchunks > a.stride) return;
  float coef = 1.0f;
  if (a.do_norm) {
    const float ss = ordered_sum(a.partial + (int64_t)blockIdx.y * a.stride, nchunks);
    const float norm = sqrtf(ss);
    if (a.norm_out && blockIdx.x == 0 && tid == 0) a.norm_out[blockIdx.y] = norm;
    if (a.do_clip) {
      const float c = a.max_norm / (norm + 1e-6f);
      coef = c > 1.0f ? 1.0f : c;
    }
  }
  const int grid = (int)gridDim.x, b = (int)blockIdx.x;
  for (int s = 0; s < r.nseg; ++s) {
    const int c0 = r.chunk0[s], nck = r.chunk0[s + 1] - c0;
    if (nck == 0) continue;
    const Seg sg = r.seg[s];
    float* m = r.m + sg.moff;
    float* v = r.v + sg.moff;
    const bool blend = a.do_blend && sg.t;      // a net bound without targets takes no blend
    const bool vec = aligned16(sg.p) && aligned16(sg.g) && aligned16(m) && aligned16(v) && (!blend || aligned16(sg.t));
    int k = (b - c0) % grid;
    if (k < 0) k += grid;
    for (; k < nck; k += grid) {      // the chunks c0 + k = b (mod grid)
      const int64_t i = (int64_t)k * CHUNK + 4 * tid;
      if (i >= sg.n) continue;
      if (vec && i + 4 <= sg.n) {
        const float4 g4 = *reinterpret_cast<const float4*>(sg.g + i);
        float4 p4 = *reinterpret_cast<float4*>(sg.p + i), m4 = *reinterpret_cast<float4*>(m + i), v4 = *reinterpret_cast<float4*>(v + i);
        float4 t4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (blend) t4 = *reinterpret_cast<float4*>(sg.t + i);
        adam_elem<false>(a, 0.0f, 1.0f, coef, g4.x, p4.x, m4.x, v4.x, t4.x);
        adam_elem<false>(a, 0.0f, 1.0f, coef, g4.y, p4.y, m4.y, v4.y, t4.y);
        adam_elem<false>(a, 0.0f, 1.0f, coef, g4.z, p4.z, m4.z, v4.z, t4.z);
        adam_elem<false>(a, 0.0f, 1.0f, coef, g4.w, p4.w, m4.w, v4.w, t4.w);
        *reinterpret_cast<float4*>(sg.p + i) = p4;
        *reinterpret_cast<float4*>(m + i) = m4;
        *reinterpret_cast<float4*>(v + i) = v4;
        if (blend) *reinterpret_cast<float4*>(sg.t + i) = t4;
      } else {
        for (int j = 0; j < 4 && i + j < sg.n; ++j) {
          float p1 = sg.p[i + j], m1 = m[i + j], v1 = v[i + j], t1 = blend ? sg.t[i + j] : 0.0f;
          adam_elem<false>(a, 0.0f, 1.0f, coef, sg.g[i + j], p1, m1, v1, t1);
          sg.p[i + j] = p1, m[i + j] = m1, v[i + j] = v1;
          if (blend) sg.t[i + j] = t1;
        }
      }
    }
  }
}

// the two bias corrections of one step: formed in double, one cast to float (mdr_adam_step and mdr_adam_corrections share them)
float step_size_of(double lr, double beta1, int64_t step) { return (float)(lr / (1.0 - std::pow(beta1, (double)step))); }
float bc2_sqrt_of(double beta2, int64_t step) { return (float)std::sqrt(1.0 - std::pow(beta2, (double)step)); }

int64_t workspace_bytes(int64_t total_floats) {
  // chunks <= sum over the segments of ceil(count / CHUNK) <= total / CHUNK + segments
  return ((total_floats / CHUNK + MDR_ADAM_MAX_SEGMENTS) * (int64_t)sizeof(float) + 15) & ~(int64_t)15;
}

}  // namespace

extern "C" {

int64_t mdr_adam_workspace_bytes(int64_t total_floats) { return total_floats < 0 ? -1 : workspace_bytes(total_floats); }

}  // extern "C"

namespace {

// mdr_adam_step (corrections NULL: the bias corrections of `step` as kernel arguments) and mdr_adam_step_table (from device memory)
int adam_step(const mdr_adam_segments_t* segments, float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
              int64_t step, const float* corrections, int32_t slot, const int32_t* base_dev, double max_grad_norm, double grad_clamp, double tau,
              void* workspace, float* total_norm_out, int32_t max_fused_floats, void* stream) {
  const bool table = corrections != nullptr;
  if (!segments || segments->struct_size != sizeof(mdr_adam_segments_t) || !exp_avg || !exp_avg_sq) return MDR_ERR_INVALID;
  if (segments->nb_segments < 0) return MDR_ERR_INVALID;
  if (segments->nb_segments > MDR_ADAM_MAX_SEGMENTS) return MDR_ERR_UNSUPPORTED;
  if (step < 1 || max_fused_floats < 0) return MDR_ERR_INVALID;
  if (!(lr == lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(tau <= 1.0)) return MDR_ERR_INVALID;
  if (grad_clamp != grad_clamp || grad_clamp <= 0.0) return MDR_ERR_INVALID;      // INFINITY: no clamp
  const bool blend = tau > 0.0;
  const bool clip = max_grad_norm > 0.0 && !std::isinf(max_grad_norm);      // <= 0, inf or NaN: no clip
  TableStepArgs a{};
  int64_t total = 0, chunks = 0;
  for (int s = 0; s < segments->nb_segments; ++s) {
    const mdr_adam_segment_t& in = segments->seg[s];
    if (!in.param || in.count < 0) return MDR_ERR_INVALID;
    if (blend && in.grad && !in.target) return MDR_ERR_INVALID;
    a.seg[s] = Seg{in.param, in.grad, blend ? in.target : nullptr, in.count, total};
    a.chunk0[s] = (int32_t)chunks;
    if (in.grad) chunks += (in.count + CHUNK - 1) / CHUNK;
    total += in.count;
    if (chunks > INT32_MAX / 2) return MDR_ERR_UNSUPPORTED;
  }
  a.nseg = segments->nb_segments, a.nchunks = (int32_t)chunks;
  a.chunk0[a.nseg] = a.nchunks;
  if (chunks == 0 && !total_norm_out) return MDR_OK;
  a.m = exp_avg, a.v = exp_avg_sq, a.norm_out = total_norm_out;
  a.b1 = (float)beta1, a.omb1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.omb2 = (float)(1.0 - beta2);
  a.step_size = table ? 0.0f : step_size_of(lr, beta1, step);
  a.bc2_sqrt = table ? 1.0f : bc2_sqrt_of(beta2, step);
  a.corrections = corrections, a.base_dev = base_dev, a.slot = slot;
  a.eps = (float)eps, a.max_norm = (float)max_grad_norm, a.clamp = (float)grad_clamp;
  a.tau = blend ? (float)tau : 0.0f, a.omtau = blend ? (float)(1.0 - tau) : 0.0f;
  a.do_clip = clip, a.do_norm = clip || total_norm_out != nullptr, a.do_blend = blend;
  hipStream_t st = (hipStream_t)stream;
  const int64_t limit = max_fused_floats == 0 ? DEFAULT_MAX_FUSED_FLOATS : (int64_t)max_fused_floats;
  const bool fused = !a.do_norm || (total <= limit && chunks <= MAX_FUSED_CHUNKS);
  const unsigned grid = (unsigned)(chunks < 1 ? 1 : (chunks > MAX_GRID ? MAX_GRID : chunks));
  if (fused) {
    if (table)
      hipLaunchKernelGGL((k_adam_step<true, true>), dim3(grid), dim3(THREADS), 0, st, a);
    else
      hipLaunchKernelGGL((k_adam_step<true, false>), dim3(grid), dim3(THREADS), 0, st, static_cast<const StepArgs&>(a));
  } else {
    if (!workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
    a.partial = static_cast<const float*>(workspace);
    hipLaunchKernelGGL(k_adam_sumsq, dim3((unsigned)((chunks + 3) / 4)), dim3(THREADS), 0, st, static_cast<const StepArgs&>(a), static_cast<float*>(workspace));
    if (table)
      hipLaunchKernelGGL((k_adam_step<false, true>), dim3(grid), dim3(THREADS), 0, st, a);
    else
      hipLaunchKernelGGL((k_adam_step<false, false>), dim3(grid), dim3(THREADS), 0, st, static_cast<const StepArgs&>(a));
  }
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int mdr_adam_step(const mdr_adam_segments_t* segments, float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                  int64_t step, double max_grad_norm, double grad_clamp, double tau, void* workspace, float* total_norm_out,
                  int32_t max_fused_floats, void* stream) {
  return adam_step(segments, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, nullptr, 0, nullptr, max_grad_norm, grad_clamp, tau, workspace,
                   total_norm_out, max_fused_floats, stream);
}

int mdr_adam_step_table(const mdr_adam_segments_t* segments, float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                        const float* corrections, int32_t slot, const int32_t* base_dev, double max_grad_norm, double grad_clamp, double tau,
                        void* workspace, float* total_norm_out, int32_t max_fused_floats, void* stream) {
  if (!corrections || slot < 0) return MDR_ERR_INVALID;
  return adam_step(segments, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, 1, corrections, slot, base_dev, max_grad_norm, grad_clamp, tau,
                   workspace, total_norm_out, max_fused_floats, stream);
}

int64_t mdr_adam_nets_table_bytes(int32_t nb_nets) { return nb_nets < 0 ? -1 : (int64_t)nb_nets * (int64_t)sizeof(NetRec); }

int mdr_adam_nets_bind(void* table, int32_t net, const mdr_adam_segments_t* segments, float* exp_avg, float* exp_avg_sq, void* stream) {
  if (!table || ((uintptr_t)table & 15u) || net < 0) return MDR_ERR_INVALID;
  if (!segments || segments->struct_size != sizeof(mdr_adam_segments_t) || !exp_avg || !exp_avg_sq) return MDR_ERR_INVALID;
  if (segments->nb_segments < 0) return MDR_ERR_INVALID;
  if (segments->nb_segments > MDR_ADAM_MAX_SEGMENTS) return MDR_ERR_UNSUPPORTED;
  NetRec rec{};
  int64_t total = 0, chunks = 0;
  for (int s = 0; s < segments->nb_segments; ++s) {      // mdr_adam_step's own table: the same chunks, the same moment offsets
    const mdr_adam_segment_t& in = segments->seg[s];
    if (!in.param || in.count < 0) return MDR_ERR_INVALID;
    rec.seg[s] = Seg{in.param, in.grad, in.target, in.count, total};
    rec.chunk0[s] = (int32_t)chunks;
    if (in.grad) chunks += (in.count + CHUNK - 1) / CHUNK;
    total += in.count;
    if (chunks > INT32_MAX / 2) return MDR_ERR_UNSUPPORTED;
  }
  rec.nseg = segments->nb_segments, rec.nchunks = (int32_t)chunks;
  rec.chunk0[rec.nseg] = rec.nchunks;
  rec.m = exp_avg, rec.v = exp_avg_sq;
  hipLaunchKernelGGL(k_adam_bind, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, rec, static_cast<NetRec*>(table) + net);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int mdr_adam_step_nets(const void* table, int32_t nb_nets, int64_t max_net_floats, double lr, double beta1, double beta2, double eps, int64_t step,
                       double max_grad_norm, double grad_clamp, double tau, void* workspace, float* total_norm_out, void* stream) {
  if (!table || nb_nets < 0 || max_net_floats < 0 || step < 1) return MDR_ERR_INVALID;
  if (!(lr == lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(tau <= 1.0)) return MDR_ERR_INVALID;
  if (grad_clamp != grad_clamp || grad_clamp <= 0.0) return MDR_ERR_INVALID;
  const int64_t stride = workspace_bytes(max_net_floats) / (int64_t)sizeof(float);
  if (stride > INT32_MAX / 2) return MDR_ERR_UNSUPPORTED;
  if (nb_nets == 0) return MDR_OK;
  const bool blend = tau > 0.0;
  const bool clip = max_grad_norm > 0.0 && !std::isinf(max_grad_norm);
  NetsArgs a{};
  a.table = static_cast<const NetRec*>(table), a.norm_out = total_norm_out, a.stride = (int32_t)stride;
  a.b1 = (float)beta1, a.omb1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.omb2 = (float)(1.0 - beta2);
  a.step_size = step_size_of(lr, beta1, step), a.bc2_sqrt = bc2_sqrt_of(beta2, step);
  a.eps = (float)eps, a.max_norm = (float)max_grad_norm, a.clamp = (float)grad_clamp;
  a.tau = blend ? (float)tau : 0.0f, a.omtau = blend ? (float)(1.0 - tau) : 0.0f;
  a.do_clip = clip, a.do_norm = clip || total_norm_out != nullptr, a.do_blend = blend;
  hipStream_t st = (hipStream_t)stream;
  // a net of max_net_floats has at most `stride` chunks: one workgroup per chunk of the largest net, as mdr_adam_step launches
  const int64_t most = max_net_floats / CHUNK + MDR_ADAM_MAX_SEGMENTS;
  const unsigned grid = (unsigned)(most > MAX_GRID ? MAX_GRID : most);
  if (a.do_norm) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
    a.partial = static_cast<const float*>(workspace);
    hipLaunchKernelGGL(k_adam_sumsq_nets, dim3((grid + 3) / 4, (unsigned)nb_nets), dim3(THREADS), 0, st, a.table, a.clamp, static_cast<float*>(workspace),
                       a.stride);
  }
  hipLaunchKernelGGL(k_adam_step_nets, dim3(grid, (unsigned)nb_nets), dim3(THREADS), 0, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int mdr_adam_corrections(double lr, double beta1, double beta2, int64_t first_step, int64_t count, float* out_host_floats) {
  if (!out_host_floats || first_step < 1 || count < 0) return MDR_ERR_INVALID;
  if (!(lr == lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return MDR_ERR_INVALID;
  for (int64_t k = 0; k < count; ++k) {
    out_host_floats[2 * k] = step_size_of(lr, beta1, first_step + k);
    out_host_floats[2 * k + 1] = bc2_sqrt_of(beta2, first_step + k);
  }
  return MDR_OK;
}

}  // extern "C"
