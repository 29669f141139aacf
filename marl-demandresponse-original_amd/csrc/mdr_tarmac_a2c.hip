// TarMAC A2C (include/mdr_policy.h: mdr_tarmac_a2c_forward, mdr_tarmac_a2c_comm, mdr_tarmac_a2c_grad): the act step and the update
// step of the reference's train_tarmac.py - MultiAgentPolicy (agents/tarmac/model.py:132-266) under A2C_ACKTR.update_multi_agent
// (agents/tarmac/a2c_acktr.py:59-107) - with the weights streamed from L2 (the helpers of csrc/mdr_stream_mlp.h).
//
// One env-step b of N agents, row r = b N + n, input [obs | comm_in] of F + C columns from two buffers (never concatenated in HBM):
//   h1 = leaky(W1 in + b1);  x = W2 h1 + b2;  logits = Wd x (no bias);
//   xbar_b = (sum_n x_bn in agent order) / N;  m = Wc1 xbar + bc1;  a = leaky(m);  V_b = Wc2 a + bc2        (one value per env-step)
//   q, k = Wq x + bq, Wk x + bk;  v = Wv x + bv;  attn_ij = softmax_j(q_i k_j / sqrt(C)) over ALL agents j of the env, j = i included;
//   comm_out = attn v.
// The update of B env-steps (count = B N):  delta_bn = ret_bn - V_b;  with d = l_taken - l_other, t = exp(-|d|):
//   p_taken, p_other = 1 / (1 + t) and t / (1 + t) (which is which by the sign of d);  -log p_taken = softplus(-d) = max(-d, 0) + log1p(t);
//   H = p_taken softplus(-d) + p_other softplus(d);
//   value_loss = sum delta^2 / count;  action_loss = -sum delta log p_taken / count;  entropy = sum H / count;
//   loss = value_coef value_loss + action_loss - entropy_coef entropy  (delta detached in the action loss).
//   d loss / d l_taken = g = inv p_other (entropy_coef p_taken d - delta), d loss / d l_other = -g  (dH / dl_k = -p_k (log p_k + H) and
//   log p_taken + H = p_other d), inv = the fp32 value of 1 / count;  dV_b = cv (sum_n delta_bn in agent order), cv = the fp32 value of
//   -2 value_coef / count;  da = (dV Wc2) leaky'(m);  dxbar = Wc1^T da;  dx_bn = Wd^T dlogits_bn + dxbar_b / N;  dz1 = leaky'(h1) W2^T dx.
// leaky'(z) = 1 for z > 0 and 0.01 otherwise (torch's rule); the sign of the activation carries it.
//
// Four launches:
//   row pass      a workgroup of 8 waves per tile of 16 rows, wave w owning the 16-unit block w of both layers; the tile's input is
//                 staged from `obs` and `comm_in` into one LDS image.  Every contraction of a row runs inside ONE wave on one
//                 accumulator in ascending steps of four k: a row's bits depend neither on the tile nor on the grid.
//   env-step pass a workgroup per env-step: xbar, the critic, the heads of its N agents, the three loss terms (agent order), dV, da, dxbar / N.
//   row backward  dx and dz1 of a tile.
//   weight pass   one wave per 16 x 16 block of a weight gradient, summed over the rows in row order on the MFMA; the blocks of
//                 column 0 take the bias; one more wave sums the loss terms over the env-steps (64 strided sums added in lane order).
// No floating-point atomics, no partials whose order depends on the grid.  Rows past the batch are stored as exact zeros.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_stream_mlp.h"

namespace {

using namespace mdr_stream;

constexpr int NW = 8;                 // waves per row-pass workgroup: one per 16-unit block of S <= 128
constexpr int TILE = 16;
constexpr int MAX_S = 128, MAX_F = 128, MAX_C = 32, MAX_K = 16, MAX_N = 64;
constexpr int MAX_IN = MAX_F + MAX_C;
constexpr int UNR = 8;
constexpr int WW = 4;                 // waves per weight-pass workgroup
constexpr int UNR_W = 8;
constexpr int ST = 256;               // threads of an env-step workgroup
constexpr int CT = 256;               // threads of an attention workgroup
constexpr float SLOPE = 0.01f;

__device__ __forceinline__ float leaky(float z) { return z > 0.0f ? z : SLOPE * z; }

// a block's values into the LDS image and, where asked, the rows of `out` (row stride ld, units below lim)
__device__ __forceinline__ void put_block(const f32x4& v, float* imgT, float* out, int64_t ld, int lim, int64_t row, int u0, int c, int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) imgT[(u0 + 4 * g + i) * LT + c] = v[i];
  if (out && u0 + 4 * g < lim) *reinterpret_cast<f32x4*>(out + row * ld + u0 + 4 * g) = v;      // lim, ld multiples of 4
}

struct Net {
  const float *w1, *b1, *w2, *b2, *wc1, *bc1, *wc2, *bc2, *wq, *bq, *wk, *bk, *wv, *bv, *wd;
  int F, C, S, K;
};

struct RowArgs {
  Net n;
  const float *obs, *comm;
  int64_t ld_obs, ld_comm;
  const int64_t* index;
  int64_t R, ntiles;       // rows B N, tiles of 16
  int N;
  float *h1, *x;           // h1 [Rp][Sp] or null; x [.][ldx]
  int64_t ldx;
  int xlim, xpad, lpad;    // xpad, lpad: x, logits have rows up to the tile's end (the workspace)
  float* logits;           // [R][2]
};

// ---- the row pass: h1, x and the logits of tiles of 16 rows
__global__ __launch_bounds__(64 * NW) void k_a2c_rows(RowArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[(MAX_IN + 2 * MAX_S) * LT];
  float* inT = lds;
  float* h1T = lds + MAX_IN * LT;
  float* xT = h1T + MAX_S * LT;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int F = a.n.F, Cc = a.n.C, S = a.n.S, KIN = F + Cc, KP = (KIN + 3) & ~3, Sp = 16 * blocks16(S);
  const int nbS = blocks16(S);
  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t row = t * TILE + c;
    const bool valid = row < a.R;
    __syncthreads();      // the tile before is read
    for (int e = tid; e < TILE * KP; e += 64 * NW) {
      const int f = e % KP, rr = e / KP;
      const int64_t r = t * TILE + rr;
      float v = 0.0f;
      if (r < a.R && f < KIN) {
        const int64_t b = r / a.N, nn = r - b * a.N;
        const int64_t src = (a.index ? a.index[b] : b) * a.N + nn;
        v = f < F ? a.obs[src * a.ld_obs + f] : a.comm[src * a.ld_comm + (f - F)];
      }
      inT[f * LT + rr] = v;
    }
    __syncthreads();
    if (w < nbS) {
      f32x4 acc = bias_block(a.n.b1, S, 16 * w, g);
      fwd_accum<UNR>(acc, a.n.w1, KIN, S, 16 * w, 0, KIN, inT, c, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = valid ? leaky(acc[i]) : 0.0f;
      put_block(acc, h1T, a.h1, Sp, Sp, row, 16 * w, c, g);
    }
    __syncthreads();
    if (w < nbS) {
      f32x4 z = bias_block(a.n.b2, S, 16 * w, g);
      fwd_accum<UNR>(z, a.n.w2, S, S, 16 * w, 0, S, h1T, c, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = valid ? z[i] : 0.0f;
      // x past R lies inside the padded workspace only: a caller's x [R][S] is written for valid rows alone
      put_block(z, xT, (valid || a.xpad) ? a.x : nullptr, a.ldx, a.xlim, row, 16 * w, c, g);
    }
    __syncthreads();
    if (w == 0) {      // the two logits: units 0 and 1 of one block, no bias
      f32x4 l = {0, 0, 0, 0};
      fwd_accum<UNR>(l, a.n.wd, S, 2, 0, 0, S, xT, c, g);
      if (g == 0 && (valid || a.lpad)) {      // past R: exact zeros, inside the workspace only
        a.logits[2 * row] = l[0];
        a.logits[2 * row + 1] = l[1];
      }
    }
  }
}

struct StepArgs {
  Net n;
  const float* x;          // [.][ldx]
  int64_t ldx;
  const float* logits;     // [R][2]
  const int64_t* action;   // whole buffer, rows j N + n
  const float* ret;
  const int64_t* index;
  int64_t B, Bp, R, Rp;
  int N;
  float inv, cv, ec;       // 1 / (B N), -2 value_coef / (B N), entropy_coef
  float *value, *advantage;
  float *dl;               // [Rp][2]
  float *xbar, *act, *da, *dxm;      // [Bp][Sp]
  float *dv;               // [Bp]
  float *terms;            // [Bp][4]: sum_n delta^2, sum_n delta log p, sum_n H, 0
};

__device__ __forceinline__ float wave_sum(float p) {      // a fixed tree over the 64 lanes
  p += __shfl_xor(p, 32);
  p += __shfl_xor(p, 16);
  p += __shfl_xor(p, 8);
  p += __shfl_xor(p, 4);
  p += __shfl_xor(p, 2);
  p += __shfl_xor(p, 1);
  return p;
}

// ---- the env-step pass
template <bool GRAD>
__global__ __launch_bounds__(ST) void k_a2c_steps(StepArgs a) {
  __shared__ float sx[MAX_S], sa[MAX_S], sda[MAX_S], sd[MAX_N], sq[MAX_N], sl[MAX_N], sh[MAX_N], sdv;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int S = a.n.S, Sp = 16 * blocks16(S), N = a.N;
  const float fN = (float)N;
  const int64_t end = GRAD ? a.Bp : a.B;
  for (int64_t b = blockIdx.x; b < end; b += gridDim.x) {
    __syncthreads();      // the env-step before is read
    if (b >= a.B) {       // GRAD: the padding rows of the weight pass hold zeros
      if (tid < Sp) a.xbar[b * Sp + tid] = 0.0f, a.act[b * Sp + tid] = 0.0f, a.da[b * Sp + tid] = 0.0f, a.dxm[b * Sp + tid] = 0.0f;
      if (tid < 4) a.terms[4 * b + tid] = 0.0f;
      if (tid == 0) a.dv[b] = 0.0f;
      continue;
    }
    if (tid < MAX_S) {
      float xb = 0.0f;
      if (tid < S) {
        float sum = 0.0f;
        for (int n = 0; n < N; ++n) sum += a.x[(b * N + n) * a.ldx + tid];
        xb = sum / fN;
      }
      sx[tid] = xb;
      sa[tid] = 0.0f;
      if (GRAD && tid < Sp) a.xbar[b * Sp + tid] = xb;
    }
    __syncthreads();
    for (int u = w; u < S; u += ST / 64) {
      float p = lane < S ? a.n.wc1[u * S + lane] * sx[lane] : 0.0f;
      if (lane + 64 < S) p = fmaf(a.n.wc1[u * S + lane + 64], sx[lane + 64], p);
      p = wave_sum(p);
      if (lane == 0) sa[u] = leaky(p + a.n.bc1[u]);
    }
    __syncthreads();
    float p = lane < S ? a.n.wc2[lane] * sa[lane] : 0.0f;
    if (lane + 64 < S) p = fmaf(a.n.wc2[lane + 64], sa[lane + 64], p);
    const float V = wave_sum(p) + a.n.bc2[0];      // every wave holds it
    if (tid == 0 && a.value) a.value[b] = V;
    if constexpr (!GRAD) continue;
    if (tid < N) {
      const int64_t r = b * N + tid, src = (a.index ? a.index[b] : b) * N + tid;
      const float l0 = a.logits[2 * r], l1 = a.logits[2 * r + 1];
      const int taken = a.action[src] != 0;
      const float delta = a.ret[src] - V;
      if (a.advantage) a.advantage[r] = delta;
      const float d = taken ? l1 - l0 : l0 - l1;
      const float t = expf(-fabsf(d)), den = 1.0f + t, big = 1.0f / den, small = t / den, lse = log1pf(t);
      const float pa = d >= 0.0f ? big : small, po = d >= 0.0f ? small : big;
      const float spn = fmaxf(-d, 0.0f) + lse, spp = fmaxf(d, 0.0f) + lse;      // -log p_taken, -log p_other
      const float hn = pa * spn, ho = po * spp;
      sd[tid] = delta;
      sq[tid] = delta * delta;
      sl[tid] = delta * spn;            // -delta log p_taken
      sh[tid] = hn + ho;
      const float e1 = a.ec * pa;
      const float e2 = e1 * d;
      const float e3 = e2 - delta;
      const float e4 = po * e3;
      const float gl = a.inv * e4;
      a.dl[2 * r + taken] = gl;
      a.dl[2 * r + 1 - taken] = -gl;
    }
    if (b == a.B - 1 && tid < a.Rp - a.R) {      // the rows past the batch
      a.dl[2 * (a.R + tid)] = 0.0f;
      a.dl[2 * (a.R + tid) + 1] = 0.0f;
    }
    __syncthreads();
    if (tid == 0) {      // the env-step's sums in agent order
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
      for (int n = 0; n < N; ++n) s0 += sd[n], s1 += sq[n], s2 += sl[n], s3 += sh[n];
      const float dV = a.cv * s0;
      sdv = dV;
      a.dv[b] = dV;
      a.terms[4 * b] = s1, a.terms[4 * b + 1] = s2, a.terms[4 * b + 2] = s3, a.terms[4 * b + 3] = 0.0f;
    }
    __syncthreads();
    if (tid < Sp) {
      float v = 0.0f, av = 0.0f;
      if (tid < S) {
        av = sa[tid];
        const float t = sdv * a.n.wc2[tid];
        v = av > 0.0f ? t : SLOPE * t;
      }
      sda[tid] = v;
      a.da[b * Sp + tid] = v;
      a.act[b * Sp + tid] = av;
    }
    __syncthreads();
    if (tid < Sp) {
      float q = 0.0f;
      if (tid < S) {
        float acc = 0.0f;
        for (int u = 0; u < S; ++u) acc = fmaf(a.n.wc1[u * S + tid], sda[u], acc);
        q = acc / fN;
      }
      a.dxm[b * Sp + tid] = q;
    }
  }
}

struct BackArgs {
  Net n;
  int64_t R, ntiles;
  int N;
  const float *h1, *dl, *dxm;
  float *dx, *dz1;         // [Rp][Sp]
};

// dzin[k0 + 4 g + i][row c] = leaky'(hin) sum_{u < Hout} W[u][k0 + m] dzout[u][row], in place of hin's image (bwd_block's loop)
__device__ __forceinline__ void bwd_block_leaky(const float* __restrict__ W, int Hout, int Hin, int k0, const float* dzoutT, float* hinT, float* ws,
                                                int Hp, int64_t row, int c, int g) {
  f32x4 acc = {0, 0, 0, 0};
  const int kc = k0 + c;
  const bool kok = kc < Hin;
  const float* wc = W + (kok ? kc : 0);
  const int ks = 4 * blocks16(Hout);
  for (int q0 = 0; q0 < ks; q0 += UNR) {
    float av[UNR];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int u = 4 * (q0 + i) + g;
      av[i] = (kok && u < Hout) ? wc[(int64_t)u * Hin] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
      if (q0 + i < ks) acc = mfma(av[i], dzoutT[(4 * (q0 + i) + g) * LT + c], acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = hinT[(k0 + 4 * g + i) * LT + c] > 0.0f ? acc[i] : SLOPE * acc[i];
  store_block(acc, hinT, ws, Hp, row, k0, c, g);
}

// ---- the row pass backward: dx and dz1 of tiles of 16 rows
__global__ __launch_bounds__(64 * NW) void k_a2c_rows_bwd(BackArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * MAX_S * LT];
  float* h1T = lds;
  float* dxT = lds + MAX_S * LT;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int S = a.n.S, Sp = 16 * blocks16(S), nbS = blocks16(S);
  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t row = t * TILE + c;      // < Rp: h1's rows past R hold zeros
    const bool valid = row < a.R;
    __syncthreads();
    for (int e = tid; e < TILE * Sp; e += 64 * NW) {
      const int u = e % Sp, rr = e / Sp;
      h1T[u * LT + rr] = a.h1[(t * TILE + rr) * Sp + u];
    }
    if (w < nbS) {
      f32x4 v = {0, 0, 0, 0};
      if (valid) {
        const float dl0 = a.dl[2 * row], dl1 = a.dl[2 * row + 1];
        const int64_t b = row / a.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = 16 * w + 4 * g + i;
          if (s < S) {
            float y = a.n.wd[s] * dl0;
            y = fmaf(a.n.wd[S + s], dl1, y);
            v[i] = y + a.dxm[b * Sp + s];
          }
        }
      }
      store_block(v, dxT, a.dx, Sp, row, 16 * w, c, g);
    }
    __syncthreads();
    if (w < nbS) bwd_block_leaky(a.n.w2, S, S, 16 * w, dxT, h1T, a.dz1, Sp, row, c, g);
  }
}

// ---- the weight pass
struct Layer {
  const float *dz, *in;      // dz [rows][ldz], in [rows][lin] (layer 0: gathered from obs | comm)
  int64_t ldz, lin, rows, off_w, off_b;      // rows: the valid ones; off_b < 0: no bias
  int M, Nn, nbm, nbn, first;                // first: the layer's first block
};

struct WeightArgs {
  Layer l[5];
  int total;               // blocks of all layers; block `total` is the losses'
  int F;
  const float *obs, *comm;
  int64_t ld_obs, ld_comm;
  const int64_t* index;
  int N;
  const float* terms;
  int64_t B;
  float count;
  float *grad, *losses;
};

__global__ __launch_bounds__(64 * WW) void k_a2c_weights(WeightArgs a) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  for (int blk = blockIdx.x * WW + w; blk <= a.total; blk += gridDim.x * WW) {
    if (blk == a.total) {
      // the three losses: 64 strided sums, added in lane order
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
      for (int64_t b = lane; b < a.B; b += 64) s0 += a.terms[4 * b], s1 += a.terms[4 * b + 1], s2 += a.terms[4 * b + 2];
      float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
      for (int l = 0; l < 64; ++l) t0 += __shfl(s0, l), t1 += __shfl(s1, l), t2 += __shfl(s2, l);
      if (lane == 0) a.losses[0] = t0 / a.count, a.losses[1] = t1 / a.count, a.losses[2] = t2 / a.count;
      continue;
    }
    int li = 0;
#pragma unroll
    for (int i = 1; i < 5; ++i)
      if (blk >= a.l[i].first) li = i;
    const Layer& L = a.l[li];
    const int rel = blk - L.first, mb = rel / L.nbn, nbk = rel - mb * L.nbn;
    const int m = 16 * mb + c, n = 16 * nbk + c;
    const bool mok = m < L.M, nok = n < L.Nn;
    const bool bias = nbk == 0 && L.off_b >= 0;
    f32x4 acc = {0, 0, 0, 0}, accb = {0, 0, 0, 0};
    for (int64_t r0 = 0; r0 < L.rows; r0 += 4 * UNR_W) {
      float av[UNR_W], bv[UNR_W];
#pragma unroll
      for (int i = 0; i < UNR_W; ++i) {
        // every load unconditional from an address clamped into its array, the value selected afterwards
        const int64_t r = r0 + 4 * i + g;
        const bool rin = r < L.rows;
        const int64_t rc = rin ? r : L.rows - 1;
        const float x = L.dz[rc * L.ldz + (mok ? m : 0)];
        av[i] = (rin && mok) ? x : 0.0f;
        float y;
        if (li != 0) {
          y = L.in[rc * L.lin + (nok ? n : 0)];
        } else {
          const int64_t b = rc / a.N, src = (a.index ? a.index[b] : b) * a.N + (rc - b * a.N);
          const int nc = nok ? n : 0;
          y = nc < a.F ? a.obs[src * a.ld_obs + nc] : a.comm[src * a.ld_comm + (nc - a.F)];
        }
        bv[i] = (rin && nok) ? y : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < UNR_W; ++i) {      // rows past the batch add exact zeros
        acc = mfma(av[i], bv[i], acc);
        if (bias) accb = mfma(av[i], 1.0f, accb);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mm = 16 * mb + 4 * g + i;
      if (mm < L.M) {
        if (nok) a.grad[L.off_w + (int64_t)mm * L.Nn + n] = acc[i];
        if (bias && c == 0) a.grad[L.off_b + mm] = accb[i];
      }
    }
  }
}

// ---- the attention of one env: q, k, v from x, dense softmax over all N senders, comm_out = attn v
struct CommArgs {
  Net n;
  const float* x;          // [E N][S]
  int64_t E;
  int N;
  float sqrtc;             // the fp32 value of sqrt(C)
  float* out;
  int64_t ldo;
  float* attn;             // [E][N][N] or null
};

constexpr int XS = MAX_S + 1, QS = MAX_K + 1, VS = MAX_C + 1, SS = MAX_N + 1;      // odd row strides: no bank conflicts down a column

__global__ __launch_bounds__(CT) void k_a2c_comm(CommArgs a) {
  __shared__ float sx[MAX_N * XS];      // x [N][S], then the scores [N][N]
  __shared__ float sq[MAX_N * QS], sk[MAX_N * QS], sv[MAX_N * VS], ssum[MAX_N];
  static_assert(MAX_N * SS <= MAX_N * XS, "the scores take x's place");
  const int tid = threadIdx.x;
  const int N = a.N, S = a.n.S, K = a.n.K, Cc = a.n.C;
  float* sc = sx;
  for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
    __syncthreads();      // the env before is read
    for (int i = tid; i < N * S; i += CT) {
      const int n = i / S, s = i - n * S;
      sx[n * XS + s] = a.x[(e * N + n) * S + s];
    }
    __syncthreads();
    // outputs o of [q | k | v] for agent n, n fastest: the lanes of a wave share a weight row; k ascending on one accumulator
    const int O = 2 * K + Cc;
    for (int i = tid; i < O * N; i += CT) {
      const int o = i / N, n = i - o * N;
      const float *wr, *bp;
      float* dst;
      if (o < K) wr = a.n.wq + o * S, bp = a.n.bq + o, dst = sq + n * QS + o;
      else if (o < 2 * K) wr = a.n.wk + (o - K) * S, bp = a.n.bk + (o - K), dst = sk + n * QS + (o - K);
      else wr = a.n.wv + (o - 2 * K) * S, bp = a.n.bv + (o - 2 * K), dst = sv + n * VS + (o - 2 * K);
      float acc = *bp;
      const float* xr = sx + n * XS;
      for (int s = 0; s < S; ++s) acc = fmaf(wr[s], xr[s], acc);
      *dst = acc;
    }
    __syncthreads();      // x is read: the scores take its place
    for (int p = tid; p < N * N; p += CT) {
      const int i = p / N, j = p - i * N;
      float acc = 0.0f;
      for (int k = 0; k < K; ++k) acc = fmaf(sq[i * QS + k], sk[j * QS + k], acc);
      sc[i * SS + j] = acc / a.sqrtc;
    }
    __syncthreads();
    if (tid < N) {      // the row's maximum, exponentials and their sum in ascending j
      float* row = sc + tid * SS;
      float mx = row[0];
      for (int j = 1; j < N; ++j) mx = fmaxf(mx, row[j]);
      float sum = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float ex = expf(row[j] - mx);
        row[j] = ex;
        sum += ex;
      }
      ssum[tid] = sum;
    }
    __syncthreads();
    for (int p = tid; p < N * N; p += CT) {
      const int i = p / N, j = p - i * N;
      const float at = sc[i * SS + j] / ssum[i];
      sc[i * SS + j] = at;
      if (a.attn) a.attn[(e * N + i) * N + j] = at;
    }
    __syncthreads();
    for (int p = tid; p < N * Cc; p += CT) {
      const int i = p / Cc, cc = p - i * Cc;
      float acc = 0.0f;
      for (int j = 0; j < N; ++j) acc = fmaf(sc[i * SS + j], sv[j * VS + cc], acc);
      a.out[(e * N + i) * a.ldo + cc] = acc;
    }
  }
}

// ---- host side
int shape(const mdr_tarmac_a2c_net_t* n) {
  if (!n || n->struct_size != sizeof(mdr_tarmac_a2c_net_t) || n->num_obs < 1 || n->num_comm < 1 || n->state_size < 1 || n->num_key < 1)
    return MDR_ERR_INVALID;
  if (n->num_obs > MAX_F || n->num_comm > MAX_C || n->num_comm % 4 || n->state_size > MAX_S || n->state_size % 4 || n->num_key > MAX_K ||
      n->num_key % 4)
    return MDR_ERR_UNSUPPORTED;
  return MDR_OK;
}

bool trunk_ok(const mdr_tarmac_a2c_net_t* n) {
  return n->common_w0 && n->common_b0 && n->common_w2 && n->common_b2 && n->critic_w0 && n->critic_b0 && n->critic_w3 && n->critic_b3 &&
         n->dist_w;
}
bool comm_ok(const mdr_tarmac_a2c_net_t* n) { return n->query_w && n->query_b && n->key_w && n->key_b && n->value_w && n->value_b; }

Net net_of(const mdr_tarmac_a2c_net_t* n) {
  Net d;
  d.w1 = n->common_w0, d.b1 = n->common_b0, d.w2 = n->common_w2, d.b2 = n->common_b2;
  d.wc1 = n->critic_w0, d.bc1 = n->critic_b0, d.wc2 = n->critic_w3, d.bc2 = n->critic_b3;
  d.wq = n->query_w, d.bq = n->query_b, d.wk = n->key_w, d.bk = n->key_b, d.wv = n->value_w, d.bv = n->value_b, d.wd = n->dist_w;
  d.F = n->num_obs, d.C = n->num_comm, d.S = n->state_size, d.K = n->num_key;
  return d;
}

int64_t grad_floats(const mdr_tarmac_a2c_net_t* n) {
  const int64_t S = n->state_size, I = (int64_t)n->num_obs + n->num_comm;
  return S * I + S + S * S + S + S * S + S + S + 1 + 2 * S;
}

// floats: h1, x, dx, dz1 [Rp][Sp] | logits, dl [Rp][2] | xbar, a, da, dxbar / N [Bp][Sp] | dV [Bp] | terms [Bp][4]
int64_t ws_floats(const mdr_tarmac_a2c_net_t* n, int64_t B, int64_t N) {
  const int64_t Rp = pad16(B * N), Bp = pad16(B), Sp = pad16(n->state_size);
  return 4 * Rp * Sp + 4 * Rp + 4 * Bp * Sp + Bp + 4 * Bp;
}

int steps_ok(int64_t nb_steps, int32_t nb_agents, int32_t max_workgroups) {
  if (nb_steps < 0 || nb_agents < 1 || max_workgroups < 0) return MDR_ERR_INVALID;
  if (nb_agents > MAX_N || nb_steps > (int64_t)1 << 24) return MDR_ERR_UNSUPPORTED;
  return MDR_OK;
}

int launched() { return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP; }

int64_t capped(int64_t items, int cap) { return items < cap ? items : cap; }

}  // namespace

extern "C" {

int64_t mdr_tarmac_a2c_grad_floats(const mdr_tarmac_a2c_net_t* net) {
  if (shape(net) != MDR_OK) return -1;
  return grad_floats(net);
}

int64_t mdr_tarmac_a2c_workspace_bytes(const mdr_tarmac_a2c_net_t* net, int64_t nb_steps, int32_t nb_agents, int32_t max_workgroups) {
  if (shape(net) != MDR_OK || steps_ok(nb_steps, nb_agents, max_workgroups) != MDR_OK) return -1;
  const int64_t f = ws_floats(net, nb_steps, nb_agents);
  return (f > 4 ? f : 4) * (int64_t)sizeof(float);
}

int mdr_tarmac_a2c_forward(const mdr_tarmac_a2c_net_t* net, const float* obs, int64_t ld_obs, const float* comm_in, int64_t ld_comm,
                           const int64_t* index, int64_t nb_steps, int32_t nb_agents, int32_t max_workgroups, void* workspace, float* logits,
                           float* value, float* x, void* stream) {
  if (!obs || !comm_in || !logits || !value || ((uintptr_t)x & 15u) || ((uintptr_t)workspace & 15u) || (!x && !workspace)) return MDR_ERR_INVALID;
  const int rc = shape(net);
  if (rc == MDR_ERR_INVALID) return rc;
  const int rs = steps_ok(nb_steps, nb_agents, max_workgroups);
  if (rs == MDR_ERR_INVALID || !trunk_ok(net) || ld_obs < net->num_obs || ld_comm < net->num_comm) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (rs != MDR_OK) return rs;
  if (nb_steps == 0) return MDR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  const int64_t R = nb_steps * nb_agents, Sp = pad16(net->state_size);
  RowArgs a{};
  a.n = net_of(net), a.obs = obs, a.comm = comm_in, a.ld_obs = ld_obs, a.ld_comm = ld_comm, a.index = index;
  a.R = R, a.ntiles = (R + TILE - 1) / TILE, a.N = nb_agents, a.h1 = nullptr, a.logits = logits;
  a.lpad = 0;
  if (x) a.x = x, a.ldx = net->state_size, a.xlim = net->state_size, a.xpad = 0;
  else a.x = static_cast<float*>(workspace) + pad16(R) * Sp, a.ldx = Sp, a.xlim = (int)Sp, a.xpad = 1;      // x's place in the workspace of the update
  hipLaunchKernelGGL(k_a2c_rows, dim3((unsigned)capped(a.ntiles, cap)), dim3(64 * NW), 0, st, a);
  if (launched() != MDR_OK) return MDR_ERR_HIP;
  StepArgs s{};
  s.n = a.n, s.x = a.x, s.ldx = a.ldx, s.index = index, s.B = nb_steps, s.N = nb_agents, s.value = value;
  hipLaunchKernelGGL(k_a2c_steps<false>, dim3((unsigned)capped(nb_steps, cap)), dim3(ST), 0, st, s);
  return launched();
}

int mdr_tarmac_a2c_comm(const mdr_tarmac_a2c_net_t* net, const float* x, int64_t nb_envs, int32_t nb_agents, int32_t max_workgroups,
                        float* comm_out, int64_t ld_out, float* attn, void* stream) {
  if (!x || !comm_out) return MDR_ERR_INVALID;
  const int rc = shape(net);
  if (rc == MDR_ERR_INVALID) return rc;
  const int rs = steps_ok(nb_envs, nb_agents, max_workgroups);
  if (rs == MDR_ERR_INVALID || !comm_ok(net) || ld_out < net->num_comm) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (rs != MDR_OK) return rs;
  if (nb_envs == 0) return MDR_OK;
  CommArgs a{};
  a.n = net_of(net), a.x = x, a.E = nb_envs, a.N = nb_agents, a.sqrtc = (float)std::sqrt((double)net->num_comm);
  a.out = comm_out, a.ldo = ld_out, a.attn = attn;
  // the library's own grid: several workgroups per compute unit (a workgroup of 256 threads and ~50 KiB of LDS: three fit)
  const int cap = max_workgroups > 0 ? max_workgroups : 3 * lib_cap(0);
  hipLaunchKernelGGL(k_a2c_comm, dim3((unsigned)capped(nb_envs, cap)), dim3(CT), 0, (hipStream_t)stream, a);
  return launched();
}

int mdr_tarmac_a2c_grad(const mdr_tarmac_a2c_net_t* net, const float* obs, int64_t ld_obs, const float* comm_in, int64_t ld_comm,
                        const int64_t* action, const float* ret, const int64_t* index, int64_t nb_steps, int32_t nb_agents, float value_coef,
                        float entropy_coef, int32_t max_workgroups, void* workspace, float* grad, float* losses, float* value, float* advantage,
                        void* stream) {
  if (!obs || !comm_in || !action || !ret || !grad || !losses || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  const int rc = shape(net);
  if (rc == MDR_ERR_INVALID) return rc;
  const int rs = steps_ok(nb_steps, nb_agents, max_workgroups);
  if (rs == MDR_ERR_INVALID || !trunk_ok(net) || ld_obs < net->num_obs || ld_comm < net->num_comm) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (rs != MDR_OK) return rs;
  hipStream_t st = (hipStream_t)stream;
  const int64_t G = grad_floats(net);
  if (nb_steps == 0) {      // no kernel: zeros
    if (hipMemsetAsync(grad, 0, (size_t)G * sizeof(float), st) != hipSuccess || hipMemsetAsync(losses, 0, 3 * sizeof(float), st) != hipSuccess)
      return MDR_ERR_HIP;
    return MDR_OK;
  }
  const int cap = lib_cap(max_workgroups);
  const int S = net->state_size, F = net->num_obs, Cc = net->num_comm, I = F + Cc;
  const int64_t B = nb_steps, N = nb_agents, R = B * N, Rp = pad16(R), Bp = pad16(B), Sp = pad16(S);
  float* p = static_cast<float*>(workspace);
  float* h1 = p; p += Rp * Sp;
  float* xx = p; p += Rp * Sp;
  float* dx = p; p += Rp * Sp;
  float* dz1 = p; p += Rp * Sp;
  float* lg = p; p += 2 * Rp;
  float* dl = p; p += 2 * Rp;
  float* xbar = p; p += Bp * Sp;
  float* act = p; p += Bp * Sp;
  float* da = p; p += Bp * Sp;
  float* dxm = p; p += Bp * Sp;
  float* dv = p; p += Bp;
  float* terms = p;
  const double count = (double)B * (double)N;

  RowArgs a{};
  a.n = net_of(net), a.obs = obs, a.comm = comm_in, a.ld_obs = ld_obs, a.ld_comm = ld_comm, a.index = index;
  a.R = R, a.ntiles = Rp / TILE, a.N = nb_agents, a.h1 = h1, a.x = xx, a.ldx = Sp, a.xlim = (int)Sp, a.xpad = 1, a.lpad = 1, a.logits = lg;
  hipLaunchKernelGGL(k_a2c_rows, dim3((unsigned)capped(a.ntiles, cap)), dim3(64 * NW), 0, st, a);
  if (launched() != MDR_OK) return MDR_ERR_HIP;

  StepArgs s{};
  s.n = a.n, s.x = xx, s.ldx = Sp, s.logits = lg, s.action = action, s.ret = ret, s.index = index, s.B = B, s.Bp = Bp, s.R = R, s.Rp = Rp;
  s.N = nb_agents, s.inv = (float)(1.0 / count), s.cv = (float)(-2.0 * (double)value_coef / count), s.ec = entropy_coef;
  s.value = value, s.advantage = advantage, s.dl = dl, s.xbar = xbar, s.act = act, s.da = da, s.dxm = dxm, s.dv = dv, s.terms = terms;
  hipLaunchKernelGGL(k_a2c_steps<true>, dim3((unsigned)capped(Bp, cap)), dim3(ST), 0, st, s);
  if (launched() != MDR_OK) return MDR_ERR_HIP;

  BackArgs k{};
  k.n = a.n, k.R = R, k.ntiles = Rp / TILE, k.N = nb_agents, k.h1 = h1, k.dl = dl, k.dxm = dxm, k.dx = dx, k.dz1 = dz1;
  hipLaunchKernelGGL(k_a2c_rows_bwd, dim3((unsigned)capped(k.ntiles, cap)), dim3(64 * NW), 0, st, k);
  if (launched() != MDR_OK) return MDR_ERR_HIP;

  WeightArgs wa{};
  const int64_t oW1 = 0, ob1 = (int64_t)S * I, oW2 = ob1 + S, ob2 = oW2 + (int64_t)S * S, oC1 = ob2 + S, obc1 = oC1 + (int64_t)S * S,
                oC2 = obc1 + S, obc2 = oC2 + S, oWd = obc2 + 1;
  //                 dz   in     ldz lin rows off_w off_b  M  Nn
  wa.l[0] = Layer{dz1, nullptr, Sp, 0, R, oW1, ob1, S, I, 0, 0, 0};
  wa.l[1] = Layer{dx, h1, Sp, Sp, R, oW2, ob2, S, S, 0, 0, 0};
  wa.l[2] = Layer{da, xbar, Sp, Sp, B, oC1, obc1, S, S, 0, 0, 0};
  wa.l[3] = Layer{dv, act, 1, Sp, B, oC2, obc2, 1, S, 0, 0, 0};
  wa.l[4] = Layer{dl, xx, 2, Sp, R, oWd, -1, 2, S, 0, 0, 0};
  int total = 0;
  for (Layer& L : wa.l) {
    L.nbm = blocks16(L.M), L.nbn = blocks16(L.Nn), L.first = total;
    total += L.nbm * L.nbn;
  }
  wa.total = total, wa.F = F, wa.obs = obs, wa.comm = comm_in, wa.ld_obs = ld_obs, wa.ld_comm = ld_comm, wa.index = index, wa.N = nb_agents;
  wa.terms = terms, wa.B = B, wa.count = (float)count, wa.grad = grad, wa.losses = losses;
  int grid = (total + 1 + WW - 1) / WW;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  hipLaunchKernelGGL(k_a2c_weights, dim3((unsigned)grid), dim3(64 * WW), 0, st, wa);
  return launched();
}

}  // extern "C"
