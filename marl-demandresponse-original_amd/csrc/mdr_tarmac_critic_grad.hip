// TarMAC-PPO's centralised critic step (include/mdr_policy.h: mdr_tarmac_critic_value, mdr_tarmac_critic_grad): value, advantage,
// value loss and gradient of TarMAC_Critic (agents/network.py:241-259) as TarmacPPO.update takes them (agents/tarmac_ppo.py:159-166,
// 196-204), weights streamed from L2.
//
// The network is Linear(J, H1) - ReLU - Linear(H1, H2) - ReLU - Linear(H2, N) on the joint observation of an env-step, J = N F up
// to 4096 columns (50 houses of 51 features: 2550), with one value per agent: its last layer is a matrix layer in both directions.
// The scheme is mdr_maddpg_grad.hip's (the helpers of both are csrc/mdr_stream_mlp.h):
//
//   row pass     one workgroup of 16 waves.  With nb = max(blocks16(H1), blocks16(H2), blocks16(N)) the workgroup takes G = 16 / nb
//                (rounded down) tiles of 16 minibatch rows at once: wave w belongs to tile slot w / nb and owns the 16-unit block
//                w % nb of every layer of that slot's tile.  All slots stream the same weights at the same time - at the
//                reference's 64 hidden units four tiles share every weight line a workgroup asks L2 for.  The joint input is
//                staged in chunks of KCe = min(128, 512 / G rounded down to a power of two) columns per slot while the first layer's
//                accumulators stay in registers.  Every contraction of a row runs inside ONE wave, on one accumulator, in an order of
//                k that the shape alone fixes (ascending steps of four; the first layer in fwd_accum_wide's groups of 16): a row's
//                bits depend neither on its slot nor on the grid nor on the chunk width.
//                  V = W3 h2 + b3;  delta = target[j] - V (rounded once);  advantage = delta;  term = delta^2;
//                  dV = (-2 delta) inv, inv = the fp32 value of 1 / (B N) formed on the host in double - ONE scale for autograd's
//                  mean(0).mean(0) (which divides by B and then by N);  dz2 = relu'(h2) W3^T dV;  dz1 = relu'(h1) W2^T dz2.
//                h1, h2, dz1, dz2 [Bp][pad16(H)], dV [Bp][pad16(N)] and the rows' summed terms [Bp] are left in the workspace.
//   weight pass  one wave per 16 x 16 block of a weight gradient: dW[m][n] = sum_r dz[r][m] in[r][n] over the minibatch rows in row
//                order on the MFMA - no partials, no floating-point atomics.  The first layer's input is gathered again from
//                `state` through `index`.  The blocks of column 0 also take the bias; one more wave sums the loss,
//                loss = (sum_r term_r) / (float)(B N): 64 strided sums added in lane order.
//
// relu'(z) = 1 iff relu(z) > 0.  Rows past the minibatch are forwarded as zero inputs and given zero dV: they add exact zeros.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_stream_mlp.h"

namespace {

using namespace mdr_stream;

constexpr int NW = 16;                // waves per row-pass workgroup
constexpr int TILE = 16;              // minibatch rows per tile
constexpr int MAX_H = 256, MAX_J = 4096, MAX_N = 64;
constexpr int XCOLS = 512;            // staged input columns of all tile slots together
constexpr int WW = 4;                 // waves per weight-pass workgroup
constexpr int UNR = 8;                // row pass: MFMA k-steps whose weights are loaded together
constexpr int UQ1 = 4;                // the wide first layer: groups of 16 columns whose weights are loaded together
constexpr int UNR_W = 8;              // weight pass: MFMA k-steps whose global operands are loaded together

// LDS of the row pass (floats): the slots' input chunks, three images (h1 / dz1, h2 / dz2, dV) of G slots x nb blocks <= 256 units,
// the blocks' shares of a row's loss term, the env-steps of the rows
constexpr int S_X = 0, S_H1 = S_X + XCOLS * LT, S_H2 = S_H1 + MAX_H * LT, S_DV = S_H2 + MAX_H * LT, S_TP = S_DV + MAX_H * LT,
              S_JR = S_TP + NW * TILE, S_END = S_JR + 2 * NW * TILE;      // S_JR: the env-steps of the pass's rows, int64 (8-byte aligned)
constexpr int STAGE_TRIPS = XCOLS * TILE / (64 * NW);      // staged elements per thread and chunk at the most
constexpr int STAGE_BATCH = 4;                             // of which this many loads are in flight together
static_assert(S_JR % 2 == 0 && XCOLS * TILE % (64 * NW) == 0 && STAGE_TRIPS % STAGE_BATCH == 0, "layout");

// fwd_accum (csrc/mdr_stream_mlp.h) with every weight load unconditional: the address is clamped into the row (the last column of the
// chunk for k-steps past it, row 0 for a unit past H) and the value selected afterwards, so the UNR loads of a loop trip are in flight
// together instead of each waiting under its own branch.  The same k order on the same accumulator: the same bits as fwd_accum.
template <int UNR>
__device__ __forceinline__ void fwd_accum_flat(f32x4& acc, const float* __restrict__ W, int ldw, int H, int u0, int k0, int kn, const float* inT,
                                               int c, int g) {
  const int u = u0 + c;
  const bool uok = u < H;
  const float* wr = W + (int64_t)(uok ? u : 0) * ldw + k0;
  const int ks = (kn + 3) >> 2, last = kn - 1;      // kn >= 1
  for (int q0 = 0; q0 < ks; q0 += UNR) {
    float av[UNR];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int kk = 4 * (q0 + i) + g;
      const float v = wr[kk < kn ? kk : last];
      av[i] = (uok && kk < kn) ? v : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
      if (q0 + i < ks) acc = mfma(av[i], inT[(4 * (q0 + i) + g) * LT + c], acc);
  }
}

// The wide first layer: the chunk's kn columns in groups of 16, of which lane (c, g) loads the four consecutive weights W[u0 + c][k0 +
// 16 Q + 4 g ..+ 3] at once and spends them on four MFMA steps - step (Q, e) contracts the columns 16 Q + 4 g + e, g = 0..3.  One
// 16-byte load per four k-steps instead of four 4-byte loads from the same 16 cache lines: the row pass is bound by the number of load
// instructions, not by bytes.  UQ groups are in flight together; the last, partial group goes element by element.  A chunk starts
// at a multiple of 16 and only the last one is partial, so the order of the sum does not depend on the chunk width.
template <int UQ>
__device__ __forceinline__ void fwd_accum_wide(f32x4& acc, const float* __restrict__ W, int ldw, int H, int u0, int k0, int kn, const float* inT,
                                               int c, int g) {
  const int u = u0 + c;
  const bool uok = u < H;
  const float* wr = W + (int64_t)(uok ? u : 0) * ldw + k0;
  const int full = kn >> 4;
  for (int Q0 = 0; Q0 < full; Q0 += UQ) {
    f32x4 av[UQ];
#pragma unroll
    for (int i = 0; i < UQ; ++i) {
      const int Q = Q0 + i < full ? Q0 + i : full - 1;      // an address inside the row for the groups past the end
      f32x4 t;
      __builtin_memcpy(&t, wr + 16 * Q + 4 * g, sizeof(t));      // 4-byte aligned: a row starts at u * ldw floats
#pragma unroll
      for (int e = 0; e < 4; ++e) av[i][e] = uok ? t[e] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < UQ; ++i)
      if (Q0 + i < full) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma(av[i][e], inT[(16 * (Q0 + i) + 4 * g + e) * LT + c], acc);
      }
  }
  const int kt = 16 * full;
  if (kt < kn) {      // inT holds zeros from kn up to the chunk's width, a multiple of 16
    float at[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = kt + 4 * g + e;
      const float v = wr[kk < kn ? kk : kn - 1];
      at[e] = (uok && kk < kn) ? v : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma(at[e], inT[(kt + 4 * g + e) * LT + c], acc);
  }
}

struct RowArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int J, H1, H2, N;
  int nb, G, KCe, lk;          // blocks per slot, tile slots per workgroup, staged columns per slot = 1 << lk
  const float* state;         // env-step j at state + j * ld
  int64_t ld;
  const float* target;        // [env-steps][N]
  const int64_t* index;
  int64_t B, ntiles;
  float inv;                  // 1 / (B N)
  float *value, *advantage;   // [B][N], may be null
  float *h1, *h2, *dz1, *dz2, *dv, *term;      // workspace: [Bp][H1p], [Bp][H2p], ..., [Bp][Np], [Bp]
};

template <bool GRAD>
__global__ __launch_bounds__(64 * NW) void k_tcritic_rows(RowArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int nb = a.nb, G = a.G, KCe = a.KCe;
  const int gi = w / nb, bi = w - gi * nb;      // tile slot and block of this wave; slots >= G idle
  const int nb1 = blocks16(a.H1), nb2 = blocks16(a.H2), nbo = blocks16(a.N);
  const int H1p = 16 * nb1, H2p = 16 * nb2, Np = 16 * nbo;
  const int sg = gi < G ? gi : 0;               // idle waves point at slot 0 and touch nothing
  float* xT = lds + S_X + sg * KCe * LT;
  float* h1T = lds + S_H1 + sg * nb * 16 * LT;  // h1, then dz1
  float* h2T = lds + S_H2 + sg * nb * 16 * LT;  // h2, then dz2
  float* dvT = lds + S_DV + sg * nb * 16 * LT;
  float* tp = lds + S_TP + sg * nb * TILE;      // [block][row]
  int64_t* jrow = reinterpret_cast<int64_t*>(lds + S_JR);      // [slot][row]: the row's env-step, -1 past the minibatch
  const int lk = a.lk, total = G * TILE * KCe;

  for (int64_t base = (int64_t)blockIdx.x * G; base < a.ntiles; base += (int64_t)gridDim.x * G) {
    const int64_t t = base + gi;
    const bool act = gi < G && t < a.ntiles;
    const int64_t row = t * TILE + c;      // the row this lane's MFMA column and head work belong to
    const bool valid = act && row < a.B;

    if (tid < G * TILE) {      // read by the staging below, behind the chunk loop's first barrier; last read before the pass's other barriers
      const int64_t rr = base * TILE + tid;
      jrow[tid] = rr < a.B ? (a.index ? a.index[rr] : rr) : -1;
    }
    // ---- layer 1 over the joint input in chunks of KCe columns per slot
    f32x4 acc = bias_block(a.b1, a.H1, 16 * bi, g);
    for (int k0 = 0; k0 < a.J; k0 += KCe) {
      const int kn = a.J - k0 < KCe ? a.J - k0 : KCe;
      __syncthreads();      // the chunk before is read
      // element e = (slot, row, column f) with f fastest; every load unconditional from an address clamped into `state` (env-step 0,
      // column 0 where the element is a zero), the value selected afterwards: a thread's loads are in flight together
#pragma unroll 1
      for (int it0 = 0; it0 < STAGE_TRIPS; it0 += STAGE_BATCH) {
        float sv[STAGE_BATCH];
#pragma unroll
        for (int it = 0; it < STAGE_BATCH; ++it) {
          const int e = tid + (it0 + it) * 64 * NW, ec = e < total ? e : total - 1;
          const int f = ec & (KCe - 1), sr = ec >> lk, col = k0 + f;      // sr = slot * 16 + row
          const int64_t j = jrow[sr];
          const bool ok = j >= 0 && col < a.J;
          const float v = a.state[(ok ? j : 0) * a.ld + (ok ? col : 0)];
          sv[it] = ok ? v : 0.0f;
        }
#pragma unroll
        for (int it = 0; it < STAGE_BATCH; ++it) {
          const int e = tid + (it0 + it) * 64 * NW;
          if (e < total) lds[S_X + ((e >> (lk + 4)) * KCe + (e & (KCe - 1))) * LT + ((e >> lk) & 15)] = sv[it];
        }
      }
      __syncthreads();
      if (act && bi < nb1) fwd_accum_wide<UQ1>(acc, a.w1, a.J, a.H1, 16 * bi, k0, kn, xT, c, g);
    }
    if (act && bi < nb1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.0f);
      store_block(acc, h1T, GRAD ? a.h1 : nullptr, H1p, row, 16 * bi, c, g);
    }
    __syncthreads();
    // ---- layer 2
    if (act && bi < nb2) {
      f32x4 z = bias_block(a.b2, a.H2, 16 * bi, g);
      fwd_accum_flat<UNR>(z, a.w2, a.H1, a.H2, 16 * bi, 0, a.H1, h1T, c, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = fmaxf(z[i], 0.0f);
      store_block(z, h2T, GRAD ? a.h2 : nullptr, H2p, row, 16 * bi, c, g);
    }
    __syncthreads();
    // ---- layer 3 and the head: agents 16 bi + 4 g + i of row c
    if (act && bi < nbo) {
      f32x4 v = bias_block(a.b3, a.N, 16 * bi, g);
      fwd_accum_flat<UNR>(v, a.w3, a.H2, a.N, 16 * bi, 0, a.H2, h2T, c, g);
      f32x4 dv = {0, 0, 0, 0};
      float part = 0.0f;
      if (valid) {
        const int64_t j = a.index ? a.index[row] : row;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * bi + 4 * g + i;
          if (k < a.N) {
            if (a.value) a.value[row * a.N + k] = v[i];
            if constexpr (GRAD) {
              const float delta = a.target[j * a.N + k] - v[i];
              if (a.advantage) a.advantage[row * a.N + k] = delta;
              const float sq = delta * delta;
              part += sq;
              const float twice = -2.0f * delta;
              dv[i] = twice * a.inv;
            }
          }
        }
      }
      if constexpr (GRAD) {
        store_block(dv, dvT, a.dv, Np, row, 16 * bi, c, g);
        // the block's share of the row's term: the lane's four agents, then the four lanes of the row in a fixed tree
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (g == 0) tp[bi * TILE + c] = part;
      }
    }
    if constexpr (!GRAD) continue;      // the next pass begins with a barrier
    __syncthreads();
    // ---- dz2 = relu'(h2) W3^T dV in place of h2's image; the row's term in block order
    if (act && bi < nb2) bwd_block<UNR>(a.w3, a.N, a.H2, 16 * bi, dvT, h2T, a.dz2, H2p, row, c, g);
    if (act && bi == 0 && g == 0) {
      float s = 0.0f;
      for (int b = 0; b < nbo; ++b) s += tp[b * TILE + c];
      a.term[row] = s;
    }
    __syncthreads();
    // ---- dz1 = relu'(h1) W2^T dz2 in place of h1's image (a wave reads and writes its own block of it)
    if (act && bi < nb1) bwd_block<UNR>(a.w2, a.H2, a.H1, 16 * bi, h2T, h1T, a.dz1, H1p, row, c, g);
  }
}

// ---- the weight pass
struct WeightArgs {
  int J, H1, H2, N;
  int H1p, H2p, Np;
  const float *h1, *h2, *dz1, *dz2, *dv, *term;
  const float* state;
  int64_t ld;
  const int64_t* index;
  int64_t B, Bp;
  float count;                 // (float)(B N)
  float* grad;
  float* loss;
  int nbk, nb1, nb2, nbo;      // 16-blocks of J, H1, H2, N
};

__global__ __launch_bounds__(64 * WW) void k_tcritic_weights(WeightArgs a) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int n1 = a.nb1 * a.nbk, n2 = a.nb2 * a.nb1, n3 = a.nbo * a.nb2;
  const int total = n1 + n2 + n3 + 1;
  const int64_t oW1 = 0, ob1 = (int64_t)a.H1 * a.J, oW2 = ob1 + a.H1, ob2 = oW2 + (int64_t)a.H2 * a.H1, oW3 = ob2 + a.H2,
                ob3 = oW3 + (int64_t)a.N * a.H2;
  for (int blk = blockIdx.x * WW + w; blk < total; blk += gridDim.x * WW) {
    if (blk == total - 1) {
      // the loss: 64 strided sums, added in lane order
      float s = 0.0f;
      for (int64_t r = lane; r < a.B; r += 64) s += a.term[r];
      float sum = 0.0f;
      for (int l = 0; l < 64; ++l) sum += __shfl(s, l);
      if (lane == 0) *a.loss = a.B > 0 ? sum / a.count : 0.0f;
      continue;
    }
    int layer, mb, nbk;
    if (blk < n1) layer = 0, mb = blk / a.nbk, nbk = blk - mb * a.nbk;
    else if (blk < n1 + n2) layer = 1, mb = (blk - n1) / a.nb1, nbk = (blk - n1) - mb * a.nb1;
    else layer = 2, mb = (blk - n1 - n2) / a.nb2, nbk = (blk - n1 - n2) - mb * a.nb2;
    const int M = layer == 0 ? a.H1 : layer == 1 ? a.H2 : a.N;
    const int Nn = layer == 0 ? a.J : layer == 1 ? a.H1 : a.H2;
    const float* dz = layer == 0 ? a.dz1 : layer == 1 ? a.dz2 : a.dv;
    const int ldz = layer == 0 ? a.H1p : layer == 1 ? a.H2p : a.Np;
    const float* in = layer == 1 ? a.h1 : a.h2;
    const int lin = layer == 1 ? a.H1p : a.H2p;
    const int m = 16 * mb + c, n = 16 * nbk + c;
    const bool mok = m < M, nok = n < Nn;
    f32x4 acc = {0, 0, 0, 0}, accb = {0, 0, 0, 0};
    for (int64_t r0 = 0; r0 < a.Bp; r0 += 4 * UNR_W) {      // UNR_W k-steps of four rows, their operands in flight together
      float av[UNR_W], bv[UNR_W];
#pragma unroll
      for (int i = 0; i < UNR_W; ++i) {
        // every load unconditional, from an address clamped into its array, the value selected afterwards: all in flight together
        const int64_t r = r0 + 4 * i + g;
        const bool rin = r < a.Bp;
        const int64_t rc = rin ? r : a.Bp - 1;
        const float x = dz[rc * ldz + (mok ? m : 0)];
        av[i] = (rin && mok) ? x : 0.0f;
        if (layer != 0) {
          const float y = in[rc * lin + (nok ? n : 0)];
          bv[i] = (rin && nok) ? y : 0.0f;
        } else {
          const int64_t rb = r < a.B ? r : a.B - 1;      // Bp > 0 here, so B > 0
          const int64_t j = a.index ? a.index[rb] : rb;
          const float y = a.state[j * a.ld + (nok ? n : 0)];
          bv[i] = (r < a.B && nok) ? y : 0.0f;
        }
      }
#pragma unroll
      for (int i = 0; i < UNR_W; ++i) {      // rows past Bp add exact zeros
        acc = mfma(av[i], bv[i], acc);
        if (nbk == 0) accb = mfma(av[i], 1.0f, accb);
      }
    }
    float* dW = a.grad + (layer == 0 ? oW1 : layer == 1 ? oW2 : oW3);
    float* db = a.grad + (layer == 0 ? ob1 : layer == 1 ? ob2 : ob3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mm = 16 * mb + 4 * g + i;
      if (mm < M) {
        if (nok) dW[(int64_t)mm * Nn + n] = acc[i];
        if (nbk == 0 && c == 0) db[mm] = accb[i];
      }
    }
  }
}

// MDR_OK, MDR_ERR_INVALID or MDR_ERR_UNSUPPORTED for the shape fields of `n`
int shape(const mdr_mlp_t* n) {
  if (!n || n->struct_size != sizeof(mdr_mlp_t) || n->num_state <= 0 || n->hidden1 <= 0 || n->hidden2 <= 0 || n->num_out < 1) return MDR_ERR_INVALID;
  if (n->num_state % n->num_out != 0) return MDR_ERR_INVALID;      // J = N F
  if (n->num_state > MAX_J || n->hidden1 > MAX_H || n->hidden2 > MAX_H || n->num_out > MAX_N) return MDR_ERR_UNSUPPORTED;
  return MDR_OK;
}
bool pointers_ok(const mdr_mlp_t* n) { return n->w1 && n->b1 && n->w2 && n->b2 && n->w3 && n->b3; }

int64_t grad_floats(const mdr_mlp_t* n) {
  return (int64_t)n->hidden1 * n->num_state + n->hidden1 + (int64_t)n->hidden2 * n->hidden1 + n->hidden2 + (int64_t)n->num_out * n->hidden2 + n->num_out;
}

// floats of the workspace over nb_rows rows: h1, dz1 [Bp][H1p], h2, dz2 [Bp][H2p], dV [Bp][Np], term [Bp]
int64_t ws_floats(const mdr_mlp_t* n, int64_t nb_rows) {
  const int64_t Bp = pad16(nb_rows);
  return Bp * (2 * pad16(n->hidden1) + 2 * pad16(n->hidden2) + pad16(n->num_out) + 1);
}

void fill_rows(RowArgs& a, const mdr_mlp_t* n, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows) {
  a.w1 = n->w1, a.b1 = n->b1, a.w2 = n->w2, a.b2 = n->b2, a.w3 = n->w3, a.b3 = n->b3;
  a.J = n->num_state, a.H1 = n->hidden1, a.H2 = n->hidden2, a.N = n->num_out;
  int nb = blocks16(a.H1);
  if (blocks16(a.H2) > nb) nb = blocks16(a.H2);
  if (blocks16(a.N) > nb) nb = blocks16(a.N);
  a.nb = nb, a.G = NW / nb;
  int kce = KC;
  while (kce * a.G > XCOLS) kce >>= 1;      // G = 16: 32 columns
  a.KCe = kce;
  a.lk = 0;
  while ((1 << a.lk) < kce) ++a.lk;
  a.state = state, a.ld = ld_state, a.index = index, a.B = nb_rows, a.ntiles = (nb_rows + TILE - 1) / TILE;
}

void carve(RowArgs& r, WeightArgs& wa, const mdr_mlp_t* n, void* workspace, int64_t nb_rows) {
  const int64_t Bp = pad16(nb_rows), H1p = pad16(n->hidden1), H2p = pad16(n->hidden2), Np = pad16(n->num_out);
  float* p = static_cast<float*>(workspace);
  r.h1 = p, p += Bp * H1p;
  r.dz1 = p, p += Bp * H1p;
  r.h2 = p, p += Bp * H2p;
  r.dz2 = p, p += Bp * H2p;
  r.dv = p, p += Bp * Np;
  r.term = p;
  wa.J = n->num_state, wa.H1 = n->hidden1, wa.H2 = n->hidden2, wa.N = n->num_out, wa.H1p = (int)H1p, wa.H2p = (int)H2p, wa.Np = (int)Np;
  wa.h1 = r.h1, wa.h2 = r.h2, wa.dz1 = r.dz1, wa.dz2 = r.dz2, wa.dv = r.dv, wa.term = r.term;
  wa.B = nb_rows, wa.Bp = Bp;
  wa.nbk = blocks16(n->num_state), wa.nb1 = blocks16(n->hidden1), wa.nb2 = blocks16(n->hidden2), wa.nbo = blocks16(n->num_out);
}

template <bool GRAD>
int launch_rows(const RowArgs& a, int cap, hipStream_t st) {
  const size_t bytes = (size_t)S_END * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_tcritic_rows<GRAD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MDR_ERR_HIP;
  const int64_t passes = (a.ntiles + a.G - 1) / a.G;
  const int64_t grid = passes < cap ? passes : cap;
  hipLaunchKernelGGL(k_tcritic_rows<GRAD>, dim3((unsigned)grid), dim3(64 * NW), bytes, st, a);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int launch_weights(const WeightArgs& wa, int cap, hipStream_t st) {
  const int total = wa.nb1 * wa.nbk + wa.nb2 * wa.nb1 + wa.nbo * wa.nb2 + 1;
  int grid = (total + WW - 1) / WW;
  // max_workgroups bounds this pass as well; the library's own choice leaves every block its own wave
  if (cap > 0 && grid > cap) grid = cap;
  hipLaunchKernelGGL(k_tcritic_weights, dim3((unsigned)grid), dim3(64 * WW), 0, st, wa);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

}  // namespace

extern "C" {

int64_t mdr_tarmac_critic_grad_floats(const mdr_mlp_t* critic) {
  if (shape(critic) != MDR_OK) return -1;
  return grad_floats(critic);
}

int64_t mdr_tarmac_critic_workspace_bytes(const mdr_mlp_t* critic, int64_t nb_rows, int32_t max_workgroups) {
  if (shape(critic) != MDR_OK || nb_rows < 0 || max_workgroups < 0) return -1;
  const int64_t f = ws_floats(critic, nb_rows);
  return (f > 4 ? f : 4) * (int64_t)sizeof(float);
}

int mdr_tarmac_critic_value(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* index, int64_t nb_rows,
                            int32_t max_workgroups, float* value, void* stream) {
  if (!state || !value) return MDR_ERR_INVALID;
  const int rc = shape(critic);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(critic) || nb_rows < 0 || max_workgroups < 0 || ld_state < critic->num_state) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (nb_rows == 0) return MDR_OK;
  RowArgs a{};
  fill_rows(a, critic, state, ld_state, index, nb_rows);
  a.value = value;
  return launch_rows<false>(a, lib_cap(max_workgroups), (hipStream_t)stream);
}

int mdr_tarmac_critic_grad(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const float* target, const int64_t* index,
                           int64_t nb_rows, int32_t max_workgroups, void* workspace, float* grad, float* loss, float* value,
                           float* advantage, void* stream) {
  if (!state || !target || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  const int rc = shape(critic);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(critic) || nb_rows < 0 || max_workgroups < 0 || ld_state < critic->num_state) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  RowArgs a{};
  WeightArgs wa{};
  fill_rows(a, critic, state, ld_state, index, nb_rows);
  carve(a, wa, critic, workspace, nb_rows);
  const double count = (double)nb_rows * (double)critic->num_out;
  a.target = target, a.value = value, a.advantage = advantage, a.inv = nb_rows > 0 ? (float)(1.0 / count) : 0.0f;
  if (nb_rows > 0 && launch_rows<true>(a, lib_cap(max_workgroups), st) != MDR_OK) return MDR_ERR_HIP;
  wa.state = state, wa.ld = ld_state, wa.index = index, wa.count = (float)count, wa.grad = grad, wa.loss = loss;
  return launch_weights(wa, max_workgroups, st);
}

}  // extern "C"
