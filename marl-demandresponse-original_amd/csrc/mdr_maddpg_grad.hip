// MADDPG's update step (include/mdr_policy.h: mdr_maddpg_target, mdr_maddpg_critic_grad, mdr_maddpg_actor_grad): the wide joint critic
// and the gumbel-softmax actor of agents/ddpg.py:305-339, weights streamed from L2.
//
// Reference: MADDPG.update evaluates, per agent a, the target actor on every agent's next state (a hard gumbel-softmax pick each), the
// target critic on cat(next states, picks), the critic's mse loss against y = r_a + gamma Q', and the actor's loss -mean Q(states,
// actions with a's replaced by its own straight-through sample) + 1e-3 mean(logits^2).  Both nets are DDPG_Network
// (agents/network.py:80-100): Linear - ReLU - Linear - ReLU - Linear with 256 hidden units, the critic on J = N (F + 2) inputs - 1060 at
// the reference's 20 agents.  W1 is then 1 MB and W2 256 KB: neither fits the 160 KB of LDS mdr_ppo_grad.hip keeps its weights in, and one
// partial gradient per workgroup would be 1.4 MB each.  So this family has two kinds of kernel:
//
//   row pass     one workgroup of 16 waves per tile of 16 minibatch rows.  Wave w owns the 16-unit block w of every hidden layer (H <=
//                256: at most 16 blocks).  The MFMA A operand - the weights, torch's [out][in] layout - comes from global memory (L2): a
//                workgroup meets every weight once per tile, so staging it in LDS buys no reuse.  The B operand - the tile's activations,
//                transposed [unit][row] with row stride LT = 20 - comes from LDS; the joint input is staged in chunks of KC = 128
//                columns while the first layer's accumulators stay in registers.  Everything of a row happens here: forward, the head
//                (pick / TD target / mse / the actor's loss), the backward down to dz1.  What the weight gradients need - h1, h2, dz1,
//                dz2 [row][unit], dlogits, the rows' loss terms - is left in the workspace.
//   weight pass  one wave per 16 x 16 block of a weight gradient: dW[m][n] = sum_r dz[r][m] in[r][n] over the minibatch rows in row
//                order, k = the rows on v_mfma_f32_16x16x4_f32 - no partials, no floating-point atomics, the same bits whatever the
//                grid.  The first layer's input is gathered again from `state` / `action` through `index`, never stored.  The blocks
//                of column 0 also take the bias (the same product against ones); one more wave sums the loss terms.
//
// With one net of a kind per agent (mdr_maddpg_target_all, mdr_maddpg_critic_grad_all, mdr_maddpg_actor_grad_all) both passes take the
// agent as a grid axis - row-pass tile t is tile t mod TB of agent t / TB, a weight-pass block's agent is blockIdx.y - and run the
// same bodies on that agent's slices: N times the workgroups per launch, the bits of the N single-agent calls.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 (A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: col = l & 15, row = 4 (l >> 4) +
// reg).  relu'(z) = 1 iff z > 0 iff relu(z) > 0, so the backward reads the activations, not z.  Rows past the minibatch are forwarded as
// zero inputs and given zero dlogits: they add exact zeros.  The 1 / B of the mean sits in dlogits, as autograd has it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/mdr.h"
#include "../../include/mdr_policy.h"
#include "mdr_stream_mlp.h"

namespace {

using namespace mdr_stream;

constexpr int NW = 16;                // waves per row-pass workgroup = the most 16-unit blocks of a hidden layer
constexpr int TILE = 16;              // minibatch rows per tile
constexpr int MAX_F = 64, MAX_H = 256, MAX_J = 1280;
constexpr int WW = 4;                 // waves per weight-pass workgroup
constexpr int UNR_W = 8;              // weight pass: MFMA k-steps whose global operands are loaded together

// LDS of the row pass (floats): the input chunk, four activation images, the heads' partial sums, the tile's picks
constexpr int S_X = 0, S_A0 = S_X + KC * LT, S_A1 = S_A0 + MAX_H * LT, S_C0 = S_A1 + MAX_H * LT, S_C1 = S_C0 + MAX_H * LT,
              S_LP = S_C1 + MAX_H * LT, S_PK = S_LP + NW * TILE * 2, S_END = S_PK + TILE;

struct Net {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int K, H1, H2, O;
};

// MODE_PICK_AGENTS: the picks with one target actor per agent (mdr_maddpg_target_agents) - tiles of 16 minibatch rows of ONE agent
// MODE_*_ALL: the target critic, the critic's step and the actor's step of ALL agents in one launch, one net of a kind per agent
// (mdr_maddpg_target_all, mdr_maddpg_critic_grad_all, mdr_maddpg_actor_grad_all): tile t is tile t mod TB of agent t / TB's own
// minibatch and does what the mode without _ALL does for that agent on that agent's slices - the same instructions, hence the same bits
enum Mode : int {
  MODE_PICK = 0,
  MODE_TARGET = 1,
  MODE_CRITIC = 2,
  MODE_ACTOR = 3,
  MODE_PICK_AGENTS = 4,
  MODE_TARGET_ALL = 5,
  MODE_CRITIC_ALL = 6,
  MODE_ACTOR_ALL = 7
};
constexpr bool all_agents(Mode m) { return m >= MODE_TARGET_ALL; }
constexpr Mode per_agent_mode(Mode m) { return all_agents(m) ? (Mode)(m - MODE_TARGET_ALL + MODE_TARGET) : m; }

struct RowArgs {
  Net actor, critic;
  const float* state;         // the buffer's state (next_state for the target): env-step j at state + j * ld
  int64_t ld;
  const int64_t* action;      // [env-steps][N]
  const int64_t* index;
  int64_t B;                  // minibatch rows
  int64_t R, ntiles;          // rows of this launch (MODE_PICK: B * N) and its tiles
  int N, F, agent;
  const float* noise;         // MODE_PICK: [B][N][2]; MODE_ACTOR: [B][2]
  float tau, gamma, pse, invB;
  const float* reward;        // [env-steps][N]
  const float* y;             // MODE_CRITIC: [B]
  uint8_t* picks;             // [B][N]: MODE_PICK writes, MODE_TARGET reads
  float *out0, *out1;         // TARGET: y, next_q; CRITIC: q; ACTOR: q, logits
  float *h1, *h2, *dz1, *dz2, *dl, *term;      // workspace of the net whose gradient is taken: [Rp][H1p], [Rp][H2p], ..., [Rp][2], [Rp]
};

// MODE_PICK_AGENTS: the nets' pointers travel in the kernel argument block (32 x 48 bytes: no device table to own); the shapes are
// those of r.actor.  Tile t: agent k = t / TB, minibatch rows 16 (t mod TB) + c - the MFMA A operand, the weights, is one net's
struct NetPtrs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};
struct PickAgentsArgs {
  RowArgs r;
  int64_t TB;      // tiles per agent: ceil(B / 16)
  NetPtrs nets[MDR_MAX_AGENT_NETS];
};
// MODE_*_ALL: r holds what the agents share (the shapes in r.actor / r.critic, the buffer, B, the scalars) and the bases of the
// per-agent arrays - index [N][B], noise [N][B][2], y / q [N][B], logits [N][B][2], picks [N][B][N], the workspace images, each
// agent's ws floats apart; agent a's tiles shift them by a.  critics: the net the critic's input goes through (TARGET_ALL: the
// target critics); actors: MODE_ACTOR_ALL only.  12 x 32 pointers and r: 3.4 KB of the 4 KB argument block
struct AllAgentsArgs {
  RowArgs r;
  int64_t TB;      // tiles per agent: ceil(B / 16)
  int64_t ws;      // floats of one agent's workspace
  NetPtrs critics[MDR_MAX_AGENT_NETS];
  NetPtrs actors[MDR_MAX_AGENT_NETS];
};
template <Mode MODE>
using ArgsOf = std::conditional_t<MODE == MODE_PICK_AGENTS, PickAgentsArgs, RowArgs>;
__host__ __device__ __forceinline__ const RowArgs& row_args(const RowArgs& a) { return a; }
__host__ __device__ __forceinline__ const RowArgs& row_args(const PickAgentsArgs& a) { return a.r; }
__host__ __device__ __forceinline__ const RowArgs& row_args(const AllAgentsArgs& a) { return a.r; }

__device__ __forceinline__ void set_ptrs(Net& n, const NetPtrs& p) { n.w1 = p.w1, n.b1 = p.b1, n.w2 = p.w2, n.b2 = p.b2, n.w3 = p.w3, n.b3 = p.b3; }

// the wave's share of two dot products over its block of vT: sum_u coef_o[u * su] vT[u][row c] -> lp[w][row][o]
__device__ __forceinline__ void dot2_share(const float* vT, const float* __restrict__ coef0, const float* __restrict__ coef1, int64_t su, int H, float* lp,
                                           int w, int c, int g) {
  float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = 16 * w + 4 * g + i;
    if (u < H) {
      const float v = vT[u * LT + c];
      p0 = fmaf(coef0[u * su], v, p0);
      if (coef1) p1 = fmaf(coef1[u * su], v, p1);
    }
  }
  p0 += __shfl_xor(p0, 16);
  p0 += __shfl_xor(p0, 32);
  p1 += __shfl_xor(p1, 16);
  p1 += __shfl_xor(p1, 32);
  if (g == 0) {
    lp[(w * TILE + c) * 2] = p0;
    lp[(w * TILE + c) * 2 + 1] = p1;
  }
}

// the blocks' shares in block order: the same bits in every lane of row c
__device__ __forceinline__ void dot2_sum(const float* lp, int nb, int c, float& s0, float& s1) {
  s0 = 0.0f, s1 = 0.0f;
  for (int b = 0; b < nb; ++b) {
    s0 += lp[(b * TILE + c) * 2];
    s1 += lp[(b * TILE + c) * 2 + 1];
  }
}

// the tiles blockIdx.x, + gridDim.x, ... of a row pass: the body of k_maddpg_rows and k_maddpg_rows_all
template <Mode FULL, class Args>
__device__ __forceinline__ void maddpg_rows(const Args args) {
  constexpr Mode MODE = per_agent_mode(FULL);      // what a tile does
  constexpr bool ALL = all_agents(FULL);           // ... for the agent the tile belongs to
  const RowArgs& a0 = row_args(args);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  float* xT = lds + S_X;
  float* a0T = lds + S_A0;      // the actor's h1, then dz1
  float* a1T = lds + S_A1;      // the actor's h2, then dz2
  float* c0T = lds + S_C0;      // the critic's h1, then dz1
  float* c1T = lds + S_C1;      // the critic's h2, then dz2
  float* lp = lds + S_LP;
  float* pk = lds + S_PK;       // MODE_ACTOR: the tile's picks of agent a, 0 / 1
  // weights in flight per wave (MFMA k-steps loaded together); the actor's step holds more live state, so fewer fit its 128 registers
  constexpr int UNR = MODE == MODE_ACTOR ? 4 : 8;
  constexpr bool AGENTS = MODE == MODE_PICK_AGENTS;
  constexpr bool PICKS = MODE == MODE_PICK || AGENTS;
  constexpr bool HAS_ACTOR = PICKS || MODE == MODE_ACTOR;
  constexpr bool HAS_CRITIC = !PICKS;
  const int NF = a0.N * a0.F;

  for (int64_t t = blockIdx.x; t < a0.ntiles; t += gridDim.x) {
    int64_t tl = t;                  // the tile's number among the tiles of its rows
    [[maybe_unused]] RowArgs mine;   // ALL: the arguments of the tile's agent
    const RowArgs* ap = &a0;
    if constexpr (ALL) {
      // agent ag's tile tl: every per-agent array shifted to slice ag, the nets' pointers from the tables - read through the
      // argument block's own address, as MODE_PICK_AGENTS reads its table
      const int ag = (int)(t / args.TB);
      tl = t - ag * args.TB;
      mine = a0;
      const char* seg = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
      set_ptrs(mine.critic, reinterpret_cast<const NetPtrs*>(seg + offsetof(AllAgentsArgs, critics))[ag]);
      if constexpr (MODE == MODE_ACTOR) set_ptrs(mine.actor, reinterpret_cast<const NetPtrs*>(seg + offsetof(AllAgentsArgs, actors))[ag]);
      const int64_t o = ag * a0.B;
      mine.agent = ag;
      mine.index += o;
      if constexpr (MODE == MODE_TARGET) mine.picks += o * a0.N, mine.out0 += o;
      if constexpr (MODE == MODE_CRITIC) mine.y += o;
      if constexpr (MODE == MODE_ACTOR) mine.noise += 2 * o;
      if (MODE != MODE_TARGET && mine.out0) mine.out0 += o;
      if (mine.out1) mine.out1 += MODE == MODE_ACTOR ? 2 * o : o;
      if constexpr (MODE != MODE_TARGET) {
        const int64_t wo = ag * args.ws;
        mine.h1 += wo, mine.dz1 += wo, mine.h2 += wo, mine.dz2 += wo, mine.dl += wo, mine.term += wo;
      }
      ap = &mine;
    }
    const RowArgs& a = *ap;
    const Net& A0 = a.actor;
    const Net& Cn = a.critic;
    int64_t row = tl * TILE + c;     // the row this lane's MFMA column and head work belong to
    bool valid = row < a.R;
    Net A = A0;
    [[maybe_unused]] int kt = 0;         // AGENTS: the tile's agent and its first minibatch row
    [[maybe_unused]] int64_t i0 = 0;
    if constexpr (AGENTS) {
      kt = (int)(t / args.TB);
      i0 = (t - kt * args.TB) * TILE;
      valid = i0 + c < a.B;
      row = (i0 + c) * a.N + kt;      // of noise and picks: [B][N]
      // the table is read through the argument block's own address (its first argument starts the block): indexing the by-value
      // parameter by a variable would copy all of it to private memory
      const char* seg = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
      const NetPtrs net = reinterpret_cast<const NetPtrs*>(seg + offsetof(PickAgentsArgs, nets))[kt];
      A.w1 = net.w1, A.b1 = net.b1, A.w2 = net.w2, A.b2 = net.b2, A.w3 = net.w3, A.b3 = net.b3;
    }
    float l0 = 0.0f, l1 = 0.0f, p0 = 0.0f, p1 = 0.0f;
    bool pick = false;

    if constexpr (HAS_ACTOR) {
      // ---- the actor's input: F floats of agent k of env-step j
      for (int e = tid; e < TILE * MAX_F; e += 64 * NW) {
        const int r = e / MAX_F, f = e - r * MAX_F;
        const int64_t rr = tl * TILE + r;
        float v = 0.0f;
        if (f < a.F && (AGENTS ? i0 + r < a.B : rr < a.R)) {
          const int64_t i = AGENTS ? i0 + r : MODE == MODE_PICK ? rr / a.N : rr;
          const int k = AGENTS ? kt : MODE == MODE_PICK ? (int)(rr - i * a.N) : a.agent;
          const int64_t j = a.index ? a.index[i] : i;
          v = a.state[j * a.ld + (int64_t)k * a.F + f];
        }
        xT[f * LT + r] = v;
      }
      __syncthreads();
      const int nb1 = blocks16(A.H1), nb2 = blocks16(A.H2);
      float* wsh1 = MODE == MODE_ACTOR ? a.h1 : nullptr;
      float* wsh2 = MODE == MODE_ACTOR ? a.h2 : nullptr;
      if (w < nb1) {
        f32x4 acc = bias_block(A.b1, A.H1, 16 * w, g);
        fwd_accum<UNR>(acc, A.w1, A.K, A.H1, 16 * w, 0, A.K, xT, c, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.0f);
        store_block(acc, a0T, wsh1, 16 * nb1, row, 16 * w, c, g);
      }
      __syncthreads();
      if (w < nb2) {
        f32x4 acc = bias_block(A.b2, A.H2, 16 * w, g);
        fwd_accum<UNR>(acc, A.w2, A.H1, A.H2, 16 * w, 0, A.H1, a0T, c, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.0f);
        store_block(acc, a1T, wsh2, 16 * nb2, row, 16 * w, c, g);
        dot2_share(a1T, A.w3, A.w3 + A.H2, 1, A.H2, lp, w, c, g);      // the lane's own four units: its own stores
      }
      __syncthreads();
      dot2_sum(lp, nb2, c, l0, l1);
      l0 += A.b3[0];
      l1 += A.b3[1];
      // F.gumbel_softmax(logits, tau, hard=True): t = (logits + g) / tau, the pick its argmax (a tie: action 0), p = softmax(t)
      float t0 = 0.0f, t1 = 0.0f;
      if (valid) {
        const float sum0 = l0 + a.noise[row * 2], sum1 = l1 + a.noise[row * 2 + 1];
        t0 = sum0 / a.tau;
        t1 = sum1 / a.tau;
      }
      pick = t1 > t0;
      if constexpr (PICKS) {
        if (valid && w == 0 && g == 0) a.picks[row] = pick ? 1 : 0;
        __syncthreads();      // xT, lp and the images are rewritten by the next tile
        continue;
      }
      p1 = 1.0f / (1.0f + expf(t0 - t1));
      p0 = 1.0f / (1.0f + expf(t1 - t0));
      if (w == 0 && g == 0) pk[c] = pick ? 1.0f : 0.0f;
      if (valid && w == 0 && g == 0 && a.out1) {
        a.out1[row * 2] = l0;
        a.out1[row * 2 + 1] = l1;
      }
    }

    if constexpr (HAS_CRITIC) {
      const int nb1 = blocks16(Cn.H1), nb2 = blocks16(Cn.H2);
      const int J = Cn.K;
      float* wsh1 = MODE == MODE_CRITIC ? a.h1 : nullptr;
      float* wsh2 = MODE == MODE_CRITIC ? a.h2 : nullptr;
      // ---- F1 over the joint input x = state_j (N F floats) | onehot(action of agent 0) | ... in chunks of KC columns
      f32x4 acc = bias_block(Cn.b1, Cn.H1, 16 * w, g);
      for (int k0 = 0; k0 < J; k0 += KC) {
        const int kn = J - k0 < KC ? J - k0 : KC;
        __syncthreads();      // the chunk before (or the actor's input, or pk) is read
        for (int e = tid; e < TILE * KC; e += 64 * NW) {
          const int r = e / KC, f = e - r * KC, col = k0 + f;
          const int64_t rr = tl * TILE + r;
          float v = 0.0f;
          if (col < J && rr < a.B) {
            const int64_t j = a.index ? a.index[rr] : rr;
            if (col < NF) {
              v = a.state[j * a.ld + col];
            } else {
              const int k = (col - NF) >> 1, bit = (col - NF) & 1;
              int act;
              if (MODE == MODE_TARGET) act = a.picks[rr * a.N + k] != 0;
              else if (MODE == MODE_ACTOR && k == a.agent) act = pk[r] != 0.0f;
              else act = a.action[j * a.N + k] != 0;
              v = act == bit ? 1.0f : 0.0f;
            }
          }
          xT[f * LT + r] = v;
        }
        __syncthreads();
        if (w < nb1) fwd_accum<UNR>(acc, Cn.w1, J, Cn.H1, 16 * w, k0, kn, xT, c, g);
      }
      if (w < nb1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.0f);
        store_block(acc, c0T, wsh1, 16 * nb1, row, 16 * w, c, g);
      }
      __syncthreads();
      if (w < nb2) {
        f32x4 z = bias_block(Cn.b2, Cn.H2, 16 * w, g);
        fwd_accum<UNR>(z, Cn.w2, Cn.H1, Cn.H2, 16 * w, 0, Cn.H1, c0T, c, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = fmaxf(z[i], 0.0f);
        store_block(z, c1T, wsh2, 16 * nb2, row, 16 * w, c, g);
        dot2_share(c1T, Cn.w3, nullptr, 1, Cn.H2, lp, w, c, g);
      }
      __syncthreads();
      float q, unused;
      dot2_sum(lp, nb2, c, q, unused);
      q += Cn.b3[0];

      if constexpr (MODE == MODE_TARGET) {
        // ddpg.py:317-322: y = reward_a + gamma Q'; the product and the sum are two statements, each rounds on its own
        if (valid && w == 0 && g == 0) {
          const int64_t j = a.index ? a.index[row] : row;
          const float discounted = a.gamma * q;
          a.out0[row] = a.reward[j * a.N + a.agent] + discounted;
          if (a.out1) a.out1[row] = q;
        }
        __syncthreads();
        continue;
      }

      // ---- the head: d loss / d q of the row
      float dq = 0.0f, term = 0.0f;
      if (valid) {
        if constexpr (MODE == MODE_CRITIC) {
          const float delta = q - a.y[row];      // F.mse_loss(q, y)
          term = delta * delta;
          const float twice = 2.0f * delta;
          dq = twice * a.invB;
        } else {
          dq = -a.invB;                          // -critic(...).mean()
        }
        if (w == 0 && g == 0 && a.out0) a.out0[row] = q;
      }
      // dz2 = relu'(z2) dq W3, in place of h2's image
      if (w < nb2) {
        f32x4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int u = 16 * w + 4 * g + i;
          d[i] = (u < Cn.H2 && c1T[u * LT + c] > 0.0f) ? dq * Cn.w3[u] : 0.0f;
        }
        store_block(d, c1T, MODE == MODE_CRITIC ? a.dz2 : nullptr, 16 * nb2, row, 16 * w, c, g);
      }
      __syncthreads();
      if (w < nb1) bwd_block<UNR>(Cn.w2, Cn.H2, Cn.H1, 16 * w, c1T, c0T, MODE == MODE_CRITIC ? a.dz1 : nullptr, 16 * nb1, row, c, g);

      if constexpr (MODE == MODE_CRITIC) {
        if (w == 0 && g == 0) {
          a.dl[row * 2] = dq;
          a.dl[row * 2 + 1] = 0.0f;
          a.term[row] = term;
        }
        __syncthreads();
        continue;
      }

      if constexpr (MODE == MODE_ACTOR) {
        // c_o = dz1 . W1[:, N F + 2 a + o]: the two input columns the actor's sample feeds, nothing else of W1^T dz1
        const float* col0 = Cn.w1 + NF + 2 * a.agent;
        if (w < nb1) dot2_share(c0T, col0, col0 + 1, J, Cn.H1, lp, w, c, g);      // the lane's own stores of bwd_block
        __syncthreads();
        float cc0, cc1;
        dot2_sum(lp, nb1, c, cc0, cc1);
        // through y_soft = softmax(t): dl_0 = p0 p1 (c0 - c1) / tau + pse l0 / B, dl_1 the negative + pse l1 / B
        float d0 = 0.0f, d1 = 0.0f;
        if (valid) {
          const float pp = p0 * p1;
          const float diff = cc0 - cc1;
          const float s = pp * diff / a.tau;
          const float r0 = a.pse * l0 * a.invB, r1 = a.pse * l1 * a.invB;
          d0 = s + r0;
          d1 = r1 - s;
          const float sq = l0 * l0 + l1 * l1;
          term = 0.5f * a.pse * sq - q;
        }
        const int nba1 = blocks16(A.H1), nba2 = blocks16(A.H2);
        if (w < nba2) {
          f32x4 d;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int u = 16 * w + 4 * g + i;
            d[i] = (u < A.H2 && a1T[u * LT + c] > 0.0f) ? fmaf(d0, A.w3[u], d1 * A.w3[A.H2 + u]) : 0.0f;
          }
          store_block(d, a1T, a.dz2, 16 * nba2, row, 16 * w, c, g);
        }
        __syncthreads();
        if (w < nba1) bwd_block<UNR>(A.w2, A.H2, A.H1, 16 * w, a1T, a0T, a.dz1, 16 * nba1, row, c, g);
        if (w == 0 && g == 0) {
          a.dl[row * 2] = d0;
          a.dl[row * 2 + 1] = d1;
          a.term[row] = term;
        }
        __syncthreads();
      }
    }
  }
}

template <Mode MODE>
__global__ __launch_bounds__(64 * NW) void k_maddpg_rows(ArgsOf<MODE> args) {
  maddpg_rows<MODE>(args);
}

template <Mode MODE>
__global__ __launch_bounds__(64 * NW) void k_maddpg_rows_all(AllAgentsArgs args) {
  maddpg_rows<MODE>(args);
}

// ---- the weight pass
struct WeightArgs {
  int K, H1, H2, O;            // of the net whose gradient is taken
  int H1p, H2p;
  const float *h1, *h2, *dz1, *dz2, *dl, *term;
  const float* state;
  int64_t ld;
  const int64_t* action;
  const int64_t* index;
  int64_t B, Bp;
  int N, F, agent;             // agent < 0: the joint input (the critic's); else the F floats of that agent (the actor's)
  float* grad;
  float* loss;
  int nbk, nb1, nb2;           // 16-blocks of K, H1, H2
};

// the blocks blockIdx.x * WW + wave, + gridDim.x * WW, ... of the gradient `a` describes
__device__ __forceinline__ void weight_blocks(const WeightArgs a) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int n1 = a.nb1 * a.nbk, n2 = a.nb2 * a.nb1, n3 = a.nb2;
  const int total = n1 + n2 + n3 + 1;
  const int oW1 = 0, ob1 = a.H1 * a.K, oW2 = ob1 + a.H1, ob2 = oW2 + a.H2 * a.H1, oW3 = ob2 + a.H2, ob3 = oW3 + a.O * a.H2;
  const int NF = a.N * a.F;
  for (int blk = blockIdx.x * WW + w; blk < total; blk += gridDim.x * WW) {
    if (blk == total - 1) {
      // the loss: 64 strided sums, added as a tree across the lanes (every lane ends on the same sum).  A chain in lane order
      // carried the rounding of a running sum B times the mean term: off by two float32 spacings of the loss at B = 24, where
      // torch's pairwise mean is within a third of one (profiles/learner_golden_README.md)
      float s = 0.0f;
      for (int64_t r = lane; r < a.B; r += 64) s += a.term[r];
      float sum = s;
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      if (lane == 0) *a.loss = a.B > 0 ? sum / (float)a.B : 0.0f;
      continue;
    }
    int layer, mb, nbk;
    if (blk < n1) layer = 0, mb = blk / a.nbk, nbk = blk - mb * a.nbk;
    else if (blk < n1 + n2) layer = 1, mb = (blk - n1) / a.nb1, nbk = (blk - n1) - mb * a.nb1;
    else layer = 2, mb = 0, nbk = blk - n1 - n2;
    const int M = layer == 0 ? a.H1 : layer == 1 ? a.H2 : a.O;
    const int Nn = layer == 0 ? a.K : layer == 1 ? a.H1 : a.H2;
    const float* dz = layer == 0 ? a.dz1 : layer == 1 ? a.dz2 : a.dl;
    const int ldz = layer == 0 ? a.H1p : layer == 1 ? a.H2p : 2;
    const float* in = layer == 1 ? a.h1 : a.h2;
    const int lin = layer == 1 ? a.H1p : a.H2p;
    const int m = 16 * mb + c, n = 16 * nbk + c;
    const bool mok = m < M, nok = n < Nn;
    f32x4 acc = {0, 0, 0, 0}, accb = {0, 0, 0, 0};
    for (int64_t r0 = 0; r0 < a.Bp; r0 += 4 * UNR_W) {      // UNR_W k-steps of four rows, their operands in flight together
      float av[UNR_W], bv[UNR_W];
#pragma unroll
      for (int i = 0; i < UNR_W; ++i) {
        const int64_t r = r0 + 4 * i + g;
        av[i] = 0.0f, bv[i] = 0.0f;
        if (r < a.Bp) {
          if (mok) av[i] = dz[r * ldz + m];
          if (layer != 0) {
            if (nok) bv[i] = in[r * lin + n];
          } else if (nok && r < a.B) {
            const int64_t j = a.index ? a.index[r] : r;
            if (a.agent >= 0) bv[i] = a.state[j * a.ld + (int64_t)a.agent * a.F + n];
            else if (n < NF) bv[i] = a.state[j * a.ld + n];
            else bv[i] = ((a.action[j * a.N + ((n - NF) >> 1)] != 0) == (bool)((n - NF) & 1)) ? 1.0f : 0.0f;
          }
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

__global__ __launch_bounds__(64 * WW) void k_maddpg_weights(WeightArgs a) { weight_blocks(a); }

// the weight pass of all agents (mdr_maddpg_critic_grad_all, mdr_maddpg_actor_grad_all): blockIdx.y is the agent; its workspace, its
// minibatch, its slice of grad [N][G] and of loss [N] lie one stride each behind agent 0's, which `w` describes
struct WeightAllArgs {
  WeightArgs w;
  int64_t ws, G;      // floats of one agent's workspace and of one gradient
  int actor;          // the actor's step: agent y's input is its own F floats (WeightArgs::agent = y)
};

__global__ __launch_bounds__(64 * WW) void k_maddpg_weights_all(WeightAllArgs b) {
  const int64_t y = blockIdx.y;
  WeightArgs a = b.w;
  const int64_t wo = y * b.ws;
  a.h1 += wo, a.h2 += wo, a.dz1 += wo, a.dz2 += wo, a.dl += wo, a.term += wo;
  a.index += y * a.B;
  a.agent = b.actor ? (int)y : -1;
  a.grad += y * b.G;
  a.loss += y;
  weight_blocks(a);
}

bool fields_ok(const mdr_mlp_t* n) {
  return n && n->struct_size == sizeof(mdr_mlp_t) && n->num_state > 0 && n->hidden1 > 0 && n->hidden2 > 0 && n->num_out > 0;
}
bool pointers_ok(const mdr_mlp_t* n) { return n->w1 && n->b1 && n->w2 && n->b2 && n->w3 && n->b3; }
bool covered(const mdr_mlp_t* n) {
  return n->num_state <= MAX_J && n->hidden1 <= MAX_H && n->hidden2 <= MAX_H && (n->num_out == 1 || n->num_out == 2);
}
// MDR_OK, MDR_ERR_INVALID or MDR_ERR_UNSUPPORTED for the pair of nets of one call (actor may be null: the critic's step)
int pair_shape(const mdr_mlp_t* actor, const mdr_mlp_t* critic, int32_t nb_agents) {
  if ((actor && !fields_ok(actor)) || !fields_ok(critic) || nb_agents < 1) return MDR_ERR_INVALID;
  if (critic->num_state % nb_agents != 0 || critic->num_state / nb_agents < 3) return MDR_ERR_INVALID;      // J = N (F + 2), F >= 1
  const int F = critic->num_state / nb_agents - 2;
  if (actor && actor->num_state != F) return MDR_ERR_INVALID;
  if (!covered(critic) || critic->num_out != 1 || F > MAX_F) return MDR_ERR_UNSUPPORTED;
  if (actor && (!covered(actor) || actor->num_out != 2)) return MDR_ERR_UNSUPPORTED;
  return MDR_OK;
}

Net make_net(const mdr_mlp_t* n) { return Net{n->w1, n->b1, n->w2, n->b2, n->w3, n->b3, n->num_state, n->hidden1, n->hidden2, n->num_out}; }

int64_t grad_floats(const mdr_mlp_t* n) {
  return (int64_t)n->hidden1 * n->num_state + n->hidden1 + (int64_t)n->hidden2 * n->hidden1 + n->hidden2 + (int64_t)n->num_out * n->hidden2 + n->num_out;
}

// floats of the workspace the gradient of `n` over nb_rows rows takes: h1, dz1 [Bp][H1p], h2, dz2 [Bp][H2p], dl [Bp][2], term [Bp]
int64_t ws_floats(const mdr_mlp_t* n, int64_t nb_rows) {
  const int64_t Bp = pad16(nb_rows);
  return Bp * (2 * pad16(n->hidden1) + 2 * pad16(n->hidden2) + 3);
}

template <Mode MODE, class Args>
int launch_rows(const Args& args, int cap, hipStream_t st) {
  const RowArgs& a = row_args(args);
  const size_t bytes = (size_t)S_END * sizeof(float);
  void (*kernel)(Args);
  if constexpr (all_agents(MODE)) kernel = k_maddpg_rows_all<MODE>;
  else kernel = k_maddpg_rows<MODE>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MDR_ERR_HIP;
  const int64_t grid = a.ntiles < cap ? a.ntiles : cap;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * NW), bytes, st, args);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

void carve(RowArgs& r, WeightArgs& wa, const mdr_mlp_t* n, void* workspace, int64_t nb_rows) {
  const int64_t Bp = pad16(nb_rows), H1p = pad16(n->hidden1), H2p = pad16(n->hidden2);
  float* p = static_cast<float*>(workspace);
  r.h1 = p, p += Bp * H1p;
  r.dz1 = p, p += Bp * H1p;
  r.h2 = p, p += Bp * H2p;
  r.dz2 = p, p += Bp * H2p;
  r.dl = p, p += Bp * 2;
  r.term = p;
  wa.K = n->num_state, wa.H1 = n->hidden1, wa.H2 = n->hidden2, wa.O = n->num_out, wa.H1p = (int)H1p, wa.H2p = (int)H2p;
  wa.h1 = r.h1, wa.h2 = r.h2, wa.dz1 = r.dz1, wa.dz2 = r.dz2, wa.dl = r.dl, wa.term = r.term;
  wa.B = nb_rows, wa.Bp = Bp;
  wa.nbk = blocks16(n->num_state), wa.nb1 = blocks16(n->hidden1), wa.nb2 = blocks16(n->hidden2);
}

int launch_weights(const WeightArgs& wa, int cap, hipStream_t st) {
  const int total = wa.nb1 * wa.nbk + wa.nb2 * wa.nb1 + wa.nb2 + 1;
  int grid = (total + WW - 1) / WW;
  // max_workgroups bounds this pass as well; the library's own choice leaves every block its own wave
  if (cap > 0 && grid > cap) grid = cap;
  hipLaunchKernelGGL(k_maddpg_weights, dim3((unsigned)grid), dim3(64 * WW), 0, st, wa);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

int launch_weights_all(const WeightAllArgs& b, int nb_agents, int cap, hipStream_t st) {
  const int total = b.w.nb1 * b.w.nbk + b.w.nb2 * b.w.nb1 + b.w.nb2 + 1;
  int grid = (total + WW - 1) / WW;
  if (cap > 0 && grid > cap) grid = cap;      // max_workgroups bounds the workgroups of ONE agent here: the agent is the grid's y
  hipLaunchKernelGGL(k_maddpg_weights_all, dim3((unsigned)grid, (unsigned)nb_agents), dim3(64 * WW), 0, st, b);
  return hipGetLastError() == hipSuccess ? MDR_OK : MDR_ERR_HIP;
}

// The nets of the _all calls, one of a kind per agent, 1 <= nb_agents <= MDR_MAX_AGENT_NETS (actors may be null: the critic's step).
// MDR_ERR_INVALID: a refusal; otherwise pair_shape of agent 0's pair, for the caller to return after its own argument checks
int all_fields(const mdr_mlp_t* actors, const mdr_mlp_t* critics, int32_t nb_agents) {
  for (int k = 0; k < nb_agents; ++k)
    if ((actors && !fields_ok(&actors[k])) || !fields_ok(&critics[k])) return MDR_ERR_INVALID;
  const int rc = pair_shape(actors ? &actors[0] : nullptr, &critics[0], nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  for (int k = 0; k < nb_agents; ++k)
    if ((actors && !pointers_ok(&actors[k])) || !pointers_ok(&critics[k])) return MDR_ERR_INVALID;
  return rc;
}

bool one_shape(const mdr_mlp_t* nets, int32_t nb) {
  for (int k = 1; k < nb; ++k) {
    const mdr_mlp_t &n = nets[k], &n0 = nets[0];
    if (n.num_state != n0.num_state || n.hidden1 != n0.hidden1 || n.hidden2 != n0.hidden2 || n.num_out != n0.num_out) return false;
  }
  return true;
}

void set_table(NetPtrs* table, const mdr_mlp_t* nets, int32_t nb) {
  for (int k = 0; k < nb; ++k) table[k] = NetPtrs{nets[k].w1, nets[k].b1, nets[k].w2, nets[k].b2, nets[k].w3, nets[k].b3};
}

static_assert(sizeof(AllAgentsArgs) <= 4096, "the kernel argument block");

}  // namespace

extern "C" {

int64_t mdr_maddpg_grad_floats(const mdr_mlp_t* net) {
  if (!fields_ok(net) || !covered(net)) return -1;
  return grad_floats(net);
}

int64_t mdr_maddpg_workspace_bytes(const mdr_mlp_t* actor, const mdr_mlp_t* critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups) {
  if (!actor || pair_shape(actor, critic, nb_agents) != MDR_OK || nb_rows < 0 || max_workgroups < 0) return -1;
  const int64_t fa = ws_floats(actor, nb_rows), fc = ws_floats(critic, nb_rows);
  const int64_t f = fa > fc ? fa : fc;
  return (f > 4 ? f : 4) * (int64_t)sizeof(float);
}

int mdr_maddpg_target(const mdr_mlp_t* tgt_actor, const mdr_mlp_t* tgt_critic, const float* next_state, int64_t ld_state, const float* reward,
                      const int64_t* index, int64_t nb_rows, int32_t nb_agents, int32_t agent, const float* noise, float tau, float gamma,
                      int32_t max_workgroups, float* y, float* next_q, uint8_t* next_action, void* stream) {
  if (!tgt_actor || !next_state || !reward || !noise || !y || !next_action) return MDR_ERR_INVALID;
  const int rc = pair_shape(tgt_actor, tgt_critic, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(tgt_actor) || !pointers_ok(tgt_critic)) return MDR_ERR_INVALID;
  const int F = tgt_actor->num_state;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F || agent < 0 || agent >= nb_agents) return MDR_ERR_INVALID;
  if (!(tau > 0.0f) || !(fabsf(tau) <= FLT_MAX) || !(fabsf(gamma) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (nb_rows == 0) return MDR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  RowArgs a{};
  a.actor = make_net(tgt_actor), a.critic = make_net(tgt_critic);
  a.state = next_state, a.ld = ld_state, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F, a.agent = agent;
  a.noise = noise, a.tau = tau, a.gamma = gamma, a.reward = reward, a.picks = next_action, a.out0 = y, a.out1 = next_q;
  a.R = nb_rows * nb_agents, a.ntiles = (a.R + TILE - 1) / TILE;
  if (launch_rows<MODE_PICK>(a, cap, st) != MDR_OK) return MDR_ERR_HIP;
  a.R = nb_rows, a.ntiles = (a.R + TILE - 1) / TILE;
  return launch_rows<MODE_TARGET>(a, cap, st);
}

int mdr_maddpg_target_agents(const mdr_mlp_t* tgt_actors, int32_t nb_nets, const mdr_mlp_t* tgt_critic, const float* next_state,
                             int64_t ld_state, const float* reward, const int64_t* index, int64_t nb_rows, int32_t nb_agents, int32_t agent,
                             const float* noise, float tau, float gamma, int32_t max_workgroups, float* y, float* next_q,
                             uint8_t* next_action, void* stream) {
  if (!tgt_actors || !next_state || !reward || !noise || !y || !next_action || nb_nets < 1 || nb_nets != nb_agents) return MDR_ERR_INVALID;
  if (nb_nets > MDR_MAX_AGENT_NETS) return MDR_ERR_UNSUPPORTED;
  for (int k = 0; k < nb_nets; ++k)
    if (!fields_ok(&tgt_actors[k])) return MDR_ERR_INVALID;
  const int rc = pair_shape(&tgt_actors[0], tgt_critic, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(tgt_critic)) return MDR_ERR_INVALID;
  for (int k = 0; k < nb_nets; ++k)
    if (!pointers_ok(&tgt_actors[k])) return MDR_ERR_INVALID;
  const int F = tgt_actors[0].num_state;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F || agent < 0 || agent >= nb_agents) return MDR_ERR_INVALID;
  if (!(tau > 0.0f) || !(fabsf(tau) <= FLT_MAX) || !(fabsf(gamma) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  for (int k = 1; k < nb_nets; ++k) {
    const mdr_mlp_t &n = tgt_actors[k], &n0 = tgt_actors[0];
    if (n.num_state != n0.num_state || n.hidden1 != n0.hidden1 || n.hidden2 != n0.hidden2 || n.num_out != n0.num_out) return MDR_ERR_UNSUPPORTED;
  }
  if (nb_rows == 0) return MDR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  PickAgentsArgs pa{};
  static_assert(sizeof(PickAgentsArgs) <= 4096, "the kernel argument block");
  RowArgs& a = pa.r;
  a.actor = make_net(&tgt_actors[0]), a.critic = make_net(tgt_critic);
  a.state = next_state, a.ld = ld_state, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F, a.agent = agent;
  a.noise = noise, a.tau = tau, a.gamma = gamma, a.reward = reward, a.picks = next_action, a.out0 = y, a.out1 = next_q;
  for (int k = 0; k < nb_nets; ++k)
    pa.nets[k] = NetPtrs{tgt_actors[k].w1, tgt_actors[k].b1, tgt_actors[k].w2, tgt_actors[k].b2, tgt_actors[k].w3, tgt_actors[k].b3};
  // the picks: per agent ceil(B / 16) tiles of that agent's rows, through that agent's own target actor (ddpg.py:282-284)
  pa.TB = (nb_rows + TILE - 1) / TILE;
  a.R = nb_rows * nb_agents, a.ntiles = pa.TB * nb_agents;
  if (launch_rows<MODE_PICK_AGENTS>(pa, cap, st) != MDR_OK) return MDR_ERR_HIP;
  a.R = nb_rows, a.ntiles = (a.R + TILE - 1) / TILE;
  return launch_rows<MODE_TARGET>(a, cap, st);
}

int mdr_maddpg_critic_grad(const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* action, const int64_t* index,
                           int64_t nb_rows, int32_t nb_agents, const float* y, int32_t max_workgroups, void* workspace, float* grad,
                           float* loss, float* q, void* stream) {
  if (!state || !action || !y || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  const int rc = pair_shape(nullptr, critic, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(critic)) return MDR_ERR_INVALID;
  const int F = critic->num_state / nb_agents - 2;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  RowArgs a{};
  WeightArgs wa{};
  carve(a, wa, critic, workspace, nb_rows);
  a.critic = make_net(critic);
  a.state = state, a.ld = ld_state, a.action = action, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F, a.agent = -1;
  a.y = y, a.out0 = q, a.invB = nb_rows > 0 ? 1.0f / (float)nb_rows : 0.0f;
  a.R = nb_rows, a.ntiles = (a.R + TILE - 1) / TILE;
  if (nb_rows > 0 && launch_rows<MODE_CRITIC>(a, cap, st) != MDR_OK) return MDR_ERR_HIP;
  wa.state = state, wa.ld = ld_state, wa.action = action, wa.index = index, wa.N = nb_agents, wa.F = F, wa.agent = -1;
  wa.grad = grad, wa.loss = loss;
  return launch_weights(wa, max_workgroups, st);
}

int mdr_maddpg_actor_grad(const mdr_mlp_t* actor, const mdr_mlp_t* critic, const float* state, int64_t ld_state, const int64_t* action,
                          const int64_t* index, int64_t nb_rows, int32_t nb_agents, int32_t agent, const float* noise, float tau, float pse,
                          int32_t max_workgroups, void* workspace, float* grad, float* loss, float* q, float* logits, void* stream) {
  if (!actor || !state || !action || !noise || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u)) return MDR_ERR_INVALID;
  const int rc = pair_shape(actor, critic, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  if (!pointers_ok(actor) || !pointers_ok(critic)) return MDR_ERR_INVALID;
  const int F = actor->num_state;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F || agent < 0 || agent >= nb_agents) return MDR_ERR_INVALID;
  if (!(tau > 0.0f) || !(fabsf(tau) <= FLT_MAX) || !(fabsf(pse) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  RowArgs a{};
  WeightArgs wa{};
  carve(a, wa, actor, workspace, nb_rows);
  a.actor = make_net(actor), a.critic = make_net(critic);
  a.state = state, a.ld = ld_state, a.action = action, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F, a.agent = agent;
  a.noise = noise, a.tau = tau, a.pse = pse, a.out0 = q, a.out1 = logits, a.invB = nb_rows > 0 ? 1.0f / (float)nb_rows : 0.0f;
  a.R = nb_rows, a.ntiles = (a.R + TILE - 1) / TILE;
  if (nb_rows > 0 && launch_rows<MODE_ACTOR>(a, cap, st) != MDR_OK) return MDR_ERR_HIP;
  wa.state = state, wa.ld = ld_state, wa.action = action, wa.index = index, wa.N = nb_agents, wa.F = F, wa.agent = agent;
  wa.grad = grad, wa.loss = loss;
  return launch_weights(wa, max_workgroups, st);
}

int64_t mdr_maddpg_workspace_bytes_all(const mdr_mlp_t* actor, const mdr_mlp_t* critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups) {
  const int64_t one = mdr_maddpg_workspace_bytes(actor, critic, nb_agents, nb_rows, max_workgroups);
  if (one < 0 || nb_agents > MDR_MAX_AGENT_NETS) return -1;
  const int64_t fa = ws_floats(actor, nb_rows), fc = ws_floats(critic, nb_rows);
  const int64_t f = (fa > fc ? fa : fc) * nb_agents;
  return (f > 4 ? f : 4) * (int64_t)sizeof(float);
}

int mdr_maddpg_target_all(const mdr_mlp_t* tgt_actors, const mdr_mlp_t* tgt_critics, const float* next_state, int64_t ld_state,
                          const float* reward, const int64_t* index, int64_t nb_rows, int32_t nb_agents, const float* noise, float tau,
                          float gamma, int32_t max_workgroups, float* y, float* next_q, uint8_t* next_action, void* stream) {
  if (!tgt_actors || !tgt_critics || !next_state || !reward || !index || !noise || !y || !next_action || nb_agents < 1) return MDR_ERR_INVALID;
  if (nb_agents > MDR_MAX_AGENT_NETS) return MDR_ERR_UNSUPPORTED;
  const int rc = all_fields(tgt_actors, tgt_critics, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  const int F = tgt_actors[0].num_state;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F) return MDR_ERR_INVALID;
  if (!(tau > 0.0f) || !(fabsf(tau) <= FLT_MAX) || !(fabsf(gamma) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (!one_shape(tgt_actors, nb_agents) || !one_shape(tgt_critics, nb_agents)) return MDR_ERR_UNSUPPORTED;
  if (nb_rows == 0) return MDR_OK;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  // the picks of all N minibatches: mdr_maddpg_target_agents' launch over the N B concatenated rows (a row's pick does not depend on
  // the tile it sits in, so these tiles may straddle two agents' minibatches)
  PickAgentsArgs pa{};
  RowArgs& p = pa.r;
  p.actor = make_net(&tgt_actors[0]), p.critic = make_net(&tgt_critics[0]);
  p.state = next_state, p.ld = ld_state, p.index = index, p.B = nb_rows * nb_agents, p.N = nb_agents, p.F = F;
  p.noise = noise, p.tau = tau, p.gamma = gamma, p.reward = reward, p.picks = next_action;
  set_table(pa.nets, tgt_actors, nb_agents);
  pa.TB = (p.B + TILE - 1) / TILE;
  p.R = p.B * nb_agents, p.ntiles = pa.TB * nb_agents;
  if (launch_rows<MODE_PICK_AGENTS>(pa, cap, st) != MDR_OK) return MDR_ERR_HIP;
  // agent a's y from its own target critic on its own minibatch, reward column a
  AllAgentsArgs aa{};
  RowArgs& a = aa.r;
  a = p;
  a.B = nb_rows, a.out0 = y, a.out1 = next_q;
  set_table(aa.critics, tgt_critics, nb_agents);
  aa.TB = (nb_rows + TILE - 1) / TILE;
  a.R = nb_rows, a.ntiles = aa.TB * nb_agents;
  return launch_rows<MODE_TARGET_ALL>(aa, cap, st);
}

int mdr_maddpg_critic_grad_all(const mdr_mlp_t* critics, const float* state, int64_t ld_state, const int64_t* action, const int64_t* index,
                               int64_t nb_rows, int32_t nb_agents, const float* y, int32_t max_workgroups, void* workspace, float* grad,
                               float* loss, float* q, void* stream) {
  if (!critics || !state || !action || !index || !y || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u) || nb_agents < 1)
    return MDR_ERR_INVALID;
  if (nb_agents > MDR_MAX_AGENT_NETS) return MDR_ERR_UNSUPPORTED;
  const int rc = all_fields(nullptr, critics, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  const int F = critics[0].num_state / nb_agents - 2;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (!one_shape(critics, nb_agents)) return MDR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  AllAgentsArgs aa{};
  WeightAllArgs wb{};
  RowArgs& a = aa.r;
  WeightArgs& wa = wb.w;
  carve(a, wa, &critics[0], workspace, nb_rows);      // agent 0's; agent k's lie k ws behind
  aa.ws = wb.ws = ws_floats(&critics[0], nb_rows), wb.G = grad_floats(&critics[0]), wb.actor = 0;
  a.critic = make_net(&critics[0]);
  set_table(aa.critics, critics, nb_agents);
  a.state = state, a.ld = ld_state, a.action = action, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F, a.agent = -1;
  a.y = y, a.out0 = q, a.invB = nb_rows > 0 ? 1.0f / (float)nb_rows : 0.0f;
  aa.TB = (nb_rows + TILE - 1) / TILE;
  a.R = nb_rows, a.ntiles = aa.TB * nb_agents;
  if (nb_rows > 0 && launch_rows<MODE_CRITIC_ALL>(aa, cap, st) != MDR_OK) return MDR_ERR_HIP;
  wa.state = state, wa.ld = ld_state, wa.action = action, wa.index = index, wa.N = nb_agents, wa.F = F, wa.agent = -1;
  wa.grad = grad, wa.loss = loss;
  return launch_weights_all(wb, nb_agents, max_workgroups, st);
}

int mdr_maddpg_actor_grad_all(const mdr_mlp_t* actors, const mdr_mlp_t* critics, const float* state, int64_t ld_state, const int64_t* action,
                              const int64_t* index, int64_t nb_rows, int32_t nb_agents, const float* noise, float tau, float pse,
                              int32_t max_workgroups, void* workspace, float* grad, float* loss, float* q, float* logits, void* stream) {
  if (!actors || !critics || !state || !action || !index || !noise || !grad || !loss || !workspace || ((uintptr_t)workspace & 15u) || nb_agents < 1)
    return MDR_ERR_INVALID;
  if (nb_agents > MDR_MAX_AGENT_NETS) return MDR_ERR_UNSUPPORTED;
  const int rc = all_fields(actors, critics, nb_agents);
  if (rc == MDR_ERR_INVALID) return rc;
  const int F = actors[0].num_state;
  if (nb_rows < 0 || max_workgroups < 0 || ld_state < (int64_t)nb_agents * F) return MDR_ERR_INVALID;
  if (!(tau > 0.0f) || !(fabsf(tau) <= FLT_MAX) || !(fabsf(pse) <= FLT_MAX)) return MDR_ERR_INVALID;
  if (rc != MDR_OK) return rc;
  if (!one_shape(actors, nb_agents) || !one_shape(critics, nb_agents)) return MDR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int cap = lib_cap(max_workgroups);
  AllAgentsArgs aa{};
  WeightAllArgs wb{};
  RowArgs& a = aa.r;
  WeightArgs& wa = wb.w;
  carve(a, wa, &actors[0], workspace, nb_rows);
  aa.ws = wb.ws = ws_floats(&actors[0], nb_rows), wb.G = grad_floats(&actors[0]), wb.actor = 1;
  a.actor = make_net(&actors[0]), a.critic = make_net(&critics[0]);
  set_table(aa.actors, actors, nb_agents);
  set_table(aa.critics, critics, nb_agents);
  a.state = state, a.ld = ld_state, a.action = action, a.index = index, a.B = nb_rows, a.N = nb_agents, a.F = F;
  a.noise = noise, a.tau = tau, a.pse = pse, a.out0 = q, a.out1 = logits, a.invB = nb_rows > 0 ? 1.0f / (float)nb_rows : 0.0f;
  aa.TB = (nb_rows + TILE - 1) / TILE;
  a.R = nb_rows, a.ntiles = aa.TB * nb_agents;
  if (nb_rows > 0 && launch_rows<MODE_ACTOR_ALL>(aa, cap, st) != MDR_OK) return MDR_ERR_HIP;
  wa.state = state, wa.ld = ld_state, wa.action = action, wa.index = index, wa.N = nb_agents, wa.F = F, wa.agent = 0;
  wa.grad = grad, wa.loss = loss;
  return launch_weights_all(wb, nb_agents, max_workgroups, st);
}

}  // extern "C"
