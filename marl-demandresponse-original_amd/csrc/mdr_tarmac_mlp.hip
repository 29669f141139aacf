// TarMAC-PPO actor, the per-agent MLPs on the matrix cores (include/mdr_policy.h: mdr_tarmac_actor_t, mdr_tarmac_actor_sample).
//
// Reference: TarMAC_Actor.forward / TarMAC_Comm.forward (agents/network.py:103-238).  Everything an agent computes on its own is a
// chain of dense layers; the chain is cut only where the attention needs the rows of other agents (mdr_tarmac_comm, mdr_tarmac.hip,
// used unchanged).  Exact fp32 on v_mfma_f32_16x16x4_f32, 16 agents per wavefront, agents on the MFMA column index, units on the row
// index, as k_actor_sample16 (mdr_policy.hip): C/D col = lane & 15, row = 4 (lane >> 4) + reg, so the accumulator a lane holds after
// one layer - units 16 kb + 4 g + reg of its own agent - IS the B operand of the next layer's k-step q = 4 kb + reg when the weight
// columns are stored in that order.  No LDS and no lane movement for the activations; the biases start the accumulators.
//
//   k_tarmac_encode  obs rows -> obs2hidden (F -> H relu -> H) = x -> cat[:, 0:H]; from the same registers hidden2query | hidden2key |
//                    hidden2value (H -> H tanh -> K | K | V) -> qkv [A][K + K + V], the buffer mdr_tarmac_comm reads in place
//   k_tarmac_encode_obs  the same from the env's compact state: the features are built in the wave's LDS window (mdr_observe.h)
//                    instead of being read from observation rows - mdr_env_tarmac_actor_sample
//   k_tarmac_rehop   hops >= 1: [comm, h] -> msg_state2state (H + V -> H + V tanh -> H) = h' -> state; the same projections -> qkv
//   k_tarmac_head    cat = [x, comm] -> comm_hidden2action (H + V -> H relu -> 2) (hidden2action on x without communication), the
//                    two-logit softmax and the action draw of mdr_logits_sample (mdr_draw.h)
//
// A sample step is 1 + hops + (hops - 1) + 1 launches.  Each kernel is a persistent grid of min(ceil(tiles / waves), CUs) workgroups
// that stage their weights ONCE into LDS in fragment order (up to ~125 KB: one workgroup per CU) and stride over the tiles.  Rows
// are addressed with 64-bit offsets: no 4 GiB slicing.
//
// mdr_tarmac_actor_t.precision = MDR_TARMAC_BF16X3 takes the same chain through the kernels of mdr_tarmac_mlp_bf16.hip.
//
// Two instantiations per kernel: the block counts of the reference's sizes (H = 64, K <= 16, V <= 16: 4 / 1 / 5 blocks of 16 units
// for H / V / H + V) with compile-time fragment strides, 16 waves per workgroup in under 128 registers and no scratch; and a general
// form compiled for the largest covered shape whose loops stop at the run-time block counts, 8 waves per workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdr_tarmac_mlp.h"

namespace {

// The A operands of one k-step: a lane's weight for each of the mb output blocks.  Stored in chunks of four blocks,
// [chunk j][lane][i < w_j], w_j = min(4, mb - 4 j): a full chunk is one ds_read_b128 per lane, a chunk of one block has consecutive
// lanes on consecutive banks.
template <int MB, bool EXACT>
__device__ __forceinline__ void load_w(const float* step, int mb, int lane, float (&w)[MB]) {
#pragma unroll
  for (int j = 0; j < (MB + 3) / 4; ++j) {
    const int wj = EXACT ? (MB - 4 * j < 4 ? MB - 4 * j : 4) : (mb - 4 * j < 4 ? mb - 4 * j : 4);
    if (!EXACT && wj <= 0) break;
    const float* p = step + 256 * j + lane * wj;
    if (wj == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      w[4 * j] = v.x;
      if (4 * j + 1 < MB) w[4 * j + 1 < MB ? 4 * j + 1 : 0] = v.y;
      if (4 * j + 2 < MB) w[4 * j + 2 < MB ? 4 * j + 2 : 0] = v.z;
      if (4 * j + 3 < MB) w[4 * j + 3 < MB ? 4 * j + 3 : 0] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < wj && 4 * j + i < MB) w[4 * j + i < MB ? 4 * j + i : 0] = p[i];
    }
  }
}

template <int MB>
__device__ __forceinline__ void init_bias(const float* bias, int g, int mb, f32x4 (&out)[MB]) {
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    if (b < mb)
      out[b] = *reinterpret_cast<const f32x4*>(bias + 16 * b + 4 * g);
    else
      out[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}

// out += W . act(in): the B operand of k-step q = 4 kb + reg is register [kb][reg] of the previous layer as it is
template <int MBI, int MBO, bool EXACT, int ACT>
__device__ __forceinline__ void layer_regs(const float* frag, const f32x4 (&in)[MBI], int mbi, f32x4 (&out)[MBO], int mbo, int lane) {
#pragma unroll
  for (int q = 0; q < 4 * MBI; ++q) {
    if (EXACT || q < 4 * mbi) {
      const float b = activate<ACT>(in[q >> 2][q & 3]);
      float w[MBO];
      load_w<MBO, EXACT>(frag + q * 64 * mbo, mbo, lane, w);
#pragma unroll
      for (int mb = 0; mb < MBO; ++mb)
        if (EXACT || mb < mbo) out[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[mb], b, out[mb], 0, 0, 0);
    }
  }
}

// out += W . x for k-steps fed from the lane's feature registers
template <int XS, int MBO, bool EXACT>
__device__ __forceinline__ void layer_feats(const float* frag, const float (&xr)[XS], int S, f32x4 (&out)[MBO], int mbo, int lane) {
#pragma unroll
  for (int s = 0; s < XS; ++s) {
    if (s < S) {
      float w[MBO];
      load_w<MBO, EXACT>(frag + s * 64 * mbo, mbo, lane, w);
#pragma unroll
      for (int mb = 0; mb < MBO; ++mb)
        if (EXACT || mb < mbo) out[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[mb], xr[s], out[mb], 0, 0, 0);
    }
  }
}

// Features [first, first + S) of a row of D floats into the lane's registers; indices past the row are read at D - 1 and meet zero
// weights.  `vec`: S is a multiple of 4, first + S <= D and the row is 16-byte aligned.
template <int XS>
__device__ __forceinline__ void load_feats(const float* row, int first, int S, int D, int vec, float (&xr)[XS]) {
  if (vec) {
#pragma unroll
    for (int j = 0; j < XS / 4; ++j)
      if (4 * j < S) {
        const float4 v = *reinterpret_cast<const float4*>(row + first + 4 * j);
        xr[4 * j] = v.x, xr[4 * j + 1] = v.y, xr[4 * j + 2] = v.z, xr[4 * j + 3] = v.w;
      }
  } else {
#pragma unroll
    for (int s = 0; s < XS; ++s)
      if (s < S) xr[s] = row[min(first + s, D - 1)];
  }
}

// hidden2query | hidden2key | hidden2value on the hidden state a lane holds, written packed to its agent's qkv row.
// frag_proj: the three first layers [p < 3][4 mbh steps][64 mbh], then the second layers of query (1 block), key (1), value (mbv).
template <int MBH, int MBV, bool EXACT>
__device__ __forceinline__ void projections(const float* fp, const float* vec, const VecLayout& L, const f32x4 (&h)[MBH], int mbh, int mbv,
                                            int K, int V, float* qkv_row, bool valid, int lane) {
  const int g = lane >> 4;
  const int steps = 4 * mbh;
  const int n1 = steps * 64 * mbh;
  const float* f2 = fp + 3 * n1;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    f32x4 t[MBH];
    init_bias<MBH>(vec + L.p1 + p * 16 * mbh, g, mbh, t);
    layer_regs<MBH, MBH, EXACT, ACT_NONE>(fp + p * n1, h, mbh, t, mbh, lane);
    if (p < 2) {
      f32x4 o[1];
      init_bias<1>(vec + (p == 0 ? L.q2 : L.k2), g, 1, o);
      layer_regs<MBH, 1, EXACT, ACT_TANH>(f2 + p * steps * 64, t, mbh, o, 1, lane);
      if (valid && 4 * g < K) *reinterpret_cast<f32x4*>(qkv_row + p * K + 4 * g) = o[0];
    } else {
      f32x4 o[MBV];
      init_bias<MBV>(vec + L.v2, g, mbv, o);
      layer_regs<MBH, MBV, EXACT, ACT_TANH>(f2 + 2 * steps * 64, t, mbh, o, mbv, lane);
#pragma unroll
      for (int mb = 0; mb < MBV; ++mb)
        if (valid && 16 * mb + 4 * g < V) *reinterpret_cast<f32x4*>(qkv_row + 2 * K + 16 * mb + 4 * g) = o[mb];
    }
  }
}

template <int MBH, int MBV, bool EXACT>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_encode(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* fa = lds;
  float* fp = fa + a.na;
  float* vec = fp + a.np;
  const int tid = threadIdx.x;
  stage(fa, a.fa, a.na, tid);
  if (a.with_comm) stage(fp, a.fp, a.np, tid);
  stage(vec, a.vec, a.nvec, tid);
  __syncthreads();
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv;
  const VecLayout L = vec_layout(mbh, mbv, a.mbm);
  const int lane0 = tid & 63, r = lane0 & 15;
  constexpr int NW = EXACT ? WAVES : WAVES_GEN;
  const int64_t wave = (int64_t)blockIdx.x * NW + (tid >> 6), nwaves = (int64_t)gridDim.x * NW;
  const float* f2 = fa + a.S0 * 64 * mbh;
  for (int64_t t = wave; t < a.ntiles; t += nwaves) {
    const int lane = tile_local(lane0), g = lane >> 4;
    const int64_t agent = t * 16 + r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    float xr[16];
    load_feats<16>(a.in0 + ac * a.ld0, g * a.S0, a.S0, a.D0, a.vec0, xr);
    f32x4 t1[MBH], x[MBH];
    init_bias<MBH>(vec + L.o1, g, mbh, t1);
    layer_feats<16, MBH, EXACT>(fa, xr, a.S0, t1, mbh, lane);
    init_bias<MBH>(vec + L.o2, g, mbh, x);
    layer_regs<MBH, MBH, EXACT, ACT_RELU>(f2, t1, mbh, x, mbh, lane);
    float* cat_row = a.cat + ac * a.ldcat;
#pragma unroll
    for (int mb = 0; mb < MBH; ++mb)
      if (valid && 16 * mb + 4 * g < a.H) *reinterpret_cast<f32x4*>(cat_row + 16 * mb + 4 * g) = x[mb];
    if (a.with_comm) projections<MBH, MBV, EXACT>(fp, vec, L, x, mbh, mbv, a.K, a.V, a.qkv + ac * a.ldqkv, valid, lane);
  }
}

// Observe -> act (mdr_env_tarmac_actor_sample): k_tarmac_encode with its 13 features per lane read from the wave's LDS window
// instead of an observation row.  The window is staged from the env's compact state by the helpers of mdr_observe.h exactly as
// k_actor_observe16 (mdr_policy.hip) stages it for the default observation - 16 consecutive agents per wave, one window per wave -
// and holds normStateDict feature n of tile row r at float ROW r + (n < 11 ? 40 + n : n - 11).  Lane group g takes the features
// 13 g + s of its agent, the k-step order of frag_encode, so the MFMA sequence and its operands are those of the rows path; index
// 51, the pad of group 3's last k-step, reads feature 50 as the rows path does (against a zero weight).
// Row stride: TARMAC_OBS_ROW = 60 floats.  The features are read with 4-byte LDS loads in which the 16 lanes of a group address the
// same column of 16 consecutive rows, on 32 banks of 4 bytes.  The stride has to stay a multiple of 4 floats for the 16-byte stores
// of the staging (an odd one would be conflict-free); 60 = 28 (mod 32) puts the 16 rows on 8 banks, two lanes each, where OBS_ROW = 56
// = 24 (mod 32) - chosen for 16-byte reads - folds them onto 4, four lanes each.  The window has no pad behind its rows: no read
// goes past float 52 of a row.  16 windows of 3840 bytes beside the ~94 KB of weights: 157 KB with the row table, under the 160 KB.
// The loads of a wave's next tile are issued before the tile's matrix work and land during it; its rows are staged behind layer 1,
// once the features of the current tile are consumed, and gathered at the end of the tile.
template <int MBH, int MBV, bool EXACT, bool STORE, bool GEN>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_encode_obs(MlpArgs a, mdr::ObserveArgs o, float* rows_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TILE = 16, ROW = TARMAC_OBS_ROW, WIN = TILE * ROW;
  float* fa = lds;
  float* fp = fa + a.na;
  float* vec = fp + a.np;
  const int tid = threadIdx.x;
  const int NW = (int)(blockDim.x >> 6);      // as many of the form's waves as the windows leave room for
  float* rows = vec + a.nvec + (tid >> 6) * WIN;
  uint16_t* table = reinterpret_cast<uint16_t*>(vec + a.nvec + NW * WIN);      // [TILE * 51] (only when rows are stored)
  stage(fa, a.fa, a.na, tid);
  if (a.with_comm) stage(fp, a.fp, a.np, tid);
  stage(vec, a.vec, a.nvec, tid);
  const int lane0 = tid & 63, r = lane0 & 15;
  for (int i = lane0; i < WIN; i += 64) rows[i] = 0.0f;
  if (STORE) observe_build_table<TILE, ROW>(table, tid, 64 * NW);
  __syncthreads();
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv;
  const VecLayout L = vec_layout(mbh, mbv, a.mbm);
  const int64_t wave = (int64_t)blockIdx.x * NW + (tid >> 6), nwaves = (int64_t)gridDim.x * NW;
  const float* f2 = fa + a.S0 * 64 * mbh;
  const double* sig_row = observe_sig_row(o);
  TileCursor tc;
  tc.init(wave * TILE, nwaves * TILE, o.N);
  float xr[16] = {};
  auto gather = [&](int64_t first_agent) {
    const int g = lane0 >> 4;
    float* row = rows + r * ROW;
    const float lock = row[4 * OBS_C + 11], y = row[4 * OBS_C + 12];
    // the senders' seconds_since_off become quotients by the RECEIVER's lockout, in place: lane group g takes the messages g, g + 4
    // and g + 8 of its agent's row (k_actor_observe16)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int m = g + 4 * i;
      if (m < OBS_C) row[4 * m + 1] = mdr::div_by_lockout(row[4 * m + 1], lock, y);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int s = 0; s < 13; ++s) {
      const int n = min(13 * g + s, 50);
      xr[s] = row[n < 11 ? 4 * OBS_C + n : n - 11];
    }
    if (STORE)
      observe_store_rows<TILE>(rows, table, rows_out + first_agent * 51, lane0,
                               GEN ? (int)((a.A - first_agent) < (int64_t)TILE ? (a.A - first_agent) : (int64_t)TILE) : TILE);
  };
  SegSlot slot{};
  if (wave < a.ntiles) {
    if (GEN) {
      const HouseRegs first = observe_load_gen<TILE>(o, sig_row, tc.e, tc.h0, wave * TILE, a.A, lane0, slot);
      observe_stage_gen<false, ROW>(o, first, slot, rows);
    } else {
      const HouseRegs first = observe_load<TILE>(o, sig_row, tc.e, tc.h0, lane0);
      observe_stage<TILE, false, ROW>(o, first, rows, lane0);
    }
    observe_window_fence();
    gather(wave * TILE);
  }
  for (int64_t t = wave; t < a.ntiles; t += nwaves) {
    const int lane = tile_local(lane0), g = lane >> 4;
    const int64_t agent = t * 16 + r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    const bool more = t + nwaves < a.ntiles;
    tc.next();
    HouseRegs nxt{};
    if (more) nxt = GEN ? observe_load_gen<TILE>(o, sig_row, tc.e, tc.h0, (t + nwaves) * TILE, a.A, lane0, slot) : observe_load<TILE>(o, sig_row, tc.e, tc.h0, lane0);
    f32x4 t1[MBH], x[MBH];
    init_bias<MBH>(vec + L.o1, g, mbh, t1);
    layer_feats<16, MBH, EXACT>(fa, xr, a.S0, t1, mbh, lane);
    if (more) {      // the features are in the MFMA pipeline: the window is free for the next tile's rows
      if (GEN) observe_stage_gen<false, ROW>(o, nxt, slot, rows);
      else observe_stage<TILE, false, ROW>(o, nxt, rows, lane0);
    }
    init_bias<MBH>(vec + L.o2, g, mbh, x);
    layer_regs<MBH, MBH, EXACT, ACT_RELU>(f2, t1, mbh, x, mbh, lane);
    float* cat_row = a.cat + ac * a.ldcat;
#pragma unroll
    for (int mb = 0; mb < MBH; ++mb)
      if (valid && 16 * mb + 4 * g < a.H) *reinterpret_cast<f32x4*>(cat_row + 16 * mb + 4 * g) = x[mb];
    if (a.with_comm) projections<MBH, MBV, EXACT>(fp, vec, L, x, mbh, mbv, a.K, a.V, a.qkv + ac * a.ldqkv, valid, lane);
    if (more) {
      observe_window_fence();
      gather((t + nwaves) * TILE);
    }
  }
}

// frag_msg: layer 1 [V / 4 + H / 4 steps][64 mbm] - the comm columns of the concatenation [comm, h] first - then layer 2
// [4 mbm steps][64 mbh]
template <int MBH, int MBV, int MBM, bool EXACT>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_rehop(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* fa = lds;
  float* fp = fa + a.na;
  float* vec = fp + a.np;
  const int tid = threadIdx.x;
  stage(fa, a.fa, a.na, tid);
  stage(fp, a.fp, a.np, tid);
  stage(vec, a.vec, a.nvec, tid);
  __syncthreads();
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv, mbm = EXACT ? MBM : a.mbm;
  const VecLayout L = vec_layout(mbh, mbv, mbm);
  const int lane0 = tid & 63, r = lane0 & 15;
  constexpr int NW = EXACT ? WAVES : WAVES_GEN;
  const int64_t wave = (int64_t)blockIdx.x * NW + (tid >> 6), nwaves = (int64_t)gridDim.x * NW;
  const float* f1h = fa + a.S0 * 64 * mbm;
  const float* f2 = f1h + a.S1 * 64 * mbm;
  for (int64_t t = wave; t < a.ntiles; t += nwaves) {
    const int lane = tile_local(lane0), g = lane >> 4;
    const int64_t agent = t * 16 + r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    float xc[4 * MBV], xh[4 * MBH];
    load_feats<4 * MBV>(a.in0 + ac * a.ld0, g * a.S0, a.S0, a.V, a.vec0, xc);
    load_feats<4 * MBH>(a.in1 + ac * a.ld1, g * a.S1, a.S1, a.H, a.vec1, xh);
    f32x4 m[MBM], h[MBH];
    init_bias<MBM>(vec + L.m1, g, mbm, m);
    layer_feats<4 * MBV, MBM, EXACT>(fa, xc, a.S0, m, mbm, lane);
    layer_feats<4 * MBH, MBM, EXACT>(f1h, xh, a.S1, m, mbm, lane);
    init_bias<MBH>(vec + L.m2, g, mbh, h);
    layer_regs<MBM, MBH, EXACT, ACT_TANH>(f2, m, mbm, h, mbh, lane);
    float* st_row = a.state + ac * (int64_t)a.H;
#pragma unroll
    for (int mb = 0; mb < MBH; ++mb)
      if (valid && 16 * mb + 4 * g < a.H) *reinterpret_cast<f32x4*>(st_row + 16 * mb + 4 * g) = h[mb];
    projections<MBH, MBV, EXACT>(fp, vec, L, h, mbh, mbv, a.K, a.V, a.qkv + ac * a.ldqkv, valid, lane);
  }
}

// frag_head: [D / 4 steps][64 mbh], D = H + V (H without communication): the row [x, comm] as it lies in cat
template <int MBH, int XS, bool EXACT>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_head(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* fa = lds;
  float* vec = fa + a.na;
  const int tid = threadIdx.x;
  stage(fa, a.fa, a.na, tid);
  stage(vec, a.vec, a.nvec, tid);
  __syncthreads();
  const int mbh = EXACT ? MBH : a.mbh;
  const VecLayout L = vec_layout(mbh, a.mbv, a.mbm);
  const int lane0 = tid & 63, r = lane0 & 15;
  constexpr int NW = EXACT ? WAVES : WAVES_GEN;
  const int64_t wave = (int64_t)blockIdx.x * NW + (tid >> 6), nwaves = (int64_t)gridDim.x * NW;
  const float bias3 = vec[L.b3];
  for (int64_t t = wave; t < a.ntiles; t += nwaves) {
    const int lane = tile_local(lane0), g = lane >> 4;
    const int64_t agent = t * 16 + r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    float xr[XS];
    load_feats<XS>(a.in0 + ac * a.ld0, g * a.S0, a.S0, a.D0, a.vec0, xr);
    f32x4 acc[MBH];
    init_bias<MBH>(vec + L.h1, g, mbh, acc);
    layer_feats<XS, MBH, EXACT>(fa, xr, a.S0, acc, mbh, lane);
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
}

// ---------------------------------------------------------------------------------------------------------------------- host

bool shape_positive(int F, int H, int K, int V) { return F > 0 && H > 0 && K > 0 && V > 0; }
bool shape_covered(int F, int H, int K, int V) {
  return F <= MAX_F && H % 4 == 0 && H <= MAX_H && K % 4 == 0 && K <= MAX_K && V % 4 == 0 && V <= MAX_V;
}

int64_t encode_floats(int F, int H) { return ((int64_t)(F + 3) / 4 + 4 * blocks(H)) * 64 * blocks(H); }
int64_t proj_floats(int H, int V) { return (int64_t)4 * blocks(H) * 64 * (3 * blocks(H) + 2 + blocks(V)); }
int64_t msg_floats(int H, int V) { return (int64_t)((V + H) / 4) * 64 * blocks(H + V) + (int64_t)4 * blocks(H + V) * 64 * blocks(H); }
int64_t head_floats(int H, int V, int with_comm) { return (int64_t)((H + (with_comm ? V : 0)) / 4) * 64 * blocks(H); }

}  // namespace

extern "C" {

int64_t mdr_tarmac_frag_encode_floats(int32_t num_state, int32_t hidden) {
  return (num_state > 0 && hidden > 0 && num_state <= MAX_F && hidden <= MAX_H) ? encode_floats(num_state, hidden) : -1;
}
int64_t mdr_tarmac_frag_proj_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V) ? proj_floats(hidden, num_value) : -1;
}
int64_t mdr_tarmac_frag_msg_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V && hidden % 4 == 0 && num_value % 4 == 0) ? msg_floats(hidden, num_value) : -1;
}
int64_t mdr_tarmac_frag_head_floats(int32_t hidden, int32_t num_value, int32_t with_comm) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V && hidden % 4 == 0 && num_value % 4 == 0)
             ? head_floats(hidden, num_value, with_comm) : -1;
}
int64_t mdr_tarmac_vec_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V) ? vec_layout(blocks(hidden), blocks(num_value), blocks(hidden + num_value)).total : -1;
}

int64_t mdr_tarmac_frag_words(const mdr_tarmac_actor_t* actor, int32_t part) {
  if (!actor || actor->struct_size != sizeof(mdr_tarmac_actor_t) || part < 0 || part > 3) return -1;
  const int F = actor->num_state, H = actor->hidden, K = actor->num_key, V = actor->num_value, wc = actor->with_comm != 0;
  if (!shape_positive(F, H, K, V) || !shape_covered(F, H, K, V)) return -1;
  if (actor->precision == MDR_TARMAC_FP32)
    return part == 0 ? encode_floats(F, H) : part == 1 ? proj_floats(H, V) : part == 2 ? msg_floats(H, V) : head_floats(H, V, wc);
  if (actor->precision == MDR_TARMAC_BF16X3)
    return part == 0 ? encode_words(F, H) : part == 1 ? proj_words(H, V) : part == 2 ? msg_words(H, V) : head_words(H, V, wc);
  return -1;
}

int64_t mdr_tarmac_actor_workspace_bytes(const mdr_tarmac_actor_t* actor, int64_t nb_agents) {
  if (!actor || actor->struct_size != sizeof(mdr_tarmac_actor_t) || nb_agents < 0) return -1;
  const int H = actor->hidden, K = actor->num_key, V = actor->num_value;
  if (!shape_positive(1, H, K, V)) return -1;
  int64_t floats = H;
  if (actor->with_comm) floats += V + K + K + V + (actor->num_hops > 1 ? H : 0);
  return nb_agents * floats * (int64_t)sizeof(float);
}

// The launch chain of a sample.  `o` == nullptr: from the observation rows `obs`; else from the env's compact state (`obs` unused),
// `rows_out` optional.  Every refusal comes before the first launch.
static int sample_chain(const mdr_tarmac_actor_t* actor, const float* obs, const mdr::ObserveArgs* o, float* rows_out, int32_t nb_envs,
                        int32_t nb_houses, uint64_t seed, uint64_t step, const int32_t* step_dev, void* workspace, uint8_t* action, float* a_prob,
                        float* probs, void* stream) {
  if (!actor || actor->struct_size != sizeof(mdr_tarmac_actor_t) || (!obs && !o) || !workspace || !action) return MDR_ERR_INVALID;
  if (nb_envs < 0 || nb_houses <= 0) return MDR_ERR_INVALID;
  const int F = actor->num_state, H = actor->hidden, K = actor->num_key, V = actor->num_value;
  const int hops = actor->num_hops, wc = actor->with_comm != 0;
  if (!shape_positive(F, H, K, V) || hops < 1 || actor->nb_comm < 0) return MDR_ERR_INVALID;
  if (actor->mode != MDR_TARMAC_NEIGHBOURS && actor->mode != MDR_TARMAC_NONE) return MDR_ERR_INVALID;
  if (!(actor->defect_prob >= 0.0f && actor->defect_prob <= 1.0f)) return MDR_ERR_INVALID;
  if (actor->precision != MDR_TARMAC_FP32 && actor->precision != MDR_TARMAC_BF16X3) return MDR_ERR_INVALID;
  if (!actor->frag_encode || !actor->frag_head || !actor->vec) return MDR_ERR_INVALID;
  if (wc && (!actor->frag_proj || (hops > 1 && !actor->frag_msg))) return MDR_ERR_INVALID;
  if (!aligned16(workspace) || !aligned16(actor->frag_encode) || !aligned16(actor->frag_head) || !aligned16(actor->vec) ||
      !aligned16(actor->frag_proj) || !aligned16(actor->frag_msg) || ((uintptr_t)obs & 3u) || ((uintptr_t)rows_out & 3u))
    return MDR_ERR_INVALID;
  if (!shape_covered(F, H, K, V) || hops > MAX_HOPS) return MDR_ERR_UNSUPPORTED;
  if (o && !mdr::tarmac_observe_covered(*o, F, actor->precision == MDR_TARMAC_BF16X3 ? 32 : 16)) return MDR_ERR_UNSUPPORTED;
  const int c = actor->nb_comm < nb_houses - 1 ? actor->nb_comm : nb_houses - 1;
  if (wc && actor->mode == MDR_TARMAC_NEIGHBOURS && c > MAX_C) return MDR_ERR_UNSUPPORTED;
  const int64_t A = (int64_t)nb_envs * nb_houses;
  if (A >= ((int64_t)1 << 35)) return MDR_ERR_UNSUPPORTED;      // the grids of mdr_tarmac_comm
  if (A == 0) return MDR_OK;
  hipStream_t s = (hipStream_t)stream;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  if (actor->precision == MDR_TARMAC_BF16X3)
    return mdr::tarmac_sample_bf16(actor, obs, o, rows_out, nb_envs, nb_houses, seed, step, step_dev, workspace, action, a_prob, probs, cus, stream);

  const int mbh = blocks(H), mbv = blocks(V), mbm = blocks(H + V);
  const VecLayout L = vec_layout(mbh, mbv, mbm);
  const bool exact = mbh == 4 && mbv == 1 && (!wc || hops == 1 || mbm == 5);
  const int64_t ldcat = wc ? H + V : H, ldqkv = K + K + V;
  float* cat = static_cast<float*>(workspace);
  float* qkv = cat + A * ldcat;
  float* state = qkv + A * ldqkv;

  MlpArgs a{};
  a.vec = actor->vec, a.nvec = L.total;
  a.cat = cat, a.qkv = qkv, a.state = state, a.ldcat = ldcat, a.ldqkv = ldqkv;
  a.action = action, a.a_prob = a_prob, a.probs = probs;
  a.A = A, a.ntiles = (A + 15) / 16;
  a.H = H, a.K = K, a.V = V, a.mbh = mbh, a.mbv = mbv, a.mbm = mbm;
  a.with_comm = wc, a.greedy = actor->greedy != 0;
  a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.step_lo = (uint32_t)step, a.step_hi = (uint32_t)(step >> 32);
  a.step_dev = step_dev;
  a.np = wc ? (int)proj_floats(H, V) : 0;
  auto whole4 = [](int S, int D) { return (S % 4 == 0 && 4 * S == D) ? 1 : 0; };

  // ---- obs -> x (-> qkv)
  a.fa = actor->frag_encode, a.fp = actor->frag_proj, a.na = (int)encode_floats(F, H);
  a.in0 = obs, a.ld0 = F, a.D0 = F, a.S0 = (F + 3) / 4;
  a.vec0 = whole4(a.S0, F) && aligned16(obs);
  int rc;
  if (o) {      // the same layers on features built in LDS: whole-tile staging where no tile of 16 leaves its env
    const bool gen = o->N % 16 != 0;
#define MDR_TARMAC_OBS(...)                                                                                                  \
  (rows_out ? (gen ? launch_observe(k_tarmac_encode_obs<__VA_ARGS__, true, true>, waves, 16, a, *o, rows_out, cus, s)       \
                   : launch_observe(k_tarmac_encode_obs<__VA_ARGS__, true, false>, waves, 16, a, *o, rows_out, cus, s))     \
            : (gen ? launch_observe(k_tarmac_encode_obs<__VA_ARGS__, false, true>, waves, 16, a, *o, rows_out, cus, s)      \
                   : launch_observe(k_tarmac_encode_obs<__VA_ARGS__, false, false>, waves, 16, a, *o, rows_out, cus, s)))
    const int waves = exact ? WAVES : WAVES_GEN;
    rc = exact ? MDR_TARMAC_OBS(4, 1, true) : MDR_TARMAC_OBS(4, 2, false);
#undef MDR_TARMAC_OBS
  } else {
    rc = exact ? launch(k_tarmac_encode<4, 1, true>, WAVES, a, a.na + a.np + a.nvec, cus, s)
               : launch(k_tarmac_encode<4, 2, false>, WAVES_GEN, a, a.na + a.np + a.nvec, cus, s);
  }
  if (rc != MDR_OK) return rc;
  if (wc) {
    for (int hop = 0; hop < hops; ++hop) {
      if (hop > 0) {      // [comm, h] -> h' -> qkv
        a.fa = actor->frag_msg, a.na = (int)msg_floats(H, V);
        a.in0 = cat + H, a.ld0 = ldcat, a.D0 = V, a.S0 = V / 4;
        a.in1 = hop == 1 ? cat : state, a.ld1 = hop == 1 ? ldcat : H, a.S1 = H / 4;
        a.vec0 = whole4(a.S0, V), a.vec1 = whole4(a.S1, H);
        rc = exact ? launch(k_tarmac_rehop<4, 1, 5, true>, WAVES, a, a.na + a.np + a.nvec, cus, s)
                   : launch(k_tarmac_rehop<4, 2, 6, false>, WAVES_GEN, a, a.na + a.np + a.nvec, cus, s);
        if (rc != MDR_OK) return rc;
      }
      rc = mdr_tarmac_comm(qkv, ldqkv, qkv + K, ldqkv, qkv + 2 * K, ldqkv, nb_envs, nb_houses, K, V, actor->nb_comm, actor->mode, actor->defect_prob,
                           seed, step, step_dev, hop, cat + H, ldcat, stream);
      if (rc != MDR_OK) return rc;
    }
  }
  // ---- [x, comm] -> logits -> action
  a.fa = actor->frag_head, a.na = (int)head_floats(H, V, wc);
  a.in0 = cat, a.ld0 = ldcat, a.D0 = (int)ldcat, a.S0 = (int)ldcat / 4;
  a.vec0 = whole4(a.S0, (int)ldcat);
  return (mbh == 4 && a.S0 <= 20) ? launch(k_tarmac_head<4, 20, true>, WAVES, a, a.na + a.nvec, cus, s)
                                  : launch(k_tarmac_head<4, 24, false>, WAVES_GEN, a, a.na + a.nvec, cus, s);
}

int mdr_tarmac_actor_sample(const mdr_tarmac_actor_t* actor, const float* obs, int32_t nb_envs, int32_t nb_houses, uint64_t seed, uint64_t step,
                            const int32_t* step_dev, void* workspace, uint8_t* action, float* a_prob, float* probs, void* stream) {
  if (!obs) return MDR_ERR_INVALID;
  return sample_chain(actor, obs, nullptr, nullptr, nb_envs, nb_houses, seed, step, step_dev, workspace, action, a_prob, probs, stream);
}

}  // extern "C"

namespace mdr {

int tarmac_sample_observe(const mdr_tarmac_actor_t* actor, const ObserveArgs& o, uint64_t seed, uint64_t step, const int32_t* step_dev,
                          void* workspace, uint8_t* action, float* a_prob, float* probs, float* rows_out, hipStream_t stream) {
  return sample_chain(actor, nullptr, &o, rows_out, o.E, o.N, seed, step, step_dev, workspace, action, a_prob, probs, (void*)stream);
}

}  // namespace mdr
