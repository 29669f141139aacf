// TarMAC-PPO actor, the per-agent MLPs on the matrix cores (include/mdr_policy.h: mdr_tarmac_actor_t, mdr_tarmac_actor_sample).
//
// Reference: TarMAC_Actor.forward / TarMAC_Comm.forward (agents/network.py:103-238).  Everything an agent computes on its own is a
// chain of dense layers; the chain is cut only where the attention needs the rows of other agents (mdr_tarmac_comm, mdr_tarmac.hip,
// used unchanged).  Exact fp32 on v_mfma_f32_16x16x4_f32, 16 agents per wavefront, agents on the MFMA column index, units on the row
// index, as k_actor_sample16 (mdr_policy.hip): C/D col = lane & 15, row = 4 (lane >> 4) + reg, so the accumulator a lane holds after
// one layer - units 16 kb + 4 g + reg of its own agent - IS the B operand of the next layer's k-step q = 4 kb + reg when the weight
// columns are stored in that order.  No LDS and no lane movement for the activations; the biases start the accumulators.
//
//   k_tarmac_encode  features -> obs2hidden (F -> H relu -> H) = x -> cat[:, 0:H]; from the same registers hidden2query | hidden2key |
//                    hidden2value (H -> H tanh -> K | K | V) -> qkv [A][K + K + V], the buffer mdr_tarmac_comm reads in place.
//                    One kernel over a feature source: <..., RowsSource> reads the observation rows, <..., ObserveSource<STORE, GEN>>
//                    builds the features from the env's compact state in the wave's LDS window (ObserveWindow, mdr_tarmac_mlp.h;
//                    mdr_observe.h) - mdr_env_tarmac_actor_sample
//   k_tarmac_rehop   hops >= 1: [comm, h] -> msg_state2state (H + V -> H + V tanh -> H) = h' -> state; the same projections -> qkv
//   k_tarmac_head    cat = [x, comm] -> comm_hidden2action (H + V -> H relu -> 2) (hidden2action on x without communication), then
//                    head_finish (mdr_tarmac_mlp.h): the two-logit softmax and the action draw of mdr_logits_sample (mdr_draw.h)
//
// Every kernel opens with stage_weights (mdr_tarmac_mlp.h).  The host side is one chain for both precisions, run_chain<Forms>
// (mdr_tarmac_mlp.h), behind the argument checks of sample_chain below; Fp32Forms is what this file brings to it.
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

// Where k_tarmac_encode's 16 agents get their features, 13 per lane: lane group g takes the features 13 g + s of its agent, the
// k-step order of frag_encode.  begin() -> the lane's features for tile t; after_layer1() once they are in the MFMA pipeline; end().
struct RowsSource : NoHooks {      // the agent's observation row
  static constexpr bool WINDOWS = false;
  __device__ __forceinline__ RowsSource(int64_t, int64_t) {}
  __device__ __forceinline__ const float (&begin(int64_t, const float* row, int first, int S, int D, int vec, float (&xr)[16]))[16] {
    load_feats<16>(row, first, S, D, vec, xr);
    return xr;
  }
};

// Observe -> act (mdr_env_tarmac_actor_sample), k_tarmac_encode<..., ObserveSource<STORE, GEN>>: the features are read from the
// wave's LDS window (ObserveWindow, mdr_tarmac_mlp.h) - 16 consecutive agents per wave, one window per wave - so the MFMA sequence and
// its operands are those of the rows path; index 51, the pad of group 3's last k-step, reads feature 50 (against a zero weight).
// Row stride: TARMAC_OBS_ROW = 60 floats.  The features are read with 4-byte LDS loads in which the 16 lanes of a group address the
// same column of 16 consecutive rows, on 32 banks of 4 bytes.  The stride has to stay a multiple of 4 floats for the 16-byte stores
// of the staging (an odd one would be conflict-free); 60 = 28 (mod 32) puts the 16 rows on 8 banks, two lanes each, where OBS_ROW = 56
// = 24 (mod 32) - chosen for 16-byte reads - folds them onto 4, four lanes each.  The window has no pad behind its rows: no read
// goes past float 52 of a row.  16 windows of 3840 bytes beside the ~94 KB of weights: 157 KB with the row table, under the 160 KB.
// The loads of a wave's next tile are issued before the tile's matrix work and land during it; its rows are staged behind layer 1,
// once the features of the current tile are consumed, and gathered at the end of the tile.
template <bool STORE, bool GEN>
struct ObserveSource : ObserveWindow<16, STORE, GEN> {
  using W = ObserveWindow<16, STORE, GEN>;
  static constexpr bool WINDOWS = true;
  static constexpr int TILE = 16;
  float xr[16];

  __device__ __forceinline__ ObserveSource(int64_t A, int64_t ntiles, const WindowArgs& x) : W{x.o, x.rows_out, A, ntiles} {}

  __device__ __forceinline__ void gather(int64_t first_agent) {
    const int g = this->lane0 >> 4, r = this->lane0 & 15;
    this->lockout_quotients(r, g);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const float* row = this->rows + r * W::ROW;
#pragma unroll
    for (int s = 0; s < 13; ++s) xr[s] = row[W::at(min(13 * g + s, 50))];
    this->store_rows(first_agent);
  }
  __device__ __forceinline__ void prime(int64_t wave, int64_t nwaves) {
    this->start(wave, nwaves);
#pragma unroll
    for (int s = 0; s < 16; ++s) xr[s] = 0.0f;
    if (wave < this->ntiles) {
      this->load(wave * TILE);
      this->stage_rows();
      observe_window_fence();
      gather(wave * TILE);
    }
  }
  __device__ __forceinline__ const float (&begin(int64_t t, const float*, int, int, int, int, float (&)[16]))[16] {
    this->advance(t);
    if (this->more) this->load(this->next_tile * TILE);
    return xr;
  }
  __device__ __forceinline__ void after_layer1() {      // the window is free for the next tile's rows
    if (this->more) this->stage_rows();
  }
  __device__ __forceinline__ void end() {
    if (this->more) {
      observe_window_fence();
      gather(this->next_tile * TILE);
    }
  }
};

// obs2hidden on the source's features, x -> cat, the projections -> qkv.  The observe source runs with as many of the form's waves as
// its windows leave room for.
template <int MBH, int MBV, bool EXACT, class Source, class... SourceArgs>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_encode(MlpArgs a, SourceArgs... x) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Source src(a.A, a.ntiles, x...);
  const int nw = Source::WINDOWS ? (int)(blockDim.x >> 6) : (EXACT ? WAVES : WAVES_GEN);
  const Staged S = stage_weights(lds, Fragments{a.fa, a.fp, a.vec, a.na, a.np, a.nvec}, a.with_comm != 0, nw,
                                 [&]() { src.carve(lds + a.na + a.np + a.nvec, nw); });
  src.prime(S.wave, S.nwaves);
  const float *fa = S.fa, *fp = S.fp, *vec = S.vec;
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv;
  const VecLayout L = vec_layout(mbh, mbv, a.mbm);
  const float* f2 = fa + a.S0 * 64 * mbh;
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const int64_t agent = t * 16 + S.r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    float fresh[16];      // the rows source fills it for every tile; the observe source carries its own from the previous tile's end
    const float (&xr)[16] = src.begin(t, a.in0 + ac * a.ld0, g * a.S0, a.S0, a.D0, a.vec0, fresh);
    f32x4 t1[MBH], x1[MBH];
    init_bias<MBH>(vec + L.o1, g, mbh, t1);
    layer_feats<16, MBH, EXACT>(fa, xr, a.S0, t1, mbh, lane);
    src.after_layer1();
    init_bias<MBH>(vec + L.o2, g, mbh, x1);
    layer_regs<MBH, MBH, EXACT, ACT_RELU>(f2, t1, mbh, x1, mbh, lane);
    float* cat_row = a.cat + ac * a.ldcat;
#pragma unroll
    for (int mb = 0; mb < MBH; ++mb)
      if (valid && 16 * mb + 4 * g < a.H) *reinterpret_cast<f32x4*>(cat_row + 16 * mb + 4 * g) = x1[mb];
    if (a.with_comm) projections<MBH, MBV, EXACT>(fp, vec, L, x1, mbh, mbv, a.K, a.V, a.qkv + ac * a.ldqkv, valid, lane);
    src.end();
  }
}

// frag_msg: layer 1 [V / 4 + H / 4 steps][64 mbm] - the comm columns of the concatenation [comm, h] first - then layer 2
// [4 mbm steps][64 mbh]
template <int MBH, int MBV, int MBM, bool EXACT>
__global__ __launch_bounds__(64 * (EXACT ? WAVES : WAVES_GEN)) void k_tarmac_rehop(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Staged S = stage_weights(lds, Fragments{a.fa, a.fp, a.vec, a.na, a.np, a.nvec}, true, EXACT ? WAVES : WAVES_GEN);
  const float *fa = S.fa, *fp = S.fp, *vec = S.vec;
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv, mbm = EXACT ? MBM : a.mbm;
  const VecLayout L = vec_layout(mbh, mbv, mbm);
  const float* f1h = fa + a.S0 * 64 * mbm;
  const float* f2 = f1h + a.S1 * 64 * mbm;
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const int64_t agent = t * 16 + S.r;
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
  const Staged S = stage_weights(lds, Fragments{a.fa, nullptr, a.vec, a.na, 0, a.nvec}, false, EXACT ? WAVES : WAVES_GEN);
  const float *fa = S.fa, *vec = S.vec;
  const int mbh = EXACT ? MBH : a.mbh;
  const VecLayout L = vec_layout(mbh, a.mbv, a.mbm);
  const float bias3 = vec[L.b3];
  const DrawArgs draw{a.action, a.a_prob, a.probs, a.greedy, a.k0, a.k1, a.step_lo, a.step_hi, a.step_dev};
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const int64_t agent = t * 16 + S.r;
    const bool valid = agent < a.A;
    const int64_t ac = valid ? agent : a.A - 1;
    float xr[XS];
    load_feats<XS>(a.in0 + ac * a.ld0, g * a.S0, a.S0, a.D0, a.vec0, xr);
    f32x4 acc[MBH];
    init_bias<MBH>(vec + L.h1, g, mbh, acc);
    layer_feats<XS, MBH, EXACT>(fa, xr, a.S0, acc, mbh, lane);
    head_finish<MBH, EXACT>(acc, vec, L, mbh, g, bias3, draw, agent, valid);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- host

bool shape_positive(int F, int H, int K, int V) { return F > 0 && H > 0 && K > 0 && V > 0; }
bool shape_covered(int F, int H, int K, int V) {
  return F <= MAX_F && H % 4 == 0 && H <= MAX_H && K % 4 == 0 && K <= MAX_K && V % 4 == 0 && V <= MAX_V;
}

struct Fp32Forms : FragFloats {
  static constexpr int TILE = 16;
  static int waves(bool exact) { return exact ? WAVES : WAVES_GEN; }
  static int row_steps(int n) { return (n + 3) / 4; }
  static int whole_vectors(int S, int D) { return (S % 4 == 0 && 4 * S == D) ? 1 : 0; }
  static bool head_exact(int mbh, int S) { return mbh == 4 && S <= 20; }
  static MlpKernel encode_kernel(bool exact) { return exact ? k_tarmac_encode<4, 1, true, RowsSource> : k_tarmac_encode<4, 2, false, RowsSource>; }
  template <bool EXACT, bool STORE, bool GEN>
  static MlpObserveKernel observe_form() {
    return k_tarmac_encode<4, EXACT ? 1 : 2, EXACT, ObserveSource<STORE, GEN>, WindowArgs>;
  }
  template <bool EXACT>
  static MlpObserveKernel observe_form(bool store, bool gen) {
    return store ? (gen ? observe_form<EXACT, true, true>() : observe_form<EXACT, true, false>())
                 : (gen ? observe_form<EXACT, false, true>() : observe_form<EXACT, false, false>());
  }
  static MlpObserveKernel encode_observe_kernel(bool exact, bool store, bool gen) {
    return exact ? observe_form<true>(store, gen) : observe_form<false>(store, gen);
  }
  static MlpKernel rehop_kernel(bool exact) { return exact ? k_tarmac_rehop<4, 1, 5, true> : k_tarmac_rehop<4, 2, 6, false>; }
  static MlpKernel head_kernel(bool exact) { return exact ? k_tarmac_head<4, 20, true> : k_tarmac_head<4, 24, false>; }
};

}  // namespace

extern "C" {

int64_t mdr_tarmac_frag_encode_floats(int32_t num_state, int32_t hidden) {
  return (num_state > 0 && hidden > 0 && num_state <= MAX_F && hidden <= MAX_H) ? Fp32Forms::encode(num_state, hidden) : -1;
}
int64_t mdr_tarmac_frag_proj_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V) ? Fp32Forms::proj(hidden, num_value) : -1;
}
int64_t mdr_tarmac_frag_msg_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V && hidden % 4 == 0 && num_value % 4 == 0) ? Fp32Forms::msg(hidden, num_value) : -1;
}
int64_t mdr_tarmac_frag_head_floats(int32_t hidden, int32_t num_value, int32_t with_comm) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V && hidden % 4 == 0 && num_value % 4 == 0)
             ? Fp32Forms::head(hidden, num_value, with_comm) : -1;
}
int64_t mdr_tarmac_vec_floats(int32_t hidden, int32_t num_value) {
  return (hidden > 0 && num_value > 0 && hidden <= MAX_H && num_value <= MAX_V) ? vec_layout(blocks(hidden), blocks(num_value), blocks(hidden + num_value)).total : -1;
}

int64_t mdr_tarmac_frag_words(const mdr_tarmac_actor_t* actor, int32_t part) {
  if (!actor || actor->struct_size != sizeof(mdr_tarmac_actor_t) || part < 0 || part > 3) return -1;
  const int F = actor->num_state, H = actor->hidden, K = actor->num_key, V = actor->num_value, wc = actor->with_comm != 0;
  if (!shape_positive(F, H, K, V) || !shape_covered(F, H, K, V)) return -1;
  auto words = [&](auto frag) { return part == 0 ? frag.encode(F, H) : part == 1 ? frag.proj(H, V) : part == 2 ? frag.msg(H, V) : frag.head(H, V, wc); };
  return actor->precision == MDR_TARMAC_FP32 ? words(FragFloats{}) : actor->precision == MDR_TARMAC_BF16X3 ? words(FragWords{}) : -1;
}

int64_t mdr_tarmac_actor_workspace_bytes(const mdr_tarmac_actor_t* actor, int64_t nb_agents) {
  if (!actor || actor->struct_size != sizeof(mdr_tarmac_actor_t) || nb_agents < 0) return -1;
  const int H = actor->hidden, K = actor->num_key, V = actor->num_value;
  if (!shape_positive(1, H, K, V)) return -1;
  int64_t floats = H;
  if (actor->with_comm) floats += V + K + K + V + (actor->num_hops > 1 ? H : 0);
  return nb_agents * floats * (int64_t)sizeof(float);
}

// The argument checks of a sample, then its launch chain (run_chain, mdr_tarmac_mlp.h) in the actor's precision.  `o` == nullptr: from the
// observation rows `obs`; else from the env's compact state (`obs` unused), `rows_out` optional.  Every refusal comes before the first launch.
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
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  return actor->precision == MDR_TARMAC_BF16X3
             ? mdr::tarmac_sample_bf16(actor, obs, o, rows_out, nb_envs, nb_houses, seed, step, step_dev, workspace, action, a_prob, probs, cus, stream)
             : run_chain<Fp32Forms>(actor, obs, o, rows_out, nb_envs, nb_houses, seed, step, step_dev, workspace, action, a_prob, probs, cus, stream);
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
