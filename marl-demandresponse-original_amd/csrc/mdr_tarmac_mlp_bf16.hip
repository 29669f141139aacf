// TarMAC-PPO actor, the per-agent MLPs of mdr_tarmac_mlp.hip on v_mfma_f32_16x16x32_bf16 (mdr_tarmac_actor_t.precision =
// MDR_TARMAC_BF16X3): every product is Wh xh + Wl xh + Wh xl on operands split into a bf16 head and tail (mdr_bf16_split.h), fp32
// accumulators that start from the fp32 bias, as k_actor_sample_bf16 (mdr_policy.hip).  Activations, the head's last layer, the
// softmax and the draw are the fp32 vector code of the exact forms; mdr_tarmac_comm runs unchanged on the fp32 workspace.
//
// Operand layout: A[row = lane & 15][k = 8 g + j], B[k = 8 g + j][col = lane & 15], g = lane >> 4, j < 8; C/D col = lane & 15, row =
// 4 g + reg.  A k-step fed from memory covers 32 consecutive floats of the agent's row, lane group g its floats [32 s + 8 g, + 8).  A
// k-step fed from registers covers the output blocks 2 s and 2 s + 1 of the previous layer: element j is the lane's own accumulator
// register [2 s + (j >> 2)][j & 3] - no LDS and no lane movement for the activations.  Whatever a k-step covers past the end of its
// input (a row's tail, the second half of an odd block count) is an explicit zero on both sides: the fragments carry zero weights
// there, and the lane builds a zero operand instead of reading on.
//
// A wavefront takes NCOL = 2 column blocks of 16 agents per tile: every weight fragment read from LDS feeds two sets of MFMAs.
// Fragments in LDS: 2 KiB per (k-step, output block) pair, [t = head | tail][lane][8 bf16] - 94 KB (encode) and 117 KB (rehop) at
// the reference's sizes, 98 / 127 KB at the largest covered shape: one workgroup of 8 waves per CU, two waves per SIMD.
//
// Two instantiations per kernel, as the fp32 forms: the block counts of the reference's sizes (H = 64, V <= 16) at compile time, and a
// general form compiled for the largest covered shape whose loops stop at the run-time block counts.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdr_bf16_split.h"
#include "mdr_tarmac_mlp.h"

namespace {

constexpr int WAVES_BF16 = 8;      // per workgroup: two per SIMD, up to 256 registers
constexpr int NCOL = 2;         // 16-agent column blocks per wavefront and tile

template <int MB>
__device__ __forceinline__ void init_bias(const float* bias, int g, int mb, f32x4 (&out)[NCOL][MB]) {
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const f32x4 v = b < mb ? *reinterpret_cast<const f32x4*>(bias + 16 * b + 4 * g) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < NCOL; ++c) out[c][b] = v;
  }
}

// out += W . B for one k-step: `step` -> its mbo (k-step, block) pairs, each [head | tail][64 lanes] fragments of 8 bf16
template <int MBO, bool EXACT>
__device__ __forceinline__ void mma_step(const uint4* step, int mbo, int lane, const bf16x8 (&Bh)[NCOL], const bf16x8 (&Bl)[NCOL],
                                         f32x4 (&out)[NCOL][MBO]) {
#pragma unroll
  for (int mb = 0; mb < MBO; ++mb) {
    if (EXACT || mb < mbo) {
      const bf16x8 Ah = __builtin_bit_cast(bf16x8, step[(mb * 2 + 0) * 64 + lane]);
      const bf16x8 Al = __builtin_bit_cast(bf16x8, step[(mb * 2 + 1) * 64 + lane]);
#pragma unroll
      for (int c = 0; c < NCOL; ++c) {
        out[c][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh[c], out[c][mb], 0, 0, 0);
        out[c][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al, Bh[c], out[c][mb], 0, 0, 0);
        out[c][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bl[c], out[c][mb], 0, 0, 0);
      }
    }
  }
}

// The B operands of k-step s fed from the previous layer's accumulators: blocks 2 s and 2 s + 1, zero past the last block
template <int MBI, int ACT>
__device__ __forceinline__ void split_regs(const f32x4 (&in)[NCOL][MBI], int s, bf16x8 (&Bh)[NCOL], bf16x8 (&Bl)[NCOL]) {
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int b = 2 * s + (j >> 2);
      v[j] = b < MBI ? activate<ACT>(in[c][b < MBI ? b : 0][j & 3]) : 0.0f;
    }
    uint4 bh, bl;
    split8(v, bh, bl);
    Bh[c] = __builtin_bit_cast(bf16x8, bh);
    Bl[c] = __builtin_bit_cast(bf16x8, bl);
  }
}

// The B operands of a k-step fed from memory: floats [first, first + 8) of each column block's row of D floats, zero past the row.
// `vec`: every row is 16-byte aligned (first is a multiple of 8).
__device__ __forceinline__ void split_rows(const float* const (&row)[NCOL], int first, int D, int vec, bf16x8 (&Bh)[NCOL], bf16x8 (&Bl)[NCOL]) {
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    float v[8];
    if (vec && first + 8 <= D) {
      const float4 lo = *reinterpret_cast<const float4*>(row[c] + first);
      const float4 hi = *reinterpret_cast<const float4*>(row[c] + first + 4);
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = first + j < D ? row[c][first + j] : 0.0f;
    }
    uint4 bh, bl;
    split8(v, bh, bl);
    Bh[c] = __builtin_bit_cast(bf16x8, bh);
    Bl[c] = __builtin_bit_cast(bf16x8, bl);
  }
}

// The agents of tile t: column block c holds agents (t NCOL + c) 16 + r; rows past the last agent are read at the last agent's
struct Tile {
  int64_t agent[NCOL], ac[NCOL];
  bool valid[NCOL];
};

__device__ __forceinline__ Tile tile_of(int64_t t, int r, int64_t A) {
  Tile T;
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    T.agent[c] = (t * NCOL + c) * 16 + r;
    T.valid[c] = T.agent[c] < A;
    T.ac[c] = T.valid[c] ? T.agent[c] : A - 1;
  }
  return T;
}

template <int MB>
__device__ __forceinline__ void store_blocks(const f32x4 (&x)[NCOL][MB], float* const (&row)[NCOL], const bool (&valid)[NCOL], int n, int g) {
#pragma unroll
  for (int c = 0; c < NCOL; ++c)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
      if (valid[c] && 16 * mb + 4 * g < n) *reinterpret_cast<f32x4*>(row[c] + 16 * mb + 4 * g) = x[c][mb];
}

// hidden2query | hidden2key | hidden2value on the hidden state a lane holds, which is split ONCE for the three first layers.
// frag_proj: the three first layers [p < 3][sh k-steps][mbh pairs], then the second layers of query (1 block), key (1), value (mbv).
template <int MBH, int MBV, bool EXACT>
__device__ __forceinline__ void projections(const uint4* fp, const float* vec, const VecLayout& L, const f32x4 (&h)[NCOL][MBH], int mbh, int mbv,
                                            int K, int V, float* const (&qkv_row)[NCOL], const bool (&valid)[NCOL], int lane) {
  constexpr int SH = (MBH + 1) / 2;
  const int g = lane >> 4;
  const int sh = EXACT ? SH : ksteps_regs(mbh);
  bf16x8 Hh[SH][NCOL], Hl[SH][NCOL];
#pragma unroll
  for (int s = 0; s < SH; ++s)
    if (EXACT || s < sh) split_regs<MBH, ACT_NONE>(h, s, Hh[s], Hl[s]);
  const int n1 = sh * mbh * 128;      // uint4 of one first layer
  const uint4* f2 = fp + 3 * n1;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    f32x4 t[NCOL][MBH];
    init_bias<MBH>(vec + L.p1 + p * 16 * mbh, g, mbh, t);
#pragma unroll
    for (int s = 0; s < SH; ++s)
      if (EXACT || s < sh) mma_step<MBH, EXACT>(fp + p * n1 + s * mbh * 128, mbh, lane, Hh[s], Hl[s], t);
    if (p < 2) {
      f32x4 o[NCOL][1];
      init_bias<1>(vec + (p == 0 ? L.q2 : L.k2), g, 1, o);
#pragma unroll
      for (int s = 0; s < SH; ++s)
        if (EXACT || s < sh) {
          bf16x8 Bh[NCOL], Bl[NCOL];
          split_regs<MBH, ACT_TANH>(t, s, Bh, Bl);
          mma_step<1, true>(f2 + (p * sh + s) * 128, 1, lane, Bh, Bl, o);
        }
      float* dst[NCOL];
#pragma unroll
      for (int c = 0; c < NCOL; ++c) dst[c] = qkv_row[c] + p * K;
      store_blocks<1>(o, dst, valid, K, g);
    } else {
      f32x4 o[NCOL][MBV];
      init_bias<MBV>(vec + L.v2, g, mbv, o);
#pragma unroll
      for (int s = 0; s < SH; ++s)
        if (EXACT || s < sh) {
          bf16x8 Bh[NCOL], Bl[NCOL];
          split_regs<MBH, ACT_TANH>(t, s, Bh, Bl);
          mma_step<MBV, EXACT>(f2 + (2 * sh + s * mbv) * 128, mbv, lane, Bh, Bl, o);
        }
      float* dst[NCOL];
#pragma unroll
      for (int c = 0; c < NCOL; ++c) dst[c] = qkv_row[c] + 2 * K;
      store_blocks<MBV>(o, dst, valid, V, g);
    }
  }
}

// The two halves of a split k-step of 8 floats per column block
__device__ __forceinline__ void split_cols(const float (&v)[NCOL][8], bf16x8 (&Bh)[NCOL], bf16x8 (&Bl)[NCOL]) {
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    uint4 bh, bl;
    split8(v[c], bh, bl);
    Bh[c] = __builtin_bit_cast(bf16x8, bh);
    Bl[c] = __builtin_bit_cast(bf16x8, bl);
  }
}

// Where k_tarmac_encode_bf16's 32 agents get the floats of the two row-fed k-steps.  begin() for tile t; operands(s) -> the B operands
// of k-step s; after_layer1() once both are split; end().
struct RowsSource : NoHooks {      // the agents' observation rows
  static constexpr bool WINDOWS = false;
  const float* row[NCOL];
  int D, vec;
  __device__ __forceinline__ RowsSource(int64_t, int64_t) {}
  __device__ __forceinline__ void begin(int64_t, const Tile& T, const float* in0, int64_t ld0, int D0, int vec0) {
#pragma unroll
    for (int c = 0; c < NCOL; ++c) row[c] = in0 + T.ac[c] * ld0;
    D = D0, vec = vec0;
  }
  __device__ __forceinline__ void operands(int s, int g, bf16x8 (&Bh)[NCOL], bf16x8 (&Bl)[NCOL]) { split_rows(row, 32 * s + 8 * g, D, vec, Bh, Bl); }
};

// Observe -> act (mdr_env_tarmac_actor_sample): the floats are read from the wave's LDS window (ObserveWindow, mdr_tarmac_mlp.h)
// instead of observation rows, as ObserveSource of mdr_tarmac_mlp.hip does for the fp32 form.  A tile is 32 consecutive agents -
// column block c holds the tile rows 16 c + r - staged as k_actor_observe_bf16 (mdr_policy.hip) stages its tiles of 32; element j of
// lane group g in k-step s is normStateDict feature n = 32 s + 8 g + j, and an explicit zero from n = 51 on, as split_rows builds it.
// Row stride: TARMAC_OBS_ROW = 60 for the same 4-byte reads of one column of 16 consecutive rows.  8 windows of 7680 bytes beside
// ~95 KB of fragments: 158 KB with the row table.
// OVERLAP: the loads of the next tile are issued before the tile's matrix work; its rows are staged once both k-steps have been
// split.  The general form has no registers left to carry them, or the next tile's features, across the layers (it spills with
// them): it loads and stages at the tile's end and reads its features when the tile starts.
template <bool OVERLAP, bool STORE, bool GEN>
struct ObserveSource : ObserveWindow<16 * NCOL, STORE, GEN> {
  using W = ObserveWindow<16 * NCOL, STORE, GEN>;
  static constexpr bool WINDOWS = true;
  static constexpr int TILE = 16 * NCOL;
  float xr[NCOL][16];      // element j of k-step s: [8 s + j]

  __device__ __forceinline__ ObserveSource(int64_t A, int64_t ntiles, const WindowArgs& x) : W{x.o, x.rows_out, A, ntiles} {}

  __device__ __forceinline__ void gather(int64_t first_agent) {
    const int g = this->lane0 >> 4, r = this->lane0 & 15;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) this->lockout_quotients(16 * c + r, g);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    this->store_rows(first_agent);
  }
  __device__ __forceinline__ void feats() {
    const int g = this->lane0 >> 4, r = this->lane0 & 15;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      const float* row = this->rows + (16 * c + r) * W::ROW;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int n = 32 * (k >> 3) + 8 * g + (k & 7);
        const float v = row[W::at(min(n, 50))];
        xr[c][k] = n < 51 ? v : 0.0f;
      }
    }
  }
  __device__ __forceinline__ void prime(int64_t wave, int64_t nwaves) {
    this->start(wave, nwaves);
    if (wave < this->ntiles) {
      this->load(wave * TILE);
      this->stage_rows();
      observe_window_fence();
      gather(wave * TILE);
      if (OVERLAP) feats();
    }
  }
  __device__ __forceinline__ void begin(int64_t t, const Tile&, const float*, int64_t, int, int) {
    if (!OVERLAP) feats();
    this->advance(t);
    if (OVERLAP && this->more) this->load(this->next_tile * TILE);
  }
  __device__ __forceinline__ void operands(int s, int, bf16x8 (&Bh)[NCOL], bf16x8 (&Bl)[NCOL]) {
    float v[NCOL][8];
#pragma unroll
    for (int c = 0; c < NCOL; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[c][j] = xr[c][8 * s + j];
    split_cols(v, Bh, Bl);
  }
  __device__ __forceinline__ void after_layer1() {      // the window is free for the next tile's rows
    if (OVERLAP && this->more) this->stage_rows();
  }
  __device__ __forceinline__ void end() {
    if (this->more) {
      if (!OVERLAP) {
        this->load(this->next_tile * TILE);
        this->stage_rows();
      }
      observe_window_fence();
      gather(this->next_tile * TILE);
      if (OVERLAP) feats();
    }
  }
};

// obs2hidden on the source's floats, x -> cat, the projections -> qkv.  The observe source runs with as many of the form's waves as
// its windows leave room for.
// frag_encode: obs2hidden.0 [S0 = ceil(F / 32) k-steps fed from the obs row][mbh pairs], then obs2hidden.2 [ceil(mbh / 2)][mbh]
template <int MBH, int MBV, bool EXACT, class Source, class... SourceArgs>
__global__ __launch_bounds__(64 * WAVES_BF16) void k_tarmac_encode_bf16(MlpArgs a, SourceArgs... x) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Source src(a.A, a.ntiles, x...);
  const int nw = Source::WINDOWS ? (int)(blockDim.x >> 6) : WAVES_BF16;
  const Staged S = stage_weights(lds, Fragments{a.fa, a.fp, a.vec, a.na, a.np, a.nvec}, a.with_comm != 0, nw,
                                 [&]() { src.carve(lds + a.na + a.np + a.nvec, nw); });
  src.prime(S.wave, S.nwaves);
  const float* vec = S.vec;
  const uint4* fa4 = reinterpret_cast<const uint4*>(S.fa);
  const uint4* fp4 = reinterpret_cast<const uint4*>(S.fp);
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv;
  constexpr int SH = (MBH + 1) / 2;
  const int sh = EXACT ? SH : ksteps_regs(mbh);
  const VecLayout L = vec_layout(mbh, mbv, a.mbm);
  const uint4* f2 = fa4 + a.S0 * mbh * 128;
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const Tile T = tile_of(t, S.r, a.A);
    src.begin(t, T, a.in0, a.ld0, a.D0, a.vec0);
    float* cat_row[NCOL];
    float* qkv_row[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      cat_row[c] = a.cat + T.ac[c] * a.ldcat;
      qkv_row[c] = a.qkv + T.ac[c] * a.ldqkv;
    }
    f32x4 t1[NCOL][MBH], x1[NCOL][MBH];
    init_bias<MBH>(vec + L.o1, g, mbh, t1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (s < a.S0) {
        bf16x8 Bh[NCOL], Bl[NCOL];
        src.operands(s, g, Bh, Bl);
        mma_step<MBH, EXACT>(fa4 + s * mbh * 128, mbh, lane, Bh, Bl, t1);
      }
    src.after_layer1();
    init_bias<MBH>(vec + L.o2, g, mbh, x1);
#pragma unroll
    for (int s = 0; s < SH; ++s)
      if (EXACT || s < sh) {
        bf16x8 Bh[NCOL], Bl[NCOL];
        split_regs<MBH, ACT_RELU>(t1, s, Bh, Bl);
        mma_step<MBH, EXACT>(f2 + s * mbh * 128, mbh, lane, Bh, Bl, x1);
      }
    store_blocks<MBH>(x1, cat_row, T.valid, a.H, g);
    if (a.with_comm) projections<MBH, MBV, EXACT>(fp4, vec, L, x1, mbh, mbv, a.K, a.V, qkv_row, T.valid, lane);
    src.end();
  }
}

// frag_msg: msg_state2state.0 [S0 = ceil(V / 32) k-steps fed from the comm columns, then S1 = ceil(H / 32) fed from h][mbm pairs],
// then msg_state2state.2 [ceil(mbm / 2)][mbh]
template <int MBH, int MBV, int MBM, bool EXACT>
__global__ __launch_bounds__(64 * WAVES_BF16) void k_tarmac_rehop_bf16(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Staged S = stage_weights(lds, Fragments{a.fa, a.fp, a.vec, a.na, a.np, a.nvec}, true, WAVES_BF16);
  const float* vec = S.vec;
  const uint4* fa4 = reinterpret_cast<const uint4*>(S.fa);
  const uint4* fp4 = reinterpret_cast<const uint4*>(S.fp);
  const int mbh = EXACT ? MBH : a.mbh, mbv = EXACT ? MBV : a.mbv, mbm = EXACT ? MBM : a.mbm;
  constexpr int SM = (MBM + 1) / 2;
  const int sm = EXACT ? SM : ksteps_regs(mbm);
  const VecLayout L = vec_layout(mbh, mbv, mbm);
  const uint4* f1h = fa4 + a.S0 * mbm * 128;
  const uint4* f2 = f1h + a.S1 * mbm * 128;
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const Tile T = tile_of(t, S.r, a.A);
    const float* rc[NCOL];
    const float* rh[NCOL];
    float* st_row[NCOL];
    float* qkv_row[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      rc[c] = a.in0 + T.ac[c] * a.ld0;
      rh[c] = a.in1 + T.ac[c] * a.ld1;
      st_row[c] = a.state + T.ac[c] * (int64_t)a.H;
      qkv_row[c] = a.qkv + T.ac[c] * a.ldqkv;
    }
    f32x4 m[NCOL][MBM], h[NCOL][MBH];
    init_bias<MBM>(vec + L.m1, g, mbm, m);
    {
      bf16x8 Bh[NCOL], Bl[NCOL];      // V <= 32: one k-step
      split_rows(rc, 8 * g, a.V, a.vec0, Bh, Bl);
      mma_step<MBM, EXACT>(fa4, mbm, lane, Bh, Bl, m);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (s < a.S1) {
        bf16x8 Bh[NCOL], Bl[NCOL];
        split_rows(rh, 32 * s + 8 * g, a.H, a.vec1, Bh, Bl);
        mma_step<MBM, EXACT>(f1h + s * mbm * 128, mbm, lane, Bh, Bl, m);
      }
    init_bias<MBH>(vec + L.m2, g, mbh, h);
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (EXACT || s < sm) {
        bf16x8 Bh[NCOL], Bl[NCOL];
        split_regs<MBM, ACT_TANH>(m, s, Bh, Bl);
        mma_step<MBH, EXACT>(f2 + s * mbh * 128, mbh, lane, Bh, Bl, h);
      }
    store_blocks<MBH>(h, st_row, T.valid, a.H, g);
    projections<MBH, MBV, EXACT>(fp4, vec, L, h, mbh, mbv, a.K, a.V, qkv_row, T.valid, lane);
  }
}

// frag_head: [S0 = ceil(D / 32) k-steps fed from the row [x, comm] as it lies in cat][mbh pairs], D = H + V (H without communication)
template <int MBH, bool EXACT>
__global__ __launch_bounds__(64 * WAVES_BF16) void k_tarmac_head_bf16(MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Staged S = stage_weights(lds, Fragments{a.fa, nullptr, a.vec, a.na, 0, a.nvec}, false, WAVES_BF16);
  const float* vec = S.vec;
  const uint4* fa4 = reinterpret_cast<const uint4*>(S.fa);
  const int mbh = EXACT ? MBH : a.mbh;
  const VecLayout L = vec_layout(mbh, a.mbv, a.mbm);
  const float bias3 = vec[L.b3];
  const DrawArgs draw{a.action, a.a_prob, a.probs, a.greedy, a.k0, a.k1, a.step_lo, a.step_hi, a.step_dev};
  for (int64_t t = S.wave; t < a.ntiles; t += S.nwaves) {
    const int lane = tile_local(S.lane0), g = lane >> 4;
    const Tile T = tile_of(t, S.r, a.A);
    const float* row[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) row[c] = a.in0 + T.ac[c] * a.ld0;
    f32x4 acc[NCOL][MBH];
    init_bias<MBH>(vec + L.h1, g, mbh, acc);
#pragma unroll
    for (int s = 0; s < 3; ++s)      // D <= 96
      if (s < a.S0) {
        bf16x8 Bh[NCOL], Bl[NCOL];
        split_rows(row, 32 * s + 8 * g, a.D0, a.vec0, Bh, Bl);
        mma_step<MBH, EXACT>(fa4 + s * mbh * 128, mbh, lane, Bh, Bl, acc);
      }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      f32x4 col[MBH];      // a copy the compiler sees through: acc itself stays out of the helper's hands and in separate registers
#pragma unroll
      for (int mb = 0; mb < MBH; ++mb) col[mb] = acc[c][mb];
      head_finish<MBH, EXACT>(col, vec, L, mbh, g, bias3, draw, T.agent[c], T.valid[c]);
    }
  }
}

struct Bf16Forms : FragWords {
  static constexpr int TILE = 16 * NCOL;
  static int waves(bool) { return WAVES_BF16; }
  static int row_steps(int n) { return ksteps_rows(n); }
  static int whole_vectors(int, int D) { return D % 4 == 0; }
  static bool head_exact(int mbh, int) { return mbh == 4; }
  static MlpKernel encode_kernel(bool exact) {
    return exact ? k_tarmac_encode_bf16<4, 1, true, RowsSource> : k_tarmac_encode_bf16<4, 2, false, RowsSource>;
  }
  template <bool EXACT, bool STORE, bool GEN>
  static MlpObserveKernel observe_form() {
    return k_tarmac_encode_bf16<4, EXACT ? 1 : 2, EXACT, ObserveSource<EXACT, STORE, GEN>, WindowArgs>;
  }
  template <bool EXACT>
  static MlpObserveKernel observe_form(bool store, bool gen) {
    return store ? (gen ? observe_form<EXACT, true, true>() : observe_form<EXACT, true, false>())
                 : (gen ? observe_form<EXACT, false, true>() : observe_form<EXACT, false, false>());
  }
  static MlpObserveKernel encode_observe_kernel(bool exact, bool store, bool gen) {
    return exact ? observe_form<true>(store, gen) : observe_form<false>(store, gen);
  }
  static MlpKernel rehop_kernel(bool exact) { return exact ? k_tarmac_rehop_bf16<4, 1, 5, true> : k_tarmac_rehop_bf16<4, 2, 6, false>; }
  static MlpKernel head_kernel(bool exact) { return exact ? k_tarmac_head_bf16<4, true> : k_tarmac_head_bf16<4, false>; }
};

}  // namespace

namespace mdr {

int tarmac_sample_bf16(const mdr_tarmac_actor_t* actor, const float* obs, const ObserveArgs* o, float* rows_out, int32_t nb_envs, int32_t nb_houses,
                       uint64_t seed, uint64_t step, const int32_t* step_dev, void* workspace, uint8_t* action, float* a_prob, float* probs, int cus,
                       void* stream) {
  return run_chain<Bf16Forms>(actor, obs, o, rows_out, nb_envs, nb_houses, seed, step, step_dev, workspace, action, a_prob, probs, cus, stream);
}

}  // namespace mdr
