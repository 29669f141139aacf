// Observe -> act, the staging every kernel form shares: a wavefront builds the default observation of a tile of consecutive agents
// in its LDS window from the env's compact state (mdr_policy.hip describes the window; k_actor_observe16 / k_actor_observe_bf16
// there and the observe forms of the TarMAC encode kernels in mdr_tarmac_mlp.hip / mdr_tarmac_mlp_bf16.hip read it back).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mdr_device.h"
#include "mdr_kernels.h"

namespace {


// A lane-dependent value hidden from loop-invariant code motion: what is derived from it (LDS addresses of the row copy, 64-bit
// products for the Philox counter) is then re-derived where it is used - one or two vector instructions - instead of being
// hoisted out of the tile loop into registers the loop does not have (r02: those were the kernels' scratch spills).
__device__ __forceinline__ int tile_local(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

constexpr int OBS_HALO = 5, OBS_C = 10, OBS_ROW = 56, OBS_PAD = 16;   // floats; 56 = 40 + 11 + L + 1/L + 3 (16-byte rows)
// The extended form (ObserveArgs.ext; template parameter EXT): optional state columns, c != 10 circular neighbours, link defects.
// A row is [4 c message floats | own features in normStateDict order | zeros up to 64 | L | 1 / L | pad]: feature k of a row is
// normStateDict index (k < 4 c ? own + k : k - 4 c), the packed weights follow (mdr_actor_t.feature_order = 1), F = 4 c + own <= 64.
// The row stride of the extended form is a run-time value (ObserveArgs.row; L and 1 / L sit in its floats row - 2, row - 1): the
// features rounded up to 16 bytes, so that as many windows fit the LDS as for the default shape where the shape allows it.
constexpr int OBS_MAX_C = 13;                         // (run-time strides: 4 c + own + 2 rounded up to 4 * odd, at most 68)
typedef float v4f_nt __attribute__((ext_vector_type(4)));

// between a wave's window stores and its loads of what OTHER lanes stored
__device__ __forceinline__ void observe_window_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

struct HouseRegs {
  float Ta, Tm, tg, db, cap, pm;
  int sso, lk;
  unsigned fl;
  float sig, pw;
  float Ua, Cm, Ca, Hm, COP, latent;   // EXT: the thermal / hvac columns, already divided by their defaults
  float x_od, x_sd, x_cd, x_sh, x_ch, x_sol;   // EXT: the per-env columns (k_observe_env_extras)
};

__device__ __forceinline__ const double* observe_sig_row(const mdr::ObserveArgs& o) {
  if (o.cursor == nullptr) return o.sig_now;
  return o.sig_now + (int64_t)min(o.cursor[0], o.cursor_max + 1) * o.E;   // as rebase(ObsArgs&) in mdr_kernels.hip
}

// A load at a 32-bit byte offset from a wave-uniform base (`global_load v, voffset, s[base:base+1]`): the extended forms read up to 15
// per-house arrays at ONE house index - one offset register instead of a 64-bit address per array (the launcher keeps 4 A below 2^32)
template <class T>
__device__ __forceinline__ T ld32(const T* base, uint32_t byte_offset) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_offset);
}

// the per-house / per-env columns of the extended form (thermal, hvac: per house, divided by their defaults; the rest: k_observe_env_extras)
template <bool ENV = true>   // ENV = false: the per-env columns come later (observe_env_extras_now: whole-tile staging, one env per tile)
__device__ __forceinline__ void observe_load_extras(const mdr::ObserveArgs& o, HouseRegs& r, uint32_t i4, int e) {
  if (o.f_thermal) {
    if (ENV) r.x_od = o.env_extra_a[e];
    r.Ua = ld32(o.Ua, i4) * o.inv_Ua;
    r.Cm = ld32(o.Cm, i4) * o.inv_Cm;
    r.Ca = ld32(o.Ca, i4) * o.inv_Ca;
    r.Hm = ld32(o.Hm, i4) * o.inv_Hm;
  }
  if (o.f_hvac) {
    r.COP = ld32(o.COP, i4) * o.inv_COP;
    r.latent = ld32(o.latent, i4) * o.inv_latent;
  }
  if (!ENV) return;
  if (o.f_day) {
    r.x_sd = o.env_extra_a[(int64_t)o.E + e];
    r.x_cd = o.env_extra_a[2 * (int64_t)o.E + e];
  }
  if (o.f_hour) {
    r.x_sh = o.env_extra_a[3 * (int64_t)o.E + e];
    r.x_ch = o.env_extra_b[e];
  }
  if (o.f_solar) r.x_sol = o.env_extra_b[(int64_t)o.E + e];
}

// The per-env columns of ONE env, fetched when its tile's rows are staged (whole-tile staging: up to six registers less to carry
// from the loads before layer 1 to the staging behind it; the index is wave-uniform)
__device__ __forceinline__ void observe_env_extras_now(const mdr::ObserveArgs& o, HouseRegs& r, int e_uniform) {
  const int e = __builtin_amdgcn_readfirstlane(e_uniform);
  if (o.f_thermal) r.x_od = o.env_extra_a[e];
  if (o.f_day) {
    r.x_sd = o.env_extra_a[(int64_t)o.E + e];
    r.x_cd = o.env_extra_a[2 * (int64_t)o.E + e];
  }
  if (o.f_hour) {
    r.x_sh = o.env_extra_a[3 * (int64_t)o.E + e];
    r.x_ch = o.env_extra_b[e];
  }
  if (o.f_solar) r.x_sol = o.env_extra_b[(int64_t)o.E + e];
}

// the own features of the extended form in normStateDict order (obs_features() in mdr_kernels.hip), optional ones where they belong;
// L and 1 / L behind them in the row's last two floats
__device__ __forceinline__ void observe_write_own_ext(const mdr::ObserveArgs& o, const HouseRegs& r, float* row, int c, int ROW) {
  const float L = (float)r.lk;
  float* own = row + 4 * c;
  int j = 0;
  own[j++] = (r.Ta + o.obs_tshift) * 0.2f;
  own[j++] = (r.Tm + o.obs_tshift) * 0.2f;
  own[j++] = (r.tg + o.obs_tshift) * 0.2f;
  if (o.f_thermal) own[j++] = r.x_od;
  own[j++] = r.db;
  if (o.f_day) {
    own[j++] = r.x_sd;
    own[j++] = r.x_cd;
  }
  if (o.f_hour) {
    own[j++] = r.x_sh;
    own[j++] = r.x_ch;
  }
  if (o.f_solar) own[j++] = r.x_sol;
  own[j++] = r.cap * o.inv_cap;
  if (o.f_thermal) {
    own[j++] = r.Ua;
    own[j++] = r.Cm;
    own[j++] = r.Ca;
    own[j++] = r.Hm;
  }
  if (o.f_hvac) {
    own[j++] = r.COP;
    own[j++] = r.latent;
  }
  own[j++] = (r.fl & 1u) ? 1.0f : 0.0f;
  own[j++] = (r.fl & 2u) ? 1.0f : 0.0f;
  own[j++] = (float)r.sso / L;
  own[j++] = L / L;
  own[j++] = r.sig;
  own[j++] = r.pw;
  row[ROW - 2] = L;
  row[ROW - 1] = 1.0f / L;
}

// A tile of TILE consecutive agents inside ONE env (N a multiple of the tile): lane l stages the house at window position l, the window
// being the tile's houses and the c around them (`before` of them in front; the default: 5 + 5)
template <int TILE, bool EXT = false>
__device__ __forceinline__ HouseRegs observe_load(const mdr::ObserveArgs& o, const double* sig_row, int e, int h0, int lane) {
  const int before = EXT ? o.before : OBS_HALO, c = EXT ? o.c : 2 * OBS_HALO;
  HouseRegs r{};
  if (lane < TILE + c) {
    int hh = h0 - before + lane;
    hh += hh < 0 ? o.N : 0;
    hh -= hh >= o.N ? o.N : 0;
    const int64_t i = (int64_t)e * o.N + hh;
    if (EXT) {
      const uint32_t i1 = (uint32_t)i, i4 = i1 << 2;
      r.Ta = ld32(o.Ta, i4);
      r.Tm = ld32(o.Tm, i4);
      r.tg = ld32(o.target, i4);
      r.db = ld32(o.deadband, i4);
      r.cap = ld32(o.capacity, i4);
      r.pm = ld32(o.P_max, i4);
      r.sso = ld32(o.sso, i4);
      r.lk = ld32(o.lockout, i4);
      r.fl = ld32(o.flags, i1);
      observe_load_extras<false>(o, r, i4, e);
    } else {
      r.Ta = o.Ta[i];
      r.Tm = o.Tm[i];
      r.tg = o.target[i];
      r.db = o.deadband[i];
      r.cap = o.capacity[i];
      r.pm = o.P_max[i];
      r.sso = o.sso[i];
      r.lk = o.lockout[i];
      r.fl = o.flags[i];
    }
  }
  r.sig = (float)(sig_row[e] * o.inv_obs_norm);   // utils.py:832-841, per env
  r.pw = (float)(o.P[e] * o.inv_obs_norm);
  return r;
}

template <int TILE, bool EXT = false, int ROWC = 0>
__device__ __forceinline__ void observe_stage(const mdr::ObserveArgs& o, const HouseRegs& r, float* rows, int lane, int e = 0) {
  const float4 rec = make_float4((r.Ta - r.tg) * 0.2f, (float)r.sso, ((r.fl & 1u) ? r.pm : 0.0f) * o.inv_norm_reg, r.pm * o.inv_norm_reg);
  if (EXT) {
    const int before = o.before, c = o.c;
    const int ROW = ROWC ? ROWC : o.row;   // (the fp32 forms know their stride at compile time)
    if (lane >= TILE + c) return;
#pragma unroll
    for (int m = 0; m < OBS_MAX_C; ++m) {
      if (m >= c) break;
      const int off = m < before ? m - before : m - before + 1;   // slot m listens to house h + off (env 816-828)
      const int rr = lane - before - off;                         // ... so this house is slot m of the agent at tile row rr
      if (rr >= 0 && rr < TILE) *reinterpret_cast<float4*>(rows + rr * ROW + 4 * m) = rec;
    }
    const int rr = lane - before;
    HouseRegs own = r;
    observe_env_extras_now(o, own, e);
    if (rr >= 0 && rr < TILE) observe_write_own_ext(o, own, rows + rr * ROW, c, ROW);
    return;
  }
  if (lane >= TILE + 2 * OBS_HALO) return;
  constexpr int DROW = ROWC ? ROWC : OBS_ROW;   // (the default form: OBS_ROW unless the kernel picks its own stride)
#pragma unroll
  for (int m = 0; m < OBS_C; ++m) {
    const int rr = lane - m - (m >= OBS_HALO ? 1 : 0);   // the agent this house is sender slot m of (env 816-828)
    if (rr >= 0 && rr < TILE) *reinterpret_cast<float4*>(rows + rr * DROW + 4 * m) = rec;
  }
  const int rr = lane - OBS_HALO;
  if (rr >= 0 && rr < TILE) {
    const float L = (float)r.lk;
    float* own = rows + rr * DROW + 4 * OBS_C;
    *reinterpret_cast<float4*>(own) = make_float4((r.Ta + o.obs_tshift) * 0.2f, (r.Tm + o.obs_tshift) * 0.2f, (r.tg + o.obs_tshift) * 0.2f, r.db);
    *reinterpret_cast<float4*>(own + 4) = make_float4(r.cap * o.inv_cap, (r.fl & 1u) ? 1.0f : 0.0f, (r.fl & 2u) ? 1.0f : 0.0f, (float)r.sso / L);
    *reinterpret_cast<float4*>(own + 8) = make_float4(L / L, r.sig, r.pw, L);
    own[12] = 1.0f / L;
  }
}

// ---- any cluster size (N >= 11): a tile of TILE consecutive agents may start anywhere in an env and span several (the reference
// trains with 20 houses and deploys with 50).  The tile is cut into per-env segments; a segment of `len` houses [hs, hs + len)
// stages the window of houses hs - 5 .. hs + len + 4 (circular) - or the whole env when that wraps onto itself (len + 10 >= N).
// Windows are laid out one after the other over the lanes (at most 52 lanes for TILE = 32, 36 for TILE = 16: checked for every
// N and tile start); a staging lane keeps (house, segment bounds, first tile row of the segment) with its loaded values.
struct SegSlot {
  int j, hs, len, rb;   // this lane's house in its segment's env; the segment's receivers [hs, hs + len) = tile rows [rb, rb + len)
  bool live;
  int e;                // ... and that env (the extended form fetches its per-env columns when the rows are staged)
};

template <int TILE, bool EXT = false, bool TABLE = false>
__device__ __forceinline__ HouseRegs observe_load_gen(const mdr::ObserveArgs& o, const double* sig_row, int e0, int h0, int64_t a0, int64_t A,
                                                      int lane, SegSlot& slot) {
  // senders before the house / in all (env 816-828).  TABLE (link tables, random_sample): the window is the tile's houses alone -
  // one lane per agent - and the senders' records are gathered when the rows are staged
  const int before = TABLE ? 0 : (EXT ? o.before : OBS_HALO), c = TABLE ? 0 : (EXT ? o.c : 2 * OBS_HALO);
  HouseRegs r{};
  slot = SegSlot{0, 0, 0, 0, false, 0};
  // the segment walk is wave-uniform: keep it on the scalar unit (the tile index comes out of threadIdx, which the compiler
  // cannot see is uniform across the wave)
  int rem = __builtin_amdgcn_readfirstlane((int)((A - a0) < (int64_t)TILE ? (A - a0) : (int64_t)TILE));
  int e = __builtin_amdgcn_readfirstlane(e0), hs = __builtin_amdgcn_readfirstlane(h0), wb = 0, rb = 0, my_e = 0;
#pragma unroll 1
  while (rem > 0) {                          // at most 4 segments
    const int len = min(o.N - hs, rem);
    const bool whole = len + c >= o.N;
    const int start = whole ? 0 : (hs - before + o.N) % o.N;
    const int wlen = whole ? o.N : len + c;
    if (lane >= wb && lane < wb + wlen) {
      int j = start + (lane - wb);
      j -= j >= o.N ? o.N : 0;
      slot = SegSlot{j, hs, len, rb, true, e};
      my_e = e;
    }
    wb += wlen;
    rb += len;
    rem -= len;
    hs = 0;
    e += 1;
  }
  if (slot.live) {
    const int64_t i = (int64_t)my_e * o.N + slot.j;
    if (EXT) {
      const uint32_t i1 = (uint32_t)i, i4 = i1 << 2;
      r.Ta = ld32(o.Ta, i4);
      r.Tm = ld32(o.Tm, i4);
      r.tg = ld32(o.target, i4);
      r.db = ld32(o.deadband, i4);
      r.cap = ld32(o.capacity, i4);
      r.pm = ld32(o.P_max, i4);
      r.sso = ld32(o.sso, i4);
      r.lk = ld32(o.lockout, i4);
      r.fl = ld32(o.flags, i1);
      observe_load_extras<false>(o, r, i4, my_e);
    } else {
      r.Ta = o.Ta[i];
      r.Tm = o.Tm[i];
      r.tg = o.target[i];
      r.db = o.deadband[i];
      r.cap = o.capacity[i];
      r.pm = o.P_max[i];
      r.sso = o.sso[i];
      r.lk = o.lockout[i];
      r.fl = o.flags[i];
    }
    r.sig = (float)(sig_row[my_e] * o.inv_obs_norm);
    r.pw = (float)(o.P[my_e] * o.inv_obs_norm);
  }
  return r;
}

template <bool EXT = false, int ROWC = 0, bool TABLE = false>
__device__ __forceinline__ void observe_stage_gen(const mdr::ObserveArgs& o, const HouseRegs& r, const SegSlot& slot, float* rows) {
  if (!slot.live) return;
  const int ROW = ROWC ? ROWC : (EXT ? o.row : OBS_ROW);   // (the fp32 extended forms know their stride at compile time)
  const int before = EXT ? o.before : OBS_HALO, c = EXT ? o.c : OBS_C;
  const float4 rec = make_float4((r.Ta - r.tg) * 0.2f, (float)r.sso, ((r.fl & 1u) ? r.pm : 0.0f) * o.inv_norm_reg, r.pm * o.inv_norm_reg);
#pragma unroll
  for (int m = 0; m < (EXT ? OBS_MAX_C : OBS_C); ++m) {
    if (TABLE || (EXT && m >= c)) break;
    const int off = m < before ? m - before : m - before + 1;   // slot m listens to house h + off (env 816-828)
    int h = slot.j - off;                                      // ... so this house is slot m of house j - off
    h += h < 0 ? o.N : 0;
    h -= h >= o.N ? o.N : 0;
    const int k = h - slot.hs;
    if (k >= 0 && k < slot.len) *reinterpret_cast<float4*>(rows + (slot.rb + k) * ROW + 4 * m) = rec;
  }
  const int k = slot.j - slot.hs;
  if (EXT) {
    if (TABLE) {   // this lane's house is a receiver (the window holds nothing else): its c senders by the table, four at a time
      float* row = rows + (slot.rb + k) * ROW;
      const int32_t* ids = o.links + (int64_t)slot.e * o.links_env_stride + (int64_t)slot.j * c;
      const float4* recs = reinterpret_cast<const float4*>(o.msg_rec) + (int64_t)slot.e * o.N;
#pragma unroll 1
      for (int m0 = 0; m0 < c; m0 += 4) {
        const int last = c - 1;
        const int s0 = ids[m0], s1 = ids[min(m0 + 1, last)], s2 = ids[min(m0 + 2, last)], s3 = ids[min(m0 + 3, last)];
        const float4 r0 = recs[s0], r1 = recs[s1], r2 = recs[s2], r3 = recs[s3];
        float* dst = row + 4 * m0;
        *reinterpret_cast<float4*>(dst) = r0;
        if (m0 + 1 < c) *reinterpret_cast<float4*>(dst + 4) = r1;
        if (m0 + 2 < c) *reinterpret_cast<float4*>(dst + 8) = r2;
        if (m0 + 3 < c) *reinterpret_cast<float4*>(dst + 12) = r3;
      }
    }
    if (k >= 0 && k < slot.len) {
      HouseRegs own = r;
      const int e = slot.e;      // per lane here: a tile may span envs
      if (o.f_thermal) own.x_od = o.env_extra_a[e];
      if (o.f_day) {
        own.x_sd = o.env_extra_a[(int64_t)o.E + e];
        own.x_cd = o.env_extra_a[2 * (int64_t)o.E + e];
      }
      if (o.f_hour) {
        own.x_sh = o.env_extra_a[3 * (int64_t)o.E + e];
        own.x_ch = o.env_extra_b[e];
      }
      if (o.f_solar) own.x_sol = o.env_extra_b[(int64_t)o.E + e];
      observe_write_own_ext(o, own, rows + (slot.rb + k) * ROW, c, ROW);
    }
    return;
  }
  if (k >= 0 && k < slot.len) {
    const float L = (float)r.lk;
    float* own = rows + (slot.rb + k) * ROW + 4 * OBS_C;
    *reinterpret_cast<float4*>(own) = make_float4((r.Ta + o.obs_tshift) * 0.2f, (r.Tm + o.obs_tshift) * 0.2f, (r.tg + o.obs_tshift) * 0.2f, r.db);
    *reinterpret_cast<float4*>(own + 4) = make_float4(r.cap * o.inv_cap, (r.fl & 1u) ? 1.0f : 0.0f, (r.fl & 2u) ? 1.0f : 0.0f, (float)r.sso / L);
    *reinterpret_cast<float4*>(own + 8) = make_float4(L / L, r.sig, r.pw, L);
    own[12] = 1.0f / L;
  }
}

// Optional side product of observe -> act: the tile's observation rows, in normStateDict order, for the transition buffer
// (train_ppo.py:87-98 stores `state` with every transition).  The window holds them already - in staging order and with the raw
// seconds_since_off, which the gathering lanes replace by the quotient they computed - so the tile's TILE * 51 contiguous
// output floats are copied out with 16-byte non-temporal stores through a source-offset table built once per workgroup
// (output float o = 51 r + n  <-  window float OBS_ROW r + (n < 11 ? 40 + n : n - 11)).
template <int TILE, int ROW = OBS_ROW>
__device__ __forceinline__ void observe_build_table(uint16_t* table, int tid, int nthreads) {
  for (int o = tid; o < TILE * 51; o += nthreads) {
    const int r = o / 51, n = o - 51 * r;
    table[o] = (uint16_t)(ROW * r + (n < 11 ? 4 * OBS_C + n : n - 11));
  }
}
template <int TILE>
__device__ __forceinline__ void observe_build_table_ext(uint16_t* table, int tid, int nthreads, int own, int c, int row) {
  const int F = own + 4 * c;
  for (int o = tid; o < TILE * F; o += nthreads) {
    const int r = o / F, n = o - F * r;
    table[o] = (uint16_t)(row * r + (n < own ? 4 * c + n : n - own));
  }
}

template <int TILE, bool EXT = false>
__device__ __forceinline__ void observe_store_rows(const float* rows, const uint16_t* table, float* out_tile, int lane_in, int nrows = TILE, int F = 51) {
  constexpr int QUADS = TILE * (EXT ? 64 : 51) / 4;   // 408 | 204 (EXT: the bound for F = 64)
  const int lane = tile_local(lane_in);
  if (!EXT) F = 51;
  if (((uintptr_t)out_tile & 15u) != 0) {   // a transition buffer whose per-step slice is not 16-byte aligned (A * F % 4 != 0): 4-byte stores
    for (int i = lane; i < nrows * F; i += 64) __builtin_nontemporal_store(rows[table[i]], out_tile + i);
    return;
  }
  const int quads = nrows * F / 4;      // the last tile of a batch may hold fewer agents (F nrows need not be a multiple of 4)
  if (lane < nrows * F - 4 * quads) out_tile[4 * quads + lane] = rows[table[4 * quads + lane]];
#pragma unroll
  for (int i = 0; i < (QUADS + 63) / 64; ++i) {
    const int q = i * 64 + lane;
    if (q < quads) {
      const uint2 src = *reinterpret_cast<const uint2*>(table + 4 * q);   // four 16-bit window offsets
      v4f_nt v = {rows[src.x & 0xFFFFu], rows[src.x >> 16], rows[src.y & 0xFFFFu], rows[src.y >> 16]};
      __builtin_nontemporal_store(v, reinterpret_cast<v4f_nt*>(out_tile) + q);
    }
  }
}

// (env, first house) of a tile, advanced by a fixed stride without a division per tile
struct TileCursor {
  int e, h0, de, dh, N;
  __device__ __forceinline__ void init(int64_t first_agent, int64_t stride_agents, int n) {
    N = n;
    e = (int)(first_agent / n);
    h0 = (int)(first_agent - (int64_t)e * n);
    de = (int)(stride_agents / n);
    dh = (int)(stride_agents - (int64_t)de * n);
  }
  __device__ __forceinline__ void next() {
    e += de;
    h0 += dh;
    if (h0 >= N) {
      h0 -= N;
      e += 1;
    }
  }
};

// ---- the window of one wavefront, as the matrix-core actors use it (the TarMAC encode kernels of mdr_tarmac_mlp.hip /
// mdr_tarmac_mlp_bf16.hip, the 256-unit actor of mdr_mlp_actor_observe.hip)
constexpr int TARMAC_OBS_ROW = 60;      // floats per staged row (ObserveSource, mdr_tarmac_mlp.hip, says why)

// The window of one wavefront behind the staged weights: TILE consecutive agents' rows, staged from the env's compact state by the
// helpers of mdr_observe.h exactly as k_actor_observe16 / k_actor_observe_bf16 (mdr_policy.hip) stage theirs for the default
// observation, and what the two precisions do with it alike.  GEN: tiles that may leave their env (N no multiple of TILE).  STORE:
// the rows are also written to rows_out through the workgroup's offset table.
template <int TILE, bool STORE, bool GEN>
struct ObserveWindow {
  static constexpr int ROW = TARMAC_OBS_ROW, WIN = TILE * ROW;
  const mdr::ObserveArgs& o;
  float* rows_out;
  int64_t A, ntiles;
  float* rows;
  uint16_t* table;      // [TILE * 51] (only when rows are stored)
  const double* sig_row;
  int lane0;
  TileCursor tc;
  SegSlot slot;
  HouseRegs nxt;
  int64_t next_tile, stride;      // the wavefront's tile after this one
  bool more;                      // ... is there

  // normStateDict feature n of a tile row sits at this float of the row
  static __device__ __forceinline__ int at(int n) { return n < 11 ? 4 * OBS_C + n : n - 11; }

  // before the workgroup's barrier: `nw` = as many of the form's waves as the windows leave room for
  __device__ __forceinline__ void carve(float* behind_weights, int nw) {
    const int tid = threadIdx.x;
    rows = behind_weights + (tid >> 6) * WIN;
    table = reinterpret_cast<uint16_t*>(behind_weights + nw * WIN);
    lane0 = tid & 63;
    for (int i = lane0; i < WIN; i += 64) rows[i] = 0.0f;
    if (STORE) observe_build_table<TILE, ROW>(table, tid, 64 * nw);
  }
  __device__ __forceinline__ void start(int64_t wave, int64_t nwaves) {
    sig_row = observe_sig_row(o);
    tc.init(wave * TILE, nwaves * TILE, o.N);
    slot = SegSlot{};
    stride = nwaves;
  }
  __device__ __forceinline__ void advance(int64_t t) {
    next_tile = t + stride;
    more = next_tile < ntiles;
    tc.next();
    nxt = HouseRegs{};
  }
  // the compact state of the tile at the cursor, which starts at first_agent, into registers / from them into the window
  __device__ __forceinline__ void load(int64_t first_agent) {
    nxt = GEN ? observe_load_gen<TILE>(o, sig_row, tc.e, tc.h0, first_agent, A, lane0, slot) : observe_load<TILE>(o, sig_row, tc.e, tc.h0, lane0);
  }
  __device__ __forceinline__ void stage_rows() {
    if (GEN) observe_stage_gen<false, ROW>(o, nxt, slot, rows);
    else observe_stage<TILE, false, ROW>(o, nxt, rows, lane0);
  }
  // the senders' seconds_since_off become quotients by the RECEIVER's lockout, in place: lane group g takes the messages g, g + 4
  // and g + 8 of tile row `r` (k_actor_observe16)
  __device__ __forceinline__ void lockout_quotients(int r, int g) {
    float* row = rows + r * ROW;
    const float lock = row[4 * OBS_C + 11], y = row[4 * OBS_C + 12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int m = g + 4 * i;
      if (m < OBS_C) row[4 * m + 1] = mdr::div_by_lockout(row[4 * m + 1], lock, y);
    }
  }
  __device__ __forceinline__ void store_rows(int64_t first_agent) {
    if (STORE)
      observe_store_rows<TILE>(rows, table, rows_out + first_agent * 51, lane0,
                               GEN ? (int)((A - first_agent) < (int64_t)TILE ? (A - first_agent) : (int64_t)TILE) : TILE);
  }
};

}  // namespace

namespace mdr {

// Lanes the general staging needs for a tile of `tile` agents (c senders per house, N houses per env): a tile is cut into per-env
// segments, each staging its houses plus the c around them - or the whole env when that wraps onto itself; worst case over the tile
// starts (the pattern repeats with the env).
inline int observe_window_lanes(int N, int c, int tile) {
  int worst = 0;
  const int starts = N < 4096 ? N : 1;   // big envs: at most two segments, tile + 2 c lanes
  for (int h0 = 0; h0 < starts; ++h0) {
    int lanes = 0, hs = h0, rem = tile;
    while (rem > 0) {
      const int len = N - hs < rem ? N - hs : rem;
      lanes += len + c >= N ? N : len + c;
      rem -= len;
      hs = 0;
    }
    if (lanes > worst) worst = lanes;
  }
  if (N >= 4096) worst = tile + 2 * c;
  return worst;
}

}  // namespace mdr
