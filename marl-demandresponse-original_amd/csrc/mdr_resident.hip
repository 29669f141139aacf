// The interior steps of mdr_env_rollout with the houses resident in registers (large batches: mdr_api.hip's resident rule).
//
// A translation unit of its own because its loop is bound by vector issue, where code generation options matter that matter to
// no other kernel: build.py can give a single source extra flags (SOURCE_FLAGS, build_variant's source_flags) while every other
// kernel keeps the flags and the instruction stream it had.  The product build passes -fno-slp-vectorize: the thermal map's f32
// operations are plain v_add / v_mul / v_fma instead of SLP-packed pairs (v_pk_*_f32), the same bits and 10 % more house-steps/s in
// bench.py now that one launch covers the rollout (profiles/r12_README.md; with a launch per table window the difference stayed
// under the project's bar, profiles/r11_README.md).  -ffp-contract=on applies here as everywhere.
//
// An interior step has no env-wide reduction, no reward and no obs: step_fused_interior is step_vec's loads, house_step and the
// state stores, and a house depends on itself and on its env's od_old / solar_new rows alone.  So `ro.nsteps` of them are one
// launch: the prologue loads a house through the very helpers the interior step uses (the same bits arrive in registers), the loop
// reads one float2 per env and step - {od_old, solar_new} of that step, from the rollout rows mdr_api.hip fills in front of the launch
// (mdr_rollout_rows.hip: [nsteps + 1][E], the address steps by E entries, the row behind the last step is a spare one so that the
// load one step ahead needs no clamp) - and advances the houses as k_rollout_fused does - lane masks, blank houses in the lanes
// past the env's end so that every ballot sees the whole wave - and the epilogue stores Ta, Tm, sso and flags, nothing else: the
// full step that ends the rollout overwrites every other output.  No LDS, no barrier, no accumulator.
//
// The loop body is house_advance_lean_m (mdr_device.h): the first step of a launch in the general form, every later one in the lean
// form (one add, one compare, one select for the HVAC's integer state), and the lock mask once, behind the last step
// (house_lock_m on the `can` mask that step left in scalar registers).  A blank lane's sso is never stored and is left to grow by
// dt per step: mdr_api.hip keeps dt x (steps of a launch) below 2^31.
//
// Where one lockout holds for every house (UNIFORM_LOCKOUT of the param_uniform word: every configuration the reference trains with)
// the steps behind the first run house_advance_stamp_m instead: the house keeps the TIME its HVAC was last on, not a counter, and the
// launch's step time is a scalar that doubles as the loop's counter - one compare against a scalar and one select steered by on2
// itself for the HVAC's integer state: no add, no OR for the select's mask, no lockout register, no separate loop counter.  The
// same bits (tests/test_stamp_step_algebra.py, tests/test_gpu_rollout_resident_stamps.py).  The word is device-side, so each kernel
// holds both forms of its body behind one wave-uniform branch, each with the registers it needs.
//
// The row of a step.  With the bang-bang rule compiled in (resident_row_ahead) a trip is: the front - the compares, the mask logic
// on the scalar unit and the selects of the HVAC's state machine, which read no row -, then the ONE wait for this step's row, which
// was loaded in the trip before, then the load of the next step's row, right behind that wait (in front of it the wait would cover it
// too), then the back, the thermal map.  A load so has a whole trip of cover.  row_arrived / row_ahead hold the order; the loops
// run two trips per turn with the two row registers changing places, so that no copy stands between a load and its wait.  The
// source said "load the next row, use the one before" before as well, but the compiler folded the two loads into one load of the
// trip's own row at the top of the trip, waited for 27 instructions later.  k_rollout_resident<4,1,256,true> per trip: 61 vector and
// 15.5 other instructions (153 per pair of trips; before: 61 and 17), the counter form 64 and 20 (profiles/r14_README.md).  The
// controllers' loops (BB false) keep the form they had, the load at the top of the trip that uses it: rotated they lose a wave per SIMD.
//
// The step forms it replaces, by env->plan as launch_step picks them:
//   k_rollout_resident<VEC, TILES, THREADS, BB>   for k_step_fused<VEC, TILES, THREADS, 1, ..>: the rows are wave-uniform scalar
//                                                 loads, in flight for a whole trip
//   k_rollout_resident_group<GROUP, VEC, BB>      for k_step_group<GROUP, VEC, 1, ..>: each lane reads its own env's rows with
//                                                 vector loads, neighbouring envs from one line
// BB: the bang-bang rule compiled in; otherwise controller_cmd_m, or - external actions - the caller's buffer, which nothing
// writes during a rollout: read once, one constant mask.
#include <cstdint>

#include "mdr_device.h"
#include "mdr_kernels.h"
#include "mdr_step_common.h"

namespace mdr {

template <int VEC>
__device__ __forceinline__ void resident_load(const StepArgs& a, uint32_t uni, bool coded, bool packed, bool ext, int64_t i, HouseIn* hs,
                                              unsigned* act) {
  float Ta[VEC], Tm[VEC], k01[VEC], s0[VEC], k10[VEC], s1[VEC], iu[VEC], q[VEC], pm[VEC], tg[VEC], db[VEC];
  int sso[VEC], lk[VEC];
  unsigned fl[VEC];
  load_vec<VEC>(a.Ta, i, Ta);
  load_vec<VEC>(a.Tm, i, Tm);
  load_vec<VEC>(a.sso, i, sso);
  load_bytes<VEC>(a.flags, i, fl);
  if (ext) load_bytes<VEC>(a.actions, i, act);
  load_thermal<VEC>(a, packed, i, k01, s0, k10, s1, iu);
  load_hvac<VEC>(a, coded, i, q, pm);
  load_param_or_first<VEC>((uni & UNIFORM_TARGET) != 0u, a.target, i, tg);
  load_param_or_first<VEC>((uni & UNIFORM_DEADBAND) != 0u, a.deadband, i, db);
  load_vec_or_first<VEC>((uni & UNIFORM_LOCKOUT) != 0u, a.lockout, i, lk);
#pragma unroll
  for (int v = 0; v < VEC; ++v) hs[v] = HouseIn{Ta[v], Tm[v], sso[v], fl[v], k01[v], s0[v], k10[v], s1[v], iu[v], q[v], pm[v], tg[v], db[v], lk[v]};
}

template <int VEC>
__device__ __forceinline__ void resident_store(const StepArgs& a, int64_t i, const HouseIn* hs, const uint64_t* on_m, const uint64_t* lock_m) {
  float nTa[VEC], nTm[VEC];
  int nsso[VEC];
  unsigned nfl[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    nTa[v] = hs[v].Ta;
    nTm[v] = hs[v].Tm;
    nsso[v] = hs[v].sso;
    nfl[v] = house_flags(lane_bit(on_m[v]), lane_bit(lock_m[v]));
  }
  store_vec<VEC>(a.Ta, i, nTa);
  store_vec<VEC>(a.Tm, i, nTm);
  store_vec<VEC>(a.sso, i, nsso);
  store_bytes<VEC>(a.flags, i, nfl);
}

// One step of a lane's VEC houses, every lane, also those past the env's end (k_rollout_fused): blank houses, no divergent branch
// around the ballots.
template <int VEC, bool BB, bool LEAN>
__device__ __forceinline__ void resident_advance(const StepArgs& a, bool ext, HouseIn* hs, uint64_t* on_m, uint64_t* can_m, uint64_t* cmd_m,
                                                 float od_old, float solar) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (BB) cmd_m[v] = __builtin_amdgcn_ballot_w64(hs[v].Ta > hs[v].target);   // agents/bangbang_controllers.py:49-59
    else if (!ext) cmd_m[v] = controller_cmd_m(a.action_source, hs[v].Ta, hs[v].target, hs[v].deadband, on_m[v]);
    const HouseLeanM n = house_advance_lean_m<LEAN>(hs[v], on_m[v], cmd_m[v], od_old, solar, a.dt);
    hs[v].Ta = n.Ta;
    hs[v].Tm = n.Tm;
    hs[v].sso = n.sso;
    on_m[v] = n.on;
    can_m[v] = n.can;
  }
}

// The steps behind the first in two halves, for the loops: the front is the HVAC's state machine of every house of the lane - it
// reads no row - and the back the thermal map with the step's {od_old, solar}.  Front then back is resident_advance<.., true>, or,
// under a uniform lockout, the same step in the time-stamp form (house_advance_stamp_m; hs[v].sso holds the stamp z), expression
// for expression.
template <int VEC, bool BB>
__device__ __forceinline__ void resident_front(const StepArgs& a, bool ext, HouseIn* hs, uint64_t* on_m, uint64_t* can_m, uint64_t* cmd_m) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (BB) cmd_m[v] = __builtin_amdgcn_ballot_w64(hs[v].Ta > hs[v].target);   // agents/bangbang_controllers.py:49-59
    else if (!ext) cmd_m[v] = controller_cmd_m(a.action_source, hs[v].Ta, hs[v].target, hs[v].deadband, on_m[v]);
    const HouseFrontM f = house_lean_front<true>(hs[v], on_m[v], cmd_m[v], a.dt);
    hs[v].sso = f.sso;
    on_m[v] = f.on;
    can_m[v] = f.can;
  }
}

template <int VEC, bool BB>
__device__ __forceinline__ void resident_front_stamp(const StepArgs& a, bool ext, HouseIn* hs, uint64_t* on_m, uint64_t* can_m, uint64_t* cmd_m,
                                                     int Tn, int Ts_minus_L) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (BB) cmd_m[v] = __builtin_amdgcn_ballot_w64(hs[v].Ta > hs[v].target);   // agents/bangbang_controllers.py:49-59
    else if (!ext) cmd_m[v] = controller_cmd_m(a.action_source, hs[v].Ta, hs[v].target, hs[v].deadband, on_m[v]);
    const HouseFrontM f = house_stamp_front(hs[v].sso, on_m[v], cmd_m[v], Tn, Ts_minus_L);
    hs[v].sso = f.sso;
    on_m[v] = f.on;
    can_m[v] = f.can;
  }
}

template <int VEC>
__device__ __forceinline__ void resident_back(HouseIn* hs, const uint64_t* on_m, float od_old, float solar) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const HouseTemps t = house_thermal_back(hs[v], on_m[v], od_old, solar);
    hs[v].Ta = t.Ta;
    hs[v].Tm = t.Tm;
  }
}

// The row a loop loaded one trip ago, wanted now: the values pass through an empty statement the compiler cannot see through, so
// the wait for the load stands here - behind the trip's front - and nowhere earlier.  Without it the compiler folds "load the next
// row, use the one loaded before" into one load of this trip's row at the top of the trip and waits for it half a trip later.  The
// "memory" clobber keeps the next load behind the statement - a load in front of the wait would be waited for as well - and the
// row's byte offset passes through it too: the next address is that offset plus a constant, one 32-bit add, whatever the loop
// optimiser would rather have.  SCALAR: the wave-uniform scalar load of the fused form (lgkmcnt); otherwise the per-lane vector
// load of the group form (vmcnt; these return in order).
template <bool SCALAR>
__device__ __forceinline__ float2 row_arrived(float2 r, uint32_t& off) {
  __builtin_amdgcn_sched_barrier(0);   // the trip's front stays in front of the wait
  if constexpr (SCALAR) asm volatile("" : "+s"(r.x), "+s"(r.y), "+s"(off) : : "memory");
  else asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(off) : : "memory");
  return r;
}

__device__ __forceinline__ float2 row_at(const float2* rows, uint32_t off) {
  return *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(rows) + off);
}

// ... and the load of the row one step ahead, issued right there: the scheduler may move nothing across its end, so the load is
// neither sunk into the arithmetic behind it nor is any of that hoisted in front of the wait.
__device__ __forceinline__ float2 row_ahead(const float2* rows, uint32_t& off, uint32_t step) {
  off += step;
  const float2 r = row_at(rows, off);
  __builtin_amdgcn_sched_barrier(0);
  return r;
}

// Where k_rollout_resident holds the stamp copy of its body at all: one tile per lane with the bang-bang rule compiled in.  A lane
// mask is a scalar register pair and a house has three, so with more tiles, or with the controller's own scalars, the masks fill
// the scalar register file already and a second copy of the body spills more of them into vector lanes (several tiles) or costs a
// wave per SIMD (controllers with several tiles): those keep the counter form alone, as it was.  Every group instantiation holds
// both bodies (profiles/r13_resource_usage.txt).
constexpr bool resident_stamps(int tiles, bool bb) { return bb && tiles == 1; }

// Which loops wait for a row behind their front (row_arrived) and load the next one there: those with the bang-bang rule compiled
// in.  A controller's command hangs on a per-house branch around the caller's actions, which cuts a trip into a dozen basic
// blocks; rotated, those loops need 8 more vector registers per tile and lose a wave per SIMD (profiles/r14_resource_usage.txt),
// so they keep the loop they had: the row is loaded at the top of the trip that uses it.
constexpr bool resident_row_ahead(bool bb) { return bb; }

// STAMP: the loop in the time-stamp form; the caller passes it where `uni` has UNIFORM_LOCKOUT.
template <int VEC, int TILES, int THREADS, bool BB, bool STAMP>
__device__ __forceinline__ void rollout_resident_body(const StepArgs& a, const RolloutArgs& ro, const float2* __restrict__ rows, const RowStrides& rs,
                                                      uint32_t uni) {
  const int e = blockIdx.x;
  const int64_t base = (int64_t)e * a.N;
  const bool coded = hvac_coded(a) != 0u, packed = thermal_packed(a) != 0u;
  const bool ext = !BB && a.action_source == MDR_ACTIONS_EXTERNAL;
  HouseIn hs[TILES][VEC];
  uint64_t on_m[TILES][VEC], can_m[TILES][VEC], cmd_m[TILES][VEC];   // the HVAC's on bit, the last step's `can` and the latest command as lane masks
  bool live[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int h = (t * THREADS + (int)threadIdx.x) * VEC;
    live[t] = h < a.N;
    unsigned act[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      hs[t][v] = HouseIn{};
      act[v] = 0u;
    }
    if (live[t]) resident_load<VEC>(a, uni, coded, packed, ext, base + h, hs[t], act);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {   // (outside the branch: a ballot is a wave-wide value)
      on_m[t][v] = __builtin_amdgcn_ballot_w64(live[t] && (hs[t][v].flags & 1u) != 0u);
      cmd_m[t][v] = __builtin_amdgcn_ballot_w64(live[t] && act[v] != 0u);
    }
  }
  // {od, solar} of step 0; every step's row lies rs.step entries behind the one before.  Byte offsets in 32 bits: the launcher
  // checks that the rows end below 4 GiB
  const uint32_t row_step = rs.step * (uint32_t)sizeof(float2);
  uint32_t row = (uint32_t)e * rs.env * (uint32_t)sizeof(float2);
  float2 nxt;   // the row of the step after the one at work: loaded a step ahead, waited for where that step first reads it
  {   // step 0 in the general form: the state as it was handed in
    const float2 cur = row_at(rows, row);
    row += row_step;
    nxt = row_at(rows, row);
    if (resident_row_ahead(BB)) nxt = row_arrived<true>(nxt, row);   // (not a plain load: the compiler would merge it with the loops' into one load at the top of a trip)
#pragma unroll
    for (int t = 0; t < TILES; ++t) resident_advance<VEC, BB, false>(a, ext, hs[t], on_m[t], can_m[t], cmd_m[t], cur.x, cur.y);
  }
  uint64_t lock_m[TILES][VEC];
  if (STAMP) {   // one lockout for every house: time stamps, on => sso == 0 from here on
    const int L = __builtin_amdgcn_readfirstlane(a.lockout[0]);   // a scalar, also where the loader's copy of it sits in a vector register
    const int Tend = ro.nsteps * a.dt;   // (< 2^31: mdr_api.hip's bound on the steps of a launch)
    int Ts = a.dt;                       // step 1 starts here
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) hs[t][v].sso = house_stamp(lane_bit(on_m[t][v]), hs[t][v].sso, Ts, a.dt);   // hs[][].sso holds the stamp from here
    }
    const auto trip = [&](float2& cur, float2& ahead) {   // uses `cur`, loaded a trip ago, and loads `ahead` for the next trip
      const int Tn = Ts + a.dt;
#pragma unroll
      for (int t = 0; t < TILES; ++t) resident_front_stamp<VEC, BB>(a, ext, hs[t], on_m[t], can_m[t], cmd_m[t], Tn, Ts - L);
      cur = row_arrived<true>(cur, row);   // this step's row: the only wait for it
      ahead = row_ahead(rows, row, row_step);     // the next step's, in flight until the next trip's front is through (behind the last step: the spare entry)
#pragma unroll
      for (int t = 0; t < TILES; ++t) resident_back<VEC>(hs[t], on_m[t], cur.x, cur.y);
      Ts = Tn;
    };
    // Two trips per turn, the two row registers changing places: a load ahead cannot land in the registers the trip at work still
    // reads, and with one trip per turn the compiler copies the pair at the end of every trip - and waits for the load there.
    float2 odd = nxt;
    for (int pairs = (ro.nsteps - 1) >> 1; pairs > 0; --pairs) {
      trip(nxt, odd);
      trip(odd, nxt);
    }
    if (Ts != Tend) trip(nxt, odd);   // the time is the loops' step counter
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        hs[t][v].sso = house_stamp_sso(hs[t][v].sso, Tend, a.dt);   // back into the counter, in front of the lock mask, which reads it
        lock_m[t][v] = house_lock_m(can_m[t][v], on_m[t][v], hs[t][v].sso, L, a.dt);
      }
    }
  } else {   // a streamed lockout column: the counter
    if (resident_row_ahead(BB)) {
      const auto trip = [&](float2& cur, float2& ahead) {   // on => sso == 0 from here on
#pragma unroll
        for (int t = 0; t < TILES; ++t) resident_front<VEC, BB>(a, ext, hs[t], on_m[t], can_m[t], cmd_m[t]);
        cur = row_arrived<true>(cur, row);
        ahead = row_ahead(rows, row, row_step);
#pragma unroll
        for (int t = 0; t < TILES; ++t) resident_back<VEC>(hs[t], on_m[t], cur.x, cur.y);
      };
      float2 odd = nxt;
      for (int pairs = (ro.nsteps - 1) >> 1; pairs > 0; --pairs) {
        trip(nxt, odd);
        trip(odd, nxt);
      }
      if (((ro.nsteps - 1) & 1) != 0) trip(nxt, odd);
    } else {
      float2 cur = nxt;
      for (int s = 1; s < ro.nsteps; ++s) {   // on => sso == 0 from here on
        row += row_step;
        nxt = row_at(rows, row);
#pragma unroll
        for (int t = 0; t < TILES; ++t) resident_advance<VEC, BB, true>(a, ext, hs[t], on_m[t], can_m[t], cmd_m[t], cur.x, cur.y);
        cur = nxt;
      }
    }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {   // (outside the branch below: a ballot is a wave-wide value)
#pragma unroll
      for (int v = 0; v < VEC; ++v) lock_m[t][v] = house_lock_m(can_m[t][v], on_m[t][v], hs[t][v].sso, hs[t][v].lockout, a.dt);
    }
  }
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    if (!live[t]) continue;
    resident_store<VEC>(a, base + (t * THREADS + (int)threadIdx.x) * VEC, hs[t], on_m[t], lock_m[t]);
  }
}

// The word of uniform columns is device-side, so the two forms of the loop are two copies of the body behind one wave-uniform branch
// (like `coded` / `packed`), each with the registers it needs: without the bit the instruction stream is the counter form's.
template <int VEC, int TILES, int THREADS, bool BB>
__global__ __launch_bounds__(THREADS) void k_rollout_resident(StepArgs a, RolloutArgs ro, const float2* __restrict__ rows, RowStrides rs) {
  if (ro.nsteps <= 0) return;
  const uint32_t uni = uniform_word(a);
  if (resident_stamps(TILES, BB) && (uni & UNIFORM_LOCKOUT) != 0u) rollout_resident_body<VEC, TILES, THREADS, BB, true>(a, ro, rows, rs, uni);
  else rollout_resident_body<VEC, TILES, THREADS, BB, false>(a, ro, rows, rs, uni);
}

template <int GROUP, int VEC, bool BB, bool STAMP>
__device__ __forceinline__ void rollout_resident_group_body(const StepArgs& a, const RolloutArgs& ro, const float2* __restrict__ rows,
                                                            const RowStrides& rs, uint32_t uni) {
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / GROUP;
  const int lane = threadIdx.x % GROUP;
  const bool env_ok = gid < a.E;
  const int e = env_ok ? (int)gid : a.E - 1;
  const bool active = env_ok && lane * VEC < a.N;
  const int64_t i = (int64_t)e * a.N + lane * VEC;
  const bool coded = hvac_coded(a) != 0u, packed = thermal_packed(a) != 0u;
  const bool ext = !BB && a.action_source == MDR_ACTIONS_EXTERNAL;
  HouseIn hs[VEC];
  unsigned act[VEC];
  uint64_t on_m[VEC], can_m[VEC], lock_m[VEC], cmd_m[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    hs[v] = HouseIn{};
    act[v] = 0u;
  }
  if (active) resident_load<VEC>(a, uni, coded, packed, ext, i, hs, act);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {   // idle lanes hold blank houses (k_rollout_group): the masks are formed in wave-uniform control flow
    on_m[v] = __builtin_amdgcn_ballot_w64(active && (hs[v].flags & 1u) != 0u);
    cmd_m[v] = __builtin_amdgcn_ballot_w64(active && act[v] != 0u);
  }
  // several envs per wave: each lane reads its own env's rows (an idle env_ok == false lane: env E - 1's)
  const uint32_t row_step = rs.step * (uint32_t)sizeof(float2);
  uint32_t row = (uint32_t)e * rs.env * (uint32_t)sizeof(float2);
  float2 nxt;   // as in k_rollout_resident, in vector registers: the loads return in order, the wait is a vmcnt
  {   // step 0 in the general form
    const float2 cur = row_at(rows, row);
    row += row_step;
    nxt = row_at(rows, row);
    if (resident_row_ahead(BB)) nxt = row_arrived<false>(nxt, row);
    resident_advance<VEC, BB, false>(a, ext, hs, on_m, can_m, cmd_m, cur.x, cur.y);
  }
  if (STAMP) {   // time stamps, as in k_rollout_resident
    const int L = __builtin_amdgcn_readfirstlane(a.lockout[0]);
    const int Tend = ro.nsteps * a.dt;
    int Ts = a.dt;
#pragma unroll
    for (int v = 0; v < VEC; ++v) hs[v].sso = house_stamp(lane_bit(on_m[v]), hs[v].sso, Ts, a.dt);
    if (resident_row_ahead(BB)) {
      const auto trip = [&](float2& cur, float2& ahead) {
        const int Tn = Ts + a.dt;
        resident_front_stamp<VEC, BB>(a, ext, hs, on_m, can_m, cmd_m, Tn, Ts - L);
        cur = row_arrived<false>(cur, row);
        ahead = row_ahead(rows, row, row_step);
        resident_back<VEC>(hs, on_m, cur.x, cur.y);
        Ts = Tn;
      };
      float2 odd = nxt;
      for (int pairs = (ro.nsteps - 1) >> 1; pairs > 0; --pairs) {
        trip(nxt, odd);
        trip(odd, nxt);
      }
      if (Ts != Tend) trip(nxt, odd);
    } else {
      float2 cur = nxt;
      while (Ts != Tend) {
        row += row_step;
        nxt = row_at(rows, row);
        const int Tn = Ts + a.dt;
        resident_front_stamp<VEC, BB>(a, ext, hs, on_m, can_m, cmd_m, Tn, Ts - L);
        resident_back<VEC>(hs, on_m, cur.x, cur.y);
        cur = nxt;
        Ts = Tn;
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      hs[v].sso = house_stamp_sso(hs[v].sso, Tend, a.dt);
      lock_m[v] = house_lock_m(can_m[v], on_m[v], hs[v].sso, L, a.dt);
    }
  } else {
    if (resident_row_ahead(BB)) {
      const auto trip = [&](float2& cur, float2& ahead) {   // on => sso == 0 from here on
        resident_front<VEC, BB>(a, ext, hs, on_m, can_m, cmd_m);
        cur = row_arrived<false>(cur, row);
        ahead = row_ahead(rows, row, row_step);
        resident_back<VEC>(hs, on_m, cur.x, cur.y);
      };
      float2 odd = nxt;
      for (int pairs = (ro.nsteps - 1) >> 1; pairs > 0; --pairs) {
        trip(nxt, odd);
        trip(odd, nxt);
      }
      if (((ro.nsteps - 1) & 1) != 0) trip(nxt, odd);
    } else {
      float2 cur = nxt;
      for (int s = 1; s < ro.nsteps; ++s) {   // on => sso == 0 from here on
        row += row_step;
        nxt = row_at(rows, row);
        resident_advance<VEC, BB, true>(a, ext, hs, on_m, can_m, cmd_m, cur.x, cur.y);
        cur = nxt;
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) lock_m[v] = house_lock_m(can_m[v], on_m[v], hs[v].sso, hs[v].lockout, a.dt);
  }
  if (active) resident_store<VEC>(a, i, hs, on_m, lock_m);
}

template <int GROUP, int VEC, bool BB>
__global__ __launch_bounds__(256) void k_rollout_resident_group(StepArgs a, RolloutArgs ro, const float2* __restrict__ rows, RowStrides rs) {
  if (ro.nsteps <= 0) return;
  const uint32_t uni = uniform_word(a);
  if ((uni & UNIFORM_LOCKOUT) != 0u) rollout_resident_group_body<GROUP, VEC, BB, true>(a, ro, rows, rs, uni);
  else rollout_resident_group_body<GROUP, VEC, BB, false>(a, ro, rows, rs, uni);
}

// The interior steps of mdr_env_rollout, r.nsteps of them, by the STEP plan: the grid and the lane mapping of the k_step_fused /
// k_step_group instantiation that launch_step would launch r.nsteps times.  Other step forms have no interior form: an error.
bool rollout_resident_supported(const StepPlan& p) { return p.kind == STEP_FUSED || p.kind == STEP_GROUP; }

template <int VEC, int THREADS>
static void launch_resident_tiles(const StepArgs& a, const RolloutArgs& r, const float2* rows, const RowStrides& rs, int tiles, hipStream_t s) {
  const dim3 g((unsigned)a.E), b(THREADS);
  const bool bb = a.action_source == MDR_ACTIONS_BANGBANG;
#define MDR_RESIDENT(T)                                                                     \
  if (bb) hipLaunchKernelGGL((k_rollout_resident<VEC, T, THREADS, true>), g, b, 0, s, a, r, rows, rs); \
  else hipLaunchKernelGGL((k_rollout_resident<VEC, T, THREADS, false>), g, b, 0, s, a, r, rows, rs);   \
  break;
  switch (tiles) {
    case 1: MDR_RESIDENT(1)
    case 2: MDR_RESIDENT(2)
    case 3: MDR_RESIDENT(3)
    default: MDR_RESIDENT(4)
  }
#undef MDR_RESIDENT
}

hipError_t launch_rollout_resident(const StepArgs& a, const RolloutArgs& r, const float2* rows, const StepPlan& p, hipStream_t s) {
  if (!rollout_resident_supported(p) || a.cursor != nullptr || rows == nullptr || a.E < 1) return hipErrorInvalidValue;
  // the loops address the rows by 32-bit byte offsets: the spare row behind the last step ends below 4 GiB
  if (((uint64_t)(r.nsteps > 0 ? r.nsteps : 0) + 1) * (uint64_t)a.E >= ((uint64_t)1 << 29)) return hipErrorInvalidValue;
  // Where the rows lie, as two 32-bit kernel arguments: row r of env e at rows[e * env + r * step].  (Formed from a.E inside the
  // kernel the same strides cost k_rollout_resident<4,1,256,true> a scalar register, and the allocator then copies one row pair
  // right behind its load - a wait of the full latency in every second trip.)
  const RowStrides rs{1u, (uint32_t)a.E};
  if (p.kind == STEP_FUSED) {
    if (p.vec == 4) {
      if (p.threads == 64) launch_resident_tiles<4, 64>(a, r, rows, rs, p.tiles, s);
      else if (p.threads == 128) launch_resident_tiles<4, 128>(a, r, rows, rs, p.tiles, s);
      else launch_resident_tiles<4, 256>(a, r, rows, rs, p.tiles, s);
    } else {
      launch_resident_tiles<1, 256>(a, r, rows, rs, p.tiles, s);
    }
    return hipGetLastError();
  }
  const int64_t lanes = (int64_t)a.E * p.threads;
  const dim3 g((unsigned)((lanes + 255) / 256)), b(256);
  const bool bb = a.action_source == MDR_ACTIONS_BANGBANG;
#define MDR_RESIDENT_GV(G, V)                                                                   \
  if (bb) hipLaunchKernelGGL((k_rollout_resident_group<G, V, true>), g, b, 0, s, a, r, rows, rs);         \
  else hipLaunchKernelGGL((k_rollout_resident_group<G, V, false>), g, b, 0, s, a, r, rows, rs);
#define MDR_RESIDENT_G(G)                          \
  if (p.vec == 4) { MDR_RESIDENT_GV(G, 4) }        \
  else if (p.vec == 2) { MDR_RESIDENT_GV(G, 2) }   \
  else { MDR_RESIDENT_GV(G, 1) }                   \
  break;
  switch (p.threads) {
    case 1: MDR_RESIDENT_G(1)
    case 2: MDR_RESIDENT_G(2)
    case 4: MDR_RESIDENT_G(4)
    case 8: MDR_RESIDENT_G(8)
    case 16: MDR_RESIDENT_G(16)
    case 32: MDR_RESIDENT_G(32)
    default: MDR_RESIDENT_G(64)
  }
#undef MDR_RESIDENT_G
#undef MDR_RESIDENT_GV
  return hipGetLastError();
}

}  // namespace mdr
