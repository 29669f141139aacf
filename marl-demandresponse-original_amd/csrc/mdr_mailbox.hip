// One externally driven step of a house shard with the per-step exchange through the MAILBOX (mdr_env_step_mailbox), and the
// neighbour-message halo through the same mailbox (mdr_mailbox_halo_push / _pull).  MI355X (gfx950, wave64).
//
// k_step_mailbox is a one-step instance of k_rollout_persist (mdr_persist.hip) whose commands come from the caller's action
// plane (or an in-kernel controller), in ONE launch instead of step_begin_records - all-gather - step_end_records:
//   house workgroup b of env e   steps its 1024 houses (256 when nb_houses % 4 != 0) - the grouping of mdr_persist_records and of
//                                the records path - keeps the new state in REGISTERS, reduces the very (power sum, penalty sum,
//                                penalty max) record k_step_partial writes and pushes it into the mailbox of every rank;
//   reducer workgroup of env e   (blockIdx.x == nblk) waits for the world * records records of the step, re-sums them in the
//                                fixed order of k_step_finish (thread t: ranks in order, records t, t + 256, ...; then the
//                                workgroup tree) - bit-identical totals on every rank and to the records path - and publishes
//                                the totals into this rank's mailbox;
//   house workgroups             pick the totals up and only then write state, rewards, observation planes and P.  A wait that
//                                gives up leaves before any write: the houses keep their state from before the step.
//
// Tags.  One tag per step, from the handle's counter that the persistent rollout also advances (mdr_env::mailbox_tag): the two
// paths share one tag space and one set of slots.  Slot safety: a rank's launches are stream-ordered and a rank's step t + 1
// needs the records of step t + 1 of EVERY rank, which a rank pushes only after its own step t has ended.  So while this rank
// reads slot (t mod SLOTS) a peer is at most one step ahead (pushing tag t + 1 into slot t + 1); within a persistent rollout the
// argument of mdr_persist.hip holds (at most 2 * depth + 2 <= SLOTS tags in flight).  A granule matches only its own full 32-bit
// tag, so what a slot held SLOTS steps ago is never mistaken for the current step.
//
// Waits are bounded in TIME (the device's constant-rate clock, wall_clock64): a peer process may lag by milliseconds while its host
// runs the actor.  On expiry the waiter writes {tag, kind << 28 | workgroup} into word 0 of every rank's mailbox (kinds 3 / 4 /
// 5: mdr_mailbox.h); every waiter polls word 0 as well, and a launch that finds it set at its start leaves without writing.
//
// Reference: env/MA_DemandResponse.py:1005-1055 (ClusterHouses.step; power sum 1042-1050), 274-321 (common penalties), 976-1001
// (messages); train_ppo.py:62-77 (observe -> act -> step).
#include <algorithm>
#include <cstdlib>

#include "mdr_device.h"
#include "mdr_kernels.h"
#include "mdr_mailbox.h"
#include "mdr_step_common.h"

namespace mdr {

constexpr int HALO_SLOTS = 2;   // halo exchanges in flight: a peer is at most one exchange ahead (see mailbox_halo_*)

// wave 0's lanes r < world: rank r's error word
template <bool SYS>
__device__ __forceinline__ gu64* abort_lane_ptr(const PersistArgs& m) {
  const int lane = threadIdx.x & 63;
  gu64* p = nullptr;
#pragma unroll
  for (int r = 0; r < MDR_MAX_SHARDS; ++r)
    if (r < m.world && lane == r && threadIdx.x < 64) p = (gu64*)m.box[r];
  return p;
}

// s_flag: 0 = go on, 1 = the error word was found set (another waiter gave up), 2 = this workgroup's wait gave up
template <int VEC, bool SYS>
__global__ __launch_bounds__(256) void k_step_mailbox(StepArgs a, PersistArgs m, uint64_t timeout_ticks) {
  __shared__ double lds_red[3 * 4];
  __shared__ double lds_tot[3];
  __shared__ int s_flag;
  const int e = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int nblk = m.nrec[m.rank];
  const bool need_pen = a.penalty_mode != MDR_PENALTY_INDIVIDUAL_L2;
  const int ng = need_pen ? PERSIST_G : 2;   // granules that travel: the power sum alone unless a common penalty mode needs the rest
  const uint32_t tag = m.tag_base;
  const int slot = (int)(tag % PERSIST_SLOTS);
  gu64* const own = (gu64*)m.box[m.rank];
  gu64* const abort_ptr = abort_lane_ptr<SYS>(m);

  if (blk >= nblk) {
    // ---------------------------------------------------------------- reducer of env e: the records of every rank, finish order
    if (tid == 0) s_flag = abort_raised<SYS>(own) ? 1 : 0;
    __syncthreads();
    if (s_flag) return;
    Red3 acc{0.0, 0.0, 0.0f};
    int fail = 0;
    const uint64_t t0 = (uint64_t)wall_clock64();
    uint32_t spins = 0;
    for (int r = 0; r < m.world && !fail; ++r) {
      const int nr = m.nrec[r];
      for (int b = tid; b < nr; b += 256) {
        const gu64* rec = own + rec_offset(m, a.E, slot, e, r, b);
        unsigned long long y[PERSIST_G];
        for (;;) {
          bool ok = true;
#pragma unroll
          for (int g = 0; g < PERSIST_G; ++g) {
            y[g] = (g < ng) ? granule_load<SYS>(rec + g) : ((unsigned long long)tag << 32);
            ok &= (uint32_t)(y[g] >> 32) == tag;
          }
          if (ok) break;
          if ((++spins & 15u) == 0u) {
            if (abort_raised<SYS>(own)) fail = 1;
            else if ((uint64_t)wall_clock64() - t0 > timeout_ticks) fail = 2;
            if (fail) break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        if (fail) break;
        acc.sum_p += __hiloint2double((int)(uint32_t)y[1], (int)(uint32_t)y[0]);
        acc.sum_pen += __hiloint2double((int)(uint32_t)y[3], (int)(uint32_t)y[2]);
        acc.max_pen = fmaxf(acc.max_pen, __uint_as_float((uint32_t)y[4]));
      }
    }
    if (fail) atomicMax(&s_flag, fail);
    const Red3 tot = block_reduce<256>(acc, lds_red);   // its barrier publishes s_flag
    if (s_flag) {
      if (s_flag == 2) raise_abort<SYS>(abort_ptr, tag, MAILBOX_FAIL_RECORDS);
      return;
    }
    if (tid < ng) {   // the totals, one granule per lane, into this rank's mailbox
      const uint32_t v = tid == 0 ? (uint32_t)__double2loint(tot.sum_p) : tid == 1 ? (uint32_t)__double2hiint(tot.sum_p)
                       : tid == 2 ? (uint32_t)__double2loint(tot.sum_pen) : tid == 3 ? (uint32_t)__double2hiint(tot.sum_pen)
                                  : __float_as_uint(tot.max_pen);
      granule_store<SYS>(own + tot_offset(m, a.E, slot, e) + tid, tag, v);
    }
    return;
  }

  // ------------------------------------------------------------------ house workgroup
  const int h = (blk * 256 + tid) * VEC;
  const bool live = h < a.N;
  const int64_t i = (int64_t)e * a.N + h;
  // the error word: requested first, consulted once the step is computed (before anything leaves the workgroup)
  const bool aborted0 = tid == 0 && abort_raised<SYS>(own);
  HouseOut o[VEC];
  int lk[VEC];
  unsigned act[VEC];
  Red3 acc{0.0, 0.0, 0.0f};
  if (live) {
    const float od_e = a.od_old[e], so_e = a.solar_new[e];
    float od[VEC], so[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      od[v] = od_e;
      so[v] = so_e;
    }
    house_step_vec<VEC>(a, i, od, so, o, lk, act);
    float p = 0.0f, ps = 0.0f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {   // partial_block's arithmetic (mdr_kernels.hip)
      p += o[v].power;
      ps += o[v].pen;
      acc.max_pen = fmaxf(acc.max_pen, o[v].pen);
    }
    acc.sum_p = (double)p;
    acc.sum_pen = (double)ps;
  }
  if (tid == 0) s_flag = aborted0 ? 1 : 0;
  const Red3 rec = block_reduce<256>(acc, lds_red);   // the record of this workgroup, in every thread; its barrier publishes s_flag
  if (s_flag) return;
  if (tid < m.world * ng) {   // lane (rank r, granule g) writes granule g of the record into rank r's mailbox
    const int r = tid / ng, g = tid - (tid / ng) * ng;
    gu64* dst = nullptr;
#pragma unroll
    for (int q = 0; q < MDR_MAX_SHARDS; ++q)
      if (q == r) dst = (gu64*)m.box[q];
    const uint32_t v = g == 0 ? (uint32_t)__double2loint(rec.sum_p) : g == 1 ? (uint32_t)__double2hiint(rec.sum_p)
                     : g == 2 ? (uint32_t)__double2loint(rec.sum_pen) : g == 3 ? (uint32_t)__double2hiint(rec.sum_pen)
                              : __float_as_uint(rec.max_pen);
    granule_store<SYS>(dst + rec_offset(m, a.E, slot, e, m.rank, blk) + g, tag, v);
  }
  if (tid < 64) {   // wave 0 picks the totals up (lanes past the granules that travel read the last of them)
    const gu64* src = own + tot_offset(m, a.E, slot, e) + min(lane, ng - 1);
    const uint64_t t0 = (uint64_t)wall_clock64();
    unsigned long long x = granule_load<SYS>(src);
    int fail = 0;
    uint32_t spins = 0;
    while (!__all((uint32_t)(x >> 32) == tag)) {
      if ((++spins & 15u) == 0u) {
        if (__builtin_amdgcn_readfirstlane(abort_raised<SYS>(own) ? 1 : 0)) fail = 1;
        else if ((uint64_t)wall_clock64() - t0 > timeout_ticks) fail = 2;
        if (fail) break;
      }
      __builtin_amdgcn_s_sleep(1);
      x = granule_load<SYS>(src);
    }
    if (fail == 2) raise_abort<SYS>(abort_ptr, tag, MAILBOX_FAIL_TOTALS);
    const uint32_t val = (uint32_t)x;
    const int v0 = __builtin_amdgcn_readlane((int)val, 0), v1 = __builtin_amdgcn_readlane((int)val, 1);
    const int v2 = need_pen ? __builtin_amdgcn_readlane((int)val, 2) : 0, v3 = need_pen ? __builtin_amdgcn_readlane((int)val, 3) : 0;
    const int v4 = need_pen ? __builtin_amdgcn_readlane((int)val, 4) : 0;   // (granules that did not travel: zeros)
    if (lane == 0) {
      lds_tot[0] = __hiloint2double(v1, v0);
      lds_tot[1] = __hiloint2double(v3, v2);
      lds_tot[2] = (double)__int_as_float(v4);
      s_flag = fail;
    }
  }
  __syncthreads();
  if (s_flag) return;   // nothing written: the houses keep the state from before the step
  const double P = lds_tot[0], sum_pen = lds_tot[1];
  const float max_pen = (float)lds_tot[2];
  if (blk == 0 && tid == 0) a.P[e] = P;
  if (!live) return;
  float nTa[VEC], nTm[VEC], pen[VEC];
  int nsso[VEC];
  unsigned nfl[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    nTa[v] = o[v].Ta;
    nTm[v] = o[v].Tm;
    nsso[v] = o[v].sso;
    nfl[v] = o[v].flags;
    pen[v] = o[v].pen;
  }
  store_vec<VEC>(a.Ta, i, nTa);
  store_vec<VEC>(a.Tm, i, nTm);
  store_vec<VEC>(a.sso, i, nsso);
  store_bytes<VEC>(a.flags, i, nfl);
  if (a.action_source != MDR_ACTIONS_EXTERNAL && a.actions != nullptr) store_bytes<VEC>(a.actions, i, act);
  store_obs_local<VEC>(a, i, o, lk);
  store_reward_power<VEC>(a, i, pen, sum_pen, max_pen, signal_term(a, P, a.sig_old[e]), (float)(a.sig_new[e] * a.inv_obs_norm),
                          (float)(P * a.inv_obs_norm));
}

template <typename K>
static hipError_t mailbox_capacity(K kernel, int64_t* blocks) {
  int dev = 0, per_cu = 0, cus = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0);
  if (err != hipSuccess) return err;
  err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (err != hipSuccess) return err;
  // the runtime's answer can be one workgroup per CU above what the hardware admits for SGPR-heavy 256-thread kernels
  // (MI355X_MICROARCH.md, residency): count no more than four per CU, as the persistent rollout does
  *blocks = (int64_t)std::min(per_cu, 4) * cus;
  return hipSuccess;
}

hipError_t mailbox_resident_blocks(int vec, bool sys, int64_t* blocks) {
  if (vec == 4) return sys ? mailbox_capacity(k_step_mailbox<4, true>, blocks) : mailbox_capacity(k_step_mailbox<4, false>, blocks);
  return sys ? mailbox_capacity(k_step_mailbox<1, true>, blocks) : mailbox_capacity(k_step_mailbox<1, false>, blocks);
}

uint64_t mailbox_timeout_ticks(uint32_t timeout_us) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
    khz = 100000;   // the MI300 / MI355X constant-rate clock: 100 MHz
  const uint64_t us = timeout_us ? timeout_us : MAILBOX_DEFAULT_TIMEOUT_US;
  return us * (uint64_t)khz / 1000u;
}

hipError_t launch_step_mailbox(const StepArgs& a, const PersistArgs& m, bool sys, uint64_t timeout_ticks, hipStream_t s) {
  const dim3 g((unsigned)(m.nrec[m.rank] + 1), (unsigned)a.E), b(256);
  if (a.N % 4 == 0) {
    if (sys) hipLaunchKernelGGL((k_step_mailbox<4, true>), g, b, 0, s, a, m, timeout_ticks);
    else hipLaunchKernelGGL((k_step_mailbox<4, false>), g, b, 0, s, a, m, timeout_ticks);
  } else {
    if (sys) hipLaunchKernelGGL((k_step_mailbox<1, true>), g, b, 0, s, a, m, timeout_ticks);
    else hipLaunchKernelGGL((k_step_mailbox<1, false>), g, b, 0, s, a, m, timeout_ticks);
  }
  return hipGetLastError();
}

// ---- halo: [HALO_SLOTS][world][count] granules behind the totals of every rank's mailbox (base = its granule offset).
// Push: this rank's `count` floats, one per granule, into its row of every rank's halo slot.  Pull: every granule of the slot,
// bounded in time, unpacked into out[world][count].  A peer is at most one exchange ahead (its exchange t + 1 cannot end before
// this rank has pushed t + 1, which it does after its own pull of t), so two slots suffice; the tag is the caller's count of exchanges.
template <bool SYS>
__global__ __launch_bounds__(256) void k_halo_push(PersistArgs m, int64_t base, const float* __restrict__ src, int64_t count, uint32_t tag) {
  __shared__ int s_abort;
  gu64* const own = (gu64*)m.box[m.rank];
  if (threadIdx.x == 0) s_abort = abort_raised<SYS>(own) ? 1 : 0;
  __syncthreads();
  if (s_abort) return;
  const int64_t off = base + ((int64_t)(tag % HALO_SLOTS) * m.world + m.rank) * count;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (int64_t)gridDim.x * 256) {
    const uint32_t v = __float_as_uint(src[j]);
#pragma unroll
    for (int r = 0; r < MDR_MAX_SHARDS; ++r)
      if (r < m.world) granule_store<SYS>((gu64*)m.box[r] + off + j, tag, v);
  }
}

template <bool SYS>
__global__ __launch_bounds__(256) void k_halo_pull(PersistArgs m, int64_t base, float* __restrict__ out, int64_t count, uint32_t tag,
                                                   uint64_t timeout_ticks) {
  __shared__ int s_flag;
  gu64* const own = (gu64*)m.box[m.rank];
  gu64* const abort_ptr = abort_lane_ptr<SYS>(m);
  if (threadIdx.x == 0) s_flag = abort_raised<SYS>(own) ? 1 : 0;
  __syncthreads();
  if (s_flag) return;
  const gu64* slot = own + base + (int64_t)(tag % HALO_SLOTS) * m.world * count;
  const int64_t total = (int64_t)m.world * count;
  const uint64_t t0 = (uint64_t)wall_clock64();
  int fail = 0;
  uint32_t spins = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total && !fail; j += (int64_t)gridDim.x * 256) {
    unsigned long long x = granule_load<SYS>(slot + j);
    while ((uint32_t)(x >> 32) != tag) {
      if ((++spins & 15u) == 0u) {
        if (abort_raised<SYS>(own)) fail = 1;
        else if ((uint64_t)wall_clock64() - t0 > timeout_ticks) fail = 2;
        if (fail) break;
      }
      __builtin_amdgcn_s_sleep(1);
      x = granule_load<SYS>(slot + j);
    }
    if (!fail) out[j] = __uint_as_float((uint32_t)x);
  }
  if (fail) atomicMax(&s_flag, fail);
  __syncthreads();
  if (s_flag == 2) raise_abort<SYS>(abort_ptr, tag, MAILBOX_FAIL_HALO);
}

constexpr int HALO_MAX_BLOCKS = 64;   // the pull spins: keep it to a corner of the device so that a peer sharing it can push

hipError_t launch_halo_push(const PersistArgs& m, int64_t base, const float* src, int64_t count, uint32_t tag, bool sys, hipStream_t s) {
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(HALO_MAX_BLOCKS, (count + 255) / 256));
  if (sys) hipLaunchKernelGGL(k_halo_push<true>, dim3((unsigned)blocks), dim3(256), 0, s, m, base, src, count, tag);
  else hipLaunchKernelGGL(k_halo_push<false>, dim3((unsigned)blocks), dim3(256), 0, s, m, base, src, count, tag);
  return hipGetLastError();
}

hipError_t launch_halo_pull(const PersistArgs& m, int64_t base, float* out, int64_t count, uint32_t tag, bool sys, uint64_t timeout_ticks,
                            hipStream_t s) {
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(HALO_MAX_BLOCKS, (m.world * count + 255) / 256));
  if (sys) hipLaunchKernelGGL(k_halo_pull<true>, dim3((unsigned)blocks), dim3(256), 0, s, m, base, out, count, tag, timeout_ticks);
  else hipLaunchKernelGGL(k_halo_pull<false>, dim3((unsigned)blocks), dim3(256), 0, s, m, base, out, count, tag, timeout_ticks);
  return hipGetLastError();
}

int64_t mailbox_halo_granules(int world, int64_t count) { return (int64_t)HALO_SLOTS * world * count; }

}  // namespace mdr
