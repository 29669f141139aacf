// The rollout rows of mdr_env_rollout's resident launches: what the interior steps of one launch read from the time tables, for as
// many steps as the launch runs, in the layout its loop wants.
//
// An interior step r of a launch that starts at time index k reads two floats per env: tab_od at time index k + r and tab_solar at
// k + r + 1.  The tables hold table_steps + 1 time indices, so a launch that reads them ends where they end, and every window costs a
// pass over the houses' state and parameters that the result does not need.  k_fill_rollout_rows builds the two values for any
// (k, nrows) as [nrows][E] float2 {od(k + r), solar(k + r + 1)}: the launch is then bounded by the capacity of that buffer alone.
//
// A translation unit of its own: the instruction streams of every other kernel stay what they were.
//
// The values are produced by the very expressions of k_fill_tables (mdr_kernels.hip) for tab_od and tab_solar from the very inputs -
// od_ext rows while j < od_ext_rows and the sinusoid behind them, the TAG_OD_NOISE Gaussian when temp_std != 0, solar_on, the final
// (float)(od - temp_ref) - and no signal, no abs_noise, no Perlin: bit-identical to the table entries (tests/test_gpu_rollout_rows.py).
// One thread per (env, minute) as in k_fill_tables_tile: what depends on the minute only - the calendar, the outdoor sinusoid, the
// solar polynomial - is evaluated once there, and the thread then walks the time indices that fall into its minute (60 / dt of them:
// one Philox + Gaussian each).  At dt >= 60 s every time index has a minute of its own: one thread per (env, time index).
// Thread id = slot * E + env: a wave holds consecutive envs, whose time indices of one slot are the same or neighbouring rows.
// The grid covers slots * E threads - 1088 workgroups for 4096 envs and 999 steps of 4 s - since the fill is on the rollout's
// critical path, in front of the launch that reads it.
#include <cstdint>

#include "mdr_device.h"
#include "mdr_kernels.h"

namespace mdr {

// a.j0 = k, a.rows = nrows; time index offsets q = 0 .. nrows are walked: od for q < nrows (row q), solar for q >= 1 (row q - 1)
__global__ __launch_bounds__(256) void k_fill_rollout_rows(TableArgs a, float2* __restrict__ dst, int slots, int by_minute) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)slots * a.E) return;
  const int slot = (int)(id / a.E);
  const int e = (int)(id % a.E);
  const uint32_t eg = (uint32_t)(e + a.env_offset);
  const int64_t t_first = a.t0[e] + a.j0 * (int64_t)a.dt;
  int64_t q0, q1, t_cal;
  if (by_minute) {   // dt < 60: the time indices whose time lies in minute `slot` of the launch
    int64_t m_first = t_first / 60;
    if (t_first - m_first * 60 < 0) m_first -= 1;
    const int64_t lo = (int64_t)slot * 60 - (t_first - m_first * 60), hi = lo + 60;   // seconds from t_first, [lo, hi)
    q0 = lo <= 0 ? 0 : (lo + a.dt - 1) / a.dt;
    q1 = min((int64_t)a.rows + 1, (hi + a.dt - 1) / a.dt);
    t_cal = (m_first + slot) * 60;
  } else {
    q0 = slot;
    q1 = slot + 1;
    t_cal = t_first + (int64_t)slot * a.dt;
  }
  if (q0 >= q1) return;
  const Civil c = civil_from_epoch(t_cal);
  float* out = reinterpret_cast<float*>(dst);

  // utils.house_solar_gain (utils.py:1277-1350); identical for every house of the env
  // Row r holds the solar value of time index r + 1: for every index of this minute but the first that is the row the loop below
  // writes one index earlier - one 8-byte store; the first index's value goes to the row in front of this minute's rows, whose od
  // another thread writes.
  const float solar = a.solar_on ? (float)(a.area_shading * solar_cooling_load(c.hour, c.minute, c.month, c.day)) : 0.0f;
  if (q0 >= 1) out[2 * ((q0 - 1) * a.E + e) + 1] = solar;

  // ClusterHouses.compute_OD_temp (env 1057-1081): minute resolution, coldest at 06:00 + phase
  const double amp = 0.5 * (a.day_temp - a.night_temp), bias = 0.5 * (a.day_temp + a.night_temp);
  const double tday = (double)c.hour + (double)c.minute / 60.0;
  const double od_base = amp * sin(6.283185307179586476925286766559 * (tday + (-6.0 + a.phase[e])) / 24.0) + bias;
  const int64_t q_end = min(q1, (int64_t)a.rows);
  for (int64_t q = q0; q < q_end; ++q) {
    const int64_t j = a.j0 + q;
    double od;
    if (a.od_ext != nullptr && j < a.od_ext_rows) {
      od = a.od_ext[j * a.E + e];
    } else {
      od = od_base;
      if (a.temp_std != 0.0) {   // random.gauss(0, 0) adds exactly 0 in the reference; skipping the draw changes nothing
        const u32x4 g = philox4x32_10(eg, (uint32_t)j, a.episode, TAG_OD_NOISE, a.k0, a.k1);
        od += a.temp_std * gauss01(g.x, g.y);
      }
    }
    const float od_f = (float)(od - a.temp_ref);
    if (q + 1 < q1) dst[q * a.E + e] = make_float2(od_f, solar);   // index q + 1 lies in this minute too
    else out[2 * (q * a.E + e)] = od_f;
  }
}

// dst[nrows][E] <- {od(a.j0 + r), solar(a.j0 + r + 1)}; of `a` the signal fields and the table pointers are not read
hipError_t launch_rollout_rows(const TableArgs& a, float2* dst, hipStream_t s) {
  if (dst == nullptr || a.rows < 1 || a.rows > (1 << 20) || a.E < 1 || a.dt < 1) return hipErrorInvalidValue;
  const int by_minute = a.dt < 60 ? 1 : 0;
  const int64_t slots = by_minute ? (59 + (int64_t)a.rows * a.dt) / 60 + 1 : (int64_t)a.rows + 1;
  const int64_t threads = slots * a.E;
  hipLaunchKernelGGL(k_fill_rollout_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, dst, (int)slots, by_minute);
  return hipGetLastError();
}

}  // namespace mdr
