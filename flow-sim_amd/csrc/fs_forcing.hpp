// fs_forcing.hpp - what a hydrograph boundary is forced with, built on the device: the target block [level][B] a batch's step kernels
// read (BCDesc::target), which the host otherwise samples member by member and uploads.
//   sample  target[k][r] = offset_r + scale_r * np.interp(k dt_r - shift_r; times, values[table_r]): Hydrograph.sample
//           (hydrograph.py:26-32) of a table each member scales, lifts and delays
//   route   level-pool routing of that inflow through a reservoir, GerdHydrograph.build (cases/gerd_roseires/gerd_discharge.py:12-56)
//           generalised to data: a volume curve, up to kPoolMaxWeirs weirs with an opening ramp, a base flow; one brentq per level,
//           serial in time, every member its own pool
//
// The first part - the outlet capacity, the release rule and one level of the pool recurrence - is plain C++, generic over how a
// sample is read: tests/test_forcing_host.py compiles it with the system compiler under sanitizers and holds it to the reference's own
// tables and to scipy's evaluation counts.  The kernels follow under __HIPCC__; they are instantiated in fs_part_forcing.hip, compute in
// fp64 whatever the batch's type, and have no row in the dispatch table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/flowsim_abi.h"
#include "fs_init_state.hpp"      // fs::brent_root
#include "fs_reduce.hpp"          // fs::interp_series

#if defined(__HIPCC__)
#define FS_FRC_HD __host__ __device__ __forceinline__
#else
#define FS_FRC_HD inline
#endif

namespace fs {

constexpr int kPoolMaxCurve = 64;       // points of the volume curve
constexpr int kPoolMaxWeirs = 8;

// What the outlets pass at pool level z (effective_capacity, gerd_discharge.py:70-94): the weirs in the caller's order, the base flow
// (the turbines) last, as the reference adds them.  coef(w): C_w times the member's multiplier; crest(w); top(w): where the weir's
// opening ramp (alpha, gerd_discharge.py:96-105) reaches 1 - at or below the crest: no ramp.  head^1.5 is head * sqrt(head): against
// pow it moves the release by an ulp and no stage bit.
template <typename Coef, typename Crest, typename Top>
FS_FRC_HD double pool_capacity(int n_w, Coef &&coef, Crest &&crest, Top &&top, double base_flow, double z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double sum = 0.0;
  for (int w = 0; w < n_w; ++w) {
    const double c = crest(w), t = top(w);
    double head = z - c;
    if (!(head > 0.0)) head = 0.0;
    double q = coef(w) * (head * __builtin_sqrt(head));
    if (t > c) {
      const double ramp = z <= c ? 0.0 : (z >= t ? 1.0 : (z - c) / (t - c));
      q = q * ramp;
    }
    sum += q;
  }
  return sum + base_flow;
}

// The release rule (release, gerd_discharge.py:58-68): above the hold level whatever the outlets pass, at or below it the inflow,
// but no more than they pass and no less than the base flow
FS_FRC_HD double pool_release(double inflow, double capacity, double z, double hold, double base_flow) {
  if (z > hold) return capacity;
  const double q = inflow < capacity ? inflow : capacity;
  return q > base_flow ? q : base_flow;
}

struct PoolLevel {
  double stage, release;      // z1, qout1
  bool bracketed;             // false: brentq's ValueError; stage and release are NaN
  int evals;                  // evaluations of the imbalance, as brentq's full_output counts them
};

// One level of the recurrence (gerd_discharge.py:27-46).  volume(z): the curve; capacity(z): pool_capacity of this member; dt: the
// member's time step; vol_scale: m3 -> the curve's unit.  Both ends of the bracket are evaluated first, as brentq does.
template <typename Volume, typename Capacity>
FS_FRC_HD PoolLevel pool_level(Volume &&volume, Capacity &&capacity, double hold, double base_flow, double z0, double qin0, double qout0,
                               double qin1, double dt, double vol_scale, double z_lo, double z_hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double mean_in = 0.5 * (qin1 + qin0);
  const double v0 = volume(z0);
  auto imbalance = [&](double z1)
#if defined(__HIPCC__)
      __attribute__((always_inline))
#endif
  {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double mean_out = 0.5 * (pool_release(qin1, capacity(z1), z1, hold, base_flow) + qout0);
    return (volume(z1) - v0) - (mean_in - mean_out) * dt * vol_scale;
  };
  PoolLevel out;
  const double f_lo = imbalance(z_lo), f_hi = imbalance(z_hi);
  out.stage = brent_root(imbalance, z_lo, f_lo, z_hi, f_hi, &out.bracketed, &out.evals);
  if (out.bracketed) {
    out.release = pool_release(qin1, capacity(out.stage), out.stage, hold, base_flow);
  } else {
    out.stage = red_nan(); out.release = red_nan();
  }
  return out;
}

// ---- what the host validates before a launch (fs_abi.hip); each check returns the error text or nullptr ----

inline const char *check_sampled_tables(const double *times, const double *values, int n_pts, int n_tables, const int32_t *table_of, std::size_t B) {
  if (!times || !values) return "fs_batch_set_bc_sampled: null table";
  if (n_pts < 1 || n_tables < 1) return "fs_batch_set_bc_sampled: n_pts and n_tables must be >= 1";
  for (int j = 0; j + 1 < n_pts; ++j)
    if (!(times[j + 1] > times[j])) return "fs_batch_set_bc_sampled: times must be increasing";
  if (n_pts == 1 && !(times[0] == times[0])) return "fs_batch_set_bc_sampled: times must be increasing";
  if (table_of)
    for (std::size_t r = 0; r < B; ++r)
      if (table_of[r] < 0 || table_of[r] >= n_tables) return "fs_batch_set_bc_sampled: table_of must be 0 .. n_tables - 1";
  return nullptr;
}

inline const char *check_pool(const double *curve_stage, const double *curve_volume, int n_curve, const double *weirs, int n_w,
                              double base_flow, double vol_scale, double z_lo, double z_hi) {
  if (!curve_stage || !curve_volume) return "fs_batch_route_pool: null volume curve";
  if (n_curve < 2 || n_curve > kPoolMaxCurve) return "fs_batch_route_pool: the volume curve takes 2 .. 64 points";
  for (int j = 0; j + 1 < n_curve; ++j)
    if (!(curve_stage[j + 1] > curve_stage[j])) return "fs_batch_route_pool: curve stages must be increasing";
  for (int j = 0; j < n_curve; ++j)
    if (!(curve_volume[j] == curve_volume[j])) return "fs_batch_route_pool: curve volumes must be numbers";
  if (n_w < 0 || n_w > kPoolMaxWeirs) return "fs_batch_route_pool: at most 8 weirs";
  if (n_w > 0 && !weirs) return "fs_batch_route_pool: null weirs";
  for (int w = 0; w < n_w; ++w) {
    const double *p = weirs + 4 * w;
    if (!(p[0] >= 0) || !(p[1] == p[1]) || !(p[2] == p[2])) return "fs_batch_route_pool: a weir needs C >= 0, a crest and a ramp top";
    if (p[3] != 0.0) return "fs_batch_route_pool: the fourth number of a weir is reserved and must be 0";
  }
  if (!(base_flow >= 0) || !(vol_scale > 0)) return "fs_batch_route_pool: base_flow >= 0 and vol_scale > 0 required";
  if (!(z_lo < z_hi)) return "fs_batch_route_pool: the bracket needs z_lo < z_hi";
  return nullptr;
}

}  // namespace fs

#if defined(__HIPCC__)

namespace fs {

// target[k][r] for every level and member: one thread per (level, member), the member minor - a wave stores 64 consecutive members
// of one row.  The tables (a few hundred bytes) are read through the caches.
template <typename R> struct SampleArgs {
  R *target;                     // [L][B]
  int32_t L, B, n_pts, n_tables;
  const double *times, *values;  // [n_pts], [n_tables][n_pts]
  const int32_t *table_of;       // [B] or nullptr: table 0
  const double *scale, *offset, *shift;      // [B] or nullptr: 1, 0, 0
  const double *reach_dt;        // [B] or nullptr: dt
  double dt;
};

template <typename R> __global__ __launch_bounds__(256) void sample_target_kernel(const SampleArgs<R> a) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.B) return;
  const double dt = a.reach_dt ? a.reach_dt[r] : a.dt;
  const double *v = a.values + (size_t)(a.table_of ? a.table_of[r] : 0) * a.n_pts;
  const double *t = a.times;
  for (int k = blockIdx.y; k < a.L; k += gridDim.y) {         // (one level per workgroup up to the grid's 65 535 rows)
    double x = (double)k * dt;                                 // np.arange(n) * dt
    if (a.shift) x = x - a.shift[r];
    double y = interp_series(a.n_pts, [=](int j) { return t[j]; }, [=](int j) { return v[j]; }, x);
    if (a.scale) y = a.scale[r] * y;
    if (a.offset) y = a.offset[r] + y;
    a.target[(size_t)k * a.B + r] = (R)y;
  }
}

constexpr int kPoolLanes = 64;          // members per workgroup of the routing: one wave, one lane per member, serial over the levels

template <typename R> struct PoolArgs {
  R *target;                     // [L][B]: the inflow on entry, the release on return
  double *stage;                 // [L][B]
  int32_t *info;                 // [2][B]: FS_POOL_* bits (zeroed before the launch), the first level without a bracket (-1)
  int32_t L, B, n_curve, n_w;
  const double *curve_stage, *curve_volume;      // [n_curve]
  const double *weirs;           // [n_w][4]: C, crest, ramp_top, reserved
  const double *weir_scale;      // [n_w][B] or nullptr
  const double *initial_stage;   // [B]
  const double *reach_dt;        // [B] or nullptr: dt
  double dt, base_flow, vol_scale, z_lo, z_hi;
};

// The recurrence is serial in time, the batch supplies the parallelism (as in the backwater march, fs_init_state.hpp).  A lane's loads
// and stores of level k are one row's consecutive members: coalesced as they are.  The curve and the weirs sit in LDS, each lane's own
// scaled coefficients in a column of its own.
template <typename R> __global__ __launch_bounds__(kPoolLanes) void route_pool_kernel(const PoolArgs<R> a) {
  __shared__ double s_z[kPoolMaxCurve], s_v[kPoolMaxCurve];
  __shared__ double s_crest[kPoolMaxWeirs], s_top[kPoolMaxWeirs];
  __shared__ double s_coef[kPoolMaxWeirs][kPoolLanes];
  const int lane = threadIdx.x, B = a.B;
  const bool valid = blockIdx.x * kPoolLanes + lane < B;
  const int r = valid ? blockIdx.x * kPoolLanes + lane : B - 1;
  const int n_curve = a.n_curve, n_w = a.n_w;
  if (lane < n_curve) { s_z[lane] = a.curve_stage[lane]; s_v[lane] = a.curve_volume[lane]; }
  if (lane < n_w) { s_crest[lane] = a.weirs[4 * lane + 1]; s_top[lane] = a.weirs[4 * lane + 2]; }
  for (int w = 0; w < n_w; ++w) {
#pragma clang fp contract(off)
    const double c = a.weirs[4 * w];
    s_coef[w][lane] = a.weir_scale ? c * a.weir_scale[(size_t)w * B + r] : c;
  }
  __syncthreads();
  if (!valid) return;      // (the padding lanes of the last workgroup have filled their share of LDS; no barrier follows)
  auto volume = [&](double z) __attribute__((always_inline)) {
    return interp_series(n_curve, [&](int j) { return s_z[j]; }, [&](int j) { return s_v[j]; }, z);
  };
  auto capacity = [&](double z) __attribute__((always_inline)) {
    return pool_capacity(n_w, [&](int w) { return s_coef[w][lane]; }, [&](int w) { return s_crest[w]; }, [&](int w) { return s_top[w]; },
                         a.base_flow, z);
  };
  const double dt = a.reach_dt ? a.reach_dt[r] : a.dt;
  const double hold = a.initial_stage[r];
  double z0 = hold, qin0 = (double)a.target[r];
  double qout0 = pool_release(qin0, capacity(z0), z0, hold, a.base_flow);
  int flags = 0, where = -1;
  a.target[r] = (R)qout0; a.stage[r] = z0;
#pragma clang loop unroll(disable)
  for (int k = 1; k < a.L; ++k) {
    const size_t at = (size_t)k * B + r;
    const double qin1 = (double)a.target[at];
    if (!flags) {
      const PoolLevel s = pool_level(volume, capacity, hold, a.base_flow, z0, qin0, qout0, qin1, dt, a.vol_scale, a.z_lo, a.z_hi);
      if (!s.bracketed) { flags = FS_POOL_NO_BRACKET; where = k; }
      z0 = s.stage; qin0 = qin1; qout0 = s.release;      // (NaN from the level without a bracket on)
    }
    a.target[at] = (R)qout0; a.stage[at] = z0;
  }
  a.info[r] = flags; a.info[(size_t)B + r] = where;
}

// the launchers (fs_part_forcing.hip); false: this build has no such kernel
bool launch_sample_target(const SampleArgs<double> &a, hipStream_t st);
bool launch_sample_target(const SampleArgs<float> &a, hipStream_t st);
bool launch_route_pool(const PoolArgs<double> &a, hipStream_t st);
bool launch_route_pool(const PoolArgs<float> &a, hipStream_t st);

}  // namespace fs
#endif
