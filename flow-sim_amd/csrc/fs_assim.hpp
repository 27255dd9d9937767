// fs_assim.hpp - the analysis step of a stochastic ensemble Kalman filter on the members of a batch (fs_batch_assimilate): the
// observations are gauge signals of the current state, the state vector is (h, Q) at every node, and the update is
//   x_r  +=  sum_j  taper_j o cov(x, y_j)  [ (cov(y, y) + diag(variance))^-1 (value + perturb_r - y_r) ]_j          for every active member r
//   host     from the m x B gathered gauge values: the anomalies S, the innovation covariance C, its Cholesky factor and the
//            coefficients Z = C^-1 D - O(m^2 B) flops in fp64, sequential, every product rounded
//   moments  per (field, node) and chunk of FS_ASSIM_CHUNK members: the sums of d = x_r - c, d d and d S_jr over the active members
//   combine  the chunk partials in chunk order: the prior mean and variance of every node and the cross covariances P
//   update   per active member: x_r += sum_j (taper_ji P_fji) Z_jr in (hk, hg) and (Qk, Qg), depths floored
//
// The first part - what the host can refuse, the layouts of the partials and of the outputs, and the coefficients - is plain C++,
// generic over how a sample is read: tests/test_assim_host.py compiles it with the system compiler under sanitizers and holds it to a
// sequential restatement bit for bit.  The kernels follow under __HIPCC__; they are instantiated in fs_part_assim.hip and have no row in
// the dispatch table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flowsim_abi.h"

namespace fs {

static_assert(FS_ASSIM_MAX_OBS == 16, "the kernels are instantiated on the buckets 1, 2, 4, 8, 16 of the observation count");
static_assert(FS_ASSIM_CHUNK == 256, "part of the contract: the bits of the moments depend on where the partial sums are cut");

inline bool assim_finite(double x) { return x - x == 0.0; }

// the smallest of 1, 2, 4, 8, 16 that holds m observations: the rows m .. bucket - 1 of S and Z are zero
inline int assim_bucket(int m) { return m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : m <= 8 ? 8 : 16; }

// What fs_batch_assimilate is handed, as far as the host can judge it without the state: n_obs of 1 .. FS_ASSIM_MAX_OBS, gauges of
// 0 .. n_gauges - 1, signals FS_GAUGE_*, finite values, finite variances > 0, finite perturbations [n_obs][B] (or none), tapers
// [n_obs][N] in [0, 1] (or none), a finite depth floor >= 0.  Returns the error text, or nothing.
inline std::string check_observations(const char *entry, int32_t n_obs, const int32_t *gauge, const int32_t *signal, const double *value,
                                      const double *variance, const double *perturb, const double *taper, double depth_floor, int32_t n_gauges,
                                      size_t B, size_t N) {
  const std::string e(entry);
  if (n_obs < 1 || n_obs > FS_ASSIM_MAX_OBS) return e + ": n_obs must be 1 .. " + std::to_string(FS_ASSIM_MAX_OBS) + ", not " + std::to_string(n_obs);
  if (!gauge || !signal || !value || !variance) return e + ": null gauge, signal, value or variance";
  for (int32_t j = 0; j < n_obs; ++j) {
    const std::string at = " (observation " + std::to_string(j) + ")";
    if (gauge[j] < 0 || gauge[j] >= n_gauges) return e + ": gauge " + std::to_string(gauge[j]) + " is not one of 0 .. " + std::to_string(n_gauges - 1) + at;
    if (signal[j] < 0 || signal[j] >= FS_GAUGE_NROWS)
      return e + ": signal " + std::to_string(signal[j]) + " is not one of FS_GAUGE_DEPTH .. FS_GAUGE_VELOCITY (0 .. 3)" + at;
    if (!assim_finite(variance[j]) || !(variance[j] > 0.0)) return e + ": variances must be finite and > 0" + at;
    if (!assim_finite(value[j])) return e + ": values must be finite" + at;
  }
  if (perturb)
    for (size_t k = 0; k < (size_t)n_obs * B; ++k)
      if (!assim_finite(perturb[k])) return e + ": perturbations must be finite (observation " + std::to_string(k / B) + ", member " + std::to_string(k % B) + ")";
  if (taper)
    for (size_t k = 0; k < (size_t)n_obs * N; ++k)
      if (!(taper[k] >= 0.0 && taper[k] <= 1.0))                                        // (a NaN is not)
        return e + ": tapers must be finite and in [0, 1] (observation " + std::to_string(k / N) + ", node " + std::to_string(k % N) + ")";
  if (!assim_finite(depth_floor) || depth_floor < 0.0) return e + ": depth_floor must be finite and >= 0";
  return {};
}

// the partial sums [chunks][2][m + 2][N] (field 0: h, 1: Q; rows: s1, s2, p_0 .. p_{m-1}), the prior [4][N] (mean h, var h, mean Q,
// var Q) and the cross covariances [2][m][N], in elements; S and Z travel member-major, [B][bucket], so that a member's column is
// one run of doubles
struct AssimLayout {
  size_t B, N, m;
  size_t chunks() const { return (B + FS_ASSIM_CHUNK - 1) / FS_ASSIM_CHUNK; }
  size_t rows() const { return m + 2; }
  size_t partials() const { return chunks() * 2 * rows() * N; }
  size_t partial(size_t chunk, size_t field, size_t row) const { return ((chunk * 2 + field) * rows() + row) * N; }      // node 0 of it
  size_t prior() const { return 4 * N; }
  size_t prior_row(size_t field, size_t moment) const { return (field * 2 + moment) * N; }
  size_t cross() const { return 2 * m * N; }
  size_t cross_row(size_t field, size_t j) const { return (field * m + j) * N; }
  size_t bucket() const { return (size_t)assim_bucket((int)m); }
  size_t columns() const { return B * bucket(); }
  size_t column(size_t r) const { return r * bucket(); }
};

// What the host computes of an analysis, in fp64, sequentially in member order, every product rounded.  active[B]; y(j, r): the
// gathered value of observation j in member r (read for active members only); value[m], variance[m]; perturb [m][B] or nullptr.
//   ybar[m]     sum_r y_jr / n_a
//   S[m][B]     y_jr - ybar_j                                         (0 for inactive members)
//   Cov[m][m]   sum_r S_jr S_lr / (n_a - 1) + [j == l] variance_j
//   L[m][m]     its square-root-free lower Cholesky factor C = L' D L'^T, row by row: the unit lower triangle L' below the diagonal, the
//               pivots D ON the diagonal (the upper triangle is 0).  No square root: one observation is then Z = D / C, one rounding
//   Z[m][B]     C^-1 (value + perturb_r - y_r): the forward substitution with L', the division by the pivots, the backward
//               substitution with L'^T, per member  (0 for inactive members)
// Returns the error text (fewer than two active members, a NaN among the active samples, a pivot that is not positive and finite), or
// nothing; *n_active is set either way.
template <typename Sample>
std::string analysis_coefficients(const char *entry, int m, size_t B, const int32_t *active, Sample &&y, const double *value, const double *variance,
                                  const double *perturb, std::vector<double> &ybar, std::vector<double> &S, std::vector<double> &Cov,
                                  std::vector<double> &L, std::vector<double> &Z, int32_t *n_active) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const std::string e(entry);
  const size_t M = (size_t)m;
  int32_t na = 0;
  for (size_t r = 0; r < B; ++r) na += active[r] != 0;
  *n_active = na;
  if (na < 2) return e + ": " + std::to_string(na) + " active member(s): an analysis needs at least two members that hold every observed gauge";
  ybar.assign(M, 0.0); S.assign(M * B, 0.0); Cov.assign(M * M, 0.0); L.assign(M * M, 0.0); Z.assign(M * B, 0.0);
  for (size_t j = 0; j < M; ++j) {
    double s = 0.0;
    for (size_t r = 0; r < B; ++r) {
      if (!active[r]) continue;
      const double v = y(j, r);
      if (v != v) return e + ": member " + std::to_string(r) + " holds a NaN in observation " + std::to_string(j);
      s += v;
    }
    ybar[j] = s / (double)na;
    for (size_t r = 0; r < B; ++r)
      if (active[r]) S[j * B + r] = y(j, r) - ybar[j];
  }
  for (size_t j = 0; j < M; ++j)
    for (size_t l = 0; l <= j; ++l) {
      double s = 0.0;
      for (size_t r = 0; r < B; ++r) {
        if (!active[r]) continue;
        const double p = S[j * B + r] * S[l * B + r];
        s += p;
      }
      double c = s / (double)(na - 1);
      if (j == l) c += variance[j];
      Cov[j * M + l] = c; Cov[l * M + j] = c;
    }
  for (size_t j = 0; j < M; ++j)
    for (size_t l = 0; l <= j; ++l) {
      double s = Cov[j * M + l];
      for (size_t k = 0; k < l; ++k) {
        const double t = L[j * M + k] * L[k * M + k];
        const double p = t * L[l * M + k];
        s -= p;
      }
      if (j == l) {
        if (!(s > 0.0) || !assim_finite(s))
          return e + ": the innovation covariance is not positive definite (pivot " + std::to_string(j) + " of its Cholesky factor)";
        L[j * M + j] = s;
      } else {
        L[j * M + l] = s / L[l * M + l];
      }
    }
  double w[FS_ASSIM_MAX_OBS], z[FS_ASSIM_MAX_OBS];
  for (size_t r = 0; r < B; ++r) {
    if (!active[r]) continue;
    for (size_t j = 0; j < M; ++j) {
      const double target = perturb ? value[j] + perturb[j * B + r] : value[j];
      double s = target - y(j, r);
      for (size_t k = 0; k < j; ++k) {
        const double p = L[j * M + k] * w[k];
        s -= p;
      }
      w[j] = s;
    }
    for (size_t j = M; j-- > 0;) {
      double s = w[j] / L[j * M + j];
      for (size_t k = j + 1; k < M; ++k) {
        const double p = L[k * M + j] * z[k];
        s -= p;
      }
      z[j] = s;
    }
    for (size_t j = 0; j < M; ++j) Z[j * B + r] = z[j];
  }
  return {};
}

}  // namespace fs

#if defined(__HIPCC__)

#include <hip/hip_runtime.h>

namespace fs {

template <typename R> struct AssimArgs {
  int32_t B, N, m, n_active, first_active;
  R *hk, *Qk, *hg, *Qg;           // [B][N]
  const int32_t *active;          // [B]
  const double *S, *Z;            // [B][bucket]: member-major columns, rows m .. bucket - 1 zero
  const double *taper;            // [m][N] or nullptr (ones)
  double depth_floor;
  double *partials;               // [chunks][2][m + 2][N]
  double *prior;                  // [4][N]
  double *cross;                  // [2][m][N]
  int32_t *clamped;               // [B], zeroed before the launch
};

constexpr int kAssimThreads = 256;      // nodes per workgroup: adjacent lanes take adjacent nodes of a member's row

// a value every lane reads from the same address, never written while the kernel runs (an S or Z column, an active flag): read through
// the constant address space, so that the load is a scalar one and the value is the same register for the whole wave
template <typename T> __device__ __forceinline__ T assim_uniform(const T *p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) T *>(reinterpret_cast<uintptr_t>(p));
}

// One thread per node; blockIdx.y: the chunk of FS_ASSIM_CHUNK members, blockIdx.z: the field.  Every member row is one coalesced load
// in the batch dtype; the member's flag and its S column are wave-uniform.  The 2 + kM accumulators are named by fully unrolled
// loops over a compile-time bound, so they are registers.  The sums run over the active members in member order, every product
// rounded: a lane's partials depend on (field, node, chunk) alone.
template <typename R, int kM> __global__ __launch_bounds__(kAssimThreads) void assim_moments_kernel(const AssimArgs<R> a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kAssimThreads + threadIdx.x;
  if (i >= a.N) return;
  const size_t N = a.N;
  const int chunk = blockIdx.y, f = blockIdx.z;
  const R *x = (f == 0 ? a.hk : a.Qk) + i;
  const double c = (double)x[(size_t)a.first_active * N];
  double s1 = 0.0, s2 = 0.0, p[kM];
#pragma unroll
  for (int j = 0; j < kM; ++j) p[j] = 0.0;
  const int r0 = chunk * FS_ASSIM_CHUNK, r1 = min(a.B, r0 + FS_ASSIM_CHUNK);
#pragma unroll 4
  for (int r = r0; r < r1; ++r) {
    const R xr = x[(size_t)r * N];                       // (a row of the batch: readable whether the member is active or not)
    if (!assim_uniform(a.active + r)) continue;
    const double d = (double)xr - c;
    const double dd = d * d;
    s1 += d; s2 += dd;
#pragma unroll
    for (int j = 0; j < kM; ++j) {
      const double t = d * assim_uniform(a.S + (size_t)r * kM + j);
      p[j] += t;
    }
  }
  double *out = a.partials + ((size_t)(chunk * 2 + f) * (a.m + 2)) * N + i;
  out[0] = s1; out[N] = s2;
#pragma unroll
  for (int j = 0; j < kM; ++j)
    if (j < a.m) out[(size_t)(2 + j) * N] = p[j];
}

// One thread per (field, node): the partials of every row in chunk order, then mean = c + s1 / n_a, var = (s2 - s1 s1 / n_a) /
// (n_a - 1) and P_j = p_j / (n_a - 1)
template <typename R> __global__ __launch_bounds__(kAssimThreads) void assim_combine_kernel(const AssimArgs<R> a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kAssimThreads + threadIdx.x;
  if (i >= a.N) return;
  const size_t N = a.N, rows = (size_t)a.m + 2;
  const int f = blockIdx.y, chunks = (a.B + FS_ASSIM_CHUNK - 1) / FS_ASSIM_CHUNK;
  const double c = (double)(f == 0 ? a.hk : a.Qk)[(size_t)a.first_active * N + i];
  const double na = (double)a.n_active, na1 = (double)(a.n_active - 1);
  double s1 = 0.0, s2 = 0.0;
  for (size_t row = 0; row < rows; ++row) {
    const double *part = a.partials + ((size_t)f * rows + row) * N + i;
    double s = part[0];
    for (int k = 1; k < chunks; ++k) s += part[(size_t)k * 2 * rows * N];
    if (row == 0) s1 = s;
    else if (row == 1) s2 = s;
    else a.cross[((size_t)f * a.m + (row - 2)) * N + i] = s / na1;
  }
  const double q = s1 / na, sq = s1 * s1, t = sq / na;
  a.prior[((size_t)f * 2) * N + i] = c + q;
  a.prior[((size_t)f * 2 + 1) * N + i] = (s2 - t) / na1;
}

// One thread per node; blockIdx.y: a chunk of FS_ASSIM_CHUNK members, blockIdx.z: the field.  The kM weights taper_ji P_fji of the
// node stay in registers; per active member the Z column is wave-uniform and the increment sum_j w_j Z_jr runs in j order from 0.0,
// every product rounded.  The state and the Newton start vector take the same increment, each rounded to the batch dtype on its
// own.  A new depth below the floor (or NaN) becomes the floor in hk and, at that node, in hg; the nodes of hk where that happened
// are counted per member - one integer atomic per wave, so the count does not depend on the order.  Inactive members are not touched.
template <typename R, int kM> __global__ __launch_bounds__(kAssimThreads) void assim_update_kernel(const AssimArgs<R> a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kAssimThreads + threadIdx.x;
  const bool in = i < a.N;
  const size_t N = a.N, at = in ? (size_t)i : 0;
  const int f = blockIdx.z;
  double w[kM];
#pragma unroll
  for (int j = 0; j < kM; ++j) {
    w[j] = 0.0;
    if (j < a.m) {
      const double P = a.cross[((size_t)f * a.m + j) * N + at];
      w[j] = a.taper ? a.taper[(size_t)j * N + at] * P : P;
    }
  }
  R *xk = (f == 0 ? a.hk : a.Qk) + at, *xg = (f == 0 ? a.hg : a.Qg) + at;
  const double floor = a.depth_floor;
  const int r0 = blockIdx.y * FS_ASSIM_CHUNK, r1 = min(a.B, r0 + FS_ASSIM_CHUNK);
  for (int r = r0; r < r1; ++r) {
    if (!assim_uniform(a.active + r)) continue;
    double inc = 0.0;
#pragma unroll
    for (int j = 0; j < kM; ++j) {
      const double t = w[j] * assim_uniform(a.Z + (size_t)r * kM + j);
      inc += t;
    }
    bool low = false;
    if (in) {
      double vk = (double)xk[(size_t)r * N] + inc, vg = (double)xg[(size_t)r * N] + inc;
      if (f == 0) {
        low = !(vk >= floor);
        if (low) vk = floor;
        if (low || !(vg >= floor)) vg = floor;
      }
      xk[(size_t)r * N] = (R)vk; xg[(size_t)r * N] = (R)vg;
    }
    if (f == 0) {
      const unsigned long long mask = __ballot(low);
      if (mask && (threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(a.clamped + r, (int32_t)__popcll(mask));
    }
  }
}

// the launcher (fs_part_assim.hip): moments, combine, update on one stream; false: this build has no such kernels
bool launch_assimilate(const AssimArgs<double> &a, hipStream_t st);
bool launch_assimilate(const AssimArgs<float> &a, hipStream_t st);

}  // namespace fs
#endif
