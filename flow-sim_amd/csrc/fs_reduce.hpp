// fs_reduce.hpp - ensemble post-processing on the device: three reductions of the boundary hydrograph block [level][4][B] a batch keeps
// (fs_batch_get_hydrographs), so that a large ensemble hands back what its user reads instead of the block itself:
//   summarize  per reach: the numbers of the reference's result summary (solver.py:188-233) - sums, peaks, median-volume levels
//   lookup     per reach: np.interp of one signal over another at shared abscissae, and its RMSE against a target
//              (cases/gerd_roseires/n_calibrate.py:55-67; the Q= branch of model.run, model.py:105-113)
//   bands      per (level, signal): min, max, mean, std and exact quantiles across the members
//
// The first part - the walks over ONE series - is plain C++, generic over how a sample is read: tests/test_reduce_host.py compiles it
// with the system compiler under sanitizers and holds it to numpy on the reference's own histories.  The kernels follow under
// __HIPCC__; they are instantiated in fs_part_reduce.hip and have no row in the dispatch table.
#pragma once
#include <cstdint>

#include "../../include/flowsim_abi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_RED_HD __host__ __device__ __forceinline__
#else
#define FS_RED_HD inline
#endif

namespace fs {

FS_RED_HD double red_nan() { return __builtin_nan(""); }

// The reference's result summary of one reach (solver.py:203-229) over m levels.  h_in(k), q_in(k), h_out(k), q_out(k): the sample of
// level k = 0 .. m-1 as a double; put(row, value) receives the FS_SUM_* rows.  Sums run in level order (np.sum is pairwise: they agree
// within m eps sum|Q|); a peak's level is the first index of the maximum (np.argmax).  The median-volume level is the reference's, quirk
// included: with cum_i = sum(Q[:i]) the first i with cum_i >= 0.5 cum_{m-1} - the last sample is never counted, cum_0 = 0, and with
// negative flows "first" still decides.  The second walk adds in the order of the first, so that its cum_{m-1} IS the threshold's.
// m = 0 (a reach that completed no row of the range): sums 0, peaks NaN, levels -1.
template <typename HIn, typename QIn, typename HOut, typename QOut, typename Put>
FS_RED_HD void summarize_series(int m, HIn &&h_in, QIn &&q_in, HOut &&h_out, QOut &&q_out, Put &&put) {
  double s_in = 0.0, s_out = 0.0, s_net = 0.0, cum_in = 0.0, cum_out = 0.0;
  double pq_in = red_nan(), pq_out = red_nan(), ph_in = red_nan(), ph_out = red_nan();
  int lq_in = -1, lq_out = -1, lh_in = -1, lh_out = -1;
  for (int k = 0; k < m; ++k) {
    const double hi = h_in(k), qi = q_in(k), ho = h_out(k), qo = q_out(k);
    if (k == m - 1) { cum_in = s_in; cum_out = s_out; }
    s_in += qi; s_out += qo; s_net += qi - qo;
    if (k == 0 || qi > pq_in) { pq_in = qi; lq_in = k; }
    if (k == 0 || qo > pq_out) { pq_out = qo; lq_out = k; }
    if (k == 0 || hi > ph_in) { ph_in = hi; lh_in = k; }
    if (k == 0 || ho > ph_out) { ph_out = ho; lh_out = k; }
  }
  int med_in = m > 0 ? 0 : -1, med_out = med_in;      // (no i passes the test only if a sample is NaN: np.argmax of all-False, 0)
  {
    const double half = 0.5 * cum_in;
    double c = 0.0;
    for (int i = 0; i < m; ++i) {
      if (c >= half) { med_in = i; break; }
      c += q_in(i);
    }
  }
  {
    const double half = 0.5 * cum_out;
    double c = 0.0;
    for (int i = 0; i < m; ++i) {
      if (c >= half) { med_out = i; break; }
      c += q_out(i);
    }
  }
  put(FS_SUM_LEVELS, (double)m);
  put(FS_SUM_Q_IN, s_in); put(FS_SUM_Q_OUT, s_out); put(FS_SUM_Q_NET, s_net);
  put(FS_SUM_PEAK_Q_IN, pq_in); put(FS_SUM_PEAK_Q_IN_LEVEL, (double)lq_in);
  put(FS_SUM_PEAK_Q_OUT, pq_out); put(FS_SUM_PEAK_Q_OUT_LEVEL, (double)lq_out);
  put(FS_SUM_PEAK_H_IN, ph_in); put(FS_SUM_PEAK_H_IN_LEVEL, (double)lh_in);
  put(FS_SUM_PEAK_H_OUT, ph_out); put(FS_SUM_PEAK_H_OUT_LEVEL, (double)lh_out);
  put(FS_SUM_MEDIAN_IN_LEVEL, (double)med_in); put(FS_SUM_MEDIAN_OUT_LEVEL, (double)med_out);
}

// np.interp(x, xp, fp) at one abscissa, as numpy's compiled loop evaluates it (arr_interp: clamp to the end values; the interval is
// the largest j with xp[j] <= x; a hit on a sample returns that sample; slope * (x - xp[j]) + fp[j], unfused).  xp(j), fp(j): sample
// j = 0 .. m-1.  On a series that is not nondecreasing the bisection still ends, on some interval: fs_batch_lookup flags such a reach.
template <typename Xp, typename Fp>
FS_RED_HD double interp_series(int m, Xp &&xp, Fp &&fp, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (m < 1 || x != x) return red_nan();
  if (m == 1) return fp(0);
  if (x > xp(m - 1)) return fp(m - 1);
  if (x < xp(0)) return fp(0);
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x >= xp(mid)) lo = mid + 1; else hi = mid;
  }
  const int j = lo - 1;
  if (j < 0) return fp(0);
  if (j >= m - 1) return fp(m - 1);
  const double xj = xp(j), fj = fp(j);
  if (xj == x) return fj;
  const double xn = xp(j + 1), fn = fp(j + 1);
  const double slope = (fn - fj) / (xn - xj);
  double v = slope * (x - xj) + fj;
  if (v != v) {                            // numpy's second and third try (an infinite sample or a zero-width interval)
    v = slope * (x - xn) + fn;
    if (v != v && fj == fn) v = fj;
  }
  return v;
}

// does the series descend anywhere?  (np.interp is defined for nondecreasing xp only)
template <typename Xp> FS_RED_HD bool series_descends(int m, Xp &&xp) {
  bool down = false;
  double prev = m > 0 ? xp(0) : 0.0;
  for (int j = 1; j < m; ++j) {
    const double v = xp(j);
    down = down || v < prev;
    prev = v;
  }
  return down;
}

// mean((v - t)^2) over n_q pairs, in order (np.mean adds fewer than eight terms in order too); the RMSE is its square root
template <typename V, typename T> FS_RED_HD double mean_square_series(int n_q, V &&v, T &&t) {
  double ss = 0.0;
  for (int i = 0; i < n_q; ++i) {
    const double d = v(i) - t(i);
    ss += d * d;
  }
  return ss / (double)n_q;
}

// numpy's default quantile (method "linear") between the two order statistics a <= b around the virtual index, gamma in [0, 1)
// (numpy/lib/_function_base_impl.py: _lerp), kept inside [a, b].  A virtual index that is an integer (gamma == 0) and two equal order
// statistics ARE the order statistic a: nothing is computed, so that an infinite member gives that infinity where numpy's inf - inf
// and inf * 0 give NaN (finite members: the same bits as the arithmetic, a + d * 0 and a + 0 * gamma).  An interpolation between an
// infinite and a finite member stays numpy's.
FS_RED_HD double quantile_lerp(double a, double b, double gamma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (gamma == 0.0 || a == b) return a;
  const double d = b - a;
  double v = gamma >= 0.5 ? b - d * (1.0 - gamma) : a + d * gamma;
  if (v < a) v = a;
  if (v > b) v = b;
  return v;
}

constexpr int kBandMaxQ = 16;                    // quantile levels per call of the band kernels (fs_host_post.hpp checks it)

}  // namespace fs

#if defined(__HIPCC__)

namespace fs {

// what every reduction reads: the hydrograph block in the batch's type, the per-reach status and Newton counts, the range
template <typename R> struct ReduceArgs {
  const R *hydro;                // [max_levels][4][B]
  const int32_t *status;         // [B]
  const int32_t *iters;          // [max_levels][B]
  int32_t B, level;              // the batch's current level: rows 0 .. level exist
  int32_t first, n;              // the range [first, first + n), inside 0 .. level
};

__device__ __forceinline__ bool red_failed(int32_t st) { return st != FS_OK && st != FS_ILL_CONDITIONED; }

// rows of the range that reach r completed.  A failed reach stops at its failing level: the last level that holds a Newton count
// (include/flowsim_abi.h: the count of the failing level is what that level began, the rows of later levels are 0); the rows before it
// are complete.
template <typename R> __device__ __forceinline__ int red_rows(const ReduceArgs<R> &a, int r) {
  int complete = a.level + 1;
  if (red_failed(a.status[r])) {
    complete = 1;
    for (int k = a.level; k >= 1; --k)
      if (a.iters[(size_t)k * a.B + r] > 0) { complete = k; break; }
  }
  const int m = complete - a.first;
  return m < 0 ? 0 : (m > a.n ? a.n : m);
}

constexpr int kSumLanes = 64;           // reaches per workgroup of the summary walk: one wave, one lane per reach (385 levels deep, so many
                                        // small workgroups spread a 32 768-member batch over every CU)

// out[FS_SUM_NROWS][B]: one lane per reach walks its four columns; consecutive lanes read consecutive members of a row
template <typename R> __global__ __launch_bounds__(kSumLanes) void summarize_kernel(const ReduceArgs<R> a, double *out) {
  const int r = blockIdx.x * kSumLanes + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B;
  const R *base = a.hydro + (size_t)a.first * 4 * B + r;
  auto col = [&](int s) { return [=](int k) { return (double)base[((size_t)k * 4 + s) * B]; }; };
  summarize_series(red_rows(a, r), col(0), col(1), col(2), col(3), [&](int row, double v) { out[(size_t)row * B + r] = v; });
}

// values[n_q][B]: one thread per (reach, query); a workgroup shares its query (blockIdx.y), which sits in a scalar register
template <typename R>
__global__ __launch_bounds__(256) void lookup_kernel(const ReduceArgs<R> a, int x_row, int y_row, const double *y_offset, const double *xq,
                                                     double *values) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B;
  const double x = xq[blockIdx.y];
  const double off = y_offset ? y_offset[r] : 0.0;
  const R *base = a.hydro + (size_t)a.first * 4 * B + r;
  auto xp = [=](int k) { return (double)base[((size_t)k * 4 + x_row) * B]; };
  auto fp = [=](int k) { return (double)base[((size_t)k * 4 + y_row) * B] + off; };
  values[(size_t)blockIdx.y * B + r] = interp_series(red_rows(a, r), xp, fp, x);
}

// per reach: is x nondecreasing over the rows it completed (info bit 0), and the RMSE of its values against the target
template <typename R>
__global__ __launch_bounds__(256) void lookup_finish_kernel(const ReduceArgs<R> a, int x_row, const double *values, const double *target, int n_q,
                                                            double *rmse, int32_t *info) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B;
  if (info) {
    const R *base = a.hydro + (size_t)a.first * 4 * B + r;
    info[r] = series_descends(red_rows(a, r), [=](int k) { return (double)base[((size_t)k * 4 + x_row) * B]; }) ? 1 : 0;
  }
  if (rmse)
    rmse[r] = __builtin_sqrt(mean_square_series(n_q, [=](int i) { return values[(size_t)i * B + r]; }, [=](int i) { return target[i]; }));
}

// ---- cross-member bands ----
constexpr int kBandThreads = 256;
constexpr int kBandTargets = 2 * kBandMaxQ;      // order statistics: the two around every virtual index

// the order-preserving integer image of a double (-0.0 has been folded into +0.0 before): negative values reversed below the positive
__device__ __forceinline__ unsigned long long band_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double band_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <typename Op> __device__ __forceinline__ double band_reduce(double v, double *scratch, Op op) {
  const int t = threadIdx.x;
  __syncthreads();                               // (the scratch of the reduction before is read)
  scratch[t] = v;
  __syncthreads();
  for (int w = kBandThreads / 2; w > 0; w >>= 1) {
    if (t < w) scratch[t] = op(scratch[t], scratch[t + w]);
    __syncthreads();
  }
  return scratch[0];
}

// One workgroup per (level, signal) row of B contiguous members.  Members whose status is a failure are left out.  min / max / mean /
// std: two passes in fp64.  Quantiles: exact order statistics by a most-significant-byte radix select over band_key - all 2 n_q ranks at
// once, one pass over the row (from L2: 256 KB at 32 768 fp64 members) per byte that min and max do not share, counts in LDS.
template <typename R>
__global__ __launch_bounds__(kBandThreads) void bands_kernel(const ReduceArgs<R> a, const double *q, int n_q, double *moments, double *quantiles,
                                                             int32_t *n_members) {
  __shared__ double s_red[kBandThreads];
  __shared__ unsigned int s_hist[kBandTargets][256];
  __shared__ unsigned long long s_pfx[kBandTargets];
  __shared__ unsigned int s_rank[kBandTargets];
  const int t = threadIdx.x, B = a.B;
  const int row = blockIdx.x;                                  // (level - first) * 4 + signal
  const R *x = a.hydro + ((size_t)a.first * 4 + row) * (size_t)B;
  const double nan = red_nan();

  double mn = __builtin_inf(), mx = -__builtin_inf(), sum = 0.0, cnt = 0.0, bad = 0.0;
  for (int i = t; i < B; i += kBandThreads) {
    if (red_failed(a.status[i])) continue;
    const double v = (double)x[i] + 0.0;
    if (v != v) bad += 1.0;
    mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    sum += v; cnt += 1.0;
  }
  auto add = [](double p, double r) { return p + r; };
  mn = band_reduce(mn, s_red, [](double p, double r) { return r < p ? r : p; });
  mx = band_reduce(mx, s_red, [](double p, double r) { return r > p ? r : p; });
  sum = band_reduce(sum, s_red, add);
  cnt = band_reduce(cnt, s_red, add);
  bad = band_reduce(bad, s_red, add);
  const int m = (int)cnt;
  const bool none = m == 0 || bad > 0.0;                       // no member left, or a NaN among them (numpy: NaN throughout)
  const double mean = sum / cnt;
  double ss = 0.0;
  for (int i = t; i < B; i += kBandThreads) {
    if (red_failed(a.status[i])) continue;
    const double d = ((double)x[i] + 0.0) - mean;
    ss += d * d;
  }
  ss = band_reduce(ss, s_red, add);
  if (t == 0) {
    if (n_members) n_members[row / 4] = m;                     // (the four signals of a level write the same count)
    if (moments) {
      double *o = moments + (size_t)row * 4;
      o[0] = none ? nan : mn; o[1] = none ? nan : mx; o[2] = none ? nan : mean; o[3] = none ? nan : __builtin_sqrt(ss / cnt);
    }
  }
  if (!quantiles || n_q < 1) return;
  double *qo = quantiles + (size_t)row * n_q;
  if (none) {
    if (t < n_q) qo[t] = nan;
    return;
  }
  const unsigned long long kmin = band_key(mn), kmax = band_key(mx);
  const int S = 2 * n_q;
  if (t < n_q) {                                               // the ranks around the virtual index (m - 1) q
    const double vi = (double)(m - 1) * q[t];
    int lo = (int)__builtin_floor(vi);
    lo = lo < 0 ? 0 : (lo > m - 1 ? m - 1 : lo);
    s_rank[2 * t] = (unsigned)lo;
    s_rank[2 * t + 1] = (unsigned)(lo + 1 > m - 1 ? m - 1 : lo + 1);
    s_pfx[2 * t] = kmin; s_pfx[2 * t + 1] = kmin;              // (the bytes min and max share are every member's)
  }
  __syncthreads();
  if (kmin != kmax) {
    const int lead = __clzll((long long)(kmin ^ kmax)) / 8;    // bytes, from the top, that every member shares
    if (t < S) s_pfx[t] &= lead == 0 ? 0ull : ~0ull << (64 - 8 * lead);
    for (int shift = 56 - 8 * lead; shift >= 0; shift -= 8) {
      for (int i = t; i < S * 256; i += kBandThreads) (&s_hist[0][0])[i] = 0u;
      __syncthreads();
      for (int i0 = 0; i0 < B; i0 += kBandThreads) {
        const int i = i0 + t;
        const bool in = i < B && !red_failed(a.status[i]);
        const unsigned long long key = in ? band_key((double)x[i] + 0.0) : 0ull;
        const unsigned bin = (unsigned)(key >> shift) & 255u;
        for (int s = 0; s < S; ++s) {
          // members that carry target s's bytes so far; a wave whose members all fall into one bin adds once
          const bool act = in && (shift == 56 || ((key ^ s_pfx[s]) >> (shift + 8)) == 0ull);
          const unsigned long long mask = __ballot(act);
          if (mask == 0ull) continue;
          const unsigned lb = (unsigned)__shfl((int)bin, __ffsll((long long)mask) - 1);
          if (__ballot(act && bin == lb) == mask) {
            if ((t & 63) == __ffsll((long long)mask) - 1) atomicAdd(&s_hist[s][lb], (unsigned)__popcll(mask));
          } else if (act) {
            atomicAdd(&s_hist[s][bin], 1u);
          }
        }
      }
      __syncthreads();
      if (t < S) {                                             // the bin that holds the rank, and the rank inside it
        unsigned rank = s_rank[t], below = 0u, b = 0u;
        for (; b < 255u; ++b) {
          const unsigned c = s_hist[t][b];
          if (rank < below + c) break;
          below += c;
        }
        s_rank[t] = rank - below;
        s_pfx[t] |= (unsigned long long)b << shift;
      }
      __syncthreads();
    }
  }
  if (t < n_q) {
    const double lo_v = band_unkey(s_pfx[2 * t]), hi_v = band_unkey(s_pfx[2 * t + 1]);
    const double vi = (double)(m - 1) * q[t];
    double g = vi - __builtin_floor(vi);
    if (vi >= (double)(m - 1)) g = 0.0;
    qo[t] = quantile_lerp(lo_v, hi_v, g);
  }
}

// the launchers (fs_part_reduce.hip); false: this build has no such kernel
bool launch_summarize(const ReduceArgs<double> &a, double *out, hipStream_t st);
bool launch_summarize(const ReduceArgs<float> &a, double *out, hipStream_t st);
struct LookupArgs {
  int32_t x_row, y_row, n_q;
  const double *y_offset, *xq, *target;     // device: [B] or nullptr, [n_q], [n_q] or nullptr
  double *values, *rmse;                    // device: [n_q][B], [B] or nullptr
  int32_t *info;                            // device: [B] or nullptr
};
bool launch_lookup(const ReduceArgs<double> &a, const LookupArgs &l, hipStream_t st);
bool launch_lookup(const ReduceArgs<float> &a, const LookupArgs &l, hipStream_t st);
struct BandArgs {
  const double *q; int32_t n_q;             // device [n_q]
  double *moments, *quantiles;              // device [n][4][4], [n][4][n_q] or nullptr
  int32_t *n_members;                       // device [n] or nullptr
};
bool launch_bands(const ReduceArgs<double> &a, const BandArgs &p, hipStream_t st);
bool launch_bands(const ReduceArgs<float> &a, const BandArgs &p, hipStream_t st);

}  // namespace fs
#endif
