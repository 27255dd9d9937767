// fs_envelope.hpp - flood envelopes of a stored history (fs_batch_envelope) and their bands across the members
// (fs_batch_profile_bands): what a flood study reads along the reach, reduced where the history is.
//   envelope       per (reach, node): the extremes of depth, stage, flow, velocity, Froude number and top width over the levels, the
//                  levels at which they occur, and when and for how long one of them stood at or above a threshold (bank, levee crest)
//   profile bands  per node, across the members: min, max, mean, std, exact quantiles of one row of that envelope, and the fraction of
//                  members that crossed the threshold there
//
// The first part - the walk over ONE series - is plain C++, generic over how a sample is read: tests/test_envelope_host.py compiles it
// with the system compiler under sanitizers and holds it to numpy.  The kernels follow under __HIPCC__; they are instantiated in
// fs_part_envelope.hip and have no row in the dispatch table.
#pragma once
#include <cstdint>

#include "../../include/flowsim_abi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_ENV_HD __host__ __device__ __forceinline__
#else
#define FS_ENV_HD inline
#endif

namespace fs {

// the extremes of one series so far.  Levels are first indices (np.argmax / np.argmin); a NaN sample behaves as in numpy: from the
// first NaN on the extreme is NaN and its level is that sample's.  No sample yet: levels -1 (the values are then not read).
template <typename T> struct EnvExtremes {
  T mx, mn;
  int32_t mx_level, mn_level;
};
template <typename T> FS_ENV_HD void env_begin(EnvExtremes<T> &s) { s.mx = s.mn = T(0); s.mx_level = s.mn_level = -1; }
template <typename T> FS_ENV_HD void env_take(EnvExtremes<T> &s, int k, T v) {
  const bool none = s.mx_level < 0;          // !(v <= mx): v is greater, or NaN; an extreme that is NaN stays
  if (none || (s.mx == s.mx && !(v <= s.mx))) { s.mx = v; s.mx_level = k; }
  if (none || (s.mn == s.mn && !(v >= s.mn))) { s.mn = v; s.mn_level = k; }
}

// the levels at which one series stood at or above a threshold: the first, the last, how many (-1, -1, 0: never).  A NaN threshold
// ("not assessed") and a NaN sample compare false, as numpy's >= does.
struct EnvCrossing {
  int32_t first, last, count;
};
FS_ENV_HD void env_begin(EnvCrossing &c) { c.first = c.last = -1; c.count = 0; }
template <typename T> FS_ENV_HD void env_take(EnvCrossing &c, int k, T v, T threshold) {
  if (v >= threshold) {
    if (c.first < 0) c.first = k;
    c.last = k;
    ++c.count;
  }
}

// one series of m samples, sample(k) in the type the comparisons run in; put(row, value) receives the FS_ENV_* statistics (a series
// without samples: NaN extremes, levels -1), cross(row, value) the FS_ENV_CROSS_* rows against `threshold`
template <typename T, typename Sample, typename Put, typename Cross>
FS_ENV_HD void envelope_series(int m, Sample &&sample, T threshold, Put &&put, Cross &&cross) {
  EnvExtremes<T> s;
  EnvCrossing c;
  env_begin(s);
  env_begin(c);
  for (int k = 0; k < m; ++k) {
    const T v = sample(k);
    env_take(s, k, v);
    env_take(c, k, v, threshold);
  }
  const double nan = __builtin_nan("");
  put(FS_ENV_MAX, m > 0 ? (double)s.mx : nan); put(FS_ENV_MAX_LEVEL, (double)s.mx_level);
  put(FS_ENV_MIN, m > 0 ? (double)s.mn : nan); put(FS_ENV_MIN_LEVEL, (double)s.mn_level);
  cross(FS_ENV_CROSS_FIRST, (double)c.first); cross(FS_ENV_CROSS_LAST, (double)c.last); cross(FS_ENV_CROSS_COUNT, (double)c.count);
}

constexpr int kEnvQuantities = 6;      // FS_ENV_DEPTH .. FS_ENV_TOP_WIDTH, in bit order

}  // namespace fs

#if defined(__HIPCC__)

#include "fs_derive.hpp"
#include "fs_reduce.hpp"

namespace fs {

template <typename R> struct EnvelopeArgs {
  int32_t B, N, first, n, section_mode;
  const R *hist_h, *hist_Q;       // [levels][B][N]
  SectionTables<R> sec;
  const int32_t *reach_nodes;     // [B] or nullptr (see DeriveArgs)
  ReduceArgs<R> rows;             // status, Newton counts and the range: red_rows says how many rows of a reach enter
  int32_t quantities;             // FS_ENV_* bit mask: which of the six are written, in bit order
  int32_t cross_q;                // 0 .. 5: the quantity held against the threshold, or -1: no crossings
  const R *threshold;             // [N], or [B][N] with threshold_per_reach; rounded once to the batch's type
  int32_t threshold_per_reach;
  double *out;                    // [n_selected][FS_ENV_NSTAT][B][N]
  double *crossing;               // [FS_ENV_NCROSS][B][N] or nullptr
  int32_t *levels;                // [B]: rows that entered
};
FS_ARGS_LAYOUT(EnvelopeArgs, 192, 40, reach_nodes, 96);

// One thread per V consecutive (reach, node) elements, as derive_fields_kernel: 16-byte history loads, consecutive threads on consecutive
// elements.  16 B in per element and level and nothing out until the walk is over: the loads of U levels are issued before the first of
// them is used.  The section, its area and its top width come from the helpers derive_fields_kernel calls (section_at, section_area_top:
// fs_derive.hpp), inlined here; what no selected quantity needs (the area, the divisions, the square root) is skipped, uniformly over the grid -
// with all six selected the walk is bound by its fp64 divisions, as derive_fields_kernel is, not by HBM.  kNeed: the quantities this
// instantiation can walk - kEnvPlain (depth, stage, flow: no section, a third of the registers, twice the waves) or FS_ENV_ALL.
constexpr int kEnvPlain = FS_ENV_DEPTH | FS_ENV_STAGE | FS_ENV_FLOW;
template <typename R, int V, int U, int kNeed> __global__ __launch_bounds__(256) void envelope_kernel(const EnvelopeArgs<R> a) {
  const size_t BN = (size_t)a.B * a.N;
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i0 >= BN) return;
  const int cnt = (int)(BN - i0 < (size_t)V ? BN - i0 : (size_t)V);
  const bool whole = cnt == V && BN % V == 0;        // every level's row of this thread starts on a 16-byte boundary
  SecParams<R> s[V];
  PolyNode<R> pnode[V];
  bool beyond[V];                            // ragged batches: a slot past the reach's own node count
  int rows[V];                               // rows of the range that the element's reach completed
  R thr[V];
  EnvExtremes<R> ext[V][kEnvQuantities];
  EnvCrossing crs[V];
  int most = 0;
  const int selected = a.quantities & kNeed;
  const int need = (a.quantities | (a.cross_q >= 0 ? 1 << a.cross_q : 0)) & kNeed;      // the quantities that are walked
  const bool need_flow = (need & (FS_ENV_FLOW | FS_ENV_VELOCITY | FS_ENV_FROUDE)) != 0;      // else the flow history is not read
  const bool need_area = (need & (FS_ENV_VELOCITY | FS_ENV_FROUDE | FS_ENV_TOP_WIDTH)) != 0;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const size_t i = i0 + (e < cnt ? e : 0);
    const int reach = (int)(i / a.N), node = (int)(i - (size_t)reach * a.N);
    const int nodes_r = a.reach_nodes ? a.reach_nodes[reach] : a.N;
    beyond[e] = node >= nodes_r;
    rows[e] = red_rows(a.rows, reach);
    if (node == 0 && e < cnt && a.levels) a.levels[reach] = rows[e];
    most = rows[e] > most ? rows[e] : most;
    thr[e] = a.cross_q >= 0 ? a.threshold[a.threshold_per_reach ? i : (size_t)node] : R(0);
    section_at(a.sec, a.section_mode, a.B, a.N, reach, node, nodes_r, s[e], pnode[e]);
    env_begin(crs[e]);
#pragma unroll
    for (int q = 0; q < kEnvQuantities; ++q) env_begin(ext[e][q]);
  }
  for (int k0 = 0; k0 < most; k0 += U) {     // (rows of a failed reach beyond its own count are loaded and not taken)
    R hh[U][V], QQ[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u < most ? k0 + u : most - 1;
      const size_t src = (size_t)(a.first + k) * BN + i0;
      load_pack<R, V>(a.hist_h + src, whole, cnt, hh[u]);
      if (need_flow) {
        load_pack<R, V>(a.hist_Q + src, whole, cnt, QQ[u]);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) QQ[u][e] = R(0);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u;
      R (&h)[V] = hh[u];
      R (&Q)[V] = QQ[u];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (beyond[e]) { h[e] = R(1); Q[e] = R(0); }        // (never written by the step kernel)
        const SecParams<R> &se = s[e];
        R Ae = R(0), Te = R(0), Ve = R(0), Fre = R(0);
        if (need_area) section_area_top(se, pnode[e], h[e], Ae, Te);
        if (need & FS_ENV_VELOCITY) Ve = Q[e] / Ae;
        if (need & FS_ENV_FROUDE) {              // hydraulics.py:155-168 with its clamps
          const R Vc = Q[e] / fmax_(Ae, R(1e-6)), D = Ae / fmax_(Te, R(1e-6));
          Fre = Vc / sqrt_(R(kG) * fmax_(D, R(1e-6)));
        }
        const R val[kEnvQuantities] = {h[e], h[e] + se.z, Q[e], Ve, Fre, Te};      // FS_ENV_DEPTH .. FS_ENV_TOP_WIDTH
        if (k < rows[e]) {
#pragma unroll
          for (int q = 0; q < kEnvQuantities; ++q) {
            if (!(need & (1 << q))) continue;
            env_take(ext[e][q], k, val[q]);
            if (q == a.cross_q) env_take(crs[e], k, val[q], thr[e]);
          }
        }
      }
    }
  }
  const double nan = red_nan();
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if (e >= cnt) continue;
    const bool none = rows[e] < 1;
    int sel = 0;
#pragma unroll
    for (int q = 0; q < kEnvQuantities; ++q) {
      if (!(selected & (1 << q))) continue;
      double *o = a.out + (size_t)sel * FS_ENV_NSTAT * BN + i0 + e;
      const EnvExtremes<R> &x = ext[e][q];
      o[(size_t)FS_ENV_MAX * BN] = beyond[e] ? 0.0 : none ? nan : (double)x.mx;
      o[(size_t)FS_ENV_MAX_LEVEL * BN] = beyond[e] ? -1.0 : (double)x.mx_level;
      o[(size_t)FS_ENV_MIN * BN] = beyond[e] ? 0.0 : none ? nan : (double)x.mn;
      o[(size_t)FS_ENV_MIN_LEVEL * BN] = beyond[e] ? -1.0 : (double)x.mn_level;
      ++sel;
    }
    if (a.crossing) {
      double *o = a.crossing + i0 + e;
      o[(size_t)FS_ENV_CROSS_FIRST * BN] = beyond[e] ? -1.0 : (double)crs[e].first;
      o[(size_t)FS_ENV_CROSS_LAST * BN] = beyond[e] ? -1.0 : (double)crs[e].last;
      o[(size_t)FS_ENV_CROSS_COUNT * BN] = beyond[e] ? 0.0 : (double)crs[e].count;
    }
  }
}

// ---- across the members, per node ----
constexpr int kTransposeTile = 32;
// (the two kernels below are templates so that only fs_part_envelope.hip, which names them, holds their code)

struct TransposeRows { const double *row[2]; };       // device [B][N] each; blockIdx.z says which

// row[z][B][N] -> out[z][N][B] (doubles), 32 x 32 tiles through LDS: both sides move whole rows of a tile
template <int kTile> __global__ __launch_bounds__(kTile * 8) void transpose_rows_kernel(const TransposeRows in, double *out, int B, int N) {
  __shared__ double tile[kTile][kTile + 1];
  const double *src = in.row[blockIdx.z];
  double *dst = out + (size_t)blockIdx.z * B * N;
  const int n0 = blockIdx.x * kTile, b0 = blockIdx.y * kTile;
  for (int j = threadIdx.y; j < kTile; j += 8) {
    const int b = b0 + j, n = n0 + threadIdx.x;
    if (b < B && n < N) tile[j][threadIdx.x] = src[(size_t)b * N + n];
  }
  __syncthreads();
  for (int j = threadIdx.y; j < kTile; j += 8) {
    const int n = n0 + j, b = b0 + threadIdx.x;
    if (b < B && n < N) dst[(size_t)n * B + b] = tile[threadIdx.x][j];
  }
}

struct ProfileBandArgs {
  const double *x;                // [N][B]: the chosen row of the envelope, transposed
  const double *count;            // [N][B]: its crossing counts, transposed, or nullptr
  const int32_t *status;          // [B]
  const int32_t *levels;          // [B]: rows of each member that entered the envelope
  const int32_t *reach_nodes;     // [B] or nullptr
  int32_t B, N;
  const double *q; int32_t n_q;   // device [n_q]
  double *moments, *quantiles, *exceed;      // device [N][4], [N][n_q], [N] or nullptr
  int32_t *n_members;             // device [N] or nullptr
};

// One workgroup per node, on the B contiguous members of its transposed row: bands_kernel's two passes and radix select (fs_reduce.hpp)
// with the members that are left out decided per node - failed, without rows, or (ragged batches) without this node.
template <int kThreads> __global__ __launch_bounds__(kThreads) void profile_bands_kernel(const ProfileBandArgs a) {
  static_assert(kThreads == kBandThreads, "band_reduce folds kBandThreads partial results");
  __shared__ double s_red[kBandThreads];
  __shared__ unsigned int s_hist[kBandTargets][256];
  __shared__ unsigned long long s_pfx[kBandTargets];
  __shared__ unsigned int s_rank[kBandTargets];
  const int t = threadIdx.x, B = a.B;
  const int node = blockIdx.x;
  const double *x = a.x + (size_t)node * B;
  const double nan = red_nan();
  const int n_q = a.n_q;
  auto enters = [&](int i) { return !red_failed(a.status[i]) && a.levels[i] > 0 && node < (a.reach_nodes ? a.reach_nodes[i] : a.N); };

  double mn = __builtin_inf(), mx = -__builtin_inf(), sum = 0.0, cnt = 0.0, bad = 0.0, over = 0.0;
  for (int i = t; i < B; i += kBandThreads) {
    if (!enters(i)) continue;
    const double v = x[i] + 0.0;
    if (v != v) bad += 1.0;
    mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    sum += v; cnt += 1.0;
    if (a.count && a.count[(size_t)node * B + i] > 0.0) over += 1.0;
  }
  auto add = [](double p, double r) { return p + r; };
  mn = band_reduce(mn, s_red, [](double p, double r) { return r < p ? r : p; });
  mx = band_reduce(mx, s_red, [](double p, double r) { return r > p ? r : p; });
  sum = band_reduce(sum, s_red, add);
  cnt = band_reduce(cnt, s_red, add);
  bad = band_reduce(bad, s_red, add);
  over = band_reduce(over, s_red, add);
  const int m = (int)cnt;
  const bool none = m == 0 || bad > 0.0;                       // no member left, or a NaN among them (numpy: NaN throughout)
  const double mean = sum / cnt;
  double ss = 0.0;
  for (int i = t; i < B; i += kBandThreads) {
    if (!enters(i)) continue;
    const double d = (x[i] + 0.0) - mean;
    ss += d * d;
  }
  ss = band_reduce(ss, s_red, add);
  if (t == 0) {
    if (a.n_members) a.n_members[node] = m;
    if (a.exceed) a.exceed[node] = m == 0 ? nan : over / cnt;
    if (a.moments) {
      double *o = a.moments + (size_t)node * 4;
      o[0] = none ? nan : mn; o[1] = none ? nan : mx; o[2] = none ? nan : mean; o[3] = none ? nan : __builtin_sqrt(ss / cnt);
    }
  }
  if (!a.quantiles || n_q < 1) return;
  double *qo = a.quantiles + (size_t)node * n_q;
  if (none) {
    if (t < n_q) qo[t] = nan;
    return;
  }
  const unsigned long long kmin = band_key(mn), kmax = band_key(mx);
  const int S = 2 * n_q;
  if (t < n_q) {                                               // the ranks around the virtual index (m - 1) q
    const double vi = (double)(m - 1) * a.q[t];
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
        const bool in = i < B && enters(i);
        const unsigned long long key = in ? band_key(x[i] + 0.0) : 0ull;
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
    const double vi = (double)(m - 1) * a.q[t];
    double g = vi - __builtin_floor(vi);
    if (vi >= (double)(m - 1)) g = 0.0;
    qo[t] = quantile_lerp(lo_v, hi_v, g);
  }
}

// the launchers (fs_part_envelope.hip); false: this build has no such kernel.  unroll: levels whose loads one thread has in flight (0: the launcher's choice)
bool launch_envelope(const EnvelopeArgs<double> &a, int unroll, hipStream_t st);
bool launch_envelope(const EnvelopeArgs<float> &a, int unroll, hipStream_t st);
bool launch_transpose_rows(const TransposeRows &rows, int n_rows, double *out, int B, int N, hipStream_t st);
bool launch_profile_bands(const ProfileBandArgs &a, hipStream_t st);

}  // namespace fs
#endif
