// fs_gauge.hpp - interior gauges: the series of depth, flow, stage and velocity at stations inside the reach (fs_batch_set_gauges,
// fs_batch_gauges), kept per gauge in a block of the hydrograph block's shape, gauge[G][max_levels][FS_GAUGE_NROWS][B], so that
// fs_batch_gauge_bands and fs_batch_gauge_lookup are the shipped kernels of fs_reduce.hpp on it; and the fit of each member to a gauge
// record (fs_batch_gauge_score).
//   gather   per (level, member): the two nodes around every gauge from the history row (or the current state), the four quantities as
//            fs_batch_derive evaluates them, and a + weight (b - a) in fp64
//   score    per member: count, bias, RMSE, Nash-Sutcliffe efficiency and the peaks of one signal of one gauge against observations
//
// The first part - the value of a gauge between its two nodes, the validation of a gauge list, the layouts of the block and of the
// marks, and the walk of one member's series against its observations - is plain C++, generic over how a sample is read:
// tests/test_gauge_host.py compiles it with the system compiler under sanitizers and holds it to a sequential restatement bit for
// bit.  The kernels follow under __HIPCC__; they are instantiated in fs_part_gauges.hip and have no row in the dispatch table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/flowsim_abi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_GAUGE_HD __host__ __device__ __forceinline__
#else
#define FS_GAUGE_HD inline
#endif

namespace fs {

static_assert(FS_GAUGE_NROWS == 4, "a gauge's block has the shape of the hydrograph block: bands_kernel and lookup_kernel walk four rows a level");
static_assert(FS_GAUGE_MAX <= 32, "one int32 of marks per (level, member): bit g is gauge g's");

// the value at weight w in [0, 1) of the way from a (node) to b (node + 1): the product is rounded before the sum.  w == 0 IS a - b
// may be anything (the caller does not read a node that may not exist, and hands whatever it likes)
FS_GAUGE_HD double gauge_value(double a, double b, double w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (w == 0.0) return a;
  const double d = b - a;
  const double p = w * d;
  return a + p;
}

// does a reach of `nodes` nodes have a gauge at (node, w)?  Both nodes it reads must be the reach's own.
FS_GAUGE_HD bool gauge_on_reach(int node, double w, int nodes) { return node >= 0 && node < nodes && (w == 0.0 || node + 1 < nodes); }

// what fs_batch_set_gauges is handed: n_gauges of 0 .. FS_GAUGE_MAX, and `count` = n_gauges (shared) or B n_gauges (per reach)
// positions in rows of N node slots.  Returns the error text, or nothing.
inline std::string check_gauge_list(const char *entry, int32_t n_gauges, const int32_t *node, const double *weight, size_t count, int32_t N) {
  const std::string e(entry);
  if (n_gauges < 0 || n_gauges > FS_GAUGE_MAX) return e + ": n_gauges must be 0 .. " + std::to_string(FS_GAUGE_MAX) + ", not " + std::to_string(n_gauges);
  if (n_gauges == 0) return {};
  if (!node || !weight) return e + ": null node or weight";
  for (size_t i = 0; i < count; ++i) {
    const std::string at = " (entry " + std::to_string(i) + ")";
    if (node[i] < 0 || node[i] >= N) return e + ": node " + std::to_string(node[i]) + " is not inside 0 .. " + std::to_string(N - 1) + at;
    const double w = weight[i];
    if (!(w >= 0.0 && w < 1.0)) return e + ": weights must be finite and in [0, 1)" + at;      // (a NaN is not)
    if (w != 0.0 && node[i] + 1 >= N)
      return e + ": a gauge with a weight that is not 0 reads node + 1 = " + std::to_string(node[i] + 1) + ", which is not inside 0 .. " +
             std::to_string(N - 1) + at;
  }
  return {};
}

// the block gauge[G][L][FS_GAUGE_NROWS][B] and the marks [L][B], in elements
struct GaugeLayout {
  size_t G, L, B;
  size_t per_gauge() const { return L * FS_GAUGE_NROWS * B; }                       // one gauge's block: the hydrograph block's shape
  size_t block() const { return G * per_gauge(); }
  size_t marks() const { return L * B; }
  size_t row(size_t g, size_t level, size_t q) const { return (g * L + level) * FS_GAUGE_NROWS * B + q * B; }      // member 0 of it
  size_t mark(size_t level) const { return level * B; }
};

// One member's series of one gauge signal against its observations over m levels.  marked(k): does the row of level k hold values;
// sim(k), obs(k): the simulated and the observed value (sim is read at counted levels only; a NaN obs: no observation).  A level
// counts when it is marked and observed.  Two walks in level order, every product rounded: the count, the sum of the observations and
// the first-index maxima (np.max / np.argmax: a NaN takes the peak at its first level and keeps it), then the sums of the error, its
// square and the squared deviation of the observations from their mean.  put(row, value) receives the FS_GS_* rows; levels are relative
// to the range's first, as doubles.  m counted == 0: count 0, levels -1, the rest NaN.
template <typename Marked, typename Sim, typename Obs, typename Put>
FS_GAUGE_HD void score_series(int m, Marked &&marked, Sim &&sim, Obs &&obs, Put &&put) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int cnt = 0, ls = -1, lo = -1;
  double sum_o = 0.0, ps = 0.0, po = 0.0;
  for (int k = 0; k < m; ++k) {
    if (!marked(k)) continue;
    const double o = obs(k);
    if (o != o) continue;
    const double s = sim(k);
    if (cnt == 0 || (ps == ps && !(s <= ps))) { ps = s; ls = k; }
    if (cnt == 0 || o > po) { po = o; lo = k; }
    sum_o += o;
    ++cnt;
  }
  const double nan = __builtin_nan("");
  const bool none = cnt == 0;
  const double mean_o = none ? nan : sum_o / (double)cnt;
  double se = 0.0, sq = 0.0, so = 0.0;
  for (int k = 0; k < m; ++k) {
    if (!marked(k)) continue;
    const double o = obs(k);
    if (o != o) continue;
    const double e = sim(k) - o, d = o - mean_o;
    const double ee = e * e, dd = d * d;
    se += e; sq += ee; so += dd;
  }
  const double ratio = sq / so;
  put(FS_GS_COUNT, (double)cnt);
  put(FS_GS_BIAS, none ? nan : se / (double)cnt);
  put(FS_GS_RMSE, none ? nan : __builtin_sqrt(sq / (double)cnt));
  put(FS_GS_NSE, none ? nan : 1.0 - ratio);
  put(FS_GS_PEAK_SIM, none ? nan : ps);
  put(FS_GS_PEAK_SIM_LEVEL, (double)ls);
  put(FS_GS_PEAK_ERROR, none ? nan : ps - po);
  put(FS_GS_PEAK_LAG, none ? nan : (double)(ls - lo));
}

}  // namespace fs

#if defined(__HIPCC__)

#include "fs_derive.hpp"
#include "fs_reduce.hpp"

namespace fs {

template <typename R> struct GaugeArgs {
  int32_t B, N, section_mode, n_gauges;
  const R *src_h, *src_Q;         // row (k, r) of the range starts at src + k level_stride + r N
  int64_t level_stride;           // B N: the histories from the range's first level on; 0: the current state (a range of one row)
  SectionTables<R> sec;
  const int32_t *reach_nodes;     // [B] or nullptr (see DeriveArgs)
  ReduceArgs<R> rows;             // status, Newton counts and the range: red_rows says how many rows of a reach enter
  const int32_t *node;            // [G], or [B][G] in the per-reach instantiation
  const double *weight;           // the same shape
  double *gauge;                  // [G][max_levels][FS_GAUGE_NROWS][B]: the handle's block (not the range's part of it)
  int32_t *mark;                  // [max_levels][B]: bit g set where gauge g's row holds values
  int32_t max_levels;
};

// a value every lane reads from the same address, never written while the kernel runs: read through the constant address space, so
// that the load is a scalar one and the value lives in scalar registers
template <typename T> __device__ __forceinline__ T load_shared_position(const T *p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) T *>(reinterpret_cast<uintptr_t>(p));
}

constexpr int kGaugeThreads = 256;
constexpr int kGaugeUnroll = 4;        // gauges whose loads a thread has in flight before the first of them is used

// One thread per (level, member): blockIdx.y walks the levels, consecutive lanes take consecutive members, so every store - one per
// (gauge, quantity) - is a row of consecutive doubles of the member-minor block.  The loads are the other way round: consecutive members
// are N elements apart, one cache line per lane, four lines per gauge and lane at most (depth and flow at node and node + 1, which
// share a line more often than not) against the N sizeof(R) / 128 lines a streamed row costs.  The loads of kGaugeUnroll gauges are
// issued before the first is used.  Shared positions (kPerReach false) are read through a uniform index and stay in scalar registers;
// per-reach ones are a lane's own.  The section, its bed level and its area come from the helpers derive_fields_kernel calls
// (section_at, section_area_top: fs_derive.hpp), inlined here under the library's contraction setting so that stage and velocity carry
// derive's bits; only gauge_value rounds its product.  Node + 1 is neither read nor evaluated where the weight is 0; a row that holds
// nothing (failed reach, gauge beyond the reach) evaluates nothing.  No atomics, no LDS, no cross-lane traffic: a row's value depends
// on (level, member, gauge) alone.  A thread writes the marks of its (level, member) once, all gauges in one word.
template <typename R, bool kPerReach> __global__ __launch_bounds__(kGaugeThreads) void gauge_gather_kernel(const GaugeArgs<R> a) {
  const int r = blockIdx.x * kGaugeThreads + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B, N = a.N, L = a.max_levels;
  const int G = a.n_gauges;
  const int nodes_r = a.reach_nodes ? a.reach_nodes[r] : a.N;
  const int m = red_rows(a.rows, r);
  const double nan = red_nan();
  for (int k = blockIdx.y; k < a.rows.n; k += gridDim.y) {
    const size_t level = (size_t)(a.rows.first + k);
    const R *h_row = a.src_h + (size_t)k * a.level_stride + (size_t)r * N;
    const R *Q_row = a.src_Q + (size_t)k * a.level_stride + (size_t)r * N;
    const bool live = k < m;                            // a failed reach: the rows from its failing level on hold nothing
    uint32_t bits = 0;
    for (int g0 = 0; g0 < G; g0 += kGaugeUnroll) {
      int node[kGaugeUnroll];
      double w[kGaugeUnroll];
      bool has[kGaugeUnroll], two[kGaugeUnroll];
      R ha[kGaugeUnroll], Qa[kGaugeUnroll], hb[kGaugeUnroll], Qb[kGaugeUnroll];
#pragma unroll
      for (int u = 0; u < kGaugeUnroll; ++u) {
        const int g = g0 + u < G ? g0 + u : G - 1;
        if (kPerReach) {
          node[u] = a.node[(size_t)r * G + g]; w[u] = a.weight[(size_t)r * G + g];
        } else {
          node[u] = load_shared_position(a.node + g); w[u] = load_shared_position(a.weight + g);
        }
        has[u] = live && gauge_on_reach(node[u], w[u], nodes_r);
        two[u] = has[u] && w[u] != 0.0;
        const int ia = has[u] ? node[u] : 0, ib = two[u] ? node[u] + 1 : ia;      // (no address outside [row, row + nodes_r))
        ha[u] = h_row[ia]; Qa[u] = Q_row[ia];
        hb[u] = h_row[ib]; Qb[u] = Q_row[ib];
      }
#pragma unroll
      for (int u = 0; u < kGaugeUnroll; ++u) {
        const int g = g0 + u;
        if (g >= G) continue;
        double v[FS_GAUGE_NROWS] = {nan, nan, nan, nan};
        if (has[u]) {
          SecParams<R> se;
          PolyNode<R> pnode;
          R Ae, Te;
          section_at(a.sec, a.section_mode, a.B, a.N, (size_t)r, node[u], nodes_r, se, pnode);
          section_area_top(se, pnode, ha[u], Ae, Te);
          const double va[FS_GAUGE_NROWS] = {(double)ha[u], (double)Qa[u], (double)(ha[u] + se.z), (double)(Qa[u] / Ae)};
          double vb[FS_GAUGE_NROWS] = {0.0, 0.0, 0.0, 0.0};
          if (two[u]) {
            section_at(a.sec, a.section_mode, a.B, a.N, (size_t)r, node[u] + 1, nodes_r, se, pnode);
            section_area_top(se, pnode, hb[u], Ae, Te);
            vb[FS_GAUGE_DEPTH] = (double)hb[u]; vb[FS_GAUGE_FLOW] = (double)Qb[u];
            vb[FS_GAUGE_STAGE] = (double)(hb[u] + se.z); vb[FS_GAUGE_VELOCITY] = (double)(Qb[u] / Ae);
          }
#pragma unroll
          for (int q = 0; q < FS_GAUGE_NROWS; ++q) v[q] = gauge_value(va[q], vb[q], w[u]);
          bits |= 1u << g;
        }
        double *o = a.gauge + (((size_t)g * L + level) * FS_GAUGE_NROWS) * B + r;
#pragma unroll
        for (int q = 0; q < FS_GAUGE_NROWS; ++q) o[(size_t)q * B] = v[q];
      }
    }
    a.mark[level * B + r] = (int32_t)bits;
  }
}

struct ScoreArgs {
  const double *gauge;            // [max_levels][FS_GAUGE_NROWS][B]: ONE gauge's block
  const int32_t *mark;            // [max_levels][B]
  int32_t bit, signal;            // the gauge's bit of the marks; FS_GAUGE_*
  const double *observed;         // [n], or [n][B] with observed_per_reach
  int32_t observed_per_reach;
  double *out;                    // [FS_GS_NROWS][B]
};

constexpr int kScoreLanes = 64;        // members per workgroup of the score walk: one wave, one lane per member, as summarize_kernel

// one lane per member walks its levels of the range twice, in level order; consecutive lanes read consecutive members of a row
// (a template, as gauge_members_kernel below, so that only fs_part_gauges.hip, which names them, holds their code; the block is fp64
// whatever the batch's type, so the range comes as a ReduceArgs<double>, of which red_rows reads the status and the Newton counts)
template <int kLanes> __global__ __launch_bounds__(kLanes) void gauge_score_kernel(const ReduceArgs<double> a, const ScoreArgs p) {
  const int r = blockIdx.x * kLanes + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B;
  const double *sim = p.gauge + ((size_t)a.first * FS_GAUGE_NROWS + p.signal) * B + r;
  const int32_t *mark = p.mark + (size_t)a.first * B + r;
  const double *obs = p.observed + (p.observed_per_reach ? (size_t)r : 0);
  const size_t obs_stride = p.observed_per_reach ? B : 1;
  const int32_t bit = p.bit;
  score_series(red_rows(a, r), [=](int k) { return ((mark[(size_t)k * B] >> bit) & 1) != 0; },
               [=](int k) { return sim[(size_t)k * FS_GAUGE_NROWS * B]; }, [=](int k) { return obs[(size_t)k * obs_stride]; },
               [&](int row, double v) { p.out[(size_t)row * B + r] = v; });
}

// members[B] := the batch's status of a member that has the gauge, FS_NAN for one that does not: the status bands_kernel leaves a
// member out by, so that a reach without the gauge is left out of that gauge's bands as a failed one is
template <int kThreads> __global__ __launch_bounds__(kThreads) void gauge_members_kernel(const int32_t *status, const int32_t *reach_nodes,
                                                                                        const int32_t *node, const double *weight, int G,
                                                                                        int g, int per_reach, int N, int B, int32_t *members) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= B) return;
  const size_t at = per_reach ? (size_t)r * G + g : (size_t)g;
  members[r] = gauge_on_reach(node[at], weight[at], reach_nodes ? reach_nodes[r] : N) ? status[r] : (int32_t)FS_NAN;
}

// the launchers (fs_part_gauges.hip); false: this build has no such kernel
bool launch_gauge_gather(const GaugeArgs<double> &a, bool per_reach, hipStream_t st);
bool launch_gauge_gather(const GaugeArgs<float> &a, bool per_reach, hipStream_t st);
bool launch_gauge_score(const ReduceArgs<double> &a, const ScoreArgs &p, hipStream_t st);
bool launch_gauge_members(const int32_t *status, const int32_t *reach_nodes, const int32_t *node, const double *weight, int G, int g,
                          int per_reach, int N, int B, int32_t *members, hipStream_t st);

}  // namespace fs
#endif
