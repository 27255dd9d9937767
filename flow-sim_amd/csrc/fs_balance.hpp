// fs_balance.hpp - reductions ALONG the reach (fs_batch_reach_integrals) and the discrete water balance built on them
// (fs_batch_water_balance): how much water is in the channel, how much land is under water, and whether the run conserved mass.
//   reach integrals  per (level, reach): the trapezoid-rule volume and water surface of the node areas and top widths, and the length
//                    of reach whose stage stands at or above a threshold - one row of FS_INT_NROWS doubles, laid out as the hydrograph
//                    block, integ[level][FS_INT_NROWS][B], so that fs_batch_integral_bands is the shipped bands_kernel on it
//   water balance    per reach, from each evaluated row to the next (a span): the change of storage minus the net inflow volume of
//                    the Preissmann continuity row, (V_k - V_j) - sum dt [theta (Q_0 - Q_last)_l + (1 - theta) (Q_0 - Q_last)_{l-1}],
//                    which the scheme closes to its Newton tolerance; and its totals over the range
//
// The first part - the trapezoid weights of one row, the nodes one lane adds, the fold of the lanes' sums, and the walk over one
// reach's spans - is plain C++, generic over how a sample is read: tests/test_balance_host.py compiles it with the system compiler
// under sanitizers and holds it to numpy.  The kernels follow under __HIPCC__; they are instantiated in fs_part_balance.hip and have
// no row in the dispatch table.
#pragma once
#include <cstdint>

#include "../../include/flowsim_abi.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_BAL_HD __host__ __device__ __forceinline__
#else
#define FS_BAL_HD inline
#endif

namespace fs {

constexpr int kIntLanes = 64;          // lanes that share one row of the integrals: one wavefront

// the trapezoid rule over the nodes of one reach: half at node 0 and at the reach's own last node, one between
FS_BAL_HD double trapezoid_weight(int node, int nodes) { return (node == 0 || node == nodes - 1) ? 0.5 : 1.0; }

// the packs of one row that lane `lane` of `lanes` takes: V consecutive nodes at a stride of lanes V, in node order.  pack(i0, cnt)
// receives the first node and how many of the V exist (the row's last pack may be short); no node at or beyond `nodes` is named.
template <typename Pack> FS_BAL_HD void lane_packs(int nodes, int lane, int lanes, int V, Pack &&pack) {
  for (int i0 = lane * V; i0 < nodes; i0 += lanes * V) pack(i0, nodes - i0 < V ? nodes - i0 : V);
}

// the fixed tree that folds the lanes' sums: lane l adds lane l ^ 32, then l ^ 16 ... l ^ 1 (kIntLanes a power of two); every lane ends
// with the same bits, whatever the rows beside it hold.  The kernel runs it with __shfl_xor; this is its host statement.
FS_BAL_HD void fold_lanes(double (&p)[kIntLanes]) {
  for (int m = kIntLanes / 2; m >= 1; m >>= 1) {
    double q[kIntLanes];
    for (int l = 0; l < kIntLanes; ++l) q[l] = p[l] + p[l ^ m];
    for (int l = 0; l < kIntLanes; ++l) p[l] = q[l];
  }
}

// The water balance of ONE reach over the m rows it completed in the range.  evaluated(k): does row k hold integrals; vol(k): its
// FS_INT_VOLUME (read for evaluated rows only); q_in(k), q_out(k): the flow at node 0 and at the reach's last node, as doubles.  A span
// runs from one evaluated row to the next: one level where every row was evaluated, a chunk of levels where the state was marked now
// and then.  put_row(k, residual) receives FS_INT_BALANCE of every evaluated row - 0 for the first of the range, else the span's
// storage change minus its net inflow volume, accumulated level by level in level order; put_total(row, value) the FS_BAL_* rows.
// Levels are relative to the range's first, as doubles (-1: none).  A NaN volume or flow makes the residuals of the spans it touches
// NaN, and with them the sums; the largest |residual| then is NaN at the first such span's level, as np.max / np.argmax.
template <typename Ev, typename Vol, typename QIn, typename QOut, typename PutRow, typename PutTotal>
FS_BAL_HD void balance_walk(int m, Ev &&evaluated, Vol &&vol, QIn &&q_in, QOut &&q_out, double theta, double dt, PutRow &&put_row,
                            PutTotal &&put_total) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int spans = 0, first = -1, last = -1, worst_level = -1;
  double v_first = 0.0, v_prev = 0.0, net = 0.0, in = 0.0;      // net, in: of the open span
  double sum_net = 0.0, sum_in = 0.0, sum_res = 0.0, worst = 0.0;
  double qi_prev = 0.0, qo_prev = 0.0;
  for (int k = 0; k < m; ++k) {
    const double qi = q_in(k), qo = q_out(k);
    if (first >= 0) {
      net += dt * (theta * (qi - qo) + (1.0 - theta) * (qi_prev - qo_prev));
      in += dt * (theta * qi + (1.0 - theta) * qi_prev);
    }
    qi_prev = qi; qo_prev = qo;
    if (!evaluated(k)) continue;
    const double v = vol(k);
    if (first < 0) {
      first = k; v_first = v;
      put_row(k, 0.0);
    } else {
      const double res = (v - v_prev) - net, mag = res < 0.0 ? -res : res;
      put_row(k, res);
      ++spans;
      sum_net += net; sum_in += in; sum_res += res;
      if (worst_level < 0 || (worst == worst && !(mag <= worst))) { worst = mag; worst_level = k; }
    }
    v_prev = v; last = k;
    net = 0.0; in = 0.0;
  }
  const double nan = __builtin_nan("");
  put_total(FS_BAL_SPANS, (double)spans);
  put_total(FS_BAL_FIRST_LEVEL, (double)first); put_total(FS_BAL_LAST_LEVEL, (double)last);
  put_total(FS_BAL_STORAGE_CHANGE, first >= 0 ? v_prev - v_first : nan);
  put_total(FS_BAL_NET_INFLOW, sum_net); put_total(FS_BAL_INFLOW, sum_in);
  put_total(FS_BAL_RESIDUAL, sum_res);
  put_total(FS_BAL_WORST, spans > 0 ? worst : nan); put_total(FS_BAL_WORST_LEVEL, (double)worst_level);
  put_total(FS_BAL_RELATIVE, spans > 0 ? sum_res / sum_in : nan);
}

}  // namespace fs

#if defined(__HIPCC__)

#include "fs_derive.hpp"
#include "fs_reduce.hpp"

namespace fs {

template <typename R> struct IntegralArgs {
  int32_t B, N, section_mode;
  const R *src;                   // row (k, r) of the range starts at src + k level_stride + r N
  int64_t level_stride;           // B N: the depth history from the range's first level on; 0: the current state (a range of one row)
  SectionTables<R> sec;
  const int32_t *reach_nodes;     // [B] or nullptr (see DeriveArgs)
  ReduceArgs<R> rows;             // status, Newton counts and the range: red_rows says how many rows of a reach enter
  const double *dx;               // [B]: the caller's fp64 node spacing of each reach
  const R *threshold;             // [N], or [B][N] with threshold_per_reach; rounded once to the batch's type; nullptr: none
  int32_t threshold_per_reach;
  double *integ;                  // [max_levels][FS_INT_NROWS][B]: the handle's block (not the range's part of it)
  int32_t *mark;                  // [max_levels][B]: 1 where a row holds integrals
};
FS_ARGS_LAYOUT(IntegralArgs, 176, 32, reach_nodes, 88);

// One wavefront per (level, reach) row, four rows per 256-thread workgroup; consecutive waves take consecutive reaches of a level, so the
// grid streams the depth history once, in address order.  A lane takes the packs of V consecutive nodes (16 bytes) that lane_packs
// names - pack p of the row goes to lane p mod 64 whatever the row's address - and adds its terms in node order; the wave closes with
// fold_lanes' tree over __shfl_xor: no atomics, no LDS.  A row's value therefore depends on nothing but the row: not on B, not on the
// reach's place in the batch, not on the range asked for, and not on which array the row came from (history or current state: the
// same instantiation, the same assignment of nodes to lanes).
// Loads: a row starts at element r N, which for odd N is no 16-byte boundary.  A pack is one 16-byte load only when its own address is
// aligned and all V nodes exist; every other pack is read element by element.  No address outside [row, row + nodes) is touched.
// Area and top width are evaluated in the batch's type by the helpers derive_fields_kernel calls (section_at, section_area_top:
// fs_derive.hpp), inlined here; the section parameters are read per row (shared tables: from L1 / L2; per-reach tables: eight values
// per node and row from L2 / MALL).  Products with the weights and all sums are fp64.
// A wave that takes 2 or 4 consecutive rows in turn, their loads in flight together and shared tables read once, was measured and not
// kept (158 and 256 VGPRs, 3 and 1 waves per SIMD; the C4 history in 2.93 and 5.21 ms against 2.88 ms); two short
// rows packed into one wave (N <= 32 V) were not built: the C4 rows fill 61 of 64 lanes.
template <typename R, int V> __global__ __launch_bounds__(256) void reach_integrals_kernel(const IntegralArgs<R> a) {
  const int lane = threadIdx.x & (kIntLanes - 1);
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (size_t)a.rows.n * a.B) return;            // (the whole wave)
  const int k = (int)(row / a.B), reach = (int)(row - (size_t)k * a.B);
  const size_t B = a.B;
  const int level = a.rows.first + k;
  double *o = a.integ + (size_t)level * FS_INT_NROWS * B + reach;
  const double nan = red_nan();
  if (k >= red_rows(a.rows, reach)) {                   // a failed reach: the rows from its failing level on hold nothing
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < FS_INT_NROWS; ++q) o[(size_t)q * B] = nan;
      a.mark[(size_t)level * B + reach] = 0;
    }
    return;
  }
  const int nodes_r = a.reach_nodes ? a.reach_nodes[reach] : a.N;
  const R *h_row = a.src + (size_t)k * a.level_stride + (size_t)reach * a.N;
  const bool aligned = (reinterpret_cast<uintptr_t>(h_row) & 15u) == 0;
  double sum_a = 0.0, sum_t = 0.0, sum_l = 0.0;
  lane_packs(nodes_r, lane, kIntLanes, V, [&](int i0, int cnt) {
    R h[V];
    load_pack<R, V>(h_row + i0, aligned && cnt == V, cnt, h);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int node = i0 + (e < cnt ? e : 0);
      SecParams<R> se;
      PolyNode<R> pnode;
      R Te, Ae;
      section_at(a.sec, a.section_mode, a.B, a.N, reach, node, nodes_r, se, pnode);
      section_area_top(se, pnode, h[e], Ae, Te);
      bool over = false;
      if (a.threshold) over = h[e] + se.z >= a.threshold[a.threshold_per_reach ? (size_t)reach * a.N + node : (size_t)node];
      if (e < cnt) {
        const double w = trapezoid_weight(node, nodes_r);
        sum_a += w * (double)Ae; sum_t += w * (double)Te; sum_l += over ? w : 0.0;
      }
    }
  });
#pragma unroll
  for (int m = kIntLanes / 2; m >= 1; m >>= 1) {        // fold_lanes
    sum_a += __shfl_xor(sum_a, m, kIntLanes); sum_t += __shfl_xor(sum_t, m, kIntLanes); sum_l += __shfl_xor(sum_l, m, kIntLanes);
  }
  if (lane == 0) {
    const double dx = a.dx[reach];
    o[(size_t)FS_INT_VOLUME * B] = dx * sum_a;
    o[(size_t)FS_INT_SURFACE * B] = dx * sum_t;
    o[(size_t)FS_INT_LENGTH_OVER * B] = a.threshold ? dx * sum_l : nan;
    o[(size_t)FS_INT_BALANCE * B] = nan;                // (fs_batch_water_balance writes it)
    a.mark[(size_t)level * B + reach] = 1;
  }
}

struct BalanceArgs {
  double *integ;                  // [max_levels][FS_INT_NROWS][B]
  const int32_t *mark;            // [max_levels][B]
  const double *theta, *dt;       // [B]: the caller's fp64 values of each reach
  double *totals;                 // [FS_BAL_NROWS][B] or nullptr
};

constexpr int kBalLanes = 64;          // reaches per workgroup of the balance walk: one wave, one lane per reach, as summarize_kernel

// one lane per reach walks its rows of the range in level order; consecutive lanes read consecutive members of a row
template <typename R> __global__ __launch_bounds__(kBalLanes) void balance_kernel(const ReduceArgs<R> a, const BalanceArgs p) {
  const int r = blockIdx.x * kBalLanes + threadIdx.x;
  if (r >= a.B) return;
  const size_t B = a.B;
  const R *hyd = a.hydro + (size_t)a.first * 4 * B + r;
  double *integ = p.integ + (size_t)a.first * FS_INT_NROWS * B + r;
  const int32_t *mark = p.mark + (size_t)a.first * B + r;
  balance_walk(red_rows(a, r), [=](int k) { return mark[(size_t)k * B] != 0; },
               [=](int k) { return integ[((size_t)k * FS_INT_NROWS + FS_INT_VOLUME) * B]; },
               [=](int k) { return (double)hyd[((size_t)k * 4 + 1) * B]; }, [=](int k) { return (double)hyd[((size_t)k * 4 + 3) * B]; },
               p.theta[r], p.dt[r], [=](int k, double v) { integ[((size_t)k * FS_INT_NROWS + FS_INT_BALANCE) * B] = v; },
               [&](int row, double v) { if (p.totals) p.totals[(size_t)row * B + r] = v; });
}

// n doubles := NaN, n int32 := 0: rows that hold no integrals
template <int kThreads> __global__ __launch_bounds__(kThreads) void clear_integrals_kernel(double *integ, size_t n_integ, int32_t *mark, size_t n_mark) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_integ) integ[i] = red_nan();
  if (i < n_mark) mark[i] = 0;
}

// the launchers (fs_part_balance.hip); false: this build has no such kernel
bool launch_reach_integrals(const IntegralArgs<double> &a, hipStream_t st);
bool launch_reach_integrals(const IntegralArgs<float> &a, hipStream_t st);
bool launch_balance(const ReduceArgs<double> &a, const BalanceArgs &p, hipStream_t st);
bool launch_balance(const ReduceArgs<float> &a, const BalanceArgs &p, hipStream_t st);
bool launch_clear_integrals(double *integ, size_t n_integ, int32_t *mark, size_t n_mark, hipStream_t st);

}  // namespace fs
#endif
