// kernel instantiations of libflowsim_hip.so, part "gauges": interior gauge series and their fit scores (fs_gauge.hpp).  These kernels
// are not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
//
// The translation unit keeps the library's contraction setting: the section helpers of fs_derive.hpp must round here as they round in
// derive_fields_kernel, whose stage and velocity a gauge row is held to bit for bit.  What must round every product - gauge_value,
// score_series - says so itself (#pragma clang fp contract(off) in the function, as interp_series and balance_walk).
#include "fs_gauge.hpp"

namespace fs {
namespace {

// one thread per (level, member); history rows and the current state go through the same instantiation
template <typename R> bool gauge_gather(const GaugeArgs<R> &a, bool per_reach, hipStream_t st) {
  if (a.n_gauges < 1 || a.rows.n < 1) return true;
  const dim3 grid((unsigned)((a.B + kGaugeThreads - 1) / kGaugeThreads), (unsigned)(a.rows.n < 65535 ? a.rows.n : 65535));
  if (per_reach) hipLaunchKernelGGL((gauge_gather_kernel<R, true>), grid, dim3(kGaugeThreads), 0, st, a);
  else hipLaunchKernelGGL((gauge_gather_kernel<R, false>), grid, dim3(kGaugeThreads), 0, st, a);
  return true;
}

}  // namespace

bool launch_gauge_gather(const GaugeArgs<double> &a, bool per_reach, hipStream_t st) { return gauge_gather(a, per_reach, st); }
bool launch_gauge_gather(const GaugeArgs<float> &a, bool per_reach, hipStream_t st) { return gauge_gather(a, per_reach, st); }

bool launch_gauge_score(const ReduceArgs<double> &a, const ScoreArgs &p, hipStream_t st) {
  hipLaunchKernelGGL((gauge_score_kernel<kScoreLanes>), dim3((unsigned)((a.B + kScoreLanes - 1) / kScoreLanes)), dim3(kScoreLanes), 0, st, a, p);
  return true;
}

bool launch_gauge_members(const int32_t *status, const int32_t *reach_nodes, const int32_t *node, const double *weight, int G, int g,
                          int per_reach, int N, int B, int32_t *members, hipStream_t st) {
  hipLaunchKernelGGL((gauge_members_kernel<256>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, status, reach_nodes, node, weight, G, g,
                     per_reach, N, B, members);
  return true;
}

}  // namespace fs
