// kernel instantiations of libflowsim_hip.so, part "reduce": ensemble post-processing on the device (fs_reduce.hpp).  These kernels are
// not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
#include "fs_reduce.hpp"

namespace fs {
namespace {

dim3 blocks_of(int n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

template <typename R> bool summarize(const ReduceArgs<R> &a, double *out, hipStream_t st) {
  hipLaunchKernelGGL((summarize_kernel<R>), blocks_of(a.B, kSumLanes), dim3(kSumLanes), 0, st, a, out);
  return true;
}

template <typename R> bool lookup(const ReduceArgs<R> &a, const LookupArgs &l, hipStream_t st) {
  hipLaunchKernelGGL((lookup_kernel<R>), dim3((unsigned)((a.B + 255) / 256), (unsigned)l.n_q), dim3(256), 0, st, a, (int)l.x_row, (int)l.y_row,
                     l.y_offset, l.xq, l.values);
  if (l.rmse || l.info)
    hipLaunchKernelGGL((lookup_finish_kernel<R>), blocks_of(a.B, 256), dim3(256), 0, st, a, (int)l.x_row, (const double *)l.values, l.target,
                       (int)l.n_q, l.rmse, l.info);
  return true;
}

template <typename R> bool bands(const ReduceArgs<R> &a, const BandArgs &p, hipStream_t st) {
  hipLaunchKernelGGL((bands_kernel<R>), dim3((unsigned)a.n * 4u), dim3(kBandThreads), 0, st, a, p.q, (int)p.n_q, p.moments, p.quantiles,
                     p.n_members);
  return true;
}

}  // namespace

bool launch_summarize(const ReduceArgs<double> &a, double *out, hipStream_t st) { return summarize(a, out, st); }
bool launch_summarize(const ReduceArgs<float> &a, double *out, hipStream_t st) { return summarize(a, out, st); }
bool launch_lookup(const ReduceArgs<double> &a, const LookupArgs &l, hipStream_t st) { return lookup(a, l, st); }
bool launch_lookup(const ReduceArgs<float> &a, const LookupArgs &l, hipStream_t st) { return lookup(a, l, st); }
bool launch_bands(const ReduceArgs<double> &a, const BandArgs &p, hipStream_t st) { return bands(a, p, st); }
bool launch_bands(const ReduceArgs<float> &a, const BandArgs &p, hipStream_t st) { return bands(a, p, st); }

}  // namespace fs
