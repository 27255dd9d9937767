// kernel instantiations of libflowsim_hip.so, part "forcing": boundary targets sampled and routed on the device (fs_forcing.hpp).
// These kernels are not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
//
// The whole translation unit is compiled without contraction: what it restates - np.interp, the reference's mass balance, scipy's
// brentq - rounds every product before it adds, and so do fs::interp_series and fs::brent_root here.
#pragma clang fp contract(off)
#include "fs_forcing.hpp"

namespace fs {
namespace {

template <typename R> bool sample_target(const SampleArgs<R> &a, hipStream_t st) {
  const unsigned rows = (unsigned)(a.L < 65535 ? a.L : 65535);
  hipLaunchKernelGGL((sample_target_kernel<R>), dim3((unsigned)((a.B + 255) / 256), rows), dim3(256), 0, st, a);
  return true;
}

template <typename R> bool route_pool(const PoolArgs<R> &a, hipStream_t st) {
  hipLaunchKernelGGL((route_pool_kernel<R>), dim3((unsigned)((a.B + kPoolLanes - 1) / kPoolLanes)), dim3(kPoolLanes), 0, st, a);
  return true;
}

}  // namespace

bool launch_sample_target(const SampleArgs<double> &a, hipStream_t st) { return sample_target(a, st); }
bool launch_sample_target(const SampleArgs<float> &a, hipStream_t st) { return sample_target(a, st); }
bool launch_route_pool(const PoolArgs<double> &a, hipStream_t st) { return route_pool(a, st); }
bool launch_route_pool(const PoolArgs<float> &a, hipStream_t st) { return route_pool(a, st); }

}  // namespace fs
