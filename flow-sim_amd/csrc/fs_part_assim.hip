// kernel instantiations of libflowsim_hip.so, part "assim": the ensemble Kalman analysis of fs_batch_assimilate (fs_assim.hpp).  These
// kernels are not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
//
// Every kernel of this part rounds every product (#pragma clang fp contract(off) in the kernel, as gauge_value and score_series): the
// device is held bit for bit to a sequential restatement that cannot fuse.
#include "fs_assim.hpp"

namespace fs {
namespace {

// the moments and the update on the bucket kM of the observation count (1, 2, 4, 8, 16), the combine between them
template <typename R, int kM> void assim_launch(const AssimArgs<R> &a, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.N + kAssimThreads - 1) / kAssimThreads), chunks = (unsigned)((a.B + FS_ASSIM_CHUNK - 1) / FS_ASSIM_CHUNK);
  hipLaunchKernelGGL((assim_moments_kernel<R, kM>), dim3(tiles, chunks, 2), dim3(kAssimThreads), 0, st, a);
  hipLaunchKernelGGL((assim_combine_kernel<R>), dim3(tiles, 2), dim3(kAssimThreads), 0, st, a);
  hipLaunchKernelGGL((assim_update_kernel<R, kM>), dim3(tiles, chunks, 2), dim3(kAssimThreads), 0, st, a);
}

template <typename R> bool assimilate(const AssimArgs<R> &a, hipStream_t st) {
  switch (assim_bucket(a.m)) {
    case 1: assim_launch<R, 1>(a, st); break;
    case 2: assim_launch<R, 2>(a, st); break;
    case 4: assim_launch<R, 4>(a, st); break;
    case 8: assim_launch<R, 8>(a, st); break;
    default: assim_launch<R, 16>(a, st); break;
  }
  return true;
}

}  // namespace

bool launch_assimilate(const AssimArgs<double> &a, hipStream_t st) { return assimilate(a, st); }
bool launch_assimilate(const AssimArgs<float> &a, hipStream_t st) { return assimilate(a, st); }

}  // namespace fs
