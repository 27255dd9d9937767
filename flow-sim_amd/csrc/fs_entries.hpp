// fs_entries.hpp - what a row of the instantiation lists (fs_entry_list.hpp) becomes under hipcc: the launcher, and the three macros
// that take a row X(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL) - FS_INSTANTIATE (the fs_part_*.hip translation units: compiled in
// parallel by the Makefile, one translation unit with all ~130 kernels takes 2.5 minutes), FS_DECLARE (fs_abi.hip: extern) and
// FS_TABLE_ROW (fs_abi.hip: the dispatch table).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include "fs_entry_list.hpp"
#include "fs_dispatch.hpp"
#include "fs_kernel.hpp"
#include "fs_derive.hpp"

typedef void (*FsLaunchFn)(const void *args, int B, hipStream_t st);

// the kernel of a row, by its kind, with every template argument written out (what FS_INSTANTIATE / FS_DECLARE name; fs_launch launches the same)
#define FS_KERNEL_STEP(R, SEC, M, W, FULL, BCK, DIAG, TAIL) fs::preissmann_step_kernel<R, SEC, M, W, !(FULL), (int)(BCK), (DIAG) != 0, TAIL, false>
#define FS_KERNEL_TEAM(R, SEC, M, W, FULL, BCK, DIAG, TAIL) fs::preissmann_step_kernel<R, SEC, M, W, !(FULL), (int)(BCK), (DIAG) != 0, TAIL, true>
#define FS_KERNEL_LONG(R, SEC, M, W, FULL, BCK, DIAG, TAIL) fs::preissmann_long_kernel<R, SEC, M, W, (int)(BCK)>

// one workgroup of W waves per reach (a team: team_size of them)
template <int KIND, typename R, int SEC, int M, int W, bool RAGGED, int BCK, bool DIAG, int TAIL>
void fs_launch(const void *args, int B, hipStream_t st) {
  const fs::KernelArgs<R> &a = *static_cast<const fs::KernelArgs<R> *>(args);
  if constexpr (KIND == FS_KIND_LONG) {
    hipLaunchKernelGGL((fs::preissmann_long_kernel<R, SEC, M, W, BCK>), dim3(B), dim3(64 * W), 0, st, a);
  } else if constexpr (KIND == FS_KIND_TEAM) {
    // FS_TEAM_TEST_DROP=1 (tests only): one workgroup too few, so that the last reach's team waits for a member that never comes - the bounded
    // wait of the exchange must then end that reach with FS_TEAM_STALL and leave the others alone (tests/test_gpu_ragged_batches.py)
    const int grid = B * a.team_size - (std::getenv("FS_TEAM_TEST_DROP") ? 1 : 0);
    hipLaunchKernelGGL((fs::preissmann_step_kernel<R, SEC, M, W, RAGGED, BCK, DIAG, TAIL, true>), dim3(grid), dim3(64 * W), 0, st, a);
  } else {
    hipLaunchKernelGGL((fs::preissmann_step_kernel<R, SEC, M, W, RAGGED, BCK, DIAG, TAIL, false>), dim3(B), dim3(64 * W), 0, st, a);
  }
}
#define FS_LAUNCHER(KIND, R, SEC, M, W, FULL, BCK, DIAG, TAIL) fs_launch<FS_KIND_##KIND, R, SEC, M, W, !(FULL), (int)(BCK), (DIAG) != 0, TAIL>

// explicit instantiation (fs_part_*.hip) / extern declaration (fs_abi.hip) / dispatch-table row (fs_abi.hip: Entry) of one list row
#define FS_INSTANTIATE(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL)                                       \
  template __global__ void FS_KERNEL_##KIND(R, SEC, M, W, FULL, BCK, DIAG, TAIL)(const fs::KernelArgs<R>); \
  template void FS_LAUNCHER(KIND, R, SEC, M, W, FULL, BCK, DIAG, TAIL)(const void *, int, hipStream_t);
#define FS_DECLARE(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL)                                                  \
  extern template __global__ void FS_KERNEL_##KIND(R, SEC, M, W, FULL, BCK, DIAG, TAIL)(const fs::KernelArgs<R>); \
  extern template void FS_LAUNCHER(KIND, R, SEC, M, W, FULL, BCK, DIAG, TAIL)(const void *, int, hipStream_t);
#define FS_TABLE_ROW(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL)                                                         \
  { FS_KEY(KIND, R, DT, SEC, M, W, FULL, BCK, DIAG, TAIL), &FS_LAUNCHER(KIND, R, SEC, M, W, FULL, BCK, DIAG, TAIL),          \
    (const void *)&FS_KERNEL_##KIND(R, SEC, M, W, FULL, BCK, DIAG, TAIL) },
