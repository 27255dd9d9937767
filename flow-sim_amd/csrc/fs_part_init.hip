// kernel instantiations of libflowsim_hip.so, part "init": initial conditions on the device (fs_init_state.hpp).  These kernels are
// not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
#include "fs_init_state.hpp"

namespace fs {
namespace {

template <typename R, int SEC> void launch_one(const InitArgs<R> &p, hipStream_t st) {
  const size_t B = p.k.B, N = p.k.N;
  if (p.method == FS_IC_GVF)
    hipLaunchKernelGGL((init_backwater_kernel<R, SEC>), dim3((unsigned)((B + kInitLanes - 1) / kInitLanes)), dim3(kInitLanes), 0, st, p);
  else
    hipLaunchKernelGGL((init_per_node_kernel<R, SEC>), dim3((unsigned)((B * N + 255) / 256)), dim3(256), 0, st, p);
}

}  // namespace

bool launch_init_state(int section_mode, const InitArgs<double> &p, hipStream_t st) {
  switch (section_mode) {
    case FS_SEC_RECT_UNIFORM: launch_one<double, FS_SEC_RECT_UNIFORM>(p, st); return true;
    case FS_SEC_TRAP_UNIFORM: launch_one<double, FS_SEC_TRAP_UNIFORM>(p, st); return true;
    case FS_SEC_TABLE: launch_one<double, FS_SEC_TABLE>(p, st); return true;
    case FS_SEC_IRREGULAR: launch_one<double, FS_SEC_IRREGULAR>(p, st); return true;
  }
  return false;
}

bool launch_init_state(int section_mode, const InitArgs<float> &p, hipStream_t st) {
  switch (section_mode) {
    case FS_SEC_RECT_UNIFORM: launch_one<float, FS_SEC_RECT_UNIFORM>(p, st); return true;
    case FS_SEC_TRAP_UNIFORM: launch_one<float, FS_SEC_TRAP_UNIFORM>(p, st); return true;
    case FS_SEC_TABLE: launch_one<float, FS_SEC_TABLE>(p, st); return true;
  }
  return false;      // FS_SEC_IRREGULAR is fp64 only
}

}  // namespace fs
