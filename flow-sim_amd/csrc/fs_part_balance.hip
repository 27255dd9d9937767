// kernel instantiations of libflowsim_hip.so, part "balance": reach integrals and the discrete water balance (fs_balance.hpp).  These
// kernels are not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
#include "fs_balance.hpp"

namespace fs {
namespace {

// one wavefront per (level, reach) row, four rows per workgroup; history rows and the current state go through the same instantiation
template <typename R> bool reach_integrals(const IntegralArgs<R> &a, hipStream_t st) {
  constexpr int V = (int)(16 / sizeof(R));
  const size_t rows = (size_t)a.rows.n * a.B;
  hipLaunchKernelGGL((reach_integrals_kernel<R, V>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  return true;
}

template <typename R> bool balance(const ReduceArgs<R> &a, const BalanceArgs &p, hipStream_t st) {
  hipLaunchKernelGGL((balance_kernel<R>), dim3((unsigned)((a.B + kBalLanes - 1) / kBalLanes)), dim3(kBalLanes), 0, st, a, p);
  return true;
}

}  // namespace

bool launch_reach_integrals(const IntegralArgs<double> &a, hipStream_t st) { return reach_integrals(a, st); }
bool launch_reach_integrals(const IntegralArgs<float> &a, hipStream_t st) { return reach_integrals(a, st); }
bool launch_balance(const ReduceArgs<double> &a, const BalanceArgs &p, hipStream_t st) { return balance(a, p, st); }
bool launch_balance(const ReduceArgs<float> &a, const BalanceArgs &p, hipStream_t st) { return balance(a, p, st); }

bool launch_clear_integrals(double *integ, size_t n_integ, int32_t *mark, size_t n_mark, hipStream_t st) {
  const size_t n = n_integ > n_mark ? n_integ : n_mark;
  if (n == 0) return true;
  hipLaunchKernelGGL((clear_integrals_kernel<256>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, integ, n_integ, mark, n_mark);
  return true;
}

}  // namespace fs
