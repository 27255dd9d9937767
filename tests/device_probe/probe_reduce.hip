// probe_reduce.hip - TEST INFRASTRUCTURE ONLY: the launchers of the post-processing kernels (fs_reduce.hpp, fs_envelope.hpp) on arrays
// the caller chooses, so that tests/test_gpu_band_select.py can hand bands_kernel, profile_bands_kernel, transpose_rows_kernel,
// summarize_kernel and lookup_kernel rows that no stepped batch produces.  This source holds no kernel: libfs_probe.so links the
// library's own build/fs_part_reduce.o and build/fs_part_envelope.o next to it, so the machine code under test is the shipped one.
//
// Every wrapper takes HOST pointers, checks the sizes every index of the kernel depends on, allocates, copies in, launches,
// synchronises, copies out, frees, and returns the first HIP error (0 = hipSuccess; fsp_error_string in probe.hip).  An optional
// array is passed as NULL.
#include <stdint.h>
#include "../../flow-sim_amd/csrc/fs_envelope.hpp"
#include "probe_call.hpp"

namespace {
using namespace fs;
using fsp::Call;
using fsp::kBadArg;

// the block a batch keeps, as the caller laid it out: hydro[levels][4][B], status[B], iters[levels][B]; rows 0 .. level exist
template <typename R> struct Block {
  const R *hydro; const int32_t *status, *iters;
  int B, levels, level, first, n;
  bool valid() const { return hydro && status && iters && B >= 1 && levels >= 1 && level >= 0 && level < levels && first >= 0 && n >= 1 && first + n <= level + 1; }
  ReduceArgs<R> upload(Call &c) const {
    ReduceArgs<R> a;
    a.hydro = c.in(hydro, (size_t)levels * 4 * B); a.status = c.in(status, (size_t)B); a.iters = c.in(iters, (size_t)levels * B);
    a.B = B; a.level = level; a.first = first; a.n = n;
    return a;
  }
};

template <typename R> int bands(const Block<R> &b, const double *q, int n_q, double *moments, double *quantiles, int32_t *n_members) {
  if (!b.valid() || n_q < 0 || n_q > kBandMaxQ || (n_q > 0 && !q)) return kBadArg;
  Call c;
  const ReduceArgs<R> a = b.upload(c);
  BandArgs p;
  p.q = n_q > 0 ? c.in(q, (size_t)n_q) : nullptr; p.n_q = n_q;
  p.moments = moments ? c.out(moments, (size_t)b.n * 16) : nullptr;
  p.quantiles = quantiles && n_q > 0 ? c.out(quantiles, (size_t)b.n * 4 * n_q) : nullptr;
  p.n_members = n_members ? c.out(n_members, (size_t)b.n) : nullptr;
  if (c.ok() && !launch_bands(a, p, 0)) c.check(hipErrorNotSupported);
  return c.finish();
}

template <typename R> int summarize(const Block<R> &b, double *out) {
  if (!b.valid() || !out) return kBadArg;
  Call c;
  const ReduceArgs<R> a = b.upload(c);
  double *d = c.out(out, (size_t)FS_SUM_NROWS * b.B);
  if (c.ok() && !launch_summarize(a, d, 0)) c.check(hipErrorNotSupported);
  return c.finish();
}

template <typename R>
int lookup(const Block<R> &b, int x_row, int y_row, const double *y_offset, const double *xq, int n_q, const double *target, double *values,
           double *rmse, int32_t *info) {
  if (!b.valid() || x_row < 0 || x_row > 3 || y_row < 0 || y_row > 3 || n_q < 1 || n_q > 65535 || !xq || !values || (rmse && !target)) return kBadArg;
  Call c;
  const ReduceArgs<R> a = b.upload(c);
  LookupArgs l;
  l.x_row = x_row; l.y_row = y_row; l.n_q = n_q;
  l.y_offset = y_offset ? c.in(y_offset, (size_t)b.B) : nullptr;
  l.xq = c.in(xq, (size_t)n_q); l.target = rmse ? c.in(target, (size_t)n_q) : nullptr;
  l.values = c.out(values, (size_t)n_q * b.B);
  l.rmse = rmse ? c.out(rmse, (size_t)b.B) : nullptr; l.info = info ? c.out(info, (size_t)b.B) : nullptr;
  if (c.ok() && !launch_lookup(a, l, 0)) c.check(hipErrorNotSupported);
  return c.finish();
}

}  // namespace

extern "C" {

#define FSP_BOTH(T, S)                                                                                                                    \
  int fsp_bands_##S(const T *hydro, const int32_t *status, const int32_t *iters, int B, int levels, int level, int first, int n,          \
                    const double *q, int n_q, double *moments, double *quantiles, int32_t *n_members) {                                   \
    return bands<T>(Block<T>{hydro, status, iters, B, levels, level, first, n}, q, n_q, moments, quantiles, n_members);                   \
  }                                                                                                                                       \
  int fsp_summarize_##S(const T *hydro, const int32_t *status, const int32_t *iters, int B, int levels, int level, int first, int n,      \
                        double *out) {                                                                                                    \
    return summarize<T>(Block<T>{hydro, status, iters, B, levels, level, first, n}, out);                                                 \
  }                                                                                                                                       \
  int fsp_lookup_##S(const T *hydro, const int32_t *status, const int32_t *iters, int B, int levels, int level, int first, int n,         \
                     int x_row, int y_row, const double *y_offset, const double *xq, int n_q, const double *target, double *values,       \
                     double *rmse, int32_t *info) {                                                                                       \
    return lookup<T>(Block<T>{hydro, status, iters, B, levels, level, first, n}, x_row, y_row, y_offset, xq, n_q, target, values, rmse,   \
                     info);                                                                                                               \
  }
FSP_BOTH(double, f64)
FSP_BOTH(float, f32)
#undef FSP_BOTH

// x[N][B], count[N][B] or NULL, status[B], levels[B], reach_nodes[B] or NULL -> moments[N][4], quantiles[N][n_q], exceed[N], n_members[N]
int fsp_profile_bands(const double *x, const double *count, const int32_t *status, const int32_t *levels, const int32_t *reach_nodes, int B,
                      int N, const double *q, int n_q, double *moments, double *quantiles, double *exceed, int32_t *n_members) {
  if (!x || !status || !levels || B < 1 || N < 1 || n_q < 0 || n_q > kBandMaxQ || (n_q > 0 && !q)) return kBadArg;
  Call c;
  const size_t BN = (size_t)B * N;
  ProfileBandArgs a;
  a.x = c.in(x, BN); a.count = count ? c.in(count, BN) : nullptr;
  a.status = c.in(status, (size_t)B); a.levels = c.in(levels, (size_t)B); a.reach_nodes = reach_nodes ? c.in(reach_nodes, (size_t)B) : nullptr;
  a.B = B; a.N = N;
  a.q = n_q > 0 ? c.in(q, (size_t)n_q) : nullptr; a.n_q = n_q;
  a.moments = moments ? c.out(moments, (size_t)N * 4) : nullptr;
  a.quantiles = quantiles && n_q > 0 ? c.out(quantiles, (size_t)N * n_q) : nullptr;
  a.exceed = exceed ? c.out(exceed, (size_t)N) : nullptr;
  a.n_members = n_members ? c.out(n_members, (size_t)N) : nullptr;
  if (c.ok() && !launch_profile_bands(a, 0)) c.check(hipErrorNotSupported);
  return c.finish();
}

// row0[B][N], row1[B][N] (n_rows == 2) -> out[n_rows][N][B]
int fsp_transpose_rows(const double *row0, const double *row1, int n_rows, int B, int N, double *out) {
  if (!row0 || !out || n_rows < 1 || n_rows > 2 || (n_rows == 2 && !row1) || B < 1 || N < 1) return kBadArg;
  Call c;
  const size_t BN = (size_t)B * N;
  TransposeRows rows;
  rows.row[0] = c.in(row0, BN); rows.row[1] = n_rows == 2 ? c.in(row1, BN) : nullptr;
  double *d = c.out(out, (size_t)n_rows * BN);
  if (c.ok() && !launch_transpose_rows(rows, n_rows, d, B, N, 0)) c.check(hipErrorNotSupported);
  return c.finish();
}

}
