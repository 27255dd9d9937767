// kernel instantiations of libflowsim_hip.so, part "envelope": flood envelopes of a stored history and their bands across the members
// (fs_envelope.hpp).  These kernels are not step kernels: they have no row in fs_entry_list.hpp and no entry in the dispatch table.
#include "fs_envelope.hpp"

namespace fs {
namespace {

// one thread per 16 bytes of (reach, node) elements, `unroll` levels' loads in flight: 1, 4 or - the plain quantities only - 8
template <typename R, int U, int kNeed> void envelope_launch(const EnvelopeArgs<R> &a, hipStream_t st) {
  constexpr int V = (int)(16 / sizeof(R));
  const size_t BN = (size_t)a.B * a.N, threads = (BN + V - 1) / V;
  hipLaunchKernelGGL((envelope_kernel<R, V, U, kNeed>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
}

template <typename R> bool envelope(const EnvelopeArgs<R> &a, int unroll, hipStream_t st) {
  const int need = a.quantities | (a.cross_q >= 0 ? 1 << a.cross_q : 0);
  if (unroll <= 0) unroll = 4;               // the library's choice (tools/time_envelope.py, profiles/round11/envelope_timing.json)
  if ((need & ~kEnvPlain) == 0) {
    if (unroll <= 1) envelope_launch<R, 1, kEnvPlain>(a, st);
    else if (unroll < 8) envelope_launch<R, 4, kEnvPlain>(a, st);
    else envelope_launch<R, 8, kEnvPlain>(a, st);
  } else {
    if (unroll <= 1) envelope_launch<R, 1, FS_ENV_ALL>(a, st);
    else envelope_launch<R, 4, FS_ENV_ALL>(a, st);
  }
  return true;
}

}  // namespace

bool launch_envelope(const EnvelopeArgs<double> &a, int unroll, hipStream_t st) { return envelope(a, unroll, st); }
bool launch_envelope(const EnvelopeArgs<float> &a, int unroll, hipStream_t st) { return envelope(a, unroll, st); }

bool launch_transpose_rows(const TransposeRows &rows, int n_rows, double *out, int B, int N, hipStream_t st) {
  const dim3 grid((unsigned)((N + kTransposeTile - 1) / kTransposeTile), (unsigned)((B + kTransposeTile - 1) / kTransposeTile), (unsigned)n_rows);
  hipLaunchKernelGGL((transpose_rows_kernel<kTransposeTile>), grid, dim3(kTransposeTile, 8), 0, st, rows, out, B, N);
  return true;
}

bool launch_profile_bands(const ProfileBandArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((profile_bands_kernel<kBandThreads>), dim3((unsigned)a.N), dim3(kBandThreads), 0, st, a);
  return true;
}

}  // namespace fs
