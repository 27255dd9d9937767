// fs_host_post.hpp - what the post-processing entry points of the ABI (fs_abi.hip: summarize, lookup, bands, envelope, profile bands,
// reach integrals, water balance, integral bands, gauge bands and lookups) decide before anything is launched: the checks of their ranges and quantile levels,
// the rows of an envelope, and where the outputs of a call lie in the handle's result block.  Plain C++17 with no HIP header:
// tests/host_post/ builds it with the system compiler under AddressSanitizer / UBSan.  A check returns the error text, or nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/flowsim_abi.h"
#include "fs_envelope.hpp"
#include "fs_reduce.hpp"

namespace fs {

// the range [first, first + n) must hold computed rows only: rows 0 .. level of a batch, and none before the level it was restarted at
// (not_restored: what the restart left empty there, "the hydrograph rows before it were not restored" or the history)
inline std::string check_computed_range(const char *entry, int32_t first, int32_t n, int32_t level, int32_t restart_level,
                                        const char *not_restored) {
  if (first < 0 || n < 1 || (int64_t)first + n > (int64_t)level + 1)
    return std::string(entry) + ": levels [" + std::to_string(first) + ", " + std::to_string((int64_t)first + n) + ") are not inside 0 .. " +
           std::to_string(level) + ", the levels this batch has computed";
  if (restart_level > 0 && first < restart_level)
    return std::string(entry) + ": this batch was restarted at level " + std::to_string(restart_level) + "; " + not_restored;
  return {};
}

// the quantile levels of a band call: at most kBandMaxQ, each inside [0, 1] (a NaN is not)
inline std::string check_quantile_levels(const char *entry, const double *q, int32_t n_q) {
  if (n_q < 0 || n_q > kBandMaxQ) return std::string(entry) + ": n_q must be 0 .. " + std::to_string(kBandMaxQ);
  if (n_q > 0 && !q) return std::string(entry) + ": null quantile levels";
  for (int i = 0; i < n_q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return std::string(entry) + ": quantile levels must be in [0, 1]";
  return {};
}

// what fs_batch_lookup is handed besides its range (entry, rows: fs_batch_gauge_lookup's name and what its rows 0..3 are)
inline std::string check_lookup_args(int32_t x_row, int32_t y_row, const double *xq, int32_t n_q, const double *target, bool want_rmse,
                                     const char *entry = "fs_batch_lookup", const char *rows = "h[0], Q[0], h[N-1], Q[N-1]") {
  const std::string e(entry);
  if (x_row < 0 || x_row > 3 || y_row < 0 || y_row > 3) return e + ": x_row and y_row are 0..3 (" + rows + ")";
  if (n_q < 1 || n_q > 65535) return e + ": n_q must be 1 .. 65535";
  if (!xq) return e + ": null query abscissae";
  if (want_rmse && !target) return e + ": rmse needs a target";
  return {};
}

// The [B][N] rows of an envelope: FS_ENV_NSTAT for each selected quantity, in bit order, then - with a threshold - the FS_ENV_NCROSS
// crossing rows.
struct EnvRows {
  int quantities, n_selected = 0;       // the selected FS_ENV_* bits, and how many
  int cross_row, n_rows;                // the first crossing row, where the (quantity, statistic) rows end; and where the crossing rows do
  EnvRows(int mask, bool crossings) : quantities(mask & FS_ENV_ALL) {
    for (int k = 0; k < kEnvQuantities; ++k) n_selected += (quantities >> k) & 1;
    cross_row = n_selected * FS_ENV_NSTAT;
    n_rows = cross_row + (crossings ? (int)FS_ENV_NCROSS : 0);
  }
  // the row of statistic `stat` of `quantity` (one selected FS_ENV_* bit), or of crossing row `stat` (quantity FS_ENV_CROSSING); -1: none
  int row_of(int quantity, int stat) const {
    if (quantity == FS_ENV_CROSSING) return n_rows > cross_row && stat >= 0 && stat < FS_ENV_NCROSS ? cross_row + stat : -1;
    const int k = quantity_index(quantity);
    if (k < 0 || !((quantities >> k) & 1) || stat < 0 || stat >= FS_ENV_NSTAT) return -1;
    int before = 0;
    for (int j = 0; j < k; ++j) before += (quantities >> j) & 1;
    return before * FS_ENV_NSTAT + stat;
  }
  // 0 .. kEnvQuantities - 1 for one FS_ENV_* bit (a threshold_quantity), else -1
  static int quantity_index(int quantity) {
    for (int k = 0; k < kEnvQuantities; ++k)
      if (quantity == (1 << k)) return k;
    return -1;
  }
};

// Where the outputs of a band call lie in the handle's result block, as offsets in doubles from its start: moments [series][rows][4],
// quantiles [series][rows][n_q], with `extra` one more double per series, then the members [series] as int32 - that block begins on
// the 8-byte boundary the doubles before it leave.  n_q: 0 when no quantiles are computed.
struct BandLayout {
  size_t series, n_moments, n_quantiles;           // elements of members (and of the extra row), of moments, of quantiles
  size_t moments, quantiles, extra, members;       // offsets
  size_t bytes;                                    // the whole block
};
inline BandLayout band_layout(size_t series, size_t rows, size_t n_q, bool extra) {
  BandLayout l;
  l.series = series; l.n_moments = series * rows * 4; l.n_quantiles = series * rows * n_q;
  l.moments = 0; l.quantiles = l.n_moments; l.extra = l.quantiles + l.n_quantiles; l.members = l.extra + (extra ? series : 0);
  l.bytes = l.members * sizeof(double) + series * sizeof(int32_t);
  return l;
}

// ... and of fs_batch_lookup: values [n_q][B], rmse [B], then info [B] as int32
struct LookupLayout {
  size_t n_values;
  size_t values, rmse, info;                       // offsets in doubles
  size_t bytes;
};
inline LookupLayout lookup_layout(size_t n_q, size_t B) {
  LookupLayout l;
  l.n_values = n_q * B;
  l.values = 0; l.rmse = l.n_values; l.info = l.rmse + B;
  l.bytes = l.info * sizeof(double) + B * sizeof(int32_t);
  return l;
}

}  // namespace fs
