// fs_host_pack.hpp - what the host side of the ABI (fs_abi.hip) computes before anything goes to the device: the extended geometry
// table, the polylines in their device layout with their stage tables, the choice between tables and the edge walk, the validation
// of boundary arguments, the per-reach scheme array.  Plain C++17 with no HIP header (the FS_ST_HD marks of fs_stage_table.hpp
// apart): tests/host_pack/ builds it with the system compiler under AddressSanitizer / UBSan and holds it against a record.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/flowsim_abi.h"
#include "fs_stage_table.hpp"

namespace fs {

// rows the library appends to the caller's FS_GEO_* table on upload (extend_table): geometry-only quantities
enum { FS_GEOX_SM = FS_GEO_NPARAM, FS_GEOX_SFP, FS_GEOX_TB, FS_GEOX_AM, FS_GEOX_PM, FS_GEOX_RNM, FS_GEOX_KM15, FS_GEOX_KL15,
       FS_GEOX_KR15, FS_GEOX_NROWS };

FS_ST_HD constexpr bool bc_is_storage(int kind) { return kind == FS_BC_STORAGE || kind == FS_BC_STORAGE_CURVE; }
// the section modes of one closed form per reach, and those with a table row per node (FS_SEC_IRREGULAR: and polylines)
constexpr bool sec_is_uniform(int sec) { return sec == FS_SEC_RECT_UNIFORM || sec == FS_SEC_TRAP_UNIFORM; }
constexpr bool sec_has_tables(int sec) { return sec == FS_SEC_TABLE || sec == FS_SEC_IRREGULAR; }

// The caller's TrapezoidalSection table [FS_GEO_NPARAM][N] plus the rows of what follows from it alone
// (FS_GEOX_*: side-slope roots, bankfull geometry, reciprocal / -1.5-power roughnesses), computed here
// once in double so that no node evaluation of any Newton iteration has to.
inline std::vector<double> extend_table(const double *t, size_t N) {
  std::vector<double> x((size_t)FS_GEOX_NROWS * N, 0.0);
  std::memcpy(x.data(), t, (size_t)FS_GEO_NPARAM * N * sizeof(double));
  auto in = [&](int row, size_t i) { return t[(size_t)row * N + i]; };
  for (size_t i = 0; i < N; ++i) {
    const double b = in(FS_GEO_B_MAIN, i), m = in(FS_GEO_M_MAIN, i), hbf = in(FS_GEO_H_BANKFULL, i), mfp = in(FS_GEO_M_FP, i);
    const double sm = std::sqrt(1.0 + m * m), Tb = b + 2.0 * m * hbf;
    const double nm = in(FS_GEO_N_MAIN, i), nl = in(FS_GEO_N_LEFT, i), nr = in(FS_GEO_N_RIGHT, i);
    auto put = [&](int row, double v) { x[(size_t)row * N + i] = v; };
    put(FS_GEOX_SM, sm); put(FS_GEOX_SFP, std::sqrt(1.0 + mfp * mfp)); put(FS_GEOX_TB, Tb);
    put(FS_GEOX_AM, (b + Tb) / 2.0 * hbf); put(FS_GEOX_PM, b + 2.0 * hbf * sm);
    put(FS_GEOX_RNM, nm > 0 ? 1.0 / nm : 0.0); put(FS_GEOX_KM15, nm > 0 ? std::pow(nm, -1.5) : 0.0);
    put(FS_GEOX_KL15, nl > 0 ? std::pow(nl, -1.5) : 0.0); put(FS_GEOX_KR15, nr > 0 ? std::pow(nr, -1.5) : 0.0);
  }
  return x;
}

// polylines of one channel: validated and transposed into the vertex-major device layout ([P][N]; unused slots repeat the last
// vertex so that no lane ever reads NaN).  Returns an error text or nullptr.
inline const char *pack_polylines(const double *table, const int32_t *n_pts, int32_t max_pts, const double *x, const double *z,
                                  const double *limits, size_t N, double *xt, double *zt, double *lim, double *tz) {
  const size_t P = max_pts;
  for (size_t i = 0; i < N; ++i) {
    const int c = n_pts[i];
    if (c == 0) continue;
    if (c < 2 || c > max_pts) return "fs_batch_set_geometry_irregular: n_pts must be 0 or 2..max_pts";
    double zmin = z[i * P];
    for (int j = 0; j < c; ++j) {
      const double xv = x[i * P + j], zv = z[i * P + j];
      if (!(xv == xv) || !(zv == zv)) return "x and z must have the same shape";            // cross_section.py:222 (NaN padding inside the count)
      if (j && xv < x[i * P + j - 1]) return "fs_batch_set_geometry_irregular: x must be ascending (IrregularSection sorts it, cross_section.py:231)";
      zmin = zv < zmin ? zv : zmin;
    }
    if (table[(size_t)FS_GEO_Z_BED * N + i] != zmin)
      return "fs_batch_set_geometry_irregular: table row Z_BED must hold min(z) of a polyline node (IrregularSection.z_min)";
    for (size_t j = 0; j < P; ++j) {
      const size_t src = i * P + (j < (size_t)c ? j : (size_t)c - 1);
      xt[j * N + i] = x[src]; zt[j * N + i] = z[src];
    }
    lim[i] = limits[2 * i]; lim[N + i] = limits[2 * i + 1];
    const double node_const[5] = {table[(size_t)FS_GEO_N_LEFT * N + i], table[(size_t)FS_GEO_N_MAIN * N + i],
                                  table[(size_t)FS_GEO_N_RIGHT * N + i], table[(size_t)FS_GEO_CURVATURE * N + i], zmin};
    if (!tz) continue;                 // no stage tables for this batch (plan_irregular): the kernels walk the edges
    // the node's table, then into the device layout: breakpoints [N][KP], intervals [P][FS_PT_BLOCK / 2][N] pairs (fs_poly.hpp)
    std::vector<double> blk(poly_table_stride(max_pts));
    build_stage_table(x + i * P, z + i * P, c, limits[2 * i], limits[2 * i + 1], max_pts, blk.data(), node_const);
    pack_stage_table_node(blk.data(), max_pts, N, i, tz);
  }
  return nullptr;
}

// Stage tables: poly_table_stride(P) numbers per node (about 10 KB at 40 stations) - times N, times one set per reach for
// per-reach channels.  Beyond a bound (FS_POLY_TABLE_MAX_BYTES, default 8 GiB: staged once on the host, then resident in HBM)
// the batch gets no tables and every evaluation walks its polyline's edges (fs_poly.hpp: poly_K = 0 - same results, about five
// times the instructions); FS_POLY_WALK=1 forces that path.  fs_batch_poly_tables() says which one it is.
struct PolyTableLimits {
  bool force_walk = false;                   // FS_POLY_WALK (set to anything)
  size_t max_bytes = (size_t)8 << 30;        // FS_POLY_TABLE_MAX_BYTES
};

inline PolyTableLimits poly_limits_from_environment() {
  PolyTableLimits how;
  if (const char *env = std::getenv("FS_POLY_TABLE_MAX_BYTES")) how.max_bytes = (size_t)std::strtoull(env, nullptr, 10);
  how.force_walk = std::getenv("FS_POLY_WALK") != nullptr;
  return how;
}

// no stage tables for n_sets channels of N nodes with max_pts stations?  *table_mib: what the tables take, whole MiB
inline bool poly_tables_walk(size_t n_sets, size_t N, int32_t max_pts, const PolyTableLimits &how, size_t *table_mib) {
  const double table_bytes = (double)n_sets * (double)N * (double)poly_table_stride(max_pts) * sizeof(double);
  if (table_mib) *table_mib = (size_t)(table_bytes / (1 << 20));
  return how.force_walk || table_bytes > (double)how.max_bytes;
}

// what set_irregular uploads: n_sets channels (1: shared by the batch; B: one per reach), each packed and extended
struct IrregularPlan {
  std::vector<double> xt, zt, lim;    // [n_sets][P][N], [n_sets][P][N], [n_sets][2][N]
  std::vector<double> tabs;           // [n_sets][FS_GEOX_NROWS][N]
  std::vector<double> tz;             // [n_sets][N * poly_table_stride(P)], empty: walk
  bool walk = false;
  size_t table_mib = 0;               // what the stage tables take (the texts about not fitting say it)
};

// tables [n_sets][NPARAM][N], n_pts [n_sets][N], x / z [n_sets][N][P], limits [n_sets][N][2].  Returns an error text or "".
inline std::string plan_irregular(const double *table, const int32_t *n_pts, int32_t max_pts, const double *x, const double *z,
                                  const double *limits, size_t N, size_t n_sets, const PolyTableLimits &how, IrregularPlan &out) {
  const size_t P = max_pts, per = (size_t)FS_GEOX_NROWS * N;
  out.xt.assign(n_sets * P * N, 0.0); out.zt.assign(n_sets * P * N, 0.0); out.lim.assign(n_sets * 2 * N, 0.0);
  out.tabs.resize(n_sets * per);
  const size_t tstride = (size_t)poly_table_stride(max_pts);
  out.walk = poly_tables_walk(n_sets, N, max_pts, how, &out.table_mib);
  out.tz.clear();
  try {
    if (!out.walk) out.tz.assign(n_sets * N * tstride, std::numeric_limits<double>::infinity());
  } catch (const std::bad_alloc &) {
    return "fs_batch_set_geometry_irregular: no host memory to stage " + std::to_string(out.table_mib) +
           " MiB of stage tables (lower FS_POLY_TABLE_MAX_BYTES to fall back to the edge walk)";
  }
  for (size_t r = 0; r < n_sets; ++r) {
    const double *tab_r = table + r * FS_GEO_NPARAM * N;
    if (const char *err = pack_polylines(tab_r, n_pts + r * N, max_pts, x + r * N * P, z + r * N * P, limits + r * 2 * N, N,
                                         out.xt.data() + r * P * N, out.zt.data() + r * P * N, out.lim.data() + r * 2 * N,
                                         out.walk ? nullptr : out.tz.data() + r * N * tstride))
      return err;
    const std::vector<double> ext = extend_table(tab_r, N);
    std::memcpy(out.tabs.data() + r * per, ext.data(), per * sizeof(double));
  }
  return "";
}

// ---- boundary arguments: each check returns the error text or nullptr ----

// the area curve of an FS_BC_STORAGE_CURVE boundary (at(i): parameter row i): nc stages, strictly increasing; no curve: a surface area
template <typename At> const char *check_area_curve(At at, int nc) {
  for (int j = 0; j + 1 < nc; ++j)
    if (!(at(FS_SC_NFIXED + j + 1) > at(FS_SC_NFIXED + j))) return "fs_batch_set_bc: area-curve stages must be increasing";
  if (nc == 0 && !(at(FS_SC_SURFACE_AREA) > 0)) return "Insufficient arguments for boundary condition.";
  return nullptr;
}

// what a side's per-reach kinds come to
struct SideKinds {
  bool need_target = false;       // some reach follows a hydrograph
  bool any_storage = false;       // some reach's boundary is a storage kind
  bool some_host_rows = false;    // FS_BC_HOST_ROW among them
  // The side's representative kind (what the dispatch and fs_batch_step look at): one host-evaluated reach makes the batch one that
  // advances with fs_batch_iterate on the kernels of boundary class -1, one general reservoir makes it one for those kernels too.
  int kind = 0;
};

// fs_batch_set_bc_per_reach_wide: kinds[B], params[n_params][B]; tables: the section mode is FS_SEC_TABLE or FS_SEC_IRREGULAR
inline const char *check_bc_per_reach(int side, const int32_t *kinds, const double *params, int n_params, bool have_target, size_t B,
                                      bool tables, SideKinds &out) {
  out = SideKinds();
  for (size_t r = 0; r < B; ++r) {
    if (kinds[r] == FS_BC_STORAGE_CURVE) {   // a general reservoir behind THIS reach: its FS_SC_* rows, its own area curve of its own length
      if (!tables) return "fs_batch_set_bc_per_reach: FS_BC_STORAGE_CURVE needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR";
      if (side != FS_DOWNSTREAM) return "fs_batch_set_bc: the storage boundary is downstream only";
      auto at = [&](int i) { return params[(size_t)i * B + r]; };
      const int nc = n_params > FS_SC_N_CURVE ? (int)at(FS_SC_N_CURVE) : -1;
      if (nc < 0 || nc == 1 || FS_SC_NFIXED + 2 * nc > n_params)
        return "fs_batch_set_bc_per_reach: an FS_BC_STORAGE_CURVE reach needs FS_SC_NFIXED + 2*n_curve parameter rows (n_curve 0 or >= 2)";
      if (const char *err = check_area_curve(at, nc)) return err;
      continue;
    }
    if (kinds[r] == FS_BC_HOST_ROW) {      // a plugin without a device form on THIS reach
      if (!tables) return "fs_batch_set_bc_per_reach: FS_BC_HOST_ROW needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR";
      continue;
    }
    if (kinds[r] < 0 || kinds[r] > FS_BC_STORAGE) return "Invalid boundary condition.";        // boundary.py:33
    if (kinds[r] == FS_BC_STORAGE && side != FS_DOWNSTREAM) return "fs_batch_set_bc: the storage boundary is downstream only";
    out.need_target = out.need_target || kinds[r] == FS_BC_FLOW_HYDROGRAPH || kinds[r] == FS_BC_STAGE_HYDROGRAPH;
  }
  if (out.need_target && !have_target) return "Insufficient arguments for boundary condition.";                     // boundary.py:87
  out.kind = kinds[0];
  for (size_t r = 0; r < B; ++r) {
    out.any_storage = out.any_storage || bc_is_storage(kinds[r]);
    out.some_host_rows = out.some_host_rows || kinds[r] == FS_BC_HOST_ROW;
    if (kinds[r] == FS_BC_STORAGE_CURVE) out.kind = FS_BC_STORAGE_CURVE;
  }
  if (out.some_host_rows) out.kind = FS_BC_HOST_ROW;
  return nullptr;
}

// fs_batch_set_bc: one kind for the batch; params[n_params] or, per_reach, params[n_params][B]
inline const char *check_bc(int side, int kind, const double *params, int n_params, int per_reach, bool have_target, size_t B,
                            bool tables) {
  static const int need[] = {0, 1, 1, 2, 4, 5, 10, 5};
  if (kind < 0 || kind > FS_BC_HOST_ROW) return "Invalid boundary condition.";        // boundary.py:33
  if (kind == FS_BC_HOST_ROW) {
    if (!tables) return "fs_batch_set_bc: FS_BC_HOST_ROW needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR";
    if (n_params != 3 || !per_reach) return "fs_batch_set_bc: FS_BC_HOST_ROW takes params[3][B] (per_reach = 1) or NULL";
    return nullptr;
  }
  if (kind == FS_BC_STORAGE_CURVE) {
    // shared by the batch (params[n_params]) or one reservoir per reach (per_reach = 1: params[n_params][B], every reach its own
    // scalars, area curve and outflow rating curve; the curves of a batch have the same number of points)
    if (!params || n_params < FS_SC_NFIXED) return "Insufficient arguments for boundary condition.";
    const size_t Bn = per_reach ? B : 1;
    for (size_t r = 0; r < Bn; ++r) {
      auto at = [&](int i) { return per_reach ? params[(size_t)i * Bn + r] : params[i]; };
      const int nc = (int)at(FS_SC_N_CURVE);
      if (nc < 0 || nc == 1 || n_params != FS_SC_NFIXED + 2 * nc)
        return "fs_batch_set_bc: FS_BC_STORAGE_CURVE needs FS_SC_NFIXED + 2*n_curve parameters (n_curve 0 or >= 2; per reach: the same n_curve for all)";
      if (const char *err = check_area_curve(at, nc)) return err;
    }
  } else if (n_params != need[kind]) return "Insufficient arguments for boundary condition.";      // boundary.py:83
  if (n_params > 0 && !params) return "Insufficient arguments for boundary condition.";
  if ((kind == FS_BC_FLOW_HYDROGRAPH || kind == FS_BC_STAGE_HYDROGRAPH) && !have_target)
    return "Insufficient arguments for boundary condition.";                                // boundary.py:87
  if (bc_is_storage(kind) && side != FS_DOWNSTREAM) return "fs_batch_set_bc: the storage boundary is downstream only";
  return nullptr;
}

// the first `rows` of the scheme values (theta, dt, dx, tolerance, max_iter) as a [rows][B] array: per-reach values where the caller
// gave them (per_reach[i] not empty), the batch's elsewhere.  Unless `always`, empty where nothing is per reach.
inline std::vector<double> reach_scheme_rows(const std::vector<double> *per_reach, const double *wide, int rows, size_t B, bool always) {
  bool any = always;
  for (int i = 0; i < rows; ++i) any = any || !per_reach[i].empty();
  std::vector<double> v;
  if (!any) return v;
  v.resize(rows * B);
  for (int i = 0; i < rows; ++i)
    for (size_t r = 0; r < B; ++r) v[i * B + r] = per_reach[i].empty() ? wide[i] : per_reach[i][r];
  return v;
}

// the [5][B] array the kernels of boundary classes 0 and -1 read.  Empty: nothing is per reach.
inline std::vector<double> merge_reach_scheme(const std::vector<double> per_reach[5], const double wide[5], size_t B) {
  return reach_scheme_rows(per_reach, wide, 5, B, false);
}

}  // namespace fs
