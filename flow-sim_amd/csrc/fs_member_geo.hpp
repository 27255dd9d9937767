// fs_member_geo.hpp - geometry ensembles of ONE surveyed (polyline) channel, built on the device: every member's polylines, bed
// levels, roughnesses and stage tables from the shared channel and a per-member transform, where the per-reach setter
// (fs_batch_set_geometry_irregular_per_reach) has the host build, stage and upload one channel per member.
//
//   transform   z'_j = z_j + dz_strip(j)[r][i]: vertex j of node i is in the left strip where x_j < liml_i, in the right one where
//               x_j > limr_i, in the main channel otherwise (the strips of get_equivalent_n, cross_section.py:449-500);
//               (n_left, n_main, n_right)' = (n_left, n_main, n_right)_i * n_scale[0..2][r];  z_bed' = min_j z'_j
//               (IrregularSection.z_min, cross_section.py:231-233).  x, the limits and the curvature stay.
//   tables      what build_stage_table (fs_stage_table.hpp; cross_section.py:248-328, :449-500) writes for the member's polyline, in
//               the device layout of pack_stage_table_node, bit for bit: per interval the edges in ascending order, each term formed
//               and added to the running sums as the host builder does.  Only + - * / sqrt and comparisons occur, all correctly
//               rounded in fp64 on the device, and the translation unit is compiled without contraction.
//
// The first part - the transform of one node, the next breakpoint, one interval's coefficients, its run count - is plain C++, generic
// over how a vertex is read: tests/test_member_geometry.py compiles it with the system compiler under sanitizers and holds it to
// build_stage_table.  No sort and no private array: the distinct elevations come in ascending order from a min-above-previous scan.
// The kernels follow under __HIPCC__; they are instantiated in fs_part_geometry.hip and have no row in the dispatch table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fs_host_pack.hpp"       // FS_GEOX_*, fs_stage_table.hpp: FS_PT_*, poly_table_bp

#if defined(__HIPCC__)
#define FS_MG_HD __host__ __device__ __forceinline__
#else
#define FS_MG_HD inline
#endif

namespace fs {

constexpr double kMemberInf = __builtin_huge_val();

// the strip of a vertex at station x: 0 left, 1 main, 2 right
FS_MG_HD int member_strip(double x, double liml, double limr) { return x < liml ? 0 : (x > limr ? 2 : 1); }

// The transform of one node: its c vertices (x(j), z(j)) shifted by their strip's dz[0..2] into put(j, z') for all P slots (the
// slots beyond c repeat the transformed last vertex).  Returns z_bed' = min_j z'_j.
template <typename GetX, typename GetZ, typename Put>
FS_MG_HD double member_node(int c, int P, GetX &&x, GetZ &&z, double liml, double limr, const double dz[3], Put &&put) {
  double zmin = kMemberInf, last = 0.0;
  for (int j = 0; j < P; ++j) {
    if (j < c) {
      const int s = member_strip(x(j), liml, limr);
      last = z(j) + (s == 0 ? dz[0] : (s == 1 ? dz[1] : dz[2]));
      zmin = last < zmin ? last : zmin;
    }
    put(j, last);
  }
  return zmin;
}

// The next breakpoint: the smallest vertex elevation above prev (-inf: the lowest), +inf where there is none.  Called with its own
// result again and again it walks the distinct elevations in ascending order - std::sort + std::unique of build_stage_table.
template <typename GetZ> FS_MG_HD double member_next_level(int c, GetZ &&z, double prev) {
  double next = kMemberInf;
  for (int j = 0; j < c; ++j) {
    const double v = z(j);
    if (v > prev && v < next) next = v;
  }
  return next;
}

// The FS_PT_NCOEF coefficients of the interval above breakpoint z0k, as build_stage_table sums them (same terms, same order)
template <typename GetX, typename GetZ>
FS_MG_HD void member_interval_coefs(int c, GetX &&x, GetZ &&z, double liml, double limr, double z0k, double (&co)[FS_PT_NCOEF]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int q = 0; q < FS_PT_NCOEF; ++q) co[q] = 0.0;
  const double xa = x(0), xb = x(c - 1);
  double x0 = xa, za = z(0);
  for (int e = 0; e + 1 < c; ++e) {
    const double x1 = x(e + 1), zb = z(e + 1);
    const double dx = x1 - x0, dz = zb - za, len = __builtin_sqrt(dx * dx + dz * dz);
    const bool w0 = za <= z0k, w1 = zb <= z0k;
    if (w0 || w1) {
      double a0 = 0, a1 = 0, a2 = 0, p0 = 0, p1 = 0, t0 = 0, t1 = 0;
      if (w0 && w1) {
        a0 = dx * (z0k - 0.5 * (za + zb)); a1 = dx; p0 = len; t0 = dx;
      } else {
        const double zw = w0 ? za : zb, adz = __builtin_fabs(dz), d = z0k - zw;
        const double cA = 0.5 * dx / adz, cP = len / adz, cT = dx / adz;
        a0 = cA * d * d; a1 = 2.0 * cA * d; a2 = cA; p0 = cP * d; p1 = cP; t0 = cT * d; t1 = cT;
      }
      co[FS_PT_A0] += a0; co[FS_PT_A1] += a1; co[FS_PT_A2] += a2; co[FS_PT_P0] += p0; co[FS_PT_P1] += p1;
      co[FS_PT_T0] += t0; co[FS_PT_T1] += t1;
      if (x0 >= xa && x1 <= liml) {
        co[FS_PT_STRIP + 0] += a0; co[FS_PT_STRIP + 1] += a1; co[FS_PT_STRIP + 2] += a2; co[FS_PT_STRIP + 3] += p0; co[FS_PT_STRIP + 4] += p1;
      }
      if (x0 >= liml && x1 <= limr) {
        co[FS_PT_STRIP + 5] += a0; co[FS_PT_STRIP + 6] += a1; co[FS_PT_STRIP + 7] += a2; co[FS_PT_STRIP + 8] += p0; co[FS_PT_STRIP + 9] += p1;
      }
      if (x0 >= limr && x1 <= xb) {
        co[FS_PT_STRIP + 10] += a0; co[FS_PT_STRIP + 11] += a1; co[FS_PT_STRIP + 12] += a2; co[FS_PT_STRIP + 13] += p0; co[FS_PT_STRIP + 14] += p1;
      }
    }
    x0 = x1; za = zb;
  }
}

// The wetted runs of >= 2 vertices of the interval above z0k
template <typename GetZ> FS_MG_HD int member_run_count(int c, GetZ &&z, double z0k) {
  int runs = 0, run = 0;
  for (int v = 0; v < c; ++v) {
    const bool wet = z(v) <= z0k;
    if (wet) ++run;
    if (!wet || v == c - 1) { runs += run >= 2; run = 0; }
  }
  return runs;
}

// One interval's block of FS_PT_BLOCK doubles, pair by pair into put2(q, first, second), q < FS_PT_BLOCK / 2: the coefficients, the
// run count, the bounds [zlo, zhi) (zlo = +inf: an interval the node does not have - zeros) and the node's five constants.
template <typename GetX, typename GetZ, typename Put2>
FS_MG_HD void member_interval_block(int c, GetX &&x, GetZ &&z, double liml, double limr, double zlo, double zhi, const double (&node_const)[5],
                                    Put2 &&put2) {
  double co[FS_PT_NCOEF];
  int runs = 0;
  if (zlo < kMemberInf) {
    member_interval_coefs(c, x, z, liml, limr, zlo, co);
    runs = member_run_count(c, z, zlo);
  } else {
    for (int q = 0; q < FS_PT_NCOEF; ++q) co[q] = 0.0;
  }
  for (int q = 0; q < FS_PT_NCOEF / 2; ++q) put2(q, co[2 * q], co[2 * q + 1]);
  put2(FS_PT_NSUB / 2, (double)runs, zlo);
  put2(FS_PT_ZHI / 2, zhi, node_const[0]);
  put2(FS_PT_NM / 2, node_const[1], node_const[2]);
  put2(FS_PT_CURV / 2, node_const[3], node_const[4]);
  put2(FS_PT_USED / 2, 0.0, 0.0);
}
static_assert(FS_PT_NCOEF == 22 && FS_PT_NSUB == 22 && FS_PT_ZLO == 23 && FS_PT_ZHI == 24 && FS_PT_NL == 25 && FS_PT_NM == 26 &&
              FS_PT_NR == 27 && FS_PT_CURV == 28 && FS_PT_ZMIN == 29 && FS_PT_USED == 30 && FS_PT_BLOCK == 32 && FS_PT_STRIP == 7,
              "member_interval_block pairs the block's slots as fs_stage_table.hpp numbers them");

// One node's whole table: its breakpoints into put_bp(k, level), k < poly_table_bp(P) (+inf beyond the last one), and its P interval
// blocks, pair by pair, into put2(k, q, first, second) - build_stage_table's content in its order.  The kernel stores into the
// node-minor device layout, the CPU test into build_stage_table's own.
template <typename GetX, typename GetZ, typename PutBp, typename Put2>
FS_MG_HD void member_table_walk(int c, int P, GetX &&x, GetZ &&z, double liml, double limr, const double (&node_const)[5], PutBp &&put_bp,
                                Put2 &&put2) {
  const int KP = poly_table_bp(P);
  double lev = member_next_level(c, z, -kMemberInf);
  for (int k = 0; k < P; ++k) {
    const double next = lev < kMemberInf ? member_next_level(c, z, lev) : kMemberInf;
    put_bp(k, lev);
    member_interval_block(c, x, z, liml, limr, lev, next, node_const, [&](int q, double u, double v) { put2(k, q, u, v); });
    lev = next;
  }
  for (int k = P; k < KP; ++k) put_bp(k, kMemberInf);
}

// The transforms as the caller hands them over, dz_* [B][N] and n_scale [3][B], each of them or nullptr: the error text or nullptr, in
// plain C++ like check_bc of fs_host_pack.hpp (here and not there: tests/test_host_pack.py holds every text of that header to its
// record).  The shared channel must be polylines throughout: a trapezoid-family node's FS_GEOX_* power rows would have to be rebuilt
// per member with pow.
inline const char *check_member_transforms(const int32_t *n_pts, const double *dz_left, const double *dz_main, const double *dz_right,
                                           const double *n_scale, size_t B, size_t N) {
  for (size_t i = 0; i < N; ++i)
    if (n_pts[i] == 0)
      return "fs_batch_set_geometry_irregular_members: every node must be a polyline (n_pts > 0); trapezoid-family members go through fs_batch_set_geometry_table_per_reach";
  for (const double *dz : {dz_left, dz_main, dz_right})
    if (dz)
      for (size_t q = 0; q < B * N; ++q)
        if (!(dz[q] - dz[q] == 0.0)) return "fs_batch_set_geometry_irregular_members: dz_left, dz_main and dz_right must be finite";
  if (n_scale)
    for (size_t q = 0; q < 3 * B; ++q)
      if (!(n_scale[q] > 0.0) || !(n_scale[q] - n_scale[q] == 0.0))
        return "fs_batch_set_geometry_irregular_members: n_scale must be finite and > 0";
  return nullptr;
}

// what the two kernels read and write (fp64: FS_SEC_IRREGULAR is fp64 only)
struct MemberGeoArgs {
  const double *x0, *z0, *lim0;      // the shared channel: [P][N], [P][N], [2][N]
  const int32_t *n0;                 // [N]
  const double *tab0;                // [FS_GEOX_NROWS][N]
  const double *dz[3];               // [B][N] each or nullptr
  const double *n_scale;             // [3][B] or nullptr
  double *x, *z, *lim;               // the members': [B][P][N], [B][P][N], [B][2][N]
  int32_t *n;                        // [B][N]
  double *tab;                       // [B][FS_GEOX_NROWS][N]
  double *tz;                        // [B][N * poly_table_stride(P)] (member_tables_kernel)
  int64_t B, N;
  int32_t P;
};

#if defined(__HIPCC__)

bool launch_member_sections(const MemberGeoArgs &a, hipStream_t st);
bool launch_member_tables(const MemberGeoArgs &a, hipStream_t st);

constexpr int kMemberLanes = 64;      // one wave per block: 64 consecutive nodes of one member

// Lanes along the nodes: every read of the vertex-major polylines and every write of a member's is one contiguous 512-byte access of
// the wave.  grid: B * ceil(N / kLanes) blocks, member-major.  (Templates: the header is included by the ABI's translation unit too.)
template <int kLanes> __global__ void __launch_bounds__(kLanes) member_sections_kernel(const MemberGeoArgs a) {
  const int64_t groups = (a.N + kLanes - 1) / kLanes;
  const int64_t r = (int64_t)blockIdx.x / groups, i = ((int64_t)blockIdx.x % groups) * kLanes + threadIdx.x;
  if (r >= a.B || i >= a.N) return;
  const int64_t N = a.N;
  const int P = a.P, c = a.n0[i];
  const double liml = a.lim0[i], limr = a.lim0[N + i];
  double dz[3];
  for (int s = 0; s < 3; ++s) dz[s] = a.dz[s] ? a.dz[s][r * N + i] : 0.0;
  double *xr = a.x + r * P * N + i, *zr = a.z + r * P * N + i;
  const double zmin = member_node(c, P, [&](int j) { return a.x0[(int64_t)j * N + i]; }, [&](int j) { return a.z0[(int64_t)j * N + i]; }, liml, limr, dz,
                                  [&](int j, double v) { zr[(int64_t)j * N] = v; });
  for (int j = 0; j < P; ++j) xr[(int64_t)j * N] = a.x0[(int64_t)j * N + i];
  a.lim[r * 2 * N + i] = liml; a.lim[r * 2 * N + N + i] = limr;
  a.n[r * N + i] = c;
  double *tr = a.tab + r * FS_GEOX_NROWS * N + i;
  for (int row = 0; row < FS_GEOX_NROWS; ++row) {
    double v = a.tab0[(int64_t)row * N + i];
    if (row == FS_GEO_Z_BED) v = zmin;
    if (a.n_scale) {
      if (row == FS_GEO_N_LEFT) v = v * a.n_scale[r];
      if (row == FS_GEO_N_MAIN) v = v * a.n_scale[a.B + r];
      if (row == FS_GEO_N_RIGHT) v = v * a.n_scale[2 * a.B + r];
    }
    tr[(int64_t)row * N] = v;
  }
}

// The stage tables of the members' polylines (written by member_sections_kernel on the same stream).  One lane per node: it walks its
// breakpoints in ascending order (member_next_level: O(P) reads that hit L2) and per interval its edges; every 16-byte store into the
// node-minor table is one contiguous 1 KB access of the wave.
template <int kLanes> __global__ void __launch_bounds__(kLanes) member_tables_kernel(const MemberGeoArgs a) {
  const int64_t groups = (a.N + kLanes - 1) / kLanes;
  const int64_t r = (int64_t)blockIdx.x / groups, i = ((int64_t)blockIdx.x % groups) * kLanes + threadIdx.x;
  if (r >= a.B || i >= a.N) return;
  const int64_t N = a.N;
  const int P = a.P, c = a.n[r * N + i];
  const double *xr = a.x + r * P * N + i, *zr = a.z + r * P * N + i;
  auto x = [&](int j) { return xr[(int64_t)j * N]; };
  auto z = [&](int j) { return zr[(int64_t)j * N]; };
  const double liml = a.lim[r * 2 * N + i], limr = a.lim[r * 2 * N + N + i];
  const double *tr = a.tab + r * FS_GEOX_NROWS * N + i;
  const double node_const[5] = {tr[(int64_t)FS_GEO_N_LEFT * N], tr[(int64_t)FS_GEO_N_MAIN * N], tr[(int64_t)FS_GEO_N_RIGHT * N],
                                tr[(int64_t)FS_GEO_CURVATURE * N], tr[(int64_t)FS_GEO_Z_BED * N]};
  double *tz = a.tz + r * N * (int64_t)poly_table_stride(P);
  double *bp = tz + i * poly_table_bp(P);
  double2 *blocks = reinterpret_cast<double2 *>(tz + N * poly_table_bp(P)) + i;
  member_table_walk(c, P, x, z, liml, limr, node_const, [&](int k, double v) { bp[k] = v; },
                    [&](int k, int q, double u, double v) { blocks[((int64_t)k * (FS_PT_BLOCK / 2) + q) * N] = make_double2(u, v); });
}

#endif  // __HIPCC__

}  // namespace fs
