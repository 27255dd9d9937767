// fs_stage_table.hpp - the stage table of a polyline node: its layout (FS_PT_*, poly_table_bp / poly_table_stride, read by
// fs_poly.hpp on the device) and its construction on the host (build_stage_table, pack_stage_table_node, called by
// fs_host_pack.hpp: pack_polylines).  Plain C++ apart from the __host__ __device__ marks under hipcc: tests/stage_table/ builds the
// builder with the system compiler under AddressSanitizer / UBSan and checks every coefficient against the CPU oracle.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#ifdef __HIPCC__
#define FS_ST_HD __host__ __device__
#else
#define FS_ST_HD
#endif

namespace fs {

// Stage table.  Between two consecutive vertex elevations the set of wet vertices is fixed, and what properties() /
// get_equivalent_n() sum edge by edge (cross_section.py:248-328, :449-500) are low-order polynomials of the stage:
//   an edge wet at both ends adds   dx (s - zmid)            to A,  its length to P,  dx to T;
//   a water's-edge edge adds        (dx / 2|dz|) (s - zw)^2  to A,  (len / |dz|) (s - zw) to P,  (dx / |dz|) (s - zw) to T
// (zw: elevation of its wet end).  Expanded in u = s - tz[k] >= 0 every coefficient is a sum of non-negative terms - no
// cancellation, so the 1e-6 finite differences of dR_dA / dA_dh (:523-538) survive.  Per interval: whole section A (3), P (2),
// T (2), then A (3) and P (2) of the left, main and right roughness strips (an edge belongs to a strip by its two stations, :459).
// An interval's block then carries what an evaluation inside it needs and nothing else has to be fetched: its own bounds (the
// next evaluation of the node starts from the interval of the last one, node_terms_poly_hinted), the node's three Manning
// values, its curvature and z_min.  32 doubles = two 128-byte lines, fetched with sixteen 16-byte loads off one address.
enum { FS_PT_A0 = 0, FS_PT_A1, FS_PT_A2, FS_PT_P0, FS_PT_P1, FS_PT_T0, FS_PT_T1, FS_PT_STRIP = 7, FS_PT_NCOEF = 22, FS_PT_NSUB = 22,
       FS_PT_ZLO = 23, FS_PT_ZHI = 24, FS_PT_NL = 25, FS_PT_NM = 26, FS_PT_NR = 27, FS_PT_CURV = 28, FS_PT_ZMIN = 29, FS_PT_USED = 30,
       FS_PT_BLOCK = 32 };
// doubles of one node's stage table for polylines of up to P vertices
// (the breakpoints padded with +inf to a multiple of 16: the scan fetches them 16 at a time, eight 16-byte loads in flight)
FS_ST_HD constexpr int poly_table_bp(int P) { return (P + 16) & ~15; }
FS_ST_HD constexpr int poly_table_stride(int P) { return poly_table_bp(P) + P * FS_PT_BLOCK; }   // per node, both parts

// Stage table of one polyline of c vertices (xs ascending): breakpoints = the distinct vertex elevations; for each interval between
// two of them the polynomial coefficients of A, P, T and of the three roughness strips' (A, P) in u = stage - lower breakpoint, and
// the number of wetted runs of >= 2 vertices.  Written to blk[poly_table_stride(P)] as [KP] breakpoints + [P][FS_PT_BLOCK] (each
// interval's entry also carries its bounds and the node's constants).
inline void build_stage_table(const double *xs, const double *zs, int c, double liml, double limr, int P, double *blk,
                              const double node_const[5] /* n_left, n_main, n_right, curvature, z_min */) {
  std::vector<double> lev(zs, zs + c);
  std::sort(lev.begin(), lev.end());
  lev.erase(std::unique(lev.begin(), lev.end()), lev.end());
  const int K = (int)lev.size(), KP = poly_table_bp(P);
  const double inf = std::numeric_limits<double>::infinity();
  for (int j = 0; j < KP; ++j) blk[j] = j < K ? lev[j] : inf;
  const double xa = xs[0], xb = xs[c - 1];
  for (int k = 0; k < P; ++k) {
    double *co = blk + KP + (size_t)k * FS_PT_BLOCK;
    for (int q = 0; q < FS_PT_BLOCK; ++q) co[q] = 0.0;
    int runs = 0;
    if (k < K) {
      const double z0k = lev[k];
      auto wet = [&](int v) { return zs[v] <= z0k; };          // wet for every stage of the open interval above lev[k]
      for (int e = 0; e + 1 < c; ++e) {
        const double x0 = xs[e], x1 = xs[e + 1], za = zs[e], zb = zs[e + 1];
        const double dx = x1 - x0, dz = zb - za, len = std::sqrt(dx * dx + dz * dz);
        const bool w0 = wet(e), w1 = wet(e + 1);
        double a0 = 0, a1 = 0, a2 = 0, p0 = 0, p1 = 0, t0 = 0, t1 = 0;
        if (w0 && w1) {                                        // A = dx (s - zmid) = dx (z0k - zmid) + dx u
          a0 = dx * (z0k - 0.5 * (za + zb)); a1 = dx; p0 = len; t0 = dx;
        } else if (w0 != w1) {                                 // water's edge: (dx / 2|dz|) (s - zw)^2, (len / |dz|) (s - zw), (dx / |dz|) (s - zw)
          const double zw = w0 ? za : zb, adz = std::fabs(dz), d = z0k - zw;
          const double cA = 0.5 * dx / adz, cP = len / adz, cT = dx / adz;
          a0 = cA * d * d; a1 = 2.0 * cA * d; a2 = cA; p0 = cP * d; p1 = cP; t0 = cT * d; t1 = cT;
        } else {
          continue;
        }
        co[FS_PT_A0] += a0; co[FS_PT_A1] += a1; co[FS_PT_A2] += a2; co[FS_PT_P0] += p0; co[FS_PT_P1] += p1;
        co[FS_PT_T0] += t0; co[FS_PT_T1] += t1;
        const bool in[3] = {x0 >= xa && x1 <= liml, x0 >= liml && x1 <= limr, x0 >= limr && x1 <= xb};      // cross_section.py:459
        for (int sidx = 0; sidx < 3; ++sidx)
          if (in[sidx]) {
            double *o = co + FS_PT_STRIP + 5 * sidx;
            o[0] += a0; o[1] += a1; o[2] += a2; o[3] += p0; o[4] += p1;
          }
      }
      int run = 0;
      for (int v = 0; v < c; ++v) {
        if (wet(v)) ++run;
        if (!wet(v) || v == c - 1) { runs += run >= 2; run = 0; }
      }
    }
    co[FS_PT_NSUB] = (double)runs;
    // what an evaluation that starts from this interval needs besides the coefficients (fs_poly.hpp: node_terms_poly_hinted)
    co[FS_PT_ZLO] = k < K ? lev[k] : inf; co[FS_PT_ZHI] = k + 1 < K ? lev[k + 1] : inf;
    for (int q = 0; q < 5; ++q) co[FS_PT_NL + q] = node_const[q];
  }
}

// Node i's table blk (build_stage_table) into the device layout of a channel of N nodes: breakpoints [N][KP], intervals
// [P][FS_PT_BLOCK / 2][N] 16-byte pairs (NODE-MINOR, fs_poly.hpp: PolyNode).  tz holds N * poly_table_stride(P) doubles.
inline void pack_stage_table_node(const double *blk, int P, size_t N, size_t i, double *tz) {
  const size_t KP = poly_table_bp(P);
  std::memcpy(tz + i * KP, blk, KP * sizeof(double));
  double *co = tz + N * KP;
  for (size_t q = 0; q < (size_t)P * FS_PT_BLOCK; q += 2) {
    co[((q / 2) * N + i) * 2] = blk[KP + q]; co[((q / 2) * N + i) * 2 + 1] = blk[KP + q + 1];
  }
}

}  // namespace fs
