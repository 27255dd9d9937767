// Host driver of fs_member_geo.hpp for tests/test_member_geometry.py: the core functions the geometry kernels are made of - the
// transform of one node, the next breakpoint, one interval's coefficients, its run count - built with the system compiler (under
// -fsanitize=address,undefined there), driven node by node, next to fs::build_stage_table on the polylines the test transformed itself.
//
//   member_geo_driver tables IN OUT
//     IN (text, numbers as C99 hex floats): "B N P", then per node "c liml limr n_left n_main n_right curvature", its c stations and its
//     c elevations; then per member "s_left s_main s_right" (n_scale) and per node "dz_left dz_main dz_right", the test's own
//     "n_left' n_main' n_right' z_bed'" and its c transformed elevations.
//     OUT (raw doubles) per member, per node: z' [P], z_bed', n' [3] from the header; the table [poly_table_stride(P)] the header's walk
//     gives on ITS z'; the table build_stage_table gives on the TEST's z' and constants.
//   member_geo_driver check IN
//     IN: "B N", n_pts [N], four 0/1 flags (dz_left, dz_main, dz_right, n_scale given), then the given arrays ([B][N] / [3][B]).
//     Prints what fs::check_member_transforms says ("ok" for nullptr).
#include <cstdio>
#include <cstring>
#include <vector>

#include "fs_member_geo.hpp"

namespace {

bool read(std::FILE *in, double &v) { return std::fscanf(in, "%lf", &v) == 1; }

bool read(std::FILE *in, std::vector<double> &v) {
  for (double &q : v)
    if (!read(in, q)) return false;
  return true;
}

int tables(std::FILE *in, std::FILE *out) {
  long B = 0, N = 0;
  int P = 0;
  if (std::fscanf(in, "%ld %ld %d", &B, &N, &P) != 3 || B < 1 || N < 1 || P < 2) return 2;
  struct Node { int c; double liml, limr, n[3], curv; std::vector<double> x, z; };
  std::vector<Node> nodes(N);
  for (Node &nd : nodes) {
    if (std::fscanf(in, "%d", &nd.c) != 1 || nd.c < 2 || nd.c > P) return 2;
    if (!read(in, nd.liml) || !read(in, nd.limr) || !read(in, nd.n[0]) || !read(in, nd.n[1]) || !read(in, nd.n[2]) || !read(in, nd.curv)) return 2;
    nd.x.resize(nd.c); nd.z.resize(nd.c);            // exactly c: a read past the polyline is an ASan report
    if (!read(in, nd.x) || !read(in, nd.z)) return 2;
  }
  const size_t S = (size_t)fs::poly_table_stride(P);
  for (long r = 0; r < B; ++r) {
    double ns[3];
    if (!read(in, ns[0]) || !read(in, ns[1]) || !read(in, ns[2])) return 2;
    for (const Node &nd : nodes) {
      double dz[3], want_const[5];
      std::vector<double> want_z(nd.c);
      if (!read(in, dz[0]) || !read(in, dz[1]) || !read(in, dz[2])) return 2;
      if (!read(in, want_const[0]) || !read(in, want_const[1]) || !read(in, want_const[2]) || !read(in, want_const[4]) || !read(in, want_z)) return 2;
      want_const[3] = nd.curv;
      std::vector<double> got(P + 4), zt(nd.c), mine(S, -1.0), ref(S, -1.0);
      auto x = [&](int j) { return nd.x.at(j); };
      got[P] = fs::member_node(nd.c, P, x, [&](int j) { return nd.z.at(j); }, nd.liml, nd.limr, dz, [&](int j, double v) {
        got.at(j) = v;
        if (j < nd.c) zt.at(j) = v;
      });
      for (int s = 0; s < 3; ++s) got[P + 1 + s] = nd.n[s] * ns[s];
      const double node_const[5] = {got[P + 1], got[P + 2], got[P + 3], nd.curv, got[P]};
      const size_t KP = (size_t)fs::poly_table_bp(P);
      fs::member_table_walk(nd.c, P, x, [&](int j) { return zt.at(j); }, nd.liml, nd.limr, node_const, [&](int k, double v) { mine.at(k) = v; },
                            [&](int k, int q, double u, double v) {
                              mine.at(KP + (size_t)k * fs::FS_PT_BLOCK + 2 * q) = u;
                              mine.at(KP + (size_t)k * fs::FS_PT_BLOCK + 2 * q + 1) = v;
                            });
      fs::build_stage_table(nd.x.data(), want_z.data(), nd.c, nd.liml, nd.limr, P, ref.data(), want_const);
      if (std::fwrite(got.data(), sizeof(double), got.size(), out) != got.size() || std::fwrite(mine.data(), sizeof(double), S, out) != S ||
          std::fwrite(ref.data(), sizeof(double), S, out) != S) return 1;
    }
  }
  return 0;
}

int check(std::FILE *in) {
  long B = 0, N = 0;
  if (std::fscanf(in, "%ld %ld", &B, &N) != 2 || B < 1 || N < 1) return 2;
  std::vector<int32_t> n_pts(N);
  for (int32_t &c : n_pts)
    if (std::fscanf(in, "%d", &c) != 1) return 2;
  int given[4];
  if (std::fscanf(in, "%d %d %d %d", &given[0], &given[1], &given[2], &given[3]) != 4) return 2;
  std::vector<double> arr[4];
  for (int q = 0; q < 4; ++q)
    if (given[q]) {
      arr[q].resize(q < 3 ? (size_t)B * N : (size_t)3 * B);
      if (!read(in, arr[q])) return 2;
    }
  auto opt = [&](int q) { return given[q] ? arr[q].data() : nullptr; };
  const char *err = fs::check_member_transforms(n_pts.data(), opt(0), opt(1), opt(2), opt(3), (size_t)B, (size_t)N);
  std::printf("%s\n", err ? err : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const bool tab = argc == 4 && !std::strcmp(argv[1], "tables"), chk = argc == 3 && !std::strcmp(argv[1], "check");
  if (!tab && !chk) { std::fprintf(stderr, "usage: %s tables IN OUT | check IN\n", argv[0]); return 2; }
  std::FILE *in = std::fopen(argv[2], "r");
  if (!in) { std::perror(argv[2]); return 2; }
  int rc = 0;
  if (chk) {
    rc = check(in);
  } else {
    std::FILE *out = std::fopen(argv[3], "wb");
    if (!out) { std::perror(argv[3]); std::fclose(in); return 2; }
    rc = tables(in, out);
    if (std::fclose(out) != 0 && rc == 0) rc = 1;
  }
  std::fclose(in);
  if (rc == 2) std::fprintf(stderr, "bad input\n");
  return rc;
}
