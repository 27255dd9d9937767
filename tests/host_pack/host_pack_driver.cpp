// host_pack_driver.cpp - the host-side packing and validation of libflowsim_hip.so (fs_host_pack.hpp) under the system compiler and
// its sanitizers (tests/test_host_pack.py):
//   host_pack_driver poly IN OUT     IN: int64 N, P, n_sets, force_walk, max_bytes; tables [n_sets][FS_GEO_NPARAM][N], x [n_sets][N][P],
//                                    z [n_sets][N][P], limits [n_sets][N][2] (float64), n_pts [n_sets][N] (int32).
//                                    OUT: xt, zt, lim, the extended tables, tz (none on the walk) of fs::plan_irregular, float64.
//                                    Prints "ok <walk> <MiB of tables>" or the error text.
//   host_pack_driver table IN OUT    IN: int64 N; table [FS_GEO_NPARAM][N].  OUT: fs::extend_table of it.
//   host_pack_driver checks IN       IN: one case per line (numbers as C hex floats where they are not integers)
//                                      wide side kind n_params per_reach has_params has_target B tables params...
//                                      per side n_params has_target B tables kinds[B] params[n_params][B]
//                                      scheme B mask wide[5] values[5][B]         (mask bit i: row i is per reach)
//                                      walk n_sets N max_pts force_walk max_bytes
//                                    Prints per case the text of fs::check_bc / fs::check_bc_per_reach or "ok" (per reach: followed by
//                                    any_storage, some_host_rows and the representative kind), or the rows of fs::merge_reach_scheme,
//                                    or what fs::poly_tables_walk says and its MiB of tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "fs_host_pack.hpp"

template <typename T> static bool read_n(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static bool write_all(const char *path, const std::vector<const std::vector<double> *> &parts) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  for (const std::vector<double> *p : parts)
    if (!p->empty() && std::fwrite(p->data(), sizeof(double), p->size(), f) != p->size()) { std::fclose(f); return false; }
  return std::fclose(f) == 0;
}

static int run_poly(const char *in, const char *out) {
  FILE *f = std::fopen(in, "rb");
  std::vector<int64_t> head;
  if (!f || !read_n(f, head, 5)) return 2;
  const size_t N = head[0], P = head[1], S = head[2];
  std::vector<double> tab, x, z, lim;
  std::vector<int32_t> cnt;
  const bool got = read_n(f, tab, S * FS_GEO_NPARAM * N) && read_n(f, x, S * N * P) && read_n(f, z, S * N * P) && read_n(f, lim, S * N * 2) &&
                   read_n(f, cnt, S * N);
  std::fclose(f);
  if (!got) return 2;
  fs::PolyTableLimits how;
  how.force_walk = head[3] != 0; how.max_bytes = (size_t)head[4];
  fs::IrregularPlan plan;
  const std::string err = fs::plan_irregular(tab.data(), cnt.data(), (int32_t)P, x.data(), z.data(), lim.data(), N, S, how, plan);
  if (!err.empty()) { std::printf("%s\n", err.c_str()); return 0; }
  std::printf("ok %d %zu\n", plan.walk ? 1 : 0, plan.table_mib);
  return write_all(out, {&plan.xt, &plan.zt, &plan.lim, &plan.tabs, &plan.tz}) ? 0 : 2;
}

static int run_table(const char *in, const char *out) {
  FILE *f = std::fopen(in, "rb");
  std::vector<int64_t> head;
  std::vector<double> tab;
  if (!f || !read_n(f, head, 1) || !read_n(f, tab, (size_t)FS_GEO_NPARAM * head[0])) return 2;
  std::fclose(f);
  const std::vector<double> ext = fs::extend_table(tab.data(), (size_t)head[0]);
  return write_all(out, {&ext}) ? 0 : 2;
}

static int run_checks(const char *in) {
  std::ifstream f(in);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string what, tok;
    ss >> what;
    std::vector<double> v;
    while (ss >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
    size_t at = 0;
    auto next = [&]() { return at < v.size() ? v[at++] : 0.0; };
    if (what == "wide") {
      const int side = (int)next(), kind = (int)next(), n_params = (int)next(), per_reach = (int)next();
      const bool has_params = next() != 0, has_target = next() != 0;
      const size_t B = (size_t)next();
      const bool tables = next() != 0;
      const std::vector<double> params(v.begin() + (long)at, v.end());
      const char *err = fs::check_bc(side, kind, has_params ? params.data() : nullptr, n_params, per_reach, has_target, B, tables);
      std::printf("%s\n", err ? err : "ok");
    } else if (what == "per") {
      const int side = (int)next(), n_params = (int)next();
      const bool has_target = next() != 0;
      const size_t B = (size_t)next();
      const bool tables = next() != 0;
      std::vector<int32_t> kinds(B);
      for (size_t r = 0; r < B; ++r) kinds[r] = (int32_t)next();
      const std::vector<double> params(v.begin() + (long)at, v.end());
      if (params.size() != (size_t)n_params * B) return 2;
      fs::SideKinds sk;
      const char *err = fs::check_bc_per_reach(side, kinds.data(), params.data(), n_params, has_target, B, tables, sk);
      if (err) std::printf("%s\n", err);
      else std::printf("ok %d %d %d\n", sk.any_storage ? 1 : 0, sk.some_host_rows ? 1 : 0, sk.kind);
    } else if (what == "scheme") {
      const size_t B = (size_t)next();
      const int mask = (int)next();
      double wide[5];
      for (double &w : wide) w = next();
      std::vector<double> rows[5];
      for (int i = 0; i < 5; ++i)
        for (size_t r = 0; r < B; ++r) {
          const double val = next();
          if (mask & (1 << i)) rows[i].push_back(val);
        }
      const std::vector<double> m = fs::merge_reach_scheme(rows, wide, B);
      if (m.empty()) std::printf("none");
      for (double val : m) std::printf("%a ", val);
      std::printf("\n");
    } else if (what == "walk") {
      const size_t n_sets = (size_t)next(), N = (size_t)next();
      const int32_t max_pts = (int32_t)next();
      fs::PolyTableLimits how;
      how.force_walk = next() != 0; how.max_bytes = (size_t)next();
      size_t mib = 0;
      const bool walk = fs::poly_tables_walk(n_sets, N, max_pts, how, &mib);
      std::printf("%d %zu\n", walk ? 1 : 0, mib);
    } else if (!what.empty()) {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "poly")) return run_poly(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "table")) return run_table(argv[2], argv[3]);
  if (argc == 3 && !std::strcmp(argv[1], "checks")) return run_checks(argv[2]);
  std::fprintf(stderr, "usage: %s poly IN OUT | table IN OUT | checks IN\n", argv[0]);
  return 1;
}
