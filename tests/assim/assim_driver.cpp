// Driver of tests/test_assim_host.py: the plain-C++ half of flow-sim_amd/csrc/fs_assim.hpp on records read from the file named on the
// command line.  Records, whitespace separated ("nan" and "inf" are numbers here):
//   K name n_obs count n_gauges B N null has_perturb has_taper depth_floor gauge[count] signal[count] value[count] variance[count]
//          perturb[count B]? taper[count N]?        check_observations (null 1: no arrays are handed)
//                                                                                    -> "K name" the text, or "ok"
//   L name B N m chunk field row j r              AssimLayout                        -> "L name" chunks rows partials partial prior
//                                                                                       prior_row(field, 1) cross cross_row(field, j)
//                                                                                       bucket columns column(r)
//   A name m B has_perturb active[B] y[m B] value[m] variance[m] perturb[m B]?
//                                                 analysis_coefficients; y is read for active members only (the driver checks that)
//                                                                                    -> "A name ok" n_active stray ybar[m] S[m B] C[m m]
//                                                                                       L[m m] Z[m B], or "A name refused" n_active text
// Numbers go out with 17 significant digits, which read back to the same doubles.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "fs_assim.hpp"

namespace {

bool number(std::ifstream &in, double &x) {
  std::string tok;
  if (!(in >> tok)) return false;
  char *end = nullptr;
  x = std::strtod(tok.c_str(), &end);
  return end != tok.c_str() && *end == '\0';
}

bool numbers(std::ifstream &in, std::vector<double> &v) {
  for (double &x : v)
    if (!number(in, x)) return false;
  return true;
}

int bad(const std::string &name) { std::fprintf(stderr, "bad record %s\n", name.c_str()); return 2; }

int check_record(std::ifstream &in, const std::string &name) {
  long n_obs = 0, count = 0, n_gauges = 0, B = 0, N = 0, null = 0, has_p = 0, has_t = 0;
  double floor = 0.0;
  in >> n_obs >> count >> n_gauges >> B >> N >> null >> has_p >> has_t;
  if (!in || count < 0 || B < 0 || N < 0 || !number(in, floor)) return bad(name);
  std::vector<double> gauge_d((size_t)count), signal_d((size_t)count), value((size_t)count), variance((size_t)count);
  std::vector<double> perturb(has_p ? (size_t)(count * B) : 0), taper(has_t ? (size_t)(count * N) : 0);
  if (!numbers(in, gauge_d) || !numbers(in, signal_d) || !numbers(in, value) || !numbers(in, variance) || !numbers(in, perturb) ||
      !numbers(in, taper))
    return bad(name);
  std::vector<int32_t> gauge, signal;
  for (double v : gauge_d) gauge.push_back((int32_t)v);
  for (double v : signal_d) signal.push_back((int32_t)v);
  const std::string text =
      fs::check_observations("entry", (int32_t)n_obs, null ? nullptr : gauge.data(), null ? nullptr : signal.data(), null ? nullptr : value.data(),
                             null ? nullptr : variance.data(), has_p ? perturb.data() : nullptr, has_t ? taper.data() : nullptr, floor,
                             (int32_t)n_gauges, (size_t)B, (size_t)N);
  std::printf("K %s %s\n", name.c_str(), text.empty() ? "ok" : text.c_str());
  return 0;
}

int layout_record(std::ifstream &in, const std::string &name) {
  size_t B = 0, N = 0, m = 0, chunk = 0, field = 0, row = 0, j = 0, r = 0;
  in >> B >> N >> m >> chunk >> field >> row >> j >> r;
  if (!in) return bad(name);
  const fs::AssimLayout lay{B, N, m};
  std::printf("L %s %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", name.c_str(), lay.chunks(), lay.rows(), lay.partials(), lay.partial(chunk, field, row),
              lay.prior(), lay.prior_row(field, 1), lay.cross(), lay.cross_row(field, j), lay.bucket(), lay.columns(), lay.column(r));
  return 0;
}

void put(const std::vector<double> &v) {
  for (double x : v) std::printf(" %.17g", x);
}

int analysis_record(std::ifstream &in, const std::string &name) {
  long m = 0, B = 0, has_p = 0;
  in >> m >> B >> has_p;
  if (!in || m < 1 || m > FS_ASSIM_MAX_OBS || B < 0) return bad(name);
  std::vector<double> active_d((size_t)B), y((size_t)(m * B)), value((size_t)m), variance((size_t)m), perturb(has_p ? (size_t)(m * B) : 0);
  if (!numbers(in, active_d) || !numbers(in, y) || !numbers(in, value) || !numbers(in, variance) || !numbers(in, perturb)) return bad(name);
  std::vector<int32_t> active;
  for (double v : active_d) active.push_back(v != 0.0);
  std::vector<double> ybar, S, C, L, Z;
  int32_t na = -1;
  int stray = 0;
  const std::string text = fs::analysis_coefficients(
      "entry", (int)m, (size_t)B, active.data(),
      [&](size_t j, size_t r) {
        if (!active.at(r)) ++stray;
        return y.at(j * (size_t)B + r);
      },
      value.data(), variance.data(), has_p ? perturb.data() : nullptr, ybar, S, C, L, Z, &na);
  if (!text.empty()) {
    std::printf("A %s refused %d %s\n", name.c_str(), na, text.c_str());
    return 0;
  }
  std::printf("A %s ok %d %d", name.c_str(), na, stray);
  put(ybar); put(S); put(C); put(L); put(Z);
  std::printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: assim_driver FILE\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string kind, name;
  while (in >> kind >> name) {
    int rc = 2;
    if (kind == "K") rc = check_record(in, name);
    else if (kind == "L") rc = layout_record(in, name);
    else if (kind == "A") rc = analysis_record(in, name);
    else std::fprintf(stderr, "unknown record %s\n", kind.c_str());
    if (rc) return rc;
  }
  return 0;
}
