// Driver of tests/test_reduce_host.py: the per-series walks of flow-sim_amd/csrc/fs_reduce.hpp (summarize_series, interp_series,
// series_descends, mean_square_series) on columns read from the file named on the command line.  Records, whitespace separated:
//   S name m  h_in[m] q_in[m] h_out[m] q_out[m]     -> "S name" and the FS_SUM_NROWS numbers
//   L name m n_q  xp[m] fp[m] xq[n_q] target[n_q]   -> "L name info rmse" and the n_q values
// Numbers go out with 17 significant digits, which read back to the same doubles.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "fs_reduce.hpp"

namespace {

std::vector<double> take(std::ifstream &in, int n) {
  std::vector<double> v((size_t)n);
  for (double &x : v) in >> x;
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: reduce_driver FILE\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string kind, name;
  while (in >> kind >> name) {
    int m = 0;
    in >> m;
    if (kind == "S") {
      const std::vector<double> h_in = take(in, m), q_in = take(in, m), h_out = take(in, m), q_out = take(in, m);
      if (!in) { std::fprintf(stderr, "short record %s\n", name.c_str()); return 2; }
      double out[FS_SUM_NROWS];
      auto col = [](const std::vector<double> &v) { return [&v](int k) { return v.at((size_t)k); }; };
      fs::summarize_series(m, col(h_in), col(q_in), col(h_out), col(q_out), [&](int row, double v) { out[row] = v; });
      std::printf("S %s", name.c_str());
      for (double v : out) std::printf(" %.17g", v);
      std::printf("\n");
    } else if (kind == "L") {
      int n_q = 0;
      in >> n_q;
      const std::vector<double> xp = take(in, m), fp = take(in, m), xq = take(in, n_q), target = take(in, n_q);
      if (!in) { std::fprintf(stderr, "short record %s\n", name.c_str()); return 2; }
      auto col = [](const std::vector<double> &v) { return [&v](int k) { return v.at((size_t)k); }; };
      std::vector<double> values;
      for (double x : xq) values.push_back(fs::interp_series(m, col(xp), col(fp), x));
      const int info = fs::series_descends(m, col(xp)) ? 1 : 0;
      const double rmse = std::sqrt(fs::mean_square_series(n_q, col(values), col(target)));
      std::printf("L %s %d %.17g", name.c_str(), info, rmse);
      for (double v : values) std::printf(" %.17g", v);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown record %s\n", kind.c_str());
      return 2;
    }
  }
  return 0;
}
