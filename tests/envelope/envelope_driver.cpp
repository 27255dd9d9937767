// Driver of tests/test_envelope_host.py: the walk over one series of flow-sim_amd/csrc/fs_envelope.hpp (envelope_series) on series read
// from the file named on the command line.  Records, whitespace separated ("nan" is a number here):
//   E name m threshold  v[m]     -> "E name" and max, max_level, min, min_level, first, last, count
// Numbers go out with 17 significant digits, which read back to the same doubles.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "fs_envelope.hpp"

namespace {

bool number(std::ifstream &in, double &x) {
  std::string tok;
  if (!(in >> tok)) return false;
  char *end = nullptr;
  x = std::strtod(tok.c_str(), &end);
  return end != tok.c_str() && *end == '\0';
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: envelope_driver FILE\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string kind, name;
  while (in >> kind >> name) {
    if (kind != "E") { std::fprintf(stderr, "unknown record %s\n", kind.c_str()); return 2; }
    int m = -1;
    double threshold = 0.0;
    in >> m;
    if (!in || m < 0 || !number(in, threshold)) { std::fprintf(stderr, "bad record %s\n", name.c_str()); return 2; }
    std::vector<double> v((size_t)m);
    for (double &x : v)
      if (!number(in, x)) { std::fprintf(stderr, "short record %s\n", name.c_str()); return 2; }
    double stat[FS_ENV_NSTAT], cross[FS_ENV_NCROSS];
    fs::envelope_series<double>(m, [&v](int k) { return v.at((size_t)k); }, threshold, [&](int row, double x) { stat[row] = x; },
                                [&](int row, double x) { cross[row] = x; });
    std::printf("E %s", name.c_str());
    for (double x : stat) std::printf(" %.17g", x);
    for (double x : cross) std::printf(" %.17g", x);
    std::printf("\n");
  }
  return 0;
}
