// Driver of tests/test_gauge_host.py: the plain-C++ half of flow-sim_amd/csrc/fs_gauge.hpp on records read from the file named on the
// command line.  Records, whitespace separated ("nan" and "inf" are numbers here):
//   V name a b w                                  gauge_value                        -> "V name" value
//   C name n_gauges N count null node[count] weight[count]
//                                                 check_gauge_list (null 1: no arrays are handed)
//                                                                                    -> "C name" the text, or "ok"
//   L name G L B g level q                        GaugeLayout                        -> "L name" per_gauge block marks row mark
//   R name node w nodes                           gauge_on_reach                     -> "R name" 0 | 1
//   S name m marked[m] sim[m] obs[m]              score_series; sim is read at counted levels only (the driver checks that)
//                                                                                    -> "S name" the FS_GS_NROWS rows, then reads of sim at levels that do not count
// Numbers go out with 17 significant digits, which read back to the same doubles.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "fs_gauge.hpp"

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

int value_record(std::ifstream &in, const std::string &name) {
  double a, b, w;
  if (!number(in, a) || !number(in, b) || !number(in, w)) return bad(name);
  std::printf("V %s %.17g\n", name.c_str(), fs::gauge_value(a, b, w));
  return 0;
}

int check_record(std::ifstream &in, const std::string &name) {
  long n_gauges = 0, N = 0, count = 0, null = 0;
  in >> n_gauges >> N >> count >> null;
  if (!in || count < 0) return bad(name);
  std::vector<double> node_d((size_t)count), weight((size_t)count);
  if (!numbers(in, node_d) || !numbers(in, weight)) return bad(name);
  std::vector<int32_t> node;
  for (double v : node_d) node.push_back((int32_t)v);
  const std::string text = fs::check_gauge_list("entry", (int32_t)n_gauges, null ? nullptr : node.data(), null ? nullptr : weight.data(),
                                                (size_t)count, (int32_t)N);
  std::printf("C %s %s\n", name.c_str(), text.empty() ? "ok" : text.c_str());
  return 0;
}

int layout_record(std::ifstream &in, const std::string &name) {
  size_t G = 0, L = 0, B = 0, g = 0, level = 0, q = 0;
  in >> G >> L >> B >> g >> level >> q;
  if (!in) return bad(name);
  const fs::GaugeLayout lay{G, L, B};
  std::printf("L %s %zu %zu %zu %zu %zu\n", name.c_str(), lay.per_gauge(), lay.block(), lay.marks(), lay.row(g, level, q), lay.mark(level));
  return 0;
}

int reach_record(std::ifstream &in, const std::string &name) {
  double node, w, nodes;
  if (!number(in, node) || !number(in, w) || !number(in, nodes)) return bad(name);
  std::printf("R %s %d\n", name.c_str(), fs::gauge_on_reach((int)node, w, (int)nodes) ? 1 : 0);
  return 0;
}

int score_record(std::ifstream &in, const std::string &name) {
  int m = -1;
  in >> m;
  if (!in || m < 0) return bad(name);
  std::vector<double> marked((size_t)m), sim((size_t)m), obs((size_t)m);
  if (!numbers(in, marked) || !numbers(in, sim) || !numbers(in, obs)) return bad(name);
  double rows[FS_GS_NROWS];
  for (double &x : rows) x = -12345.0;
  int stray = 0;
  fs::score_series(m, [&](int k) { return marked.at((size_t)k) != 0.0; },
                   [&](int k) {
                     if (marked.at((size_t)k) == 0.0 || obs.at((size_t)k) != obs.at((size_t)k)) ++stray;
                     return sim.at((size_t)k);
                   },
                   [&](int k) { return obs.at((size_t)k); }, [&](int row, double v) { rows[row] = v; });
  std::printf("S %s", name.c_str());
  for (double x : rows) std::printf(" %.17g", x);
  std::printf(" %d\n", stray);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: gauge_driver FILE\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string kind, name;
  while (in >> kind >> name) {
    int rc = 2;
    if (kind == "V") rc = value_record(in, name);
    else if (kind == "C") rc = check_record(in, name);
    else if (kind == "L") rc = layout_record(in, name);
    else if (kind == "R") rc = reach_record(in, name);
    else if (kind == "S") rc = score_record(in, name);
    else std::fprintf(stderr, "unknown record %s\n", kind.c_str());
    if (rc) return rc;
  }
  return 0;
}
