// Stand-alone driver of flow-sim_amd/csrc/fs_host_post.hpp for tests/test_host_post.py: reads one request per line from the file
// named on the command line and answers each with one line.  Built with the system compiler under AddressSanitizer and UBSan.
//   consts                                          -> kBandMaxQ FS_ENV_NSTAT FS_ENV_NCROSS FS_ENV_CROSSING kEnvQuantities
//   range first n level restart_level noun(0|1)     -> the text (empty: accepted)
//   quant n_q null|levels...                        -> the text
//   lookupargs x_row y_row xq(0|1) n_q target(0|1) want_rmse(0|1) -> the text
//   rows mask crossings(0|1)                        -> n_selected cross_row n_rows
//   rowof mask crossings quantity stat              -> row
//   qindex quantity                                 -> index
//   band series rows n_q extra(0|1)                 -> series n_moments n_quantiles moments quantiles extra members bytes
//   lookup n_q B                                    -> n_values values rmse info bytes
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fs_host_post.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  static const char *const kNouns[2] = {"the hydrograph rows before it were not restored", "the history before it was not restored"};
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what;
    ss >> what;
    if (what == "consts") {
      std::cout << fs::kBandMaxQ << ' ' << (int)FS_ENV_NSTAT << ' ' << (int)FS_ENV_NCROSS << ' ' << (int)FS_ENV_CROSSING << ' ' << fs::kEnvQuantities << '\n';
    } else if (what == "range") {
      long first, n, level, restart;
      int noun;
      ss >> first >> n >> level >> restart >> noun;
      std::cout << fs::check_computed_range("entry", (int32_t)first, (int32_t)n, (int32_t)level, (int32_t)restart, kNouns[noun]) << '\n';
    } else if (what == "quant") {
      int n_q;
      std::string tok;
      std::vector<double> q;               // exactly the levels handed over: a read past them is the sanitizer's to find
      bool null = false;
      ss >> n_q;
      while (ss >> tok) {
        if (tok == "null") null = true;
        else q.push_back(std::strtod(tok.c_str(), nullptr));
      }
      std::cout << fs::check_quantile_levels("entry", null ? nullptr : q.data(), n_q) << '\n';
    } else if (what == "lookupargs") {
      int x_row, y_row, xq, n_q, target, want_rmse;
      ss >> x_row >> y_row >> xq >> n_q >> target >> want_rmse;
      const double one = 1.0;
      std::cout << fs::check_lookup_args(x_row, y_row, xq ? &one : nullptr, n_q, target ? &one : nullptr, want_rmse != 0) << '\n';
    } else if (what == "rows") {
      int mask, crossings;
      ss >> mask >> crossings;
      const fs::EnvRows r(mask, crossings != 0);
      std::cout << r.n_selected << ' ' << r.cross_row << ' ' << r.n_rows << '\n';
    } else if (what == "rowof") {
      int mask, crossings, quantity, stat;
      ss >> mask >> crossings >> quantity >> stat;
      std::cout << fs::EnvRows(mask, crossings != 0).row_of(quantity, stat) << '\n';
    } else if (what == "qindex") {
      int quantity;
      ss >> quantity;
      std::cout << fs::EnvRows::quantity_index(quantity) << '\n';
    } else if (what == "band") {
      size_t series, rows, n_q;
      int extra;
      ss >> series >> rows >> n_q >> extra;
      const fs::BandLayout l = fs::band_layout(series, rows, n_q, extra != 0);
      std::cout << l.series << ' ' << l.n_moments << ' ' << l.n_quantiles << ' ' << l.moments << ' ' << l.quantiles << ' ' << l.extra << ' ' << l.members
                << ' ' << l.bytes << '\n';
    } else if (what == "lookup") {
      size_t n_q, B;
      ss >> n_q >> B;
      const fs::LookupLayout l = fs::lookup_layout(n_q, B);
      std::cout << l.n_values << ' ' << l.values << ' ' << l.rmse << ' ' << l.info << ' ' << l.bytes << '\n';
    } else {
      return 3;
    }
  }
  return 0;
}
