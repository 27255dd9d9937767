// Stand-alone driver of the plain-C++ part of flow-sim_amd/csrc/fs_forcing.hpp (tests/test_forcing_host.py builds it with the system
// compiler under AddressSanitizer and UBSan and runs it as a program).
//
// input (text, whitespace separated):
//   POOL n_curve n_w n_pts levels dt base_flow vol_scale z_lo z_hi
//        curve_stage[n_curve] curve_volume[n_curve] weirs[n_w][4] times[n_pts] values[n_pts]
//   M id scale shift initial_stage            (any number of members)
//   CHECKS                                    (the argument checks of the host side on a fixed set of bad inputs)
// output of CHECKS: K name text-or-"ok";  S id inflow[levels]   Q id release[levels]   Z id stage[levels]   E id evals[levels]   F id first level without a bracket
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "fs_forcing.hpp"

static void print_row(const char *tag, const std::string &id, const std::vector<double> &v) {
  std::printf("%s %s", tag, id.c_str());
  for (double x : v) std::printf(" %.17g", x);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: forcing_driver RECORDS\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string word;
  int n_curve = 0, n_w = 0, n_pts = 0, levels = 0;
  double dt = 0, base_flow = 0, vol_scale = 0, z_lo = 0, z_hi = 0;
  std::vector<double> cz, cv, weirs, times, values;
  auto read = [&](std::vector<double> &v, int n) { v.resize(n); for (double &x : v) in >> x; };
  while (in >> word) {
    if (word == "POOL") {
      in >> n_curve >> n_w >> n_pts >> levels >> dt >> base_flow >> vol_scale >> z_lo >> z_hi;
      if (n_curve < 2 || n_curve > fs::kPoolMaxCurve || n_w < 0 || n_w > fs::kPoolMaxWeirs || n_pts < 1 || levels < 2) return 3;
      read(cz, n_curve); read(cv, n_curve); read(weirs, 4 * n_w); read(times, n_pts); read(values, n_pts);
    } else if (word == "M") {
      std::string id;
      double scale, shift, z_init;
      in >> id >> scale >> shift >> z_init;
      if (levels < 2) return 3;
      std::vector<double> inflow(levels), release(levels), stage(levels), evals(levels, 0.0);
      for (int k = 0; k < levels; ++k) {
        const double x = (double)k * dt - shift;
        inflow[k] = scale * fs::interp_series(n_pts, [&](int j) { return times[j]; }, [&](int j) { return values[j]; }, x);
      }
      auto volume = [&](double z) { return fs::interp_series(n_curve, [&](int j) { return cz[j]; }, [&](int j) { return cv[j]; }, z); };
      auto capacity = [&](double z) {
        return fs::pool_capacity(n_w, [&](int w) { return weirs[4 * w]; }, [&](int w) { return weirs[4 * w + 1]; },
                                 [&](int w) { return weirs[4 * w + 2]; }, base_flow, z);
      };
      double z0 = z_init, qin0 = inflow[0], qout0 = fs::pool_release(qin0, capacity(z0), z0, z_init, base_flow);
      release[0] = qout0; stage[0] = z0;
      int failed = -1;
      for (int k = 1; k < levels; ++k) {
        if (failed < 0) {
          const fs::PoolLevel s = fs::pool_level(volume, capacity, z_init, base_flow, z0, qin0, qout0, inflow[k], dt, vol_scale, z_lo, z_hi);
          if (!s.bracketed) failed = k;
          evals[k] = s.evals;
          z0 = s.stage; qin0 = inflow[k]; qout0 = s.release;
        }
        release[k] = qout0; stage[k] = z0;
      }
      print_row("S", id, inflow); print_row("Q", id, release); print_row("Z", id, stage); print_row("E", id, evals);
      std::printf("F %s %d\n", id.c_str(), failed);
    } else if (word == "CHECKS") {
      auto say = [](const char *name, const char *text) { std::printf("K %s %s\n", name, text ? text : "ok"); };
      const double up[3] = {0.0, 1.0, 2.0}, down[3] = {0.0, 2.0, 1.0}, flat[3] = {0.0, 1.0, 1.0}, nan3[3] = {0.0, fs::red_nan(), 2.0};
      const int32_t idx_ok[2] = {0, 1}, idx_hi[2] = {0, 2}, idx_lo[2] = {-1, 0};
      const double vals[6] = {1, 2, 3, 4, 5, 6};
      say("tables_ok", fs::check_sampled_tables(up, vals, 3, 2, idx_ok, 2));
      say("tables_one_point", fs::check_sampled_tables(up, vals, 1, 1, nullptr, 2));
      say("tables_null", fs::check_sampled_tables(nullptr, vals, 3, 2, nullptr, 2));
      say("tables_none", fs::check_sampled_tables(up, vals, 0, 1, nullptr, 2));
      say("tables_descending", fs::check_sampled_tables(down, vals, 3, 2, nullptr, 2));
      say("tables_repeated", fs::check_sampled_tables(flat, vals, 3, 2, nullptr, 2));
      say("tables_nan", fs::check_sampled_tables(nan3, vals, 3, 2, nullptr, 2));
      say("tables_index_high", fs::check_sampled_tables(up, vals, 3, 2, idx_hi, 2));
      say("tables_index_negative", fs::check_sampled_tables(up, vals, 3, 2, idx_lo, 2));
      std::vector<double> longz(fs::kPoolMaxCurve + 1), manyw(4 * (fs::kPoolMaxWeirs + 1), 0.0);
      for (size_t j = 0; j < longz.size(); ++j) longz[j] = (double)j;
      const double w_ok[8] = {2.0, 0.5, 1.0, 0.0, 3.0, 1.5, 1.5, 0.0}, w_reserved[4] = {2.0, 0.5, 1.0, 7.0}, w_negative[4] = {-2.0, 0.5, 1.0, 0.0};
      say("pool_ok", fs::check_pool(up, vals, 3, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_full", fs::check_pool(longz.data(), longz.data(), fs::kPoolMaxCurve, manyw.data(), fs::kPoolMaxWeirs, 0.0, 1.0, 0.0, 2.0));
      say("pool_no_weirs", fs::check_pool(up, vals, 3, nullptr, 0, 1.0, 1e-6, 0.0, 2.0));
      say("pool_null_curve", fs::check_pool(up, nullptr, 3, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_curve_short", fs::check_pool(up, vals, 1, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_curve_long", fs::check_pool(longz.data(), longz.data(), fs::kPoolMaxCurve + 1, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_curve_descending", fs::check_pool(down, vals, 3, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_volume_nan", fs::check_pool(up, nan3, 3, w_ok, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_nine_weirs", fs::check_pool(up, vals, 3, manyw.data(), fs::kPoolMaxWeirs + 1, 1.0, 1e-6, 0.0, 2.0));
      say("pool_null_weirs", fs::check_pool(up, vals, 3, nullptr, 2, 1.0, 1e-6, 0.0, 2.0));
      say("pool_negative_weir", fs::check_pool(up, vals, 3, w_negative, 1, 1.0, 1e-6, 0.0, 2.0));
      say("pool_reserved", fs::check_pool(up, vals, 3, w_reserved, 1, 1.0, 1e-6, 0.0, 2.0));
      say("pool_negative_base", fs::check_pool(up, vals, 3, w_ok, 2, -1.0, 1e-6, 0.0, 2.0));
      say("pool_zero_scale", fs::check_pool(up, vals, 3, w_ok, 2, 1.0, 0.0, 0.0, 2.0));
      say("pool_bracket_equal", fs::check_pool(up, vals, 3, w_ok, 2, 1.0, 1e-6, 2.0, 2.0));
      say("pool_bracket_reversed", fs::check_pool(up, vals, 3, w_ok, 2, 1.0, 1e-6, 3.0, 2.0));
      say("pool_bracket_nan", fs::check_pool(up, vals, 3, w_ok, 2, 1.0, 1e-6, fs::red_nan(), 2.0));
    } else {
      return 4;
    }
  }
  return 0;
}
