// Driver of tests/test_init_state_host.py: fs::brent_root (flow-sim_amd/csrc/fs_init_state.hpp) on functions built from
// + - * sqrt only, so that this build and Python evaluate them to the same bits.  Prints "name root evals bracketed" per function.
#include <cmath>
#include <cstdio>

#include "fs_init_state.hpp"

namespace {

template <typename F> void run(const char *name, F f, double a, double b) {
  bool bracketed = false;
  int evals = 0;
  const double root = fs::brent_root(f, a, f(a), b, f(b), &bracketed, &evals);
  std::printf("%s %.17g %d %d\n", name, root, evals, bracketed ? 1 : 0);
}

}  // namespace

int main() {
  run("cubic", [](double x) { return x * x * x - 2.0 * x - 5.0; }, 2.0, 3.0);
  run("sqrt_shift", [](double x) { return std::sqrt(x) - 1.7; }, 0.0, 100.0);
  // Manning's normal flow of a rectangle 20 m wide in powers this test can write with sqrt: Q - (A^2.5 / P) sqrt(S) / n
  run("conveyance_like", [](double h) { const double A = 20.0 * h, P = 20.0 + 2.0 * h; return 120.0 - A * A * std::sqrt(A) / P * std::sqrt(2e-4) / 0.03; }, 0.0, 100.0);
  run("far_root", [](double x) { return (x - 99.999) * (x + 3.0); }, 0.0, 100.0);
  run("flat_then_steep", [](double x) { const double u = x - 1.0; return u * u * u * u * u * u * u - 1e-9; }, 0.0, 3.0);
  run("root_at_a", [](double x) { return x * (x - 5.0) - 0.0; }, 0.0, 3.0);
  run("high_datum", [](double x) { const double d = x - 480.25; return 35.0 - 9.0 * d * std::sqrt(d); }, 480.25, 580.25);
  run("no_bracket", [](double x) { return x * x + 1.0; }, -1.0, 2.0);
  return 0;
}
