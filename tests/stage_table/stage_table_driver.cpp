// Host driver of fs_stage_table.hpp for tests/test_stage_table.py: builds the stage tables of a channel with the system compiler
// (under -fsanitize=address,undefined there) and writes them out.
//
//   stage_table_driver IN OUT
//
// IN (text): "N P", then per node "c liml limr n_left n_main n_right curvature z_min" and its c stations and c elevations.
// OUT (raw doubles): N blocks of poly_table_stride(P) as build_stage_table writes them, then the same N tables packed node-minor
// by pack_stage_table_node (the device layout, N * poly_table_stride(P) doubles).
#include <cstdio>
#include <vector>

#include "fs_stage_table.hpp"

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  std::FILE *in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  long N = 0; int P = 0;
  if (std::fscanf(in, "%ld %d", &N, &P) != 2 || N < 1 || P < 2) { std::fprintf(stderr, "bad header\n"); return 2; }
  const size_t S = (size_t)fs::poly_table_stride(P);
  std::vector<double> blocks(N * S), packed(N * S, -1.0);
  for (long i = 0; i < N; ++i) {
    int c = 0;
    double liml, limr, nc[5];
    if (std::fscanf(in, "%d %lf %lf %lf %lf %lf %lf %lf", &c, &liml, &limr, &nc[0], &nc[1], &nc[2], &nc[3], &nc[4]) != 8 || c < 2 || c > P) {
      std::fprintf(stderr, "bad node %ld\n", i); return 2;
    }
    std::vector<double> x(c), z(c);             // exactly c: a read past the polyline is an ASan report
    for (int j = 0; j < c; ++j) if (std::fscanf(in, "%lf", &x[j]) != 1) return 2;
    for (int j = 0; j < c; ++j) if (std::fscanf(in, "%lf", &z[j]) != 1) return 2;
    std::vector<double> blk(S);
    fs::build_stage_table(x.data(), z.data(), c, liml, limr, P, blk.data(), nc);
    std::copy(blk.begin(), blk.end(), blocks.begin() + i * S);
    fs::pack_stage_table_node(blk.data(), P, (size_t)N, (size_t)i, packed.data());
  }
  std::fclose(in);
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const bool ok = std::fwrite(blocks.data(), sizeof(double), blocks.size(), out) == blocks.size() &&
                  std::fwrite(packed.data(), sizeof(double), packed.size(), out) == packed.size();
  return std::fclose(out) == 0 && ok ? 0 : 1;
}
